// Mini-batch assembly from a packed, device-resident dataset (fastegnn_amd/data.py: PackedDataset / PackedLoader): what
// data.collate does with B slices, eight torch.cat calls and two host-to-device copies, as TWO launches whose count does not
// depend on B.
//   plan    one workgroup: the batch's exclusive node and edge offsets [B+1] from the B frame ids and the packed tables' offsets
//   gather  one launch over every output table: each table is a run of contiguous per-frame segments, so the batch is a
//           segmented copy -- flat output element -> frame (bounded binary search in the batch offsets) -> source address.
// Segment starts are not 16-byte aligned (rows are 3, 2 or 1 floats wide), so every access is one element per lane (4 bytes for
// the float tables, 8 for edge_index and batch): consecutive lanes read and write consecutive addresses inside a segment.  64-bit
// indices, no atomics, nothing read outside [src_ptr[id], src_ptr[id+1]) of a frame: ids are clamped to [0, n_frames) in the
// kernels and an element whose offset does not fall inside its frame's source segment is skipped.
//   graph   (optional, two more launches) the batch's SORTED index -- what fastegnn_build_csr would make of the batch's edge_index --
//           from the frames' own sorted indices, kept in the packed dataset: the same segmented walk with an offset added to every
//           integer, then csr.hip's chunk kernel on the assembled rowptr.  No sort, no atomics, no workspace.
// Equal-sized frames (data.py: PackedStream) need neither offsets nor a search, and their order is drawn here:
//   draw            one workgroup: the next batch's frame numbers from {seed, epoch, cursor} in device memory (keyed_perm.h)
//   gather_uniform  one launch over every output table AND the graph arrays: slot = element / segment length, 16- or 8-byte
//                   accesses wherever a frame's segment and the two base addresses allow them; then the chunk kernel.
#include "kernels.h"
#include "keyed_perm.h"

namespace fe {

constexpr int CL_PLAN_THREADS = 1024;
constexpr int CL_THREADS = 256;
constexpr int CL_UNROLL = 8;                        // elements per thread and tile: that many loads in flight before the stores
constexpr int CL_TILE = CL_THREADS * CL_UNROLL;
constexpr int CL_MAX_JOBS = FASTEGNN_COLLATE_TABLES + 2;   // the float tables, the two rows of edge_index, batch
constexpr int CL_MAX_BLOCKS = 2048;                 // beyond that the workgroups stride over the tiles

enum { CL_NODE = 0, CL_EDGE = 1, CL_FRAME = 2 };    // what a table's rows are counted in
enum { CL_COPY32 = 0, CL_INDEX64 = 1, CL_BATCH64 = 2 };

struct ClJob {
  const void *src;
  void *dst;
  long long n;         // output elements
  long long tile0;     // first tile of the job
  long long src_rows;  // rows of the source table (nothing is read at or beyond it)
  int width, kind, op;
};
struct ClJobs {
  ClJob job[CL_MAX_JOBS];
  long long n_tiles;
  int n_jobs;
};
struct ClPtrs {
  const int64_t *ids;
  const int64_t *src[2];   // the packed tables' node / edge offsets [n_frames + 1]
  const int64_t *out[2];   // the batch's node / edge offsets [B + 1]
  int B, n_frames;
};

__device__ __forceinline__ long long clamp_id(long long id, int n_frames) {
  return id < 0 ? 0 : (id >= n_frames ? (long long)n_frames - 1 : id);
}

// ---- plan: exclusive scans of the frames' node and edge counts, 1024 frames per round with a running carry ----
__global__ __launch_bounds__(CL_PLAN_THREADS) void collate_plan_kernel(const int64_t *__restrict__ ids, int B,
                                                                        const int64_t *__restrict__ src_node_ptr,
                                                                        const int64_t *__restrict__ src_edge_ptr, int n_frames,
                                                                        int64_t *__restrict__ node_ptr_out,
                                                                        int64_t *__restrict__ edge_ptr_out) {
  __shared__ long long wsum[2][CL_PLAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  long long carry[2] = {0, 0};   // the same in every thread
  for (int base = 0; base < B; base += CL_PLAN_THREADS) {
    const int i = base + t;
    long long c[2] = {0, 0};
    if (i < B) {
      const long long id = clamp_id(ids[i], n_frames);
      c[0] = src_node_ptr[id + 1] - src_node_ptr[id];
      c[1] = src_edge_ptr[id + 1] - src_edge_ptr[id];
      c[0] = c[0] < 0 ? 0 : c[0];
      c[1] = c[1] < 0 ? 0 : c[1];
    }
    long long s[2] = {c[0], c[1]};   // inclusive scan inside the wave
    for (int off = 1; off < 64; off <<= 1)
      for (int k = 0; k < 2; ++k) {
        const long long v = __shfl_up(s[k], off);
        if (lane >= off) s[k] += v;
      }
    if (lane == 63) {
      wsum[0][wave] = s[0];
      wsum[1][wave] = s[1];
    }
    __syncthreads();
    long long before[2] = {0, 0}, total[2] = {0, 0};
    for (int w = 0; w < CL_PLAN_THREADS / 64; ++w)
      for (int k = 0; k < 2; ++k) {
        const long long v = wsum[k][w];
        if (w < wave) before[k] += v;
        total[k] += v;
      }
    if (i < B) {
      node_ptr_out[i] = carry[0] + before[0] + s[0] - c[0];
      edge_ptr_out[i] = carry[1] + before[1] + s[1] - c[1];
    }
    carry[0] += total[0];
    carry[1] += total[1];
    __syncthreads();   // wsum is rewritten by the next round
  }
  if (t == 0) {
    node_ptr_out[B] = carry[0];
    edge_ptr_out[B] = carry[1];
  }
}

// ---- gather ----
// largest f in [lo, hi] with ptr[f] * w <= e (ptr[lo] * w <= e is the caller's; a frame without rows shares its offset with the
// next one, which this rule skips)
__device__ __forceinline__ int find_frame(const int64_t *__restrict__ ptr, int lo, int hi, long long e, long long w) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ptr[mid] * w <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct ClSeg {   // frame f of the batch in one table: its first output element and its source segment, in elements
  long long out0, src0, len, node0;
};
__device__ __forceinline__ ClSeg load_seg(const ClPtrs &P, int kind, int f, long long w) {
  const long long id = clamp_id(P.ids[f], P.n_frames);
  const long long s0 = P.src[kind][id], s1 = P.src[kind][id + 1];
  ClSeg g;
  g.out0 = P.out[kind][f] * w;
  g.src0 = s0 * w;
  g.len = (s1 - s0) * w;
  g.node0 = P.out[CL_NODE][f];
  return g;
}

// One tile of one table.  UNIFORM: the whole tile lies in frame flo (its segment data is the same for every lane and is loaded
// once); otherwise every element finds its frame in [flo, fhi].
template <int OP, bool UNIFORM>
__device__ __forceinline__ void gather_tile(const ClJob &jb, const ClPtrs &P, long long e0, long long e1, int flo, int fhi) {
  const long long w = jb.width, src_end = jb.src_rows * w;
  long long src_at[CL_UNROLL], add[CL_UNROLL];
  ClSeg g0 = {};
  if (UNIFORM) g0 = load_seg(P, jb.kind, flo, w);
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) {
    const long long e = e0 + u * CL_THREADS + threadIdx.x;
    src_at[u] = -1;
    add[u] = 0;
    if (e < e1) {
      int f = flo;
      ClSeg g = g0;
      if (!UNIFORM) {
        f = find_frame(P.out[jb.kind], flo, fhi, e, w);
        g = load_seg(P, jb.kind, f, w);
      }
      const long long local = e - g.out0;
      if (local >= 0 && local < g.len && g.src0 >= 0 && g.src0 + local < src_end) {
        src_at[u] = g.src0 + local;
        add[u] = OP == CL_BATCH64 ? (long long)f : g.node0;
      }
    }
  }
  if (OP == CL_COPY32) {
    const unsigned *__restrict__ src = (const unsigned *)jb.src;
    unsigned *__restrict__ dst = (unsigned *)jb.dst;
    unsigned v[CL_UNROLL];
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u) v[u] = src_at[u] >= 0 ? src[src_at[u]] : 0u;
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u)
      if (src_at[u] >= 0) dst[e0 + u * CL_THREADS + threadIdx.x] = v[u];
  } else if (OP == CL_INDEX64) {
    const long long *__restrict__ src = (const long long *)jb.src;
    long long *__restrict__ dst = (long long *)jb.dst;
    long long v[CL_UNROLL];
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u) v[u] = src_at[u] >= 0 ? src[src_at[u]] : 0;
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u)
      if (src_at[u] >= 0) dst[e0 + u * CL_THREADS + threadIdx.x] = v[u] + add[u];
  } else {
    long long *__restrict__ dst = (long long *)jb.dst;
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u)
      if (src_at[u] >= 0) dst[e0 + u * CL_THREADS + threadIdx.x] = add[u];
  }
}

// loc_mean: one row of `width` floats per frame on both sides, so the frame is a division
__device__ __forceinline__ void gather_tile_frames(const ClJob &jb, const ClPtrs &P, long long e0, long long e1) {
  const long long w = jb.width;
  const float *__restrict__ src = (const float *)jb.src;
  float *__restrict__ dst = (float *)jb.dst;
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) {
    const long long e = e0 + u * CL_THREADS + threadIdx.x;
    if (e < e1) {
      const long long f = e / w;
      const long long id = clamp_id(P.ids[f], P.n_frames);
      if (id < jb.src_rows) dst[e] = src[id * w + (e - f * w)];
    }
  }
}

__global__ __launch_bounds__(CL_THREADS) void collate_gather_kernel(const ClJobs J, const ClPtrs P) {
  for (long long tile = blockIdx.x; tile < J.n_tiles; tile += gridDim.x) {
    int j = 0;
    for (int k = 1; k < J.n_jobs; ++k)
      if (tile >= J.job[k].tile0) j = k;
    const ClJob &jb = J.job[j];
    const long long e0 = (tile - jb.tile0) * CL_TILE;
    const long long e1 = e0 + CL_TILE < jb.n ? e0 + CL_TILE : jb.n;
    if (jb.kind == CL_FRAME) {
      gather_tile_frames(jb, P, e0, e1);
      continue;
    }
    const int64_t *__restrict__ po = P.out[jb.kind];
    const int flo = find_frame(po, 0, P.B - 1, e0, jb.width);
    const int fhi = find_frame(po, flo, P.B - 1, e1 - 1, jb.width);
    if (flo == fhi) {
      if (jb.op == CL_COPY32) gather_tile<CL_COPY32, true>(jb, P, e0, e1, flo, fhi);
      else if (jb.op == CL_INDEX64) gather_tile<CL_INDEX64, true>(jb, P, e0, e1, flo, fhi);
      else gather_tile<CL_BATCH64, true>(jb, P, e0, e1, flo, fhi);
    } else {
      if (jb.op == CL_COPY32) gather_tile<CL_COPY32, false>(jb, P, e0, e1, flo, fhi);
      else if (jb.op == CL_INDEX64) gather_tile<CL_INDEX64, false>(jb, P, e0, e1, flo, fhi);
      else gather_tile<CL_BATCH64, false>(jb, P, e0, e1, flo, fhi);
    }
  }
}

// ---- graph: the batch's sorted index from the frames' own (fastegnn_collate_graph) ----
// The same segmented walk over int32 outputs.  CG_PTR: rowptr / cscptr, int64 positions in the packed edge table -> positions in the
// batch's (minus the frame's first packed edge, plus its first edge in the batch); the job is one element longer than the batch has
// nodes, and that last element is the edge total.  CG_NODE_ID: erow / col, frame-local node ids + the frame's first node.
// CG_EDGE_ID: perm / csc_eid, frame-local edge positions + the frame's first edge.  CG_ZERO: rowptr / cscptr of a batch without edges.
enum { CG_PTR = 3, CG_NODE_ID = 4, CG_EDGE_ID = 5, CG_ZERO = 6 };

template <int OP>
__device__ __forceinline__ long long graph_add(const ClPtrs &P, int f, const ClSeg &g) {
  if (OP == CG_NODE_ID) return g.node0;
  const long long eo = P.out[CL_EDGE][f];
  return OP == CG_EDGE_ID ? eo : eo - P.src[CL_EDGE][clamp_id(P.ids[f], P.n_frames)];
}

template <int OP, bool UNIFORM>
__device__ __forceinline__ void graph_tile(const ClJob &jb, const ClPtrs &P, long long e0, long long e1, int flo, int fhi,
                                           long long n_edges_out) {
  const long long n_seg = OP == CG_PTR ? jb.n - 1 : jb.n;   // elements that come from a frame's segment
  long long src_at[CL_UNROLL], add[CL_UNROLL];
  ClSeg g0 = {};
  long long add0 = 0;
  if (UNIFORM) {
    g0 = load_seg(P, jb.kind, flo, 1);
    add0 = graph_add<OP>(P, flo, g0);
  }
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) {
    const long long e = e0 + u * CL_THREADS + threadIdx.x;
    src_at[u] = -1;
    add[u] = 0;
    if (e < e1 && e < n_seg) {
      ClSeg g = g0;
      long long a = add0;
      if (!UNIFORM) {
        const int f = find_frame(P.out[jb.kind], flo, fhi, e, 1);
        g = load_seg(P, jb.kind, f, 1);
        a = graph_add<OP>(P, f, g);
      }
      const long long local = e - g.out0;
      if (local >= 0 && local < g.len && g.src0 >= 0 && g.src0 + local < jb.src_rows) {
        src_at[u] = g.src0 + local;
        add[u] = a;
      }
    }
  }
  int32_t *__restrict__ dst = (int32_t *)jb.dst;
  long long v[CL_UNROLL];
  if (OP == CG_PTR) {
    const long long *__restrict__ src = (const long long *)jb.src;
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u) v[u] = src_at[u] >= 0 ? src[src_at[u]] : 0;
  } else {
    const int32_t *__restrict__ src = (const int32_t *)jb.src;
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u) v[u] = src_at[u] >= 0 ? (long long)src[src_at[u]] : 0;
  }
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) {
    const long long e = e0 + u * CL_THREADS + threadIdx.x;
    if (src_at[u] >= 0) dst[e] = (int32_t)(v[u] + add[u]);
    else if (OP == CG_PTR && e == n_seg && e < e1) dst[e] = (int32_t)n_edges_out;
  }
}

__global__ __launch_bounds__(CL_THREADS) void collate_graph_kernel(const ClJobs J, const ClPtrs P, const long long n_edges_out) {
  for (long long tile = blockIdx.x; tile < J.n_tiles; tile += gridDim.x) {
    int j = 0;
    for (int k = 1; k < J.n_jobs; ++k)
      if (tile >= J.job[k].tile0) j = k;
    const ClJob &jb = J.job[j];
    const long long e0 = (tile - jb.tile0) * CL_TILE;
    const long long e1 = e0 + CL_TILE < jb.n ? e0 + CL_TILE : jb.n;
    if (jb.op == CG_ZERO || P.B == 0) {   // no edge anywhere: every offset is 0 (a batch of no frames holds that one element)
      int32_t *__restrict__ dst = (int32_t *)jb.dst;
      for (long long e = e0 + threadIdx.x; e < e1; e += CL_THREADS) dst[e] = 0;
      continue;
    }
    const int64_t *__restrict__ po = P.out[jb.kind];
    const int flo = find_frame(po, 0, P.B - 1, e0, 1);
    const int fhi = find_frame(po, flo, P.B - 1, e1 - 1, 1);
    if (flo == fhi) {
      if (jb.op == CG_PTR) graph_tile<CG_PTR, true>(jb, P, e0, e1, flo, fhi, n_edges_out);
      else if (jb.op == CG_NODE_ID) graph_tile<CG_NODE_ID, true>(jb, P, e0, e1, flo, fhi, n_edges_out);
      else graph_tile<CG_EDGE_ID, true>(jb, P, e0, e1, flo, fhi, n_edges_out);
    } else {
      if (jb.op == CG_PTR) graph_tile<CG_PTR, false>(jb, P, e0, e1, flo, fhi, n_edges_out);
      else if (jb.op == CG_NODE_ID) graph_tile<CG_NODE_ID, false>(jb, P, e0, e1, flo, fhi, n_edges_out);
      else graph_tile<CG_EDGE_ID, false>(jb, P, e0, e1, flo, fhi, n_edges_out);
    }
  }
}

static void add_job(ClJobs &J, const void *src, void *dst, long long n, long long src_rows, int width, int kind, int op) {
  if (n <= 0) return;   // an empty table (a batch without edges) takes no tile
  ClJob &jb = J.job[J.n_jobs++];
  jb.src = src;
  jb.dst = dst;
  jb.n = n;
  jb.tile0 = J.n_tiles;
  jb.src_rows = src_rows;
  jb.width = width;
  jb.kind = kind;
  jb.op = op;
  J.n_tiles += (n + CL_TILE - 1) / CL_TILE;
}

// ---- equal-sized frames (fastegnn_collate_draw / fastegnn_collate_gather_uniform): the order drawn here, a frame's place a product ----
constexpr uint64_t CU_STREAM_TAG = 0x5354524Dull;   // the `b` of the keyed permutation: apart from every graph number of an MMD draw

// One workgroup.  Every thread reads the three words first; thread 0 writes cursor and epoch behind the barrier that follows the last
// id, so all ids of a draw come from one state.
__global__ __launch_bounds__(CL_PLAN_THREADS) void collate_draw_kernel(uint64_t *state, int B, int n_frames, int shuffle, int advance,
                                                                        int64_t *__restrict__ ids_out) {
  const uint64_t seed = state[0], epoch = state[1], cursor = state[2];
  const uint64_t nb = (uint64_t)(n_frames / B);   // >= 1: the host checked n_frames >= B >= 1
  const uint64_t c = cursor % nb;
  const uint64_t gkey = perm_draw_key(seed, epoch);
  for (int base = 0; base < B; base += CL_PLAN_THREADS) {
    const int i = base + (int)threadIdx.x;
    if (i < B) {
      const uint64_t j = c * (uint64_t)B + (uint64_t)i;   // < nb * B <= n_frames
      ids_out[i] = (int64_t)(shuffle ? keyed_perm(gkey, CU_STREAM_TAG, (uint64_t)n_frames, j) : j);
    }
  }
  __syncthreads();
  if (advance && threadIdx.x == 0) {
    if (c + 1 >= nb) {
      state[2] = 0;
      state[1] = epoch + 1;
    } else {
      state[2] = c + 1;
    }
  }
}

constexpr int CU_MAX_JOBS = FASTEGNN_COLLATE_TABLES + 1 + 6;   // the float tables, the two rows of edge_index, the six graph arrays
// CU_ADD32 / CU_ADD64: units of 4, 8 or 16 bytes holding 32- / 64-bit integers, every one + slot * add_mul (a float table is CU_ADD32
// with add_mul = 0: adding 0 to the bit pattern is the copy).  CU_PTR: rowptr / cscptr, int64 -> int32, one element per lane.
enum { CU_ADD32 = 0, CU_ADD64 = 1, CU_PTR = 2, CU_ZERO = 3 };

struct CuJob {
  const void *src;
  void *dst;
  long long n;         // output units
  long long tile0;     // first tile of the job
  long long seg;       // units per frame, > 0
  long long add_mul;   // batch slot f adds f * add_mul to every integer
  long long sub_mul;   // CU_PTR: frame id takes id * sub_mul off (its first edge in the packed table)
  int op, unit;        // unit: bytes per lane access
};
struct CuJobs {
  CuJob job[CU_MAX_JOBS];
  const int64_t *ids;
  long long n_tiles, n_edges_out;
  int n_jobs, n_frames;
};

template <int UNIT> struct CuVec;
template <> struct CuVec<4> { using type = unsigned; };
template <> struct CuVec<8> { using type = uint2; };
template <> struct CuVec<16> { using type = uint4; };

__device__ __forceinline__ void cu_add64(unsigned &lo, unsigned &hi, long long a) {
  const unsigned long long v = (((unsigned long long)hi << 32) | lo) + (unsigned long long)a;
  lo = (unsigned)v;
  hi = (unsigned)(v >> 32);
}
template <bool I64> __device__ __forceinline__ void cu_add(unsigned &v, long long a) { v += (unsigned)a; }
template <bool I64> __device__ __forceinline__ void cu_add(uint2 &v, long long a) {
  if (I64) cu_add64(v.x, v.y, a);
  else { v.x += (unsigned)a; v.y += (unsigned)a; }
}
template <bool I64> __device__ __forceinline__ void cu_add(uint4 &v, long long a) {
  if (I64) { cu_add64(v.x, v.y, a); cu_add64(v.z, v.w, a); }
  else { v.x += (unsigned)a; v.y += (unsigned)a; v.z += (unsigned)a; v.w += (unsigned)a; }
}

// slot and offset inside the slot of unit e, from the tile's first slot f0 (one 64-bit division per tile; a unit's own is 32-bit
// whenever the frame's segment allows it)
__device__ __forceinline__ void cu_locate(long long e, long long f0, long long seg, long long &f, long long &local) {
  const long long d = e - f0 * seg;   // < seg + CL_TILE
  const long long q = seg < (1ll << 31) - CL_TILE ? (long long)((unsigned)d / (unsigned)seg) : d / seg;
  f = f0 + q;
  local = d - q * seg;
}

// One tile of one job: CL_UNROLL loads in flight before the stores, consecutive lanes on consecutive units.
template <int UNIT, bool I64>
__device__ __forceinline__ void uniform_tile(const CuJob &jb, const int64_t *__restrict__ ids, int n_frames, long long e0,
                                             long long e1) {
  using V = typename CuVec<UNIT>::type;
  const V *__restrict__ src = (const V *)jb.src;
  V *__restrict__ dst = (V *)jb.dst;
  const long long seg = jb.seg, f0 = e0 / seg;
  long long src_at[CL_UNROLL], add[CL_UNROLL];
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) {
    const long long e = e0 + u * CL_THREADS + threadIdx.x;
    src_at[u] = -1;
    add[u] = 0;
    if (e < e1) {
      long long f, local;
      cu_locate(e, f0, seg, f, local);
      src_at[u] = clamp_id(ids[f], n_frames) * seg + local;
      add[u] = f * jb.add_mul;
    }
  }
  V v[CL_UNROLL];
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u)
    if (src_at[u] >= 0) v[u] = src[src_at[u]];
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u)
    if (src_at[u] >= 0) {
      cu_add<I64>(v[u], add[u]);
      dst[e0 + u * CL_THREADS + threadIdx.x] = v[u];
    }
}

// rowptr / cscptr: element e < n - 1 is node `local` of slot f; the last one is the batch's edge total
__device__ __forceinline__ void uniform_ptr_tile(const CuJob &jb, const int64_t *__restrict__ ids, int n_frames, long long e0,
                                                 long long e1, long long n_edges_out) {
  const long long *__restrict__ src = (const long long *)jb.src;
  int32_t *__restrict__ dst = (int32_t *)jb.dst;
  const long long seg = jb.seg, f0 = e0 / seg;
  long long src_at[CL_UNROLL], add[CL_UNROLL], v[CL_UNROLL];
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) {
    const long long e = e0 + u * CL_THREADS + threadIdx.x;
    src_at[u] = -1;
    add[u] = 0;
    if (e < e1 && e < jb.n - 1) {
      long long f, local;
      cu_locate(e, f0, seg, f, local);
      const long long id = clamp_id(ids[f], n_frames);
      src_at[u] = id * seg + local;
      add[u] = f * jb.add_mul - id * jb.sub_mul;
    }
  }
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) v[u] = src_at[u] >= 0 ? src[src_at[u]] : 0;
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) {
    const long long e = e0 + u * CL_THREADS + threadIdx.x;
    if (src_at[u] >= 0) dst[e] = (int32_t)(v[u] + add[u]);
    else if (e == jb.n - 1 && e < e1) dst[e] = (int32_t)n_edges_out;
  }
}

__global__ __launch_bounds__(CL_THREADS) void collate_gather_uniform_kernel(const CuJobs J) {
  for (long long tile = blockIdx.x; tile < J.n_tiles; tile += gridDim.x) {
    int j = 0;
    for (int k = 1; k < J.n_jobs; ++k)
      if (tile >= J.job[k].tile0) j = k;
    const CuJob &jb = J.job[j];
    const long long e0 = (tile - jb.tile0) * CL_TILE;
    const long long e1 = e0 + CL_TILE < jb.n ? e0 + CL_TILE : jb.n;
    if (jb.op == CU_ZERO) {
      int32_t *__restrict__ dst = (int32_t *)jb.dst;
      for (long long e = e0 + threadIdx.x; e < e1; e += CL_THREADS) dst[e] = 0;
    } else if (jb.op == CU_PTR) {
      uniform_ptr_tile(jb, J.ids, J.n_frames, e0, e1, J.n_edges_out);
    } else if (jb.op == CU_ADD64) {
      if (jb.unit == 16) uniform_tile<16, true>(jb, J.ids, J.n_frames, e0, e1);
      else uniform_tile<8, true>(jb, J.ids, J.n_frames, e0, e1);
    } else {
      if (jb.unit == 16) uniform_tile<16, false>(jb, J.ids, J.n_frames, e0, e1);
      else if (jb.unit == 8) uniform_tile<8, false>(jb, J.ids, J.n_frames, e0, e1);
      else uniform_tile<4, false>(jb, J.ids, J.n_frames, e0, e1);
    }
  }
}

// the widest of 16, 8 and `elem` bytes that divides the frame's segment and both base addresses
static int cu_unit(const void *src, const void *dst, long long seg_bytes, int elem) {
  const unsigned long long any = (unsigned long long)(uintptr_t)src | (unsigned long long)(uintptr_t)dst | (unsigned long long)seg_bytes;
  return any % 16 == 0 ? 16 : (any % 8 == 0 ? 8 : elem);
}

// a job of `elems_per_frame` integers of `elem` bytes per frame over B frames; nothing for an empty table
static void add_uniform_job(CuJobs &J, const void *src, void *dst, long long elems_per_frame, int B, int elem, int op,
                            long long add_mul) {
  if (elems_per_frame <= 0) return;
  CuJob &jb = J.job[J.n_jobs++];
  jb.unit = cu_unit(src, dst, elems_per_frame * elem, elem);
  jb.src = src;
  jb.dst = dst;
  jb.seg = elems_per_frame * elem / jb.unit;
  jb.n = jb.seg * B;
  jb.tile0 = J.n_tiles;
  jb.add_mul = add_mul;
  jb.sub_mul = 0;
  jb.op = op;
  J.n_tiles += (jb.n + CL_TILE - 1) / CL_TILE;
}

static void add_uniform_ptr_job(CuJobs &J, const int64_t *src, int32_t *dst, long long nodes_per_frame, long long edges_per_frame,
                                int B) {
  CuJob &jb = J.job[J.n_jobs++];
  jb.src = src;
  jb.dst = dst;
  jb.unit = 4;
  jb.seg = nodes_per_frame > 0 ? nodes_per_frame : 1;   // a dataset of empty frames: the job is its last element alone
  jb.n = nodes_per_frame * B + 1;
  jb.tile0 = J.n_tiles;
  jb.add_mul = edges_per_frame;
  jb.sub_mul = edges_per_frame;
  jb.op = edges_per_frame > 0 && nodes_per_frame > 0 ? CU_PTR : CU_ZERO;
  J.n_tiles += (jb.n + CL_TILE - 1) / CL_TILE;
}

}  // namespace fe

using namespace fe;

extern "C" {

int fastegnn_collate_plan(const int64_t *ids, int32_t B, const int64_t *src_node_ptr, const int64_t *src_edge_ptr,
                          int32_t n_frames, int64_t *node_ptr_out, int64_t *edge_ptr_out, void *stream) {
  FE_REQUIRE(B >= 0, "collate_plan: B < 0");
  FE_REQUIRE(n_frames >= 1, "collate_plan: the packed dataset holds no frame");
  FE_REQUIRE(node_ptr_out && edge_ptr_out, "collate_plan: null output");
  FE_REQUIRE(B == 0 || (ids && src_node_ptr && src_edge_ptr), "collate_plan: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  hipLaunchKernelGGL(collate_plan_kernel, dim3(1), dim3(CL_PLAN_THREADS), 0, st, ids, B, src_node_ptr, src_edge_ptr, n_frames,
                     node_ptr_out, edge_ptr_out);
  return check_launch("collate_plan");
}

int fastegnn_collate_gather(const int64_t *ids, int32_t B, const int64_t *src_node_ptr, const int64_t *src_edge_ptr,
                            int32_t n_frames, int64_t src_nodes, int64_t src_edges, const int64_t *node_ptr_out,
                            const int64_t *edge_ptr_out, int64_t n_nodes_out, int64_t n_edges_out, const void *const *src_tables,
                            void *const *dst_tables, const int32_t *widths, int64_t *batch_out, void *stream) {
  FE_REQUIRE(B >= 0, "collate_gather: B < 0");
  FE_REQUIRE(n_frames >= 1, "collate_gather: the packed dataset holds no frame");
  FE_REQUIRE(src_nodes >= 0 && src_edges >= 0 && n_nodes_out >= 0 && n_edges_out >= 0, "collate_gather: negative size");
  if (B == 0) return FASTEGNN_OK;
  FE_REQUIRE(ids && src_node_ptr && src_edge_ptr && node_ptr_out && edge_ptr_out && src_tables && dst_tables && widths,
             "collate_gather: null pointer");
  ClJobs J = {};
  for (int t = 0; t < FASTEGNN_COLLATE_TABLES - 1; ++t) {
    FE_REQUIRE(widths[t] >= 0 && widths[t] <= (1 << 20), "collate_gather: row width out of range (0 .. 2^20)");
    const int kind = t < FASTEGNN_COLLATE_EDGE_ATTR ? CL_NODE : (t == FASTEGNN_COLLATE_EDGE_ATTR ? CL_EDGE : CL_FRAME);
    const long long rows = kind == CL_NODE ? n_nodes_out : (kind == CL_EDGE ? n_edges_out : (long long)B);
    const long long src_rows = kind == CL_NODE ? src_nodes : (kind == CL_EDGE ? src_edges : (long long)n_frames);
    FE_REQUIRE(rows * widths[t] == 0 || (src_tables[t] && dst_tables[t]), "collate_gather: null table");
    add_job(J, src_tables[t], dst_tables[t], rows * widths[t], src_rows, widths[t], kind, CL_COPY32);
  }
  const int64_t *ei_src = (const int64_t *)src_tables[FASTEGNN_COLLATE_EDGE_INDEX];
  int64_t *ei_dst = (int64_t *)dst_tables[FASTEGNN_COLLATE_EDGE_INDEX];
  FE_REQUIRE(n_edges_out == 0 || (ei_src && ei_dst), "collate_gather: null edge_index");
  for (int r = 0; r < 2 && n_edges_out > 0; ++r)   // row r of [2,E] on both sides
    add_job(J, ei_src + (size_t)r * src_edges, ei_dst + (size_t)r * n_edges_out, n_edges_out, src_edges, 1, CL_EDGE, CL_INDEX64);
  if (batch_out) add_job(J, nullptr, batch_out, n_nodes_out, src_nodes, 1, CL_NODE, CL_BATCH64);
  if (J.n_tiles == 0) return FASTEGNN_OK;   // nothing to write: no launch on an empty grid
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  ClPtrs P;
  P.ids = ids;
  P.src[0] = src_node_ptr;
  P.src[1] = src_edge_ptr;
  P.out[0] = node_ptr_out;
  P.out[1] = edge_ptr_out;
  P.B = B;
  P.n_frames = n_frames;
  const int grid = (int)(J.n_tiles < CL_MAX_BLOCKS ? J.n_tiles : CL_MAX_BLOCKS);
  hipLaunchKernelGGL(collate_gather_kernel, dim3(grid), dim3(CL_THREADS), 0, st, J, P);
  return check_launch("collate_gather");
}

int fastegnn_collate_graph(const int64_t *ids, int32_t B, const int64_t *src_node_ptr, const int64_t *src_edge_ptr, int32_t n_frames,
                           int64_t src_nodes, int64_t src_edges, const int64_t *node_ptr_out, const int64_t *edge_ptr_out,
                           int64_t n_nodes_out, int64_t n_edges_out, const int64_t *g_rowptr, const int32_t *g_erow,
                           const int32_t *g_col, const int32_t *g_perm, const int64_t *g_cscptr, const int32_t *g_csc_eid,
                           int32_t *rowptr, int32_t *erow, int32_t *col, int32_t *perm, int32_t *cscptr, int32_t *csc_eid,
                           int32_t *chunk_row, int32_t *n_chunks, void *stream) {
  FE_REQUIRE(B >= 0, "collate_graph: B < 0");
  FE_REQUIRE(n_frames >= 1, "collate_graph: the packed dataset holds no frame");
  FE_REQUIRE(src_nodes >= 0 && src_edges >= 0 && n_nodes_out >= 0 && n_edges_out >= 0, "collate_graph: negative size");
  FE_REQUIRE(n_nodes_out < 0x7fffffffll && n_edges_out <= 0x7fffffffll, "collate_graph: the batch exceeds the int32 sizes of build_csr");
  FE_REQUIRE(B > 0 || (n_nodes_out == 0 && n_edges_out == 0), "collate_graph: nodes or edges in a batch of no frames");
  FE_REQUIRE(rowptr && chunk_row && n_chunks, "collate_graph: null output");
  FE_REQUIRE((cscptr == nullptr) == (csc_eid == nullptr), "collate_graph: cscptr and csc_eid are given or omitted together");
  const bool want_csc = cscptr != nullptr;
  FE_REQUIRE((g_cscptr == nullptr) == (g_csc_eid == nullptr), "collate_graph: g_cscptr and g_csc_eid are given or omitted together");
  FE_REQUIRE(B == 0 || (ids && src_node_ptr && src_edge_ptr && node_ptr_out && edge_ptr_out), "collate_graph: null pointer");
  FE_REQUIRE(n_edges_out == 0 || (g_rowptr && g_erow && g_col && g_perm && erow && col && perm), "collate_graph: null pointer");
  FE_REQUIRE(n_edges_out == 0 || !want_csc || g_cscptr, "collate_graph: a col-keyed index is asked for but the packed tables hold none");
  const long long np1 = n_nodes_out + 1;
  const int ptr_op = n_edges_out > 0 ? CG_PTR : CG_ZERO;
  ClJobs J = {};
  add_job(J, g_rowptr, rowptr, np1, src_nodes, 1, CL_NODE, ptr_op);
  if (want_csc) add_job(J, g_cscptr, cscptr, np1, src_nodes, 1, CL_NODE, ptr_op);
  add_job(J, g_erow, erow, n_edges_out, src_edges, 1, CL_EDGE, CG_NODE_ID);
  add_job(J, g_col, col, n_edges_out, src_edges, 1, CL_EDGE, CG_NODE_ID);
  add_job(J, g_perm, perm, n_edges_out, src_edges, 1, CL_EDGE, CG_EDGE_ID);
  if (want_csc) add_job(J, g_csc_eid, csc_eid, n_edges_out, src_edges, 1, CL_EDGE, CG_EDGE_ID);
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  ClPtrs P;
  P.ids = ids;
  P.src[0] = src_node_ptr;
  P.src[1] = src_edge_ptr;
  P.out[0] = node_ptr_out;
  P.out[1] = edge_ptr_out;
  P.B = B;
  P.n_frames = n_frames;
  const int grid = (int)(J.n_tiles < CL_MAX_BLOCKS ? J.n_tiles : CL_MAX_BLOCKS);   // rowptr is never empty: at least one tile
  hipLaunchKernelGGL(collate_graph_kernel, dim3(grid), dim3(CL_THREADS), 0, st, J, P, (long long)n_edges_out);
  const int nch = csr_chunk_count((int)n_edges_out);
  *n_chunks = nch;
  launch_chunk_rows(rowptr, (int)n_nodes_out, nch, chunk_row, st);
  return check_launch("collate_graph");
}

int fastegnn_collate_draw(uint64_t *state, int32_t B, int32_t n_frames, int32_t shuffle, int32_t advance, int64_t *ids_out,
                          void *stream) {
  FE_REQUIRE(state && ids_out, "collate_draw: null pointer");
  FE_REQUIRE(B >= 1, "collate_draw: B < 1");
  FE_REQUIRE(n_frames >= B, "collate_draw: n_frames < B (a stream yields full batches only)");
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  hipLaunchKernelGGL(collate_draw_kernel, dim3(1), dim3(CL_PLAN_THREADS), 0, st, state, B, n_frames, shuffle, advance, ids_out);
  return check_launch("collate_draw");
}

int fastegnn_collate_gather_uniform(const int64_t *ids, int32_t B, int32_t n_frames, int64_t nodes_per_frame,
                                    int64_t edges_per_frame, int64_t src_nodes, int64_t src_edges, const void *const *src_tables,
                                    void *const *dst_tables, const int32_t *widths, const int64_t *g_rowptr, const int32_t *g_erow,
                                    const int32_t *g_col, const int32_t *g_perm, const int64_t *g_cscptr, const int32_t *g_csc_eid,
                                    int32_t *rowptr, int32_t *erow, int32_t *col, int32_t *perm, int32_t *cscptr, int32_t *csc_eid,
                                    int32_t *chunk_row, int32_t *n_chunks, void *stream) {
  FE_REQUIRE(B >= 1, "collate_gather_uniform: B < 1");
  FE_REQUIRE(n_frames >= 1, "collate_gather_uniform: the packed dataset holds no frame");
  FE_REQUIRE(nodes_per_frame >= 0 && edges_per_frame >= 0, "collate_gather_uniform: negative size");
  FE_REQUIRE(nodes_per_frame <= (1ll << 40) && edges_per_frame <= (1ll << 40), "collate_gather_uniform: frame size out of range");
  FE_REQUIRE(edges_per_frame == 0 || nodes_per_frame >= 1, "collate_gather_uniform: edges in frames without nodes");
  FE_REQUIRE(src_nodes == (long long)n_frames * nodes_per_frame && src_edges == (long long)n_frames * edges_per_frame,
             "collate_gather_uniform: src_nodes / src_edges are not n_frames times the per-frame counts");
  FE_REQUIRE(ids && src_tables && dst_tables && widths, "collate_gather_uniform: null pointer");
  const long long n_nodes_out = (long long)B * nodes_per_frame, n_edges_out = (long long)B * edges_per_frame;
  CuJobs J = {};
  for (int t = 0; t < FASTEGNN_COLLATE_TABLES - 1; ++t) {
    FE_REQUIRE(widths[t] >= 0 && widths[t] <= (1 << 20), "collate_gather_uniform: row width out of range (0 .. 2^20)");
    const long long count = t < FASTEGNN_COLLATE_EDGE_ATTR ? nodes_per_frame : (t == FASTEGNN_COLLATE_EDGE_ATTR ? edges_per_frame : 1);
    FE_REQUIRE(count * widths[t] == 0 || (src_tables[t] && dst_tables[t]), "collate_gather_uniform: null table");
    add_uniform_job(J, src_tables[t], dst_tables[t], count * widths[t], B, 4, CU_ADD32, 0);
  }
  const int64_t *ei_src = (const int64_t *)src_tables[FASTEGNN_COLLATE_EDGE_INDEX];
  int64_t *ei_dst = (int64_t *)dst_tables[FASTEGNN_COLLATE_EDGE_INDEX];
  FE_REQUIRE(edges_per_frame == 0 || (ei_src && ei_dst), "collate_gather_uniform: null edge_index");
  for (int r = 0; r < 2 && edges_per_frame > 0; ++r)   // row r of [2,E] on both sides
    add_uniform_job(J, ei_src + (size_t)r * src_edges, ei_dst + (size_t)r * n_edges_out, edges_per_frame, B, 8, CU_ADD64,
                    nodes_per_frame);
  const bool want_graph = rowptr != nullptr;
  if (want_graph) {
    FE_REQUIRE(chunk_row && n_chunks, "collate_gather_uniform: null output");
    FE_REQUIRE(n_nodes_out < 0x7fffffffll && n_edges_out <= 0x7fffffffll,
               "collate_gather_uniform: the batch exceeds the int32 sizes of build_csr");
    FE_REQUIRE((cscptr == nullptr) == (csc_eid == nullptr), "collate_gather_uniform: cscptr and csc_eid are given or omitted together");
    const bool want_csc = cscptr != nullptr;
    // the packed tables are looked at only where there are edges: a dataset without any holds empty (null) edge arrays
    FE_REQUIRE(edges_per_frame == 0 || (g_rowptr && g_erow && g_col && g_perm && erow && col && perm),
               "collate_gather_uniform: null pointer");
    FE_REQUIRE(edges_per_frame == 0 || !want_csc || (g_cscptr && g_csc_eid),
               "collate_gather_uniform: a col-keyed index is asked for but the packed tables hold none");
    add_uniform_ptr_job(J, g_rowptr, rowptr, nodes_per_frame, edges_per_frame, B);
    if (want_csc) add_uniform_ptr_job(J, g_cscptr, cscptr, nodes_per_frame, edges_per_frame, B);
    add_uniform_job(J, g_erow, erow, edges_per_frame, B, 4, CU_ADD32, nodes_per_frame);
    add_uniform_job(J, g_col, col, edges_per_frame, B, 4, CU_ADD32, nodes_per_frame);
    add_uniform_job(J, g_perm, perm, edges_per_frame, B, 4, CU_ADD32, edges_per_frame);
    if (want_csc) add_uniform_job(J, g_csc_eid, csc_eid, edges_per_frame, B, 4, CU_ADD32, edges_per_frame);
  }
  if (J.n_tiles == 0) return FASTEGNN_OK;   // nothing to write: no launch on an empty grid
  hipStream_t st = (hipStream_t)stream;
  J.ids = ids;
  J.n_frames = n_frames;
  J.n_edges_out = n_edges_out;
  const int grid = (int)(J.n_tiles < CL_MAX_BLOCKS ? J.n_tiles : CL_MAX_BLOCKS);
  {
    ProfScope _ps(K_MISC, st);
    hipLaunchKernelGGL(collate_gather_uniform_kernel, dim3(grid), dim3(CL_THREADS), 0, st, J);
  }
  if (want_graph) {
    ProfScope _ps(K_MISC, st);
    const int nch = csr_chunk_count((int)n_edges_out);
    *n_chunks = nch;
    launch_chunk_rows(rowptr, (int)n_nodes_out, nch, chunk_row, st);
  }
  return check_launch("collate_gather_uniform");
}

}  // extern "C"

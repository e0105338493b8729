// Mini-batch assembly from device-resident TRAJECTORIES (fastegnn_amd/data.py: TrajectoryDataset / TrajectoryLoader).  The dataset is
// the positions themselves -- one table pos [rows,3], every trajectory frame after frame -- plus the particle kinds; a sample is a pair
// (trajectory, start frame) and its node tensors are slices and differences of three frames (datasets/simulation/dataset.py:71-93,
// datasets/protein/dataset.py:81-173).  The node side of a batch of B samples is THREE launches whatever B is:
//   plan    one workgroup: the batch's node offsets ptr [B+1] and, per slot, the first source row of frames f, f+1, f+dt and of the
//           trajectory's kinds (the scan-in-rounds of collate.hip's plan kernel)
//   gather  one launch over the N nodes: loc_0, loc_t, vel_0, node_feat, node_attr, batch.  A tile finds the slots it touches by a
//           binary search in ptr; a tile inside one slot searches nothing per node (collate.hip's gather)
//   mean    one workgroup per graph: loc_mean [B,3,C], summed in fp64 in one fixed order
// A dataset with a rigid motion per sample (rotation / translation of TrajectoryDataset) runs `gather_moved` instead: the same launch
// with the slot's motion applied to loc_0, loc_t and vel_0 before they are stored; its mean is taken over the moved loc_0
// (rollout.hip's graph kernel), so that the node side is plan, the selection of the motion rows, gather_moved, mean: four launches.
// No atomics, no workspace besides the outputs and the slot table, 64-bit offsets throughout.  Sample ids, trajectory numbers and frame
// numbers are clamped, and a node whose source rows do not lie inside the tables is skipped: nothing is read outside pos / kind and
// nothing is written beyond the sizes the host gave, whatever the device arrays hold.
#include "kernels.h"

namespace fe {

constexpr int TJ_PLAN_THREADS = 1024;
constexpr int TJ_THREADS = 256;
constexpr int TJ_UNROLL = 4;                        // nodes per thread and tile: 36 loads in flight before the stores
constexpr int TJ_TILE = TJ_THREADS * TJ_UNROLL;
constexpr int TJ_MAX_BLOCKS = 2048;                 // beyond that the workgroups stride over the tiles
constexpr int TJ_MEAN_THREADS = 256;                // part of loc_mean's summation order: a change changes its last bits
constexpr int TJ_SLOT = FASTEGNN_TRAJ_SLOT_WORDS;

struct TjSet {   // the dataset's device tables
  const int64_t *samples;                   // [n_samples, 2] (trajectory, start frame)
  const int64_t *row0, *n, *T, *kind0;      // [n_traj]
  long long n_samples;
  int n_traj, delta_t;
};

struct TjBatch {
  const int64_t *ptr;     // [B + 1]
  const int64_t *slots;   // [B, TJ_SLOT]
  const float *pos, *kind, *kind_scaled;
  long long pos_rows, kind_rows, N;
  int B;
  const float *motion;   // [B, 12]: R row-major, then t (the moved gather alone)
  int has_t;
};

struct TjOut {
  float *loc_0, *loc_t, *vel_0, *node_feat, *node_attr;
  int64_t *batch;
};

__device__ __forceinline__ long long tj_clamp(long long v, long long n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---- plan: exclusive scan of the samples' node counts, 1024 samples per round with a running carry; the slot table on the way ----
__global__ __launch_bounds__(TJ_PLAN_THREADS) void traj_plan_kernel(const int64_t *__restrict__ ids, int B, const TjSet S,
                                                                     int64_t *__restrict__ ptr_out, int64_t *__restrict__ slots) {
  __shared__ long long wsum[TJ_PLAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  long long carry = 0;   // the same in every thread
  for (int base = 0; base < B; base += TJ_PLAN_THREADS) {
    const int i = base + t;
    long long c = 0;
    if (i < B) {
      const long long sid = tj_clamp(ids[i], S.n_samples);
      const long long tr = tj_clamp(S.samples[2 * sid], S.n_traj);
      const long long n = S.n[tr] < 0 ? 0 : S.n[tr];
      const long long last = S.T[tr] >= 1 ? S.T[tr] - 1 : 0;
      const long long f = tj_clamp(S.samples[2 * sid + 1], last + 1);
      const long long f1 = f + 1 < last ? f + 1 : last, ft = f + S.delta_t < last ? f + S.delta_t : last;
      const long long r0 = S.row0[tr];
      slots[(long long)i * TJ_SLOT + 0] = r0 + f * n;
      slots[(long long)i * TJ_SLOT + 1] = r0 + f1 * n;
      slots[(long long)i * TJ_SLOT + 2] = r0 + ft * n;
      slots[(long long)i * TJ_SLOT + 3] = S.kind0[tr];
      c = n;
    }
    long long s = c;   // inclusive scan inside the wave
    for (int off = 1; off < 64; off <<= 1) {
      const long long v = __shfl_up(s, off);
      if (lane >= off) s += v;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    long long before = 0, total = 0;
    for (int w = 0; w < TJ_PLAN_THREADS / 64; ++w) {
      const long long v = wsum[w];
      if (w < wave) before += v;
      total += v;
    }
    if (i < B) ptr_out[i] = carry + before + s - c;
    carry += total;
    __syncthreads();   // wsum is rewritten by the next round
  }
  if (t == 0) ptr_out[B] = carry;
}

// ---- gather ----
// largest f in [lo, hi] with ptr[f] <= e (ptr[lo] <= e is the caller's; a slot without nodes shares its offset with the next one,
// which this rule skips)
__device__ __forceinline__ int tj_find_slot(const int64_t *__restrict__ ptr, int lo, int hi, long long e) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct TjSeg {   // slot f of the batch: its first node, its node count, its source rows
  long long out0, len, r0, r1, rt, k0;
  bool ok;       // every source row of the slot lies inside the tables
};
__device__ __forceinline__ TjSeg tj_load_seg(const TjBatch &P, int f) {
  TjSeg g;
  g.out0 = P.ptr[f];
  g.len = P.ptr[f + 1] - g.out0;
  const int64_t *__restrict__ s = P.slots + (long long)f * TJ_SLOT;
  g.r0 = s[0];
  g.r1 = s[1];
  g.rt = s[2];
  g.k0 = s[3];
  // len <= N here or no node of the slot is below N; the sums below cannot wrap for rows that pass the first comparisons
  g.ok = g.len > 0 && g.r0 >= 0 && g.r1 >= 0 && g.rt >= 0 && g.k0 >= 0 && g.r0 <= P.pos_rows - g.len && g.r1 <= P.pos_rows - g.len &&
         g.rt <= P.pos_rows - g.len && g.k0 <= P.kind_rows - g.len;
  return g;
}

// |v| = sqrt((vx*vx + vy*vy) + vz*vz), every operation rounded to fp32 by itself (what numpy's float32 evaluation gives): contraction
// is switched off for these statements -- the __fmul_rn / __fadd_rn of this toolchain are plain operators and would be fused -- and
// the root is sqrtf, which this toolchain expands to the correctly rounded sequence (__fsqrt_rn is the native 1-ulp instruction here)
__device__ __forceinline__ float tj_speed(float vx, float vy, float vz) {
#pragma clang fp contract(off)
  const float xx = vx * vx;
  const float yy = vy * vy;
  const float zz = vz * vz;
  const float s = (xx + yy) + zz;
  return sqrtf(s);
}

// The rigid motion of include/fastegnn_hip.h ("rigid motions"): q[j] = ((p[0]*R[0][j] + p[1]*R[1][j]) + p[2]*R[2][j]), every operation
// rounded to fp32 by itself (contraction off, for tj_speed's reason: torch's elementwise restatement fuses nothing), then + t[j] when
// `shift` -- without it no addition runs at all (p + 0.0f would turn -0.0 into +0.0).  m: the 12 values R row-major, then t.
__device__ __forceinline__ void tj_move(const float (&m)[12], const float (&p)[3], bool shift, float (&q)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float a = p[0] * m[j];
    const float b = p[1] * m[3 + j];
    const float c = p[2] * m[6 + j];
    const float r = (a + b) + c;
    q[j] = shift ? r + m[9 + j] : r;
  }
}

// One tile of TJ_TILE nodes.  UNIFORM: the whole tile lies in slot flo (its segment is the same for every lane and is loaded once);
// otherwise every node finds its slot in [flo, fhi].  MOVED: the slot's motion (P.motion, row = the slot, which is below B) is applied
// to the three vectors before they are stored and before the speed is taken; a UNIFORM tile loads its 12 values once.
template <bool UNIFORM, bool MOVED = false>
__device__ __forceinline__ void traj_tile(const TjBatch &P, const TjOut &O, long long e0, long long e1, int flo, int fhi) {
  // a node that is skipped keeps row 0 of both tables as its source: every load below is unconditional (a load under a per-node
  // condition is branched around and waited for by itself), and the host call requires both tables to hold a row
  long long p0[TJ_UNROLL], p1[TJ_UNROLL], pt[TJ_UNROLL], pk[TJ_UNROLL];
  int slot[TJ_UNROLL];
  bool on[TJ_UNROLL];
  TjSeg g0 = {};
  if (UNIFORM) g0 = tj_load_seg(P, flo);
#pragma unroll
  for (int u = 0; u < TJ_UNROLL; ++u) {
    const long long e = e0 + u * TJ_THREADS + threadIdx.x;
    p0[u] = p1[u] = pt[u] = pk[u] = 0;
    on[u] = false;
    slot[u] = flo;
    if (e < e1) {
      TjSeg g = g0;
      if (!UNIFORM) {
        slot[u] = tj_find_slot(P.ptr, flo, fhi, e);
        g = tj_load_seg(P, slot[u]);
      }
      const long long local = e - g.out0;
      if (g.ok && local >= 0 && local < g.len) {
        on[u] = true;
        p0[u] = g.r0 + local;
        p1[u] = g.r1 + local;
        pt[u] = g.rt + local;
        pk[u] = g.k0 + local;
      }
    }
  }
  float a[TJ_UNROLL][3], b[TJ_UNROLL][3], c[TJ_UNROLL][3], kd[TJ_UNROLL], ks[TJ_UNROLL];
#pragma unroll
  for (int u = 0; u < TJ_UNROLL; ++u) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[u][k] = P.pos[p0[u] * 3 + k];
      b[u][k] = P.pos[p1[u] * 3 + k];
      c[u][k] = P.pos[pt[u] * 3 + k];
    }
    kd[u] = P.kind[pk[u]];
    ks[u] = P.kind_scaled[pk[u]];
  }
  // the motions: one row for a UNIFORM tile, else the row of every node's slot -- slot[u] lies in [flo, fhi], below B, also for a node
  // that is skipped (it keeps flo), so these loads are unconditional as well
  constexpr int TJ_ROWS = MOVED ? (UNIFORM ? 1 : TJ_UNROLL) : 1;
  float mo[TJ_ROWS][12] = {};
  if (MOVED) {
#pragma unroll
    for (int u = 0; u < TJ_ROWS; ++u) {
      const long long row = UNIFORM ? flo : slot[u];
#pragma unroll
      for (int k = 0; k < 12; ++k) mo[u][k] = P.motion[row * 12 + k];
    }
  }
#pragma unroll
  for (int u = 0; u < TJ_UNROLL; ++u) {
    if (!on[u]) continue;
    const long long e = e0 + u * TJ_THREADS + threadIdx.x;
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = b[u][k] - a[u][k];   // the difference first, then its rotation
    if (MOVED) {
      const float (&m)[12] = mo[UNIFORM ? 0 : u];
      const bool shift = P.has_t != 0;
      float qa[3], qc[3], qv[3];
      tj_move(m, a[u], shift, qa);
      tj_move(m, c[u], shift, qc);
      tj_move(m, v, false, qv);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a[u][k] = qa[k];
        c[u][k] = qc[k];
        v[k] = qv[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      O.loc_0[e * 3 + k] = a[u][k];
      O.loc_t[e * 3 + k] = c[u][k];
      O.vel_0[e * 3 + k] = v[k];
    }
    O.node_feat[e * 2 + 0] = tj_speed(v[0], v[1], v[2]);
    O.node_feat[e * 2 + 1] = ks[u];
    O.node_attr[e] = kd[u];
    O.batch[e] = slot[u];
  }
}

__global__ __launch_bounds__(TJ_THREADS) void traj_gather_kernel(const TjBatch P, const TjOut O, const long long n_tiles) {
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long e0 = tile * TJ_TILE;
    const long long e1 = e0 + TJ_TILE < P.N ? e0 + TJ_TILE : P.N;
    const int flo = tj_find_slot(P.ptr, 0, P.B - 1, e0);
    const int fhi = tj_find_slot(P.ptr, flo, P.B - 1, e1 - 1);
    if (flo == fhi) traj_tile<true>(P, O, e0, e1, flo, fhi);
    else traj_tile<false>(P, O, e0, e1, flo, fhi);
  }
}

__global__ __launch_bounds__(TJ_THREADS) void traj_gather_moved_kernel(const TjBatch P, const TjOut O, const long long n_tiles) {
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long e0 = tile * TJ_TILE;
    const long long e1 = e0 + TJ_TILE < P.N ? e0 + TJ_TILE : P.N;
    const int flo = tj_find_slot(P.ptr, 0, P.B - 1, e0);
    const int fhi = tj_find_slot(P.ptr, flo, P.B - 1, e1 - 1);
    if (flo == fhi) traj_tile<true, true>(P, O, e0, e1, flo, fhi);
    else traj_tile<false, true>(P, O, e0, e1, flo, fhi);
  }
}

// ---- mean: loc_mean[b, k, :] = (float)(sum of the graph's loc_0[:, k] in fp64 / n), repeated C times ----
// Thread t adds nodes t, t + 256, ... in ascending order; the 256 partial sums are added pairwise over strides 128, 64, .. 1.  The
// order depends on TJ_MEAN_THREADS and the node count alone: two calls give the same bits.
__global__ __launch_bounds__(TJ_MEAN_THREADS) void traj_mean_kernel(const TjBatch P, int C, float *__restrict__ loc_mean) {
  __shared__ double part[3][TJ_MEAN_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long r0 = P.slots[(long long)b * TJ_SLOT];
  long long n = P.ptr[b + 1] - P.ptr[b];
  if (n < 0 || r0 < 0 || r0 > P.pos_rows - n) n = 0;   // (n <= pos_rows or the last test fails: no wrap)
  double s[3] = {0.0, 0.0, 0.0};
  for (long long i = t; i < n; i += TJ_MEAN_THREADS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += (double)P.pos[(r0 + i) * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) part[k][t] = s[k];
  __syncthreads();
  for (int off = TJ_MEAN_THREADS / 2; off >= 1; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int k = 0; k < 3; ++k) part[k][t] += part[k][t + off];
    }
    __syncthreads();
  }
  for (int j = t; j < 3 * C; j += TJ_MEAN_THREADS)
    loc_mean[(long long)b * 3 * C + j] = n > 0 ? (float)(part[j / C][0] / (double)n) : 0.0f;
}

// the arguments the gather and the mean share
static int tj_batch(TjBatch &P, const char *who, const int64_t *ptr, const int64_t *slots, int32_t B, const float *pos,
                    int64_t pos_rows, bool need_pos) {
  if (B < 0 || pos_rows < 0) {
    set_error(std::string(who) + ": negative size");
    return FASTEGNN_E_INVALID;
  }
  if (B > 0 && (!ptr || !slots || (need_pos && !pos))) {
    set_error(std::string(who) + ": null pointer");
    return FASTEGNN_E_INVALID;
  }
  P = TjBatch{};
  P.ptr = ptr;
  P.slots = slots;
  P.pos = pos;
  P.pos_rows = pos_rows;
  P.B = B;
  return FASTEGNN_OK;
}

}  // namespace fe

using namespace fe;

extern "C" {

int fastegnn_traj_plan(const int64_t *ids, int32_t B, const int64_t *samples, int64_t n_samples, const int64_t *traj_row0,
                       const int64_t *traj_n, const int64_t *traj_T, const int64_t *traj_kind0, int32_t n_traj, int32_t delta_t,
                       int64_t *ptr_out, int64_t *slots_out, void *stream) {
  FE_REQUIRE(B >= 0, "traj_plan: B < 0");
  FE_REQUIRE(n_samples >= 1 && n_traj >= 1, "traj_plan: the dataset holds no sample or no trajectory");
  FE_REQUIRE(delta_t >= 0, "traj_plan: delta_t < 0");
  FE_REQUIRE(ptr_out, "traj_plan: null output");
  FE_REQUIRE(B == 0 || (ids && samples && traj_row0 && traj_n && traj_T && traj_kind0 && slots_out), "traj_plan: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  TjSet S;
  S.samples = samples;
  S.row0 = traj_row0;
  S.n = traj_n;
  S.T = traj_T;
  S.kind0 = traj_kind0;
  S.n_samples = n_samples;
  S.n_traj = n_traj;
  S.delta_t = delta_t;
  hipLaunchKernelGGL(traj_plan_kernel, dim3(1), dim3(TJ_PLAN_THREADS), 0, st, ids, B, S, ptr_out, slots_out);
  return check_launch("traj_plan");
}

// _gather and _gather_moved: the same checks, the same grid; `moved` picks the kernel
static int tj_gather(const char *who, const int64_t *ptr, const int64_t *slots, int32_t B, int64_t n_nodes_out, const float *pos,
                     int64_t pos_rows, const float *kind, const float *kind_scaled, int64_t kind_rows, float *loc_0, float *loc_t,
                     float *vel_0, float *node_feat, float *node_attr, int64_t *batch_out, bool moved, const float *motion, int32_t has_t,
                     void *stream) {
  const std::string w(who);
  if (n_nodes_out < 0 || kind_rows < 0) {
    set_error(w + ": negative size");
    return FASTEGNN_E_INVALID;
  }
  TjBatch P;
  const int rc = tj_batch(P, who, ptr, slots, B, pos, pos_rows, n_nodes_out > 0);
  if (rc != FASTEGNN_OK) return rc;
  if (B == 0 || n_nodes_out == 0) return FASTEGNN_OK;   // nothing to write: no launch on an empty grid
  const char *bad = nullptr;
  if (!kind || !kind_scaled || (moved && !motion)) bad = ": null pointer";
  else if (pos_rows < 1 || kind_rows < 1) bad = ": nodes asked for from empty tables";
  else if (!loc_0 || !loc_t || !vel_0 || !node_feat || !node_attr || !batch_out) bad = ": null output";
  if (bad) {
    set_error(w + bad);
    return FASTEGNN_E_INVALID;
  }
  P.kind = kind;
  P.kind_scaled = kind_scaled;
  P.kind_rows = kind_rows;
  P.N = n_nodes_out;
  P.motion = motion;
  P.has_t = has_t;
  TjOut O;
  O.loc_0 = loc_0;
  O.loc_t = loc_t;
  O.vel_0 = vel_0;
  O.node_feat = node_feat;
  O.node_attr = node_attr;
  O.batch = batch_out;
  const long long n_tiles = (n_nodes_out + TJ_TILE - 1) / TJ_TILE;
  const int grid = (int)(n_tiles < TJ_MAX_BLOCKS ? n_tiles : TJ_MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  if (moved) hipLaunchKernelGGL(traj_gather_moved_kernel, dim3(grid), dim3(TJ_THREADS), 0, st, P, O, n_tiles);
  else hipLaunchKernelGGL(traj_gather_kernel, dim3(grid), dim3(TJ_THREADS), 0, st, P, O, n_tiles);
  return check_launch(who);
}

int fastegnn_traj_gather(const int64_t *ptr, const int64_t *slots, int32_t B, int64_t n_nodes_out, const float *pos, int64_t pos_rows,
                         const float *kind, const float *kind_scaled, int64_t kind_rows, float *loc_0, float *loc_t, float *vel_0,
                         float *node_feat, float *node_attr, int64_t *batch_out, void *stream) {
  return tj_gather("traj_gather", ptr, slots, B, n_nodes_out, pos, pos_rows, kind, kind_scaled, kind_rows, loc_0, loc_t, vel_0, node_feat,
                   node_attr, batch_out, false, nullptr, 0, stream);
}

int fastegnn_traj_gather_moved(const int64_t *ptr, const int64_t *slots, int32_t B, int64_t n_nodes_out, const float *pos,
                               int64_t pos_rows, const float *kind, const float *kind_scaled, int64_t kind_rows, float *loc_0,
                               float *loc_t, float *vel_0, float *node_feat, float *node_attr, int64_t *batch_out, const float *motion,
                               int32_t has_t, void *stream) {
  return tj_gather("traj_gather_moved", ptr, slots, B, n_nodes_out, pos, pos_rows, kind, kind_scaled, kind_rows, loc_0, loc_t, vel_0,
                   node_feat, node_attr, batch_out, true, motion, has_t, stream);
}

int fastegnn_traj_mean(const int64_t *ptr, const int64_t *slots, int32_t B, const float *pos, int64_t pos_rows, int32_t C,
                       float *loc_mean, void *stream) {
  FE_REQUIRE(C >= 1 && C <= (1 << 20), "traj_mean: C out of range (1 .. 2^20)");
  TjBatch P;
  const int rc = tj_batch(P, "traj_mean", ptr, slots, B, pos, pos_rows, true);
  if (rc != FASTEGNN_OK) return rc;
  if (B == 0) return FASTEGNN_OK;
  FE_REQUIRE(loc_mean, "traj_mean: null output");
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  hipLaunchKernelGGL(traj_mean_kernel, dim3(B), dim3(TJ_MEAN_THREADS), 0, st, P, C, loc_mean);
  return check_launch("traj_mean");
}

}  // extern "C"

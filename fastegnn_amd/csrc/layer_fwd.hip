// Forward stages S1..S5 of one E_GCL_vel layer (reference: models/FastEGNN.py:192-223).
// Math per stage: oracle/factored.py (same stage names); layout conventions: common.h.
#include <cstdlib>
#include "stages.h"

namespace fe {

// =====================================================================================
// S1 node_pre:  P = h W1a^T + b1, Q = h W1b^T, A = h V1a^T  (first-Linear factorisation of
// edge_mlp.0 / edge_mlp_virtual.0, FastEGNN.py:103,114), velocity / gravity heads (:139-142).
// =====================================================================================
struct NodePreArgs {
  const float *h, *x, *wpack;
  const float *b1, *bv0, *wv2, *bv2, *bg0, *wg2, *bg2;
  float *P, *QX, *A, *svel, *sgrav;
  int N, gravity, has_vel;
  const float *vel, *wv0;   // FastRF: velocity scale from ||vel|| through coord_mlp_vel.0.weight [H,1]
  int C;
  int flags = 0;
  float act_param = 0.f;
};

// MODE: GM_X3 (bf16x3 products of the split images: fp32-grade, 2.7 x fewer matrix cycles than the fp32-input MFMA these
// node-level kernels ran on through round 2 -- 2048 -> 768 cycles per 64x64 product and tile, + one operand split per
// input) or GM_BF16 (bf16 operand mode: one product of the RNE-rounded activation)
template <int MODE>
__global__ __launch_bounds__(64 * NODE_PRE_WAVES) void node_pre_fwd_kernel(NodePreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  unsigned *img = reinterpret_cast<unsigned *>(lds);   // 5 split images: W1A W1B V1A WVEL0 WG0
  float *vec = lds + 5 * IMG3;                         // b1 bv0 wv2 bg0 wg2 wv0
  const int nimg = a.gravity ? 5 : 4;
  load_images_x3(img, wpack_x3(a.wpack, a.C, I_W1A), nimg);
  // (P in units of ln 2 when the edge stage's first layer is folded: the W1a / W1b images carry log2(e), pack.hip)
  if constexpr (edge_fold_first<MODE>()) { for (int i = threadIdx.x; i < H; i += blockDim.x) vec[i] = a.b1 ? a.b1[i] * LOG2E_F : 0.f; }
  else load_floats(vec + 0 * H, a.b1, H);
  load_floats(vec + 1 * H, a.bv0, H);
  load_floats(vec + 2 * H, a.wv2, H);
  load_floats(vec + 3 * H, a.bg0, H);
  load_floats(vec + 4 * H, a.wg2, H);
  load_floats(vec + 5 * H, a.wv0, H);
  __syncthreads();
  const int l = lane_id(), j = l & 15, q = l >> 4;
  const int wave = global_wave_id(), nwaves = (gridDim.x * blockDim.x) >> 6;
  const int ntiles = (a.N + 15) >> 4;
  const float bv2 = (a.has_vel || a.wv0) ? a.bv2[0] : 0.f;
  const float bg2 = a.gravity ? a.bg2[0] : 0.f;
  for (int tile = wave; tile < ntiles; tile += nwaves) {
    const int n = tile * 16 + j;
    const bool valid = n < a.N;
    const int nc = valid ? n : a.N - 1;
    const typename OperandOf<MODE>::type hv = make_operand<MODE>(vload_row(a.h + (size_t)nc * H, q));   // one split / rounding feeds all products
    Vec acc = vload_vec(vec, q);
    gemm_op<MODE>(img, 0, hv, acc);
    if (valid) vstore_row(a.P + (size_t)n * H, q, acc);
    acc = vzero();
    gemm_op<MODE>(img, 1, hv, acc);
    if (valid) {
      vstore_row(a.QX + (size_t)n * QXLD, q, acc);
      if (q == 0) {
        f32x4 xv = {a.x[(size_t)n * 3], a.x[(size_t)n * 3 + 1], a.x[(size_t)n * 3 + 2], 0.f};
        *reinterpret_cast<f32x4 *>(a.QX + (size_t)n * QXLD + H) = xv;
      }
    }
    acc = vzero();
    gemm_op<MODE>(img, 2, hv, acc);
    if (valid) vstore_row(a.A + (size_t)n * H, q, acc);
    float s = 0.f;
    if (a.has_vel) {
      acc = vload_vec(vec + 1 * H, q);
      gemm_op<MODE>(img, 3, hv, acc);
      s = vdot(vsilu(acc FE_ACT(a)), vload_vec(vec + 2 * H, q)) + bv2;
    } else if (a.wv0) {   // FastRF.py:139: coord_mlp_vel(||vel||), the norm is detached (:169)
      const float vx = a.vel[(size_t)nc * 3], vy = a.vel[(size_t)nc * 3 + 1], vz = a.vel[(size_t)nc * 3 + 2];
      acc = vload_vec(vec + 1 * H, q);
      vaxpy(acc, sqrt_f(vx * vx + vy * vy + vz * vz), vload_vec(vec + 5 * H, q));
      s = vdot(vsilu(acc FE_ACT(a)), vload_vec(vec + 2 * H, q)) + bv2;
    }
    if (valid && q == 0) a.svel[n] = s;
    if (a.gravity) {
      acc = vload_vec(vec + 3 * H, q);
      gemm_op<MODE>(img, 4, hv, acc);
      s = vdot(vsilu(acc FE_ACT(a)), vload_vec(vec + 4 * H, q)) + bg2;
      if (valid && q == 0) a.sgrav[n] = s;
    }
  }
}

int node_pre_forward(const fastegnn_layer_t *L, hipStream_t st) {
  FE_REQUIRE(L->h && L->x && L->wpack && L->P && L->QX && L->A && L->svel, "node_pre_forward: null buffer");
  if (L->N == 0) return FASTEGNN_OK;
  const bool grav = has(L, FASTEGNN_F_GRAVITY);
  FE_REQUIRE(!grav || L->sgrav, "node_pre_forward: sgrav null");
  const float *const *p = L->params;
  NodePreArgs a{L->h, L->x, L->wpack, p[FASTEGNN_P_EDGE0_B], p[FASTEGNN_P_VEL0_B], p[FASTEGNN_P_VEL2_W],
                p[FASTEGNN_P_VEL2_B], p[FASTEGNN_P_GRAV0_B], p[FASTEGNN_P_GRAV2_W], p[FASTEGNN_P_GRAV2_B],
                L->P, L->QX, L->A, L->svel, L->sgrav, L->N, grav ? 1 : 0,
                (p[FASTEGNN_P_VEL0_W] && !has(L, FASTEGNN_F_RF)) ? 1 : 0,
                L->vel, has(L, FASTEGNN_F_RF) ? p[FASTEGNN_P_VEL0_W] : nullptr, L->C, L->flags, L->act_param};
  FE_REQUIRE(!has(L, FASTEGNN_F_RF) || (L->vel && p[FASTEGNN_P_VEL0_W] && p[FASTEGNN_P_VEL0_B] && p[FASTEGNN_P_VEL2_W] &&
                                         p[FASTEGNN_P_VEL2_B]),
             "node_pre_forward: FastRF needs vel and the coord_mlp_vel parameters");
  const int ntiles = (L->N + 15) / 16;
  int grid = cdiv(ntiles, NODE_PRE_WAVES);
  if (grid > 256) grid = 256;
  const size_t lds = (5 * IMG3 + 6 * H) * sizeof(float);
  {
    ProfScope _ps_node_pre_fwd_kernel(K_NODE_PRE_FWD, st);
    if (has(L, FASTEGNN_F_BF16)) hipLaunchKernelGGL(node_pre_fwd_kernel<GM_BF16>, dim3(grid), dim3(64 * NODE_PRE_WAVES), lds, st, a);
    else hipLaunchKernelGGL(node_pre_fwd_kernel<GM_NODE_PRE_FWD>, dim3(grid), dim3(64 * NODE_PRE_WAVES), lds, st, a);
  }
  return check_launch("node_pre_fwd_kernel");
}

// =====================================================================================
// S2a graph_xsum: per-graph sum of coordinates and node count (global_mean_pool(coord), :212)
// =====================================================================================
// No atomics and no zeroing: the sum of a graph is built in an order that depends on the node range of the graph and on the
// block size alone, so two runs give the same bits.
//   1. graph_xsum_part_kernel: the nodes are cut into fixed blocks of NB (xsum_block_nodes); one wave per block adds the block's
//      coordinates -- lane l takes the nodes l, l + 64, ... of the block in ascending order, then a butterfly over the lanes -- and
//      stores the block's partial.  A block that straddles graphs has a partial nobody reads.
//   2. xsum_combine (one 256-thread workgroup per graph): the nodes [lo, hi) of the graph are the items
//        head nodes [lo, fb NB) | partials of the whole blocks fb .. lb - 1 | tail nodes [lb NB, hi)
//      (a graph without a whole block: its nodes alone).  Thread t adds the items t, t + 256, ... in ascending order, a butterfly
//      combines the lanes of a wave, the four waves are added as (w0 + w1) + (w2 + w3).  The count is hi - lo.
// The combine runs inside graph_pre_fwd_kernel when the layer is run as a whole (fastegnn_layer_forward: one launch fewer, every
// workgroup of a graph computes the same bits and the first one writes L->xsum) and as graph_xsum_combine_kernel behind the
// staged entry point: the same function, the same bits.
// The partials of the layer call live in L->aggm (free until the edge stage writes it).  The staged call has no layer buffer to
// spare: its partials live in g_xsum_part, ONE array per device, so staged graph_xsum calls on different streams of one device
// must not overlap.
constexpr int XS_BLOCK = 256;     // nodes per block while that leaves at most XS_MAXBLK blocks (1 M nodes): 391 waves at 100 000 nodes
constexpr int XS_MAXBLK = 4096;
__device__ float g_xsum_part[XS_MAXBLK * 4];
static int xsum_block_nodes(int N) {
  const int k = cdiv(N, XS_BLOCK * XS_MAXBLK);
  return XS_BLOCK * (k < 1 ? 1 : k);
}

__global__ __launch_bounds__(256) void graph_xsum_part_kernel(const float *x, int N, int NB, float *part) {
  if (!part) part = g_xsum_part;
  const int l = lane_id(), blk = global_wave_id();
  if ((long)blk * NB >= N) return;
  const int n0 = blk * NB, n1 = min(N, n0 + NB);
  float s[3] = {0.f, 0.f, 0.f};
#pragma unroll 4
  for (int n = n0 + l; n < n1; n += 64) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += x[(size_t)n * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off);
  if (l == 0) *reinterpret_cast<f32x4 *>(part + (size_t)blk * 4) = f32x4{s[0], s[1], s[2], 0.f};
}

// first n in [0, N) with batch[n] >= key (N if none): a 256-ary search by the whole workgroup, three rounds at 100 000 nodes
__device__ __forceinline__ int xsum_lower_bound(const int32_t *batch, int N, int key) {
  int a = 0, e = N;
  while (a < e) {
    const int S = (e - a + 255) / 256, idx = a + (int)threadIdx.x * S;
    const int c = __syncthreads_count(idx < e && batch[idx] < key);
    if (c == 0) e = a;
    else {
      e = min(e, a + c * S);
      a += (c - 1) * S + 1;
    }
  }
  return a;
}
// out[0..3] = (sum x, sum y, sum z, count) of graph b in every thread of the 256-thread workgroup; red: 16 floats of LDS.
// The node range comes from gptr (clamped to [0, N]) when the layer carries it, from the ascending batch otherwise.
__device__ __forceinline__ void xsum_combine(const float *x, const float *part, const int32_t *batch, const int32_t *gptr, int N,
                                             int NB, int b, float *red, float out[4]) {
  if (!part) part = g_xsum_part;
  int lo, hi;
  if (gptr) {
    lo = min(max(gptr[b], 0), N);
    hi = min(max(gptr[b + 1], lo), N);
  } else {
    lo = xsum_lower_bound(batch, N, b);
    hi = xsum_lower_bound(batch, N, b + 1);
  }
  int fb = (lo + NB - 1) / NB, lb = hi / NB;
  if (fb >= lb) fb = lb = hi / NB + 1;                 // no whole block: all nodes are "head" nodes
  const int nhead = min(hi, fb * NB) - lo, nblk = lb - fb, nitems = hi - lo - nblk * (NB - 1);
  float s[3] = {0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < nitems; i += 256) {
    const float *p = i < nhead ? x + (size_t)(lo + i) * 3
                               : (i < nhead + nblk ? part + (size_t)(fb + i - nhead) * 4 : x + (size_t)(lb * NB + i - nhead - nblk) * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += p[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off);
  const int l = lane_id(), w = threadIdx.x >> 6;
  if (l < 3) red[w * 4 + l] = s[l];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = (red[k] + red[4 + k]) + (red[8 + k] + red[12 + k]);
  out[3] = (float)(hi - lo);
}
__device__ __forceinline__ float xsum_pick(const float v[4], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3])); }
__global__ __launch_bounds__(256) void graph_xsum_combine_kernel(const float *x, const int32_t *batch, const int32_t *gptr, int N, int NB,
                                                                 float *xsum) {
  __shared__ float red[16];
  float v[4];
  xsum_combine(x, nullptr, batch, gptr, N, NB, blockIdx.x, red, v);
  if (threadIdx.x < 4) xsum[blockIdx.x * 4 + threadIdx.x] = xsum_pick(v, threadIdx.x);
}

// the block partials of L->x into `part` ([cdiv(N, NB)][4] floats; null: g_xsum_part)
int graph_xsum_partials(const fastegnn_layer_t *L, float *part, hipStream_t st) {
  FE_REQUIRE(L->x && (L->gptr || L->batch), "graph_xsum: null buffer");
  if (L->N == 0) return FASTEGNN_OK;
  const int NB = xsum_block_nodes(L->N);
  { ProfScope _ps_graph_xsum_kernel(K_XSUM, st); hipLaunchKernelGGL(graph_xsum_part_kernel, dim3(cdiv(cdiv(L->N, NB), 4)), dim3(256), 0, st, L->x, L->N, NB, part); }
  return check_launch("graph_xsum_part_kernel");
}
int graph_xsum(const fastegnn_layer_t *L, hipStream_t st) {
  FE_REQUIRE(L->xsum, "graph_xsum: null buffer");
  int rc = graph_xsum_partials(L, nullptr, st);
  if (rc || L->B == 0) return rc;
  { ProfScope _ps_graph_xsum_kernel(K_XSUM, st); hipLaunchKernelGGL(graph_xsum_combine_kernel, dim3(L->B), dim3(256), 0, st, L->x, L->batch, L->gptr, L->N, xsum_block_nodes(L->N), L->xsum); }
  return check_launch("graph_xsum_combine_kernel");
}

// =====================================================================================
// S2b graph_pre: centroid, Gram matrix m_X (:212-214) and the per-(graph,channel) part of
// edge_mlp_virtual.0:  Bc[b,c,:] = V1b Hv[b,:,c] + V1d mX[b][:,c] + c1   (:114)
// =====================================================================================
struct GraphPreArgs {
  const float *xsum, *Z, *HvT, *V0W, *V0B;
  float *Bc;
  int B, C, bf16;
  // the layer call (x non-null): xsum is combined here from the block partials and WRITTEN, and the pools of the virtual stage
  // are zeroed (poolV may be null)
  const float *x, *part;
  const int32_t *batch, *gptr;
  int N, NB;
  float *xsum_out, *poolV, *poolX;
};
// grid (B, GP_SPLIT): the C*64 outputs of a graph are dealt to GP_SPLIT workgroups (each recomputes the graph's small
// Gram matrix): with one big graph the stage was a single workgroup on one CU.
// The V1b and V1d blocks of edge_mlp_virtual.0.weight (row stride 2H + 1 + C) and the graph's Hv rows are staged in LDS with
// coalesced loads: a lane owns an output feature, i.e. a ROW of the weight, and read it from global memory one scattered dword per k.
constexpr int GP_SPLIT = 4;
constexpr int GP_WLD = H + 1;   // row stride of the V1b tile in LDS: lanes along o hit 64 banks
static size_t graph_pre_lds_floats(int C) { return (size_t)3 * C + C * C + H * GP_WLD + (size_t)H * (C + 1) + (size_t)C * H + 16; }
__global__ __launch_bounds__(256) void graph_pre_fwd_kernel(GraphPreArgs a) {
  extern __shared__ float sm[];
  const int C = a.C, b = blockIdx.x, ld = 2 * H + 1 + C;
  float *mz = sm;                 // [3][C]
  float *mX = mz + 3 * C;         // [C][C]
  float *wb = mX + C * C;         // [H][GP_WLD]   V1b[o][k]
  float *wd = wb + H * GP_WLD;    // [H][C + 1]    V1d[o][d]
  float *hv = wd + H * (C + 1);   // [C][H]
  float *red = hv + C * H;        // [16]
  for (int i = threadIdx.x; i < H * H; i += 256) wb[(i >> 6) * GP_WLD + (i & 63)] = a.V0W[(size_t)(i >> 6) * ld + H + (i & 63)];
  for (int i = threadIdx.x; i < H * C; i += 256) wd[(i / C) * (C + 1) + i % C] = a.V0W[(size_t)(i / C) * ld + 2 * H + 1 + i % C];
  for (int i = threadIdx.x; i < C * H; i += 256) hv[i] = a.HvT[(size_t)b * C * H + i];
  float xs[4];
  if (a.x) {
    const int gid = (blockIdx.x * gridDim.y + blockIdx.y) * 256 + threadIdx.x, gstep = gridDim.x * gridDim.y * 256;
    if (a.poolV) for (int i = gid; i < a.B * C * H; i += gstep) a.poolV[i] = 0.f;
    for (int i = gid; i < a.B * 3 * C; i += gstep) a.poolX[i] = 0.f;
    xsum_combine(a.x, a.part, a.batch, a.gptr, a.N, a.NB, b, red, xs);
    if (blockIdx.y == 0 && threadIdx.x < 4) a.xsum_out[b * 4 + threadIdx.x] = xsum_pick(xs, threadIdx.x);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[k] = a.xsum[b * 4 + k];
  }
  const float cnt = fmaxf(xs[3], 1.f);
  for (int i = threadIdx.x; i < 3 * C; i += 256) {
    int k = i / C;
    mz[i] = a.Z[(size_t)b * 3 * C + i] - (k == 0 ? xs[0] : (k == 1 ? xs[1] : xs[2])) / cnt;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += 256) {
    int c = i / C, d = i % C;
    mX[i] = mz[c] * mz[d] + mz[C + c] * mz[C + d] + mz[2 * C + c] * mz[2 * C + d];
  }
  __syncthreads();
  for (int i = blockIdx.y * 256 + threadIdx.x; i < C * H; i += 256 * gridDim.y) {
    int c = i >> 6, o = i & 63;
    const float *w = wb + o * GP_WLD, *h = hv + c * H;
    float acc = a.V0B[o];
    if (a.bf16) { for (int k = 0; k < H; ++k) acc += round_bf(w[k]) * round_bf(h[k]); }   // V1b Hv: bf16 operands
    else { for (int k = 0; k < H; ++k) acc += w[k] * h[k]; }
    for (int d = 0; d < C; ++d) acc += wd[o * (C + 1) + d] * mX[d * C + c];   // Gram columns: always fp32
    a.Bc[((size_t)b * C + c) * H + o] = acc;
  }
}
// part non-null: the layer call -- xsum from the block partials in `part` (graph_xsum_partials), pools zeroed
int graph_pre_forward(const fastegnn_layer_t *L, hipStream_t st, float *part) {
  FE_REQUIRE(L->xsum && L->Z && L->HvT && L->Bc, "graph_pre_forward: null buffer");
  FE_REQUIRE(!part || (L->x && L->poolX && (L->gptr || L->batch)), "graph_pre_forward: null buffer");
  GraphPreArgs a{L->xsum, L->Z, L->HvT, L->params[FASTEGNN_P_VIRT0_W], L->params[FASTEGNN_P_VIRT0_B], L->Bc, L->B, L->C,
                 has(L, FASTEGNN_F_BF16) ? 1 : 0, part ? L->x : nullptr, part, L->batch, L->gptr, L->N, xsum_block_nodes(L->N),
                 L->xsum, L->poolV, L->poolX};
  const size_t lds = graph_pre_lds_floats(L->C) * sizeof(float);
  { ProfScope _ps_graph_pre_fwd_kernel(K_GRAPH_PRE_FWD, st); hipLaunchKernelGGL(graph_pre_fwd_kernel, dim3(L->B, GP_SPLIT), dim3(256), lds, st, a); }
  return check_launch("graph_pre_fwd_kernel");
}

// =====================================================================================
// S3 edge: coord2radial (:180-189) + edge_model (:102-108) + real part of coord_model_vel
// (:125-133) + the segment means of node_model / coord_model_vel (:155, :287-294), fused.
// One wave walks an edge-balanced chunk of CSR rows in 16-edge tiles; sums stay in registers
// until the row changes, so every row is written exactly once (no atomics, deterministic).
// =====================================================================================
// AGGM = false (the layer call of a layer without a node update: aggm feeds node_model alone): the message tile is not transposed, its
// rows are not summed and aggm is not written; aggx is built by the same additions in the same order (bit for bit).
constexpr int EDGE_FWD_IMG_FLOATS = 2 * IMG3;
template <int MODE, bool AGGM = true>
__global__ __launch_bounds__(64 * EDGE_FWD_WAVES) void edge_fwd_kernel(EdgeArgs a, int C) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef FE_ISA_CONST   // assembly-only builds of tools/isa_budget.py: the layer flags as a constant (straight-line code of ONE configuration)
  a.flags = FE_ISA_CONST; a.ea_dim = 2; a.bx2 = nullptr; a.attw = nullptr;
#endif
  float *img = lds;                              // W2, WX1 (fp32 or split images)
  float *vec = lds + EDGE_FWD_IMG_FLOATS;        // EV_COUNT vectors
  float *tiles = vec + EV_COUNT * H;             // per wave: [16][TS] + [16][4]
  load_images_x3(reinterpret_cast<unsigned *>(img), wpack_x3(a.wpack, C, I_W2), 2);
  constexpr bool FOLD = edge_fold<false, MODE, false>();   // S.m arrives as log2(e) x the message: 1/deg absorbs the factor
  edge_load_vecs(vec, a, FOLD);
  __syncthreads();
  const int l = lane_id(), j = l & 15, q = l >> 4, wv = wave_id();
  float *mt = tiles + wv * (16 * TS + 64);
  float *xt = mt + 16 * TS;
  const int wave = global_wave_id(), nwaves = (gridDim.x * blockDim.x) >> 6;
  const bool mean = !(a.flags & FASTEGNN_F_COORDS_SUM);
  FE_T0()
  // this wave's share: a contiguous run of whole rows holding ~E/nwaves edges (chunk_row marks the row
  // boundary nearest to every CHUNK_EDGES-th edge)
  const int c0 = (int)((long)wave * a.n_chunks / nwaves), c1 = (int)((long)(wave + 1) * a.n_chunks / nwaves);
  {
    const int r0 = a.chunk_row[c0], r1 = a.chunk_row[c1];
    if (r0 < r1) {
      const int e0 = a.rowptr[r0], e1 = a.rowptr[r1];
      int cur = -1;
      float acc = 0.f, accx = 0.f;
      FE_T(7)   // chunk bookkeeping
      int cnt = 0;   // edges of the current row seen so far == its in-degree at flush time (rows never straddle waves)
      auto flush = [&]() {
        const float inv = rcp_f((float)cnt);
        if constexpr (AGGM) a.aggm[(size_t)cur * H + l] = acc * (FOLD ? inv * LN2_F : inv);
        if (l < 3) a.aggx[(size_t)cur * 3 + l] = mean ? accx * inv : accx;
      };
      // rows without edges inside this wave's range get their zeros here (no memset of aggm / aggx ahead of the kernel):
      // the wave owns the rows [r0, r1) and writes each of them exactly once
      auto zero_rows = [&](int ra, int rb) {
        for (int r = ra; r < rb; ++r) {
          if constexpr (AGGM) a.aggm[(size_t)r * H + l] = 0.f;
          if (l < 3) a.aggx[(size_t)r * 3 + l] = 0.f;
        }
      };
      EdgeIdx cur_i, nxt_i;
      if (e0 < e1) edge_load_idx(a, min(e0 + j, e1 - 1), cur_i);
      for (int base = e0; base < e1; base += 16) {
        const int nvalid = min(16, e1 - base);
        nxt_i = cur_i;
        if (base + 16 < e1) edge_load_idx(a, min(base + 16 + j, e1 - 1), nxt_i);   // next tile's indices in flight
        EdgeFwdState S;
        Vec pre;
        edge_tile_forward<false, MODE>(a, img, vec, cur_i, q, S, pre FE_TA);
        cur_i = nxt_i;
        if constexpr (AGGM) tile_store(mt, j, q, S.m);
        if (q == 0) {
          xt[j * 4 + 0] = S.dn[0] * S.s;
          xt[j * 4 + 1] = S.dn[1] * S.s;
          xt[j * 4 + 2] = S.dn[2] * S.s;
        }
        __builtin_amdgcn_wave_barrier();
        FE_T(5)   // transpose tile to LDS
        // hidden-on-lane column of the tile: all 16 LDS reads issued up front, the row-boundary walk
        // below then runs on registers and scalar compares only
        float mv[16], xv[16];
#pragma unroll
        for (int ee = 0; ee < 16; ++ee) {
          if constexpr (AGGM) mv[ee] = mt[ee * TS + l];
          xv[ee] = xt[ee * 4 + (l & 3)];
        }
        const int rowv = S.row;
        // where the row changes inside the tile: ONE lane compare with the lane below (DPP) and a ballot instead of sixteen
        // v_readlane + scalar compares; the row id itself is read only at a change (~2 per tile at degree 19)
        const int prevrow = __builtin_amdgcn_update_dpp(rowv, rowv, 0x111, 0xf, 0xf, false);   // row_shr:1 (lane 0 of a row keeps its own)
        const unsigned long long chg = __builtin_amdgcn_ballot_w64(j == 0 ? rowv != cur : rowv != prevrow);
        const unsigned starts = (unsigned)chg & 0xffffu;      // lanes 0..15 (q = 0): one bit per edge of the tile
#pragma unroll
        for (int ee = 0; ee < 16; ++ee) {
          if (ee < nvalid) {
            if ((starts >> ee) & 1u) {
              const int rw = __builtin_amdgcn_readlane(rowv, ee);
              if (cur >= 0) flush();
              zero_rows(cur >= 0 ? cur + 1 : r0, rw);
              cur = rw;
              acc = 0.f;
              accx = 0.f;
              cnt = 0;
            }
            if constexpr (AGGM) acc += mv[ee];
            accx += xv[ee];
            ++cnt;
          }
        }
        __builtin_amdgcn_wave_barrier();
        FE_T(6)   // row-segmented reduction
      }
      if (cur >= 0) flush();
      zero_rows(cur >= 0 ? cur + 1 : r0, r1);
    }
  }
  FE_TEND()
}

int edge_forward(const fastegnn_layer_t *L, hipStream_t st, bool aggm) {
  FE_REQUIRE(L->P && L->QX && L->aggm && L->aggx && L->wpack, "edge_forward: null buffer");
  FE_REQUIRE(L->ea <= 7, "edge_forward: edge_attr_nf > 7 unsupported");
  FE_REQUIRE(!has(L, FASTEGNN_F_ATTENTION) || (L->params[FASTEGNN_P_ATT_W] && L->params[FASTEGNN_P_ATT_B]),
             "edge_forward: attention params null");
  const fastegnn_graph_t &g = L->graph;
  if (g.n_edges == 0 || L->N == 0) {   // nothing to walk: the aggregates are zero (with edges the kernel writes every row)
    if (aggm) (void)hipMemsetAsync(L->aggm, 0, (size_t)L->N * H * sizeof(float), st);
    (void)hipMemsetAsync(L->aggx, 0, (size_t)L->N * 3 * sizeof(float), st);
    return check_launch("edge_forward(memset)");
  }
  FE_REQUIRE(g.rowptr && g.erow && g.col && g.chunk_row && (L->ea == 0 || L->ea_sorted), "edge_forward: null graph");
  EdgeArgs a = make_edge_args(L);
  FE_REQUIRE((size_t)L->N * QXLD < (1u << 30) && (size_t)g.n_src * QXLD < (1u << 30) && (size_t)g.n_edges * 8 < (1u << 30),
             "edge_forward: tables exceed the 32-bit offset range of the gather path");
  // one workgroup per CU once there are >= 256 x 16 row chunks; small graphs spread their chunks (32 edges) over as
  // many waves as there are chunks instead of serialising them in a few workgroups (the N-body mini-batches)
  int grid = cdiv(g.n_chunks, EDGE_FWD_WAVES);
  if (grid > 256) grid = 256;
  const size_t lds = (EDGE_FWD_IMG_FLOATS + EV_COUNT * H + EDGE_FWD_WAVES * (16 * TS + 64)) * sizeof(float);
  {
    ProfScope _ps_edge_fwd_kernel(K_EDGE_FWD, st);
    const dim3 g3(grid), b3(64 * EDGE_FWD_WAVES);
    if (!aggm) {
      if (has(L, FASTEGNN_F_BF16)) hipLaunchKernelGGL((edge_fwd_kernel<GM_BF16, false>), g3, b3, lds, st, a, L->C);
      else hipLaunchKernelGGL((edge_fwd_kernel<GM_EDGE_FWD, false>), g3, b3, lds, st, a, L->C);
    }
    else if (has(L, FASTEGNN_F_BF16)) hipLaunchKernelGGL(edge_fwd_kernel<GM_BF16>, g3, b3, lds, st, a, L->C);
    else hipLaunchKernelGGL(edge_fwd_kernel<GM_EDGE_FWD>, g3, b3, lds, st, a, L->C);
  }
  return check_launch("edge_fwd_kernel");
}

// =====================================================================================
// S4 virt: edge_mode_virtual (:111-119), virtual part of coord_model_vel (:136-142),
// coord_model_virtual (:146-150), node_model (:153-166) and the pools of node_model_virtual
// (:170), fused.  A wave owns 16 nodes and loops over the C virtual channels; the K = H*C
// contraction of node_mlp.0 accumulates in MFMA registers, v [N,C,H] never reaches HBM.
// =====================================================================================

// LDS: images V2, WXV0, WXX0 | two W3c[c] stage slots | vectors | pools | Bc / Z rows of the graph in flight
}  // namespace fe
#include "virt_fwd.h"   // VIRT_FWD_IMG_FLOATS, virt_fwd_lds_bytes, virt_fwd_kernel<MODE, PAIR>
namespace fe {

// pools_zeroed: poolV / poolX were zeroed on this stream already (the layer call: graph_pre_fwd_kernel)
int virt_forward(const fastegnn_layer_t *L, hipStream_t st, bool pools_zeroed) {
  const bool egnn = has(L, FASTEGNN_F_EGNN);
  // h_out == NULL && HvT_out == NULL (FastEGNN wiring): the node update of this layer is not wanted -- npre and poolV are not written
  // and may be null as well (include/fastegnn_hip.h)
  const bool node = egnn || has(L, FASTEGNN_F_RF) || L->h_out;
  FE_REQUIRE(node || !L->HvT_out, "virt_forward: h_out is null and HvT_out is not (both null: no node update; otherwise neither)");
  FE_REQUIRE(L->h && L->A && L->x && L->vel && L->aggm && L->aggx && L->svel && (!node || (L->npre && L->h_out)) && L->x_out &&
                 L->batch && L->wpack,
             "virt_forward: null buffer");
  FE_REQUIRE(egnn ? L->C == 0 : (L->Bc && L->Z && (!node || L->poolV) && L->poolX && L->C >= 1 && L->C <= 64),
             "virt_forward: virtual_channels must be in [1,64] (0 with FASTEGNN_F_EGNN) and the virtual buffers non-null");
  FE_REQUIRE(L->na == 0 || L->node_attr, "virt_forward: node_attr null");
  if (L->C > 0 && !pools_zeroed) {
    if (node) (void)hipMemsetAsync(L->poolV, 0, (size_t)L->B * L->C * H * sizeof(float), st);
    (void)hipMemsetAsync(L->poolX, 0, (size_t)L->B * 3 * L->C * sizeof(float), st);
  }
  if (L->N == 0) return check_launch("virt_forward(memset)");
  VirtArgs a = make_virt_args(L);
  // two waves per tile (PAIR) while that puts every tile of the input into ONE step of some workgroup: N <= 256 x 4 tiles
  static const bool pair_off = getenv("FASTEGNN_VIRT_FWD_PAIR") && atoi(getenv("FASTEGNN_VIRT_FWD_PAIR")) == 0;   // (A/B switch)
  const bool pair = GM_VIRT_FWD == GM_F16 && !pair_off && !has(L, FASTEGNN_F_BF16) && !has(L, FASTEGNN_F_RF) && !egnn && L->C >= 2 &&
                    cdiv(L->N, 16 * (VIRT_WAVES / 2)) <= 256 && virt_fwd_lds_bytes(L->C, true) <= 160 * 1024;
  const int ntg = cdiv(L->N, 16 * (pair ? VIRT_WAVES / 2 : VIRT_WAVES));
  int grid = ntg < 256 ? ntg : 256;   // one workgroup per CU (LDS), each with an equal share of the tiles
  {
    ProfScope _ps_virt_fwd_kernel(K_VIRT_FWD, st);
    const size_t lds = virt_fwd_lds_bytes(L->C, pair);
    if (!node) {
      if (has(L, FASTEGNN_F_BF16)) hipLaunchKernelGGL((virt_fwd_kernel<GM_BF16, false, false>), dim3(grid), dim3(64 * VIRT_WAVES), lds, st, a);
      else if (pair) launch_virt_fwd_pair_nonode(a, grid, lds, st);
      else hipLaunchKernelGGL((virt_fwd_kernel<GM_VIRT_FWD, false, false>), dim3(grid), dim3(64 * VIRT_WAVES), lds, st, a);
    }
    else if (has(L, FASTEGNN_F_BF16)) hipLaunchKernelGGL(virt_fwd_kernel<GM_BF16>, dim3(grid), dim3(64 * VIRT_WAVES), lds, st, a);
    else if (pair) launch_virt_fwd_pair(a, grid, lds, st);   // (virt_fwd_pair.hip: its own translation unit, see virt_fwd.h)
    else hipLaunchKernelGGL(virt_fwd_kernel<GM_VIRT_FWD>, dim3(grid), dim3(64 * VIRT_WAVES), lds, st, a);
  }
  return check_launch("virt_fwd_kernel");
}

// =====================================================================================
// S5 graph_post: coord_model_virtual's mean + residual (:148-149) and node_model_virtual
// (:168-177) on the B*C (graph, channel) rows.
// =====================================================================================
struct GraphPostArgs {
  const float *xsum, *Z, *HvT, *poolV, *poolX, *wpack, *b5, *b6;
  float *Z_out, *HvT_out;
  int B, C, flags;
  float act_param = 0.f;
};
__global__ __launch_bounds__(256) void graph_post_fwd_kernel(GraphPostArgs a) {
  const bool bf = a.flags & FASTEGNN_F_BF16;   // bf16 operand mode: activations rounded, images hold rounded weights
  // One workgroup per tile of 16 rows, the 64 output features of each product dealt to its four waves (gemm64_block).  With
  // B*C = 16 rows the stage is ONE tile: a single wave running the products one after the other, each behind its own fragment
  // loads from global memory, was the whole launch.  The waves exchange the one vector the next product contracts over (u5)
  // through LDS.
  __shared__ __attribute__((aligned(16))) float xt[16 * TS];
  const int l = lane_id(), j = l & 15, q = l >> 4, w = wave_id();
  const int M = a.B * a.C, ntiles = (M + 15) >> 4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.B * 3 * a.C; i += gridDim.x * blockDim.x) {
    const int b = i / (3 * a.C);
    a.Z_out[i] = a.Z[i] + a.poolX[i] / fmaxf(a.xsum[b * 4 + 3], 1.f);
  }
  if (a.flags & FASTEGNN_F_RF) {   // FastRF.py:186: the virtual node features pass through
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M * H; i += gridDim.x * blockDim.x) a.HvT_out[i] = a.HvT[i];
    return;
  }
  f32x4 f5a[4], f5b[4], f6[4];
  gemm64_frags(a.wpack + (size_t)I_W5A * IMG, w, f5a);
  gemm64_frags(a.wpack + (size_t)I_W5B * IMG, w, f5b);
  gemm64_frags(a.wpack + (size_t)I_W6 * IMG, w, f6);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m = tile * 16 + j;
    const bool valid = m < M;
    const int mc = valid ? m : M - 1;
    const int b = mc / a.C;
    const float inv = 1.0f / fmaxf(a.xsum[b * 4 + 3], 1.f);
    const Vec hv = vload_row(a.HvT + (size_t)mc * H, q);
    const Vec pm = vscale(vload_row(a.poolV + (size_t)mc * H, q), inv);
    f32x4 z5 = vload_block(a.b5, w, q);
    gemm64_block(f5a, bf ? vround(hv) : hv, z5);
    gemm64_block(f5b, bf ? vround(pm) : pm, z5);
    vstore_block(xt + j * TS, w, q, vblock(z5, [&](const Vec &v) { return vsilu(v FE_ACT(a)); }));
    __syncthreads();
    const Vec u5 = vload_row(xt + j * TS, q);
    f32x4 out = vload_block(a.b6, w, q);
    gemm64_block(f6, bf ? vround(u5) : u5, out);
    if (a.flags & FASTEGNN_F_RESIDUAL) out += vload_block(a.HvT + (size_t)mc * H, w, q);
    if (valid) vstore_block(a.HvT_out + (size_t)m * H, w, q, out);
    __syncthreads();   // xt is rewritten by the next tile
  }
}
// HvT_out == NULL && h_out == NULL: node_model_virtual is not wanted -- the coordinate part alone (the same expression as above)
__global__ __launch_bounds__(256) void graph_post_fwd_coords_kernel(const float *xsum, const float *Z, const float *poolX, float *Z_out,
                                                                    int B, int C) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * 3 * C; i += gridDim.x * blockDim.x) {
    const int b = i / (3 * C);
    Z_out[i] = Z[i] + poolX[i] / fmaxf(xsum[b * 4 + 3], 1.f);
  }
}
int graph_post_forward(const fastegnn_layer_t *L, hipStream_t st) {
  if (!L->HvT_out && !has(L, FASTEGNN_F_RF)) {
    FE_REQUIRE(!L->h_out, "graph_post_forward: HvT_out is null and h_out is not (both null: no node update; otherwise neither)");
    FE_REQUIRE(L->xsum && L->Z && L->poolX && L->Z_out, "graph_post_forward: null buffer");
    int grid = cdiv((long)L->B * 3 * L->C, 256);
    if (grid > 256) grid = 256;
    if (grid < 1) grid = 1;
    { ProfScope _ps_graph_post_fwd_kernel(K_GRAPH_POST_FWD, st); hipLaunchKernelGGL(graph_post_fwd_coords_kernel, dim3(grid), dim3(256), 0, st, L->xsum, L->Z, L->poolX, L->Z_out, L->B, L->C); }
    return check_launch("graph_post_fwd_coords_kernel");
  }
  FE_REQUIRE(L->xsum && L->Z && L->HvT && L->poolV && L->poolX && L->Z_out && L->HvT_out && L->wpack,
             "graph_post_forward: null buffer");
  GraphPostArgs a{L->xsum, L->Z, L->HvT, L->poolV, L->poolX, L->wpack, L->params[FASTEGNN_P_NODEV0_B],
                  L->params[FASTEGNN_P_NODEV2_B], L->Z_out, L->HvT_out, L->B, L->C, L->flags, L->act_param};
  int grid = cdiv((long)L->B * L->C, 16);   // one workgroup per tile
  if (grid > 256) grid = 256;
  if (grid < 1) grid = 1;
  { ProfScope _ps_graph_post_fwd_kernel(K_GRAPH_POST_FWD, st); hipLaunchKernelGGL(graph_post_fwd_kernel, dim3(grid), dim3(256), 0, st, a); }
  return check_launch("graph_post_fwd_kernel");
}

}  // namespace fe

#ifdef FE_STAMP_VF
extern "C" int fastegnn_debug_read_stamps_vf(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(fe::g_vf_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(fe::g_vf_stamps), z, sizeof(z));
  }
  return 0;
}
#endif
#ifdef FE_STAMP
extern "C" int fastegnn_debug_read_stamps(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(fe::g_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(fe::g_stamps), z, sizeof(z));
  }
  return 0;
}
#endif

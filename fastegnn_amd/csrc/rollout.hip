// The state update of a ROLLOUT (fastegnn_amd/rollout.py): a trained model's prediction is fed back in as the next step's input and
// scored against the trajectory's own frame.  Between two forwards the state is advanced by TWO launches whatever the batch size:
//   advance  one launch over the N nodes: vel = (x_new - x_cur) * (1 / delta_t), node_feat[:,0] = |vel| by traj.hip's rule, loc = x_new,
//            optionally record[k] = x_new; a non-finite component keeps x_cur, gets vel 0 and sets a flag word
//   graph    one workgroup per graph: loc_mean [B,3,C] of the new loc by traj.hip's mean rule and, in the same pass, the step's squared
//            error against the truth frame, sse[b], in fp64 in the same order
// and once per rollout
//   plan     truth_rows [steps,B]: the first row in pos of the truth frame of step k for slot b, -1 beyond the trajectory's end
// A rollout over a dataset with a rigid motion per sample scores with `graph_moved`: the same launch, the truth rows moved by the slot's
// motion in fp32 (the rule of traj.hip's moved gather) before the fp64 difference.
// No atomics, no workspace, nothing read back, 64-bit offsets.  Sample ids, trajectory and frame numbers are clamped as traj.hip's plan
// clamps them; a graph whose node range does not lie inside [0, N) or whose truth rows do not lie inside pos is skipped: nothing is read
// outside the tables and nothing is written beyond the sizes the host gave, whatever the device arrays hold.
#include "kernels.h"

namespace fe {

constexpr int RO_THREADS = 256;
constexpr int RO_MAX_BLOCKS = 2048;        // beyond that the workgroups stride
constexpr int RO_GRAPH_THREADS = 256;      // part of the summation order of loc_mean and sse (TJ_MEAN_THREADS of traj.hip): keep equal

__device__ __forceinline__ long long ro_clamp(long long v, long long n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---- plan ----
__global__ __launch_bounds__(RO_THREADS) void rollout_plan_kernel(const int64_t *__restrict__ ids, int B, const int64_t *__restrict__ samples,
                                                                   long long n_samples, const int64_t *__restrict__ row0,
                                                                   const int64_t *__restrict__ n_of, const int64_t *__restrict__ T_of,
                                                                   int n_traj, int delta_t, int steps, int64_t *__restrict__ truth_rows) {
  const long long total = (long long)steps * B, stride = (long long)gridDim.x * RO_THREADS;
  for (long long i = (long long)blockIdx.x * RO_THREADS + threadIdx.x; i < total; i += stride) {
    const int b = (int)(i % B);
    const long long k = i / B;
    const long long sid = ro_clamp(ids[b], n_samples);
    const long long tr = ro_clamp(samples[2 * sid], n_traj);
    const long long n = n_of[tr] < 0 ? 0 : n_of[tr];
    const long long T = T_of[tr];
    const long long last = T >= 1 ? T - 1 : 0;
    const long long f = ro_clamp(samples[2 * sid + 1], last + 1);
    const long long frame = f + (k + 1) * (long long)delta_t;   // (steps and delta_t are 32-bit: no wrap)
    truth_rows[i] = frame < T ? row0[tr] + frame * n : -1;
  }
}

// ---- advance ----
__device__ __forceinline__ bool ro_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// |v| by traj.hip's tj_speed: every operation rounded to fp32 by itself, a correctly rounded root
__device__ __forceinline__ float ro_speed(float vx, float vy, float vz) {
#pragma clang fp contract(off)
  const float xx = vx * vx;
  const float yy = vy * vy;
  const float zz = vz * vz;
  const float s = (xx + yy) + zz;
  return sqrtf(s);
}

// one subtraction, then one multiplication, each rounded by itself
__device__ __forceinline__ float ro_vel(float x_new, float x_cur, float inv_dt) {
#pragma clang fp contract(off)
  const float d = x_new - x_cur;
  return d * inv_dt;
}

// One node per lane, tail masked.  `flag` gets a plain store of the constant 1 from one lane of every wave that saw a non-finite
// component (check_finite_kernel's way: the word may be host-mapped).
__global__ __launch_bounds__(RO_THREADS) void rollout_advance_kernel(const float *__restrict__ x_new, long long N, float inv_dt,
                                                                      float *__restrict__ loc, float *__restrict__ vel,
                                                                      float *__restrict__ node_feat, float *__restrict__ record,
                                                                      volatile int *flag) {
  bool bad = false;
  const long long stride = (long long)gridDim.x * RO_THREADS;
  for (long long e = (long long)blockIdx.x * RO_THREADS + threadIdx.x; e < N; e += stride) {
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float xn = x_new[e * 3 + k], xc = loc[e * 3 + k];
      const bool ok = ro_finite(xn);
      bad |= !ok;
      v[k] = ok ? ro_vel(xn, xc, inv_dt) : 0.0f;
      if (record) record[e * 3 + k] = xn;
      loc[e * 3 + k] = ok ? xn : xc;
      vel[e * 3 + k] = v[k];
    }
    node_feat[e * 2] = ro_speed(v[0], v[1], v[2]);
  }
  if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0) {
    *flag = 1;
    __threadfence_system();
  }
}

// ---- graph: loc_mean of the new state and the step's squared error, one pass over the graph's nodes ----
// Thread t takes nodes t, t + 256, ... in ascending order; the 256 partial sums are added pairwise over strides 128, 64, .. 1
// (traj_mean_kernel's order: loc_mean has the bits fastegnn_traj_mean gives on the same rows).  A node's error term is
// (dx*dx + dy*dy) + dz*dz in fp64, every operation rounded by itself.
__device__ __forceinline__ double ro_sq3(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  const double xx = dx * dx;
  const double yy = dy * dy;
  const double zz = dz * dz;
  return (xx + yy) + zz;
}

// The rigid motion of include/fastegnn_hip.h ("rigid motions"), traj.hip's tj_move: q[j] = ((p[0]*R[0][j] + p[1]*R[1][j]) + p[2]*R[2][j]),
// every operation rounded to fp32 by itself, then + t[j] when `shift` (no addition at all without it).  m: R row-major, then t.
__device__ __forceinline__ void ro_move(const float (&m)[12], const float (&p)[3], bool shift, float (&q)[3]) {
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

// MOVED: the truth row is moved by graph b's motion (motion row b, b = the workgroup: below B) in fp32 before the fp64 difference
template <bool MOVED>
__global__ __launch_bounds__(RO_GRAPH_THREADS) void rollout_graph_kernel(const int64_t *__restrict__ ptr, const float *__restrict__ loc,
                                                                          const float *__restrict__ x_new, long long N,
                                                                          const float *__restrict__ pos, long long pos_rows,
                                                                          const int64_t *__restrict__ truth_rows, int C,
                                                                          float *__restrict__ loc_mean, double *__restrict__ sse,
                                                                          const float *__restrict__ motion, int has_t) {
  __shared__ double part[4][RO_GRAPH_THREADS];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long at = ptr[b];
  long long n = ptr[b + 1] - at;
  if (n < 0 || at < 0 || at > N - n) n = 0;   // (n <= N or the last test fails: no wrap)
  const bool score = sse != nullptr;
  long long r = score ? truth_rows[b] : -1;
  if (r < 0 || r > pos_rows - n) r = -1;      // no truth frame, or its rows are not inside pos: no score
  float m[12] = {};
  if (MOVED && r >= 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = motion[(long long)b * 12 + k];
  }
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long i = t; i < n; i += RO_GRAPH_THREADS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += (double)loc[(at + i) * 3 + k];
    if (r >= 0) {
      float p[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = pos[(r + i) * 3 + k];
      if (MOVED) {
        float q[3];
        ro_move(m, p, has_t != 0, q);
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = q[k];
      }
      double d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] = (double)x_new[(at + i) * 3 + k] - (double)p[k];
      s[3] += ro_sq3(d[0], d[1], d[2]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) part[k][t] = s[k];
  __syncthreads();
  for (int off = RO_GRAPH_THREADS / 2; off >= 1; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int k = 0; k < 4; ++k) part[k][t] += part[k][t + off];
    }
    __syncthreads();
  }
  for (int j = t; j < 3 * C; j += RO_GRAPH_THREADS)
    loc_mean[(long long)b * 3 * C + j] = n > 0 ? (float)(part[j / C][0] / (double)n) : 0.0f;
  if (score && t == 0) sse[b] = (r >= 0 && n > 0) ? part[3][0] : __builtin_nan("");
}

}  // namespace fe

using namespace fe;

extern "C" {

int fastegnn_rollout_plan(const int64_t *ids, int32_t B, const int64_t *samples, int64_t n_samples, const int64_t *traj_row0,
                          const int64_t *traj_n, const int64_t *traj_T, int32_t n_traj, int32_t delta_t, int32_t steps,
                          int64_t *truth_rows, void *stream) {
  FE_REQUIRE(B >= 0, "rollout_plan: B < 0");
  FE_REQUIRE(steps >= 1, "rollout_plan: steps < 1");
  FE_REQUIRE(n_samples >= 1 && n_traj >= 1, "rollout_plan: the dataset holds no sample or no trajectory");
  FE_REQUIRE(delta_t >= 1, "rollout_plan: delta_t < 1");
  if (B == 0) return FASTEGNN_OK;
  FE_REQUIRE(ids && samples && traj_row0 && traj_n && traj_T && truth_rows, "rollout_plan: null pointer");
  const long long blocks = ((long long)steps * B + RO_THREADS - 1) / RO_THREADS;
  const int grid = (int)(blocks < RO_MAX_BLOCKS ? blocks : RO_MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  hipLaunchKernelGGL(rollout_plan_kernel, dim3(grid), dim3(RO_THREADS), 0, st, ids, B, samples, (long long)n_samples, traj_row0, traj_n,
                     traj_T, n_traj, delta_t, steps, truth_rows);
  return check_launch("rollout_plan");
}

int fastegnn_rollout_advance(const float *x_new, int64_t n_nodes, int32_t delta_t, float *loc, float *vel, float *node_feat,
                             float *record, int32_t *flag, void *stream) {
  FE_REQUIRE(n_nodes >= 0, "rollout_advance: negative size");
  FE_REQUIRE(delta_t >= 1, "rollout_advance: delta_t < 1");
  FE_REQUIRE(flag, "rollout_advance: null flag word");
  if (n_nodes == 0) return FASTEGNN_OK;
  FE_REQUIRE(x_new && loc && vel && node_feat, "rollout_advance: null pointer");
  const long long blocks = (n_nodes + RO_THREADS - 1) / RO_THREADS;
  const int grid = (int)(blocks < RO_MAX_BLOCKS ? blocks : RO_MAX_BLOCKS);
  const float inv_dt = 1.0f / (float)delta_t;
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  hipLaunchKernelGGL(rollout_advance_kernel, dim3(grid), dim3(RO_THREADS), 0, st, x_new, (long long)n_nodes, inv_dt, loc, vel, node_feat,
                     record, flag);
  return check_launch("rollout_advance");
}

int fastegnn_rollout_graph(const int64_t *ptr, int32_t B, const float *loc, const float *x_new, int64_t n_nodes, const float *pos,
                           int64_t pos_rows, const int64_t *truth_rows, int32_t C, float *loc_mean, double *sse, void *stream) {
  FE_REQUIRE(C >= 1 && C <= (1 << 20), "rollout_graph: C out of range (1 .. 2^20)");
  FE_REQUIRE(B >= 0 && n_nodes >= 0 && pos_rows >= 0, "rollout_graph: negative size");
  if (B == 0) return FASTEGNN_OK;
  FE_REQUIRE(ptr && loc_mean && (loc || n_nodes == 0), "rollout_graph: null pointer");
  FE_REQUIRE(!sse || (x_new && pos && truth_rows), "rollout_graph: a score needs x_new, pos and truth_rows");
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  hipLaunchKernelGGL(rollout_graph_kernel<false>, dim3(B), dim3(RO_GRAPH_THREADS), 0, st, ptr, loc, x_new, (long long)n_nodes, pos,
                     (long long)pos_rows, truth_rows, C, loc_mean, sse, (const float *)nullptr, 0);
  return check_launch("rollout_graph");
}

int fastegnn_rollout_graph_moved(const int64_t *ptr, int32_t B, const float *loc, const float *x_new, int64_t n_nodes, const float *pos,
                                 int64_t pos_rows, const int64_t *truth_rows, int32_t C, float *loc_mean, double *sse,
                                 const float *motion, int32_t has_t, void *stream) {
  FE_REQUIRE(C >= 1 && C <= (1 << 20), "rollout_graph_moved: C out of range (1 .. 2^20)");
  FE_REQUIRE(B >= 0 && n_nodes >= 0 && pos_rows >= 0, "rollout_graph_moved: negative size");
  if (B == 0) return FASTEGNN_OK;
  FE_REQUIRE(ptr && loc_mean && (loc || n_nodes == 0), "rollout_graph_moved: null pointer");
  FE_REQUIRE(!sse || (x_new && pos && truth_rows), "rollout_graph_moved: a score needs x_new, pos and truth_rows");
  FE_REQUIRE(!sse || motion, "rollout_graph_moved: a score needs the motion table");
  hipStream_t st = (hipStream_t)stream;
  ProfScope _ps(K_MISC, st);
  hipLaunchKernelGGL(rollout_graph_kernel<true>, dim3(B), dim3(RO_GRAPH_THREADS), 0, st, ptr, loc, x_new, (long long)n_nodes, pos,
                     (long long)pos_rows, truth_rows, C, loc_mean, sse, motion, has_t);
  return check_launch("rollout_graph_moved");
}

}  // extern "C"

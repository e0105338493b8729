// Training-step closure on device: the caller-side pieces of the reference
// harness that bracket the hot path in utils/train.py -- edge_attr augmentation (:41-43), MSE + MMD loss
// with its gradient (:104-165, kernel() :17-20) and Adam (main_nbody.py:137) -- so that one training
// iteration never leaves the GPU.
#include <vector>

#include "kernels.h"
#include "keyed_perm.h"

namespace fe {

// out[e] = [edge_attr[e,:], ||loc[row_e] - loc[col_e]||]        (utils/train.py:41-43)
__global__ void augment_edge_attr_kernel(const int64_t *ei, const float *loc, const float *ea, int E, int k, float *out) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const long r = ei[e], c = ei[(size_t)E + e];
  float d0 = loc[r * 3] - loc[c * 3], d1 = loc[r * 3 + 1] - loc[c * 3 + 1], d2 = loc[r * 3 + 2] - loc[c * 3 + 2];
  for (int a = 0; a < k; ++a) out[(size_t)e * (k + 1) + a] = ea[(size_t)e * k + a];
  out[(size_t)e * (k + 1) + k] = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
}

// MSE part: loss[1] (and loss[0]) += sum (p-t)^2 / (3N);  g_loc = 2 (p-t) / (3N)
__global__ __launch_bounds__(256) void loss_mse_kernel(const float *pred, const float *tgt, long n3, float *g_loc, float *loss) {
  __shared__ float red[4];
  const float inv = 1.0f / (float)n3;
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (long)gridDim.x * 256) {
    const float d = pred[i] - tgt[i];
    s += d * d;
    g_loc[i] = 2.f * d * inv;
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = (red[0] + red[1] + red[2] + red[3]) * inv;
    atomicAdd(&loss[0], v);
    atomicAdd(&loss[1], v);
  }
}

// MMD part, one workgroup per graph: l_vv = sum_{c,c'} k(V_c,V_c') / (B C^2), l_rv = 2 sum_{s,c} k(R_s,V_c) / (B S C),
// k(x,y) = exp(-||x-y|| / (2 sigma^2));  loss[0] += weight (l_vv - l_rv);  gradients into g_vloc [B,3,C] and g_loc.
// cnt (may be null: every row full): row b of samp holds cnt[b] <= S valid entries and only those are staged, paired and scattered;
// l_rv keeps the divisor B S C (utils/train.py:142).  The LDS layout stays the one of S rows.
__global__ __launch_bounds__(256) void loss_mmd_kernel(const float *pred, const float *vloc, const int32_t *samp,
                                                       const int32_t *cnt, int B, int C, int S, float sigma, float weight,
                                                       float *g_loc, float *g_vloc, float *loss) {
  extern __shared__ float sm[];
  float *V = sm;             // [C][3]
  float *gV = sm + 3 * C;    // [C][3]
  float *R = gV + 3 * C;     // [S][3]
  float *gR = R + 3 * S;     // [S][3]
  __shared__ float acc;
  const int b = blockIdx.x;
  int Sb = cnt ? cnt[b] : S;
  Sb = Sb < 0 ? 0 : (Sb > S ? S : Sb);   // documented in the header: the staging below must stay inside the S rows of LDS
  const float i2s = 1.0f / (2.f * sigma * sigma);
  for (int i = threadIdx.x; i < 3 * C; i += 256) {
    int c = i / 3, k = i % 3;
    V[i] = vloc[((size_t)b * 3 + k) * C + c];
    gV[i] = 0.f;
  }
  for (int i = threadIdx.x; i < 3 * Sb; i += 256) {
    int s = i / 3, k = i % 3;
    R[i] = pred[(size_t)samp[b * S + s] * 3 + k];
    gR[i] = 0.f;
  }
  if (threadIdx.x == 0) acc = 0.f;
  __syncthreads();
  const float w_vv = weight / ((float)B * C * C), w_rv = -2.f * weight / ((float)B * S * C);
  float part = 0.f;
  for (int i = threadIdx.x; i < C * C + Sb * C; i += 256) {
    const bool vv = i < C * C;
    const int a = vv ? i / C : (i - C * C) / C, c = vv ? i % C : (i - C * C) % C;
    const float *xa = vv ? V + 3 * a : R + 3 * a;
    float *ga = vv ? gV + 3 * a : gR + 3 * a;
    const float d0 = xa[0] - V[3 * c], d1 = xa[1] - V[3 * c + 1], d2 = xa[2] - V[3 * c + 2];
    const float dist = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float kv = __expf(-dist * i2s);
    const float w = vv ? w_vv : w_rv;
    part += w * kv;
    if (dist > 0.f) {   // d/dx exp(-|x-y|/2s^2) = -k/(2s^2) (x-y)/|x-y|; zero at coincident points (cdist backward)
      const float f = -w * kv * i2s / dist;
      atomicAdd(&ga[0], f * d0); atomicAdd(&ga[1], f * d1); atomicAdd(&ga[2], f * d2);
      atomicAdd(&gV[3 * c], -f * d0); atomicAdd(&gV[3 * c + 1], -f * d1); atomicAdd(&gV[3 * c + 2], -f * d2);
    }
  }
  atomicAdd(&acc, part);
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&loss[0], acc);
  for (int i = threadIdx.x; i < 3 * C; i += 256) {
    int c = i / 3, k = i % 3;
    g_vloc[((size_t)b * 3 + k) * C + c] = gV[i];
  }
  for (int i = threadIdx.x; i < 3 * Sb; i += 256) {
    int s = i / 3, k = i % 3;
    atomicAdd(&g_loc[(size_t)samp[b * S + s] * 3 + k], gR[i]);
  }
}

// ---- the device-side MMD sample (fastegnn_mmd_sample; the permutation is defined in include/fastegnn_hip.h and lives in
// keyed_perm.h, which the packed stream's draw shares) ----
// One thread per entry (b, j), grid-stride; thread i < B also writes sample_count[i].  Reads rng and ptr, writes its own outputs:
// no atomics, and every workgroup sees the same counter because nothing in this launch writes it (mmd_advance_kernel does, behind).
__global__ __launch_bounds__(256) void mmd_sample_kernel(const int64_t *ptr, int B, int S, const uint64_t *rng, int32_t *nodes,
                                                         int32_t *count) {
  const long total = (long)B * S, stride = (long)gridDim.x * 256;
  const uint64_t gkey = perm_draw_key(rng[0], rng[1]);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total || i < B; i += stride) {
    if (i < B) {
      const int64_t n = ptr[i + 1] - ptr[i];
      count[i] = n < 0 ? 0 : (n < S ? (int32_t)n : S);
    }
    if (i >= total) continue;
    const int b = (int)(i / S), j = (int)(i % S);
    const int64_t p0 = ptr[b], n = ptr[b + 1] - p0;
    if (j >= n) { nodes[i] = -1; continue; }
    if (n <= S) { nodes[i] = (int32_t)(p0 + j); continue; }
    const uint64_t x = keyed_perm(gkey, (uint64_t)b, (uint64_t)n, (uint64_t)j);   // n > S >= 1 here
    nodes[i] = (int32_t)(p0 + (int64_t)x);
  }
}
__global__ void mmd_advance_kernel(uint64_t *rng) {
  if (blockIdx.x == 0 && threadIdx.x == 0) rng[1] += 1;
}

// fastegnn_loss_accumulate: a training step's (loss, mse) into the three fp64 words of an epoch (loss_eval_kernel's acc)
__global__ void loss_accumulate_kernel(const float *loss, const float *mse, int B, double *acc) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double b = (double)B;
    acc[0] += b * (double)mse[0];
    acc[1] += b * (double)loss[0];
    acc[2] += b;
  }
}

// torch.optim.Adam (no amsgrad; weight decay folded into the gradient), up to 24 tensors per launch.  Each tensor carries its
// own bias correction: torch keeps state['step'] per parameter and advances it only on steps where the parameter has a .grad
constexpr int ADAM_MAX = 24;
struct AdamArgs {
  float *p[ADAM_MAX], *m[ADAM_MAX], *v[ADAM_MAX];
  const float *g[ADAM_MAX];
  long n[ADAM_MAX];
  float lr_t[ADAM_MAX], inv_bc2_sqrt[ADAM_MAX];   // lr / (1 - b1^step), 1 / sqrt(1 - b2^step) of the tensor's own step
  int count;
  float b1, b2, omb1, omb2, eps, wd;   // omb = 1 - beta, rounded once from double (1.f - 0.999f is 1.3e-5 off 0.001)
};
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
  const int t = blockIdx.y;
  if (t >= a.count) return;
  float *p = a.p[t], *m = a.m[t], *v = a.v[t];
  const float *g = a.g[t];
  if (!g) return;   // torch.optim.Adam skips parameters whose .grad is None: no decay, no moment update, no step
  const float lr_t = a.lr_t[t], inv_bc2_sqrt = a.inv_bc2_sqrt[t];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n[t]; i += (long)gridDim.x * 256) {
    const float gi = g[i] + a.wd * p[i];
    const float mi = a.b1 * m[i] + a.omb1 * gi;
    const float vi = a.b2 * v[i] + a.omb2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) * inv_bc2_sqrt + a.eps);
  }
}

// workgroups per tensor of a multi-tensor launch over tensors of at most nmax elements (adam_kernel's grid)
inline int adam_grid_x(long nmax) {
  int gx = cdiv(nmax, 256 * 4);
  return gx > 64 ? 64 : (gx < 1 ? 1 : gx);
}

// sum over the 256 threads of a workgroup in a FIXED order (xor butterfly within each wave, then ((w0 + w1) + (w2 + w3))); valid in thread 0
__device__ inline double block_sum_f64(double s, double *red) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- sum of squares of all gradients, stage 1: workgroup (x, t) of a launch writes the fp64 sum of its grid-stride share of
// tensor t into its own slot part[t * gridDim.x + x] (0 for an absent gradient or a share that is empty).  fp32 x fp32 is exact in
// fp64 and nothing clamps or compares, so an Inf / NaN element reaches the slot.  No atomics: the slot layout and the order of every
// sum are fixed by the tensor sizes, which makes the result run-to-run identical.
struct SqnArgs {
  const float *g[ADAM_MAX];
  long n[ADAM_MAX];
  double *part;
};
__global__ __launch_bounds__(256) void grad_sqnorm_partial_kernel(SqnArgs a) {
  __shared__ double red[4];
  const int t = blockIdx.y;
  const float *g = a.g[t];
  double s = 0.0;
  if (g) {
    const long n = a.n[t], stride = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
    long done = 0;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {   // 16-byte loads over the aligned body, scalar tail
      const long n4 = n / 4;
      const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
      for (long i = first; i < n4; i += stride) {
        const f32x4 x = g4[i];
        s += (double)x[0] * (double)x[0];
        s += (double)x[1] * (double)x[1];
        s += (double)x[2] * (double)x[2];
        s += (double)x[3] * (double)x[3];
      }
      done = 4 * n4;
    }
    for (long i = done + first; i < n; i += stride) s += (double)g[i] * (double)g[i];
  }
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) a.part[(size_t)t * gridDim.x + blockIdx.x] = s;
}
// stage 2, ONE workgroup: thread i sums slots i, i + 256, ... in ascending order, then the fixed workgroup order
__global__ __launch_bounds__(256) void grad_sqnorm_final_kernel(const double *part, long n, double *out) {
  __shared__ double red[4];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += part[i];
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) *out = s;
}

// ---- the ORDERED training loss (fastegnn_loss_mse_mmd_ordered): the numbers and gradients of loss_mse_kernel + loss_mmd_kernel with no
// floating-point atomic; the order of every sum is fixed by (N, B, C, S) and the counts (include/fastegnn_hip.h states the rule).
// workspace: slot x < G of the MSE workgroup x, slot G + b of graph b (G = loss_ordered_mse_grid(N))
inline int loss_ordered_mse_grid(long n3) {
  long grid = cdiv(n3, 256 * 8);
  return grid > 1024 ? 1024 : (grid < 1 ? 1 : (int)grid);
}
// stage 1a: g_loc element-wise as loss_mse_kernel writes it; the squares (exact in fp64) summed per thread in grid-stride order, then
// block_sum_f64, into the workgroup's own slot
__global__ __launch_bounds__(256) void loss_mse_ordered_kernel(const float *pred, const float *tgt, long n3, float *g_loc, double *part) {
  __shared__ double red[4];
  const float inv = 1.0f / (float)n3;
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n3; i += (long)gridDim.x * 256) {
    const float d = pred[i] - tgt[i];
    s += (double)d * (double)d;
    g_loc[i] = 2.f * d * inv;
  }
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// stage 1b, one workgroup per graph, V and the Sb sampled rows in LDS.  Every gradient element has ONE owner that adds its terms in
// ascending index order in registers: thread c < C owns gV[c] (a = 0 .. C-1 of the vv term, both of its roles in pair (c, a) and
// (a, c); then s = 0 .. Sb-1 of the rv term), thread t owns gR[s] for s = t, t + 256, ... (c = 0 .. C-1).  The pair values are
// loss_mmd_kernel's fp32 ones; each owner evaluates the pairs it needs, so an rv pair is evaluated twice.  The loss terms (vv by the
// owner of c, rv by the owner of s) are summed in fp64: per thread in that order, then block_sum_f64, into slot b.
// g_loc: the rows of one graph's sample are distinct nodes and the graphs' samples are disjoint (the header's contract), so the
// plain read-add-write below, stream-ordered behind stage 1a, is the only add an address gets.
__global__ __launch_bounds__(256) void loss_mmd_ordered_kernel(const float *pred, const float *vloc, const int32_t *samp,
                                                               const int32_t *cnt, int B, int C, int S, float sigma, float weight,
                                                               float *g_loc, float *g_vloc, double *part) {
  extern __shared__ float sm[];
  __shared__ double red[4];
  float *V = sm;           // [C][3]
  float *R = sm + 3 * C;   // [S][3]
  const int b = blockIdx.x, t = threadIdx.x;
  int Sb = cnt ? cnt[b] : S;
  Sb = Sb < 0 ? 0 : (Sb > S ? S : Sb);   // as loss_mmd_kernel: the staging below must stay inside the S rows of LDS
  const float i2s = 1.0f / (2.f * sigma * sigma);
  for (int i = t; i < 3 * C; i += 256) {
    const int c = i / 3, k = i % 3;
    V[i] = vloc[((size_t)b * 3 + k) * C + c];
  }
  for (int i = t; i < 3 * Sb; i += 256) {
    const int s = i / 3, k = i % 3;
    R[i] = pred[(size_t)samp[(size_t)b * S + s] * 3 + k];
  }
  __syncthreads();
  const float w_vv = weight / ((float)B * C * C), w_rv = -2.f * weight / ((float)B * S * C);
  double lsum = 0.0;
  if (t < C) {
    const float v0 = V[3 * t], v1 = V[3 * t + 1], v2 = V[3 * t + 2];
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    for (int a = 0; a < C; ++a) {
      const float d0 = v0 - V[3 * a], d1 = v1 - V[3 * a + 1], d2 = v2 - V[3 * a + 2];
      const float dist = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
      const float kv = __expf(-dist * i2s);
      lsum += (double)(w_vv * kv);
      if (dist > 0.f) {   // zero subgradient at coincident points, as loss_mmd_kernel
        const float f = -w_vv * kv * i2s / dist;
        g0 += f * d0; g1 += f * d1; g2 += f * d2;   // pair (t, a): this thread's node in front
        g0 += f * d0; g1 += f * d1; g2 += f * d2;   // pair (a, t): the same value, -f * (V_a - V_t)
      }
    }
    for (int s = 0; s < Sb; ++s) {
      const float d0 = R[3 * s] - v0, d1 = R[3 * s + 1] - v1, d2 = R[3 * s + 2] - v2;
      const float dist = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
      if (dist > 0.f) {
        const float f = -w_rv * __expf(-dist * i2s) * i2s / dist;
        g0 -= f * d0; g1 -= f * d1; g2 -= f * d2;
      }
    }
    g_vloc[((size_t)b * 3 + 0) * C + t] = g0;
    g_vloc[((size_t)b * 3 + 1) * C + t] = g1;
    g_vloc[((size_t)b * 3 + 2) * C + t] = g2;
  }
  for (int s = t; s < Sb; s += 256) {
    const float r0 = R[3 * s], r1 = R[3 * s + 1], r2 = R[3 * s + 2];
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    for (int c = 0; c < C; ++c) {
      const float d0 = r0 - V[3 * c], d1 = r1 - V[3 * c + 1], d2 = r2 - V[3 * c + 2];
      const float dist = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
      const float kv = __expf(-dist * i2s);
      lsum += (double)(w_rv * kv);
      if (dist > 0.f) {
        const float f = -w_rv * kv * i2s / dist;
        g0 += f * d0; g1 += f * d1; g2 += f * d2;
      }
    }
    float *g = g_loc + (size_t)samp[(size_t)b * S + s] * 3;
    g[0] += g0; g[1] += g1; g[2] += g2;
  }
  lsum = block_sum_f64(lsum, red);
  if (t == 0) part[b] = lsum;
}
// stage 2, ONE workgroup (grad_sqnorm_final_kernel's scheme, once per term): thread i sums the slots i, i + 256, ... of the MSE
// workgroups, then of the graphs, each in ascending order, each followed by block_sum_f64
__global__ __launch_bounds__(256) void loss_ordered_final_kernel(const double *part, int G, int B, long n3, float *loss2) {
  __shared__ double red_mse[4], red_mmd[4];
  double s = 0.0, m = 0.0;
  for (int i = threadIdx.x; i < G; i += 256) s += part[i];
  for (int i = threadIdx.x; i < B; i += 256) m += part[G + i];
  s = block_sum_f64(s, red_mse);
  m = block_sum_f64(m, red_mmd);
  if (threadIdx.x == 0) {
    const double mse = s / (double)n3;
    loss2[0] = (float)(mse + m);
    loss2[1] = (float)mse;
  }
}

// ---- the loss of a forward-only epoch (fastegnn_loss_mse_mmd_eval): MSE and MSE + MMD of one batch, no gradients, added into three
// fp64 words on the device.  The entry point has no workspace argument, so the two-stage scheme above collapses to its second stage:
// ONE workgroup of 16 waves takes every sum in a fixed order (thread i owns elements i, i + 1024, ...; xor butterfly within a wave;
// the 16 wave sums in ascending order) -- no atomics, bit-identical from run to run.  It streams 24 bytes per node with 16-byte
// loads; the MMD part walks the graphs one after the other with the rows of the graph in LDS, as loss_mmd_kernel holds them.
constexpr int EVAL_THREADS = 1024;
__device__ inline double eval_block_sum(double s, double *red) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  __syncthreads();   // (the slots of an earlier sum have been read by everyone)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < EVAL_THREADS / 64; ++w) t += red[w];
  return t;   // the same value in every thread
}
__global__ __launch_bounds__(EVAL_THREADS) void loss_eval_kernel(const float *pred, const float *tgt, const float *vloc,
                                                                 const int32_t *samp, const int32_t *cnt, long n3, int B, int C, int S,
                                                                 float sigma, float weight, double *acc) {
  extern __shared__ float sm[];
  __shared__ double red[EVAL_THREADS / 64];
  float *V = sm;           // [C][3]
  float *R = sm + 3 * C;   // [S][3]
  // MSE: the difference and its square are exact in fp64
  double s = 0.0;
  long done = 0;
  if (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(tgt)) & 15) == 0) {   // 16-byte loads over the aligned body, scalar tail
    const long n4 = n3 / 4;
    const f32x4 *p4 = reinterpret_cast<const f32x4 *>(pred), *t4 = reinterpret_cast<const f32x4 *>(tgt);
    for (long i = threadIdx.x; i < n4; i += EVAL_THREADS) {
      const f32x4 x = p4[i], y = t4[i];
      for (int k = 0; k < 4; ++k) {
        const double d = (double)x[k] - (double)y[k];
        s += d * d;
      }
    }
    done = 4 * n4;
  }
  for (long i = done + threadIdx.x; i < n3; i += EVAL_THREADS) {
    const double d = (double)pred[i] - (double)tgt[i];
    s += d * d;
  }
  const double mse = eval_block_sum(s, red) / (double)n3;
  // MMD (samp null: not wanted): the kernel values are loss_mmd_kernel's fp32 ones, weighted and summed in fp64
  double mmd = 0.0;
  if (samp) {
    const float i2s = 1.0f / (2.f * sigma * sigma);
    const double w_vv = (double)weight / ((double)B * C * C), w_rv = -2.0 * (double)weight / ((double)B * S * C);
    double part = 0.0;
    for (int b = 0; b < B; ++b) {
      int Sb = cnt ? cnt[b] : S;
      Sb = Sb < 0 ? 0 : (Sb > S ? S : Sb);   // as loss_mmd_kernel: the staging below must stay inside the S rows of LDS
      __syncthreads();                       // the rows of the graph before are done with
      for (int i = threadIdx.x; i < 3 * C; i += EVAL_THREADS) {
        const int c = i / 3, k = i % 3;
        V[i] = vloc[((size_t)b * 3 + k) * C + c];
      }
      for (int i = threadIdx.x; i < 3 * Sb; i += EVAL_THREADS) {
        const int r = i / 3, k = i % 3;
        R[i] = pred[(size_t)samp[(size_t)b * S + r] * 3 + k];
      }
      __syncthreads();
      for (int i = threadIdx.x; i < C * C + Sb * C; i += EVAL_THREADS) {
        const bool vv = i < C * C;
        const int a = vv ? i / C : (i - C * C) / C, c = vv ? i % C : (i - C * C) % C;
        const float *xa = vv ? V + 3 * a : R + 3 * a;
        const float d0 = xa[0] - V[3 * c], d1 = xa[1] - V[3 * c + 1], d2 = xa[2] - V[3 * c + 2];
        const float kv = __expf(-sqrtf(d0 * d0 + d1 * d1 + d2 * d2) * i2s);
        part += (vv ? w_vv : w_rv) * (double)kv;
      }
    }
    mmd = eval_block_sum(part, red);
  }
  if (threadIdx.x == 0) {
    acc[0] += (double)B * mse;
    acc[1] += (double)B * (mse + mmd);
    acc[2] += (double)B;
  }
}

// ---- Adam with its per-step state on the device (fastegnn_adam_step_dev).
// The hazard: every workgroup of tensor t must see the SAME step count, so no workgroup of the element kernel may advance
// steps_dev[t] while others still read it (and all of them must take the same skip decision, from a word that a host may clear at
// any moment).  The simplest design that makes this impossible is stream order: a ONE-workgroup prologue launch reads the skip word
// and the norm once, advances the counts, and writes everything the update needs -- apply flag, clip coefficient, the fp32
// hyper-parameters, each tensor's lr_t and 1 / sqrt(bc2) -- into a scalar block; the element launches behind it on the stream read
// that block and nothing else.  No grid-wide synchronisation, no atomics, one more (tiny) launch per step.
// scalar block, fp32: [0] apply (1 / 0)  [1] clip  [2] b1  [3] b2  [4] 1 - b1  [5] 1 - b2  [6] eps  [7] wd  [8 + 2 t] lr_t  [9 + 2 t] 1 / sqrt(bc2)
constexpr int ADAM_SC_HEAD = 8;
constexpr int ADAM_PRO_MAX = 2048;   // tensors per prologue launch (their has-a-gradient bits travel in the launch arguments)
struct AdamProArgs {
  unsigned has[ADAM_PRO_MAX / 32];
  int base, count, first;
  int *steps;
  const double *hyper, *sqnorm;
  const volatile int *skip;
  float *sc;
};
__global__ __launch_bounds__(256) void adam_dev_prologue_kernel(AdamProArgs a) {
  __shared__ int apply_s;
  const double lr = a.hyper[0], b1 = a.hyper[1], b2 = a.hyper[2];
  if (threadIdx.x == 0) {
    int apply = 1;
    if (a.first) {   // the decision is taken ONCE per step: later prologue launches of the same step read it back
      double clip = 1.0;
      if (a.skip && *a.skip != 0) apply = 0;
      if (a.sqnorm) {
        const double sq = *a.sqnorm, max_norm = a.hyper[5];
        if (!__builtin_isfinite(sq)) apply = 0;
        else if (max_norm > 0.0) clip = fmin(1.0, max_norm / (sqrt(sq) + 1e-6));
      }
      a.sc[0] = apply ? 1.f : 0.f;
      a.sc[1] = (float)clip;
      a.sc[2] = (float)b1; a.sc[3] = (float)b2; a.sc[4] = (float)(1.0 - b1); a.sc[5] = (float)(1.0 - b2);
      a.sc[6] = (float)a.hyper[3]; a.sc[7] = (float)a.hyper[4];
    } else {
      apply = a.sc[0] != 0.f;
    }
    apply_s = apply;
  }
  __syncthreads();
  if (!apply_s) return;   // a skipped step: the counts stay
  for (int t = threadIdx.x; t < a.count; t += 256) {
    if (!(a.has[t >> 5] >> (t & 31) & 1u)) continue;   // no gradient: no step (torch.optim.Adam)
    const int step = a.steps[a.base + t] + 1;
    a.steps[a.base + t] = step;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    a.sc[ADAM_SC_HEAD + 2 * (a.base + t)] = (float)(lr / bc1);
    a.sc[ADAM_SC_HEAD + 2 * (a.base + t) + 1] = (float)(1.0 / sqrt(bc2));
  }
}

struct AdamDevArgs {
  float *p[ADAM_MAX], *m[ADAM_MAX], *v[ADAM_MAX];
  const float *g[ADAM_MAX];
  long n[ADAM_MAX];
  int base;
  const float *sc;
};
struct AdamCoef { float clip, b1, b2, omb1, omb2, eps, wd, lr_t, inv_bc2_sqrt; };
__device__ inline void adam_element(float &p, float &m, float &v, float g, const AdamCoef &c) {
  const float gi = g * c.clip + c.wd * p;
  m = c.b1 * m + c.omb1 * gi;
  v = c.b2 * v + c.omb2 * gi * gi;
  p -= c.lr_t * m / (sqrtf(v) * c.inv_bc2_sqrt + c.eps);
}
__global__ __launch_bounds__(256) void adam_dev_kernel(AdamDevArgs a) {
  const int t = blockIdx.y;
  const float *g = a.g[t];
  if (!g || a.sc[0] == 0.f) return;
  float *p = a.p[t], *m = a.m[t], *v = a.v[t];
  const float *sc = a.sc;
  const AdamCoef c = {sc[1], sc[2], sc[3], sc[4], sc[5], sc[6], sc[7],
                      sc[ADAM_SC_HEAD + 2 * (a.base + t)], sc[ADAM_SC_HEAD + 2 * (a.base + t) + 1]};
  const long n = a.n[t], stride = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
  long done = 0;
  if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
        reinterpret_cast<uintptr_t>(g)) & 15) == 0) {   // 16-byte loads / stores over the aligned body, scalar tail
    const long n4 = n / 4;
    f32x4 *p4 = reinterpret_cast<f32x4 *>(p), *m4 = reinterpret_cast<f32x4 *>(m), *v4 = reinterpret_cast<f32x4 *>(v);
    const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
    for (long i = first; i < n4; i += stride) {
      f32x4 pi = p4[i], mi = m4[i], vi = v4[i];
      const f32x4 gi = g4[i];
      for (int k = 0; k < 4; ++k) {
        float pk = pi[k], mk = mi[k], vk = vi[k];
        adam_element(pk, mk, vk, gi[k], c);
        pi[k] = pk; mi[k] = mk; vi[k] = vk;
      }
      m4[i] = mi; v4[i] = vi; p4[i] = pi;
    }
    done = 4 * n4;
  }
  for (long i = done + first; i < n; i += stride) adam_element(p[i], m[i], v[i], g[i], c);
}

}  // namespace fe

using namespace fe;

extern "C" {

int fastegnn_augment_edge_attr(const int64_t *edge_index, const float *loc, const float *edge_attr, int32_t E,
                               int32_t k, float *out, void *stream) {
  if (E == 0) return FASTEGNN_OK;
  FE_REQUIRE(edge_index && loc && out && (k == 0 || edge_attr), "augment_edge_attr: null pointer");
  hipLaunchKernelGGL(augment_edge_attr_kernel, dim3(cdiv(E, 256)), dim3(256), 0, (hipStream_t)stream, edge_index, loc,
                     edge_attr, E, k, out);
  return check_launch("augment_edge_attr_kernel");
}

// both loss entry points: sample_count null = every row of sample_nodes is full
static int loss_mse_mmd_launch(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                               const int32_t *sample_count, int32_t N, int32_t B, int32_t C, int32_t S, float sigma,
                               float weight, float *loss2, float *g_loc, float *g_vloc, void *stream) {
  FE_REQUIRE(loc_pred && loc_t && vloc && loss2 && g_loc && g_vloc && (S == 0 || sample_nodes),
             "loss_mse_mmd: null pointer");
  FE_REQUIRE(C <= 256 && S <= 4096, "loss_mse_mmd: C <= 256 and S <= 4096");
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(loss2, 0, 2 * sizeof(float), st);
  int grid = cdiv((long)N * 3, 256 * 8);
  if (grid > 1024) grid = 1024;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(loss_mse_kernel, dim3(grid), dim3(256), 0, st, loc_pred, loc_t, (long)N * 3, g_loc, loss2);
  const size_t lds = (size_t)(6 * C + 6 * S) * sizeof(float);
  if (B > 0)   // no graph, no MMD term (and no launch of an empty grid)
    hipLaunchKernelGGL(loss_mmd_kernel, dim3(B), dim3(256), lds, st, loc_pred, vloc, sample_nodes, sample_count, B, C, S, sigma,
                       weight, g_loc, g_vloc, loss2);
  return check_launch("loss_mse_mmd");
}

int fastegnn_loss_mse_mmd(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                          int32_t N, int32_t B, int32_t C, int32_t S, float sigma, float weight, float *loss2,
                          float *g_loc, float *g_vloc, void *stream) {
  return loss_mse_mmd_launch(loc_pred, loc_t, vloc, sample_nodes, nullptr, N, B, C, S, sigma, weight, loss2, g_loc, g_vloc,
                             stream);
}

int fastegnn_loss_mse_mmd_ragged(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                                 const int32_t *sample_count, int32_t N, int32_t B, int32_t C, int32_t S, float sigma,
                                 float weight, float *loss2, float *g_loc, float *g_vloc, void *stream) {
  FE_REQUIRE(sample_count || B == 0, "loss_mse_mmd_ragged: null sample_count (fastegnn_loss_mse_mmd is the form with full rows)");
  return loss_mse_mmd_launch(loc_pred, loc_t, vloc, sample_nodes, sample_count, N, B, C, S, sigma, weight, loss2, g_loc,
                             g_vloc, stream);
}

int fastegnn_loss_mse_mmd_eval(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                               const int32_t *sample_count, int32_t N, int32_t B, int32_t C, int32_t S, float sigma,
                               float weight, double *acc, void *stream) {
  FE_REQUIRE(acc, "loss_mse_mmd_eval: null acc (three doubles in device memory)");
  FE_REQUIRE(N >= 0 && B >= 0 && C >= 0 && S >= 0, "loss_mse_mmd_eval: negative size");
  FE_REQUIRE(C <= 256 && S <= 4096, "loss_mse_mmd_eval: C <= 256 and S <= 4096");
  if (B == 0) return FASTEGNN_OK;   // no graph: acc stays as it is
  const bool mmd = sample_nodes && S > 0;
  FE_REQUIRE((N == 0 || (loc_pred && loc_t)) && (!mmd || (vloc && loc_pred)), "loss_mse_mmd_eval: null pointer");
  const size_t lds = mmd ? (size_t)(3 * C + 3 * S) * sizeof(float) : 0;
  hipLaunchKernelGGL(loss_eval_kernel, dim3(1), dim3(EVAL_THREADS), lds, (hipStream_t)stream, loc_pred, loc_t, vloc,
                     mmd ? sample_nodes : nullptr, sample_count, (long)N * 3, B, C, S, sigma, weight, acc);
  return check_launch("loss_eval_kernel");
}

size_t fastegnn_loss_ordered_ws_doubles(int32_t N, int32_t B) {
  return (size_t)loss_ordered_mse_grid((long)(N > 0 ? N : 0) * 3) + (size_t)(B > 0 ? B : 0);
}

int fastegnn_loss_mse_mmd_ordered(const float *loc_pred, const float *loc_t, const float *vloc, const int32_t *sample_nodes,
                                  const int32_t *sample_count, int32_t N, int32_t B, int32_t C, int32_t S, float sigma,
                                  float weight, float *loss2, float *g_loc, float *g_vloc, double *ws, size_t ws_doubles,
                                  void *stream) {
  FE_REQUIRE(N >= 0 && B >= 0 && C >= 0 && S >= 0, "loss_mse_mmd_ordered: negative size");
  FE_REQUIRE(C <= 256 && S <= 4096, "loss_mse_mmd_ordered: C <= 256 and S <= 4096");
  FE_REQUIRE(loss2 && ws && (N == 0 || (loc_pred && loc_t && g_loc)), "loss_mse_mmd_ordered: null pointer");
  FE_REQUIRE(B == 0 || ((C == 0 || (vloc && g_vloc)) && (S == 0 || (sample_nodes && loc_pred && g_loc))),
             "loss_mse_mmd_ordered: null pointer");
  FE_REQUIRE(ws_doubles >= fastegnn_loss_ordered_ws_doubles(N, B), "loss_mse_mmd_ordered: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const long n3 = (long)N * 3;
  const int grid = loss_ordered_mse_grid(n3);
  hipLaunchKernelGGL(loss_mse_ordered_kernel, dim3(grid), dim3(256), 0, st, loc_pred, loc_t, n3, g_loc, ws);
  const size_t lds = (size_t)(3 * C + 3 * S) * sizeof(float);
  if (B > 0)   // no graph: the MSE only
    hipLaunchKernelGGL(loss_mmd_ordered_kernel, dim3(B), dim3(256), lds, st, loc_pred, vloc, sample_nodes, sample_count, B, C, S,
                       sigma, weight, g_loc, g_vloc, ws + grid);
  hipLaunchKernelGGL(loss_ordered_final_kernel, dim3(1), dim3(256), 0, st, (const double *)ws, grid, B, n3, loss2);
  return check_launch("loss_mse_mmd_ordered");
}

int fastegnn_loss_accumulate(const float *loss, const float *mse, int32_t B, double *acc, void *stream) {
  FE_REQUIRE(loss && mse && acc, "loss_accumulate: null pointer");
  FE_REQUIRE(B >= 0, "loss_accumulate: B < 0");
  if (B == 0) return FASTEGNN_OK;   // no graph: acc stays as it is
  hipLaunchKernelGGL(loss_accumulate_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss, mse, B, acc);
  return check_launch("loss_accumulate");
}

int fastegnn_mmd_sample(const int64_t *ptr, int32_t B, int32_t S, uint64_t *rng, int32_t advance, int32_t *sample_nodes,
                        int32_t *sample_count, void *stream) {
  FE_REQUIRE(B >= 0 && S >= 0 && S <= 4096, "mmd_sample: B >= 0 and 0 <= S <= 4096");
  FE_REQUIRE(ptr && rng && (B == 0 || sample_count) && (B == 0 || S == 0 || sample_nodes), "mmd_sample: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (B > 0) {
    const long total = (long)B * S > B ? (long)B * S : B;
    long grid = (total + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(mmd_sample_kernel, dim3((unsigned)grid), dim3(256), 0, st, ptr, B, S, rng, sample_nodes, sample_count);
  }
  if (advance) hipLaunchKernelGGL(mmd_advance_kernel, dim3(1), dim3(1), 0, st, rng);
  return check_launch("mmd_sample");
}

int fastegnn_adam_step_v2(float *const *params, const float *const *grads, float *const *exp_avg,
                          float *const *exp_avg_sq, const int64_t *numel, int32_t n_tensors, const int32_t *steps,
                          double lr, double beta1, double beta2, double eps, double weight_decay, void *stream) {
  FE_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && steps && n_tensors >= 0, "adam_step: bad argument");
  for (int t = 0; t < n_tensors; ++t)
    FE_REQUIRE(!grads[t] || steps[t] >= 1, "adam_step: a tensor with a gradient needs step >= 1");
  hipStream_t st = (hipStream_t)stream;
  for (int base = 0; base < n_tensors; base += ADAM_MAX) {
    AdamArgs a;
    a.count = n_tensors - base < ADAM_MAX ? n_tensors - base : ADAM_MAX;
    long nmax = 0;
    for (int t = 0; t < a.count; ++t) {
      a.p[t] = params[base + t]; a.g[t] = grads[base + t]; a.m[t] = exp_avg[base + t]; a.v[t] = exp_avg_sq[base + t];
      a.n[t] = numel[base + t];
      const int step = a.g[t] ? steps[base + t] : 1;   // a skipped tensor's count is not read
      const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
      a.lr_t[t] = (float)(lr / bc1);
      a.inv_bc2_sqrt[t] = (float)(1.0 / sqrt(bc2));
      if (a.n[t] > nmax) nmax = a.n[t];
    }
    a.b1 = (float)beta1; a.b2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps; a.wd = (float)weight_decay;
    int gx = cdiv(nmax, 256 * 4);
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(adam_kernel, dim3(gx, a.count), dim3(256), 0, st, a);
  }
  return check_launch("adam_kernel");
}

size_t fastegnn_grad_sqnorm_partials(const int64_t *numel, int32_t n_tensors) {
  if (!numel || n_tensors <= 0) return 1;
  size_t slots = 0;
  for (int base = 0; base < n_tensors; base += ADAM_MAX) {
    const int count = n_tensors - base < ADAM_MAX ? n_tensors - base : ADAM_MAX;
    long nmax = 0;
    for (int t = 0; t < count; ++t) nmax = numel[base + t] > nmax ? numel[base + t] : nmax;
    slots += (size_t)count * adam_grid_x(nmax);
  }
  return slots;
}

int fastegnn_grad_sqnorm(const float *const *grads, const int64_t *numel, int32_t n_tensors, double *ws,
                         size_t ws_doubles, double *out, void *stream) {
  FE_REQUIRE(grads && numel && ws && out && n_tensors >= 0, "grad_sqnorm: bad argument");
  FE_REQUIRE(ws_doubles >= fastegnn_grad_sqnorm_partials(numel, n_tensors), "grad_sqnorm: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  size_t slot = 0;
  for (int base = 0; base < n_tensors; base += ADAM_MAX) {
    SqnArgs a;
    const int count = n_tensors - base < ADAM_MAX ? n_tensors - base : ADAM_MAX;
    long nmax = 0;
    for (int t = 0; t < ADAM_MAX; ++t) {
      a.g[t] = t < count ? grads[base + t] : nullptr;
      a.n[t] = t < count ? numel[base + t] : 0;
      FE_REQUIRE(a.n[t] >= 0, "grad_sqnorm: negative numel");
      if (a.n[t] > nmax) nmax = a.n[t];
    }
    a.part = ws + slot;
    const int gx = adam_grid_x(nmax);
    hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3(gx, count), dim3(256), 0, st, a);
    slot += (size_t)count * gx;
  }
  hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(256), 0, st, ws, (long)slot, out);
  return check_launch("grad_sqnorm");
}

size_t fastegnn_adam_dev_scratch_bytes(int32_t n_tensors) {
  return (size_t)(ADAM_SC_HEAD + 2 * (n_tensors > 0 ? n_tensors : 0)) * sizeof(float);
}

int fastegnn_adam_step_dev(float *const *params, const float *const *grads, float *const *exp_avg,
                           float *const *exp_avg_sq, const int64_t *numel, int32_t n_tensors, int32_t *steps_dev,
                           const double *hyper_dev, const double *sqnorm_dev, const int32_t *skip_word, void *scratch,
                           size_t scratch_bytes, void *stream) {
  FE_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && n_tensors >= 0, "adam_step_dev: bad argument");
  FE_REQUIRE(steps_dev && hyper_dev && scratch, "adam_step_dev: the step counts, the hyper-parameters and the scratch block live in device memory");
  FE_REQUIRE(scratch_bytes >= fastegnn_adam_dev_scratch_bytes(n_tensors) && (reinterpret_cast<uintptr_t>(scratch) & 15) == 0,
             "adam_step_dev: scratch too small or not 16-byte aligned");
  for (int t = 0; t < n_tensors; ++t)
    FE_REQUIRE(numel[t] >= 0 && (!grads[t] || (params[t] && exp_avg[t] && exp_avg_sq[t])), "adam_step_dev: null tensor");
  hipStream_t st = (hipStream_t)stream;
  float *sc = static_cast<float *>(scratch);
  for (int base = 0; base < n_tensors || base == 0; base += ADAM_PRO_MAX) {   // (n_tensors = 0 still takes the decision: one launch)
    AdamProArgs pa;
    pa.base = base;
    pa.count = n_tensors - base < ADAM_PRO_MAX ? n_tensors - base : ADAM_PRO_MAX;
    pa.first = base == 0;
    for (int w = 0; w < ADAM_PRO_MAX / 32; ++w) pa.has[w] = 0u;
    for (int t = 0; t < pa.count; ++t)
      if (grads[base + t]) pa.has[t >> 5] |= 1u << (t & 31);
    pa.steps = steps_dev; pa.hyper = hyper_dev; pa.sqnorm = sqnorm_dev; pa.skip = skip_word; pa.sc = sc;
    hipLaunchKernelGGL(adam_dev_prologue_kernel, dim3(1), dim3(256), 0, st, pa);
  }
  for (int base = 0; base < n_tensors; base += ADAM_MAX) {
    AdamDevArgs a;
    const int count = n_tensors - base < ADAM_MAX ? n_tensors - base : ADAM_MAX;
    long nmax = 0;
    for (int t = 0; t < ADAM_MAX; ++t) {
      const bool in = t < count;
      a.p[t] = in ? params[base + t] : nullptr; a.g[t] = in ? grads[base + t] : nullptr;
      a.m[t] = in ? exp_avg[base + t] : nullptr; a.v[t] = in ? exp_avg_sq[base + t] : nullptr;
      a.n[t] = in ? numel[base + t] : 0;
      if (a.n[t] > nmax) nmax = a.n[t];
    }
    a.base = base; a.sc = sc;
    hipLaunchKernelGGL(adam_dev_kernel, dim3(adam_grid_x(nmax), count), dim3(256), 0, st, a);
  }
  return check_launch("adam_step_dev");
}

// every tensor at the same step: the form of ABI revisions up to 107
int fastegnn_adam_step(float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                       const int64_t *numel, int32_t n_tensors, int32_t step, float lr, float beta1, float beta2,
                       float eps, float weight_decay, void *stream) {
  FE_REQUIRE(step >= 1 && n_tensors >= 0, "adam_step: bad argument");
  std::vector<int32_t> steps((size_t)n_tensors, step);
  return fastegnn_adam_step_v2(params, grads, exp_avg, exp_avg_sq, numel, n_tensors, steps.data(), lr, beta1, beta2,
                               eps, weight_decay, stream);
}

}  // extern "C"

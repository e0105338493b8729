// The keyed permutation of include/fastegnn_hip.h ("the device-side MMD sample": mix64, mix32, eight Feistel rounds, cycle walking),
// integers only, shared by its two callers: mmd_sample_kernel (train.hip) and collate_draw_kernel (collate.hip).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace fe {

__host__ __device__ inline uint64_t mix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du;
  x ^= x >> 15; x *= 0x846CA68Bu;
  return x ^ (x >> 16);
}
constexpr int PERM_ROUNDS = 8;

// gkey = mix64(mix64(seed) ^ counter): the part of the key that one draw shares
__host__ __device__ inline uint64_t perm_draw_key(uint64_t seed, uint64_t counter) { return mix64(mix64(seed) ^ counter); }

// perm_b(j) of [0, n), 1 <= n < 2^31, j < n.
// cycle walking: E is a bijection of [0, 2^k) and j < n, so the walk stays on j's own cycle, which holds at most 2^k - n values
// >= n -- it ends within 2^k - n + 1 applications (2^k / n < 4 on average)
__host__ __device__ inline uint64_t keyed_perm(uint64_t gkey, uint64_t b, uint64_t n, uint64_t j) {
  int k = n > 1 ? 64 - __builtin_clzll((unsigned long long)(n - 1)) : 0;   // ceil(log2 n)
  if (k < 2) k = 2;
  k += k & 1;
  const int h = k >> 1;
  const uint64_t mask = (1ull << h) - 1, g = mix64(gkey ^ b);
  uint64_t key[PERM_ROUNDS];
  for (int r = 0; r < PERM_ROUNDS; ++r) key[r] = mix64(g + (uint64_t)r);
  uint64_t x = j;
  do {
    for (int r = 0; r < PERM_ROUNDS; ++r) {
      const uint64_t L = x >> h, R = x & mask;
      const uint64_t F = (uint64_t)(mix32((uint32_t)R ^ (uint32_t)key[r]) ^ (uint32_t)(key[r] >> 32)) & mask;
      x = (R << h) | (L ^ F);
    }
  } while (x >= n);
  return x;
}

}  // namespace fe

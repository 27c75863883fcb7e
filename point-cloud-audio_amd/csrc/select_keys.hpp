// Sort keys of the per-set point selections (max-K / random-K), shared by the point-set
// sub-sampler (subsample.hip) and the baselines' zero-filled inputs (baselines.hip), so that both
// keep exactly the same cells for the same (seed, draw, batch slot, set).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pca {

// ascending order of the returned key = descending order of v; -0 == +0; NaN last
__device__ __forceinline__ uint32_t desc_key(float v) {
  if (v != v) return 0xffffffffu;
  v += 0.0f;                                        // -0 -> +0
  const uint32_t u = __float_as_uint(v);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}
// splitmix64 finaliser
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// one random stream per (seed, draw, batch slot b, set)
__device__ __forceinline__ uint64_t select_stream(uint64_t seed, uint64_t draw, int64_t set, int b) {
  return mix64(seed ^ mix64(draw * 0x9e3779b97f4a7c15ull + (uint64_t)set) ^
               mix64(0x632be59bd9b4e019ull * (uint64_t)(b + 1)));
}
// high word of the random-K key of point p
__device__ __forceinline__ uint32_t rand_key(uint64_t stream, int p) {
  return (uint32_t)(mix64(stream + (uint64_t)p * 0xd1342543de82ef95ull) >> 32);
}

}  // namespace pca

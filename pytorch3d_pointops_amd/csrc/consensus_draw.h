// consensus_draw.h -- the counter-based draws of the consensus operators (ransac.hip, plane.hip), __host__ __device__:
// the hash and the draw of three distinct records.  Integers only, so a host program runs them as the kernels do
// (tests/native/ransac_hypothesis_main.cpp); consensus.h and ransac_hypothesis.h include it; nothing else defines them.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace pointops {

// lowbias32 (an xorshift-multiply chain; a bijection of uint32)
__host__ __device__ __forceinline__ uint32_t rh_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// u = hash32(seed, n, h, j): integers only, no state
__host__ __device__ __forceinline__ uint32_t rh_hash32(int64_t seed, int64_t n, int64_t h, int j) {
  const uint64_t sd = (uint64_t)seed;
  uint32_t x = rh_mix((uint32_t)sd + 0x9e3779b9u);
  x = rh_mix(x ^ (uint32_t)(sd >> 32));
  x = rh_mix(x ^ (uint32_t)n);
  x = rh_mix(x ^ (uint32_t)h);
  return rh_mix(x ^ (uint32_t)j);
}

__host__ __device__ __forceinline__ uint32_t rh_mulhi(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
}

// Three distinct positions in [0, M), uniform over the ordered triples; M >= 3.
__host__ __device__ __forceinline__ void rh_draw(int64_t seed, int64_t n, int64_t h, uint32_t M, uint32_t (&i)[3]) {
  i[0] = rh_mulhi(rh_hash32(seed, n, h, 0), M);
  i[1] = rh_mulhi(rh_hash32(seed, n, h, 1), M - 1);
  i[1] += i[1] >= i[0] ? 1u : 0u;
  const uint32_t lo = i[0] < i[1] ? i[0] : i[1], hi = i[0] < i[1] ? i[1] : i[0];
  i[2] = rh_mulhi(rh_hash32(seed, n, h, 2), M - 2);
  i[2] += i[2] >= lo ? 1u : 0u;
  i[2] += i[2] >= hi ? 1u : 0u;
}

}  // namespace pointops

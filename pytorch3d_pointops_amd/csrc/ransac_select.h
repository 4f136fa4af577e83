// ransac_select.h -- what the hypothesise-and-score operators share on the device (ransac.hip, plane.hip): the
// workgroup shape, the clamped length of a cloud and the 64-bit key reduction of the selection.  Written once; both
// files include it.
#pragma once
#include "common.h"

namespace pointops {

constexpr int kRsBlock = 256;
constexpr int kRsWaves = kRsBlock / kWave;

__device__ __forceinline__ int rs_length(const int64_t* __restrict__ lengths, int n, int P) {
  if (lengths == nullptr) return P;
  const int64_t l = lengths[n];
  return (int)(l < 0 ? 0 : (l > P ? P : l));
}

// The largest key of the workgroup, valid in thread 0.  s_key: kRsWaves words of LDS.
__device__ __forceinline__ unsigned long long rs_block_max(unsigned long long key, unsigned long long* s_key) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, kWave);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) s_key[threadIdx.x / kWave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kRsWaves; ++w) key = s_key[w] > key ? s_key[w] : key;
  }
  return key;
}

}  // namespace pointops

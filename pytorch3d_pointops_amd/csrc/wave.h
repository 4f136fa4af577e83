// wave.h -- the plain cross-lane steps of a wave64, written once (gfx950): sums, minima and maxima over the lanes,
// the inclusive scan, and the workgroup prefix built on it.  The order of the exchanges is part of the contract: the
// float sums of the chamfer kernels are pinned bit for bit.  (The specialised exchanges stay with their kernels: the
// arg-max pairs and DPP code of fps.hip, the 64-bit keys of knn_grid_wsort.hip and knn_grid_wave_kernel, wave_add.)
#pragma once
#include "common.h"

namespace pointops {

// Butterfly over groups of WIDTH consecutive lanes, offsets WIDTH / 2 down to 1: every lane ends with the group's result.
template <int WIDTH = kWave, typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = WIDTH / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}

// Inclusive prefix sum over the lanes (Hillis-Steele, offsets 1, 2, ..., SPAN / 2).  SPAN < kWave stops early: lanes
// below SPAN hold their prefix, the lanes above a sum over the SPAN lanes up to their own.
template <int SPAN = kWave>
__device__ __forceinline__ int wave_inclusive_sum(int v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int off = 1; off < SPAN; off <<= 1) {
    const int u = __shfl_up(v, off, kWave);
    if (lane >= off) v += u;
  }
  return v;
}

// Exclusive prefix of v over a workgroup of WAVES waves, one value per thread; `total` = the workgroup's sum.
// s_wsum: WAVES ints of LDS.  Exactly ONE barrier inside; the barrier that frees s_wsum for the next use is the
// caller's.  Call it from workgroup-uniform control flow only.
template <int WAVES>
__device__ __forceinline__ int block_exclusive_sum(int v, int* s_wsum, int& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int inc = wave_inclusive_sum(v);
  if (lane == kWave - 1) s_wsum[wave] = inc;
  __syncthreads();
  int excl = inc - v;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int t = s_wsum[w];
    if (w < wave) excl += t;
    total += t;
  }
  return excl;
}

}  // namespace pointops

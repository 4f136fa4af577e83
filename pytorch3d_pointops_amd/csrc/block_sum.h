// block_sum.h -- the fp64 block reduction of the per-cloud moment passes (points_alignment.hip, registration.hip): DPP
// wave sums, the four waves of a block through LDS, one partial per block (pa_block_sum), and the ascending sum of a
// cloud's partials in the one-wave solve kernels (pa_sum_partials).  No atomics: the order of every sum is fixed
// by the row index and the launch shape, so results are bit-reproducible.
#pragma once
#include "common.h"

namespace pointops {

constexpr int kPaBlock = 256;          // threads per block of the point passes
constexpr int kPaWaves = kPaBlock / kWave;
constexpr int kPaRowsPerThread = 8;    // rows per thread before a cloud gets another block
constexpr int kPaMaxBlocks = 32;       // partials per cloud (the solve sums them one after the other)

inline int pa_blocks(int64_t P) {
  const int64_t nb = ceil_div(P, (int64_t)kPaBlock * kPaRowsPerThread);
  return (int)(nb < 1 ? 1 : (nb > kPaMaxBlocks ? kPaMaxBlocks : nb));
}

// v + (v of the lane DPP control CTRL names); lanes outside the rows of ROWS add 0
template <int CTRL, int ROWS>
__device__ __forceinline__ double pa_dpp_add(double v) {
  const int hi = __double2hiint(v), lo = __double2loint(v);
  const int ohi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROWS, 0xf, false);
  const int olo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROWS, 0xf, false);
  return v + __hiloint2double(ohi, olo);
}
// sum over the wave (all 64 lanes must be active); the result is valid in lane 63
__device__ __forceinline__ double pa_wave_sum_lane63(double v) {
  v = pa_dpp_add<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v = pa_dpp_add<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  v = pa_dpp_add<0x124, 0xf>(v);  // row_ror 4
  v = pa_dpp_add<0x128, 0xf>(v);  // row_ror 8
  v = pa_dpp_add<0x142, 0xa>(v);  // row_bcast15 into rows 1, 3
  v = pa_dpp_add<0x143, 0xc>(v);  // row_bcast31 into rows 2, 3
  return v;
}

// Block sum of M per-thread fp64 values: out[m] (m < M) written by thread m.  Every thread of the block calls it.
template <int M>
__device__ __forceinline__ void pa_block_sum(const double (&acc)[M], double (*s_part)[M], double* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double v = pa_wave_sum_lane63(acc[m]);
    if (lane == kWave - 1) s_part[wave][m] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < M) {
    double v = s_part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kPaWaves; ++w) v += s_part[w][threadIdx.x];
    out[threadIdx.x] = v;
  }
}

// The other end, in the one-wave solve kernels: lane m < M adds partial m of the cloud's nb blocks (cloud_partials:
// [nb][M]) in ascending block order -- the same sum in every run -- into s_mom[m] and, where given, moments_out[m].
// A cloud that is not `live` (registration: frozen) sums nothing and reports zeros.  Every thread of the block calls it;
// s_mom is complete when it returns.
template <int M>
__device__ __forceinline__ void pa_sum_partials(const double* __restrict__ cloud_partials, int nb, bool live,
                                                double* s_mom, double* __restrict__ moments_out) {
  static_assert(M <= kWave, "one lane per moment");
  if ((int)threadIdx.x < M) {
    double v = 0.0;
    if (live) {
      const double* __restrict__ src = cloud_partials + threadIdx.x;
#pragma unroll 8
      for (int b = 0; b < nb; ++b) v += src[(int64_t)b * M];
    }
    s_mom[threadIdx.x] = v;
    if (moments_out != nullptr) moments_out[threadIdx.x] = v;
  }
  __syncthreads();
}

}  // namespace pointops

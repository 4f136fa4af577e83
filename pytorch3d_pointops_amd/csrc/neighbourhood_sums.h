// neighbourhood_sums.h -- the per-lane sums over a K-row neighbourhood, written once: its mean, its covariance about the
// mean and the backward of that covariance (covariance.hip at D <= DM; local_frames.hip at D = DM = 3).
//
//     m = mean_k x_k ;  c[a][b] = mean_k (x_k[a] - m[a]) (x_k[b] - m[b]) ;  grad_x_k = (G + G^T) (x_k - m) / K
// (the mean terms of the backward cancel because sum_k (x_k - m) = 0).  fp32 throughout, every sum in ascending k, one
// multiply by 1.0f / K at the end: whoever calls these gets the same bits from the same rows.
//
// `row(k)` gives row k as something x with x[d] for d < D: a pointer to the row where it lies in memory (covariance.hip:
// global memory or the lane's LDS row), an NbRow where it has to be gathered first (local_frames.hip).  The D of a
// runtime-D instance (D < DM) is held to by `d < D` predicates HERE, around each read and each add: an accessor that
// loads a whole row ahead of the predicates, padded with zeros or not, costs the runtime-D instances of covariance.hip
// 8 VGPRs and a wave of occupancy (92-94 VGPRs there leave 2 to spare at five waves per SIMD).
#pragma once
#include "common.h"

namespace pointops {

template <int DM>
struct NbRow {  // a row in registers
  float v[DM];
  __device__ __forceinline__ float operator[](int d) const { return v[d]; }
};

template <int DM, class Row>
__device__ __forceinline__ void nb_mean(Row&& row, int K, int D, float (&m)[DM]) {
#pragma unroll
  for (int d = 0; d < DM; ++d) m[d] = 0.0f;
  for (int k = 0; k < K; ++k) {
    const auto x = row(k);
#pragma unroll
    for (int d = 0; d < DM; ++d)
      if (d < D) m[d] += x[d];
  }
  const float inv_k = 1.0f / (float)K;
#pragma unroll
  for (int d = 0; d < DM; ++d) m[d] *= inv_k;
}

// c[a][b] for a, b < D (zero elsewhere)
template <int DM, class Row>
__device__ __forceinline__ void nb_covariance(Row&& row, int K, int D, float (&c)[DM][DM]) {
  float m[DM];
  nb_mean<DM>(row, K, D, m);
#pragma unroll
  for (int a = 0; a < DM; ++a)
#pragma unroll
    for (int b = 0; b < DM; ++b) c[a][b] = 0.0f;
  for (int k = 0; k < K; ++k) {
    const auto x = row(k);
    float v[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) v[d] = d < D ? x[d] - m[d] : 0.0f;
#pragma unroll
    for (int a = 0; a < DM; ++a)
#pragma unroll
      for (int b = 0; b < DM; ++b)
        if (a < D && b < D) c[a][b] += v[a] * v[b];
  }
  // (a select, not a branch around the multiply: the branch costs the runtime-D instances of covariance.hip 60 VGPRs)
  const float inv_k = 1.0f / (float)K;
#pragma unroll
  for (int a = 0; a < DM; ++a)
#pragma unroll
    for (int b = 0; b < DM; ++b) c[a][b] = (a < D && b < D) ? c[a][b] * inv_k : 0.0f;
}

// out[k * D + a] = sum_b ((g[a][b] + g[b][a]) / K) (x_k[b] - m[b]) for the D x D gradient g.  `out` may be the memory
// `row` reads (the staged backward works in place): row k is read whole before any of it is written, and neither
// pointer is __restrict__.
template <int DM, class Row>
__device__ __forceinline__ void nb_covariance_backward(Row&& row, int K, int D, const float* g, float* out) {
  float m[DM];
  nb_mean<DM>(row, K, D, m);
  const float inv_k = 1.0f / (float)K;
  float s[DM][DM];  // (G + G^T) / K
#pragma unroll
  for (int a = 0; a < DM; ++a)
#pragma unroll
    for (int b = 0; b < DM; ++b) s[a][b] = (a < D && b < D) ? (g[a * D + b] + g[b * D + a]) * inv_k : 0.0f;
  for (int k = 0; k < K; ++k) {
    const auto x = row(k);
    float v[DM], w[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) v[d] = d < D ? x[d] - m[d] : 0.0f;
#pragma unroll
    for (int a = 0; a < DM; ++a) {
      float acc = 0.0f;
#pragma unroll
      for (int b = 0; b < DM; ++b) acc += s[a][b] * v[b];
      w[a] = acc;
    }
#pragma unroll
    for (int a = 0; a < DM; ++a)
      if (a < D) out[k * D + a] = w[a];
  }
}

}  // namespace pointops

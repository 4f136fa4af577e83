// ransac_hypothesis.h -- the per-lane routines of ransac.hip, __host__ __device__: the edge-length test, the three-pair
// solve and the residual.  The counter-based hash and the draw, which every consensus operator shares, are in
// consensus_draw.h, included here for the host program below.
//
// They live here, as the solvers of small_solvers.h do, so that a host program can run them on millions of triples
// without a GPU (tests/native/ransac_hypothesis_main.cpp); the kernel includes this header and nothing else defines the
// functions.  The normative text is the comment of pointops_ransac_alignment in include/pointops_amd.h.
#pragma once
#include "consensus_draw.h"
#include "small_solvers.h"

namespace pointops {

__host__ __device__ __forceinline__ float rh_sqdist(const float (&a)[3], const float (&b)[3]) {
  const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// Every side of the triangle in X is within the ratio of its side in Y, and the other way round; q = ratio * ratio.
__host__ __device__ __forceinline__ bool rh_edges_ok(const float (&x)[3][3], const float (&y)[3][3], float q) {
  bool ok = true;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const int a = p == 2 ? 1 : 0, b = p == 0 ? 1 : 2;  // (0,1), (0,2), (1,2)
    const float lx = rh_sqdist(x[a], x[b]), ly = rh_sqdist(y[a], y[b]);
    ok = ok && lx >= q * ly && ly >= q * lx;
  }
  return ok;
}

// The alignment of three pairs with unit weights, eps 1e-9 and no reflection: the moments of alignment_moments_kernel
// about pair 0 in fp64, pa_solve<3>, one rounding to fp32.
__host__ __device__ __forceinline__ void rh_solve(const float (&x)[3][3], const float (&y)[3][3], bool estimate_scale,
                                                  float (&R)[3][3], float (&T)[3], float& s) {
  using S = PaSlot<3>;
  double mom[S::kCount];
#pragma unroll
  for (int m = 0; m < S::kCount; ++m) mom[m] = 0.0;
  double px[3], py[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    px[d] = (double)x[0][d];
    py[d] = (double)y[0][d];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double dx[3], dy[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      dx[d] = (double)x[k][d] - px[d];
      dy[d] = (double)y[k][d] - py[d];
    }
    mom[S::kSw] += 1.0;
    mom[S::kSw2] += 1.0;
    double xx = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mom[S::kSwx + a] += dx[a];
      mom[S::kSwy + a] += dy[a];
      mom[S::kSw2x + a] += dx[a];
      mom[S::kSw2y + a] += dy[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) mom[S::kSxy + a * 3 + b] += dx[a] * dy[b];
      xx += dx[a] * dx[a];
    }
    mom[S::kSxx] += xx;
  }
  double Rd[3][3], Td[3], sd, sg[3];
  pa_solve<3>(mom, px, py, estimate_scale, false, 1e-9, Rd, Td, sd, sg);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    T[a] = (float)Td[a];
#pragma unroll
    for (int b = 0; b < 3; ++b) R[a][b] = (float)Rd[a][b];
  }
  s = (float)sd;
}

// The residual of the score and of the evaluation: A = s R (fp32), r = x A + T, d2 = |r - y|^2, unfused, in this order.
__host__ __device__ __forceinline__ float rh_residual(const float (&A)[3][3], const float (&T)[3], float x0, float x1,
                                                      float x2, float y0, float y1, float y2) {
  const float e0 = (((x0 * A[0][0] + x1 * A[1][0]) + x2 * A[2][0]) + T[0]) - y0;
  const float e1 = (((x0 * A[0][1] + x1 * A[1][1]) + x2 * A[2][1]) + T[1]) - y1;
  const float e2 = (((x0 * A[0][2] + x1 * A[1][2]) + x2 * A[2][2]) + T[2]) - y2;
  return (e0 * e0 + e1 * e1) + e2 * e2;
}

}  // namespace pointops

// mls_fit.h -- the per-point arithmetic of smooth_mls (mls.hip) inside and after its walk: the scale of the integer
// moments, the quantized quartic weight, the mean offset, the status and the projection onto the fitted plane.
// __host__ __device__ and free of HIP types: tests/native/mls_fit_main.cpp runs it on the host.  The quantizer and the
// fp64 covariance are iss_saliency.h's (iss_quantize; iss_covariance with W for n).  The definition these functions
// implement step by step is the comment block of pointops_mls_smooth in include/pointops_amd.h; all arithmetic is
// unfused and in the order written (the build passes -ffp-contract=off).
//
// THE BOUND OF THE SUMS.  A hit has d2 < r2 in fp32, so |x_j - x_i| < r (1 + 2^-22) per coordinate (iss_saliency.h) and
// |q| <= 2^15 (1 + 2^-22) + 1/2 < 2^15 + 1:  |q_a q_b| < 2^30 + 2^17 = 2^30 (1 + 2^-13).  The weight is an integer in
// [0, 2^12].  So a term of M2 is below 2^42 (1 + 2^-13) in magnitude, a term of M1 below 2^28, a term of W at most 2^12,
// and kMlsMaxPoints = 2^20 of them stay below 2^62 (1 + 2^-13) < 2^63: no int64 sum overflows.
#pragma once
#include <math.h>
#include <stdint.h>

#include "iss_saliency.h"

#define POINTOPS_MLS_HD POINTOPS_ISS_HD

namespace pointops {

constexpr int kMlsBits = 15;                 // |q| <= 2^15 for an offset of up to 2^e >= r
constexpr int kMlsWeightBits = 12;           // wq in [0, 2^12]
constexpr int64_t kMlsMaxPoints = 1 << 20;   // 2^20 terms of |wq q_a q_b| <= 2^42 (1 + 2^-13) stay below 2^63
constexpr int kMlsMoments = 10;              // W, M1[3], M2[6] (xx, xy, xz, yy, yz, zz)

// s = 2^(15 - e), e the smallest integer with r <= 2^e (iss_scale's rule at 15 bits)
POINTOPS_MLS_HD double mls_scale(float r) { return ldexp(iss_scale(r), kMlsBits - kIssBits); }

// wq = rint(2^12 (1 - d2 / r2)^4) of a hit (d2 < r2): the quotient is ONE correctly rounded fp32 division, the rest
// fp32 products, the scaling (exact) and the rounding (half to even) in fp64.  An integer in [0, 4096].
POINTOPS_MLS_HD int32_t mls_weight(float d2, float r2) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float t = __fdiv_rn(d2, r2);
#else
  const float t = d2 / r2;
#endif
  const float u = 1.0f - t;
  float w = u * u;
  w = w * w;
  return (int32_t)rint((double)w * (double)(1 << kMlsWeightBits));
}

// the eleven integer sums of a support
struct MlsSums {
  int64_t n = 0, W = 0;
  int64_t M1[3] = {0, 0, 0};
  int64_t M2[6] = {0, 0, 0, 0, 0, 0};
};

// one hit's terms: its weight wq and its quantized offset q
POINTOPS_MLS_HD void mls_accumulate(MlsSums& a, int32_t wq, int32_t qx, int32_t qy, int32_t qz) {
  const int64_t w = wq, wx = w * qx, wy = w * qy, wz = w * qz;
  ++a.n;
  a.W += w;
  a.M1[0] += wx, a.M1[1] += wy, a.M1[2] += wz;
  a.M2[0] += wx * qx, a.M2[1] += wx * qy, a.M2[2] += wx * qz;
  a.M2[3] += wy * qy, a.M2[4] += wy * qz, a.M2[5] += wz * qz;
}

// delta = (M1 / W) / s: the weighted mean offset of the support from the point, in the units of the cloud (s is a
// power of two: the second division is exact).  W == 0 (an empty support): delta = 0.
POINTOPS_MLS_HD void mls_offset(const int64_t (&M1)[3], int64_t W, double s, double (&delta)[3]) {
  for (int a = 0; a < 3; ++a) delta[a] = W > 0 ? ((double)M1[a] / (double)W) / s : 0.0;
}

// 1: fewer than min_neighbors points in the support; else 2: the support does not determine a plane (the ascending
// eigenvalues have l1 <= 2^-20 l2: a line, a point, nothing); else 0.  Status 0 implies l2 >= l1 > 0.
POINTOPS_MLS_HD uint8_t mls_status(int64_t num_neighbors, int64_t min_neighbors, const double (&l)[3]) {
  if (num_neighbors < min_neighbors) return 1;
  if (l[1] <= 0x1p-20 * l[2]) return 2;
  return 0;
}

// The outputs of a row of status 0 from its point x, the offset delta, the ascending eigenvalues l and the eigenvectors
// (columns of v): n = column 0, its sign such that the component of largest magnitude is positive (ties to the lower
// axis); normal = n^ = fl32(n); h = (delta_x n^_x + delta_y n^_y) + delta_z n^_z and p = fl32((double)x + h n^) per
// component, in fp64 with n^ widened: the point moves along the RETURNED normal, so the two outputs reproduce each
// other exactly (delta's part along the surface times the rounding of n would otherwise show); curvature =
// fl32(l0 / ((l0 + l1) + l2)).
POINTOPS_MLS_HD void mls_project(const float (&x)[3], const double (&delta)[3], const double (&l)[3],
                                 const double (&v)[3][3], float (&p)[3], float (&normal)[3], float& curvature) {
  double n[3] = {v[0][0], v[1][0], v[2][0]};
  int big = 0;
  if (fabs(n[1]) > fabs(n[big])) big = 1;
  if (fabs(n[2]) > fabs(n[big])) big = 2;
  if (n[big] < 0.0)
    for (int a = 0; a < 3; ++a) n[a] = -n[a];
  for (int a = 0; a < 3; ++a) {
    normal[a] = (float)n[a];
    n[a] = (double)normal[a];
  }
  const double h = (delta[0] * n[0] + delta[1] * n[1]) + delta[2] * n[2];
  for (int a = 0; a < 3; ++a) p[a] = (float)((double)x[a] + h * n[a]);
  curvature = (float)(l[0] / ((l[0] + l[1]) + l[2]));
}

}  // namespace pointops

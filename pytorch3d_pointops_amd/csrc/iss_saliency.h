// iss_saliency.h -- the per-point arithmetic of iss_keypoints (iss.hip) after and around its walks: the scale of the
// integer moments, the quantizer, the fp64 covariance, the fp32 decision and the order of the non-maximum suppression.
// __host__ __device__ and free of HIP types: tests/native/iss_saliency_main.cpp compiles this header alone, with any C++
// compiler.  The definition these functions implement step by step is the comment block of pointops_iss_keypoints in
// include/pointops_amd.h; all arithmetic is unfused and in the order written (the build passes -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define POINTOPS_ISS_HD __host__ __device__ inline
#else
#define POINTOPS_ISS_HD inline
#endif

namespace pointops {

constexpr int kIssBits = 19;             // |q| <= 2^19 for an offset of up to 2^e >= rs
constexpr int64_t kIssMaxPoints = 1 << 24;  // 2^24 hits of |q a * q b| <= 2^38 stay below 2^63

// s = 2^(19 - e), e the smallest integer with rs <= 2^e (rs a finite fp32 > 0, subnormals included)
POINTOPS_ISS_HD double iss_scale(float rs) {
  int k;
  const float m = frexpf(rs, &k);  // rs = m 2^k, 0.5 <= m < 1
  const int e = m == 0.5f ? k - 1 : k;
  return ldexp(1.0, kIssBits - e);
}

// q = rint((x_j - x_i) s): the subtraction and the product in fp64 (s is a power of two: the product is exact), round
// half to even.  The callers pass hits only, |x_j - x_i| < rs (1 + 2^-22), so q fits an int32 with room.
POINTOPS_ISS_HD int32_t iss_quantize(float xj, float xi, double s) {
  return (int32_t)rint(((double)xj - (double)xi) * s);
}

// C (xx, xy, xz, yy, yz, zz) of the integer moments M1 (x, y, z), M2 (the same six) over n hits; n == 0: C = 0
POINTOPS_ISS_HD void iss_covariance(const int64_t (&M1)[3], const int64_t (&M2)[6], int64_t n, double s,
                                    double (&C)[6]) {
  if (n <= 0) {
    for (int k = 0; k < 6; ++k) C[k] = 0.0;
    return;
  }
  const double dn = (double)n;
  const double inv = 1.0 / s, inv2 = inv * inv;  // powers of two
  double m[3];
  for (int a = 0; a < 3; ++a) m[a] = (double)M1[a] / dn;
  int k = 0;
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b, ++k) C[k] = ((double)M2[k] / dn - m[a] * m[b]) * inv2;
}

// lam0 when the ascending fp32 eigenvalues pass the floor and the two ratio tests (as products: no division), else 0
POINTOPS_ISS_HD float iss_saliency(const float (&lam)[3], float g21, float g32) {
  const bool floor_ok = lam[0] > 0x1p-20f * lam[2];  // below the resolution of the moments: rounding, not structure
  const bool r21 = lam[1] < g21 * lam[2];
  const bool r32 = lam[0] < g32 * lam[1];
  return floor_ok && r21 && r32 ? lam[0] : 0.0f;
}

// j suppresses i: the larger saliency wins, ties go to the lower index
POINTOPS_ISS_HD bool iss_beats(float s_j, int64_t j, float s_i, int64_t i) {
  return s_j > s_i || (s_j == s_i && j < i);
}

}  // namespace pointops

// feature_screen.h -- the scalar definitions of the feature-matching screen (feature_match.hip; C ABI:
// pointops_feature_knn, whose FEATURE MATCHING block in include/pointops_amd.h is the definition of the operator).
// __host__ __device__ and free of HIP types and of every other header of the library:
// tests/native/feature_screen_main.cpp compiles this header alone and holds the bound below to float64.
//
// The screen orders the targets of a query by the PRODUCT form of the squared distance, which the matrix cores compute
// (v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain):
//   n(a)   = fma(a_k, a_k, n)  k = 0 .. D-1 ascending, from 0.0f                              screen_norm
//   g(a,b) = fma(a_k, b_k, g)  k ascending from 0.0f; coordinates padded with zeros add nothing  screen_dot
//   s      = fl(fl(n1 + n2) - 2 g)                                                             screen_value
// The operator's distance is the reference's r = sum_k fl(fl(a_k - b_k)^2), an unfused fp32 sum in k order
// (exact_distance).  s and r differ, and this header bounds by how much:
//   |s - r| <= E = c(D) 2^-24 (n1 + n2max) + c(D) 2^-149, rounded upwards                      screen_bound
// with n2max the largest n2 of the query's cloud and c(D) = 4 D + 8 (screen_c).  The derivation ("Feature
// matching") is the standard model fl(x op y) = (x op y)(1 + d) + e, |d| <= u = 2^-24, |e| <= 2^-150 (e only for
// products), with N = |a|^2 + |b|^2:
//   |n1 + n2 - N| <= g_D N;  |2 g - 2 a.b| <= 2 g_D sum|a_k b_k| <= g_D N;  the two roundings of s add (3 + O(D u)) u N;
//   |r - d^2| <= g_{D+2} d^2 <= 2 g_{D+2} N  (d^2 <= 2 N);   g_k = k u / (1 - k u)
// so |s - r| <= (4 D + 7 + O(D^2 u)) u N, and N <= (n1 + n2) / (1 - g_D) in the computed norms.  For D <= kScreenMaxDim
// = 256 every second-order term together is below 0.1 u N, which the eighth unit of c(D) covers.  The model needs no
// overflow anywhere: with fl(n1 + n2max) <= 2^126 every intermediate of s and of r stays below 2^128
// (|2 g| <= N (1 + g_D), r <= 2 N (1 + g_{D+2})).  A row outside that range, or with a norm that is not finite, is
// never certified (screen_row_finite).
//
// The certificate.  A lane keeps the M smallest (s, j) of the targets it sees; every target j it drops has
// (s_j, j) >= the M-th key, so s_j >= s_cut (the smallest M-th key over the lists of a query; +inf for a list that
// never filled) and r_j >= s_cut - E.  With r_K the K-th smallest exact distance among the collected targets,
//   fl(r_K + E) < s_cut   implies   r_K + E < s_cut   (rounding to nearest is monotone and s_cut is a float)
// hence r_j > r_K for every dropped j: the K nearest of the row are among the collected ones, and no tie crosses the
// cut because the comparison is strict (screen_certified).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define POINTOPS_SCREEN_HD __host__ __device__ inline
#else
#define POINTOPS_SCREEN_HD inline
#endif

namespace pointops {

constexpr int kScreenMaxDim = 256;  // the bound's derivation holds up to here (the kernel takes fewer: feature_match.hip)
constexpr int kScreenM = 8;         // keys per list
constexpr float kScreenMaxNorm = 8.507059173023462e37f;  // 2^126: above it an intermediate may overflow

POINTOPS_SCREEN_HD int screen_c(int D) { return 4 * D + 8; }

POINTOPS_SCREEN_HD float screen_norm(const float* a, int D) {
  float n = 0.0f;
  for (int k = 0; k < D; ++k) n = __builtin_fmaf(a[k], a[k], n);
  return n;
}

POINTOPS_SCREEN_HD float screen_dot(const float* a, const float* b, int D) {
  float g = 0.0f;
  for (int k = 0; k < D; ++k) g = __builtin_fmaf(a[k], b[k], g);
  return g;
}

// fl(fl(n1 + n2) - 2 g): 2 g is exact (or overflows with g), so these are two roundings whatever -ffp-contract says
POINTOPS_SCREEN_HD float screen_value(float n1, float n2, float g) {
  const float t = n1 + n2;
  const float g2 = g + g;
  return t - g2;
}

// the reference's squared distance: unfused, k ascending, from the first term
POINTOPS_SCREEN_HD float exact_distance(const float* a, const float* b, int D) {
  float acc = 0.0f;  // 0 + t == t: the same bits as starting from the first term
  for (int k = 0; k < D; ++k) {
    const float diff = a[k] - b[k];
    const float sq = diff * diff;
    acc = acc + sq;
  }
  return acc;
}

// E, rounded upwards: the float64 expression is exact up to 2^-52 relative (far inside the slack of c), the
// conversion to float rounds to nearest, and one step up repairs a conversion that went down
POINTOPS_SCREEN_HD float screen_bound(int D, float n1, float n2max) {
  const double c = (double)screen_c(D);
  const double rel = c * 5.9604644775390625e-08;     // c 2^-24
  const double abs_ = c * 1.401298464324817e-45;     // c 2^-149
  const double sum = (double)n1 + (double)n2max;
  const double prod = rel * sum;
  const double e = prod + abs_;
  float f = (float)e;
  if ((double)f < e) f = nextafterf(f, INFINITY);
  return f;
}

// whether the error model covers the row: finite norms, and no overflow in any intermediate
POINTOPS_SCREEN_HD bool screen_row_finite(int D, float n1, float n2max) {
  if (D > kScreenMaxDim) return false;
  const float t = n1 + n2max;
  return n1 >= 0.0f && n2max >= 0.0f && t <= kScreenMaxNorm;  // (a NaN fails every comparison)
}

// The certificate of one row.  `len2`: targets of its cloud; rK: the K-th smallest exact distance among the targets
// the lists hold; s_cut: the smallest M-th key of the lists (+inf for a list that never filled).  A cloud of up to M
// targets is collected whole.
POINTOPS_SCREEN_HD bool screen_certified(int D, float n1, float n2max, int len2, float rK, float E, float s_cut) {
  if (!screen_row_finite(D, n1, n2max)) return false;
  if (len2 <= kScreenM) return true;
  const float lhs = rK + E;
  return lhs < s_cut;
}

}  // namespace pointops

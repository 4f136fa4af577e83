// iss_saliency_main.cpp -- csrc/iss_saliency.h on the host, compiled alone (no HIP header, no kernel, no GPU).
//
//   iss_scale       s = 2^(19 - e), e the smallest integer with rs <= 2^e: every power of two of the fp32 range, its two
//                   neighbours, subnormals and FLT_MAX, against a search for e that uses comparisons only
//   iss_quantize    round half to even at the half-way cases, sign symmetry, the largest offsets
//   iss_covariance  random int64 moments of up to 2^24 hits of |q| <= 2^19 against the same formula evaluated with
//                   __int128 numerators and long double: the double path may differ by the roundings it is defined
//                   with: M2 / n (half an ulp of 2^38: 2^-15), the two means and their product (3 * 2^-53 relative
//                   of 2^38: 3 * 2^-15), the difference (half an ulp of 2^39: 2^-14) -- 6 * 2^-15 < 2^-12 quanta^2; n = 0
//   iss_saliency    the truth table of the three tests, each failing alone, and their edges (equality fails)
//   iss_beats       the order: larger saliency, then lower index; irreflexive, total on distinct indices
// Prints "no violation" when everything holds; a line with VIOLATION and exit status 1 otherwise.
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>

#include "../../pytorch3d_pointops_amd/csrc/iss_saliency.h"

using namespace pointops;

static int violations = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      printf("VIOLATION: ");        \
      printf(__VA_ARGS__);          \
      printf("\n");                 \
      ++violations;                 \
    }                               \
  } while (0)

static int exponent_by_search(float rs) {
  int e = -160;
  while (!((double)rs <= ldexp(1.0, e))) ++e;  // comparisons in double: 2^e is exact there
  return e;
}

static void check_scale() {
  long n = 0;
  for (int k = -149; k <= 127; ++k) {
    const float p = ldexpf(1.0f, k);
    const float around[3] = {nextafterf(p, 0.0f), p, nextafterf(p, INFINITY)};
    for (float rs : around) {
      if (!(rs > 0.0f) || rs > FLT_MAX) continue;
      const int e = exponent_by_search(rs);
      CHECK(iss_scale(rs) == ldexp(1.0, 19 - e), "iss_scale(%a) = %a, want 2^%d", rs, iss_scale(rs), 19 - e);
      ++n;
    }
  }
  CHECK(iss_scale(FLT_MAX) == ldexp(1.0, 19 - 128), "iss_scale(FLT_MAX)");
  CHECK(iss_scale(1.0f) == 524288.0 && iss_scale(0.05f) == ldexp(1.0, 23) && iss_scale(0.08f) == ldexp(1.0, 22),
        "iss_scale at the documented radii");
  std::mt19937 rng(1);
  std::uniform_int_distribution<uint32_t> bits(1, 0x7f7fffffu);
  for (int i = 0; i < 200000; ++i, ++n) {
    const uint32_t u = bits(rng);
    float rs;
    memcpy(&rs, &u, 4);
    CHECK(iss_scale(rs) == ldexp(1.0, 19 - exponent_by_search(rs)), "iss_scale(%a)", rs);
  }
  printf("iss_scale: %ld radii\n", n);
}

static void check_quantize() {
  const double s = iss_scale(1.0f);  // 2^19
  // offsets k / 2^20 are exact fp32 differences from 0: odd k is a half-way case
  for (int k = -64; k <= 64; ++k) {
    const float x = ldexpf((float)k, -20);
    const int want = (k % 2 == 0) ? k / 2 : ((k - 1) / 2 % 2 == 0 ? (k - 1) / 2 : (k + 1) / 2);
    CHECK(iss_quantize(x, 0.0f, s) == want, "iss_quantize(%d / 2^20) = %d, want %d", k, iss_quantize(x, 0.0f, s), want);
    CHECK(iss_quantize(0.0f, x, s) == -want, "iss_quantize is odd at %d / 2^20", k);
  }
  CHECK(iss_quantize(0.5f, 0.0f, s) == 262144 && iss_quantize(1.0f, 0.0f, s) == 524288, "whole quanta");
  CHECK(iss_quantize(nextafterf(1.0f, 2.0f), 0.0f, s) == 524288, "an offset of rs (1 + 2^-23)");
  CHECK(iss_quantize(-1.0f, 0.25f, s) == -655360, "negative offsets");
  // the difference is formed in double: 1 - 2^-30 is not an fp32 difference of its operands, but is exact in double
  CHECK(iss_quantize(1.0f, ldexpf(1.0f, -30), ldexp(1.0, 30)) == (1 << 30) - 1, "the subtraction is in double");
  printf("iss_quantize: half-way cases hold\n");
}

static void check_covariance() {
  std::mt19937_64 rng(2);
  const int pair[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
  double worst = 0.0;
  for (int trial = 0; trial < 200000; ++trial) {
    // moments of n hits: M1 and M2 consistent with SOME sample would be ideal; the formula is checked on any integers
    // in range, which covers them
    const int64_t n = 1 + (int64_t)(rng() % (trial % 3 == 0 ? (1u << 24) : 4096u));
    const int64_t qmax = (int64_t)1 << 19;
    int64_t M1[3], M2[6];
    for (int a = 0; a < 3; ++a) M1[a] = (int64_t)(rng() % (uint64_t)(2 * n * qmax + 1)) - n * qmax;
    for (int k = 0; k < 6; ++k) {
      const uint64_t top = (uint64_t)n * (uint64_t)(qmax * qmax);
      M2[k] = (int64_t)(rng() % (top + 1));
      if (pair[k][0] != pair[k][1] && (rng() & 1)) M2[k] = -M2[k];
    }
    const int ebits = (int)(rng() % 60) - 30;
    const double s = ldexp(1.0, ebits);
    double C[6];
    iss_covariance(M1, M2, n, s, C);
    for (int k = 0; k < 6; ++k) {
      // exact: (M2 n - M1a M1b) / n^2, numerator in __int128 (|.| < 2^63 * 2^24 + 2^87)
      const __int128 num = (__int128)M2[k] * n - (__int128)M1[pair[k][0]] * M1[pair[k][1]];
      const long double exact = (long double)num / ((long double)n * (long double)n);
      const double got_q = C[k] * s * s;  // back in quantum units: exact scaling
      const double err = (double)fabsl((long double)got_q - exact);
      if (err > worst) worst = err;
      CHECK(err <= ldexp(1.0, -12), "iss_covariance: entry %d off by %g quanta^2 (n = %lld)", k, err, (long long)n);
    }
  }
  const int64_t z1[3] = {5, -7, 9}, z2[6] = {1, 2, 3, 4, 5, 6};
  double C[6] = {1, 1, 1, 1, 1, 1};
  iss_covariance(z1, z2, 0, 1024.0, C);
  for (int k = 0; k < 6; ++k) CHECK(C[k] == 0.0, "n = 0 gives C = 0");
  // the overflow edge: 2^24 hits of |q| = 2^19, half at +q and half at -q in x
  const int64_t e1[3] = {0, 0, 0}, e2[6] = {(int64_t)1 << 62, 0, 0, 0, 0, 0};
  iss_covariance(e1, e2, (int64_t)1 << 24, ldexp(1.0, 19), C);
  CHECK(C[0] == 1.0 && C[3] == 0.0 && C[1] == 0.0, "the 2^62 moment");
  printf("iss_covariance: worst error %.3g quanta^2 (bound 2^-12 = %.3g)\n", worst, ldexp(1.0, -12));
}

static void check_saliency_and_order() {
  const float g = 0.975f;
  const float ok[3] = {1.0f, 2.0f, 4.0f};
  CHECK(iss_saliency(ok, g, g) == 1.0f, "a salient triple");
  const float plane[3] = {1e-7f, 2.0f, 4.0f};  // below the floor 2^-20 * 4 = 3.8e-6
  CHECK(iss_saliency(plane, g, g) == 0.0f, "the floor");
  const float at_floor[3] = {0x1p-18f, 2.0f, 4.0f};  // l0 == 2^-20 l2: equality fails
  CHECK(iss_saliency(at_floor, g, g) == 0.0f, "the floor is strict");
  const float over_floor[3] = {0x1.000002p-18f, 2.0f, 4.0f};
  CHECK(iss_saliency(over_floor, g, g) == over_floor[0], "just above the floor");
  const float r21[3] = {1.0f, 3.95f, 4.0f};  // l1 / l2 = 0.9875 > 0.975
  CHECK(iss_saliency(r21, g, g) == 0.0f, "gamma_21");
  const float r32[3] = {1.99f, 2.0f, 4.0f};
  CHECK(iss_saliency(r32, g, g) == 0.0f, "gamma_32");
  const float eq[3] = {2.0f, 2.0f, 2.0f};
  CHECK(iss_saliency(eq, 1.0f, 1.0f) == 0.0f, "gamma = 1: equal eigenvalues fail (strict)");
  CHECK(iss_saliency(ok, 1e-3f, 1e-3f) == 0.0f && iss_saliency(ok, 1.0f, 1.0f) == 1.0f, "gamma = 1e-3 and 1");
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  CHECK(iss_saliency(zero, g, g) == 0.0f, "the zero matrix");
  const float neg[3] = {-1e-12f, 1e-13f, 1.0f};
  CHECK(iss_saliency(neg, g, g) == 0.0f, "a negative rounding residue");
  const float allneg[3] = {-3e-12f, -2e-12f, -1e-12f};
  CHECK(iss_saliency(allneg, g, g) == 0.0f, "all negative");
  // the order
  CHECK(iss_beats(2.0f, 9, 1.0f, 3) && !iss_beats(1.0f, 3, 2.0f, 9), "the larger saliency wins");
  CHECK(iss_beats(1.0f, 3, 1.0f, 9) && !iss_beats(1.0f, 9, 1.0f, 3), "ties to the lower index");
  CHECK(!iss_beats(1.0f, 5, 1.0f, 5), "nobody beats themselves");
  CHECK(iss_beats(0.0f, 0, 0.0f, 1) && !iss_beats(0.0f, 1, 0.0f, 0), "zeros order by index too");
  std::mt19937 rng(3);
  for (int t = 0; t < 100000; ++t) {
    const float a = (float)(rng() % 4), b = (float)(rng() % 4);
    const int64_t i = rng() % 8, j = rng() % 8;
    if (i != j) CHECK(iss_beats(a, i, b, j) != iss_beats(b, j, a, i), "exactly one of two distinct points beats the other");
  }
  printf("iss_saliency, iss_beats: truth tables hold\n");
}

int main() {
  check_scale();
  check_quantize();
  check_covariance();
  check_saliency_and_order();
  if (violations) {
    printf("%d VIOLATION(s)\n", violations);
    return 1;
  }
  printf("no violation\n");
  return 0;
}

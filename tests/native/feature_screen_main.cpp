// feature_screen_main.cpp -- csrc/feature_screen.h on the host, compiled alone (no HIP header, no kernel, no GPU).
//
//   bound      |s - r| <= E over several million pairs, s = screen_value(screen_norm, screen_norm, screen_dot) and
//              r = exact_distance, for every pair whose row passes screen_row_finite: D in {1, 2, 33, 128}; ordinary
//              rows, near-duplicates of large norm (s is all cancellation), rows far from the origin, subnormal
//              coordinates, coordinates whose squares underflow, huge but finite coordinates (norms up to 2^126), and
//              mixed magnitudes; E from the pair's own n2 (the tightest n2max a cloud can have) and from a larger one
//   float64    both sides against the squared distance in float64: |s - d2| <= E and |r - d2| <= E, and E itself is not
//              below its float64 expression c 2^-24 (n1 + n2max) + c 2^-149
//   overflow   rows that fail screen_row_finite are never certified, whatever the lists hold
//   predicate  screen_certified on hand-made lists: clouds of up to M targets, the strict comparison, the sum that
//              rounds down onto the cut, lists that never filled, norms that are not finite
// Prints "no violation" when everything holds; a line with VIOLATION and exit status 1 otherwise.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../../pytorch3d_pointops_amd/csrc/feature_screen.h"

using namespace pointops;

static int violations = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      if (violations < 20) {        \
        printf("VIOLATION: ");      \
        printf(__VA_ARGS__);        \
        printf("\n");               \
      }                             \
      ++violations;                 \
    }                               \
  } while (0)

static const char* kModes[] = {"normal", "near-duplicate", "offset", "subnormal", "underflow", "huge", "mixed"};
constexpr int kModeCount = 7;

static void draw_pair(std::mt19937& rng, int mode, int D, float* a, float* b) {
  std::normal_distribution<float> g(0.0f, 1.0f);
  std::uniform_int_distribution<int> e(-40, 40);
  for (int k = 0; k < D; ++k) {
    switch (mode) {
      case 0: a[k] = g(rng), b[k] = g(rng); break;
      case 1: a[k] = 1000.0f * g(rng), b[k] = a[k] + ldexpf(g(rng), -12 + e(rng) / 8); break;
      case 2: a[k] = 1000.0f + g(rng), b[k] = 1000.0f + g(rng); break;
      case 3: a[k] = ldexpf(g(rng), -140), b[k] = ldexpf(g(rng), -141); break;
      case 4: a[k] = ldexpf(g(rng), -70), b[k] = ldexpf(g(rng), -75); break;
      case 5: a[k] = ldexpf(g(rng), 58), b[k] = ldexpf(g(rng), 57); break;
      default: a[k] = ldexpf(g(rng), e(rng)), b[k] = ldexpf(g(rng), e(rng)); break;
    }
  }
}

static long check_bound(std::mt19937& rng, int D, int mode, long pairs, long* covered) {
  std::vector<float> a((size_t)D), b((size_t)D);
  for (long p = 0; p < pairs; ++p) {
    draw_pair(rng, mode, D, a.data(), b.data());
    const float n1 = screen_norm(a.data(), D), n2 = screen_norm(b.data(), D);
    const float s = screen_value(n1, n2, screen_dot(a.data(), b.data(), D));
    const float r = exact_distance(a.data(), b.data(), D);
    double d2 = 0.0;
    for (int k = 0; k < D; ++k) {
      const double diff = (double)a[k] - (double)b[k];
      d2 += diff * diff;
    }
    for (int wider = 0; wider < 2; ++wider) {
      const float n2max = wider ? n2 * 3.0f + 1.0f : n2;
      if (!screen_row_finite(D, n1, n2max)) {
        CHECK(!screen_certified(D, n1, n2max, 100, 0.0f, 0.0f, INFINITY), "D %d %s: a row out of range is certified", D,
              kModes[mode]);
        continue;
      }
      ++*covered;
      const float E = screen_bound(D, n1, n2max);
      const double c = (double)screen_c(D);
      CHECK((double)E >= c * ldexp(1.0, -24) * ((double)n1 + (double)n2max) + c * ldexp(1.0, -149) && isfinite(E),
            "D %d %s: E = %a is below its float64 expression (n1 %a n2max %a)", D, kModes[mode], E, n1, n2max);
      CHECK(fabs((double)s - (double)r) <= (double)E, "D %d %s: |s - r| = %a above E = %a (s %a r %a)", D, kModes[mode],
            fabs((double)s - (double)r), E, s, r);
      CHECK(fabs((double)s - d2) <= (double)E, "D %d %s: |s - d2| = %a above E = %a", D, kModes[mode],
            fabs((double)s - d2), E);
      CHECK(fabs((double)r - d2) <= (double)E, "D %d %s: |r - d2| = %a above E = %a", D, kModes[mode],
            fabs((double)r - d2), E);
    }
  }
  return pairs;
}

static void check_predicate() {
  const int D = 33;
  const float up1 = nextafterf(1.0f, 2.0f);
  CHECK(screen_c(33) == 140 && screen_c(1) == 12 && screen_c(128) == 520, "c(D) = 4 D + 8");
  // a cloud of up to M targets is collected whole: certified whatever the cut says
  CHECK(screen_certified(D, 1.0f, 1.0f, kScreenM, 5.0f, 1.0f, 0.0f), "M targets");
  CHECK(screen_certified(D, 1.0f, 1.0f, 1, INFINITY, 1.0f, 0.0f), "one target, no K-th distance");
  CHECK(!screen_certified(D, 1.0f, 1.0f, kScreenM + 1, 5.0f, 1.0f, 0.0f), "M + 1 targets need the comparison");
  // strict: a dropped target may tie the K-th
  CHECK(!screen_certified(D, 1.0f, 1.0f, 100, 1.0f, 0.0f, 1.0f), "r_K + E == s_cut is not certified");
  CHECK(screen_certified(D, 1.0f, 1.0f, 100, 1.0f, 0.0f, up1), "one ulp of room is");
  CHECK(!screen_certified(D, 1.0f, 1.0f, 100, 0.75f, 0.25f, 1.0f), "exact sum on the cut");
  // 1 + 2^-25 rounds DOWN to 1: the true sum is above the cut, the rounded one is not below it
  CHECK(!screen_certified(D, 1.0f, 1.0f, 100, 1.0f, ldexpf(1.0f, -25), 1.0f), "a sum that rounds down onto the cut");
  CHECK(screen_certified(D, 1.0f, 1.0f, 100, 1.0f, ldexpf(1.0f, -25), up1), "the same sum below the next float");
  // lists that never filled: the cut is +inf
  CHECK(screen_certified(D, 1.0f, 1.0f, 9, 3.0f, 0.5f, INFINITY), "an infinite cut certifies a finite row");
  CHECK(!screen_certified(D, 1.0f, 1.0f, 9, INFINITY, 0.5f, INFINITY), "not a row without a finite K-th distance");
  // norms that are not finite, or too large for the model; a NaN anywhere
  CHECK(!screen_certified(D, NAN, 1.0f, 3, 0.0f, 0.0f, INFINITY), "NaN n1, even with three targets");
  CHECK(!screen_certified(D, 1.0f, NAN, 100, 0.0f, 0.0f, INFINITY), "NaN n2max");
  CHECK(!screen_certified(D, INFINITY, 1.0f, 100, 0.0f, 0.0f, INFINITY), "infinite n1");
  CHECK(!screen_certified(D, 1.0f, INFINITY, 3, 0.0f, 0.0f, INFINITY), "infinite n2max");
  CHECK(!screen_certified(D, kScreenMaxNorm, kScreenMaxNorm, 100, 0.0f, 0.0f, INFINITY), "n1 + n2max above 2^126");
  CHECK(screen_certified(D, kScreenMaxNorm / 2, kScreenMaxNorm / 2, 100, 0.0f, 1.0f, INFINITY), "exactly 2^126");
  CHECK(!screen_certified(D, 1.0f, 1.0f, 100, NAN, 0.0f, INFINITY), "NaN r_K");
  CHECK(!screen_certified(D, 1.0f, 1.0f, 100, 0.0f, NAN, INFINITY), "NaN E");
  CHECK(!screen_certified(D, 1.0f, 1.0f, 100, 0.0f, 0.0f, NAN), "NaN cut");
  CHECK(!screen_certified(kScreenMaxDim + 1, 1.0f, 1.0f, 3, 0.0f, 0.0f, INFINITY), "D above the derivation's range");
  // E: upwards, never zero, monotone in the norms
  CHECK(screen_bound(D, 0.0f, 0.0f) > 0.0f, "E of zero rows is the underflow term");
  CHECK(screen_bound(D, 1.0f, 2.0f) >= (float)(140.0 * 3.0 * ldexp(1.0, -24)), "E(1, 2)");
  CHECK(screen_bound(D, 1.0f, 2.0f) <= screen_bound(D, 1.0f, 2.5f), "E is monotone");
  CHECK(isfinite(screen_bound(128, kScreenMaxNorm / 2, kScreenMaxNorm / 2)), "E is finite at the largest norms");
}

int main() {
  check_predicate();
  std::mt19937 rng(20250611);
  long pairs = 0, covered = 0;
  const int dims[] = {1, 2, 33, 128};
  const long per_mode[] = {200000, 200000, 40000, 10000};  // (the host's fmaf is a library call: fewer long rows)
  for (int i = 0; i < 4; ++i)
    for (int mode = 0; mode < kModeCount; ++mode) pairs += check_bound(rng, dims[i], mode, per_mode[i], &covered);
  printf("%ld pairs, %ld bounds checked\n", pairs, covered);
  CHECK(pairs >= 3000000 && covered >= pairs, "fewer pairs covered than meant: %ld of %ld", covered, pairs);
  if (violations) {
    printf("%d VIOLATION(s)\n", violations);
    return 1;
  }
  printf("no violation\n");
  return 0;
}

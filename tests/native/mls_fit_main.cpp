// mls_fit_main.cpp -- csrc/mls_fit.h on the host (no kernel, no GPU); the eigenvectors come from csrc/small_solvers.h as
// in the kernel.
//
//   mls_scale       s = 2^(15 - e), e the smallest integer with r <= 2^e: every power of two of the fp32 range, its two
//                   neighbours, subnormals and FLT_MAX, against a search for e that uses comparisons only
//   mls_weight      against the same chain with every fp32 operation formed in double and rounded once (double holds
//                   the quotient, difference and products of two floats to more than 2 * 24 + 2 bits, so that IS the
//                   correctly rounded fp32 operation: a fused or approximate division in the build shows here), and
//                   against the real quartic in long double: the chain's error before the final rounding is below
//                   2^12 * 10 * 2^-25 < 2^-9 quanta.  wq = 4096 at d2 = 0, wq = 0 next to r2, never outside [0, 4096],
//                   never increasing in d2.
//   mls_accumulate  random supports against __int128 sums; 2^20 terms of wq = 4096 and |q| = 2^15, the largest the
//                   definition admits, reach 2^62 exactly and the covariance of that support is (2^15 / s)^2
//   fit             random supports: delta against M1 / W / s in long double; C (iss_covariance with W for n) against
//                   __int128 numerators over long double; the eigenpair (l0, n) satisfies C n = l0 n to 1e-12 l2 and
//                   |n| = 1 to 1e-14; the sign rule; p against x + h n^ (n^ = fl32(n), the returned normal) in long
//                   double within half an ulp of p and the fp64 roundings of h's three terms;
//                   curvature against long double; a support below min_neighbors is status 1, a collinear one status 2,
//                   a planar one is projected onto its plane
// Prints "no violation" when everything holds; a line with VIOLATION and exit status 1 otherwise.
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>

#include "../../pytorch3d_pointops_amd/csrc/mls_fit.h"
#include "../../pytorch3d_pointops_amd/csrc/small_solvers.h"

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

static int exponent_by_search(float r) {
  int e = -160;
  while (!((double)r <= ldexp(1.0, e))) ++e;  // comparisons in double: 2^e is exact there
  return e;
}

static void check_scale() {
  long n = 0;
  for (int k = -149; k <= 127; ++k) {
    const float p = ldexpf(1.0f, k);
    const float around[3] = {nextafterf(p, 0.0f), p, nextafterf(p, INFINITY)};
    for (float r : around) {
      if (!(r > 0.0f) || r > FLT_MAX) continue;
      const int e = exponent_by_search(r);
      CHECK(mls_scale(r) == ldexp(1.0, 15 - e), "mls_scale(%a) = %a, want 2^%d", r, mls_scale(r), 15 - e);
      ++n;
    }
  }
  CHECK(mls_scale(FLT_MAX) == ldexp(1.0, 15 - 128), "mls_scale(FLT_MAX)");
  CHECK(mls_scale(1.0f) == 32768.0 && mls_scale(0.3f) == ldexp(1.0, 16) && mls_scale(0.15f) == ldexp(1.0, 17),
        "mls_scale at the documented radii");
  printf("mls_scale: %ld radii\n", n);
}

static int64_t weight_by_double(float d2, float r2) {
  const float t = (float)((double)d2 / (double)r2);
  const float u = (float)(1.0 - (double)t);
  float w = (float)((double)u * (double)u);
  w = (float)((double)w * (double)w);
  return (int64_t)llrint((double)w * 4096.0);
}

static void check_weight() {
  std::mt19937 rng(4);
  std::uniform_real_distribution<float> unit(0.0f, 1.0f);
  double worst = 0.0;
  for (int trial = 0; trial < 400000; ++trial) {
    const float r = ldexpf(0.5f + 0.5f * unit(rng), (int)(rng() % 40) - 20);
    const float r2 = r * r;
    const float frac = trial % 4 == 0 ? 1.0f - ldexpf(unit(rng), -(int)(rng() % 20)) : unit(rng);
    float d2 = r2 * frac;
    if (!(d2 < r2)) d2 = nextafterf(r2, 0.0f);
    const int32_t wq = mls_weight(d2, r2);
    CHECK(wq >= 0 && wq <= 4096, "mls_weight(%a, %a) = %d outside [0, 4096]", d2, r2, wq);
    CHECK(wq == weight_by_double(d2, r2), "mls_weight(%a, %a) = %d, the correctly rounded chain gives %lld", d2, r2, wq,
          (long long)weight_by_double(d2, r2));
    const long double u = 1.0L - (long double)d2 / (long double)r2;
    const long double exact = 4096.0L * u * u * u * u;
    const double err = (double)fabsl((long double)wq - exact);
    if (err > worst) worst = err;
    CHECK(err <= 0.5 + ldexp(1.0, -9), "mls_weight(%a, %a) = %d, the quartic is %Lg", d2, r2, wq, exact);
    const float d2b = nextafterf(d2, r2);
    if (d2b < r2) CHECK(mls_weight(d2b, r2) <= wq, "mls_weight increases at %a / %a", d2, r2);
  }
  for (int k = -60; k <= 60; k += 3) {
    const float r2 = ldexpf(1.25f, k);
    CHECK(mls_weight(0.0f, r2) == 4096, "wq = 4096 at d2 = 0 (r2 = %a)", r2);
    CHECK(mls_weight(nextafterf(r2, 0.0f), r2) == 0, "wq = 0 next to r2 = %a", r2);
  }
  CHECK(mls_weight(0.0f, INFINITY) == 4096 && mls_weight(1e30f, INFINITY) == 4096, "r2 = inf: every finite hit weighs 1");
  CHECK(mls_weight(0.5f, 1.0f) == 256 && mls_weight(0.25f, 1.0f) == 1296, "(1/2)^4 and (3/4)^4 of 4096");
  printf("mls_weight: worst distance to the quartic %.6f quanta (bound 0.5 + 2^-9)\n", worst);
}

static void check_accumulate() {
  std::mt19937_64 rng(5);
  for (int trial = 0; trial < 20000; ++trial) {
    const int n = 1 + (int)(rng() % 64);
    MlsSums a;
    __int128 W = 0, M1[3] = {0, 0, 0}, M2[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
      const int32_t w = (int32_t)(rng() % 4097);
      int32_t q[3];
      for (int c = 0; c < 3; ++c) q[c] = (int32_t)(rng() % 65537) - 32768;
      mls_accumulate(a, w, q[0], q[1], q[2]);
      W += w;
      int k = 0;
      for (int c = 0; c < 3; ++c) {
        M1[c] += (__int128)w * q[c];
        for (int d = c; d < 3; ++d, ++k) M2[k] += (__int128)w * q[c] * q[d];
      }
    }
    bool same = a.n == n && (__int128)a.W == W;
    for (int c = 0; c < 3; ++c) same = same && (__int128)a.M1[c] == M1[c];
    for (int k = 0; k < 6; ++k) same = same && (__int128)a.M2[k] == M2[k];
    CHECK(same, "mls_accumulate differs from the __int128 sums (trial %d)", trial);
  }
  // the overflow edge: 2^20 hits of wq = 2^12 and |q| = 2^15, half at +q and half at -q in x
  MlsSums e;
  for (int i = 0; i < (1 << 20); ++i) mls_accumulate(e, 4096, i % 2 ? 32768 : -32768, 0, 0);
  CHECK(e.n == (1 << 20) && e.W == ((int64_t)1 << 32) && e.M1[0] == 0 && e.M2[0] == ((int64_t)1 << 62),
        "2^20 maximal terms: W = %lld, M2xx = %lld", (long long)e.W, (long long)e.M2[0]);
  double C[6];
  iss_covariance(e.M1, e.M2, e.W, ldexp(1.0, 15), C);
  CHECK(C[0] == 1.0 && C[1] == 0.0 && C[3] == 0.0, "the covariance of the 2^62 moment");
  MlsSums g;
  for (int i = 0; i < (1 << 20); ++i) mls_accumulate(g, 4096, 32768, -32768, 32768);
  CHECK(g.M2[1] == -((int64_t)1 << 62) && g.M1[1] == -((int64_t)1 << 47), "2^20 maximal negative terms");
  printf("mls_accumulate: sums hold up to 2^62\n");
}

struct Fit {
  uint8_t status;
  double C[6], l[3], v[3][3], delta[3];
  float p[3], n[3], curv;
};

static Fit fit(const MlsSums& a, const float (&x)[3], double s, int64_t min_neighbors) {
  Fit f{};
  double m[3][3];
  iss_covariance(a.M1, a.M2, a.W, s, f.C);
  m[0][0] = f.C[0], m[0][1] = m[1][0] = f.C[1], m[0][2] = m[2][0] = f.C[2];
  m[1][1] = f.C[3], m[1][2] = m[2][1] = f.C[4], m[2][2] = f.C[5];
  sym3_eigen_f64(m, f.l, f.v);
  f.status = mls_status(a.n, min_neighbors, f.l);
  mls_offset(a.M1, a.W, s, f.delta);
  for (int c = 0; c < 3; ++c) f.p[c] = x[c];
  if (f.status == 0) mls_project(x, f.delta, f.l, f.v, f.p, f.n, f.curv);
  return f;
}

static void check_fit() {
  std::mt19937_64 rng(6);
  std::uniform_real_distribution<float> coord(-2.0f, 2.0f);
  const int pair[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
  long fitted = 0;
  double worst_c = 0.0, worst_res = 0.0;
  for (int trial = 0; trial < 100000; ++trial) {
    const int n = 3 + (int)(rng() % 40);
    const double s = ldexp(1.0, (int)(rng() % 40) - 10);
    const int32_t span = trial % 5 == 0 ? 32768 : 1 + (int32_t)(rng() % 32768);
    const int32_t thin = trial % 3 == 0 ? 1 + (int32_t)(rng() % 64) : span;  // flat supports: a surface with noise
    MlsSums a;
    for (int i = 0; i < n; ++i) {
      const int32_t w = i == 0 ? 4096 : (int32_t)(rng() % 4097);
      mls_accumulate(a, w, i == 0 ? 0 : (int32_t)(rng() % (2 * span + 1)) - span,
                     i == 0 ? 0 : (int32_t)(rng() % (2 * span + 1)) - span,
                     i == 0 ? 0 : (int32_t)(rng() % (2 * thin + 1)) - thin);
    }
    const float x[3] = {coord(rng), coord(rng), coord(rng)};
    const Fit f = fit(a, x, s, 3);
    for (int c = 0; c < 3; ++c) {
      const long double want = (long double)a.M1[c] / (long double)a.W / (long double)s;
      CHECK(fabsl((long double)f.delta[c] - want) <= 2 * DBL_EPSILON * fabsl(want), "delta[%d] = %a, want %La", c,
            f.delta[c], want);
    }
    for (int k = 0; k < 6; ++k) {
      const int u = pair[k][0], v = pair[k][1];
      const __int128 num = (__int128)a.M2[k] * a.W - (__int128)a.M1[u] * a.M1[v];
      const long double exact = (long double)num / ((long double)a.W * (long double)a.W);
      // the roundings of the definition: M2 / W, the two means, their product, the difference -- each half an ulp of a
      // value of at most max(span, thin)^2 quanta^2
      const long double widest = span > thin ? span : thin, scale2 = widest * widest;
      const double err = (double)(fabsl((long double)(f.C[k] * s * s) - exact) / scale2);
      if (err > worst_c) worst_c = err;
      CHECK(err <= 8 * DBL_EPSILON, "C[%d] off by %g of span^2", k, err);
    }
    CHECK(f.l[0] <= f.l[1] && f.l[1] <= f.l[2], "eigenvalues ascend");
    if (f.status != 0) {
      CHECK(f.p[0] == x[0] && f.p[1] == x[1] && f.p[2] == x[2] && f.n[0] == 0.0f && f.curv == 0.0f, "a status-%d row",
            f.status);
      continue;
    }
    ++fitted;
    // the eigenpair, from the sign-fixed fp64 normal recovered as column 0 up to sign
    double nv[3] = {f.v[0][0], f.v[1][0], f.v[2][0]};
    int big = 0;
    for (int c = 1; c < 3; ++c)
      if (fabs(nv[c]) > fabs(nv[big])) big = c;
    if (nv[big] < 0.0)
      for (int c = 0; c < 3; ++c) nv[c] = -nv[c];
    const double Cm[3][3] = {{f.C[0], f.C[1], f.C[2]}, {f.C[1], f.C[3], f.C[4]}, {f.C[2], f.C[4], f.C[5]}};
    double norm2 = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double res = fabs((Cm[r][0] * nv[0] + Cm[r][1] * nv[1] + Cm[r][2] * nv[2]) - f.l[0] * nv[r]) / f.l[2];
      if (res > worst_res) worst_res = res;
      CHECK(res <= 1e-12, "C n - l0 n = %g l2", res);
      norm2 += nv[r] * nv[r];
      CHECK(f.n[r] == (float)nv[r], "normals = fl32(n), sign-fixed");
    }
    CHECK(fabs(norm2 - 1.0) <= 1e-14, "|n|^2 = 1 + %g", norm2 - 1.0);
    CHECK(nv[big] > 0.0 && f.n[big] > 0.0f, "the largest component is positive");
    // the point moves along the RETURNED normal n^ = fl32(n), widened exactly
    const double nh[3] = {(double)f.n[0], (double)f.n[1], (double)f.n[2]};
    const long double h = ((long double)f.delta[0] * nh[0] + (long double)f.delta[1] * nh[1]) + (long double)f.delta[2] * nh[2];
    const double terms = fabs(f.delta[0] * nh[0]) + fabs(f.delta[1] * nh[1]) + fabs(f.delta[2] * nh[2]);
    for (int c = 0; c < 3; ++c) {
      const long double want = (long double)x[c] + h * nh[c];
      const double ulp = (double)nextafterf(fabsf(f.p[c]), INFINITY) - (double)fabsf(f.p[c]);
      // (h is an fp64 sum of three products by definition: each term's rounding is part of the result)
      CHECK(fabsl((long double)f.p[c] - want) <= 0.5 * ulp + 4 * DBL_EPSILON * (terms + fabs((double)x[c])),
            "p[%d] = %a, want %La", c, f.p[c], want);
    }
    const long double curv = (long double)f.l[0] / ((long double)f.l[0] + f.l[1] + f.l[2]);
    CHECK(fabsl((long double)f.curv - curv) <= ldexp(1.0, -24) * fabsl(curv) + 1e-40L, "curvature = %a, want %La", f.curv, curv);
  }
  CHECK(fitted > 90000, "only %ld of the random supports were fitted", fitted);
  printf("fit: %ld supports; C within %.3g of span^2 (bound 8 eps), eigen residual %.3g l2 (bound 1e-12)\n", fitted,
         worst_c, worst_res);

  // the statuses
  const float x0[3] = {0.25f, -0.5f, 1.0f};
  MlsSums two;
  mls_accumulate(two, 4096, 0, 0, 0);
  mls_accumulate(two, 1000, 300, -200, 100);
  Fit f = fit(two, x0, 1024.0, 3);
  CHECK(f.status == 1 && f.p[0] == x0[0] && f.p[2] == x0[2] && f.n[1] == 0.0f && f.curv == 0.0f, "below min_neighbors");
  CHECK(fit(two, x0, 1024.0, 2).status == 2, "two points are a line");
  MlsSums line;
  for (int i = -20; i <= 20; ++i) mls_accumulate(line, 1 + (i + 20) * 100, 4 * i, 2 * i, i);
  f = fit(line, x0, 1024.0, 3);
  CHECK(f.status == 2 && f.p[1] == x0[1] && f.n[0] == 0.0f, "a collinear support (l1 = %g l2)", f.l[1] / f.l[2]);
  MlsSums same;
  for (int i = 0; i < 9; ++i) mls_accumulate(same, 4096, 0, 0, 0);
  CHECK(fit(same, x0, 1024.0, 3).status == 2, "coincident points");
  MlsSums none;
  CHECK(fit(none, x0, 1024.0, 0).status == 2 && fit(none, x0, 1024.0, 1).status == 1, "an empty support");
  MlsSums zero_weights;  // (cannot arise with the point itself in its support; the guard W > 0 still holds)
  for (int i = 0; i < 5; ++i) mls_accumulate(zero_weights, 0, 10 * i, i * i, 3);
  f = fit(zero_weights, x0, 1024.0, 3);
  CHECK(f.status == 2 && f.delta[0] == 0.0, "all weights zero");

  // a planar support: the lattice points of the plane x + y + z = 3 k around a point one step off it
  MlsSums plane;
  const int k = 5;
  for (int i = -6; i <= 6; ++i)
    for (int j = -6; j <= 6; ++j) mls_accumulate(plane, 1 + (i * i + 3 * j * j) % 97, 64 * i + k, 64 * j + k, -64 * (i + j) + k);
  const double s = 4096.0;
  f = fit(plane, x0, s, 3);
  CHECK(f.status == 0 && fabs(f.l[0]) <= 1e-12 * f.l[2] && fabsf(f.curv) <= 1e-12f, "a planar support: l0 = %g l2",
        f.l[0] / f.l[2]);
  const float inv_sqrt3 = 0.57735026918962576f;
  for (int c = 0; c < 3; ++c) {
    CHECK(fabsf(f.n[c] - inv_sqrt3) <= 1e-6f, "the plane's normal: n[%d] = %a", c, f.n[c]);
    CHECK(fabs((double)f.p[c] - ((double)x0[c] + k / s)) <= ldexp(1.0, -23), "onto the plane: p[%d] = %a", c, f.p[c]);
  }
  const double flip[3][3] = {{-0.6, 1, 0}, {0.6, 0, 1}, {-0.52915026221291817, 0, 0}};  // column 0 = (-0.6, 0.6, -0.529)
  const double dl[3] = {1.0, 2.0, 3.0}, dd[3] = {0.0, 0.0, 0.0};
  float pp[3], nn[3], cc;
  mls_project(x0, dd, dl, flip, pp, nn, cc);
  CHECK(nn[0] == 0.6f && nn[1] == -0.6f && nn[2] > 0.0f && pp[0] == x0[0], "a tie of magnitudes goes to the lower axis");
  CHECK(cc == (float)(1.0 / 6.0), "curvature 1 / 6");
  printf("statuses, planar support and sign rule hold\n");
}

int main() {
  check_scale();
  check_weight();
  check_accumulate();
  check_fit();
  if (violations) {
    printf("%d VIOLATION(s)\n", violations);
    return 1;
  }
  printf("no violation\n");
  return 0;
}

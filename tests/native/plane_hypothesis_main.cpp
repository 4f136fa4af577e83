// plane_hypothesis_main.cpp -- host check of csrc/plane_hypothesis.h (the per-lane routines of plane.hip) and of the
// fp64 eigen core sym3_eigen_f64 of csrc/small_solvers.h.  The functions are __host__ __device__: this program runs the
// host side of exactly the code the kernels run.  Launches no kernel; needs no GPU.  Prints the first violations and
// exits non-zero.
//
// Planes (u = 2^-24), 3M random triples at scales 1e-3, 1, 100, 1e3-offset, thin triangles included, with and without a
// cone:
//   ||n|^2 - 1| <= 4u  (a unit vector rounded to fp32: three entries off by at most u/2 |n_i| each, doubled by the
//   square, and the factor of about 2 over that);
//   |n.p_k + d| <= u (3 max|p| + |d|) for the three points  (the fp64 plane holds them to about 1e-10 |e| even for the
//   thinnest valid triangle; rounding n moves n.p by at most 1.5u max|p|, rounding d by u/2 |d|);
//   the sign rule holds on the fp32 plane; with a cone (n.A)^2 >= cos^2 - 4u.
//   Degenerate triples -- collinear and coincident points with integer coordinates (exactly degenerate), a repeated
//   point, NaN and infinite coordinates -- are invalid and leave the plane (0,0,0,0).
// Eigen core, in fp64, on chosen spectra under random rotations (generic, double, triple, rank 1, rank 2, zero):
//   l ascending; V^T V = I to 1e-14; V diag(l) V^T = C to 1e-14 max|C|.
// Refit: the moments of 5..200 points scattered on a random plane about a pivot 1e3 away from the origin recover the
//   plane: |n.n0| >= 1 - 1e-9 and the centroid on the plane to 1e-9; fewer than three points and NaN moments are refused.
// sym3_eigen: the wrapper over the core is bit-equal to the loop as it stood before the core was factored out (kept
//   below as sym3_eigen_before), on the matrix classes of small_solvers_main.cpp drawn from its seed, and on literals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../pytorch3d_pointops_amd/csrc/plane_hypothesis.h"

namespace {

using pointops::PlaneCone;

constexpr double kU32 = 5.9604644775390625e-08;  // 2^-24

uint64_t rng_state = 0x243F6A8885A308D3ull;  // (the seed of small_solvers_main.cpp)
uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uni() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }
double sym() { return 2.0 * uni() - 1.0; }
double gauss() {
  double u = uni(), v = uni();
  if (u < 1e-300) u = 1e-300;
  return sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v);
}
void rotation3(double (&q)[3][3]) {
  double w = gauss(), x = gauss(), y = gauss(), z = gauss();
  const double n = sqrt(w * w + x * x + y * y + z * z) + 1e-300;
  w /= n, x /= n, y /= n, z /= n;
  q[0][0] = 1 - 2 * (y * y + z * z), q[0][1] = 2 * (x * y - w * z), q[0][2] = 2 * (x * z + w * y);
  q[1][0] = 2 * (x * y + w * z), q[1][1] = 1 - 2 * (x * x + z * z), q[1][2] = 2 * (y * z - w * x);
  q[2][0] = 2 * (x * z - w * y), q[2][1] = 2 * (y * z + w * x), q[2][2] = 1 - 2 * (x * x + y * y);
}

int violations = 0;
void fail(const char* what, double got, double bound) {
  if (violations++ < 10) printf("VIOLATION %s: %.9g (bound %.9g)\n", what, got, bound);
}

PlaneCone no_cone() {
  PlaneCone c;
  c.use = 0;
  c.a[0] = c.a[1] = c.a[2] = c.cos_max = 0.0f;
  return c;
}

PlaneCone random_cone() {
  PlaneCone c;
  double a[3] = {gauss(), gauss(), gauss()};
  const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) + 1e-300;
  c.use = 1;
  for (int k = 0; k < 3; ++k) c.a[k] = (float)(a[k] / n);
  c.cos_max = (float)cos(1.5 * uni());
  return c;
}

bool is_zero(const float (&pl)[4]) { return pl[0] == 0.0f && pl[1] == 0.0f && pl[2] == 0.0f && pl[3] == 0.0f; }

long n_valid = 0, n_thrown = 0;
double worst_unit = 0.0, worst_on = 0.0;

void check_plane(const float (&p)[3][3], const PlaneCone& cone, bool must_be_valid) {
  float pl[4];
  const bool valid = pointops::ph_plane(p, cone, pl);
  if (!valid) {
    ++n_thrown;
    if (!is_zero(pl)) fail("invalid triple with a non-zero plane", pl[0], 0.0);
    if (must_be_valid) fail("a fat triangle was thrown out", 0.0, 0.0);
    return;
  }
  ++n_valid;
  const double n[3] = {pl[0], pl[1], pl[2]}, d = pl[3];
  const double unit = fabs(pointops::ph_sqnorm(n) - 1.0);
  worst_unit = fmax(worst_unit, unit / kU32);
  if (!(unit <= 4.0 * kU32)) fail("|n|^2 - 1", unit, 4.0 * kU32);
  double mp = 0.0;
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) mp = fmax(mp, fabs((double)p[k][a]));
  const double bound = kU32 * (3.0 * mp + fabs(d));
  for (int k = 0; k < 3; ++k) {
    const double r = fabs(n[0] * p[k][0] + n[1] * p[k][1] + n[2] * p[k][2] + d);
    if (bound > 0.0) worst_on = fmax(worst_on, r / bound);
    if (!(r <= bound)) fail("a sample point off its plane", r, bound);
  }
  if (cone.use) {
    const double dot = n[0] * cone.a[0] + n[1] * cone.a[1] + n[2] * cone.a[2];
    if (dot < -kU32) fail("the normal points against the axis", dot, 0.0);
    const double c2 = (double)cone.cos_max * cone.cos_max;
    if (!(dot * dot >= c2 - 4.0 * kU32)) fail("the normal is outside the cone", dot * dot, c2);
  } else {
    int k = 0;
    if (fabs(n[1]) > fabs(n[k])) k = 1;
    if (fabs(n[2]) > fabs(n[k])) k = 2;
    if (n[k] < 0.0) fail("the largest component of the normal is negative", n[k], 0.0);
  }
}

void check_planes() {
  for (int it = 0; it < 3000000; ++it) {
    const int kind = it % 6;
    const double scale = kind == 1 ? 1e-3 : (kind == 2 ? 100.0 : 1.0), offset = kind == 3 ? 1e3 : 0.0;
    float p[3][3];
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) p[k][a] = (float)(scale * sym() + offset);
    bool fat = kind != 3;  // (at the offset the fp32 grid is 6e-5: still a triangle, but its shape is not ours to promise)
    if (kind == 4) {       // a thin triangle: point 2 next to the line 0-1
      for (int a = 0; a < 3; ++a) p[2][a] = (float)(0.5 * ((double)p[0][a] + p[1][a]) + 1e-4 * gauss());
      fat = false;
    }
    if (fat) {  // sin of the angle at p0 >= 1e-3: a thousand times the validity test's floor
      double e1[3], e2[3];
      for (int a = 0; a < 3; ++a) e1[a] = (double)p[1][a] - p[0][a], e2[a] = (double)p[2][a] - p[0][a];
      const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      fat = pointops::ph_sqnorm(c) > 1e-6 * pointops::ph_sqnorm(e1) * pointops::ph_sqnorm(e2);
    }
    check_plane(p, no_cone(), fat);
    if (kind == 5) check_plane(p, random_cone(), false);
  }
}

void check_degenerate() {
  const float nan = NAN, inf = INFINITY;
  for (int it = 0; it < 600000; ++it) {
    const int kind = it % 6;
    float p[3][3];
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) p[k][a] = (float)((int)(next_u64() % 2001) - 1000);
    if (kind == 0)  // collinear, exactly: integers
      for (int a = 0; a < 3; ++a) p[2][a] = 2.0f * p[1][a] - p[0][a];
    if (kind == 1)  // coincident
      for (int k = 1; k < 3; ++k)
        for (int a = 0; a < 3; ++a) p[k][a] = p[0][a];
    if (kind == 2)  // a repeated point
      for (int a = 0; a < 3; ++a) p[(it / 6) % 2 + 1][a] = p[0][a];
    if (kind == 3) p[(it / 6) % 3][(it / 18) % 3] = nan;
    if (kind == 4) p[(it / 6) % 3][(it / 18) % 3] = (it / 54) % 2 ? inf : -inf;
    if (kind == 5)  // collinear along an axis at a huge scale
      for (int k = 0; k < 3; ++k) p[k][0] = 3e38f * (float)(k - 1), p[k][1] = p[k][2] = 0.0f;
    for (int c = 0; c < 2; ++c) {
      float pl[4];
      const bool valid = pointops::ph_plane(p, c ? random_cone() : no_cone(), pl);
      if (valid) fail("a degenerate triple is valid", (double)kind, 0.0);
      if (!is_zero(pl)) fail("a degenerate triple left a non-zero plane", (double)kind, 0.0);
    }
  }
}

// ------------------------------------------------------------------------------------------------ the eigen core
void compose(const double (&s)[3], double (&c)[3][3]) {
  double q[3][3];
  rotation3(q);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double v = 0.0;
      for (int k = 0; k < 3; ++k) v += q[a][k] * s[k] * q[b][k];
      c[a][b] = v;
    }
  for (int a = 0; a < 3; ++a)
    for (int b = a + 1; b < 3; ++b) c[b][a] = c[a][b];
}

double worst_orth = 0.0, worst_rec = 0.0;

void check_core() {
  for (int it = 0; it < 600000; ++it) {
    const int kind = it % 6;
    double s[3] = {0.05 + uni(), 0.05 + uni(), 0.05 + uni()};
    if (kind == 1) s[1] = s[0];
    if (kind == 2) s[1] = s[2] = s[0];
    if (kind == 3) s[1] = s[2] = 0.0;
    if (kind == 4) s[(it / 6) % 3] = 0.0;
    if (kind == 5) s[0] = s[1] = s[2] = 0.0;
    double c[3][3], a[3][3], l[3], v[3][3];
    compose(s, c);
    memcpy(a, c, sizeof(a));
    pointops::sym3_eigen_f64(a, l, v);
    if (!(l[0] <= l[1] && l[1] <= l[2])) fail("eigenvalues not ascending", l[0], l[2]);
    double cmax = 0.0, orth = 0.0, rec = 0.0;
    for (int p = 0; p < 3; ++p)
      for (int q = 0; q < 3; ++q) cmax = fmax(cmax, fabs(c[p][q]));
    for (int p = 0; p < 3; ++p)
      for (int q = 0; q < 3; ++q) {
        double g = 0.0, r = 0.0;
        for (int k = 0; k < 3; ++k) g += v[k][p] * v[k][q], r += v[p][k] * l[k] * v[q][k];
        orth = fmax(orth, fabs(g - (p == q ? 1.0 : 0.0)));
        rec = fmax(rec, fabs(r - c[p][q]));
      }
    worst_orth = fmax(worst_orth, orth);
    if (!(orth <= 1e-14)) fail("V^T V - I", orth, 1e-14);
    if (cmax > 0.0) worst_rec = fmax(worst_rec, rec / cmax);
    if (!(rec <= 1e-14 * cmax)) fail("V diag(l) V^T - C", rec, 1e-14 * cmax);
  }
}

void check_refit() {
  for (int it = 0; it < 200000; ++it) {
    double q[3][3];
    rotation3(q);
    const double n0[3] = {q[0][2], q[1][2], q[2][2]};
    const double origin[3] = {1e3 * sym(), 1e3 * sym(), 1e3 * sym()};
    const int count = 5 + (int)(next_u64() % 196);
    double pivot[3], mom[pointops::kPlaneMoments] = {0.0};
    double mean[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < count; ++i) {
      const double u = sym(), w = sym();
      double p[3];
      for (int a = 0; a < 3; ++a) p[a] = origin[a] + u * q[a][0] + w * q[a][1];
      if (i == 0) memcpy(pivot, p, sizeof(pivot));
      const double d[3] = {p[0] - pivot[0], p[1] - pivot[1], p[2] - pivot[2]};
      mom[0] += 1.0;
      mom[1] += d[0], mom[2] += d[1], mom[3] += d[2];
      mom[4] += d[0] * d[0], mom[5] += d[0] * d[1], mom[6] += d[0] * d[2];
      mom[7] += d[1] * d[1], mom[8] += d[1] * d[2], mom[9] += d[2] * d[2];
      for (int a = 0; a < 3; ++a) mean[a] += p[a] / count;
    }
    float pl[4];
    if (!pointops::ph_refit(mom, pivot, no_cone(), pl)) {
      fail("a refit of scattered points was refused", (double)count, 0.0);
      continue;
    }
    const double dot = fabs(pl[0] * n0[0] + pl[1] * n0[1] + pl[2] * n0[2]);
    if (!(dot >= 1.0 - 4.0 * kU32)) fail("refit normal", dot, 1.0);
    const double off = fabs(pl[0] * mean[0] + pl[1] * mean[1] + pl[2] * mean[2] + pl[3]);
    const double bound = kU32 * (3.0 * 1001.0 + fabs((double)pl[3]));
    if (!(off <= bound)) fail("refit: the centroid is off the plane", off, bound);
    // a cone that holds the true normal keeps the fit and turns it along the axis; the opposite cone refuses it
    PlaneCone cone;
    cone.use = 1;
    for (int a = 0; a < 3; ++a) cone.a[a] = (float)-n0[a];
    cone.cos_max = 0.99f;
    float turned[4];
    if (!pointops::ph_refit(mom, pivot, cone, turned)) fail("refit inside the cone refused", 0.0, 0.0);
    else if (!(turned[0] * cone.a[0] + turned[1] * cone.a[1] + turned[2] * cone.a[2] > 0.0f))
      fail("refit not turned along the axis", 0.0, 0.0);
    for (int a = 0; a < 3; ++a) cone.a[a] = (float)q[a][0];  // an axis in the plane
    if (pointops::ph_refit(mom, pivot, cone, turned) || !is_zero(turned)) fail("refit outside the cone kept", 0.0, 0.0);
  }
  float pl[4];
  const double pivot[3] = {0.0, 0.0, 0.0};
  double two[pointops::kPlaneMoments] = {2.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (pointops::ph_refit(two, pivot, no_cone(), pl) || !is_zero(pl)) fail("a refit of two points", 0.0, 0.0);
  double none[pointops::kPlaneMoments] = {0.0};
  if (pointops::ph_refit(none, pivot, no_cone(), pl) || !is_zero(pl)) fail("a refit of no point", 0.0, 0.0);
  double bad[pointops::kPlaneMoments] = {5.0, NAN, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
  if (pointops::ph_refit(bad, pivot, no_cone(), pl) || !is_zero(pl)) fail("a refit of NaN moments", 0.0, 0.0);
}

// ------------------------------------------------------------------------------------------------ sym3_eigen as it was
// The body of sym3_eigen before sym3_eigen_f64 was factored out of it, kept here word for word.
void sym3_eigen_before(const float (&c)[3][3], float (&lam)[3], float (&vec)[3][3]) {
  using namespace pointops;
  double a[3][3], v[3][3];
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) {
      a[r][q] = (double)c[r][q];
      v[r][q] = r == q ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kJacobiMaxSweeps; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (off <= kJacobiTol * diag) break;
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<1, 2>(a, v);
  }
  double l[3] = {a[0][0], a[1][1], a[2][2]};
  eig_order<0, 1>(l, v);
  eig_order<1, 2>(l, v);
  eig_order<0, 1>(l, v);
  for (int r = 0; r < 3; ++r) {
    lam[r] = (float)l[r];
    for (int q = 0; q < 3; ++q) vec[r][q] = (float)v[r][q];
  }
}

long n_same = 0;

void same_bits(const float (&c)[3][3]) {
  float l0[3], v0[3][3], l1[3], v1[3][3];
  sym3_eigen_before(c, l0, v0);
  pointops::sym3_eigen(c, l1, v1);
  ++n_same;
  if (memcmp(l0, l1, sizeof(l0)) != 0 || memcmp(v0, v1, sizeof(v0)) != 0) fail("sym3_eigen changed its bits", c[0][0], 0.0);
}

void check_sym3_unchanged() {
  const float literals[][3][3] = {
      {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}},
      {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}},
      {{3, 0, 0}, {0, 1, 0}, {0, 0, 2}},
      {{2, 1, 0}, {1, 2, 0}, {0, 0, 5}},
      {{1, 1, 1}, {1, 1, 1}, {1, 1, 1}},
      {{4, -2, 0.5f}, {-2, 3, 1.25f}, {0.5f, 1.25f, 6}},
      {{1e-30f, 1e-31f, 0}, {1e-31f, 2e-30f, 1e-32f}, {0, 1e-32f, 3e-30f}},
      {{1e30f, 1e29f, -1e28f}, {1e29f, 2e30f, 1e29f}, {-1e28f, 1e29f, 3e30f}},
      {{1.0f, 1e-7f, 0}, {1e-7f, 1.0f, 1e-7f}, {0, 1e-7f, 1.0f}},
      {{1e-45f, 0, 0}, {0, 1e-45f, 0}, {0, 0, 1e-45f}},
  };
  for (const auto& c : literals) same_bits(c);
  for (int it = 0; it < 500000; ++it) {
    const int kind = it % 8;
    double s[3] = {0.05 + uni(), 0.05 + uni(), 0.05 + uni()};
    if (kind == 1) s[1] = s[0];
    if (kind == 2) s[1] = s[2] = s[0];
    if (kind == 3) s[1] = s[2] = 0.0;
    if (kind == 4) s[2] = 0.0;
    if (kind == 5) s[1] = s[0] * (1.0 + 1e-7 * (0.5 + uni())), s[2] = s[0] * (1.0 + 2e-7 * (0.5 + uni()));
    if (kind == 6) s[1] = s[0] * pow(10.0, -12.0 * uni()), s[2] = s[0] * 1e-12;
    double c[3][3];
    compose(s, c);
    const double scale = kind == 7 ? ldexp(1.0, (it / 8) % 2 ? 100 : -100) : 1.0;
    float cf[3][3];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) cf[a][b] = (float)(scale * c[a][b]);
    for (int a = 0; a < 3; ++a)
      for (int b = a + 1; b < 3; ++b) cf[b][a] = cf[a][b];
    same_bits(cf);
    if (kind == 0) {  // plain random entries, symmetrised
      for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) cf[a][b] = cf[b][a] = (float)gauss();
      same_bits(cf);
    }
  }
}

}  // namespace

int main() {
  check_planes();
  check_degenerate();
  check_core();
  check_refit();
  check_sym3_unchanged();
  if (violations) {
    printf("%d VIOLATIONS\n", violations);
    return 1;
  }
  printf("plane_hypothesis: %ld valid planes (%ld thrown out; |n|^2 - 1 up to %.2fu, points off by up to %.2f of the "
         "bound), 1.2M degenerate triples, 0.6M fp64 eigenproblems (V^T V - I up to %.2e, reconstruction up to %.2e), "
         "0.2M refits, sym3_eigen bit-equal on %ld matrices: no violation\n",
         n_valid, n_thrown, worst_unit, worst_on, worst_orth, worst_rec, n_same);
  return 0;
}

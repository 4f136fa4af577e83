// ransac_hypothesis_main.cpp -- host check of csrc/ransac_hypothesis.h: the hash, the draw, the edge test and the
// three-pair solve of ransac_hypotheses_kernel.  The functions are __host__ __device__: this program runs the host side
// of exactly the code the kernel runs.  Launches no kernel; needs no GPU.  Prints the first violation and exits non-zero.
//
// Hash: literal values of rh_hash32 (the same literals as tests/test_ransac_cpu.py holds the numpy checker to).
// Draws: for M in {3, 4, 5, 6, 7, 1000, 65536, 2^31 - 1} and a few hundred thousand (seed, cloud, hypothesis) each, the
//   three positions are distinct and below M; for M = 3 every one of the 6 orders appears.
// Solve (u = 2^-24), on the fp32 outputs, both settings of estimate_scale:
//   R^T R = I to 4u and det R = 1 to 8u (R is orthogonal to 6e-14 in fp64 -- small_solvers_main.cpp -- and rounding entry
//   r by at most u |r| moves an entry of R^T R by at most 2u (Cauchy-Schwarz on two unit columns) and the determinant,
//   a sum of six products of three entries, by at most 3u each in total 3u sum |products| <= 3 sqrt(3) u < 8u);
//   exact-rigid triples y_k = fl(x_k R0 + T0): the fit is the least-squares optimum over the rigid (or similarity)
//   transforms and (R0, T0) is one of them, which leaves sum_k |x_k R0 + T0 - y_k|^2 <= 3 * 3 (u max|y|)^2 (three
//   coordinates of three points, each rounded by at most u |y|), so every residual of the fp64 fit is <= 3u max|y|;
//   rounding R, T, s to fp32 moves s x R + T by at most u s |x| (sqrt(3) + 1) + sqrt(3) u max|T|.  Bound:
//   |s x_k R + T - y_k| <= u (3 max|y| + 2 sqrt(3) (s max|x|_2 + max|T|)) + 1e-12, whatever the triangle's shape.
//   Collinear, coincident and duplicated triples, and triples at 1e-20 and 1e+15: every output finite, R orthogonal.
// Edge test: a congruent triangle passes at ratio 0.9; one with a side stretched by 1.2 fails; ratio * ratio is fp32.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../pytorch3d_pointops_amd/csrc/ransac_hypothesis.h"

namespace {

constexpr double kU32 = 5.9604644775390625e-08;  // 2^-24

uint64_t rng_state = 0x13198A2E03707344ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uni() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }
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
  if (violations++ < 10) printf("VIOLATION %s: %.6g (bound %.6g)\n", what, got, bound);
}

bool finite_all(const float (&R)[3][3], const float (&T)[3], float s) {
  bool ok = std::isfinite(s);
  for (int a = 0; a < 3; ++a) {
    ok = ok && std::isfinite(T[a]);
    for (int b = 0; b < 3; ++b) ok = ok && std::isfinite(R[a][b]);
  }
  return ok;
}

// max |R^T R - I| and |det R - 1| of the fp32 matrix, in fp64
void orthogonality(const float (&R)[3][3], double& ortho, double& det) {
  ortho = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double v = 0.0;
      for (int k = 0; k < 3; ++k) v += (double)R[k][a] * (double)R[k][b];
      ortho = fmax(ortho, fabs(v - (a == b ? 1.0 : 0.0)));
    }
  const double m[3][3] = {{R[0][0], R[0][1], R[0][2]}, {R[1][0], R[1][1], R[1][2]}, {R[2][0], R[2][1], R[2][2]}};
  det = fabs(pointops::pa_det<3>(m) - 1.0);
}

void check_rotation(const char* what, const float (&R)[3][3], const float (&T)[3], float s) {
  if (!finite_all(R, T, s)) {
    fail(what, NAN, 0.0);
    return;
  }
  double ortho, det;
  orthogonality(R, ortho, det);
  if (ortho > 4.0 * kU32) fail(what, ortho, 4.0 * kU32);
  if (det > 8.0 * kU32) fail(what, det, 8.0 * kU32);
}

void check_hash() {
  struct { int64_t seed, n, h; int j; uint32_t want; } const known[] = {
      {0, 0, 0, 0, 246052113u},           {0, 0, 0, 1, 1618519239u},
      {1, 2, 3, 2, 2304317301u},          {12345, 70000, 4095, 0, 3934780713u},
      {(1ll << 32) + 5, 1, 1, 1, 609416146u}, {(1ll << 62) + 7, 65536, 17, 2, 3197956988u}};
  for (const auto& k : known) {
    const uint32_t got = pointops::rh_hash32(k.seed, k.n, k.h, k.j);
    if (got != k.want) fail("hash32 known answer", (double)got, (double)k.want);
  }
}

void check_draws() {
  const uint32_t Ms[] = {3u, 4u, 5u, 6u, 7u, 1000u, 65536u, 2147483647u};
  for (uint32_t M : Ms) {
    int orders[27] = {0};
    for (int it = 0; it < 400000; ++it) {
      const int64_t seed = (int64_t)(next_u64() >> 1), n = (int64_t)(next_u64() % 70000), h = (int64_t)(next_u64() % 16777216);
      uint32_t i[3];
      pointops::rh_draw(seed, n, h, M, i);
      if (i[0] >= M || i[1] >= M || i[2] >= M) fail("draw out of range", (double)M, (double)M);
      if (i[0] == i[1] || i[0] == i[2] || i[1] == i[2]) fail("draw repeats a position", (double)i[0], (double)M);
      if (M == 3) orders[i[0] * 9 + i[1] * 3 + i[2]]++;
    }
    if (M == 3) {
      int seen = 0;
      for (int o : orders) seen += o > 0;
      if (seen != 6) fail("orders of three", (double)seen, 6.0);
    }
  }
}

void solve_and_check(const char* what, const float (&x)[3][3], const float (&y)[3][3], bool rigid, double s0) {
  for (int es = 0; es < 2; ++es) {
    float R[3][3], T[3], s;
    pointops::rh_solve(x, y, es != 0, R, T, s);
    check_rotation(what, R, T, s);
    if (!rigid || !finite_all(R, T, s)) continue;
    if (!es && s0 != 1.0) continue;  // a scaled triple is reproduced by the similarity fit only
    double mx = 0.0, my = 0.0, mt = 0.0;
    for (int k = 0; k < 3; ++k) {
      mx = fmax(mx, sqrt((double)x[k][0] * x[k][0] + (double)x[k][1] * x[k][1] + (double)x[k][2] * x[k][2]));
      for (int d = 0; d < 3; ++d) my = fmax(my, fabs((double)y[k][d])), mt = fmax(mt, fabs((double)T[d]));
    }
    const double bound = kU32 * (3.0 * my + 2.0 * sqrt(3.0) * ((double)s * mx + mt)) + 1e-12;
    for (int k = 0; k < 3; ++k) {
      double e2 = 0.0;
      for (int b = 0; b < 3; ++b) {
        double r = (double)T[b] - (double)y[k][b];
        for (int a = 0; a < 3; ++a) r += (double)s * (double)x[k][a] * (double)R[a][b];
        e2 += r * r;
      }
      if (sqrt(e2) > bound) fail(what, sqrt(e2), bound);
    }
  }
}

void check_solves() {
  for (int it = 0; it < 1500000; ++it) {
    double R0[3][3], T0[3] = {2.0 * uni() - 1.0, 2.0 * uni() - 1.0, 2.0 * uni() - 1.0};
    rotation3(R0);
    const int kind = it % 8;
    const double scale = kind == 5 ? 100.0 : (kind == 6 ? 1e-3 : 1.0);  // of the coordinates
    const double s0 = kind == 7 ? 0.5 + uni() : 1.0;                  // of the similarity
    float x[3][3], y[3][3];
    for (int k = 0; k < 3; ++k)
      for (int d = 0; d < 3; ++d) x[k][d] = (float)(scale * uni());
    if (kind == 4)  // a thin triangle: point 2 next to the line 0-1
      for (int d = 0; d < 3; ++d) x[2][d] = (float)(0.5 * ((double)x[0][d] + x[1][d]) + 1e-4 * gauss());
    for (int k = 0; k < 3; ++k)
      for (int b = 0; b < 3; ++b) {
        double v = T0[b] * scale;
        for (int a = 0; a < 3; ++a) v += s0 * (double)x[k][a] * R0[a][b];
        y[k][b] = (float)v;
      }
    solve_and_check("exact-rigid triple", x, y, true, s0);
  }
  // degenerate triples: finite, orthogonal
  for (int it = 0; it < 300000; ++it) {
    float x[3][3], y[3][3];
    const int kind = it % 6;
    const double scale = kind == 4 ? 1e-20 : (kind == 5 ? 1e15 : 1.0);
    for (int k = 0; k < 3; ++k)
      for (int d = 0; d < 3; ++d) {
        x[k][d] = (float)(scale * gauss());
        y[k][d] = (float)(scale * gauss());
      }
    if (kind == 0)  // collinear in X
      for (int d = 0; d < 3; ++d) x[2][d] = 2.0f * x[1][d] - x[0][d];
    if (kind == 1)  // coincident in X
      for (int k = 1; k < 3; ++k)
        for (int d = 0; d < 3; ++d) x[k][d] = x[0][d];
    if (kind == 2)  // a duplicated pair
      for (int d = 0; d < 3; ++d) x[1][d] = x[0][d], y[1][d] = y[0][d];
    if (kind == 3)  // coincident in both
      for (int k = 1; k < 3; ++k)
        for (int d = 0; d < 3; ++d) x[k][d] = x[0][d], y[k][d] = y[0][d];
    solve_and_check("degenerate triple", x, y, false, 1.0);
    (void)pointops::rh_edges_ok(x, y, 0.81f);
  }
}

void check_edges() {
  const float x[3][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}};
  const float y[3][3] = {{5, 5, 5}, {5, 6, 5}, {5, 5, 6}};       // congruent
  const float z[3][3] = {{5, 5, 5}, {5, 6.2f, 5}, {5, 5, 6}};    // one side 1.2: 1 < 0.81 * 1.44
  const float q = 0.9f * 0.9f;
  if (!pointops::rh_edges_ok(x, y, q)) fail("congruent triangle rejected", 0.0, 0.0);
  if (pointops::rh_edges_ok(x, z, q)) fail("stretched triangle accepted", 0.0, 0.0);
  if (pointops::rh_edges_ok(z, x, q)) fail("stretched triangle accepted (swapped)", 0.0, 0.0);
  if (!pointops::rh_edges_ok(x, z, 0.0f)) fail("ratio 0 rejects", 0.0, 0.0);
}

}  // namespace

int main() {
  check_hash();
  check_draws();
  check_edges();
  check_solves();
  if (violations) {
    printf("%d VIOLATIONS\n", violations);
    return 1;
  }
  printf("ransac_hypothesis: hash, 3.2M draws, 3M exact-rigid solves, 0.6M degenerate solves: no violation\n");
  return 0;
}

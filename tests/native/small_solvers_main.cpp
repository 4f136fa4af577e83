// small_solvers_main.cpp -- host check of csrc/small_solvers.h: sym3_eigen (the eigensolver of local_frames_kernel) and
// pa_svd<2|3> / pa_solve<2|3> (the solve of alignment_solve_kernel) on adversarial matrices.  The functions are
// __host__ __device__: this program runs the host side of exactly the code the kernels run.  Launches no kernel; needs
// no GPU.  Prints the first violation and exits non-zero.
//
// Matrix classes (both solvers): random entries; chosen spectra under random rotations -- generic, double and triple
// values, rank 1 and 2, relative gaps of 1e-7, values spread over 12 decades, a last value of 1e-16..1e-12 of the first
// --; nearly axis-aligned rotations (angles 1e-9..1e-3); scales 2^+-100; exact zeros off the diagonal (diagonal in any
// order, block diagonal); denormal fp32 entries; the zero matrix; for the SVD both signs of the determinant, d = 2 and 3.
//
// sym3_eigen, on its fp32 outputs (u = 2^-24):
//   lam ascending;  max|V^T V - I| <= 4u  (a unit vector rounded to fp32: 3 entries of <= u/2 each, twice, and the
//   factor 2 over the 1.66u measured);  max|V diag(lam) V^T - C| <= 8u max|C| + 2^-149  (three products of rounded
//   factors per entry; measured 2.39u.  2^-149 is the spacing of fp32 subnormals: an eigenvalue below 2^-126 is rounded
//   to that grid, not to 24 bits, and sum_j |v_aj v_bj| <= 1 carries at most that into an entry.  It is 0 next to the
//   first term unless max|C| < 2^-122);  the zero matrix gives the identity frame and zero eigenvalues, exactly.
// pa_svd, in fp64: sigma descending and >= 0;  U, V orthogonal to 1e-14;
//   max|U diag(sigma) V^T - C| <= (2 kSvdNegligible + 1e-14) sigma_1  (a column of U below kSvdNegligible sigma_1 is
//   rebuilt from orthogonality, so its term may be off by twice its size);  det U det V = +1 when sigma_d is negligible.
// pa_solve, all four (estimate_scale, allow_reflection): R^T R = I to 6e-14 (R = U E V^T: the two 1e-14 defects add, and
//   the largest entry of a 3x3 product is at most 3 times the factors' largest);  det R = +1 to 2e-13 unless reflections
//   are allowed, then |det R| = 1;  the objective sum_ab R_ab C_ab equals sigma_1 + .. + e sigma_d, e = sign(det C)
//   without reflections and +1 with them, to 1e-12 sigma_1 ((2 kSvdNegligible + 1e-14) sigma_1, the reconstruction bound,
//   where sigma_d is negligible AND reflections are allowed: the rebuilt column of U may be the mirror image, which costs
//   2 sigma_d <= 2e-12 sigma_1 -- measured 2.0e-12 at sigma_d = 1e-12 sigma_1 --; without reflections the determinant
//   rule picks the right one);  T = py - s px R for zero means.
// pa_accumulate<2|3>, pa_pivots<2|3> (the addends and pivots of the moment kernels): see run_accumulate.
// Non-finite entries: every solver returns (the sweep caps), nothing is checked about the values.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../pytorch3d_pointops_amd/csrc/small_solvers.h"

namespace {

using pointops::kSvdNegligible;
typedef long double ld;

constexpr double kU32 = 5.9604644775390625e-08;  // 2^-24

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uni() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
double sym() { return 2.0 * uni() - 1.0; }
double gauss() {
  double u = uni(), v = uni();
  if (u < 1e-300) u = 1e-300;
  return sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v);
}

// random rotation of R^3 (unit quaternion); `angle` > 0 limits the rotation angle
void rotation3(double (&q)[3][3], double angle = -1.0) {
  double w, x, y, z;
  if (angle > 0.0) {
    double ax[3] = {gauss(), gauss(), gauss()};
    const double n = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-300;
    const double h = 0.5 * angle;
    w = cos(h), x = sin(h) * ax[0] / n, y = sin(h) * ax[1] / n, z = sin(h) * ax[2] / n;
  } else {
    w = gauss(), x = gauss(), y = gauss(), z = gauss();
    const double n = sqrt(w * w + x * x + y * y + z * z) + 1e-300;
    w /= n, x /= n, y /= n, z /= n;
  }
  q[0][0] = 1 - 2 * (y * y + z * z), q[0][1] = 2 * (x * y - w * z), q[0][2] = 2 * (x * z + w * y);
  q[1][0] = 2 * (x * y + w * z), q[1][1] = 1 - 2 * (x * x + z * z), q[1][2] = 2 * (y * z - w * x);
  q[2][0] = 2 * (x * z - w * y), q[2][1] = 2 * (y * z + w * x), q[2][2] = 1 - 2 * (x * x + y * y);
}

template <int D>
void rotation(double (&q)[D][D], double angle = -1.0) {
  if constexpr (D == 3) {
    rotation3(q, angle);
  } else {
    const double a = angle > 0.0 ? angle * sym() : 6.283185307179586 * uni();
    q[0][0] = cos(a), q[0][1] = -sin(a), q[1][0] = sin(a), q[1][1] = cos(a);
  }
}

enum Spectrum { kGeneric, kDouble, kTriple, kRank1, kRank2, kGap1em7, kDecades12, kTinyLast, kSpectra };
const char* const kSpectrumNames[] = {"generic", "double", "triple", "rank1", "rank2", "gap1e-7", "12decades", "tinylast"};

// D non-negative values, unordered
template <int D>
void spectrum(int kind, double (&s)[D]) {
  for (int d = 0; d < D; ++d) s[d] = 0.05 + uni();
  switch (kind) {
    case kDouble: s[1] = s[0]; break;
    case kTriple: for (int d = 1; d < D; ++d) s[d] = s[0]; break;
    case kRank1: for (int d = 1; d < D; ++d) s[d] = 0.0; break;
    case kRank2: s[D - 1] = 0.0; break;
    case kGap1em7: for (int d = 1; d < D; ++d) s[d] = s[0] * (1.0 + 1e-7 * d * (0.5 + uni())); break;
    case kDecades12: for (int d = 1; d < D; ++d) s[d] = s[0] * pow(10.0, -12.0 * (D == 2 ? 1.0 : d == 2 ? 1.0 : uni())); break;
    case kTinyLast: s[D - 1] = s[0] * pow(10.0, -12.0 - 4.0 * uni()); break;
    default: break;
  }
  const int a = (int)(next_u64() % D), b = (int)(next_u64() % D);  // any order
  const double t = s[a];
  s[a] = s[b];
  s[b] = t;
}

long n_sym = 0, n_svd = 0, n_solve = 0;
double worst_orth32 = 0, worst_rec32 = 0, worst_orth64 = 0, worst_rec64 = 0, worst_obj = 0, worst_obj_refl = 0;

void print3(const char* name, const float (&m)[3][3]) {
  printf("  %s = [[%.9g %.9g %.9g] [%.9g %.9g %.9g] [%.9g %.9g %.9g]]\n", name, m[0][0], m[0][1], m[0][2], m[1][0],
         m[1][1], m[1][2], m[2][0], m[2][1], m[2][2]);
}

bool check_sym3(const float (&c)[3][3], const char* what) {
  ++n_sym;
  float lam[3], v[3][3];
  pointops::sym3_eigen(c, lam, v);
  double cmax = 0.0;
  bool zero = true;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      cmax = fmax(cmax, fabs((double)c[a][b]));
      zero = zero && c[a][b] == 0.0f;
    }
  bool ok = lam[0] <= lam[1] && lam[1] <= lam[2];
  const char* why = "eigenvalues not ascending";
  if (ok && zero) {
    for (int a = 0; a < 3; ++a) {
      ok = ok && lam[a] == 0.0f;
      for (int b = 0; b < 3; ++b) ok = ok && v[a][b] == (a == b ? 1.0f : 0.0f);
    }
    why = "zero matrix: not the identity frame with zero eigenvalues";
  }
  double orth = 0.0, rec = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double g = 0.0, r = 0.0;
      for (int k = 0; k < 3; ++k) {
        g += (double)v[k][a] * (double)v[k][b];
        r += (double)v[a][k] * (double)lam[k] * (double)v[b][k];
      }
      orth = fmax(orth, fabs(g - (a == b ? 1.0 : 0.0)));
      rec = fmax(rec, fabs(r - (double)c[a][b]));
    }
  if (ok && !(orth <= 4.0 * kU32)) ok = false, why = "max|V^T V - I| > 4 * 2^-24";
  const double rec_bound = 8.0 * kU32 * cmax + ldexp(1.0, -149);
  if (ok && !(rec <= rec_bound)) ok = false, why = "max|V diag(lam) V^T - C| > 8 * 2^-24 max|C|";
  if (!ok) {
    printf("VIOLATION sym3_eigen [%s]: %s\n  orth = %.3e (%.3f u)  rec = %.3e (%.3f u max|C|)\n", what, why, orth,
           orth / kU32, rec, cmax > 0 ? rec / (kU32 * cmax) : 0.0);
    print3("C", c);
    print3("V", v);
    printf("  lam = [%.9g %.9g %.9g]\n", lam[0], lam[1], lam[2]);
    return false;
  }
  worst_orth32 = fmax(worst_orth32, orth / kU32);
  if (cmax >= ldexp(1.0, -110)) worst_rec32 = fmax(worst_rec32, rec / (kU32 * cmax));
  return true;
}

// C = Q diag(l) Q^T rounded to fp32, symmetric by construction
void compose_sym(const double (&q)[3][3], const double (&l)[3], double scale, float (&c)[3][3]) {
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) {
      double r = 0.0;
      for (int k = 0; k < 3; ++k) r += q[a][k] * l[k] * q[b][k];
      c[a][b] = c[b][a] = (float)(r * scale);
    }
}

bool run_sym3(int per_class) {
  float c[3][3];
  double q[3][3], l[3];
  char what[96];
  for (int it = 0; it < per_class; ++it) {
    // random entries, any sign
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) c[a][b] = c[b][a] = (float)sym();
    if (!check_sym3(c, "random entries")) return false;
    for (int kind = 0; kind < kSpectra; ++kind) {
      spectrum<3>(kind, l);
      rotation<3>(q);
      compose_sym(q, l, 1.0, c);
      if (!check_sym3(c, kSpectrumNames[kind])) return false;
      rotation<3>(q, pow(10.0, -9.0 + 6.0 * uni()));
      compose_sym(q, l, 1.0, c);
      snprintf(what, sizeof what, "%s, nearly axis-aligned", kSpectrumNames[kind]);
      if (!check_sym3(c, what)) return false;
      rotation<3>(q);
      compose_sym(q, l, (it & 1) ? ldexp(1.0, 100) : ldexp(1.0, -100), c);
      snprintf(what, sizeof what, "%s, scale 2^%d", kSpectrumNames[kind], (it & 1) ? 100 : -100);
      if (!check_sym3(c, what)) return false;
    }
    // exact zeros off the diagonal: a diagonal in any order (signs too), and one 2x2 block
    memset(c, 0, sizeof c);
    for (int a = 0; a < 3; ++a) c[a][a] = (float)((it % 3 == 0) ? sym() : uni());
    if (it % 5 == 0) c[1][1] = c[0][0];
    if (it % 7 == 0) c[2][2] = c[0][0];
    if (!check_sym3(c, "diagonal")) return false;
    const int p = it % 3, r = (p + 1) % 3;
    c[p][r] = c[r][p] = (float)(0.5 * sym());
    if (!check_sym3(c, "block diagonal")) return false;
    // denormal fp32 entries: off the diagonal of an ordinary matrix, on it, and everywhere
    const float den[3] = {(float)ldexp(sym(), -130), (float)ldexp(sym(), -140), (float)ldexp(sym(), -149)};
    memset(c, 0, sizeof c);
    for (int a = 0; a < 3; ++a) c[a][a] = (float)uni();
    c[0][1] = c[1][0] = den[0], c[0][2] = c[2][0] = den[1], c[1][2] = c[2][1] = den[2];
    if (!check_sym3(c, "denormal off-diagonals")) return false;
    c[it % 3][it % 3] = den[it % 3];
    if (!check_sym3(c, "denormal diagonal entry")) return false;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) c[a][b] = c[b][a] = (float)ldexp(sym(), -127 - (int)(next_u64() % 22));
    if (!check_sym3(c, "all entries denormal")) return false;
  }
  memset(c, 0, sizeof c);
  if (!check_sym3(c, "zero matrix")) return false;
  c[0][0] = -0.0f, c[1][2] = c[2][1] = -0.0f;
  return check_sym3(c, "zero matrix with negative zeros");
}

template <int D>
ld det_ld(const double (&m)[D][D]) {
  if constexpr (D == 2) {
    return (ld)m[0][0] * m[1][1] - (ld)m[0][1] * m[1][0];
  } else {
    return (ld)m[0][0] * ((ld)m[1][1] * m[2][2] - (ld)m[1][2] * m[2][1]) -
           (ld)m[0][1] * ((ld)m[1][0] * m[2][2] - (ld)m[1][2] * m[2][0]) +
           (ld)m[0][2] * ((ld)m[1][0] * m[2][1] - (ld)m[1][1] * m[2][0]);
  }
}

template <int D>
double orth_defect(const double (&m)[D][D]) {
  ld worst = 0;
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < D; ++b) {
      ld g = 0;
      for (int k = 0; k < D; ++k) g += (ld)m[k][a] * m[k][b];
      worst = fmaxl(worst, fabsl(g - (a == b ? 1 : 0)));
    }
  return (double)worst;
}

template <int D>
void print_mat(const char* name, const double (&m)[D][D]) {
  printf("  %s = [", name);
  for (int a = 0; a < D; ++a) {
    printf("[");
    for (int b = 0; b < D; ++b) printf("%.17g%s", m[a][b], b + 1 < D ? " " : "");
    printf("]%s", a + 1 < D ? " " : "");
  }
  printf("]\n");
}

template <int D>
bool fail_svd(const char* what, const char* why, const double (&C)[D][D], const double (&U)[D][D],
              const double (&sg)[D], const double (&V)[D][D]) {
  printf("VIOLATION pa_svd<%d> / pa_solve<%d> [%s]: %s\n", D, D, what, why);
  print_mat<D>("C", C);
  print_mat<D>("U", U);
  print_mat<D>("V", V);
  printf("  sigma = [");
  for (int d = 0; d < D; ++d) printf("%.17g ", sg[d]);
  printf("]\n");
  return false;
}

template <int D>
bool check_svd(const double (&C)[D][D], const char* what, int det_sign = 0) {
  ++n_svd;
  double U[D][D], V[D][D], sg[D];
  pointops::pa_svd<D>(C, U, sg, V);
  for (int d = 0; d < D; ++d)
    if (!(sg[d] >= 0.0) || (d > 0 && !(sg[d - 1] >= sg[d])))
      return fail_svd<D>(what, "sigma not descending and >= 0", C, U, sg, V);
  const double ou = orth_defect<D>(U), ov = orth_defect<D>(V);
  if (!(ou <= 1e-14) || !(ov <= 1e-14)) {
    printf("  defects: U %.3e, V %.3e\n", ou, ov);
    return fail_svd<D>(what, "U or V not orthogonal to 1e-14", C, U, sg, V);
  }
  ld rec = 0;
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < D; ++b) {
      ld r = 0;
      for (int k = 0; k < D; ++k) r += (ld)U[a][k] * sg[k] * V[b][k];
      rec = fmaxl(rec, fabsl(r - C[a][b]));
    }
  if (!((double)rec <= (2.0 * kSvdNegligible + 1e-14) * sg[0])) {
    printf("  defect %.3Le, sigma_1 %.3e\n", rec, sg[0]);
    return fail_svd<D>(what, "max|U diag(sigma) V^T - C| > (2 kSvdNegligible + 1e-14) sigma_1", C, U, sg, V);
  }
  const bool negligible = !(sg[D - 1] > kSvdNegligible * sg[0]);
  if (negligible) {
    const ld dd = det_ld<D>(U) * det_ld<D>(V);
    if (!(fabsl(dd - 1) <= 1e-13L))
      return fail_svd<D>(what, "det U det V != +1 with a negligible sigma_d", C, U, sg, V);
  }
  worst_orth64 = fmax(worst_orth64, fmax(ou, ov));
  if (sg[0] > 0) worst_rec64 = fmax(worst_rec64, (double)rec / sg[0]);

  // pa_solve on moments whose centred cross-covariance is C itself: W = Sw2 = 1, zero means, pivots px, py
  using S = pointops::PaSlot<D>;
  double mom[S::kCount];
  for (int m = 0; m < S::kCount; ++m) mom[m] = 0.0;
  mom[S::kSw] = mom[S::kSw2] = 1.0;
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < D; ++b) mom[S::kSxy + a * D + b] = C[a][b];
  mom[S::kSxx] = 0.25 + uni();
  double px[D], py[D];
  for (int d = 0; d < D; ++d) px[d] = sym(), py[d] = sym();
  // sign(det C): known from the construction where C was composed (cofactors of a matrix with sigma_d ~ 1e-12 sigma_1
  // cancel to noise even in long double), computed otherwise
  const ld detC = det_sign != 0 ? (ld)det_sign : det_ld<D>(C);
  for (int flags = 0; flags < 4; ++flags) {
    ++n_solve;
    const bool scale = flags & 1, refl = flags & 2;
    double R[D][D], T[D], s, sg2[D];
    pointops::pa_solve<D>(mom, px, py, scale, refl, 1e-9, R, T, s, sg2);
    for (int d = 0; d < D; ++d)
      if (sg2[d] != sg[d]) return fail_svd<D>(what, "pa_solve: singular values differ from pa_svd's", C, U, sg, V);
    const double orr = orth_defect<D>(R);
    const ld dr = det_ld<D>(R);
    if (!(orr <= 6e-14)) return fail_svd<D>(what, "pa_solve: R not orthogonal to 6e-14", C, R, sg, V);
    if (!(fabsl((refl ? fabsl(dr) : dr) - 1) <= 2e-13L))
      return fail_svd<D>(what, refl ? "pa_solve: |det R| != 1" : "pa_solve: det R != +1", C, R, sg, V);
    ld obj = 0, want = 0;
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) obj += (ld)R[a][b] * C[a][b];
    for (int d = 0; d < D; ++d) want += (d == D - 1 && !refl && detC < 0) ? -(ld)sg[d] : (ld)sg[d];
    const double miss = (double)fabsl(obj - want);
    const double bar = (refl && negligible ? 2.0 * kSvdNegligible + 1e-14 : 1e-12) * sg[0];
    if (!(miss <= bar)) {
      printf("  scale=%d refl=%d objective %.17Lg, sum of sigma with the sign rule %.17Lg, bar %.3e\n", (int)scale,
             (int)refl, obj, want, bar);
      return fail_svd<D>(what, "pa_solve: objective differs from the optimum", C, R, sg, V);
    }
    if (sg[0] > 0) {
      if (refl && negligible) worst_obj_refl = fmax(worst_obj_refl, miss / sg[0]);
      else worst_obj = fmax(worst_obj, miss / sg[0]);
    }
    if (!std::isfinite(s) || (!scale && s != 1.0)) return fail_svd<D>(what, "pa_solve: scale", C, R, sg, V);
    for (int b = 0; b < D; ++b) {
      ld xr = 0;
      for (int a = 0; a < D; ++a) xr += (ld)px[a] * R[a][b];
      const ld t = (ld)py[b] - (ld)s * xr;
      if (!(fabsl(t - T[b]) <= 1e-14L * (1 + fabsl((ld)s) * D)))
        return fail_svd<D>(what, "pa_solve: T != py - s px R", C, R, sg, V);
    }
  }
  return true;
}

// C = U diag(s) V^T for rotations U, V (one of them mirrored when `mirror`)
template <int D>
void compose_svd(const double (&u)[D][D], const double (&s)[D], const double (&v)[D][D], bool mirror, double scale,
                 double (&C)[D][D]) {
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < D; ++b) {
      double r = 0.0;
      for (int k = 0; k < D; ++k) r += u[a][k] * s[k] * v[b][k] * (mirror && k == 0 ? -1.0 : 1.0);
      C[a][b] = r * scale;
    }
}

template <int D>
bool run_svd(int per_class) {
  double C[D][D], u[D][D], v[D][D], s[D];
  char what[96];
  for (int it = 0; it < per_class; ++it) {
    const bool mirror = it & 1;
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) C[a][b] = sym();
    if (!check_svd<D>(C, "random entries")) return false;
    for (int kind = 0; kind < kSpectra; ++kind) {
      spectrum<D>(kind, s);
      rotation<D>(u), rotation<D>(v);
      compose_svd<D>(u, s, v, mirror, 1.0, C);
      snprintf(what, sizeof what, "%s, det %c", kSpectrumNames[kind], mirror ? '-' : '+');
      const int sign = (kind == kRank1 || kind == kRank2) ? 0 : (mirror ? -1 : 1);  // rank-deficient: det C is rounding
      if (!check_svd<D>(C, what, sign)) return false;
      rotation<D>(u, pow(10.0, -9.0 + 6.0 * uni())), rotation<D>(v, pow(10.0, -9.0 + 6.0 * uni()));
      compose_svd<D>(u, s, v, mirror, 1.0, C);
      snprintf(what, sizeof what, "%s, nearly axis-aligned, det %c", kSpectrumNames[kind], mirror ? '-' : '+');
      if (!check_svd<D>(C, what, sign)) return false;
      rotation<D>(u), rotation<D>(v);
      compose_svd<D>(u, s, v, mirror, (it & 2) ? ldexp(1.0, 100) : ldexp(1.0, -100), C);
      snprintf(what, sizeof what, "%s, scale 2^%d, det %c", kSpectrumNames[kind], (it & 2) ? 100 : -100,
               mirror ? '-' : '+');
      if (!check_svd<D>(C, what, sign)) return false;
    }
    // exact zeros: a signed diagonal in any order, a signed permutation pattern, one off-diagonal entry added
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) C[a][b] = 0.0;
    for (int a = 0; a < D; ++a) C[a][a] = (it % 4 == 0 && a == 1) ? 0.0 : sym();
    if (!check_svd<D>(C, "diagonal")) return false;
    C[0][D - 1] = sym();
    if (!check_svd<D>(C, "diagonal plus one entry")) return false;
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) C[a][b] = 0.0;
    for (int a = 0; a < D; ++a) C[a][(a + 1 + it % (D - 1)) % D] = sym();
    if (!check_svd<D>(C, "scaled permutation")) return false;
    // denormal fp32 entries next to ordinary ones, and alone
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b)
        C[a][b] = (next_u64() & 1) ? (double)(float)ldexp(sym(), -127 - (int)(next_u64() % 22)) : sym();
    if (!check_svd<D>(C, "some entries denormal fp32")) return false;
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) C[a][b] = (double)(float)ldexp(sym(), -127 - (int)(next_u64() % 22));
    if (!check_svd<D>(C, "all entries denormal fp32")) return false;
  }
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < D; ++b) C[a][b] = 0.0;
  return check_svd<D>(C, "zero matrix");
}

// NaN / Inf entries: the calls must come back (sweep caps); values are not checked
template <int D>
void run_nonfinite_svd() {
  const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                         -std::numeric_limits<double>::infinity()};
  using S = pointops::PaSlot<D>;
  for (int it = 0; it < 2000; ++it) {
    double C[D][D], U[D][D], V[D][D], sg[D], R[D][D], T[D], s, px[D], py[D], mom[S::kCount];
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) C[a][b] = (next_u64() % 3 == 0) ? bad[next_u64() % 3] : sym();
    C[it % D][(it / D) % D] = bad[it % 3];
    pointops::pa_svd<D>(C, U, sg, V);
    for (int m = 0; m < S::kCount; ++m) mom[m] = (next_u64() % 4 == 0) ? bad[next_u64() % 3] : sym();
    mom[it % S::kCount] = bad[it % 3];
    for (int d = 0; d < D; ++d) px[d] = sym(), py[d] = (it % 11 == 0) ? bad[d % 3] : sym();
    for (int flags = 0; flags < 4; ++flags) pointops::pa_solve<D>(mom, px, py, flags & 1, flags & 2, 1e-9, R, T, s, sg);
  }
}

// pa_accumulate over n weighted pairs against the long double sums of the definition, slot by slot, to the bound of
// the moment tests: n 2^-52 times the sum of the addends' magnitudes (n - 1 additions and at most three roundings per
// addend, each 2^-53 relative).  pa_pivots: row 0 of each cloud as doubles, zeros for an empty cloud.
template <int D>
bool run_accumulate(int n) {
  using S = pointops::PaSlot<D>;
  double acc[S::kCount + 2];  // (registration's array is longer than the moments)
  ld want[S::kCount], mag[S::kCount];
  for (int m = 0; m < S::kCount + 2; ++m) acc[m] = 0.0;
  for (int m = 0; m < S::kCount; ++m) want[m] = mag[m] = 0.0L;
  for (int i = 0; i < n; ++i) {
    const double w = i % 7 == 0 ? 1.0 : uni();
    double x[D], y[D];
    for (int d = 0; d < D; ++d) x[d] = 100.0 * sym(), y[d] = 100.0 * sym();
    pointops::pa_accumulate<D>(acc, w, x, y);
    ld t[S::kCount];
    const ld w2 = (ld)w * w;
    t[S::kSw] = w;
    t[S::kSw2] = w2;
    t[S::kSxx] = 0.0L;
    for (int a = 0; a < D; ++a) {
      t[S::kSwx + a] = (ld)w * x[a];
      t[S::kSwy + a] = (ld)w * y[a];
      t[S::kSw2x + a] = w2 * x[a];
      t[S::kSw2y + a] = w2 * y[a];
      for (int b = 0; b < D; ++b) t[S::kSxy + a * D + b] = w2 * x[a] * y[b];
      t[S::kSxx] += w2 * x[a] * x[a];
    }
    for (int m = 0; m < S::kCount; ++m) want[m] += t[m], mag[m] += fabsl(t[m]);
  }
  for (int m = 0; m < S::kCount; ++m) {
    const ld bound = (ld)n * 2.220446049250313e-16L * mag[m];
    if (!(fabsl((ld)acc[m] - want[m]) <= bound)) {
      printf("pa_accumulate<%d>: slot %d is %.17g, the definition gives %.17Lg (bound %.3Le)\n", D, m, acc[m], want[m],
             bound);
      return false;
    }
  }
  if (acc[S::kCount] != 0.0 || acc[S::kCount + 1] != 0.0) {
    printf("pa_accumulate<%d>: wrote past the moments\n", D);
    return false;
  }
  float X[2 * 3 * D], Y[2 * 2 * D];  // two clouds of P = 3 and P2 = 2 rows
  for (int i = 0; i < 2 * 3 * D; ++i) X[i] = (float)sym();
  for (int i = 0; i < 2 * 2 * D; ++i) Y[i] = (float)sym();
  double px[D], py[D];
  pointops::pa_pivots<D>(X, Y, 1, 3, 2, 3, px, py);
  for (int d = 0; d < D; ++d)
    if (px[d] != (double)X[3 * D + d] || py[d] != (double)Y[2 * D + d]) {
      printf("pa_pivots<%d>: not row 0 of cloud 1\n", D);
      return false;
    }
  pointops::pa_pivots<D>(X, Y, 1, 3, 2, 0, px, py);
  for (int d = 0; d < D; ++d)
    if (px[d] != 0.0 || py[d] != 0.0) {
      printf("pa_pivots<%d>: an empty cloud has pivots\n", D);
      return false;
    }
  return true;
}

void run_nonfinite_sym3() {
  const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                        -std::numeric_limits<float>::infinity()};
  for (int it = 0; it < 2000; ++it) {
    float c[3][3], lam[3], v[3][3];
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) c[a][b] = c[b][a] = (next_u64() % 3 == 0) ? bad[next_u64() % 3] : (float)sym();
    const int a = it % 3, b = (it / 3) % 3;
    c[a][b] = c[b][a] = bad[it % 3];
    pointops::sym3_eigen(c, lam, v);
  }
  // the largest finite fp32 everywhere: eigenvalues overflow fp32 on the way out
  float c[3][3], lam[3], v[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) c[a][b] = std::numeric_limits<float>::max();
  pointops::sym3_eigen(c, lam, v);
}

}  // namespace

int main(int argc, char** argv) {
  const int per_class = argc > 1 ? atoi(argv[1]) : 4000;
  if (!run_sym3(per_class)) return 1;
  if (!run_svd<3>(per_class)) return 1;
  if (!run_svd<2>(per_class)) return 1;
  if (!run_accumulate<3>(per_class) || !run_accumulate<2>(per_class)) return 1;
  run_nonfinite_sym3();
  run_nonfinite_svd<3>();
  run_nonfinite_svd<2>();
  printf("sym3_eigen: %ld matrices, worst |V^T V - I| = %.3f * 2^-24, worst |V diag V^T - C| = %.3f * 2^-24 max|C|\n",
         n_sym, worst_orth32, worst_rec32);
  printf("pa_svd: %ld matrices, worst orthogonality defect %.3e, worst reconstruction defect %.3e sigma_1\n", n_svd,
         worst_orth64, worst_rec64);
  printf("pa_solve: %ld solves, worst objective miss %.3e sigma_1 (%.3e sigma_1 with reflections and a negligible "
         "sigma_d)\n", n_solve, worst_obj, worst_obj_refl);
  printf("small_solvers: no violation\n");
  return 0;
}

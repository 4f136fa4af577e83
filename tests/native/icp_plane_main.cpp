// icp_plane_main.cpp -- csrc/icp_plane.h on the host, and nothing else of the library: the 6x6 Cholesky with the
// degeneracy rule, the rotation of three angles and the fp64 compose of registration_icp's point-to-plane update.
// tests/test_registration_cpu.py compiles this with the flags of the build (once plain, once with the host sanitizers)
// and runs it; it prints one line per check and "no violation" at the end, or "VIOLATION ..." lines and exits 1.
//
//   1. Cholesky against Gaussian elimination with partial pivoting in long double, on A = Q diag(lambda) Q^T with Q
//      from a long-double Gram-Schmidt of a random matrix and lambda spread geometrically over a condition number of
//      1 .. 1e7 (every one below 1 / kIcpDegeneratePivot, so none may be called degenerate).  Bound: Cholesky solves
//      (A + dA) x = b with |dA|_2 <= n gamma_{3n+1} |A|_2 (Higham, Accuracy and Stability, Thm 10.4 with
//      | |R^T| |R| |_2 <= n |A|_2), n = 6: 114 u < 64 * 2^-52, so |x - x_ref| <= 64 cond(A) 2^-52 |x_ref| to first order.
//   2. The degeneracy rule: A = sum_{k < r} v_k v_k^T for r = 3, 4, 5 (rounded to fp64: the deficient pivots come out
//      around 1e-16 of the diagonal times the growth of the elimination before them, positive or negative) must be
//      refused WHERE the leading r x r block is sound (every pivot at least 1e-3 of its diagonal: leading_block_is_sound);
//      the rest, about 4 % of the samples, are run and counted but not judged -- the rule is relative to the diagonal and
//      does miss some of them (2 of 6000 here), which the program prints.  Matrices with exactly zero rows and columns
//      (one plane z = const as the target) must be refused always; x must be untouched by a refusal.
//   3. Rd Rd^T = I to 4 * 2^-52 in every entry, det Rd > 0, and Rd against the long-double product (Rz Ry Rx)^T.
//   4. icp_compose against the direct product of the two 4x4 homogeneous matrices in long double.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../pytorch3d_pointops_amd/csrc/icp_plane.h"

using namespace pointops;
typedef long double ld;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // [0, 1): splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
static double signed_uniform() { return 2.0 * uniform() - 1.0; }

static int g_violations = 0;
static void violation(const char* what, int trial, double got, double bound) {
  if (++g_violations <= 20) printf("VIOLATION %s: trial %d, %.6e against the bound %.6e\n", what, trial, got, bound);
}

// orthonormal columns by modified Gram-Schmidt (twice) of a random matrix, long double
static void random_orthogonal(ld (&Q)[6][6]) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) Q[r][c] = (ld)signed_uniform();
  for (int pass = 0; pass < 2; ++pass)
    for (int c = 0; c < 6; ++c) {
      for (int k = 0; k < c; ++k) {
        ld d = 0;
        for (int r = 0; r < 6; ++r) d += Q[r][c] * Q[r][k];
        for (int r = 0; r < 6; ++r) Q[r][c] -= d * Q[r][k];
      }
      ld nrm = 0;
      for (int r = 0; r < 6; ++r) nrm += Q[r][c] * Q[r][c];
      nrm = sqrtl(nrm);
      for (int r = 0; r < 6; ++r) Q[r][c] /= nrm;
    }
}

static void pack_upper(const double (&A)[6][6], double (&up)[kIcpUpper]) {
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) up[icp_upper(r, c)] = A[r][c];
}

// Gaussian elimination with partial pivoting in long double; false when a pivot is zero
static bool solve_ld(const double (&A)[6][6], const double (&b)[6], ld (&x)[6]) {
  ld M[6][7];
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) M[r][c] = (ld)A[r][c];
    M[r][6] = (ld)b[r];
  }
  for (int k = 0; k < 6; ++k) {
    int p = k;
    for (int r = k + 1; r < 6; ++r)
      if (fabsl(M[r][k]) > fabsl(M[p][k])) p = r;
    if (M[p][k] == 0) return false;
    for (int c = 0; c < 7; ++c) {
      const ld t = M[k][c];
      M[k][c] = M[p][c];
      M[p][c] = t;
    }
    for (int r = k + 1; r < 6; ++r) {
      const ld f = M[r][k] / M[k][k];
      for (int c = k; c < 7; ++c) M[r][c] -= f * M[k][c];
    }
  }
  for (int r = 5; r >= 0; --r) {
    ld v = M[r][6];
    for (int c = r + 1; c < 6; ++c) v -= M[r][c] * x[c];
    x[r] = v / M[r][r];
  }
  return true;
}

static void check_cholesky() {
  const double u52 = ldexp(1.0, -52);
  double worst = 0.0;
  int trials = 0;
  for (int e = 0; e <= 7; ++e) {
    const ld cond = powl(10.0L, (ld)e);
    for (int trial = 0; trial < 2000; ++trial, ++trials) {
      ld Q[6][6];
      random_orthogonal(Q);
      const ld scale = powl(10.0L, (ld)(6.0 * signed_uniform()));  // the rule is relative: any magnitude
      double A[6][6], b[6], up[kIcpUpper], x[6];
      for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) {
          ld v = 0;
          for (int k = 0; k < 6; ++k) v += Q[r][k] * Q[c][k] * scale * powl(cond, -(ld)k / 5.0L);
          A[r][c] = (double)v;
        }
        b[r] = signed_uniform() * (double)scale;
      }
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < r; ++c) A[r][c] = A[c][r];  // (exactly symmetric after the rounding)
      pack_upper(A, up);
      ld ref[6];
      if (!solve_ld(A, b, ref)) continue;
      if (!icp_cholesky_solve6(up, b, x)) {
        violation("cholesky refused a matrix of condition number <= 1e7", trials, (double)cond, 1e10);
        continue;
      }
      ld err = 0, nrm = 0;
      for (int r = 0; r < 6; ++r) {
        err += ((ld)x[r] - ref[r]) * ((ld)x[r] - ref[r]);
        nrm += ref[r] * ref[r];
      }
      const double rel = (double)(sqrtl(err) / sqrtl(nrm)), bound = 64.0 * (double)cond * u52;
      if (rel / bound > worst) worst = rel / bound;
      if (!(rel <= bound)) violation("cholesky solution", trials, rel, bound);
    }
  }
  printf("cholesky: %d systems, worst error / bound = %.3f\n", trials, worst);
}

// The rule measures a pivot against the diagonal entry of its own row, so the rounding residue of a deficient pivot --
// about 2^-53 of the diagonal times the growth of the elimination before it -- stays far below kIcpDegeneratePivot only
// while the pivots of the leading rank x rank block are themselves sound.  This is that condition, evaluated in long
// double: every one of the first `rank` pivots is at least 1e-3 of its diagonal entry (growth <= 1e3: residues around
// 1e-13).  About 4 random samples in a hundred miss it.  They are not held to the rule, but they are still run, and the
// program reports how many of them the rule let through: that is what the rule misses.
static bool leading_block_is_sound(const double (&A)[6][6], int rank) {
  ld L[6][6];
  for (int j = 0; j < rank; ++j) {
    ld piv = (ld)A[j][j];
    for (int k = 0; k < j; ++k) piv -= L[j][k] * L[j][k];
    if (!(piv >= 1e-3L * (ld)A[j][j])) return false;
    L[j][j] = sqrtl(piv);
    for (int i = j + 1; i < 6; ++i) {
      ld v = (ld)A[j][i];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  return true;
}

static void check_degenerate() {
  int refused = 0, trials = 0, hidden = 0, hidden_solved = 0;
  for (int rank = 3; rank <= 5; ++rank)
    for (int trial = 0; trial < 2000; ++trial, ++trials) {
      double A[6][6] = {}, up[kIcpUpper], b[6], x[6];
      for (int k = 0; k < rank; ++k) {
        double v[6];
        for (int r = 0; r < 6; ++r) v[r] = signed_uniform();
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < 6; ++c) A[r][c] += v[r] * v[c];
      }
      for (int r = 0; r < 6; ++r) {
        b[r] = signed_uniform();
        x[r] = 12345.0;
        for (int c = 0; c < r; ++c) A[r][c] = A[c][r];
      }
      pack_upper(A, up);
      if (!leading_block_is_sound(A, rank)) {
        ++hidden;
        if (icp_cholesky_solve6(up, b, x)) ++hidden_solved;
        continue;
      }
      if (icp_cholesky_solve6(up, b, x)) {
        violation("a rank-deficient matrix was solved, rank", trials, rank, 6);
        continue;
      }
      ++refused;
      for (int r = 0; r < 6; ++r)
        if (x[r] != 12345.0) violation("x written by a refused solve", trials, x[r], 12345.0);
    }
  // one plane z = const as the target: n = (0, 0, 1), J = (p_y, -p_x, 0, 0, 0, 1): exact zeros in rows 2, 3, 4
  for (int trial = 0; trial < 200; ++trial, ++trials) {
    double A[6][6] = {}, up[kIcpUpper], b[6] = {1, 1, 1, 1, 1, 1}, x[6];
    for (int i = 0; i < 50; ++i) {
      const double px = signed_uniform(), py = signed_uniform();
      const double J[6] = {py, -px, 0.0, 0.0, 0.0, 1.0};
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) A[r][c] += J[r] * J[c];
    }
    pack_upper(A, up);
    if (icp_cholesky_solve6(up, b, x)) violation("the planar target was solved", trials, 3, 6);
    else ++refused;
  }
  double nanup[kIcpUpper], b[6] = {}, x[6];
  for (int k = 0; k < kIcpUpper; ++k) nanup[k] = NAN;
  if (icp_cholesky_solve6(nanup, b, x)) violation("a NaN matrix was solved", trials, 0, 0);
  if (hidden * 10 > trials) violation("too many samples without a sound leading block", trials, hidden, trials / 10);
  printf("degeneracy: %d of %d deficient systems refused; %d more without a sound leading block, of which %d were SOLVED "
         "(the relative rule's misses)\n", refused, trials - hidden, hidden, hidden_solved);
}

static void check_rotation_and_compose() {
  const double u52 = ldexp(1.0, -52);
  double worst_orth = 0.0, worst_rot = 0.0, worst_comp = 0.0;
  const int trials = 200000;
  for (int trial = 0; trial < trials; ++trial) {
    const double span = trial % 2 ? 3.141592653589793 : 0.3;  // whole turns, and the small steps ICP takes
    const double al = span * signed_uniform(), be = span * signed_uniform(), ga = span * signed_uniform();
    double Rd[3][3];
    icp_rotation(al, be, ga, Rd);
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) {
        ld d = 0;
        for (int k = 0; k < 3; ++k) d += (ld)Rd[a][k] * (ld)Rd[c][k];
        const double e = fabs((double)(d - (a == c ? 1.0L : 0.0L)));
        if (e > worst_orth) worst_orth = e;
        if (!(e <= 4.0 * u52)) violation("Rd Rd^T - I", trial, e, 4.0 * u52);
      }
    const double det = Rd[0][0] * (Rd[1][1] * Rd[2][2] - Rd[1][2] * Rd[2][1]) -
                       Rd[0][1] * (Rd[1][0] * Rd[2][2] - Rd[1][2] * Rd[2][0]) +
                       Rd[0][2] * (Rd[1][0] * Rd[2][1] - Rd[1][1] * Rd[2][0]);
    if (!(det > 0.0)) violation("det Rd", trial, det, 0.0);
    // (Rz Ry Rx)^T in long double
    const ld ca = cosl(al), sa = sinl(al), cb = cosl(be), sb = sinl(be), cg = cosl(ga), sg = sinl(ga);
    const ld Rx[3][3] = {{1, 0, 0}, {0, ca, -sa}, {0, sa, ca}}, Ry[3][3] = {{cb, 0, sb}, {0, 1, 0}, {-sb, 0, cb}},
             Rz[3][3] = {{cg, -sg, 0}, {sg, cg, 0}, {0, 0, 1}};
    ld M[3][3];
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) {
        ld v = 0;
        for (int k = 0; k < 3; ++k)
          for (int m = 0; m < 3; ++m) v += Rz[a][k] * Ry[k][m] * Rx[m][c];
        M[a][c] = v;
      }
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) {
        const double e = fabs((double)((ld)Rd[a][c] - M[c][a]));
        if (e > worst_rot) worst_rot = e;
        if (!(e <= 4.0 * u52)) violation("Rd against (Rz Ry Rx)^T", trial, e, 4.0 * u52);
      }
    // compose: x -> x R + T, then x -> (x - c0) Rd + c0 + t
    double R[3][3], T[3], c0[3], t[3];
    icp_rotation(3.0 * signed_uniform(), 3.0 * signed_uniform(), 3.0 * signed_uniform(), R);
    ld size = 1;
    for (int a = 0; a < 3; ++a) {
      T[a] = 10.0 * signed_uniform();
      c0[a] = 10.0 * signed_uniform();
      t[a] = signed_uniform();
      size += fabsl((ld)T[a]) + fabsl((ld)c0[a]) + fabsl((ld)t[a]);
    }
    ld Rw[3][3], Tw[3];
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) {
        ld v = 0;
        for (int k = 0; k < 3; ++k) v += (ld)R[a][k] * (ld)Rd[k][c];
        Rw[a][c] = v;
      }
    for (int c = 0; c < 3; ++c) {
      ld v = (ld)c0[c] + (ld)t[c];
      for (int k = 0; k < 3; ++k) v += ((ld)T[k] - (ld)c0[k]) * (ld)Rd[k][c];
      Tw[c] = v;
    }
    icp_compose(R, T, Rd, c0, t);
    // every output is a sum of at most five terms of fp64 products: 8 roundings of 2^-53 of the terms' magnitudes
    const double bound = 4.0 * u52 * (double)size;
    for (int a = 0; a < 3; ++a) {
      const double eT = fabs((double)((ld)T[a] - Tw[a]));
      if (eT > worst_comp) worst_comp = eT;
      if (!(eT <= bound)) violation("compose T", trial, eT, bound);
      for (int c = 0; c < 3; ++c) {
        const double eR = fabs((double)((ld)R[a][c] - Rw[a][c]));
        if (!(eR <= 4.0 * u52)) violation("compose R", trial, eR, 4.0 * u52);
      }
    }
  }
  printf("rotation: %d triples, worst |Rd Rd^T - I| = %.3f * 2^-52, worst |Rd - exact| = %.3f * 2^-52\n", trials,
         worst_orth / u52, worst_rot / u52);
  printf("compose: worst |T - exact| = %.3e\n", worst_comp);
}

int main() {
  static_assert(icp_upper(0, 0) == 0 && icp_upper(0, 5) == 5 && icp_upper(1, 1) == 6 && icp_upper(5, 5) == 20,
                "the packed upper triangle, row by row");
  check_cholesky();
  check_degenerate();
  check_rotation_and_compose();
  if (g_violations) {
    printf("%d VIOLATIONS\n", g_violations);
    return 1;
  }
  printf("no violation\n");
  return 0;
}

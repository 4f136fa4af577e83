// icp_plane.h -- the per-cloud arithmetic of registration_icp's point-to-plane update (registration.hip): the 6x6
// Cholesky solve with the degeneracy rule, the exact rotation from three angles, and the fp64 compose of a step onto
// the accumulated transform.  __host__ __device__ and free of HIP types: tests/native/icp_plane_main.cpp compiles this
// header alone, with any C++ compiler.  The definition these functions implement is the REGISTRATION block of
// include/pointops_amd.h; all arithmetic is unfused fp64 in the order written (the build passes -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define POINTOPS_ICP_HD __host__ __device__ inline
#else
#define POINTOPS_ICP_HD inline
#endif

namespace pointops {

// A Cholesky pivot at or below this fraction of the ORIGINAL diagonal entry of its row makes the normal equations
// degenerate: the cloud freezes with status 1 and keeps its transform.  A definition, not a measurement.  A system of
// condition number 1/kIcpDegeneratePivot or better never trips it, and exact zeros (one axis-aligned plane as the
// target) always do.  In between the rule is a heuristic: rounding leaves a deficient pivot a residue of about 2^-53 of
// the diagonal TIMES the growth of the elimination before it, so a rank-deficient system whose leading block is itself
// nearly singular can keep a residue above the threshold and be solved (into a huge, meaningless x).
// tests/native/icp_plane_main.cpp counts them: 2 of 6000 random rank 3-5 matrices.  Nothing else guards against it.
constexpr double kIcpDegeneratePivot = 1e-10;

constexpr int kIcpMinPlane = 6;   // fewest inliers of a point-to-plane update
constexpr int kIcpMinPoint = 3;   // fewest inliers of a point-to-point update

constexpr int kIcpUpper = 21;     // entries of the upper triangle of the 6x6 matrix, row by row
// slot of A[r][c], r <= c, in the packed upper triangle: (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
POINTOPS_ICP_HD constexpr int icp_upper(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }

// Solve A x = b for the symmetric A given by its packed upper triangle `up`, by A = L L^T.  Returns false -- x is then
// not written -- when pivot j, the diagonal entry of row j after the eliminations of rows < j, is not greater than
// kIcpDegeneratePivot * A[j][j] (a NaN pivot or diagonal is degenerate as well).
POINTOPS_ICP_HD bool icp_cholesky_solve6(const double* up, const double* b, double* x) {
  double L[6][6];
  for (int j = 0; j < 6; ++j) {
    const double diag = up[icp_upper(j, j)];
    double piv = diag;
    for (int k = 0; k < j; ++k) piv = piv - L[j][k] * L[j][k];
    if (!(piv > kIcpDegeneratePivot * diag)) return false;
    const double ljj = sqrt(piv);
    L[j][j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double v = up[icp_upper(j, i)];
      for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
      L[i][j] = v / ljj;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  return true;
}

// Rd = (Rz(gamma) Ry(beta) Rx(alpha))^T: the row-vector form (x -> x Rd) of the column-vector rotation about x, then
// y, then z.  Built from the sines and cosines themselves, not linearised.
POINTOPS_ICP_HD void icp_rotation(double alpha, double beta, double gamma, double (&Rd)[3][3]) {
  const double ca = cos(alpha), sa = sin(alpha), cb = cos(beta), sb = sin(beta), cg = cos(gamma), sg = sin(gamma);
  // M = Rz Ry Rx (column vectors); Rd[r][c] = M[c][r]
  Rd[0][0] = cg * cb;
  Rd[1][0] = cg * sb * sa - sg * ca;
  Rd[2][0] = cg * sb * ca + sg * sa;
  Rd[0][1] = sg * cb;
  Rd[1][1] = sg * sb * sa + cg * ca;
  Rd[2][1] = sg * sb * ca - cg * sa;
  Rd[0][2] = -sb;
  Rd[1][2] = cb * sa;
  Rd[2][2] = cb * ca;
}

// The step x -> (x - c0) Rd + c0 + t after the transform x -> x R + T:  R <- R Rd,  T <- (T - c0) Rd + c0 + t.
POINTOPS_ICP_HD void icp_compose(double (&R)[3][3], double (&T)[3], const double (&Rd)[3][3], const double (&c0)[3],
                                 const double (&t)[3]) {
  double Rn[3][3], Tn[3];
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 3; ++c) Rn[a][c] = (R[a][0] * Rd[0][c] + R[a][1] * Rd[1][c]) + R[a][2] * Rd[2][c];
  const double d[3] = {T[0] - c0[0], T[1] - c0[1], T[2] - c0[2]};
  for (int c = 0; c < 3; ++c) Tn[c] = (((d[0] * Rd[0][c] + d[1] * Rd[1][c]) + d[2] * Rd[2][c]) + c0[c]) + t[c];
  for (int a = 0; a < 3; ++a) {
    T[a] = Tn[a];
    for (int c = 0; c < 3; ++c) R[a][c] = Rn[a][c];
  }
}

}  // namespace pointops

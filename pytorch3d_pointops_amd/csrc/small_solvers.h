// small_solvers.h -- the per-lane 3x3 / 2x2 solvers of local_frames.hip and points_alignment.hip, __host__ __device__.
//
//   sym3_eigen     cyclic Jacobi in fp64 on a symmetric fp32 3x3 matrix: ascending eigenvalues, eigenvectors as columns,
//                  rounded to fp32 (local_frames_kernel); sym3_eigen_f64 is its fp64-in, fp64-out core (plane refits).
//   pa_svd<D>      one-sided Jacobi SVD of a d x d fp64 matrix, U completed by orthogonality where a singular value is
//                  negligible; pa_solve<D> turns the reduced alignment moments into R, T, s (alignment_solve_kernel).
//   pa_accumulate  one pair's addends to those moments and pa_pivots<D> the pivots they are taken about
//                  (alignment_moments_kernel; registration.hip's point-to-point sums with w = 1).
//   dot3f, cross3f fp32 3-vectors (fpfh.hip, local_frames.hip).
//
// They live here so that a host program can run them on millions of matrices without a GPU
// (tests/native/small_solvers_main.cpp); the kernels include this header and nothing else defines the functions.
#pragma once
#include "common.h"

namespace pointops {

// ------------------------------------------------------------------------------------------ fp32 3-vectors
__host__ __device__ __forceinline__ float dot3f(const float (&a)[3], const float (&b)[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

__host__ __device__ __forceinline__ void cross3f(const float (&a)[3], const float (&b)[3], float (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// ------------------------------------------------------------------------------------------ symmetric 3x3 eigensolver
constexpr int kJacobiMaxSweeps = 12;  // 3x3 cyclic Jacobi converges quadratically: 4-6 sweeps in practice
constexpr double kJacobiTol = 1e-30;  // stop when sum of squared off-diagonals <= tol * sum of squared diagonals

// One Jacobi rotation zeroing a[P][Q] (Numerical Recipes' form); v accumulates the rotations as columns.
template <int P, int Q>
__host__ __device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double at = fabs(theta);
  double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  a[R][P] = a[P][R] = arp - s * (arq + tau * arp);
  a[R][Q] = a[Q][R] = arq + s * (arp - tau * arq);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double g = v[k][P], h = v[k][Q];
    v[k][P] = g - s * (h + tau * g);
    v[k][Q] = h + s * (g - tau * h);
  }
}

// Stable compare-exchange of eigenpairs I < J (ascending eigenvalues; equal values keep their order).
template <int I, int J>
__host__ __device__ __forceinline__ void eig_order(double (&l)[3], double (&v)[3][3]) {
  if (l[I] > l[J]) {
    const double t = l[I];
    l[I] = l[J];
    l[J] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double u = v[k][I];
      v[k][I] = v[k][J];
      v[k][J] = u;
    }
  }
}

// The fp64 core: cyclic Jacobi on the symmetric matrix a (destroyed), then the stable ordering.  Ascending eigenvalues
// l, eigenvectors as columns of v.  (segment_plane's refit calls it on an fp64 covariance: plane_hypothesis.h.)
__host__ __device__ __forceinline__ void sym3_eigen_f64(double (&a)[3][3], double (&l)[3], double (&v)[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) v[r][q] = r == q ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiMaxSweeps; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (off <= kJacobiTol * diag) break;  // also ends a zero matrix before any rotation
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<1, 2>(a, v);
  }
  l[0] = a[0][0];
  l[1] = a[1][1];
  l[2] = a[2][2];
  eig_order<0, 1>(l, v);
  eig_order<1, 2>(l, v);
  eig_order<0, 1>(l, v);
}

// Eigen-decomposition of the symmetric fp32 matrix c: ascending eigenvalues lam, eigenvectors as columns of vec.
__host__ __device__ __forceinline__ void sym3_eigen(const float (&c)[3][3], float (&lam)[3], float (&vec)[3][3]) {
  double a[3][3], l[3], v[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) a[r][q] = (double)c[r][q];
  sym3_eigen_f64(a, l, v);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    lam[r] = (float)l[r];
#pragma unroll
    for (int q = 0; q < 3; ++q) vec[r][q] = (float)v[r][q];
  }
}

// ------------------------------------------------------------------------------------------ d x d SVD and alignment
constexpr int kSvdMaxSweeps = 30;      // one-sided Jacobi converges quadratically: 3-5 sweeps in practice
constexpr double kSvdTol = 1e-15;      // columns count as orthogonal when |a_p . a_q| <= tol |a_p| |a_q|
constexpr double kSvdNegligible = 1e-12;  // sigma_j <= this * sigma_1: direction j of U comes from orthogonality

__host__ __device__ constexpr int pa_moments(int D) { return 3 + 4 * D + D * D; }
// moment slots: 0 Sw, 1 Sw2, then D each of Swx, Swy, Sw2x, Sw2y, then D*D of Sxy (row = x), then Sxx
template <int D>
struct PaSlot {
  static constexpr int kSw = 0, kSw2 = 1, kSwx = 2, kSwy = 2 + D, kSw2x = 2 + 2 * D, kSw2y = 2 + 3 * D,
                       kSxy = 2 + 4 * D, kSxx = 2 + 4 * D + D * D, kCount = 3 + 4 * D + D * D;
};

// The pivots of cloud n: row 0 of X and of Y (zero for a cloud without rows).  The moments are sums about them, so that
// clouds far from the origin lose nothing to cancellation.
template <int D>
__host__ __device__ __forceinline__ void pa_pivots(const float* __restrict__ X, const float* __restrict__ Y, int n, int P,
                                                   int P2, int64_t len, double (&px)[D], double (&py)[D]) {
  const bool hx = len > 0, hy = len > 0 && P2 > 0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    px[d] = hx ? (double)X[(int64_t)n * P * D + d] : 0.0;
    py[d] = hy ? (double)Y[(int64_t)n * P2 * D + d] : 0.0;
  }
}

// One pair's addends to the moments acc[PaSlot<D>::kCount]: weight w, x and y about the pivots.  THE statement sequence
// of the sums (alignment_moments_kernel; registration_moments_kernel's point-to-point branch with w = 1, whose products
// by 1.0 are exact): reordering it changes result bits.
template <int D, int M>
__host__ __device__ __forceinline__ void pa_accumulate(double (&acc)[M], double w, const double (&x)[D],
                                                       const double (&y)[D]) {
  using S = PaSlot<D>;
  static_assert(M >= S::kCount, "the moments are the first slots of acc");
  const double w2 = w * w;
  acc[S::kSw] += w;
  acc[S::kSw2] += w2;
  double xx = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    acc[S::kSwx + a] += w * x[a];
    acc[S::kSwy + a] += w * y[a];
    const double w2x = w2 * x[a];
    acc[S::kSw2x + a] += w2x;
    acc[S::kSw2y + a] += w2 * y[a];
#pragma unroll
    for (int b = 0; b < D; ++b) acc[S::kSxy + a * D + b] += w2x * y[b];
    xx += w2x * x[a];
  }
  acc[S::kSxx] += xx;
}

// d x d solve (fp64, one lane).  A = C on entry; on exit A V = U S: columns of A are orthogonal.
template <int D>
__host__ __device__ __forceinline__ void pa_one_sided_jacobi(double (&A)[D][D], double (&V)[D][D]) {
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kSvdMaxSweeps; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < D - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) {
          alpha += A[r][p] * A[r][p];
          beta += A[r][q] * A[r][q];
          gamma += A[r][p] * A[r][q];
        }
        if (gamma == 0.0 || fabs(gamma) <= kSvdTol * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double az = fabs(zeta);
        double t = az > 1e150 ? 0.5 / az : 1.0 / (az + sqrt(az * az + 1.0));
        if (zeta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = c * t;
#pragma unroll
        for (int r = 0; r < D; ++r) {
          const double ap = A[r][p], aq = A[r][q];
          A[r][p] = c * ap - s * aq;
          A[r][q] = s * ap + c * aq;
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = c * vp - s * vq;
          V[r][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
}

template <int D>
__host__ __device__ __forceinline__ void pa_swap_cols(double (&A)[D][D], double (&V)[D][D], double (&sg)[D], int i,
                                                      int j) {
  if (sg[i] >= sg[j]) return;  // descending, stable
  const double t = sg[i];
  sg[i] = sg[j];
  sg[j] = t;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    double u = A[r][i];
    A[r][i] = A[r][j];
    A[r][j] = u;
    u = V[r][i];
    V[r][i] = V[r][j];
    V[r][j] = u;
  }
}

template <int D>
__host__ __device__ __forceinline__ double pa_det(const double (&m)[D][D]) {
  if constexpr (D == 2) {
    return m[0][0] * m[1][1] - m[0][1] * m[1][0];
  } else {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
  }
}

// C (d x d, fp64) -> singular values sg (descending), U, V with C = U diag(sg) V^T, U and V orthogonal for ANY C:
// a negligible sigma_j takes its column of U from orthogonality, and a zero C gives U = V = I.
template <int D>
__host__ __device__ __forceinline__ void pa_svd(const double (&C)[D][D], double (&U)[D][D], double (&sg)[D],
                                                double (&V)[D][D]) {
  static_assert(D == 2 || D == 3, "closed completion of U for d = 2, 3");
  double A[D][D];
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c) A[r][c] = C[r][c];
  pa_one_sided_jacobi<D>(A, V);
#pragma unroll
  for (int c = 0; c < D; ++c) {
    double q = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) q += A[r][c] * A[r][c];
    sg[c] = sqrt(q);
  }
  pa_swap_cols<D>(A, V, sg, 0, 1);
  if constexpr (D == 3) {
    pa_swap_cols<D>(A, V, sg, 1, 2);
    pa_swap_cols<D>(A, V, sg, 0, 1);
  }
  if (!(sg[0] > 0.0)) {  // C == 0: no rotation happened, V = I and so is U
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
      for (int c = 0; c < D; ++c) U[r][c] = V[r][c];
    return;
  }
  const double detV = pa_det<D>(V);
  double u0[D];
#pragma unroll
  for (int r = 0; r < D; ++r) u0[r] = A[r][0] / sg[0];
  if constexpr (D == 2) {
    // the last column is the perpendicular of the first, on the side of A's column (det U V^T = +1 when that is nil)
    double u1[2] = {-u0[1], u0[0]};
    const double side = u1[0] * A[0][1] + u1[1] * A[1][1];
    const bool flip = sg[1] > kSvdNegligible * sg[0] ? side < 0.0 : detV < 0.0;
    const double f = flip ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      U[r][0] = u0[r];
      U[r][1] = f * u1[r];
    }
  } else {
    double u1[3];
    if (sg[1] > kSvdNegligible * sg[0]) {
#pragma unroll
      for (int r = 0; r < 3; ++r) u1[r] = A[r][1] / sg[1];
    } else {  // any unit vector perpendicular to u0: u0 x (the axis u0 leans on least)
      const double a0 = fabs(u0[0]), a1 = fabs(u0[1]), a2 = fabs(u0[2]);
      const bool k0 = a0 <= a1 && a0 <= a2, k1 = !k0 && a1 <= a2;
      const double e[3] = {k0 ? 1.0 : 0.0, k1 ? 1.0 : 0.0, (k0 || k1) ? 0.0 : 1.0};
      u1[0] = u0[1] * e[2] - u0[2] * e[1];
      u1[1] = u0[2] * e[0] - u0[0] * e[2];
      u1[2] = u0[0] * e[1] - u0[1] * e[0];
      const double nrm = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
      for (int r = 0; r < 3; ++r) u1[r] /= nrm;
    }
    // the last column is +-(u0 x u1): Jacobi left A's columns orthogonal to rounding, so this IS a_2 / sigma_2 where
    // that is meaningful, and stays a unit vector where it is not
    double u2[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
    const double side = u2[0] * A[0][2] + u2[1] * A[1][2] + u2[2] * A[2][2];
    const bool flip = (sg[1] > kSvdNegligible * sg[0] && sg[2] > kSvdNegligible * sg[0]) ? side < 0.0 : detV < 0.0;
    const double f = flip ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      U[r][0] = u0[r];
      U[r][1] = u1[r];
      U[r][2] = f * u2[r];
    }
  }
}

// Reduced raw moments (about the pivots px, py) -> R (d x d), T (d), s, singular values of C; all fp64.
template <int D>
__host__ __device__ __forceinline__ void pa_solve(const double* mom, const double (&px)[D], const double (&py)[D],
                                                  bool estimate_scale, bool allow_reflection, double eps,
                                                  double (&R)[D][D], double (&T)[D], double& s, double (&sg)[D]) {
  using S = PaSlot<D>;
  const double W = mom[S::kSw] > eps ? mom[S::kSw] : eps;
  const double sw2 = mom[S::kSw2];
  double xm[D], ym[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    xm[d] = mom[S::kSwx + d] / W;
    ym[d] = mom[S::kSwy + d] / W;
  }
  double C[D][D];
  double xcov = mom[S::kSxx];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    xcov += xm[a] * (sw2 * xm[a] - 2.0 * mom[S::kSw2x + a]);
#pragma unroll
    for (int b = 0; b < D; ++b)
      C[a][b] = (mom[S::kSxy + a * D + b] - xm[a] * mom[S::kSw2y + b] - mom[S::kSw2x + a] * ym[b] +
                 sw2 * xm[a] * ym[b]) / W;
  }
  xcov /= W;
  double U[D][D], V[D][D];
  pa_svd<D>(C, U, sg, V);
  const double e = allow_reflection ? 1.0 : (pa_det<D>(U) * pa_det<D>(V) < 0.0 ? -1.0 : 1.0);
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double r = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) r += (k == D - 1 ? e : 1.0) * U[a][k] * V[b][k];
      R[a][b] = r;
    }
  s = 1.0;
  if (estimate_scale) {
    double tr = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) tr += (k == D - 1 ? e : 1.0) * sg[k];
    s = tr / (xcov > eps ? xcov : eps);
  }
  // the means about the origin: sum w x / W = px * (sum w / W) + xm.  The factor is exactly 1 unless W was clamped to
  // eps -- a cloud whose weights are all zero (sum w = 0) has the means 0 and T = 0, whatever its row 0 holds
  const double pw = mom[S::kSw] / W;
#pragma unroll
  for (int b = 0; b < D; ++b) {
    double xr = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) xr += (px[a] * pw + xm[a]) * R[a][b];
    T[b] = (py[b] * pw + ym[b]) - s * xr;
  }
}

}  // namespace pointops

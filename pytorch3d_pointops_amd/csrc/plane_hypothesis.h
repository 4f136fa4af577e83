// plane_hypothesis.h -- the per-lane routines of plane.hip, __host__ __device__: the plane through three points with
// its validity tests, the sign rule, the fp32 residual, and the refit of a plane from fp64 moments.  (The counter-based
// draws are those of consensus_draw.h.)
//
// They live here so that a host program can run them on millions of triples without a GPU
// (tests/native/plane_hypothesis_main.cpp); the kernels include this header and nothing else defines the functions.
// The normative text is the comment of pointops_segment_plane in include/pointops_amd.h.
#pragma once
#include "small_solvers.h"

namespace pointops {

constexpr double kPlaneDegenerate = 1e-12;  // |e1 x e2|^2 must exceed this times |e1|^2 |e2|^2

// The optional cone of admissible normals: a unit axis (fp32, normalised by the host) and cos(max_angle) (fp32).
struct PlaneCone {
  int use;
  float a[3];
  float cos_max;
};

__host__ __device__ __forceinline__ double ph_sqnorm(const double (&v)[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }

__host__ __device__ __forceinline__ double ph_axis_dot(const double (&v)[3], const PlaneCone& cone) {
  return (v[0] * (double)cone.a[0] + v[1] * (double)cone.a[1]) + v[2] * (double)cone.a[2];
}

// (v . axis)^2 >= cos^2 |v|^2: multiplies and adds only.  False for NaN.
__host__ __device__ __forceinline__ bool ph_in_cone(const double (&v)[3], double sq, const PlaneCone& cone) {
  const double dot = ph_axis_dot(v, cone), c = (double)cone.cos_max;
  return dot * dot >= (c * c) * sq;
}

// The sign rule on a unit normal n and its offset d: with a cone n . axis >= 0, else the component of largest magnitude
// (the lowest index among equals) is positive.
__host__ __device__ __forceinline__ void ph_orient(double (&n)[3], double& d, const PlaneCone& cone) {
  bool flip;
  if (cone.use) {
    flip = ph_axis_dot(n, cone) < 0.0;
  } else {
    int k = 0;
    if (fabs(n[1]) > fabs(n[k])) k = 1;
    if (fabs(n[2]) > fabs(n[k])) k = 2;
    flip = (k == 0 ? n[0] : (k == 1 ? n[1] : n[2])) < 0.0;
  }
  if (flip) {
    n[0] = -n[0];
    n[1] = -n[1];
    n[2] = -n[2];
    d = -d;
  }
}

// The plane (a, b, c, d) through three fp32 points, in fp64, rounded once; false (and zeros) when the triple is
// degenerate -- collinear, coincident, not finite -- or its normal leaves the cone.
__host__ __device__ __forceinline__ bool ph_plane(const float (&p)[3][3], const PlaneCone& cone, float (&plane)[4]) {
  plane[0] = plane[1] = plane[2] = plane[3] = 0.0f;
  const double p0[3] = {(double)p[0][0], (double)p[0][1], (double)p[0][2]};
  const double e1[3] = {(double)p[1][0] - p0[0], (double)p[1][1] - p0[1], (double)p[1][2] - p0[2]};
  const double e2[3] = {(double)p[2][0] - p0[0], (double)p[2][1] - p0[1], (double)p[2][2] - p0[2]};
  const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double sq = ph_sqnorm(c);
  if (!(sq > (kPlaneDegenerate * ph_sqnorm(e1)) * ph_sqnorm(e2))) return false;
  if (cone.use && !ph_in_cone(c, sq, cone)) return false;
  const double len = sqrt(sq);
  double n[3] = {c[0] / len, c[1] / len, c[2] / len};
  double d = -((n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2]);
  ph_orient(n, d, cone);
  plane[0] = (float)n[0];
  plane[1] = (float)n[1];
  plane[2] = (float)n[2];
  plane[3] = (float)d;
  // (fp32 coordinates cannot overflow the fp64 cross product; only the offset can leave fp32: such a triple is invalid)
  if (!(fabsf(plane[3]) < INFINITY)) {
    plane[0] = plane[1] = plane[2] = plane[3] = 0.0f;
    return false;
  }
  return true;
}

// The residual of the score and of the evaluation, unfused, in this order.
__host__ __device__ __forceinline__ float ph_residual(float a, float b, float c, float d, float x, float y, float z) {
  return ((x * a + y * b) + z * c) + d;
}

// Moment slots of the refit: S1, S q (3), S q q^T (xx, xy, xz, yy, yz, zz), q = p - pivot.
constexpr int kPlaneMoments = 10;

// The least-squares plane of the moments about `pivot`: centroid and covariance in fp64, the eigenvector of the
// smallest eigenvalue (sym3_eigen_f64), the sign rule, one rounding.  False (and zeros) with fewer than three points,
// when anything is not finite, or when the normal leaves the cone.
__host__ __device__ __forceinline__ bool ph_refit(const double (&mom)[kPlaneMoments], const double (&pivot)[3],
                                                  const PlaneCone& cone, float (&plane)[4]) {
  plane[0] = plane[1] = plane[2] = plane[3] = 0.0f;
  if (!(mom[0] >= 3.0)) return false;
  const double w = mom[0];
  const double m[3] = {mom[1] / w, mom[2] / w, mom[3] / w};
  double a[3][3], l[3], v[3][3];
  a[0][0] = mom[4] / w - m[0] * m[0];
  a[0][1] = a[1][0] = mom[5] / w - m[0] * m[1];
  a[0][2] = a[2][0] = mom[6] / w - m[0] * m[2];
  a[1][1] = mom[7] / w - m[1] * m[1];
  a[1][2] = a[2][1] = mom[8] / w - m[1] * m[2];
  a[2][2] = mom[9] / w - m[2] * m[2];
  sym3_eigen_f64(a, l, v);
  double n[3] = {v[0][0], v[1][0], v[2][0]};
  const double sq = ph_sqnorm(n);
  if (!(sq > 0.5 && sq < 2.0)) return false;  // (NaN moments; Jacobi keeps v orthonormal to rounding otherwise)
  if (cone.use && !ph_in_cone(n, sq, cone)) return false;
  const double len = sqrt(sq);
  n[0] /= len;
  n[1] /= len;
  n[2] /= len;
  double d = -((n[0] * (pivot[0] + m[0]) + n[1] * (pivot[1] + m[1])) + n[2] * (pivot[2] + m[2]));
  ph_orient(n, d, cone);
  if (!(fabs(d) < 3.0e38)) return false;
  plane[0] = (float)n[0];
  plane[1] = (float)n[1];
  plane[2] = (float)n[2];
  plane[3] = (float)d;
  return true;
}

}  // namespace pointops

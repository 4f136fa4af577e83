// iss.hip -- ISS keypoint detection of a batch of clouds (C ABI: pointops_iss_keypoints; device half of
// functions/iss.py).  The definition is the comment block of the entry in include/pointops_amd.h: the support of a point
// is ball query's `dist2 < rs * rs`, its scatter matrix comes from INTEGER moments of the quantized offsets (so the sum
// does not depend on the order of the walk), the eigenvalues from sym3_eigen_f64, the decision from iss_saliency.h, and
// the keypoints are the local maxima of the saliency within rn, ties to the lower index.
//
// A fixed sequence of launches, stream-ordered, nothing read back, no atomics beyond grid_build's:
//   prepare   radius_walk_prepare with cell_radius = max(rs, rn): the lengths clamped into [0, P], and for clouds of 512
//             points and more ONE grid for both walks
//   saliency  one lane per point in cell order, one full walk with rs: per hit three quantized offsets and nine int64
//             multiply-adds; then covariance, eigenvalues, decision -> eigenvalues, saliency (and moments) at the
//             point's own index, and the saliency once more at the lane's position in the cell order
//   nms       one lane per point, one walk with rn: counts |T_i| and looks for a hit that beats the lane, reading the
//             saliency beside the records (cell order) on the cube path and by index on the raw-cloud path -> mask
// Padding rows are written by the saliency and nms launches themselves.  Each walk takes radius_walk.h's certificate
// with its own r2; a lane without it, a refused grid and a small cloud walk all pairs, which never changes a result.
// POINTOPS_DEBUG=iss_grid=0|1 forces either path.
#include <limits.h>

#include "iss_saliency.h"
#include "radius_walk.h"
#include "small_solvers.h"

namespace pointops {

constexpr int kIssMoments = 10;  // n, M1[3], M2[6]

struct IssParams {
  double s;           // iss_scale(rs)
  float g21, g32;
  int min_neighbors;
};

__global__ __launch_bounds__(kWalkBlock) void iss_saliency_kernel(WalkView v, IssParams p, float* __restrict__ eigenvalues,
                                                                  float* __restrict__ saliency, float* __restrict__ sal_cell,
                                                                  int64_t* __restrict__ moments) {
  const WalkItem it = walk_item(v);
  if (it.t >= v.P) return;
  const int64_t base = (int64_t)it.n * v.P;
  if (it.t >= it.len) {  // padding rows
    float* const ev = eigenvalues + (base + it.t) * 3;
    ev[0] = ev[1] = ev[2] = 0.0f;
    saliency[base + it.t] = 0.0f;
    if (moments != nullptr)
      for (int k = 0; k < kIssMoments; ++k) moments[(base + it.t) * kIssMoments + k] = 0;
    return;
  }
  const WalkLane<3> L = walk_lane<3>(v, it);
  int64_t cnt = 0, M1[3] = {0, 0, 0}, M2[6] = {0, 0, 0, 0, 0, 0};
  radius_walk_records<3>(v, it, L, [&](int, const float4& c, int) {
    const int32_t qx = iss_quantize(c.x, L.x, p.s), qy = iss_quantize(c.y, L.y, p.s), qz = iss_quantize(c.z, L.z, p.s);
    ++cnt;
    M1[0] += qx, M1[1] += qy, M1[2] += qz;
    M2[0] += (int64_t)qx * qx, M2[1] += (int64_t)qx * qy, M2[2] += (int64_t)qx * qz;
    M2[3] += (int64_t)qy * qy, M2[4] += (int64_t)qy * qz, M2[5] += (int64_t)qz * qz;
    return true;
  });
  double C[6], a[3][3], l[3], vec[3][3];
  iss_covariance(M1, M2, cnt, p.s, C);
  a[0][0] = C[0], a[0][1] = a[1][0] = C[1], a[0][2] = a[2][0] = C[2];
  a[1][1] = C[3], a[1][2] = a[2][1] = C[4], a[2][2] = C[5];
  sym3_eigen_f64(a, l, vec);
  const float lam[3] = {(float)l[0], (float)l[1], (float)l[2]};
  const float sal = iss_saliency(lam, p.g21, p.g32);
  float* const ev = eigenvalues + (base + L.i) * 3;
  ev[0] = lam[0], ev[1] = lam[1], ev[2] = lam[2];
  saliency[base + L.i] = sal;
  sal_cell[base + it.t] = sal;  // lane t IS position t of the cell order (or point t where the cloud has no grid)
  if (moments != nullptr) {
    int64_t* const m = moments + (base + L.i) * kIssMoments;
    m[0] = cnt;
    for (int k = 0; k < 3; ++k) m[1 + k] = M1[k];
    for (int k = 0; k < 6; ++k) m[4 + k] = M2[k];
  }
}

__global__ __launch_bounds__(kWalkBlock) void iss_nms_kernel(WalkView v, IssParams p, const float* __restrict__ saliency,
                                                             const float* __restrict__ sal_cell,
                                                             uint8_t* __restrict__ mask) {
  const WalkItem it = walk_item(v);
  if (it.t >= v.P) return;
  const int64_t base = (int64_t)it.n * v.P;
  if (it.t >= it.len) {
    mask[base + it.t] = 0;  // padding rows
    return;
  }
  const WalkLane<3> L = walk_lane<3>(v, it);
  const float si = sal_cell[base + it.t];
  bool keep = si > 0.0f;
  if (keep) {
    int cnt = 0;
    radius_walk_records<3>(v, it, L, [&](int j, const float4&, int k) {
      // (position k of the cell order on the cube path; the raw-cloud path of a cloud WITH a grid has the index only)
      const float sj = k >= 0 ? sal_cell[base + k] : saliency[base + j];
      if (iss_beats(sj, j, si, L.i)) {
        keep = false;
        return false;  // beaten: the count no longer matters
      }
      if (cnt < p.min_neighbors) ++cnt;
      return true;
    });
    keep = keep && cnt >= p.min_neighbors;
  }
  mask[base + L.i] = keep ? 1 : 0;
}

static bool iss_shape_ok(int64_t N, int64_t P) {
  // (a cloud is a grid's y coordinate; 2^24 hits keep the int64 moments below 2^63)
  return N >= 0 && N < 65536 && P >= 0 && P <= kIssMaxPoints;
}

struct IssLayout {
  WalkLayout walk;
  float* sal_cell;  // (N, P) the saliency in cell order
  size_t bytes;
};

static IssLayout iss_layout(void* ws, int64_t N, int64_t P) {
  Carver c(ws);
  IssLayout l;
  l.walk = radius_walk_carve(c, "iss_grid", N, P);
  l.sal_cell = (float*)c.take(sizeof(float) * (size_t)N * (size_t)P);
  l.bytes = c.off;
  return l;
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_iss_workspace_bytes(int64_t N, int64_t P) {
  if (!iss_shape_ok(N, P) || N == 0) return 0;
  return iss_layout(nullptr, N, P).bytes;
}

extern "C" int pointops_iss_keypoints(const float* points, const int64_t* lengths, int64_t N, int64_t P,
                                      float salient_radius, float non_max_radius, float gamma_21, float gamma_32,
                                      int64_t min_neighbors, float* eigenvalues, float* saliency, uint8_t* mask,
                                      int64_t* moments, void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(iss_shape_ok(N, P), "iss_keypoints: need 0 <= N < 65536 and 0 <= P <= 2^24");
  POINTOPS_REQUIRE(salient_radius > 0.0f && salient_radius <= FLT_MAX && non_max_radius > 0.0f &&
                       non_max_radius <= FLT_MAX,
                   "iss_keypoints: need finite radii > 0");
  POINTOPS_REQUIRE(gamma_21 > 0.0f && gamma_21 <= FLT_MAX && gamma_32 > 0.0f && gamma_32 <= FLT_MAX &&
                       min_neighbors >= 0,
                   "iss_keypoints: need finite gamma_21, gamma_32 > 0 and min_neighbors >= 0");
  if (N == 0) return POINTOPS_OK;
  const IssLayout l = iss_layout(workspace, N, P);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "iss_keypoints: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  WalkView vs;
  const float cell_radius = salient_radius > non_max_radius ? salient_radius : non_max_radius;  // ONE grid, both walks
  const int rc = radius_walk_prepare(l.walk, points, lengths, N, P, 3, cell_radius, stream, &vs);
  if (rc != POINTOPS_OK) return rc;
  if (P == 0) return check_launch("iss_keypoints");
  vs.r2 = salient_radius * salient_radius;  // fp32 products, as ball query's radius2
  WalkView vn = vs;
  vn.r2 = non_max_radius * non_max_radius;
  IssParams p;
  p.s = iss_scale(salient_radius);
  p.g21 = gamma_21;
  p.g32 = gamma_32;
  p.min_neighbors = (int)(min_neighbors > INT_MAX ? INT_MAX : min_neighbors);
  const dim3 pgrid((unsigned)ceil_div(P, kWalkBlock), (unsigned)N);
  hipLaunchKernelGGL(iss_saliency_kernel, pgrid, dim3(kWalkBlock), 0, stream, vs, p, eigenvalues, saliency, l.sal_cell,
                     moments);
  hipLaunchKernelGGL(iss_nms_kernel, pgrid, dim3(kWalkBlock), 0, stream, vn, p, (const float*)saliency,
                     (const float*)l.sal_cell, mask);
  return check_launch("iss_keypoints");
}

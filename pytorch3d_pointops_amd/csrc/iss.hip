// iss.hip -- ISS keypoint detection of a batch of clouds (C ABI: pointops_iss_keypoints; device half of
// functions/iss.py).  The definition is the comment block of the entry in include/pointops_amd.h: the support of a point
// is ball query's `dist2 < rs * rs`, its scatter matrix comes from INTEGER moments of the quantized offsets (so the sum
// does not depend on the order of the walk), the eigenvalues from sym3_eigen_f64, the decision from iss_saliency.h, and
// the keypoints are the local maxima of the saliency within rn, ties to the lower index.
//
// A fixed sequence of launches, stream-ordered, nothing read back, no atomics beyond grid_build's:
//   lengths   the cloud lengths clamped into [0, P] (radius_walk.h's kernel)
//   grid      grid_build with same = true, h_min = 1.001 max(rs, rn), refine = -1, K = 0, as cluster_dbscan calls it: ONE
//             grid for both walks -- for clouds of kIssGridMinPoints points and more
//   saliency  one lane per point in cell order, one full walk with rs: per hit three quantized offsets and nine int64
//             multiply-adds; then covariance, eigenvalues, decision -> eigenvalues, saliency (and moments) at the
//             point's own index, and the saliency once more at the lane's position in the cell order
//   nms       one lane per point, one walk with rn: counts |T_i| and looks for a hit that beats the lane, reading the
//             saliency beside the records (cell order) on the cube path and by index on the raw-cloud path -> mask
// Padding rows are written by the saliency and nms launches themselves.  Each walk takes radius_walk.h's certificate
// with its own r2; a lane without it, a refused grid and a small cloud walk all pairs, which never changes a result.
// POINTOPS_DEBUG=iss_grid=0|1 forces either path.
#include <limits.h>

#include "debug.h"
#include "grid.h"
#include "iss_saliency.h"
#include "radius_walk.h"
#include "small_solvers.h"

namespace pointops {

constexpr float kIssCellTarget = 2.0f;   // density floor of the cell size (ball query's); the radii usually decide
constexpr int kIssGridMinPoints = 512;   // smaller clouds: all pairs (the build's fixed passes cost more)
constexpr int kIssMoments = 10;          // n, M1[3], M2[6]

struct IssParams {
  double s;           // iss_scale(rs)
  float g21, g32;
  int min_neighbors;
};

__global__ __launch_bounds__(kClBlock) void iss_saliency_kernel(ClusterView v, IssParams p, float* __restrict__ eigenvalues,
                                                              float* __restrict__ saliency, float* __restrict__ sal_cell,
                                                              int64_t* __restrict__ moments) {
  GridCloud g = {};
  const ClusterItem it = cluster_item(v, g);
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
  const ClusterLane<3> L = cluster_lane<3>(v, g, it.grid, it.n, it.t);
  int64_t cnt = 0, M1[3] = {0, 0, 0}, M2[6] = {0, 0, 0, 0, 0, 0};
  cluster_walk_records<3>(v, g, L, it.n, it.len, [&](int, const float4& c, int) {
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

__global__ __launch_bounds__(kClBlock) void iss_nms_kernel(ClusterView v, IssParams p, const float* __restrict__ saliency,
                                                         const float* __restrict__ sal_cell,
                                                         uint8_t* __restrict__ mask) {
  GridCloud g = {};
  const ClusterItem it = cluster_item(v, g);
  if (it.t >= v.P) return;
  const int64_t base = (int64_t)it.n * v.P;
  if (it.t >= it.len) {
    mask[base + it.t] = 0;  // padding rows
    return;
  }
  const ClusterLane<3> L = cluster_lane<3>(v, g, it.grid, it.n, it.t);
  const float si = sal_cell[base + it.t];
  bool keep = si > 0.0f;
  if (keep) {
    int cnt = 0;
    cluster_walk_records<3>(v, g, L, it.n, it.len, [&](int j, const float4&, int k) {
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

// whether the call builds grids (the per-cloud decision is grid_build's, on the device)
static bool iss_uses_grid(int64_t N, int64_t P) {
  const long force = debug_knob("iss_grid", -1);  // 0 = never, 1 = whenever the shape allows (tests)
  if (force == 0 || N <= 0 || P <= 0 || P > knn_grid_max_points()) return false;
  return force == 1 || P >= kIssGridMinPoints;
}

struct IssLayout {
  int64_t* len;     // (N,)
  float* sal_cell;  // (N, P) the saliency in cell order
  char* grid;       // grid_carve's
  size_t bytes;
};

static IssLayout iss_layout(void* ws, int64_t N, int64_t P, bool grid) {
  Carver c(ws);
  IssLayout l;
  l.len = (int64_t*)c.take(sizeof(int64_t) * (size_t)N);
  l.sal_cell = (float*)c.take(sizeof(float) * (size_t)N * (size_t)P);
  l.grid = c.take(grid ? grid_carve(nullptr, nullptr, N, P, P, kIssCellTarget) : 0);
  l.bytes = c.off;
  return l;
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_iss_workspace_bytes(int64_t N, int64_t P) {
  if (!iss_shape_ok(N, P) || N == 0) return 0;
  return iss_layout(nullptr, N, P, iss_uses_grid(N, P)).bytes;
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
  const bool grid = iss_uses_grid(N, P);
  const IssLayout l = iss_layout(workspace, N, P, grid);
  if (!workspace_fits(workspace, workspace_bytes, l.bytes)) {
    set_error("iss_keypoints: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
    return POINTOPS_EWORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(cluster_lengths_kernel, dim3((unsigned)ceil_div(N, kClBlock)), dim3(kClBlock), 0, stream, lengths,
                     (int)N, (int)P, l.len);
  if (P == 0) return check_launch("iss_keypoints");
  ClusterView vs{};
  vs.points = points;
  vs.len = l.len;
  vs.P = (int)P;
  vs.r2 = salient_radius * salient_radius;  // fp32 products, as ball query's radius2
  if (grid) {
    GridWs ws;
    grid_carve(&ws, l.grid, N, P, P, kIssCellTarget);
    // K = 0: the build's padding of search rows has nothing to write
    const KnnArgs a = make_knn_args(points, points, l.len, l.len, N, P, P, 3, 0, 0, nullptr, nullptr, stream);
    GridBuild b{};
    b.c_target = kIssCellTarget;
    b.h_min = (salient_radius > non_max_radius ? salient_radius : non_max_radius) * 1.001f;
    b.same = true;
    b.refine = -1;
    const int rc = grid_build(a, ws, b);
    if (rc != POINTOPS_OK) return rc;
    vs.clouds = ws.cloud;
    vs.edges = ws.edges;
    vs.cell_start = ws.cell_start;
    vs.sorted = ws.sorted;
    vs.cell_cap = ws.cell_cap;
  }
  ClusterView vn = vs;
  vn.r2 = non_max_radius * non_max_radius;
  IssParams p;
  p.s = iss_scale(salient_radius);
  p.g21 = gamma_21;
  p.g32 = gamma_32;
  p.min_neighbors = (int)(min_neighbors > INT_MAX ? INT_MAX : min_neighbors);
  const dim3 pgrid((unsigned)ceil_div(P, kClBlock), (unsigned)N);
  hipLaunchKernelGGL(iss_saliency_kernel, pgrid, dim3(kClBlock), 0, stream, vs, p, eigenvalues, saliency, l.sal_cell,
                     moments);
  hipLaunchKernelGGL(iss_nms_kernel, pgrid, dim3(kClBlock), 0, stream, vn, p, (const float*)saliency,
                     (const float*)l.sal_cell, mask);
  return check_launch("iss_keypoints");
}

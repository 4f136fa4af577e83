// knn_in_radius.hip -- the K nearest points INSIDE a radius, sorted (C ABI: pointops_knn_in_radius; device half of
// functions/knn_in_radius.py).  The definition is the comment block of the entry in include/pointops_amd.h: the
// candidates of a query are ball query's (`d2 < fl32(radius * radius)`, point_dist<D, 2> of grid.h), the answer is the
// first K of them in ascending (d2, j) order.
//
// The radius is the certificate.  The target's grid has cells at least 1.001 radius wide (grid_build with h_min, as
// ball_grid.hip and radius_walk.hip build theirs), so the 3x3x3 cube around a query's cell contains its ball; that is
// not assumed but proven per query by box_lower_bound<2>(...) >= r2 -- every point outside the cube has a computed d2
// of at least r2 and fails the comparison.  A query far outside the target's box is certified too: the faces that do
// not exist drop out of the bound, and its cube holds boundary cells only.
//   lengths   both sides clamped into [0, P] (a null `lengths` = P), for grid_build and the kernel
//   grid      grid_build (reuse = 0) or grid_build_queries (reuse = 1) with K = 0: the build pads no rows and this file
//             writes every row itself; queries in cell order (qsorted, or the point order when p1 IS p2)
//   search    ONE kernel (radius_knn_kernel.h), one lane per query: a certified lane walks the nine x-runs of its cube, any other lane -- no
//             certificate, a refused grid, a call too small for a grid -- the raw cloud in index order.  Both keep the
//             KC smallest keys (d2 bits << 32 | j) of knn_radius_list.h in registers and prune by `d2 < r2` and by the
//             list's largest key.  Keys are unique and their order is the (d2, j) order, so the order in which a lane
//             meets its candidates never shows: which path a lane takes depends on the input alone and changes no byte.
// No atomics beyond grid_build's (none on results), nothing read back, nothing synchronises; every launch is on the
// caller's stream.  POINTOPS_DEBUG=knn_in_radius_grid=0|1 forces the raw path / the grid at any size that allows one.
#include <float.h>

#include "debug.h"
#include "radius_knn_kernel.h"

namespace pointops {

constexpr float kRadiusKnnCellTarget = 2.0f; // density floor of the cell size (ball query's); the radius usually decides
constexpr int kRadiusKnnGridMinPoints = 512; // smaller targets: the raw cloud (the build's fixed passes cost more)

static bool radius_knn_shape_ok(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  return N >= 0 && N < 65536 && P1 >= 0 && P1 < (1LL << 30) && P2 >= 0 && P2 <= knn_grid_max_points() && D >= 1 &&
         D <= 3 && K >= 1 && K <= 64;
}

// Whether the call builds grids, from the shape alone (the per-cloud decision is grid_build's, on the device)
static bool radius_knn_uses_grid(int64_t N, int64_t P1, int64_t P2) {
  const long force = debug_knob("knn_in_radius_grid", -1);
  if (force == 0 || N <= 0 || P1 <= 0 || P2 <= 0) return false;
  return force == 1 || P2 >= kRadiusKnnGridMinPoints;
}

struct RadiusKnnLayout {
  int64_t* len1;  // (N,)
  int64_t* len2;
  char* grid;     // grid_carve's
  bool uses_grid;
  size_t bytes;
};

static RadiusKnnLayout radius_knn_layout(void* ws, int64_t N, int64_t P1, int64_t P2) {
  Carver c(ws);
  RadiusKnnLayout l;
  l.uses_grid = radius_knn_uses_grid(N, P1, P2);
  l.len1 = (int64_t*)c.take(sizeof(int64_t) * (size_t)N);
  l.len2 = (int64_t*)c.take(sizeof(int64_t) * (size_t)N);
  l.grid = c.take(l.uses_grid ? grid_carve(nullptr, nullptr, N, P1, P2, kRadiusKnnCellTarget) : 0);
  l.bytes = c.off;
  return l;
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_knn_in_radius_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  if (!radius_knn_shape_ok(N, P1, P2, D, K) || N == 0) return 0;
  return radius_knn_layout(nullptr, N, P1, P2).bytes;
}

extern "C" int pointops_knn_in_radius(const float* p1, const float* p2, const int64_t* lengths1,
                                      const int64_t* lengths2, int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K,
                                      float radius, int64_t* idxs, float* dists, int32_t* counts, void* workspace,
                                      size_t workspace_bytes, int reuse, void* stream_) {
  POINTOPS_REQUIRE(radius_knn_shape_ok(N, P1, P2, D, K),
                   "knn_in_radius: need 0 <= N < 65536, 0 <= P1 < 2^30, 0 <= P2 <= %lld, 1 <= D <= 3 and 1 <= K <= 64",
                   (long long)knn_grid_max_points());
  POINTOPS_REQUIRE(radius > 0.0f && radius <= FLT_MAX, "knn_in_radius: need a finite radius > 0");
  POINTOPS_REQUIRE(reuse == 0 || reuse == 1, "knn_in_radius: reuse is 0 or 1");
  if (N == 0) return POINTOPS_OK;
  const RadiusKnnLayout l = radius_knn_layout(workspace, N, P1, P2);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "knn_in_radius: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  if (P1 == 0) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  clamp_lengths_async(lengths1, N, P1, l.len1, stream);
  if (reuse == 0) clamp_lengths_async(lengths2, N, P2, l.len2, stream);
  RadiusKnnView v{};
  v.p1 = p1;
  v.p2 = p2;
  v.len1 = l.len1;
  v.len2 = l.len2;
  v.P1 = (int)P1;
  v.P2 = (int)P2;
  v.K = (int)K;
  v.r2 = radius * radius;  // fp32 product, as ball query's radius2
  if (l.uses_grid) {
    GridWs ws;
    grid_carve(&ws, l.grid, N, P1, P2, kRadiusKnnCellTarget);
    // K = 0: the build's padding of search rows has nothing to write
    const KnnArgs a = make_knn_args(p1, p2, l.len1, l.len2, N, P1, P2, D, 0, 0, nullptr, nullptr, stream);
    const bool same = p1 == p2 && lengths1 == lengths2 && P1 == P2 && debug_knob("grid_same", 1) != 0;
    int rc;
    if (reuse == 0) {
      GridBuild b{};
      b.c_target = kRadiusKnnCellTarget;
      b.h_min = radius * 1.001f;
      b.same = same;
      b.refine = -1;
      rc = grid_build(a, ws, b);
    } else {
      rc = grid_build_queries(a, ws, same, 1);
    }
    if (rc != POINTOPS_OK) return rc;
    v.clouds = ws.cloud;
    v.edges = ws.edges;
    v.cell_start = ws.cell_start;
    v.sorted = ws.sorted;
    v.qsorted = ws.qsorted;
    v.cell_cap = ws.cell_cap;
  }
  radius_knn_launch(v, N, stream, (int)D, idxs, dists, counts);
  return check_launch("knn_in_radius");
}

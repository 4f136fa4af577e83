// radius_walk.hip -- the host half of radius_walk.h: what the three operators that walk (cluster.hip, iss.hip, filters.hip) do
// before their own launches, and the lengths clamp (common.h's clamp_lengths_async) that voxel_downsample starts with too.
//   lengths   the cloud lengths clamped into [0, P] (a null `lengths` = P), for grid_build and every pass
//   grid      grid_build with same = true, h_min = 1.001 cell_radius, refine = -1, K = 0 (the KNN-style workspace): the
//             cloud sorted by cells at least cell_radius wide -- for clouds of kWalkGridMinPoints points and more
#include "radius_walk.h"

#include "debug.h"

namespace pointops {

constexpr float kWalkCellTarget = 2.0f;   // density floor of the cell size (ball query's); the radius usually decides
constexpr int kWalkGridMinPoints = 512;   // smaller clouds: all pairs (the build's fixed passes cost more)

__global__ __launch_bounds__(kWalkBlock) void clamp_lengths_kernel(const int64_t* __restrict__ lengths, int N, int P,
                                                                   int64_t* __restrict__ len) {
  const int n = blockIdx.x * kWalkBlock + threadIdx.x;
  if (n >= N) return;
  len[n] = clamped_length<int64_t>(lengths, n, P);
}

void clamp_lengths_async(const int64_t* lengths, int64_t N, int64_t P, int64_t* len, hipStream_t stream) {
  hipLaunchKernelGGL(clamp_lengths_kernel, dim3((unsigned)ceil_div(N, kWalkBlock)), dim3(kWalkBlock), 0, stream, lengths,
                     (int)N, (int)P, len);
}

static bool radius_walk_uses_grid(const char* knob, int64_t N, int64_t P) {
  const long force = debug_knob(knob, -1);
  if (force == 0 || N <= 0 || P <= 0 || P > knn_grid_max_points()) return false;
  return force == 1 || P >= kWalkGridMinPoints;
}

WalkLayout radius_walk_carve(Carver& c, const char* knob, int64_t N, int64_t P) {
  WalkLayout l;
  l.uses_grid = radius_walk_uses_grid(knob, N, P);
  l.len = (int64_t*)c.take(sizeof(int64_t) * (size_t)N);
  l.grid = c.take(l.uses_grid ? grid_carve(nullptr, nullptr, N, P, P, kWalkCellTarget) : 0);
  return l;
}

int radius_walk_prepare(const WalkLayout& l, const float* points, const int64_t* lengths, int64_t N, int64_t P, int64_t D,
                        float cell_radius, hipStream_t stream, WalkView* v) {
  clamp_lengths_async(lengths, N, P, l.len, stream);
  *v = WalkView{};
  v->points = points;
  v->len = l.len;
  v->P = (int)P;
  if (!l.uses_grid) return POINTOPS_OK;
  GridWs ws;
  grid_carve(&ws, l.grid, N, P, P, kWalkCellTarget);
  // K = 0: the build's padding of search rows has nothing to write
  const KnnArgs a = make_knn_args(points, points, l.len, l.len, N, P, P, D, 0, 0, nullptr, nullptr, stream);
  GridBuild b{};
  b.c_target = kWalkCellTarget;
  b.h_min = cell_radius * 1.001f;
  b.same = true;
  b.refine = -1;
  const int rc = grid_build(a, ws, b);
  v->clouds = ws.cloud;
  v->edges = ws.edges;
  v->cell_start = ws.cell_start;
  v->sorted = ws.sorted;
  v->cell_cap = ws.cell_cap;
  return rc;
}

}  // namespace pointops

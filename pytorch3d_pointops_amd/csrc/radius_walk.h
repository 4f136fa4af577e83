// radius_walk.h -- the certified radius walk of cluster.hip, iss.hip and filters.hip: one lane per point visits every
// point of its cloud with ball query's `dist2 < r2` (point_dist<D, 2> of grid.h, unfused fp32).
//
// A WALK is ball_grid_lane_kernel's: the nine x-runs of the 3x3x3 cube around the lane's cell, taken only under that
// kernel's certificate `whole || box_lower_bound<2>(...) >= r2` (every unvisited point has dist2 >= r2).  A lane without
// the certificate, and every lane of a cloud whose grid was refused (non-finite coordinates, cell caps) or that is too
// small for one, walks the raw cloud instead: all pairs, the same comparison, so which path a lane takes depends on
// the input alone and never changes a result.  The certificate is per lane and per r2: two walks with two radii over
// one grid (cells at least as wide as the larger radius) each take their own, from a view with their own r2.
//
// The host half (radius_walk.hip) is what an operator does before its own launches: radius_walk_carve takes the walk's
// part of the operator's workspace, radius_walk_prepare clamps the lengths, builds the grids and fills the view.  The
// device half: walk_item, walk_lane, then radius_walk_records -- the one loop -- or radius_walk, its index-only form.
#pragma once
#include "grid.h"

namespace pointops {

constexpr int kWalkBlock = 256;  // threads of a per-point launch: grid (ceil(P / kWalkBlock), N)

struct WalkView {
  const float* points;       // (N, P, D)
  const int64_t* len;        // (N,) clamped
  const GridCloud* clouds;   // grid state: null when the call builds no grid
  const float* edges;
  const int* cell_start;
  const float4* sorted;
  int cell_cap, P;
  float r2;                  // the caller's: an fp32 product, as ball query's radius2
};

// ---------------------------------------------------------------------------------------------------- host
// the walk's part of an operator's workspace
struct WalkLayout {
  int64_t* len;  // (N,)
  char* grid;    // grid_carve's
  bool uses_grid;
};

// Takes the walk's arrays from the operator's Carver (sizing only where the Carver's base is null).  Whether the call
// builds grids is decided here (the per-cloud decision is grid_build's, on the device): `knob` names the operator's
// debug knob (debug.h), 0 = never, 1 = whenever the shape allows (tests), else by cloud size.
WalkLayout radius_walk_carve(Carver& c, const char* knob, int64_t N, int64_t P);

// Launches the clamp of `lengths` into l.len and, where the call builds grids, grid_build over cells at least
// 1.001 cell_radius wide; fills every field of `v` but r2.  Returns grid_build's code.
int radius_walk_prepare(const WalkLayout& l, const float* points, const int64_t* lengths, int64_t N, int64_t P, int64_t D,
                        float cell_radius, hipStream_t stream, WalkView* v);

// ---------------------------------------------------------------------------------------------------- device
// (cloud, lane, length, grid state) of a thread of the per-point launches; g: the cloud's grid where it has one
struct WalkItem {
  int n, t, len;
  bool grid;
  GridCloud g;
};
__device__ __forceinline__ WalkItem walk_item(const WalkView& v) {
  WalkItem it;
  it.n = blockIdx.y;
  it.t = blockIdx.x * kWalkBlock + threadIdx.x;
  it.len = (int)v.len[it.n];
  it.grid = false;
  it.g = {};
  if (v.clouds != nullptr) {
    it.g = v.clouds[it.n];
    it.grid = it.g.use_grid != 0;
  }
  return it;
}

template <int D>
struct WalkLane {
  int i;            // the point's index in its cloud
  float x, y, z;
  bool cube;        // walk the 3x3x3 cube (certified); else the raw cloud
  int cy, cz, X0, X1;
};

// the item's lane: position t of the cell order where the cloud has a grid, point t where it has none (t < len)
template <int D>
__device__ __forceinline__ WalkLane<D> walk_lane(const WalkView& v, const WalkItem& it) {
  const GridCloud& g = it.g;
  const int n = it.n, t = it.t;
  WalkLane<D> L;
  L.cy = L.cz = L.X0 = L.X1 = 0;
  if (it.grid) {
    const float4 q = v.sorted[(int64_t)n * (v.P + kSortedPad) + t];
    L.x = q.x, L.y = q.y, L.z = q.z;
    L.i = __float_as_int(q.w);
    int cx;
    point_cells(g, L.x, L.y, L.z, cx, L.cy, L.cz);
    L.X0 = max(cx - 1, 0), L.X1 = min(cx + 1, g.G[0] - 1);
    const int Y0 = max(L.cy - 1, 0), Y1 = min(L.cy + 1, g.G[1] - 1);
    const int Z0 = max(L.cz - 1, 0), Z1 = min(L.cz + 1, g.G[2] - 1);
    bool whole;
    const float lb = box_lower_bound<2>(g, v.edges + (int64_t)n * 3 * kEdgeStride, L.x, L.y, L.z, L.X0, L.X1, Y0, Y1,
                                        Z0, Z1, whole);
    L.cube = whole || lb >= v.r2;  // every unvisited point has computed dist2 >= lb
  } else {
    load_point3<D>(v.points + ((int64_t)n * v.P + t) * D, L.x, L.y, L.z);
    L.i = t;
    L.cube = false;
  }
  return L;
}

// fn(j, c, k) for every neighbour j of the lane (dist2 < r2, the lane itself included), until fn returns false: c its
// coordinates, k its position in the cloud's cell order -- or -1 on the raw-cloud path, which has none
template <int D, typename Fn>
__device__ __forceinline__ void radius_walk_records(const WalkView& v, const WalkItem& it, const WalkLane<D>& L, Fn fn) {
  const GridCloud& g = it.g;
  const int n = it.n, len = it.len;
  if (L.cube) {
    const float4* __restrict__ sp = v.sorted + (int64_t)n * (v.P + kSortedPad);
    const int* __restrict__ cstart = v.cell_start + (int64_t)n * (v.cell_cap + 1);
    for (int dz = -1; dz <= 1; ++dz) {
      const int z = L.cz + dz;
      if (z < 0 || z >= g.G[2]) continue;
      for (int dy = -1; dy <= 1; ++dy) {
        const int y = L.cy + dy;
        if (y < 0 || y >= g.G[1]) continue;
        const int rowbase = (z * g.G[1] + y) * g.G[0];
        const int s = cstart[rowbase + L.X0], e = cstart[rowbase + L.X1 + 1];
        for (int k = s; k < e; ++k) {
          const float4 c = sp[k];
          if (point_dist<D, 2>(L.x, L.y, L.z, c) < v.r2) {
            if (!fn(__float_as_int(c.w), c, k)) return;
          }
        }
      }
    }
  } else {
    const float* __restrict__ pts = v.points + (int64_t)n * v.P * D;
    for (int j = 0; j < len; ++j) {
      float4 c;
      load_point3<D>(pts + (int64_t)j * D, c.x, c.y, c.z);
      if (point_dist<D, 2>(L.x, L.y, L.z, c) < v.r2) {
        if (!fn(j, c, -1)) return;
      }
    }
  }
}

// fn(j) for every neighbour j of the lane (dist2 < r2, the lane itself included), until fn returns false
template <int D, typename Fn>
__device__ __forceinline__ void radius_walk(const WalkView& v, const WalkItem& it, const WalkLane<D>& L, Fn fn) {
  radius_walk_records<D>(v, it, L, [&](int j, const float4&, int) { return fn(j); });
}

}  // namespace pointops

// radius_knn_kernel.h -- the search kernel of knn_in_radius (knn_in_radius.hip owns the operator: the C ABI entry, the
// workspace and the grid build) and the choice of its template instance.  One lane per query: a lane whose 3x3x3 cube is
// certified to contain its ball walks the nine x-runs of the cube, any other lane its raw cloud in index order; both keep
// the KC smallest keys of knn_radius_list.h in registers.  The instance dispatch lives here, beside the kernel, and not in
// a knn*.hip: the dispatch sites of those files are the matrix of knn_points and ball_query
// (tests/search_instance_cases.py), and this operator's instances are run at their bucket edges by its own cases
// (tests/knn_in_radius_cases.py).
#pragma once
#include "grid.h"
#include "knn_radius_list.h"

namespace pointops {

constexpr int kRadiusKnnBlock = 256;         // threads of the search launch: grid (ceil(P1 / 256), N)
constexpr int kRadiusKnnGroup = 4;           // records of a run in flight per lane (kSortedPad covers the overrun)
constexpr Ints<1, 4, 8, 16, 32, 64> kRadiusKnnKC{};
static_assert(kRadiusKnnGroup - 1 < kSortedPad, "a group may start at a run's last record");

struct RadiusKnnView {
  const float* p1;           // (N, P1, D)
  const float* p2;           // (N, P2, D)
  const int64_t* len1;       // (N,) clamped
  const int64_t* len2;
  const GridCloud* clouds;   // grid state: null when the call builds no grid
  const float* edges;
  const int* cell_start;
  const float4* sorted;
  const float4* qsorted;
  int cell_cap, P1, P2, K;
  float r2;                  // an fp32 product, as ball query's radius2
};

template <int D, int KC>
__global__ __launch_bounds__(kRadiusKnnBlock) void knn_in_radius_kernel(RadiusKnnView v, int64_t* __restrict__ idxs,
                                                                        float* __restrict__ dists,
                                                                        int32_t* __restrict__ counts) {
  const int n = blockIdx.y;
  const int t = blockIdx.x * kRadiusKnnBlock + threadIdx.x;
  if (t >= v.P1) return;
  const int len1 = (int)v.len1[n], len2 = (int)v.len2[n];
  if (t >= len1) {  // padding rows
    const int64_t row = (int64_t)n * v.P1 + t;
    for (int k = 0; k < v.K; ++k) {
      idxs[row * v.K + k] = -1;
      dists[row * v.K + k] = 0.0f;
    }
    if (counts != nullptr) counts[row] = 0;
    return;
  }
  GridCloud g = {};
  bool grid = false;
  if (v.clouds != nullptr) {
    g = v.clouds[n];
    grid = g.use_grid != 0;
  }
  // the lane's query: position t of the cell order where the cloud has a grid, row t where it has none
  float qx, qy, qz;
  int qi = t, cy = 0, cz = 0, X0 = 0, X1 = 0;
  bool cube = false;
  const float4* __restrict__ sp = v.sorted + (int64_t)n * (v.P2 + kSortedPad);
  if (grid) {
    const float4 q = (g.same ? sp : v.qsorted + (int64_t)n * v.P1)[t];
    qx = q.x, qy = q.y, qz = q.z;
    qi = __float_as_int(q.w);
    int cx;
    point_cells(g, qx, qy, qz, cx, cy, cz);
    X0 = max(cx - 1, 0), X1 = min(cx + 1, g.G[0] - 1);
    const int Y0 = max(cy - 1, 0), Y1 = min(cy + 1, g.G[1] - 1);
    const int Z0 = max(cz - 1, 0), Z1 = min(cz + 1, g.G[2] - 1);
    bool whole;
    const float lb = box_lower_bound<2>(g, v.edges + (int64_t)n * 3 * kEdgeStride, qx, qy, qz, X0, X1, Y0, Y1, Z0, Z1,
                                        whole);
    cube = whole || lb >= v.r2;  // every unvisited point has computed d2 >= lb
  } else {
    load_point3<D>(v.p1 + ((int64_t)n * v.P1 + t) * D, qx, qy, qz);
  }

  RadiusList<KC> list;
  list.clear();
  if (cube) {
    const int* __restrict__ cstart = v.cell_start + (int64_t)n * (v.cell_cap + 1);
    for (int dz = -1; dz <= 1; ++dz) {
      const int z = cz + dz;
      if (z < 0 || z >= g.G[2]) continue;
      for (int dy = -1; dy <= 1; ++dy) {
        const int y = cy + dy;
        if (y < 0 || y >= g.G[1]) continue;
        const int rowbase = (z * g.G[1] + y) * g.G[0];
        const int s = cstart[rowbase + X0], e = cstart[rowbase + X1 + 1];
        for (int k = s; k < e; k += kRadiusKnnGroup) {
          float4 c[kRadiusKnnGroup];  // (past e: records of the next run or of the pad, masked below)
#pragma unroll
          for (int u = 0; u < kRadiusKnnGroup; ++u) c[u] = sp[k + u];
#pragma unroll
          for (int u = 0; u < kRadiusKnnGroup; ++u) {
            const float d2 = point_dist<D, 2>(qx, qy, qz, c[u]);
            if (k + u < e && d2 < v.r2) list.insert(radius_list_key(d2, __float_as_uint(c[u].w)));
          }
        }
      }
    }
  } else {
    const float* __restrict__ pts = v.p2 + (int64_t)n * v.P2 * D;
    for (int j = 0; j < len2; ++j) {
      float4 c;
      load_point3<D>(pts + (int64_t)j * D, c.x, c.y, c.z);
      const float d2 = point_dist<D, 2>(qx, qy, qz, c);
      if (d2 < v.r2) list.insert(radius_list_key(d2, (uint32_t)j));
    }
  }

  const int64_t row = (int64_t)n * v.P1 + qi;
  int64_t* __restrict__ oi = idxs + row * v.K;
  float* __restrict__ od = dists + row * v.K;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    if (k < v.K) {
      const uint64_t key = list.top[k];
      const bool hit = key != kRadiusListEmpty;
      oi[k] = hit ? (int64_t)radius_list_index(key) : -1;
      od[k] = hit ? radius_list_d2(key) : 0.0f;
      cnt += hit ? 1 : 0;
    }
  }
  if (counts != nullptr) counts[row] = cnt;
}

// the launch of the instance for (D, K): D in 1..3 and 1 <= K <= 64, checked by the caller
inline void radius_knn_launch(const RadiusKnnView& v, int64_t N, hipStream_t stream, int D, int64_t* idxs, float* dists,
                              int32_t* counts) {
  const dim3 qgrid((unsigned)ceil_div(v.P1, kRadiusKnnBlock), (unsigned)N);
  with_exact<3>(Ints<1, 2, 3>{}, D, [&](auto DT) {
    with_bucket(kRadiusKnnKC, v.K, [&](auto KC) {
      hipLaunchKernelGGL((knn_in_radius_kernel<DT, KC>), qgrid, dim3(kRadiusKnnBlock), 0, stream, v, idxs, dists,
                         counts);
    });
  });
}

}  // namespace pointops

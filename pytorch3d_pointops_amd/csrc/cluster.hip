// cluster.hip -- DBSCAN / Euclidean clustering of a batch of clouds (C ABI: pointops_cluster_dbscan; device half of
// functions/cluster.py).  The definition is the comment block of the entry in include/pointops_amd.h: neighbours are
// the pairs with ball query's `dist2 < eps * eps` (point_dist<D, 2> of grid.h, unfused fp32), a core point has at least
// min_points of them (itself included), clusters are the connected components of the neighbour graph on the core
// points numbered by their smallest member, a border point takes the smallest label among its core neighbours.
//
// A fixed sequence of launches, stream-ordered, nothing read back; the kernel boundary is the only synchronisation:
//   prepare   radius_walk_prepare with cell_radius = eps: the lengths clamped into [0, P], and for clouds of 512 points
//             and more the cloud sorted by cells at least eps wide
//   count     one lane per point: neighbours counted up to min_points -> core_mask; parent[i] = i
//   union     core lanes walk again: uf_union(i, j) for every core neighbour j < i (cluster_union.h: lock-free,
//             relaxed agent-scope atomics only, the root of a component = its smallest index)
//   flatten   core: label = find(i); non-core: the smallest root among the core neighbours, or -1.  Its own launch:
//             the roots it reads are final only once every hook of the union launch has been made.
//   scan      one workgroup per cloud: the roots (label == own index) ranked in index order -> rank[], num_clusters
//   relabel   label = rank[root]
// A WALK is radius_walk.h's: the 3x3x3 cube around the lane's cell under ball query's certificate,
// else the raw cloud by all pairs with the same comparison, so which path a lane takes depends on the input alone and
// never changes a result.  POINTOPS_DEBUG=cluster_grid=0 sends every cloud by all pairs.
#include <limits.h>

#include "cluster_union.h"
#include "radius_walk.h"
#include "wave.h"

namespace pointops {

constexpr int kClScanBlock = 1024;

template <int D>
__global__ __launch_bounds__(kWalkBlock) void cluster_count_kernel(WalkView v, int min_points,
                                                                   uint8_t* __restrict__ core_mask,
                                                                   int* __restrict__ parent) {
  const WalkItem it = walk_item(v);
  if (it.t >= v.P) return;
  if (it.t >= it.len) {
    core_mask[(int64_t)it.n * v.P + it.t] = 0;  // padding rows
    return;
  }
  const WalkLane<D> L = walk_lane<D>(v, it);
  int cnt = 0;
  radius_walk<D>(v, it, L, [&](int) { return ++cnt < min_points; });
  core_mask[(int64_t)it.n * v.P + L.i] = cnt >= min_points ? 1 : 0;
  parent[(int64_t)it.n * v.P + L.i] = L.i;
}

template <int D>
__global__ __launch_bounds__(kWalkBlock) void cluster_union_kernel(WalkView v, const uint8_t* __restrict__ core_mask,
                                                                   int* parent) {
  const WalkItem it = walk_item(v);
  if (it.t >= it.len) return;
  const WalkLane<D> L = walk_lane<D>(v, it);
  const uint8_t* __restrict__ core = core_mask + (int64_t)it.n * v.P;
  if (!core[L.i]) return;
  int* const par = parent + (int64_t)it.n * v.P;
  int up = L.i;  // an ancestor-or-self of this point: the unions start from it, not from the point every time
  radius_walk<D>(v, it, L, [&](int j) {
    if (j < L.i && core[j]) up = uf_union(par, up, j);  // (every edge once: from its larger end)
    return true;
  });
}

template <int D>
__global__ __launch_bounds__(kWalkBlock) void cluster_flatten_kernel(WalkView v, const uint8_t* __restrict__ core_mask,
                                                                     int* parent, int64_t* __restrict__ labels) {
  const WalkItem it = walk_item(v);
  if (it.t >= v.P) return;
  if (it.t >= it.len) {
    labels[(int64_t)it.n * v.P + it.t] = -1;  // padding rows
    return;
  }
  const WalkLane<D> L = walk_lane<D>(v, it);
  const uint8_t* __restrict__ core = core_mask + (int64_t)it.n * v.P;
  int* const par = parent + (int64_t)it.n * v.P;
  int root;
  if (core[L.i]) {
    root = uf_find(par, L.i);
  } else {
    root = INT_MAX;  // the smallest root = the smallest label: clusters are numbered by their smallest member
    radius_walk<D>(v, it, L, [&](int j) {
      if (core[j]) root = min(root, uf_find(par, j));
      return true;
    });
    if (root == INT_MAX) root = -1;
  }
  labels[(int64_t)it.n * v.P + L.i] = root;
}

// One workgroup per cloud loops over tiles of the index space: rank[r] = roots below r, for every root r.
__global__ __launch_bounds__(kClScanBlock) void cluster_scan_kernel(const int64_t* __restrict__ len, int P,
                                                                  const int64_t* __restrict__ labels,
                                                                  int* __restrict__ rank,
                                                                  int64_t* __restrict__ num_clusters) {
  __shared__ int s_wsum[kClScanBlock / kWave];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int length = (int)len[n];
  int base = 0;
  for (int i0 = 0; i0 < length; i0 += kClScanBlock) {
    const int i = i0 + tid;
    const int flag = (i < length && labels[(int64_t)n * P + i] == (int64_t)i) ? 1 : 0;
    int total;
    const int excl = block_exclusive_sum<kClScanBlock / kWave>(flag, s_wsum, total);
    if (flag) rank[(int64_t)n * P + i] = base + excl;
    base += total;
    __syncthreads();  // (s_wsum free again)
  }
  if (tid == 0) num_clusters[n] = base;
}

__global__ __launch_bounds__(kWalkBlock) void cluster_relabel_kernel(const int64_t* __restrict__ len, int P,
                                                                     const int* __restrict__ rank, int64_t* labels) {
  const int n = blockIdx.y, i = blockIdx.x * kWalkBlock + threadIdx.x;
  if (i >= (int)len[n]) return;
  const int64_t root = labels[(int64_t)n * P + i];
  if (root >= 0) labels[(int64_t)n * P + i] = rank[(int64_t)n * P + root];
}

static bool cluster_shape_ok(int64_t N, int64_t P, int64_t D) {
  // (a cloud is a grid's y coordinate; point indices are ints)
  return N >= 0 && N < 65536 && P >= 0 && P < (1LL << 30) && D >= 1 && D <= 3;
}

struct ClusterLayout {
  WalkLayout walk;
  int* parent;   // (N, P)
  int* rank;     // (N, P)
  size_t bytes;
};

static ClusterLayout cluster_layout(void* ws, int64_t N, int64_t P) {
  Carver c(ws);
  ClusterLayout l;
  l.walk = radius_walk_carve(c, "cluster_grid", N, P);
  l.parent = (int*)c.take(sizeof(int) * (size_t)N * (size_t)P);
  l.rank = (int*)c.take(sizeof(int) * (size_t)N * (size_t)P);
  l.bytes = c.off;
  return l;
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_cluster_workspace_bytes(int64_t N, int64_t P) {
  if (!cluster_shape_ok(N, P, 3) || N == 0) return 0;
  return cluster_layout(nullptr, N, P).bytes;
}

extern "C" int pointops_cluster_dbscan(const float* points, const int64_t* lengths, int64_t N, int64_t P, int64_t D,
                                       float eps, int64_t min_points, int64_t* labels, int64_t* num_clusters,
                                       uint8_t* core_mask, void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(cluster_shape_ok(N, P, D), "cluster_dbscan: need 0 <= N < 65536, 0 <= P < 2^30 and 1 <= D <= 3");
  POINTOPS_REQUIRE(eps > 0.0f && eps <= FLT_MAX && min_points >= 1,
                   "cluster_dbscan: need a finite eps > 0 and min_points >= 1");
  if (N == 0) return POINTOPS_OK;
  const ClusterLayout l = cluster_layout(workspace, N, P);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "cluster_dbscan: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  WalkView v;
  const int rc = radius_walk_prepare(l.walk, points, lengths, N, P, D, eps, stream, &v);
  if (rc != POINTOPS_OK) return rc;
  v.r2 = eps * eps;  // fp32 product, as ball query's radius2
  const int minp = (int)(min_points > INT_MAX ? INT_MAX : min_points);
  if (P > 0) {
    const dim3 pgrid((unsigned)ceil_div(P, kWalkBlock), (unsigned)N);
    with_exact<3>(Ints<1, 2, 3>{}, (int)D, [&](auto DT) {
      hipLaunchKernelGGL((cluster_count_kernel<DT>), pgrid, dim3(kWalkBlock), 0, stream, v, minp, core_mask, l.parent);
      hipLaunchKernelGGL((cluster_union_kernel<DT>), pgrid, dim3(kWalkBlock), 0, stream, v, (const uint8_t*)core_mask,
                         l.parent);
      hipLaunchKernelGGL((cluster_flatten_kernel<DT>), pgrid, dim3(kWalkBlock), 0, stream, v, (const uint8_t*)core_mask,
                         l.parent, labels);
    });
  }
  hipLaunchKernelGGL(cluster_scan_kernel, dim3((unsigned)N), dim3(kClScanBlock), 0, stream, v.len, (int)P,
                     (const int64_t*)labels, l.rank, num_clusters);
  if (P > 0)
    hipLaunchKernelGGL(cluster_relabel_kernel, dim3((unsigned)ceil_div(P, kWalkBlock), (unsigned)N), dim3(kWalkBlock), 0,
                       stream, v.len, (int)P, (const int*)l.rank, labels);
  return check_launch("cluster_dbscan");
}

// filters.hip -- outlier removal of a batch of clouds (C ABI: pointops_radius_outlier, pointops_statistical_outlier,
// pointops_mask_compact; device half of functions/filters.py).  The definitions are the comment block of the entries in
// include/pointops_amd.h.  Three kernel groups, every launch stream-ordered, nothing read back, no atomics beyond
// grid_build's:
//   radius       radius_walk_prepare with cell_radius = radius (the lengths clamped, a grid for clouds of 512 points and
//                more), then one lane per point in cell order: radius_walk.h's walk counting the OTHER rows, stopping once
//                the count decides the mask unless the exact counts are asked for.  POINTOPS_DEBUG=filter_grid=0|1 forces
//                either path.
//   statistics   rows     one wave per 64 rows, staged through LDS, a lane per row: m_i (filter_stats.h) -> mean_distance
//                first    one workgroup per chunk of 4096 rows: the chunk's partial of S1 and of n_f
//                spread   the same geometry: every workgroup adds the chunk partials of its cloud in chunk order -> mean;
//                         the chunk's partial of S2
//                decide   one lane per row: std, threshold (every workgroup the same; the first writes stats and
//                         threshold), mask
//                The tree of the two sums is the header's: a lane per lane, an LDS fold, the chunks one after the other.
//   compaction   count    kept rows per block of 1024 rows -> the upper half of index[n, block]
//                scan     one workgroup per cloud: the counts scanned in place -> block offsets, num_kept
//                scatter  every block ranks its kept rows behind its offset: the LOWER halves of index
//                widen    every index sign-extended from its lower half: the offsets are gone
#include <limits.h>

#include "filter_stats.h"
#include "radius_walk.h"
#include "wave.h"

namespace pointops {

constexpr int kCompactBlock = 1024;
static_assert(kFilterLanes == kWalkBlock, "one workgroup of the per-point launches is one chunk's lanes");

// ---------------------------------------------------------------------------------------------------- compaction
// the upper half of index[n, b]: block b's count, then its offset (little-endian: the halves of an int64)
__device__ __forceinline__ int* compact_slot(int64_t* index, int64_t P, int n, int b) {
  return (int*)(index + (int64_t)n * P + b) + 1;
}

__device__ __forceinline__ int compact_flag(const uint8_t* __restrict__ mask, int64_t P, int n, int64_t i) {
  return i < P && mask[(int64_t)n * P + i] != 0 ? 1 : 0;
}

__global__ __launch_bounds__(kCompactBlock) void compact_count_kernel(const uint8_t* __restrict__ mask, int64_t P,
                                                                    int64_t* index) {
  const int n = blockIdx.y, b = blockIdx.x;
  const int total = __syncthreads_count(compact_flag(mask, P, n, (int64_t)b * kCompactBlock + threadIdx.x));
  if (threadIdx.x == 0) *compact_slot(index, P, n, b) = total;
}

// One workgroup per cloud loops over tiles of the block counts: exclusive offsets in place.
__global__ __launch_bounds__(kCompactBlock) void compact_scan_kernel(int64_t P, int blocks, int64_t* index,
                                                                   int64_t* __restrict__ num_kept) {
  __shared__ int s_wsum[kCompactBlock / kWave];
  const int n = blockIdx.x, tid = threadIdx.x;
  int base = 0;
  for (int b0 = 0; b0 < blocks; b0 += kCompactBlock) {
    const int b = b0 + tid;
    const int v = b < blocks ? *compact_slot(index, P, n, b) : 0;
    int total;
    const int excl = block_exclusive_sum<kCompactBlock / kWave>(v, s_wsum, total);
    if (b < blocks) *compact_slot(index, P, n, b) = base + excl;
    base += total;
    __syncthreads();  // (s_wsum free again)
  }
  if (tid == 0) num_kept[n] = base;
}

// Writes lower halves only: no block's offset (an upper half) is touched while another block may still read it.
__global__ __launch_bounds__(kCompactBlock) void compact_scatter_kernel(const uint8_t* __restrict__ mask, int64_t P,
                                                                      int64_t* index,
                                                                      const int64_t* __restrict__ num_kept) {
  __shared__ int s_wsum[kCompactBlock / kWave];
  const int n = blockIdx.y, b = blockIdx.x;
  const int64_t i = (int64_t)b * kCompactBlock + threadIdx.x;
  const int flag = compact_flag(mask, P, n, i);
  int total;
  const int excl = block_exclusive_sum<kCompactBlock / kWave>(flag, s_wsum, total);
  int* const row = (int*)(index + (int64_t)n * P);
  if (flag) row[2 * (int64_t)(*compact_slot(index, P, n, b) + excl)] = (int)i;  // (position <= i < P)
  if (i < P && i >= num_kept[n]) row[2 * i] = -1;
}

__global__ __launch_bounds__(kWalkBlock) void compact_widen_kernel(int64_t P, int64_t* index) {
  const int64_t i = (int64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  if (i >= P) return;
  int64_t* const e = index + (int64_t)blockIdx.y * P + i;
  *e = (int64_t)*(const int*)e;
}

static bool compact_shape_ok(int64_t N, int64_t P) { return N >= 0 && N < 65536 && P >= 0 && P < (1LL << 30); }

// the compaction of mask (N > 0), behind whatever wrote it on `stream`
static void compact_launch(const uint8_t* mask, int64_t N, int64_t P, int64_t* index, int64_t* num_kept,
                           hipStream_t stream) {
  const int blocks = (int)ceil_div(P, kCompactBlock);
  const dim3 bgrid((unsigned)blocks, (unsigned)N);
  if (P > 0)
    hipLaunchKernelGGL(compact_count_kernel, bgrid, dim3(kCompactBlock), 0, stream, mask, P, index);
  hipLaunchKernelGGL(compact_scan_kernel, dim3((unsigned)N), dim3(kCompactBlock), 0, stream, P, blocks, index, num_kept);
  if (P > 0) {
    hipLaunchKernelGGL(compact_scatter_kernel, bgrid, dim3(kCompactBlock), 0, stream, mask, P, index,
                       (const int64_t*)num_kept);
    hipLaunchKernelGGL(compact_widen_kernel, dim3((unsigned)ceil_div(P, kWalkBlock), (unsigned)N), dim3(kWalkBlock), 0,
                       stream, P, index);
  }
}

// ---------------------------------------------------------------------------------------------------- radius
template <int D>
__global__ __launch_bounds__(kWalkBlock) void filter_radius_kernel(WalkView v, int min_neighbors,
                                                                   uint8_t* __restrict__ mask,
                                                                   int32_t* __restrict__ counts) {
  const WalkItem it = walk_item(v);
  if (it.t >= v.P) return;
  const int64_t base = (int64_t)it.n * v.P;
  if (it.t >= it.len) {  // padding rows
    mask[base + it.t] = 0;
    if (counts != nullptr) counts[base + it.t] = 0;
    return;
  }
  const WalkLane<D> L = walk_lane<D>(v, it);
  const bool exact = counts != nullptr;
  int cnt = 0;
  if (exact || min_neighbors > 0)  // (min_neighbors == 0 is decided before the first step)
    radius_walk<D>(v, it, L, [&](int j) {
      if (j != L.i) ++cnt;
      return exact || cnt < min_neighbors;
    });
  mask[base + L.i] = cnt >= min_neighbors ? 1 : 0;
  if (exact) counts[base + L.i] = cnt;
}

struct RadiusLayout {
  WalkLayout walk;
  size_t bytes;
};

static RadiusLayout radius_layout(void* ws, int64_t N, int64_t P) {
  Carver c(ws);
  RadiusLayout l;
  l.walk = radius_walk_carve(c, "filter_grid", N, P);
  l.bytes = c.off;
  return l;
}

// ---------------------------------------------------------------------------------------------------- statistics
// the fold of the header's tree: s[0] = the chunk's sum, read by thread 0 after the last barrier
__device__ __forceinline__ double filter_fold(double a, double* s) {
  const int t = threadIdx.x;
  s[t] = a;
  __syncthreads();
  for (int h = kFilterLanes / 2; h > 0; h >>= 1) {
    if (t < h) s[t] = s[t] + s[t + h];
    __syncthreads();
  }
  return s[0];
}

struct StatView {
  const float* dists;      // (N, P, K1)
  const int64_t* lengths;  // (N,) or null
  int P, K1, chunks;
  double* part1;           // (N, chunks) partials of S1
  double* part2;           // (N, chunks) partials of S2
  int* partn;              // (N, chunks) partials of n_f
};

// One wave per tile of 64 rows, a lane per row.  The tile's part of the table is one contiguous run of 64 K1 floats: it
// is read with coalesced loads into LDS (row stride K1 | 1 words: odd, so the lanes' rows start in different banks),
// then every lane adds up its own row (0 on padding rows, which are not loaded).
constexpr int kFilterRowTile = kWave;
static size_t filter_rows_lds(int64_t K1) { return sizeof(float) * kFilterRowTile * (size_t)(K1 | 1); }

__global__ __launch_bounds__(kFilterRowTile) void filter_rows_kernel(StatView v, float* __restrict__ mean_distance) {
  extern __shared__ float s_tile[];
  const int n = blockIdx.y, t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kFilterRowTile;
  const int len = clamped_length(v.lengths, n, v.P);
  const int cnt = v.K1 < len ? v.K1 : len;
  const int stride = v.K1 | 1;
  const int64_t below = len - i0;  // rows of the tile below the length
  const int live = below < 0 ? 0 : (below > kFilterRowTile ? kFilterRowTile : (int)below);
  const float* __restrict__ src = v.dists + ((int64_t)n * v.P + i0) * v.K1;
  for (int e = t; e < live * v.K1; e += kFilterRowTile) s_tile[(e / v.K1) * stride + e % v.K1] = src[e];
  __syncthreads();
  const int64_t i = i0 + t;
  if (i >= v.P) return;
  mean_distance[(int64_t)n * v.P + i] = t < live ? filter_row_mean(s_tile + t * stride, cnt) : 0.0f;
}

__global__ __launch_bounds__(kFilterLanes) void filter_first_kernel(StatView v,
                                                                  const float* __restrict__ mean_distance) {
  __shared__ double s_sum[kFilterLanes];
  __shared__ int s_nf[kFilterLanes / kWave];
  const int n = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
  const int len = clamped_length(v.lengths, n, v.P);
  double a = 0.0;
  int nf = 0;
  for (int j = 0; j < kFilterRowsPerLane; ++j) {
    const int64_t i = (int64_t)c * kFilterChunk + t + (int64_t)j * kFilterLanes;
    double term = 0.0;
    if (i < len) {
      const float m = mean_distance[(int64_t)n * v.P + i];
      if (filter_finite(m)) term = (double)m, ++nf;
    }
    a = a + term;
  }
  const double sum = filter_fold(a, s_sum);
  nf = wave_sum(nf);  // integers: any order
  if ((t & (kWave - 1)) == 0) s_nf[t / kWave] = nf;
  __syncthreads();
  if (t == 0) {
    int total = 0;
    for (int w = 0; w < kFilterLanes / kWave; ++w) total += s_nf[w];
    v.part1[(int64_t)n * v.chunks + c] = sum;
    v.partn[(int64_t)n * v.chunks + c] = total;
  }
}

// (S1, n_f) of cloud n: the chunk partials one after the other (every caller the same additions)
__device__ __forceinline__ void filter_first_pass(const StatView& v, int n, double& S1, int64_t& nf) {
  S1 = 0.0, nf = 0;
  for (int c = 0; c < v.chunks; ++c) {
    S1 = S1 + v.part1[(int64_t)n * v.chunks + c];
    nf += v.partn[(int64_t)n * v.chunks + c];
  }
}

__global__ __launch_bounds__(kFilterLanes) void filter_spread_kernel(StatView v,
                                                                   const float* __restrict__ mean_distance) {
  __shared__ double s_sum[kFilterLanes];
  __shared__ double s_mean;
  const int n = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
  const int len = clamped_length(v.lengths, n, v.P);
  if (t == 0) {
    double S1;
    int64_t nf;
    filter_first_pass(v, n, S1, nf);
    s_mean = filter_mean(S1, nf);
  }
  __syncthreads();
  const double mean = s_mean;
  double a = 0.0;
  for (int j = 0; j < kFilterRowsPerLane; ++j) {
    const int64_t i = (int64_t)c * kFilterChunk + t + (int64_t)j * kFilterLanes;
    double term = 0.0;
    if (i < len) {
      const float m = mean_distance[(int64_t)n * v.P + i];
      if (filter_finite(m)) term = filter_deviation2(m, mean);
    }
    a = a + term;
  }
  const double sum = filter_fold(a, s_sum);
  if (t == 0) v.part2[(int64_t)n * v.chunks + c] = sum;
}

__global__ __launch_bounds__(kWalkBlock) void filter_decide_kernel(StatView v, float std_ratio,
                                                                   const float* __restrict__ mean_distance,
                                                                   double* __restrict__ stats,
                                                                   float* __restrict__ threshold,
                                                                   uint8_t* __restrict__ mask) {
  __shared__ float s_thr;
  const int n = blockIdx.y, t = threadIdx.x;
  const int len = clamped_length(v.lengths, n, v.P);
  if (t == 0) {
    double S1, S2 = 0.0;
    int64_t nf;
    filter_first_pass(v, n, S1, nf);
    for (int c = 0; c < v.chunks; ++c) S2 = S2 + v.part2[(int64_t)n * v.chunks + c];
    const double mean = filter_mean(S1, nf), std = filter_std(S2, nf);
    s_thr = filter_threshold(mean, std, std_ratio);
    if (blockIdx.x == 0) {
      stats[(int64_t)n * 3 + 0] = mean;
      stats[(int64_t)n * 3 + 1] = std;
      stats[(int64_t)n * 3 + 2] = (double)nf;
      threshold[n] = s_thr;
    }
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kWalkBlock + t;
  if (i >= v.P) return;
  mask[(int64_t)n * v.P + i] = i < len && filter_keep(mean_distance[(int64_t)n * v.P + i], s_thr) ? 1 : 0;
}

static bool stat_shape_ok(int64_t N, int64_t P, int64_t K1) {
  return N >= 0 && N < 65536 && P >= 0 && P <= kFilterMaxPoints && K1 >= 2 && K1 <= kFilterMaxK1;
}

// (an empty cloud still has one chunk: its launches write the statistics of no rows)
static int stat_chunks(int64_t P) { return P > 0 ? (int)ceil_div(P, kFilterChunk) : 1; }

struct StatLayout {
  double* part1;
  double* part2;
  int* partn;
  size_t bytes;
};

static StatLayout stat_layout(void* ws, int64_t N, int64_t P) {
  Carver c(ws);
  StatLayout l;
  const size_t parts = (size_t)N * (size_t)stat_chunks(P);
  l.part1 = (double*)c.take(sizeof(double) * parts);
  l.part2 = (double*)c.take(sizeof(double) * parts);
  l.partn = (int*)c.take(sizeof(int) * parts);
  l.bytes = c.off;
  return l;
}

}  // namespace pointops

using namespace pointops;

extern "C" int pointops_mask_compact(const uint8_t* mask, int64_t N, int64_t P, int64_t* index, int64_t* num_kept,
                                     void* stream) {
  POINTOPS_REQUIRE(compact_shape_ok(N, P), "mask_compact: need 0 <= N < 65536 and 0 <= P < 2^30");
  if (N == 0) return POINTOPS_OK;
  compact_launch(mask, N, P, index, num_kept, (hipStream_t)stream);
  return check_launch("mask_compact");
}

extern "C" size_t pointops_radius_outlier_workspace_bytes(int64_t N, int64_t P) {
  if (!compact_shape_ok(N, P) || N == 0) return 0;
  return radius_layout(nullptr, N, P).bytes;
}

extern "C" int pointops_radius_outlier(const float* points, const int64_t* lengths, int64_t N, int64_t P, int64_t D,
                                       float radius, int64_t min_neighbors, uint8_t* mask, int32_t* counts,
                                       int64_t* index, int64_t* num_kept, void* workspace, size_t workspace_bytes,
                                       void* stream_) {
  POINTOPS_REQUIRE(compact_shape_ok(N, P) && D >= 1 && D <= 3,
                   "radius_outlier: need 0 <= N < 65536, 0 <= P < 2^30 and 1 <= D <= 3");
  POINTOPS_REQUIRE(radius > 0.0f && radius <= FLT_MAX && min_neighbors >= 0,
                   "radius_outlier: need a finite radius > 0 and min_neighbors >= 0");
  if (N == 0) return POINTOPS_OK;
  const RadiusLayout l = radius_layout(workspace, N, P);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "radius_outlier: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  WalkView v;
  const int rc = radius_walk_prepare(l.walk, points, lengths, N, P, D, radius, stream, &v);
  if (rc != POINTOPS_OK) return rc;
  if (P > 0) {
    v.r2 = radius * radius;  // fp32 product, as ball query's radius2
    const int minn = (int)(min_neighbors > INT_MAX ? INT_MAX : min_neighbors);
    const dim3 pgrid((unsigned)ceil_div(P, kWalkBlock), (unsigned)N);
    with_exact<3>(Ints<1, 2, 3>{}, (int)D, [&](auto DT) {
      hipLaunchKernelGGL((filter_radius_kernel<DT>), pgrid, dim3(kWalkBlock), 0, stream, v, minn, mask, counts);
    });
  }
  compact_launch(mask, N, P, index, num_kept, stream);
  return check_launch("radius_outlier");
}

extern "C" size_t pointops_statistical_outlier_workspace_bytes(int64_t N, int64_t P) {
  if (!stat_shape_ok(N, P, 2) || N == 0) return 0;
  return stat_layout(nullptr, N, P).bytes;
}

extern "C" int pointops_statistical_outlier(const float* dists, const int64_t* lengths, int64_t N, int64_t P,
                                            int64_t K1, float std_ratio, float* mean_distance, double* stats,
                                            float* threshold, uint8_t* mask, int64_t* index, int64_t* num_kept,
                                            void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(stat_shape_ok(N, P, K1), "statistical_outlier: need 0 <= N < 65536, 0 <= P <= 2^24 and 2 <= K1 <= 128");
  POINTOPS_REQUIRE(std_ratio >= 0.0f && std_ratio <= FLT_MAX, "statistical_outlier: need a finite std_ratio >= 0");
  if (N == 0) return POINTOPS_OK;
  const StatLayout l = stat_layout(workspace, N, P);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "statistical_outlier: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  StatView v{};
  v.dists = dists;
  v.lengths = lengths;
  v.P = (int)P;
  v.K1 = (int)K1;
  v.chunks = stat_chunks(P);
  v.part1 = l.part1;
  v.part2 = l.part2;
  v.partn = l.partn;
  const dim3 cgrid((unsigned)v.chunks, (unsigned)N);
  const dim3 pgrid((unsigned)(P > 0 ? ceil_div(P, kWalkBlock) : 1), (unsigned)N);
  if (P > 0)
    hipLaunchKernelGGL(filter_rows_kernel, dim3((unsigned)ceil_div(P, kFilterRowTile), (unsigned)N),
                       dim3(kFilterRowTile), filter_rows_lds(K1), stream, v, mean_distance);
  hipLaunchKernelGGL(filter_first_kernel, cgrid, dim3(kFilterLanes), 0, stream, v, (const float*)mean_distance);
  hipLaunchKernelGGL(filter_spread_kernel, cgrid, dim3(kFilterLanes), 0, stream, v, (const float*)mean_distance);
  hipLaunchKernelGGL(filter_decide_kernel, pgrid, dim3(kWalkBlock), 0, stream, v, std_ratio,
                     (const float*)mean_distance, stats, threshold, mask);
  compact_launch(mask, N, P, index, num_kept, stream);
  return check_launch("statistical_outlier");
}

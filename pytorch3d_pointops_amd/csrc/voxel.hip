// voxel.hip -- voxel-grid pooling of a batch of clouds (C ABI: pointops_voxel_downsample; device half of
// functions/voxel.py).  The definition is the comment block of the entry in include/pointops_amd.h: a cloud's voxels are
// its distinct cells floor((x - o) / v), numbered in ascending (c_z, c_y, c_x) order, and every voxel carries the mean of
// its members' points and features, summed in fp64 in an order that the sorted position alone fixes.
//
// A fixed sequence of launches, stream-ordered, nothing read back, no atomics on floating-point data:
//   lengths   the cloud lengths clamped into [0, P] (common.h's clamp_lengths_async)
//   bounds    fp32 min / max over the live rows, one slot per workgroup of 2048 rows (grid_build's bounding-box scheme:
//             no atomics, nothing to initialise; here non-finite rows are left out)
//   frame     one wave per cloud reduces the slots; voxel_key.h's voxel_frame decides origin, c_lo and status
//   keys      one lane per row: a record (key, cloud, row); rows of no voxel get the all-ones key
//   sort      rocPRIM's stable radix sort of the records by (cloud, key): equal keys keep ascending row index.  ONE
//             global sort over the N P records (the segmented sort reads a count back and gives a long segment a
//             single workgroup); a cloud's records end up in positions [n P, (n + 1) P)
//   scan      rocPRIM's exclusive scan of the head flags (a record whose key differs from its predecessor's), in uint32:
//             a voxel's number is a difference of two scan values of its cloud, which wrap-around leaves exact
//   finish    one lane per position: inverse through the row index, the compact row list, and per head the voxel's
//             first position, first_index and coords; the last live position writes num_voxels
//   reduce    one lane per voxel row: counts, the fill values of the rows >= V, and the means of the voxels of up to
//             kVoxelGroup members; then one wave per longer voxel.  Both evaluate the SAME expression (voxel_sum below),
//             so POINTOPS_DEBUG=voxel_long=0|1, which sends every voxel down one path, changes no byte.
#include <float.h>
#include <limits.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "debug.h"
#include "voxel_key.h"
#include "wave.h"

namespace pointops {

constexpr int kVoxelBlock = 256;
constexpr int kVoxelBoundsPerThread = 8;
constexpr int kVoxelBoundsTile = kVoxelBlock * kVoxelBoundsPerThread;  // rows per slot
constexpr int64_t kVoxelMaxPoints = (int64_t)1 << 24;
constexpr int64_t kVoxelMaxChannels = 1024;
// The shape of a voxel's sum (voxel_sum_lane and voxel_sum_wave evaluate it term for term):
//   a GROUP is 16 consecutive members, added one after the other to +0.0;
//   a CHUNK is 64 consecutive groups, combined by the aligned pairwise tree (groups 2k and 2k + 1, then pairs of pairs, ...;
//   a missing group counts +0.0, which changes nothing: no group sum is -0.0);
//   the chunks are added one after the other to +0.0.
constexpr int kVoxelGroup = 16;
constexpr int kVoxelChunkGroups = kWave;
constexpr int kVoxelChunk = kVoxelGroup * kVoxelChunkGroups;
constexpr int kVoxelLevels = 7;  // levels of the tree over 64 groups, the root included

struct VoxelRec {
  uint64_t key;
  uint32_t cloud, row;
};
static_assert(sizeof(VoxelRec) == 16, "VoxelRec");

struct VoxelRecOrder {  // (cloud, key), the cloud most significant; the row is payload
  __host__ __device__ rocprim::tuple<uint32_t&, uint64_t&> operator()(VoxelRec& r) const {
    return rocprim::tuple<uint32_t&, uint64_t&>(r.cloud, r.key);
  }
};

// a record opens a voxel: it is live and its predecessor is of another cloud or of another cell
struct VoxelHeadFlag {
  const VoxelRec* recs;
  __host__ __device__ uint32_t operator()(size_t pos) const {
    const VoxelRec r = recs[pos];
    if (r.key == kVoxelDeadKey) return 0u;
    if (pos == 0) return 1u;
    const VoxelRec q = recs[pos - 1];
    return (q.cloud != r.cloud || q.key != r.key) ? 1u : 0u;
  }
};
using VoxelFlagIterator = rocprim::transform_iterator<rocprim::counting_iterator<size_t>, VoxelHeadFlag, uint32_t>;

__device__ __forceinline__ bool voxel_row_live(const float* __restrict__ p, int i, int len) {
  // (x - x is 0 for a finite x and NaN otherwise)
  return i < len && p[0] - p[0] == 0.0f && p[1] - p[1] == 0.0f && p[2] - p[2] == 0.0f;
}

__global__ __launch_bounds__(kVoxelBlock) void voxel_bounds_kernel(const float* __restrict__ points,
                                                                  const int64_t* __restrict__ len, int P,
                                                                  float* __restrict__ slots) {
  const int n = blockIdx.y;
  const int L = (int)len[n];
  const int j0 = blockIdx.x * kVoxelBoundsTile;
  float mn[3], mx[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    mn[d] = __builtin_inff();
    mx[d] = -__builtin_inff();
  }
  const float* __restrict__ base = points + (int64_t)n * P * 3;
  for (int r = 0; r < kVoxelBoundsPerThread; ++r) {
    const int j = j0 + r * kVoxelBlock + (int)threadIdx.x;
    if (j < L) {
      const float* __restrict__ p = base + (int64_t)j * 3;
      if (voxel_row_live(p, j, L)) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          mn[d] = fminf(mn[d], p[d]);
          mx[d] = fmaxf(mx[d], p[d]);
        }
      }
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    mn[d] = wave_min(mn[d]);
    mx[d] = wave_max(mx[d]);
  }
  __shared__ float s_mn[kVoxelBlock / kWave][3], s_mx[kVoxelBlock / kWave][3];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      s_mn[wave][d] = mn[d];
      s_mx[wave][d] = mx[d];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    float a = s_mn[0][d], b = s_mx[0][d];
#pragma unroll
    for (int w = 1; w < kVoxelBlock / kWave; ++w) {
      a = fminf(a, s_mn[w][d]);
      b = fmaxf(b, s_mx[w][d]);
    }
    float* __restrict__ slot = slots + ((int64_t)n * gridDim.x + blockIdx.x) * 6;
    slot[d] = a;  // (+inf / -inf when the tile has no live row)
    slot[3 + d] = b;
  }
}

// one wave per cloud
__global__ __launch_bounds__(kWave) void voxel_frame_kernel(const float* __restrict__ slots, int nslots,
                                                           const float* __restrict__ origin, int origin_per_cloud,
                                                           float v, VoxelFrame* __restrict__ frames,
                                                           int32_t* __restrict__ status) {
  const int n = blockIdx.x;
  float mn[3], mx[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    mn[d] = __builtin_inff();
    mx[d] = -__builtin_inff();
  }
  const float* __restrict__ base = slots + (int64_t)n * nslots * 6;
  for (int s = threadIdx.x; s < nslots; s += kWave) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      mn[d] = fminf(mn[d], base[(int64_t)s * 6 + d]);
      mx[d] = fmaxf(mx[d], base[(int64_t)s * 6 + 3 + d]);
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    mn[d] = wave_min(mn[d]);
    mx[d] = wave_max(mx[d]);
  }
  if (threadIdx.x == 0) {
    const bool live = mn[0] <= mx[0];  // (a live row sets all three axes)
    const float* o = origin == nullptr ? nullptr : origin + (origin_per_cloud ? (int64_t)n * 3 : 0);
    const VoxelFrame f = voxel_frame(mn, mx, live, o, v);
    frames[n] = f;
    status[n] = f.status;
  }
}

__global__ __launch_bounds__(kVoxelBlock) void voxel_keys_kernel(const float* __restrict__ points,
                                                                const int64_t* __restrict__ len, int P, float v,
                                                                const VoxelFrame* __restrict__ frames,
                                                                VoxelRec* __restrict__ recs) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * kVoxelBlock + (int)threadIdx.x;
  if (i >= P) return;
  const float* __restrict__ p = points + ((int64_t)n * P + i) * 3;
  VoxelRec r;
  r.cloud = (uint32_t)n;
  r.row = (uint32_t)i;
  r.key = kVoxelDeadKey;
  if (voxel_row_live(p, i, (int)len[n])) r.key = voxel_key(frames[n], p[0], p[1], p[2], v);
  recs[(int64_t)n * P + i] = r;
}

// P == 0: nothing but the two per-cloud outputs
__global__ __launch_bounds__(kVoxelBlock) void voxel_empty_kernel(int N, int64_t* __restrict__ num_voxels,
                                                                 int32_t* __restrict__ status) {
  const int n = blockIdx.x * kVoxelBlock + (int)threadIdx.x;
  if (n >= N) return;
  num_voxels[n] = 0;
  status[n] = 0;
}

struct VoxelSorted {
  const VoxelRec* recs;  // (N, P) sorted by (cloud, key), stable
  const uint32_t* scan;  // (N, P) exclusive scan of the head flags over the whole batch, modulo 2^32
  uint32_t* rows;        // (N, P) the row of every position
  int32_t* vox;          // (N, P) the voxel of every position, -1 on rows of no voxel
  int32_t* start;        // (N, P + 1) first position of every voxel; [V] = the number of live rows
};

__global__ __launch_bounds__(kVoxelBlock) void voxel_finish_kernel(VoxelSorted s, int P,
                                                                  const VoxelFrame* __restrict__ frames,
                                                                  int64_t* __restrict__ num_voxels,
                                                                  int64_t* __restrict__ inverse,
                                                                  int64_t* __restrict__ first_index,
                                                                  int64_t* __restrict__ coords) {
  const int n = blockIdx.y;
  const int t = blockIdx.x * kVoxelBlock + (int)threadIdx.x;
  if (t >= P) return;
  const int64_t base = (int64_t)n * P, pos = base + t;
  const VoxelRec r = s.recs[pos];
  const bool live = r.key != kVoxelDeadKey;
  s.rows[pos] = r.row;
  if (!live) {
    s.vox[pos] = -1;
    if (r.row < (uint32_t)P) inverse[base + r.row] = -1;
    if (t == 0) num_voxels[n] = 0;  // (dead keys sort last: the cloud has no live row)
    return;
  }
  const bool head = t == 0 || s.recs[pos - 1].key != r.key;
  const int id = (int)(s.scan[pos] - s.scan[base]) + (head ? 1 : 0) - 1;  // heads of the cloud up to here, minus one
  if ((unsigned)id >= (unsigned)P || r.row >= (uint32_t)P) {  // (cannot happen: no write is aimed by an unchecked index)
    s.vox[pos] = -1;
    return;
  }
  s.vox[pos] = id;
  inverse[base + r.row] = id;
  int32_t* const start = s.start + (int64_t)n * (P + 1);
  if (head) {
    start[id] = t;
    first_index[base + id] = r.row;  // (stable sort: the first member has the lowest row)
    if (coords != nullptr) {
      uint64_t d[3];
      voxel_unpack(r.key, d);
      const VoxelFrame f = frames[n];
      int64_t* const c = coords + (base + id) * 3;
#pragma unroll
      for (int a = 0; a < 3; ++a) c[a] = voxel_coord(f, d[a], a);
    }
  }
  if (t == P - 1 || s.recs[pos + 1].key == kVoxelDeadKey) {  // the last live position
    start[id + 1] = t + 1;
    num_voxels[n] = id + 1;
  }
}

// Level by level: the running sum of group g climbs while bit `lvl` of g is set, and rests at the first clear bit.
// Every index into st is a compile-time constant after unrolling.
template <int CH>
__device__ __forceinline__ void voxel_tree_push(double (&st)[kVoxelLevels][CH], double (&s)[CH], int g) {
  bool go = true;
#pragma unroll
  for (int lvl = 0; lvl < kVoxelLevels; ++lvl) {
    if (go) {
      if ((g >> lvl) & 1) {
#pragma unroll
        for (int k = 0; k < CH; ++k) s[k] = st[lvl][k] + s[k];
      } else {
#pragma unroll
        for (int k = 0; k < CH; ++k) st[lvl][k] = s[k];
        go = false;
      }
    }
  }
}

// the tree over the first `groups` groups of a chunk (1 <= groups <= 64): the resting sums, lowest level first
template <int CH>
__device__ __forceinline__ void voxel_tree_fold(const double (&st)[kVoxelLevels][CH], int groups, double (&acc)[CH]) {
  bool have = false;
#pragma unroll
  for (int lvl = 0; lvl < kVoxelLevels; ++lvl) {
    if ((groups >> lvl) & 1) {
#pragma unroll
      for (int k = 0; k < CH; ++k) acc[k] = have ? st[lvl][k] + acc[k] : st[lvl][k];
      have = true;
    }
  }
}

// members [j0, j1) of a voxel, channels [0, CH) of src (row stride `stride`), one after the other onto +0.0
template <int CH>
__device__ __forceinline__ void voxel_group_sum(const float* __restrict__ src, int stride,
                                                const uint32_t* __restrict__ rows, int j0, int j1, double (&s)[CH]) {
#pragma unroll
  for (int k = 0; k < CH; ++k) s[k] = 0.0;
  for (int j = j0; j < j1; ++j) {
    const float* __restrict__ x = src + (int64_t)rows[j] * stride;
#pragma unroll
    for (int k = 0; k < CH; ++k) s[k] += (double)x[k];
  }
}

// one lane, the whole voxel of c members
template <int CH>
__device__ void voxel_sum_lane(const float* __restrict__ src, int stride, const uint32_t* __restrict__ rows, int c,
                               double (&tot)[CH]) {
#pragma unroll
  for (int k = 0; k < CH; ++k) tot[k] = 0.0;
  for (int c0 = 0; c0 < c; c0 += kVoxelChunk) {
    const int left = c - c0;
    const int groups = left >= kVoxelChunk ? kVoxelChunkGroups : (left + kVoxelGroup - 1) / kVoxelGroup;
    double st[kVoxelLevels][CH], s[CH], acc[CH];
#pragma unroll
    for (int lvl = 0; lvl < kVoxelLevels; ++lvl)
#pragma unroll
      for (int k = 0; k < CH; ++k) st[lvl][k] = 0.0;
    for (int g = 0; g < groups; ++g) {
      const int j0 = c0 + g * kVoxelGroup;
      voxel_group_sum<CH>(src, stride, rows, j0, j0 + kVoxelGroup < c ? j0 + kVoxelGroup : c, s);
      voxel_tree_push<CH>(st, s, g);
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) acc[k] = 0.0;
    voxel_tree_fold<CH>(st, groups, acc);
#pragma unroll
    for (int k = 0; k < CH; ++k) tot[k] += acc[k];
  }
}

// one wave, the whole voxel: a lane per group of the chunk, the tree as a butterfly with offsets 1, 2, ..., 32; every
// lane ends with the sums
template <int CH>
__device__ void voxel_sum_wave(const float* __restrict__ src, int stride, const uint32_t* __restrict__ rows, int c,
                               double (&tot)[CH]) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int k = 0; k < CH; ++k) tot[k] = 0.0;
  for (int c0 = 0; c0 < c; c0 += kVoxelChunk) {
    double s[CH];
    const int j0 = c0 + lane * kVoxelGroup;
    const int j1 = j0 + kVoxelGroup < c ? j0 + kVoxelGroup : c;
    voxel_group_sum<CH>(src, stride, rows, j0, j1, s);  // (j0 >= c: no member, +0.0)
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1)
#pragma unroll
      for (int k = 0; k < CH; ++k) s[k] += __shfl_xor(s[k], off, kWave);
#pragma unroll
    for (int k = 0; k < CH; ++k) tot[k] += s[k];
  }
}

// how a voxel is summed: by one lane that knows it has at most one group (the tree and the chunk loop reduce to the group
// sum: x + 0.0 is x for every x but -0.0, which no group sum is), by one lane whatever its size, or by one wave
enum VoxelHow { kVoxelOneGroup, kVoxelLane, kVoxelWave };

template <int CH, VoxelHow HOW>
__device__ __forceinline__ void voxel_mean(const float* __restrict__ src, int stride, const uint32_t* __restrict__ rows,
                                           int c, float* __restrict__ out) {
  double tot[CH];
  if (HOW == kVoxelWave) voxel_sum_wave<CH>(src, stride, rows, c, tot);
  else if (HOW == kVoxelLane) voxel_sum_lane<CH>(src, stride, rows, c, tot);
  else voxel_group_sum<CH>(src, stride, rows, 0, c, tot);
  const double dc = (double)c;
  if (HOW != kVoxelWave || (threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < CH; ++k) out[k] = (float)(tot[k] / dc);
  }
}

// centroid and pooled features of one voxel: members rows[0 .. c) of cloud n
template <VoxelHow HOW>
__device__ void voxel_means(const float* __restrict__ points, const float* __restrict__ features, int64_t cloud_row0,
                            int C, const uint32_t* __restrict__ rows, int c, float* __restrict__ centroid,
                            float* __restrict__ pooled) {
  voxel_mean<3, HOW>(points + cloud_row0 * 3, 3, rows, c, centroid);
  const float* __restrict__ f = features + cloud_row0 * C;  // (never dereferenced when C == 0)
  int k = 0;
  for (; k + 4 <= C; k += 4) voxel_mean<4, HOW>(f + k, C, rows, c, pooled + k);
  switch (C - k) {
    case 3: voxel_mean<3, HOW>(f + k, C, rows, c, pooled + k); break;
    case 2: voxel_mean<2, HOW>(f + k, C, rows, c, pooled + k); break;
    case 1: voxel_mean<1, HOW>(f + k, C, rows, c, pooled + k); break;
    default: break;
  }
}

// one lane per voxel row: counts, the fill of the rows >= V, and the means of the voxels of up to lane_max members
// (HOW = kVoxelOneGroup needs lane_max <= kVoxelGroup)
template <VoxelHow HOW>
__global__ __launch_bounds__(kVoxelBlock) void voxel_reduce_lane_kernel(
    VoxelSorted s, int P, int C, int lane_max, const float* __restrict__ points, const float* __restrict__ features,
    const int64_t* __restrict__ num_voxels, int64_t* __restrict__ counts, int64_t* __restrict__ first_index,
    int64_t* __restrict__ coords, float* __restrict__ centroids, float* __restrict__ pooled) {
  const int n = blockIdx.y;
  const int t = blockIdx.x * kVoxelBlock + (int)threadIdx.x;
  if (t >= P) return;
  const int64_t base = (int64_t)n * P, row = base + t;
  if (t >= (int)num_voxels[n]) {
    counts[row] = 0;
    first_index[row] = -1;
    if (coords != nullptr) coords[row * 3] = coords[row * 3 + 1] = coords[row * 3 + 2] = 0;
    centroids[row * 3] = centroids[row * 3 + 1] = centroids[row * 3 + 2] = 0.0f;
    for (int k = 0; k < C; ++k) pooled[row * C + k] = 0.0f;
    return;
  }
  const int32_t* const start = s.start + (int64_t)n * (P + 1);
  const int a = start[t], c = start[t + 1] - a;
  counts[row] = c;
  if (a < 0 || c < 0 || a + c > P) return;  // (cannot happen: the member list stays inside the cloud)
  if (c > lane_max) return;  // the wave kernel's
  voxel_means<HOW>(points, features, base, C, s.rows + base + a, c, centroids + row * 3, pooled + row * C);
}

// One wave per position that is a multiple of `step`: it takes the voxel that holds the position when it is the first
// such position of that voxel and the voxel has more than lane_max members.  step <= lane_max + 1 reaches every such
// voxel exactly once: (kVoxelGroup, kVoxelGroup) by default, (1, 0) when every voxel is to come here.
__global__ __launch_bounds__(kVoxelBlock) void voxel_reduce_wave_kernel(
    VoxelSorted s, int P, int C, int lane_max, int step, const float* __restrict__ points,
    const float* __restrict__ features, float* __restrict__ centroids, float* __restrict__ pooled) {
  const int n = blockIdx.y;
  const int w = blockIdx.x * (kVoxelBlock / kWave) + (int)threadIdx.x / kWave;
  const int64_t t = (int64_t)w * step;
  if (t >= P) return;
  const int64_t base = (int64_t)n * P;
  const int id = s.vox[base + t];
  if (id < 0) return;
  const int32_t* const start = s.start + (int64_t)n * (P + 1);
  const int a = start[id], c = start[id + 1] - a;
  if (a < 0 || a + c > P) return;              // (cannot happen, as above)
  if (c <= lane_max || t - a >= step) return;  // not long, or an earlier position of the voxel has it
  voxel_means<kVoxelWave>(points, features, base, C, s.rows + base + a, c, centroids + (base + id) * 3,
                    pooled + (base + id) * C);
}

static bool voxel_shape_ok(int64_t N, int64_t P, int64_t C) {
  return N >= 0 && N < 65536 && P >= 0 && P <= kVoxelMaxPoints && C >= 0 && C <= kVoxelMaxChannels;
}

static int voxel_cloud_bits(int64_t N) {  // clouds 0 .. N - 1
  int b = 0;
  while (((int64_t)1 << b) < N) ++b;
  return b;
}

struct VoxelLayout {
  int64_t* len;        // (N,)
  float* slots;        // (N, nslots, 6)
  VoxelFrame* frames;  // (N,)
  VoxelRec *recs_a, *recs_b;  // (N, P) each: the sort's double buffer
  uint32_t* scan;      // (N, P)
  uint32_t* rows;      // (N, P)
  int32_t* vox;        // (N, P)
  int32_t* start;      // (N, P + 1)
  void *sort_tmp, *scan_tmp;
  size_t sort_tmp_bytes, scan_tmp_bytes;
  int nslots;
  size_t bytes;
};

static VoxelLayout voxel_layout(void* ws, int64_t N, int64_t P) {
  Carver c(ws);
  VoxelLayout l;
  const size_t T = (size_t)N * (size_t)P;
  l.nslots = (int)ceil_div(P, kVoxelBoundsTile);
  l.len = (int64_t*)c.take(sizeof(int64_t) * (size_t)N);
  l.slots = (float*)c.take(sizeof(float) * 6 * (size_t)N * (size_t)l.nslots);
  l.frames = (VoxelFrame*)c.take(sizeof(VoxelFrame) * (size_t)N);
  l.recs_a = (VoxelRec*)c.take(sizeof(VoxelRec) * T);
  l.recs_b = (VoxelRec*)c.take(sizeof(VoxelRec) * T);
  l.scan = (uint32_t*)c.take(sizeof(uint32_t) * T);
  l.rows = (uint32_t*)c.take(sizeof(uint32_t) * T);
  l.vox = (int32_t*)c.take(sizeof(int32_t) * T);
  l.start = (int32_t*)c.take(sizeof(int32_t) * (size_t)N * (size_t)(P + 1));
  // rocPRIM's temporary storage, sized by its null-pointer queries (nothing is launched)
  size_t tmp = 0;
  rocprim::double_buffer<VoxelRec> db(nullptr, nullptr);
  (void)rocprim::radix_sort_keys(nullptr, tmp, db, T, VoxelRecOrder{}, 0u, (unsigned)(64 + voxel_cloud_bits(N)),
                                 (hipStream_t)0);
  l.sort_tmp_bytes = tmp;
  l.sort_tmp = c.take(tmp);
  tmp = 0;
  (void)rocprim::exclusive_scan(nullptr, tmp, VoxelFlagIterator(rocprim::counting_iterator<size_t>(0), VoxelHeadFlag{nullptr}),
                                (uint32_t*)nullptr, (uint32_t)0, T, rocprim::plus<uint32_t>(), (hipStream_t)0);
  l.scan_tmp_bytes = tmp;
  l.scan_tmp = c.take(tmp);
  l.bytes = c.off;
  return l;
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_voxel_workspace_bytes(int64_t N, int64_t P, int64_t C) {
  if (!voxel_shape_ok(N, P, C) || N == 0 || P == 0) return 0;
  return voxel_layout(nullptr, N, P).bytes;
}

extern "C" int pointops_voxel_downsample(const float* points, const int64_t* lengths, const float* features,
                                         const float* origin, int origin_per_cloud, int64_t N, int64_t P, int64_t C,
                                         float voxel_size, int64_t* num_voxels, int32_t* status, int64_t* inverse,
                                         int64_t* counts, int64_t* first_index, int64_t* coords, float* centroids,
                                         float* pooled, void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(voxel_shape_ok(N, P, C), "voxel_downsample: need 0 <= N < 65536, 0 <= P <= 2^24 and 0 <= C <= 1024");
  POINTOPS_REQUIRE(voxel_size > 0.0f && voxel_size <= FLT_MAX, "voxel_downsample: need a finite voxel_size > 0");
  POINTOPS_REQUIRE(C == 0 || (features != nullptr && pooled != nullptr),
                   "voxel_downsample: C > 0 needs features and pooled");
  if (N == 0) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  if (P == 0) {
    hipLaunchKernelGGL(voxel_empty_kernel, dim3((unsigned)ceil_div(N, kVoxelBlock)), dim3(kVoxelBlock), 0, stream,
                       (int)N, num_voxels, status);
    return check_launch("voxel_downsample");
  }
  const VoxelLayout l = voxel_layout(workspace, N, P);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "voxel_downsample: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  const size_t T = (size_t)N * (size_t)P;
  clamp_lengths_async(lengths, N, P, l.len, stream);
  hipLaunchKernelGGL(voxel_bounds_kernel, dim3((unsigned)l.nslots, (unsigned)N), dim3(kVoxelBlock), 0, stream, points,
                     (const int64_t*)l.len, (int)P, l.slots);
  hipLaunchKernelGGL(voxel_frame_kernel, dim3((unsigned)N), dim3(kWave), 0, stream, (const float*)l.slots, l.nslots,
                     origin, origin_per_cloud, voxel_size, l.frames, status);
  const dim3 pgrid((unsigned)ceil_div(P, kVoxelBlock), (unsigned)N);
  hipLaunchKernelGGL(voxel_keys_kernel, pgrid, dim3(kVoxelBlock), 0, stream, points, (const int64_t*)l.len, (int)P,
                     voxel_size, (const VoxelFrame*)l.frames, l.recs_a);
  rocprim::double_buffer<VoxelRec> db(l.recs_a, l.recs_b);
  size_t tmp = l.sort_tmp_bytes;
  if (rocprim::radix_sort_keys(l.sort_tmp, tmp, db, T, VoxelRecOrder{}, 0u, (unsigned)(64 + voxel_cloud_bits(N)),
                               stream) != hipSuccess) {
    set_error("voxel_downsample: rocprim::radix_sort_keys failed");
    return POINTOPS_ELAUNCH;
  }
  VoxelSorted s;
  s.recs = db.current();
  s.scan = l.scan;
  s.rows = l.rows;
  s.vox = l.vox;
  s.start = l.start;
  tmp = l.scan_tmp_bytes;
  if (rocprim::exclusive_scan(l.scan_tmp, tmp, VoxelFlagIterator(rocprim::counting_iterator<size_t>(0), VoxelHeadFlag{s.recs}),
                              l.scan, (uint32_t)0, T, rocprim::plus<uint32_t>(), stream) != hipSuccess) {
    set_error("voxel_downsample: rocprim::exclusive_scan failed");
    return POINTOPS_ELAUNCH;
  }
  hipLaunchKernelGGL(voxel_finish_kernel, pgrid, dim3(kVoxelBlock), 0, stream, s, (int)P,
                     (const VoxelFrame*)l.frames, num_voxels, inverse, first_index, coords);
  // which voxels a lane sums alone: up to a group by default; all of them / none of them under the knob
  const long force = debug_knob("voxel_long", -1);
  const int lane_max = force == 0 ? INT_MAX : (force == 1 ? 0 : kVoxelGroup);
  const int step = force == 1 ? 1 : kVoxelGroup;
  hipLaunchKernelGGL(force == 0 ? voxel_reduce_lane_kernel<kVoxelLane> : voxel_reduce_lane_kernel<kVoxelOneGroup>, pgrid,
                     dim3(kVoxelBlock), 0, stream, s, (int)P, (int)C, lane_max, points, features,
                     (const int64_t*)num_voxels, counts, first_index, coords, centroids, pooled);
  if (force != 0) {
    const int64_t waves = ceil_div(P, step);
    hipLaunchKernelGGL(voxel_reduce_wave_kernel, dim3((unsigned)ceil_div(waves, kVoxelBlock / kWave), (unsigned)N),
                       dim3(kVoxelBlock), 0, stream, s, (int)P, (int)C, lane_max, step, points, features, centroids,
                       pooled);
  }
  return check_launch("voxel_downsample");
}

// consensus.h -- the hypothesise-score-select skeleton of the consensus operators (ransac.hip, plane.hip), written
// once: every step that does not depend on the model.  A translation unit brings its record type, the rule that makes a
// row valid, its hypothesis and score kernels, the per-row residual of its evaluation and the copy of the winner.
//
//   draws        consensus_draw.h: the counter-based hash and the draw of three distinct records
//   compaction   cs_tile_count_kernel / cs_compact_kernel: a workgroup per tile of 2048 rows (8 consecutive rows per
//                thread) counts its valid rows; the second pass adds the counts of the tiles before its own and writes
//                its records in ascending row order (block_exclusive_sum), and the last tile M_n.  (One workgroup per
//                cloud walking all the tiles was bound by one CU's gather latency: DESIGN 4.8.)
//   selection    cs_count_kernel sums the chunk partials of a hypothesis and reduces a tile of 256 keys; cs_best
//                reduces a cloud's tile keys to the winner: integers only.  (One workgroup per cloud summing all S H
//                partials itself took as long as the scoring at H = 4096, M = 65536.)
//   evaluation   cs_block_partials: the fixed-order reduction of a block's fp64 sums and count; cs_accept / cs_publish:
//                the accept rule and the outputs every model has.
//   host         the limits, the seven workspace arrays, the launch geometry and the launches of the kernels above.
#pragma once
#include "common.h"
#include "consensus_draw.h"
#include "wave.h"

namespace pointops {

// ------------------------------------------------------------------------------------------ constants and sizing
constexpr int kCsBlock = 256;
constexpr int kCsWaves = kCsBlock / kWave;
constexpr int kCsRows = 8;                   // rows per thread: consecutive in the compaction, the evaluation's sizing
constexpr int kCsTile = kCsBlock * kCsRows;  // rows per tile of the compaction (2048)
constexpr int kCsMaxBlocks = 32;             // evaluation partials per cloud

inline int64_t cs_tiles(int64_t P) { return P > 0 ? ceil_div(P, (int64_t)kCsTile) : 1; }

inline int cs_eval_blocks(int64_t P) {
  const int64_t nb = ceil_div(P, (int64_t)kCsTile);
  return (int)(nb < 1 ? 1 : (nb > kCsMaxBlocks ? kCsMaxBlocks : nb));
}

// (the chunks of a cloud are a grid's y coordinate, the tiles of 256 hypotheses its x, the cloud its z)
inline bool cs_shape_ok(int64_t N, int64_t P, int64_t H, int chunk) {
  return N >= 0 && N < 65536 && P >= 0 && P <= 65535LL * chunk && H >= 1 && H <= (1LL << 24);
}

// ---------------------------------------------------------------------------------------------------- compaction
// SRC, by value: `Record`; enter(n) reads what cloud n's rows share (its lengths), once; key(n, i) >= 0 when row i is
// valid; store(out, at, n, i, key) writes the row's record to out[at], out the records of cloud n.  Workgroup (tile, n)
// owns rows [tile * kCsTile, +kCsTile) of cloud n; a thread owns kCsRows consecutive rows of them, so thread order is
// row order.  Returns how many of its rows are valid.
template <class SRC>
__device__ __forceinline__ int cs_tile_keys(SRC& src, int n, int (&key)[kCsRows]) {
  const int first = blockIdx.x * kCsTile + (int)threadIdx.x * kCsRows;
  src.enter(n);
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kCsRows; ++k) {
    key[k] = src.key(n, first + k);
    mine += key[k] >= 0 ? 1 : 0;
  }
  return mine;
}

template <class SRC>
__global__ __launch_bounds__(kCsBlock) void cs_tile_count_kernel(SRC src, int* __restrict__ tile_count) {
  __shared__ int s_wsum[kCsWaves];
  const int n = blockIdx.y;
  int key[kCsRows], total;
  const int mine = cs_tile_keys(src, n, key);
  block_exclusive_sum<kCsWaves>(mine, s_wsum, total);
  if (threadIdx.x == 0) tile_count[(int64_t)n * gridDim.x + blockIdx.x] = total;
}

template <class SRC>
__global__ __launch_bounds__(kCsBlock) void cs_compact_kernel(SRC src, const int* __restrict__ tile_count, int P,
                                                              typename SRC::Record* __restrict__ records,
                                                              int* __restrict__ num_valid) {
  __shared__ int s_wsum[kCsWaves];
  const int n = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
  int base = 0;
  for (int t = 0; t < tile; ++t) base += tile_count[(int64_t)n * tiles + t];  // (uniform: scalar loads)
  int key[kCsRows], total;
  const int mine = cs_tile_keys(src, n, key);
  int at = base + block_exclusive_sum<kCsWaves>(mine, s_wsum, total);
  const int first = tile * kCsTile + (int)threadIdx.x * kCsRows;
#pragma unroll
  for (int k = 0; k < kCsRows; ++k) {
    if (key[k] < 0) continue;
    src.store(records + (int64_t)n * P, at, n, first + k, key[k]);
    ++at;
  }
  if (tile == tiles - 1 && threadIdx.x == 0) num_valid[n] = base + total;
}

// ----------------------------------------------------------------------------------------------------- selection
// A hypothesis' key: count in the high word, the inverted index in the low one, so that the maximum is the largest
// count at the lowest index; 0 = no valid hypothesis (a valid one has a low word >= 1).
__device__ __forceinline__ unsigned long long cs_key(int count, int h) {
  return ((unsigned long long)(uint32_t)count << 32) | (uint32_t)(0xffffffffu - (uint32_t)h);
}

// the hypothesis of a key, -1 for none
__device__ __forceinline__ int64_t cs_key_index(unsigned long long key) {
  return key == 0ull ? -1 : (int64_t)(0xffffffffu - (uint32_t)(key & 0xffffffffull));
}

// The largest key of the workgroup, valid in thread 0.
__device__ __forceinline__ unsigned long long cs_block_max(unsigned long long key) {
  __shared__ unsigned long long s_key[kCsWaves];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, kWave);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) s_key[threadIdx.x / kWave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kCsWaves; ++w) key = s_key[w] > key ? s_key[w] : key;
  }
  return key;
}

// One lane per (cloud, hypothesis): the sum of its chunk partials (coalesced over the hypotheses), the optional
// `counts` output, and the tile's largest key.  CHUNK: the records of one scoring block.
template <int CHUNK>
__global__ __launch_bounds__(kCsBlock) void cs_count_kernel(
    const int* __restrict__ num_valid, const int* __restrict__ partials, const int* __restrict__ hyp_valid, int H,
    int S, int* __restrict__ counts, unsigned long long* __restrict__ tile_keys) {
  const int n = blockIdx.y;
  const int live = (num_valid[n] + CHUNK - 1) / CHUNK;  // <= S
  const int h = blockIdx.x * kCsBlock + (int)threadIdx.x;
  unsigned long long key = 0ull;
  if (h < H) {
    int c = -1;
    if (hyp_valid[(int64_t)n * H + h] != 0) {
      c = 0;
#pragma unroll 8
      for (int k = 0; k < live; ++k) c += partials[((int64_t)n * S + k) * H + h];
      key = cs_key(c, h);
    }
    if (counts != nullptr) counts[(int64_t)n * H + h] = c;
  }
  key = cs_block_max(key);
  if (threadIdx.x == 0) tile_keys[(int64_t)n * gridDim.x + blockIdx.x] = key;
}

// The winning hypothesis of cloud n from its tile keys, or -1; a whole workgroup calls it, thread 0 has the result.
__device__ __forceinline__ int64_t cs_best(const unsigned long long* __restrict__ tile_keys, int tiles, int n) {
  unsigned long long key = 0ull;
  for (int t = threadIdx.x; t < tiles; t += kCsBlock) {
    const unsigned long long o = tile_keys[(int64_t)n * tiles + t];
    key = o > key ? o : key;
  }
  return cs_key_index(cs_block_max(key));
}

// ---------------------------------------------------------------------------------------------------- evaluation
// A block's partials from the per-thread sums and count, in a fixed order (the rmse is a sum of doubles that reruns and
// graph replays must reproduce): the 64-lane butterfly, then thread 0 adds waves 1, 2, 3.  Sum m goes to
// out_sum[m * nb]: a cloud's partials are (K, nb), so the finishing block reads the nb partials of a sum from
// consecutive addresses.
template <int K>
__device__ __forceinline__ void cs_block_partials(double (&sum)[K], int cnt, int nb, double* __restrict__ out_sum,
                                                  int* __restrict__ out_count) {
  __shared__ double s_sum[kCsWaves][K];
  __shared__ int s_cnt[kCsWaves];
#pragma unroll
  for (int m = 0; m < K; ++m) sum[m] = wave_sum(sum[m]);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int m = 0; m < K; ++m) s_sum[threadIdx.x / kWave][m] = sum[m];
    s_cnt[threadIdx.x / kWave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kCsWaves; ++w) {
#pragma unroll
      for (int m = 0; m < K; ++m) sum[m] += s_sum[w][m];
      cnt += s_cnt[w];
    }
#pragma unroll
    for (int m = 0; m < K; ++m) out_sum[(int64_t)m * nb] = sum[m];
    *out_count = cnt;
  }
}

// The finishing block of cloud n, every thread: the candidate's count and sum of squared residuals from the block
// partials (ascending; part_sum: the nb sums of cloud n) and the accept rule.  `first`: the
// winner's own evaluation, always accepted.  stopped[n] != 0: a fit was rejected (or no hypothesis is valid) and the
// cloud keeps what it has.  The decision is workgroup-uniform; after it nothing has been read that thread 0 writes.
__device__ __forceinline__ bool cs_accept(const double* __restrict__ part_sum, const int* __restrict__ part_count,
                                          int nb, int n, int first, bool cand_ok,
                                          int* __restrict__ stopped, const int64_t* __restrict__ num_inliers, int& cnt,
                                          double& sum) {
  sum = 0.0;
  cnt = 0;
#pragma unroll 4  // (scalar loads: one wait per four partials instead of one per trip)
  for (int b = 0; b < nb; ++b) {
    sum += part_sum[b];
    cnt += part_count[(int64_t)n * nb + b];
  }
  const bool accept = first ? true : (stopped[n] == 0 && cand_ok && (int64_t)cnt >= num_inliers[n]);
  __syncthreads();
  if (!accept && threadIdx.x == 0) stopped[n] = 1;
  return accept;
}

// thread 0 of an accepted evaluation: what every model publishes
__device__ __forceinline__ void cs_publish(int n, int first, const int64_t* __restrict__ best, int cnt, double sum,
                                           int* __restrict__ stopped, int64_t* __restrict__ num_inliers,
                                           float* __restrict__ rmse) {
  if (first) stopped[n] = best[n] < 0 ? 1 : 0;
  num_inliers[n] = cnt;
  rmse[n] = (float)sqrt(sum / (double)(cnt > 1 ? cnt : 1));
}

// ----------------------------------------------------------------------------------------------------- host side
// The workspace arrays every model has.
struct CsLayout {
  int* num_valid;   // (N,)
  int* tile_count;  // (N, ceil(P / 2048))
  int* hyp_valid;   // (N, H)
  int* partials;    // (N, S, H)
  unsigned long long* tile_keys;  // (N, ceil(H / 256))
  int* part_count;  // (N, nb)
  int* stopped;     // (N,)
};

inline CsLayout cs_layout(Carver& c, int64_t N, int64_t P, int64_t H, int chunk) {
  CsLayout l;
  const size_t n = (size_t)N, h = (size_t)H;
  l.num_valid = (int*)c.take(sizeof(int) * n);
  l.tile_count = (int*)c.take(sizeof(int) * n * (size_t)cs_tiles(P));
  l.hyp_valid = (int*)c.take(sizeof(int) * n * h);
  l.partials = (int*)c.take(sizeof(int) * n * (size_t)ceil_div(P, chunk) * h);
  l.tile_keys = (unsigned long long*)c.take(sizeof(unsigned long long) * n * (size_t)ceil_div(H, kCsBlock));
  l.part_count = (int*)c.take(sizeof(int) * n * (size_t)cs_eval_blocks(P));
  l.stopped = (int*)c.take(sizeof(int) * n);
  return l;
}

// The launch geometry of every step; each runs workgroups of kCsBlock.
struct CsGrid {
  unsigned tiles, S;  // tiles of 256 hypotheses, chunks of records
  int nb;             // evaluation blocks per cloud
  dim3 compact, hyp, eval, cloud;
  CsGrid(int64_t N, int64_t P, int64_t H, int chunk)
      : tiles((unsigned)ceil_div(H, kCsBlock)), S((unsigned)ceil_div(P, chunk)), nb(cs_eval_blocks(P)),
        compact((unsigned)cs_tiles(P), (unsigned)N), hyp(tiles, (unsigned)N), eval((unsigned)nb, (unsigned)N),
        cloud((unsigned)N) {}
};

template <class SRC>
inline void cs_launch_compact(const SRC& src, const CsGrid& g, const CsLayout& l, int64_t P,
                              typename SRC::Record* records, hipStream_t stream) {
  hipLaunchKernelGGL(cs_tile_count_kernel<SRC>, g.compact, dim3(kCsBlock), 0, stream, src, l.tile_count);
  hipLaunchKernelGGL(cs_compact_kernel<SRC>, g.compact, dim3(kCsBlock), 0, stream, src, (const int*)l.tile_count,
                     (int)P, records, l.num_valid);
}

template <int CHUNK>
inline void cs_launch_count(const CsGrid& g, const CsLayout& l, int64_t H, int* counts, hipStream_t stream) {
  hipLaunchKernelGGL(cs_count_kernel<CHUNK>, g.hyp, dim3(kCsBlock), 0, stream, (const int*)l.num_valid,
                     (const int*)l.partials, (const int*)l.hyp_valid, (int)H, (int)g.S, counts, l.tile_keys);
}

}  // namespace pointops

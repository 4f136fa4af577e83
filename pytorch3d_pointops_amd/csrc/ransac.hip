// ransac.hip -- RANSAC over putative correspondences: thousands of three-pair hypotheses per cloud, each scored
// against every valid correspondence, the winner refined on its inliers.  Device half of functions/ransac.py; the
// definition is the comment of pointops_ransac_alignment in include/pointops_amd.h.
//
// The torch composition it replaces solves an (N H)-batched SVD and builds an (N, H, C) residual tensor (hundreds of MB
// at H = 4096, C = 65536).  Here nothing of that size exists:
//
//   1. ransac_pair_count_kernel / ransac_pairs_kernel   a workgroup per tile of 2048 rows (8 consecutive rows per
//      thread) counts its valid pairs; the second pass adds the counts of the tiles before its own and writes its valid
//      pairs, in ascending row order (block_exclusive_sum), as 32-byte records (x, y, row, pad), and the last tile M_n.
//      (One workgroup per cloud walking all the tiles was bound by one CU's gather latency: DESIGN 4.8.)
//   2. ransac_hypotheses_kernel   one lane per (cloud, hypothesis): draws three distinct records (or reads the caller's
//      rows), runs the validity tests and solves the three-pair alignment in fp64 (ransac_hypothesis.h).
//   3. ransac_score_kernel        the hot path, H M residuals per cloud.  One lane = one hypothesis with A = s R and T
//      in 12 VGPRs and an integer counter.  Every lane of a wave consumes the SAME record, whose address is built from
//      blockIdx and the loop counter only, so the records arrive through the scalar path (s_load_dwordx8 into SGPRs,
//      as knn.hip streams p2) and feed the VALU as scalar operands.  blockIdx.y splits the records of a cloud into
//      chunks of kRansacChunk so that a small N H still fills the device; each (chunk, hypothesis) writes one int32.
//   4. ransac_count_kernel        one lane per hypothesis sums its chunk partials and a tile of 256 reduces the 64-bit
//      key (count high, inverted index low); ransac_select_kernel, one workgroup per cloud, reduces the tile keys to
//      the winner and writes best and the candidate transform: integers only.  (One workgroup per cloud summing all
//      S H partials itself took as long as the scoring at H = 4096, M = 65536: 256 chunks of 4096 counts on 8 CUs.)
//   5. ransac_evaluate_kernel / ransac_finish_kernel   mask, count and fp64 block partials of sum d2 of a candidate
//      transform; one finishing block per cloud applies the accept rule and writes the public outputs.  Between two
//      evaluations the refinement is pointops_points_alignment weighted by the current mask, on the same stream.
//
// No atomics, no host read-back: bit-reproducible and capturable into a HIP graph.
#include "common.h"
#include "debug.h"
#include "ransac_hypothesis.h"
#include "ransac_select.h"
#include "wave.h"

namespace pointops {

constexpr int kRansacChunk = 256;  // records per scoring block (exported: pointops_ransac_chunk)
constexpr int kRsPairRows = 8;     // consecutive rows per thread of the compaction
constexpr int kRsPairTile = kRsBlock * kRsPairRows;  // rows per step of the compaction (2048)
constexpr int kRsRowsPerThread = 8;
constexpr int kRsMaxBlocks = 32;   // evaluation partials per cloud

struct alignas(32) RansacRecord {
  float x[3];
  float y[3];
  int row;
  int pad;
};
static_assert(sizeof(RansacRecord) == 32, "a record is two 16-byte stores");

inline int64_t rs_pair_tiles(int64_t P) { return P > 0 ? ceil_div(P, (int64_t)kRsPairTile) : 1; }

inline int rs_eval_blocks(int64_t P) {
  const int64_t nb = ceil_div(P, (int64_t)kRsBlock * kRsRowsPerThread);
  return (int)(nb < 1 ? 1 : (nb > kRsMaxBlocks ? kRsMaxBlocks : nb));
}

// the row of Y that row i of X is matched to, or -1 when the row is no valid correspondence
__device__ __forceinline__ int rs_target(const int64_t* __restrict__ corr, int n, int P1, int i, int len1, int len2) {
  if (i < 0 || i >= len1) return -1;
  const int64_t j = corr != nullptr ? corr[(int64_t)n * P1 + i] : (int64_t)i;
  return (j >= 0 && j < len2) ? (int)j : -1;
}

// ---------------------------------------------------------------------------------------------------- 1. compaction
// Workgroup (tile, n) owns rows [tile * kRsPairTile, +kRsPairTile) of cloud n; a thread owns kRsPairRows consecutive
// rows of them, so thread order is row order.  The targets of the thread's rows; returns how many are valid.
__device__ __forceinline__ int rs_tile_targets(const int64_t* __restrict__ corr, int n, int P1, int len1, int len2,
                                               int (&j)[kRsPairRows]) {
  const int first = blockIdx.x * kRsPairTile + (int)threadIdx.x * kRsPairRows;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kRsPairRows; ++k) {
    j[k] = rs_target(corr, n, P1, first + k, len1, len2);
    mine += j[k] >= 0 ? 1 : 0;
  }
  return mine;
}

__global__ __launch_bounds__(kRsBlock) void ransac_pair_count_kernel(
    const int64_t* __restrict__ corr, const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
    int P1, int P2, int* __restrict__ tile_pairs) {
  __shared__ int s_wsum[kRsWaves];
  const int n = blockIdx.y;
  int j[kRsPairRows], total;
  const int mine = rs_tile_targets(corr, n, P1, rs_length(lengths1, n, P1), rs_length(lengths2, n, P2), j);
  block_exclusive_sum<kRsWaves>(mine, s_wsum, total);
  if (threadIdx.x == 0) tile_pairs[(int64_t)n * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(kRsBlock) void ransac_pairs_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ corr,
    const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2, int P1, int P2,
    const int* __restrict__ tile_pairs, RansacRecord* __restrict__ records, int* __restrict__ num_pairs) {
  __shared__ int s_wsum[kRsWaves];
  const int n = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
  const float* __restrict__ xs = X + (int64_t)n * P1 * 3;
  const float* __restrict__ ys = Y + (int64_t)n * P2 * 3;
  float4* __restrict__ out = (float4*)(records + (int64_t)n * P1);
  int base = 0;
  for (int t = 0; t < tile; ++t) base += tile_pairs[(int64_t)n * tiles + t];  // (uniform: scalar loads)
  int j[kRsPairRows], total;
  const int mine = rs_tile_targets(corr, n, P1, rs_length(lengths1, n, P1), rs_length(lengths2, n, P2), j);
  int at = base + block_exclusive_sum<kRsWaves>(mine, s_wsum, total);
  const int first = tile * kRsPairTile + (int)threadIdx.x * kRsPairRows;
#pragma unroll
  for (int k = 0; k < kRsPairRows; ++k) {
    if (j[k] < 0) continue;
    const int64_t i = first + k, t = j[k];
    const float x0 = xs[i * 3], x1 = xs[i * 3 + 1], x2 = xs[i * 3 + 2];
    const float y0 = ys[t * 3], y1 = ys[t * 3 + 1], y2 = ys[t * 3 + 2];
    out[2 * (int64_t)at] = make_float4(x0, x1, x2, y0);
    out[2 * (int64_t)at + 1] = make_float4(y1, y2, __int_as_float((int)i), 0.0f);
    ++at;
  }
  if (tile == tiles - 1 && threadIdx.x == 0) num_pairs[n] = base + total;
}

// ---------------------------------------------------------------------------------------------------- 2. hypotheses
__global__ __launch_bounds__(kRsBlock) void ransac_hypotheses_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ corr,
    const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
    const int64_t* __restrict__ samples_in, int P1, int P2, int H, int64_t seed, int64_t first_cloud, float q,
    int edge_test, int estimate_scale, const RansacRecord* __restrict__ records, const int* __restrict__ num_pairs,
    float* __restrict__ ws_R, float* __restrict__ ws_T, float* __restrict__ ws_s, int* __restrict__ ws_valid,
    float* __restrict__ hyp_R, float* __restrict__ hyp_T, float* __restrict__ hyp_s,
    int64_t* __restrict__ samples_out) {
  const int n = blockIdx.y;
  const int h = blockIdx.x * kRsBlock + (int)threadIdx.x;
  if (h >= H) return;
  const int64_t slot = (int64_t)n * H + h;
  float x[3][3], y[3][3];
  int64_t rows[3] = {-1, -1, -1};
  bool valid;
  if (samples_in != nullptr) {
    const int len1 = rs_length(lengths1, n, P1), len2 = rs_length(lengths2, n, P2);
    valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      rows[k] = samples_in[slot * 3 + k];
      const int i = (rows[k] >= 0 && rows[k] < P1) ? (int)rows[k] : -1;
      const int j = rs_target(corr, n, P1, i, len1, len2);
      valid = valid && j >= 0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        x[k][d] = j >= 0 ? X[((int64_t)n * P1 + i) * 3 + d] : 0.0f;
        y[k][d] = j >= 0 ? Y[((int64_t)n * P2 + j) * 3 + d] : 0.0f;
      }
    }
    valid = valid && rows[0] != rows[1] && rows[0] != rows[2] && rows[1] != rows[2];
  } else {
    const int M = num_pairs[n];
    valid = M >= 3;
    uint32_t at[3] = {0u, 0u, 0u};
    if (valid) rh_draw(seed, first_cloud + n, h, (uint32_t)M, at);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (valid) {
        const RansacRecord r = records[(int64_t)n * P1 + at[k]];
        rows[k] = r.row;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          x[k][d] = r.x[d];
          y[k][d] = r.y[d];
        }
      } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) x[k][d] = y[k][d] = 0.0f;
      }
    }
  }
  if (valid && edge_test) valid = rh_edges_ok(x, y, q);
  float R[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}}, T[3] = {0.0f, 0.0f, 0.0f}, s = 1.0f;
  if (valid) rh_solve(x, y, estimate_scale != 0, R, T, s);
  ws_valid[slot] = valid ? 1 : 0;
  ws_s[slot] = s;
  if (hyp_s != nullptr) hyp_s[slot] = s;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ws_T[slot * 3 + a] = T[a];
    if (hyp_T != nullptr) hyp_T[slot * 3 + a] = T[a];
    if (samples_out != nullptr) samples_out[slot * 3 + a] = rows[a];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      ws_R[slot * 9 + a * 3 + b] = R[a][b];
      if (hyp_R != nullptr) hyp_R[slot * 9 + a * 3 + b] = R[a][b];
    }
  }
}

// ---------------------------------------------------------------------------------------------------- 3. scoring
// A = s R of a stored transform
__device__ __forceinline__ void rs_load_transform(const float* __restrict__ R, const float* __restrict__ T,
                                                  const float* __restrict__ s, int64_t slot, float (&A)[3][3],
                                                  float (&t)[3]) {
  const float sc = s[slot];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t[a] = T[slot * 3 + a];
#pragma unroll
    for (int b = 0; b < 3; ++b) A[a][b] = sc * R[slot * 9 + a * 3 + b];
  }
}

// LDS = false: the scalar path.  LDS = true (POINTOPS_DEBUG="ransac_lds=1", the A/B of DESIGN 4.8): the workgroup
// copies its chunk into an LDS tile and every lane reads the same address (a broadcast).  The results are the same.
template <bool LDS>
__global__ __launch_bounds__(kRsBlock) void ransac_score_kernel(
    const RansacRecord* __restrict__ records, const int* __restrict__ num_pairs, const float* __restrict__ ws_R,
    const float* __restrict__ ws_T, const float* __restrict__ ws_s, const int* __restrict__ ws_valid, int P1, int H,
    int S, float thr2, int* __restrict__ partials) {
  __shared__ float4 s_rec[LDS ? 2 * kRansacChunk : 1];
  const int n = blockIdx.z, chunk = blockIdx.y;  // wave-uniform
  const int M = num_pairs[n];
  const int beg = chunk * kRansacChunk;
  if (beg >= M) return;  // (workgroup-uniform; select reads the chunks below ceil(M / chunk) only)
  const int end = min(beg + kRansacChunk, M);
  const RansacRecord* __restrict__ rec = records + (int64_t)n * P1;
  if constexpr (LDS) {
    static_assert(kRansacChunk == kRsBlock, "one record per thread");
    if (beg + (int)threadIdx.x < end) {
      const float4* __restrict__ src = (const float4*)(rec + beg + threadIdx.x);
      s_rec[2 * threadIdx.x] = src[0];
      s_rec[2 * threadIdx.x + 1] = src[1];
    }
    __syncthreads();
  }
  const int h = blockIdx.x * kRsBlock + (int)threadIdx.x;
  const bool valid = h < H && ws_valid[(int64_t)n * H + h] != 0;
  int* __restrict__ out = partials + ((int64_t)n * S + chunk) * H;
  if (__ballot(valid) == 0ull) {  // the whole wave is invalid
    if (h < H) out[h] = -1;
    return;
  }
  float A[3][3] = {{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}}, T[3] = {0.0f, 0.0f, 0.0f};
  if (valid) rs_load_transform(ws_R, ws_T, ws_s, (int64_t)n * H + h, A, T);
  int count = 0;
  if constexpr (LDS) {
#pragma unroll 4
    for (int j = 0; j < end - beg; ++j) {
      const float4 a = s_rec[2 * j], b = s_rec[2 * j + 1];
      count += rh_residual(A, T, a.x, a.y, a.z, a.w, b.x, b.y) <= thr2 ? 1 : 0;
    }
  } else {
#pragma unroll 4
    for (int j = beg; j < end; ++j) {  // a uniform address: the record arrives in SGPRs
      const RansacRecord r = rec[j];
      count += rh_residual(A, T, r.x[0], r.x[1], r.x[2], r.y[0], r.y[1], r.y[2]) <= thr2 ? 1 : 0;
    }
  }
  if (h < H) out[h] = valid ? count : -1;
}

// ---------------------------------------------------------------------------------------------------- 4. selection
// One lane per (cloud, hypothesis): the sum of its chunk partials (coalesced over the hypotheses), the optional
// `counts` output, and the tile's largest key -- count in the high word, the inverted index in the low one, so that
// the maximum is the largest count at the lowest index; 0 = no valid hypothesis (a valid one has a low word >= 1).
__global__ __launch_bounds__(kRsBlock) void ransac_count_kernel(
    const int* __restrict__ num_pairs, const int* __restrict__ partials, const int* __restrict__ ws_valid, int H, int S,
    int* __restrict__ counts, unsigned long long* __restrict__ tile_keys) {
  __shared__ unsigned long long s_key[kRsWaves];
  const int n = blockIdx.y;
  const int live = (num_pairs[n] + kRansacChunk - 1) / kRansacChunk;  // <= S
  const int h = blockIdx.x * kRsBlock + (int)threadIdx.x;
  unsigned long long key = 0ull;
  if (h < H) {
    int c = -1;
    if (ws_valid[(int64_t)n * H + h] != 0) {
      c = 0;
      for (int k = 0; k < live; ++k) c += partials[((int64_t)n * S + k) * H + h];
      key = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)(0xffffffffu - (uint32_t)h);
    }
    if (counts != nullptr) counts[(int64_t)n * H + h] = c;
  }
  key = rs_block_max(key, s_key);
  if (threadIdx.x == 0) tile_keys[(int64_t)n * gridDim.x + blockIdx.x] = key;
}

__global__ __launch_bounds__(kRsBlock) void ransac_select_kernel(
    const unsigned long long* __restrict__ tile_keys, int tiles, const float* __restrict__ ws_R,
    const float* __restrict__ ws_T, const float* __restrict__ ws_s, int H, int64_t* __restrict__ best,
    float* __restrict__ cand_R, float* __restrict__ cand_T, float* __restrict__ cand_s) {
  __shared__ unsigned long long s_key[kRsWaves];
  const int n = blockIdx.x;
  unsigned long long key = 0ull;
  for (int t = threadIdx.x; t < tiles; t += kRsBlock) {
    const unsigned long long o = tile_keys[(int64_t)n * tiles + t];
    key = o > key ? o : key;
  }
  key = rs_block_max(key, s_key);
  if (threadIdx.x != 0) return;
  const int64_t b = key == 0ull ? -1 : (int64_t)(0xffffffffu - (uint32_t)(key & 0xffffffffull));
  best[n] = b;
  const int64_t slot = (int64_t)n * H + (b < 0 ? 0 : b);
  cand_s[n] = b < 0 ? 1.0f : ws_s[slot];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cand_T[n * 3 + a] = b < 0 ? 0.0f : ws_T[slot * 3 + a];
#pragma unroll
    for (int c = 0; c < 3; ++c) cand_R[n * 9 + a * 3 + c] = b < 0 ? (a == c ? 1.0f : 0.0f) : ws_R[slot * 9 + a * 3 + c];
  }
}

// ---------------------------------------------------------------------------------------------------- 5. evaluation
// Mask (one byte per row of X), count and sum of d2 over the inliers of the candidate transform of every cloud.
__global__ __launch_bounds__(kRsBlock) void ransac_evaluate_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ corr,
    const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2, const int64_t* __restrict__ best,
    const float* __restrict__ cand_R, const float* __restrict__ cand_T, const float* __restrict__ cand_s, int P1,
    int P2, float thr2, uint8_t* __restrict__ cand_mask, double* __restrict__ part_sum, int* __restrict__ part_count) {
  __shared__ double s_sum[kRsWaves];
  __shared__ int s_cnt[kRsWaves];
  const int n = blockIdx.y, nb = gridDim.x;
  const int len1 = rs_length(lengths1, n, P1), len2 = rs_length(lengths2, n, P2);
  const bool none = best[n] < 0;
  float A[3][3], T[3];
  rs_load_transform(cand_R, cand_T, cand_s, n, A, T);
  const float* __restrict__ xs = X + (int64_t)n * P1 * 3;
  const float* __restrict__ ys = Y + (int64_t)n * P2 * 3;
  double sum = 0.0;
  int cnt = 0;
  for (int i = blockIdx.x * kRsBlock + (int)threadIdx.x; i < P1; i += nb * kRsBlock) {
    const int j = none ? -1 : rs_target(corr, n, P1, i, len1, len2);
    bool in = false;
    if (j >= 0) {
      const float d2 = rh_residual(A, T, xs[(int64_t)i * 3], xs[(int64_t)i * 3 + 1], xs[(int64_t)i * 3 + 2],
                                   ys[(int64_t)j * 3], ys[(int64_t)j * 3 + 1], ys[(int64_t)j * 3 + 2]);
      in = d2 <= thr2;
      if (in) sum += (double)d2;
    }
    cnt += in ? 1 : 0;
    cand_mask[(int64_t)n * P1 + i] = in ? 1 : 0;
  }
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_sum[threadIdx.x / kWave] = sum;
    s_cnt[threadIdx.x / kWave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kRsWaves; ++w) {
      sum += s_sum[w];
      cnt += s_cnt[w];
    }
    part_sum[(int64_t)n * nb + blockIdx.x] = sum;
    part_count[(int64_t)n * nb + blockIdx.x] = cnt;
  }
}

// One block per cloud: the candidate's count and rmse from the block partials (ascending), the accept rule, and -- on
// acceptance -- the public transform, mask, count and rmse, and the 0/1 weights of the next fit.  `first`: the
// winner's own evaluation, always accepted.  stopped[n] != 0: a fit was rejected (or no hypothesis is valid) and the
// cloud keeps what it has.
__global__ __launch_bounds__(kRsBlock) void ransac_finish_kernel(
    const double* __restrict__ part_sum, const int* __restrict__ part_count, int nb, int first,
    const int64_t* __restrict__ best, const float* __restrict__ cand_R, const float* __restrict__ cand_T,
    const float* __restrict__ cand_s, const uint8_t* __restrict__ cand_mask, int P1, int* __restrict__ stopped,
    float* __restrict__ R, float* __restrict__ T, float* __restrict__ s, uint8_t* __restrict__ mask,
    float* __restrict__ weights, int64_t* __restrict__ num_inliers, float* __restrict__ rmse) {
  const int n = blockIdx.x;
  double sum = 0.0;
  int cnt = 0;
  for (int b = 0; b < nb; ++b) {  // (every thread: the decision is workgroup-uniform)
    sum += part_sum[(int64_t)n * nb + b];
    cnt += part_count[(int64_t)n * nb + b];
  }
  const bool accept = first ? true : (stopped[n] == 0 && (int64_t)cnt >= num_inliers[n]);
  __syncthreads();  // every thread has read stopped / num_inliers before thread 0 writes them
  if (!accept) {
    if (threadIdx.x == 0) stopped[n] = 1;
    return;
  }
  if (threadIdx.x == 0) {
    if (first) stopped[n] = best[n] < 0 ? 1 : 0;
    num_inliers[n] = cnt;
    rmse[n] = (float)sqrt(sum / (double)(cnt > 1 ? cnt : 1));
    s[n] = cand_s[n];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      T[n * 3 + a] = cand_T[n * 3 + a];
#pragma unroll
      for (int c = 0; c < 3; ++c) R[n * 9 + a * 3 + c] = cand_R[n * 9 + a * 3 + c];
    }
  }
  if ((P1 & 3) == 0 && ((uintptr_t)mask & 3) == 0) {  // four rows per access (the workspace arrays are 256-byte aligned)
    const uchar4* __restrict__ src = (const uchar4*)(cand_mask + (int64_t)n * P1);
    uchar4* __restrict__ dst = (uchar4*)(mask + (int64_t)n * P1);
    float4* __restrict__ w = (float4*)(weights + (int64_t)n * P1);
    for (int i = threadIdx.x; i < P1 / 4; i += kRsBlock) {
      const uchar4 m = src[i];
      dst[i] = m;
      w[i] = make_float4(m.x ? 1.0f : 0.0f, m.y ? 1.0f : 0.0f, m.z ? 1.0f : 0.0f, m.w ? 1.0f : 0.0f);
    }
    return;
  }
  for (int i = threadIdx.x; i < P1; i += kRsBlock) {
    const uint8_t m = cand_mask[(int64_t)n * P1 + i];
    mask[(int64_t)n * P1 + i] = m;
    weights[(int64_t)n * P1 + i] = m ? 1.0f : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------ host side
struct RansacLayout {
  RansacRecord* records;  // (N, P1)
  int* num_pairs;         // (N,)
  int* tile_pairs;        // (N, ceil(P1 / 2048))
  float *hyp_R, *hyp_T, *hyp_s;  // (N, H, 9 | 3 | 1)
  int* hyp_valid;         // (N, H)
  int* partials;          // (N, S, H)
  unsigned long long* tile_keys;  // (N, ceil(H / 256))
  float *cand_R, *cand_T, *cand_s;  // (N, 9 | 3 | 1)
  uint8_t* cand_mask;     // (N, P1)
  float* weights;         // (N, P1)
  double* part_sum;       // (N, nb)
  int* part_count;        // (N, nb)
  int* stopped;           // (N,)
  void* alignment;        // pointops_points_alignment's own
  size_t alignment_bytes;
  size_t bytes;
};

static RansacLayout ransac_layout(void* ws, int64_t N, int64_t P1, int64_t H) {
  Carver c(ws);
  RansacLayout l;
  const size_t n = (size_t)N, p = (size_t)P1, h = (size_t)H;
  const size_t S = (size_t)ceil_div(P1, kRansacChunk), nb = (size_t)rs_eval_blocks(P1);
  l.records = (RansacRecord*)c.take(sizeof(RansacRecord) * n * p);
  l.num_pairs = (int*)c.take(sizeof(int) * n);
  l.tile_pairs = (int*)c.take(sizeof(int) * n * (size_t)rs_pair_tiles(P1));
  l.hyp_R = (float*)c.take(sizeof(float) * n * h * 9);
  l.hyp_T = (float*)c.take(sizeof(float) * n * h * 3);
  l.hyp_s = (float*)c.take(sizeof(float) * n * h);
  l.hyp_valid = (int*)c.take(sizeof(int) * n * h);
  l.partials = (int*)c.take(sizeof(int) * n * S * h);
  l.tile_keys = (unsigned long long*)c.take(sizeof(unsigned long long) * n * (size_t)ceil_div(H, kRsBlock));
  l.cand_R = (float*)c.take(sizeof(float) * n * 9);
  l.cand_T = (float*)c.take(sizeof(float) * n * 3);
  l.cand_s = (float*)c.take(sizeof(float) * n);
  l.cand_mask = (uint8_t*)c.take(n * p);
  l.weights = (float*)c.take(sizeof(float) * n * p);
  l.part_sum = (double*)c.take(sizeof(double) * n * nb);
  l.part_count = (int*)c.take(sizeof(int) * n * nb);
  l.stopped = (int*)c.take(sizeof(int) * n);
  l.alignment_bytes = pointops_points_alignment_workspace_bytes(N, P1, 3);
  l.alignment = c.take(l.alignment_bytes);
  l.bytes = c.off;
  return l;
}

static bool ransac_shape_ok(int64_t N, int64_t P1, int64_t P2, int64_t H) {
  // (the chunks of a cloud are a grid's y coordinate, the tiles of 256 hypotheses its x, the cloud its z)
  return N >= 0 && N < 65536 && P1 >= 0 && P1 <= 65535LL * kRansacChunk && P2 >= 0 && P2 < (1LL << 30) && H >= 1 &&
         H <= (1LL << 24);
}

}  // namespace pointops

using namespace pointops;

extern "C" int64_t pointops_ransac_chunk(void) { return kRansacChunk; }

extern "C" size_t pointops_ransac_workspace_bytes(int64_t N, int64_t P1, int64_t H) {
  if (!ransac_shape_ok(N, P1, P1, H)) return 0;
  return ransac_layout(nullptr, N, P1, H).bytes;
}

extern "C" int pointops_ransac_alignment(
    const float* X, const float* Y, const int64_t* corr, const int64_t* lengths1, const int64_t* lengths2,
    const int64_t* samples_in, int64_t N, int64_t P1, int64_t P2, int64_t H, int64_t seed, int64_t first_cloud,
    float inlier_threshold, float edge_length_ratio, int estimate_scale, int refine_steps, float* R, float* T, float* s,
    uint8_t* inlier_mask, int64_t* num_inliers, float* rmse, int64_t* best, int32_t* counts, float* hyp_R, float* hyp_T,
    float* hyp_s, int64_t* samples_out, void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(ransac_shape_ok(N, P1, P2, H),
                   "ransac_alignment: need 0 <= N < 65536, 0 <= P1 <= 65535 * 256, 0 <= P2 < 2^30 and 1 <= H <= 2^24");
  // (P1 == 0: an empty table has no address to give, and nothing reads it)
  POINTOPS_REQUIRE(corr != nullptr || P2 == P1 || P1 == 0,
                   "ransac_alignment: without corr, Y must have P1 rows per cloud");
  POINTOPS_REQUIRE(inlier_threshold >= 0.0f && edge_length_ratio >= 0.0f && edge_length_ratio <= 1.0f,
                   "ransac_alignment: need inlier_threshold >= 0 and 0 <= edge_length_ratio <= 1");
  POINTOPS_REQUIRE(refine_steps >= 0 && first_cloud >= 0, "ransac_alignment: need refine_steps >= 0, first_cloud >= 0");
  if (N == 0) return POINTOPS_OK;
  const RansacLayout l = ransac_layout(workspace, N, P1, H);
  if (!workspace_fits(workspace, workspace_bytes, l.bytes)) {
    set_error("ransac_alignment: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
    return POINTOPS_EWORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const float thr2 = inlier_threshold * inlier_threshold;
  const float q = edge_length_ratio * edge_length_ratio;
  const int edge_test = (!estimate_scale && edge_length_ratio > 0.0f) ? 1 : 0;
  const unsigned tiles = (unsigned)ceil_div(H, kRsBlock), S = (unsigned)ceil_div(P1, kRansacChunk);
  const int nb = rs_eval_blocks(P1);

  const dim3 pair_grid((unsigned)rs_pair_tiles(P1), (unsigned)N);
  hipLaunchKernelGGL(ransac_pair_count_kernel, pair_grid, dim3(kRsBlock), 0, stream, corr, lengths1, lengths2, (int)P1,
                     (int)P2, l.tile_pairs);
  hipLaunchKernelGGL(ransac_pairs_kernel, pair_grid, dim3(kRsBlock), 0, stream, X, Y, corr, lengths1, lengths2, (int)P1,
                     (int)P2, (const int*)l.tile_pairs, l.records, l.num_pairs);
  hipLaunchKernelGGL(ransac_hypotheses_kernel, dim3(tiles, (unsigned)N), dim3(kRsBlock), 0, stream, X, Y, corr,
                     lengths1, lengths2, samples_in, (int)P1, (int)P2, (int)H, seed, first_cloud, q, edge_test,
                     estimate_scale, (const RansacRecord*)l.records, (const int*)l.num_pairs, l.hyp_R, l.hyp_T, l.hyp_s,
                     l.hyp_valid, hyp_R, hyp_T, hyp_s, samples_out);
  if (S > 0) {
    auto* score = debug_knob("ransac_lds", 0) ? ransac_score_kernel<true> : ransac_score_kernel<false>;
    hipLaunchKernelGGL(score, dim3(tiles, S, (unsigned)N), dim3(kRsBlock), 0, stream, (const RansacRecord*)l.records,
                       (const int*)l.num_pairs, (const float*)l.hyp_R, (const float*)l.hyp_T, (const float*)l.hyp_s,
                       (const int*)l.hyp_valid, (int)P1, (int)H, (int)S, thr2, l.partials);
  }
  hipLaunchKernelGGL(ransac_count_kernel, dim3(tiles, (unsigned)N), dim3(kRsBlock), 0, stream, (const int*)l.num_pairs,
                     (const int*)l.partials, (const int*)l.hyp_valid, (int)H, (int)S, counts, l.tile_keys);
  hipLaunchKernelGGL(ransac_select_kernel, dim3((unsigned)N), dim3(kRsBlock), 0, stream,
                     (const unsigned long long*)l.tile_keys, (int)tiles, (const float*)l.hyp_R, (const float*)l.hyp_T,
                     (const float*)l.hyp_s, (int)H, best, l.cand_R, l.cand_T, l.cand_s);
  int rc = check_launch("ransac_alignment");
  const int refits = P1 == 0 ? 0 : refine_steps;  // (no row, nothing to refit)
  for (int step = 0; step <= refits && rc == POINTOPS_OK; ++step) {
    if (step > 0) {
      rc = pointops_points_alignment(X, Y, corr, lengths1, l.weights, N, P1, P2, 3, estimate_scale, 0, 1e-9, l.cand_R,
                                     l.cand_T, l.cand_s, nullptr, nullptr, l.alignment, l.alignment_bytes, stream_);
      if (rc != POINTOPS_OK) return rc;
    }
    hipLaunchKernelGGL(ransac_evaluate_kernel, dim3((unsigned)nb, (unsigned)N), dim3(kRsBlock), 0, stream, X, Y, corr,
                       lengths1, lengths2, (const int64_t*)best, (const float*)l.cand_R, (const float*)l.cand_T,
                       (const float*)l.cand_s, (int)P1, (int)P2, thr2, l.cand_mask, l.part_sum, l.part_count);
    hipLaunchKernelGGL(ransac_finish_kernel, dim3((unsigned)N), dim3(kRsBlock), 0, stream, (const double*)l.part_sum,
                       (const int*)l.part_count, nb, step == 0 ? 1 : 0, (const int64_t*)best, (const float*)l.cand_R,
                       (const float*)l.cand_T, (const float*)l.cand_s, (const uint8_t*)l.cand_mask, (int)P1, l.stopped,
                       R, T, s, inlier_mask, l.weights, num_inliers, rmse);
    rc = check_launch("ransac_alignment");
  }
  return rc;
}

// ransac.hip -- RANSAC over putative correspondences: thousands of three-pair hypotheses per cloud, each scored
// against every valid correspondence, the winner refined on its inliers.  Device half of functions/ransac.py; the
// definition is the comment of pointops_ransac_alignment in include/pointops_amd.h.
//
// The torch composition it replaces solves an (N H)-batched SVD and builds an (N, H, C) residual tensor (hundreds of MB
// at H = 4096, C = 65536).  Here nothing of that size exists:
//
//   1. compaction (consensus.h over RansacPairs)   the valid pairs of a cloud, in ascending row order, as 32-byte
//      records (x, y, row, pad), and their number M_n.
//   2. ransac_hypotheses_kernel   one lane per (cloud, hypothesis): draws three distinct records (or reads the caller's
//      rows), runs the validity tests and solves the three-pair alignment in fp64 (ransac_hypothesis.h).
//   3. ransac_score_kernel        the hot path, H M residuals per cloud.  One lane = one hypothesis with A = s R and T
//      in 12 VGPRs and an integer counter.  Every lane of a wave consumes the SAME record, whose address is built from
//      blockIdx and the loop counter only, so the records arrive through the scalar path (s_load_dwordx8 into SGPRs,
//      as knn.hip streams p2) and feed the VALU as scalar operands.  blockIdx.y splits the records of a cloud into
//      chunks of kRansacChunk so that a small N H still fills the device; each (chunk, hypothesis) writes one int32.
//   4. selection (consensus.h)    the largest count at the lowest index; ransac_select_kernel copies the winner's
//      transform into the candidate.
//   5. ransac_evaluate_kernel / ransac_finish_kernel   mask, count and fp64 block partials of sum d2 of a candidate
//      transform; one finishing block per cloud applies the accept rule (consensus.h) and writes the public outputs.
//      Between two evaluations the refinement is pointops_points_alignment weighted by the current mask, on the same
//      stream.
//
// No atomics, no host read-back: bit-reproducible and capturable into a HIP graph.
#include "common.h"
#include "consensus.h"
#include "debug.h"
#include "ransac_hypothesis.h"

namespace pointops {

constexpr int kRansacChunk = 256;  // records per scoring block (exported: pointops_ransac_chunk)

struct alignas(32) RansacRecord {
  float x[3];
  float y[3];
  int row;
  int pad;
};
static_assert(sizeof(RansacRecord) == 32, "a record is two 16-byte stores");

// the row of Y that row i of X is matched to, or -1 when the row is no valid correspondence
__device__ __forceinline__ int rs_target(const int64_t* __restrict__ corr, int n, int P1, int i, int len1, int len2) {
  if (i < 0 || i >= len1) return -1;
  const int64_t j = corr != nullptr ? corr[(int64_t)n * P1 + i] : (int64_t)i;
  return (j >= 0 && j < len2) ? (int)j : -1;
}

// ---------------------------------------------------------------------------------------------------- 1. compaction
// The row source of the compaction: a row's key is its target in Y.
struct RansacPairs {
  using Record = RansacRecord;
  const float *X, *Y;
  const int64_t *corr, *lengths1, *lengths2;
  int P1, P2, len1, len2;
  __device__ __forceinline__ void enter(int n) {
    len1 = clamped_length(lengths1, n, P1);
    len2 = clamped_length(lengths2, n, P2);
  }
  __device__ __forceinline__ int key(int n, int i) const { return rs_target(corr, n, P1, i, len1, len2); }
  __device__ __forceinline__ void store(RansacRecord* __restrict__ out, int at, int n, int i, int j) const {
    const float* __restrict__ x = X + (int64_t)n * P1 * 3 + (int64_t)i * 3;
    const float* __restrict__ y = Y + (int64_t)n * P2 * 3 + (int64_t)j * 3;
    const float x0 = x[0], x1 = x[1], x2 = x[2], y0 = y[0], y1 = y[1], y2 = y[2];
    ((float4*)out)[2 * (int64_t)at] = make_float4(x0, x1, x2, y0);
    ((float4*)out)[2 * (int64_t)at + 1] = make_float4(y1, y2, __int_as_float(i), 0.0f);
  }
};

// ---------------------------------------------------------------------------------------------------- 2. hypotheses
__global__ __launch_bounds__(kCsBlock) void ransac_hypotheses_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ corr,
    const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
    const int64_t* __restrict__ samples_in, int P1, int P2, int H, int64_t seed, int64_t first_cloud, float q,
    int edge_test, int estimate_scale, const RansacRecord* __restrict__ records, const int* __restrict__ num_pairs,
    float* __restrict__ ws_R, float* __restrict__ ws_T, float* __restrict__ ws_s, int* __restrict__ ws_valid,
    float* __restrict__ hyp_R, float* __restrict__ hyp_T, float* __restrict__ hyp_s,
    int64_t* __restrict__ samples_out) {
  const int n = blockIdx.y;
  const int h = blockIdx.x * kCsBlock + (int)threadIdx.x;
  if (h >= H) return;
  const int64_t slot = (int64_t)n * H + h;
  float x[3][3], y[3][3];
  int64_t rows[3] = {-1, -1, -1};
  bool valid;
  if (samples_in != nullptr) {
    const int len1 = clamped_length(lengths1, n, P1), len2 = clamped_length(lengths2, n, P2);
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
__global__ __launch_bounds__(kCsBlock) void ransac_score_kernel(
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
    static_assert(kRansacChunk == kCsBlock, "one record per thread");
    if (beg + (int)threadIdx.x < end) {
      const float4* __restrict__ src = (const float4*)(rec + beg + threadIdx.x);
      s_rec[2 * threadIdx.x] = src[0];
      s_rec[2 * threadIdx.x + 1] = src[1];
    }
    __syncthreads();
  }
  const int h = blockIdx.x * kCsBlock + (int)threadIdx.x;
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
__global__ __launch_bounds__(kCsBlock) void ransac_select_kernel(
    const unsigned long long* __restrict__ tile_keys, int tiles, const float* __restrict__ ws_R,
    const float* __restrict__ ws_T, const float* __restrict__ ws_s, int H, int64_t* __restrict__ best,
    float* __restrict__ cand_R, float* __restrict__ cand_T, float* __restrict__ cand_s) {
  const int n = blockIdx.x;
  const int64_t b = cs_best(tile_keys, tiles, n);
  if (threadIdx.x != 0) return;
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
__global__ __launch_bounds__(kCsBlock) void ransac_evaluate_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ corr,
    const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2, const int64_t* __restrict__ best,
    const float* __restrict__ cand_R, const float* __restrict__ cand_T, const float* __restrict__ cand_s, int P1,
    int P2, float thr2, uint8_t* __restrict__ cand_mask, double* __restrict__ part_sum, int* __restrict__ part_count) {
  const int n = blockIdx.y, nb = gridDim.x;
  const int len1 = clamped_length(lengths1, n, P1), len2 = clamped_length(lengths2, n, P2);
  const bool none = best[n] < 0;
  float A[3][3], T[3];
  rs_load_transform(cand_R, cand_T, cand_s, n, A, T);
  const float* __restrict__ xs = X + (int64_t)n * P1 * 3;
  const float* __restrict__ ys = Y + (int64_t)n * P2 * 3;
  double sum[1] = {0.0};
  int cnt = 0;
  for (int i = blockIdx.x * kCsBlock + (int)threadIdx.x; i < P1; i += nb * kCsBlock) {
    const int j = none ? -1 : rs_target(corr, n, P1, i, len1, len2);
    bool in = false;
    if (j >= 0) {
      const float d2 = rh_residual(A, T, xs[(int64_t)i * 3], xs[(int64_t)i * 3 + 1], xs[(int64_t)i * 3 + 2],
                                   ys[(int64_t)j * 3], ys[(int64_t)j * 3 + 1], ys[(int64_t)j * 3 + 2]);
      in = d2 <= thr2;
      if (in) sum[0] += (double)d2;
    }
    cnt += in ? 1 : 0;
    cand_mask[(int64_t)n * P1 + i] = in ? 1 : 0;
  }
  const int64_t slot = (int64_t)n * nb + blockIdx.x;
  cs_block_partials(sum, cnt, nb, part_sum + slot, part_count + slot);
}

// One block per cloud: the accept rule and -- on acceptance -- the public transform, mask, count and rmse, and the 0/1
// weights of the next fit.
__global__ __launch_bounds__(kCsBlock) void ransac_finish_kernel(
    const double* __restrict__ part_sum, const int* __restrict__ part_count, int nb, int first,
    const int64_t* __restrict__ best, const float* __restrict__ cand_R, const float* __restrict__ cand_T,
    const float* __restrict__ cand_s, const uint8_t* __restrict__ cand_mask, int P1, int* __restrict__ stopped,
    float* __restrict__ R, float* __restrict__ T, float* __restrict__ s, uint8_t* __restrict__ mask,
    float* __restrict__ weights, int64_t* __restrict__ num_inliers, float* __restrict__ rmse) {
  const int n = blockIdx.x;
  int cnt;
  double sum;
  if (!cs_accept(part_sum + (int64_t)n * nb, part_count, nb, n, first, true, stopped, num_inliers, cnt, sum)) return;
  if (threadIdx.x == 0) {
    cs_publish(n, first, best, cnt, sum, stopped, num_inliers, rmse);
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
    for (int i = threadIdx.x; i < P1 / 4; i += kCsBlock) {
      const uchar4 m = src[i];
      dst[i] = m;
      w[i] = make_float4(m.x ? 1.0f : 0.0f, m.y ? 1.0f : 0.0f, m.z ? 1.0f : 0.0f, m.w ? 1.0f : 0.0f);
    }
    return;
  }
  for (int i = threadIdx.x; i < P1; i += kCsBlock) {
    const uint8_t m = cand_mask[(int64_t)n * P1 + i];
    mask[(int64_t)n * P1 + i] = m;
    weights[(int64_t)n * P1 + i] = m ? 1.0f : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------ host side
struct RansacLayout : CsLayout {  // (num_valid: the pairs of a cloud)
  RansacRecord* records;  // (N, P1)
  float *hyp_R, *hyp_T, *hyp_s;  // (N, H, 9 | 3 | 1)
  float *cand_R, *cand_T, *cand_s;  // (N, 9 | 3 | 1)
  uint8_t* cand_mask;     // (N, P1)
  float* weights;         // (N, P1)
  double* part_sum;       // (N, nb)
  void* alignment;        // pointops_points_alignment's own
  size_t alignment_bytes;
  size_t bytes;
};

static RansacLayout ransac_layout(void* ws, int64_t N, int64_t P1, int64_t H) {
  Carver c(ws);
  RansacLayout l;
  static_cast<CsLayout&>(l) = cs_layout(c, N, P1, H, kRansacChunk);
  const size_t n = (size_t)N, p = (size_t)P1, h = (size_t)H;
  l.records = (RansacRecord*)c.take(sizeof(RansacRecord) * n * p);
  l.hyp_R = (float*)c.take(sizeof(float) * n * h * 9);
  l.hyp_T = (float*)c.take(sizeof(float) * n * h * 3);
  l.hyp_s = (float*)c.take(sizeof(float) * n * h);
  l.cand_R = (float*)c.take(sizeof(float) * n * 9);
  l.cand_T = (float*)c.take(sizeof(float) * n * 3);
  l.cand_s = (float*)c.take(sizeof(float) * n);
  l.cand_mask = (uint8_t*)c.take(n * p);
  l.weights = (float*)c.take(sizeof(float) * n * p);
  l.part_sum = (double*)c.take(sizeof(double) * n * (size_t)cs_eval_blocks(P1));
  l.alignment_bytes = pointops_points_alignment_workspace_bytes(N, P1, 3);
  l.alignment = c.take(l.alignment_bytes);
  l.bytes = c.off;
  return l;
}

static bool ransac_shape_ok(int64_t N, int64_t P1, int64_t P2, int64_t H) {
  return cs_shape_ok(N, P1, H, kRansacChunk) && P2 >= 0 && P2 < (1LL << 30);
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
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "ransac_alignment: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  const float thr2 = inlier_threshold * inlier_threshold;
  const float q = edge_length_ratio * edge_length_ratio;
  const int edge_test = (!estimate_scale && edge_length_ratio > 0.0f) ? 1 : 0;
  const CsGrid g(N, P1, H, kRansacChunk);
  const dim3 block(kCsBlock);

  cs_launch_compact(RansacPairs{X, Y, corr, lengths1, lengths2, (int)P1, (int)P2, 0, 0}, g, l, P1, l.records, stream);
  hipLaunchKernelGGL(ransac_hypotheses_kernel, g.hyp, block, 0, stream, X, Y, corr, lengths1, lengths2, samples_in,
                     (int)P1, (int)P2, (int)H, seed, first_cloud, q, edge_test, estimate_scale,
                     (const RansacRecord*)l.records, (const int*)l.num_valid, l.hyp_R, l.hyp_T, l.hyp_s, l.hyp_valid,
                     hyp_R, hyp_T, hyp_s, samples_out);
  if (g.S > 0) {
    auto* score = debug_knob("ransac_lds", 0) ? ransac_score_kernel<true> : ransac_score_kernel<false>;
    hipLaunchKernelGGL(score, dim3(g.tiles, g.S, (unsigned)N), block, 0, stream, (const RansacRecord*)l.records,
                       (const int*)l.num_valid, (const float*)l.hyp_R, (const float*)l.hyp_T, (const float*)l.hyp_s,
                       (const int*)l.hyp_valid, (int)P1, (int)H, (int)g.S, thr2, l.partials);
  }
  cs_launch_count<kRansacChunk>(g, l, H, counts, stream);
  hipLaunchKernelGGL(ransac_select_kernel, g.cloud, block, 0, stream, (const unsigned long long*)l.tile_keys,
                     (int)g.tiles, (const float*)l.hyp_R, (const float*)l.hyp_T, (const float*)l.hyp_s, (int)H, best,
                     l.cand_R, l.cand_T, l.cand_s);
  int rc = check_launch("ransac_alignment");
  const int refits = P1 == 0 ? 0 : refine_steps;  // (no row, nothing to refit)
  for (int step = 0; step <= refits && rc == POINTOPS_OK; ++step) {
    if (step > 0) {
      rc = pointops_points_alignment(X, Y, corr, lengths1, l.weights, N, P1, P2, 3, estimate_scale, 0, 1e-9, l.cand_R,
                                     l.cand_T, l.cand_s, nullptr, nullptr, l.alignment, l.alignment_bytes, stream_);
      if (rc != POINTOPS_OK) return rc;
    }
    hipLaunchKernelGGL(ransac_evaluate_kernel, g.eval, block, 0, stream, X, Y, corr, lengths1, lengths2,
                       (const int64_t*)best, (const float*)l.cand_R, (const float*)l.cand_T, (const float*)l.cand_s,
                       (int)P1, (int)P2, thr2, l.cand_mask, l.part_sum, l.part_count);
    hipLaunchKernelGGL(ransac_finish_kernel, g.cloud, block, 0, stream, (const double*)l.part_sum,
                       (const int*)l.part_count, g.nb, step == 0 ? 1 : 0, (const int64_t*)best, (const float*)l.cand_R,
                       (const float*)l.cand_T, (const float*)l.cand_s, (const uint8_t*)l.cand_mask, (int)P1, l.stopped,
                       R, T, s, inlier_mask, l.weights, num_inliers, rmse);
    rc = check_launch("ransac_alignment");
  }
  return rc;
}

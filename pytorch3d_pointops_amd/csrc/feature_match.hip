// feature_match.hip -- the nearest one or two rows of a descriptor table for every row of another (C ABI:
// pointops_feature_knn, pointops_feature_screen_values; device half of functions/match.py).  The definition is the
// FEATURE MATCHING block of include/pointops_amd.h; the scalar definitions of the screen, its error bound and the
// certificate are feature_screen.h, which the host tests compile alone.
//
// The results are pointops_knn_points_idx's, byte for byte.  That search (knn_wide.hip for D > 8) spends a subtract, a
// multiply and an add per pair and coordinate on the vector ALU because the reference's sum is unfused.  The screen
// spends one fused multiply-add per pair and coordinate on the matrix cores instead, to ORDER the targets, and the
// unfused sum only on the few targets that can be among the nearest:
//   prologue  feature_norms_kernel: n1, n2 (fmaf chains) and the per-cloud n2max (integer atomicMax on the bits of a
//             non-negative float: order-independent; a NaN or +inf norm wins it, which marks the cloud)
//   screen    feature_screen_kernel<DH>: a wave owns 32 queries, on the COLUMN side of v_mfma_f32_32x32x2_f32, whose
//             fragment (B[k = 2 kk + (lane >> 5)][j = lane & 31]) stays in DH = ceil(D / 2) registers for the whole scan.
//             Targets stream through an LDS tile of 64 rows with an odd row stride (2 DH + 1 words): the A operand
//             read A[i = lane & 31][k = 2 kk + (lane >> 5)] puts the 32 lanes of a half wave on 32 different banks.
//             The accumulator lane (j, h) holds query j and the 16 targets i = (reg & 3) + 8 (reg >> 2) + 4 h of the
//             block, in ascending order of reg: it forms s from n1, n2 and the accumulator and offers (s, i) to a sorted
//             register list of M = 8 keys (TopK of knn_common.h: candidates arrive in index order and displace on
//             strict <, which is the (s, index) order).  No cross-lane step until the end.
//   rescore   in the same kernel: each of the two lanes of a query computes the exact distance of its 8 targets in the
//             reference's order, keeps its two smallest (r, j), and one exchange across the half waves merges them.
//   decide    lane h = 0 evaluates the certificate (screen_certified) and writes the row, or appends the query to the
//             cloud's list (integer atomicAdd: the ORDER of the list varies, no result depends on it).
//   fallback  launch_knn_wide in its qlist / qcount mode over the listed rows: always enqueued, ends on the count.
//   stats     feature_stats_kernel writes the per-cloud counts.
// A fixed sequence of one memset node and four launches on the caller's stream; nothing is read back.
#include <limits.h>

#include "debug.h"
#include "feature_screen.h"
#include "knn_common.h"
#include "knn_grid.h"

namespace pointops {

constexpr int kMatchMaxDim = 128;   // the query fragment's register budget: 64 VGPRs
constexpr int kMatchTile = 64;      // targets per LDS tile: two 32 x 32 blocks
constexpr Ints<2, 8, 16, 17, 32, 64> kMatchDH{};  // k-steps of the instances (D <= 4, 16, 32, 34, 64, 128)

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void feature_norms_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                            const int64_t* __restrict__ lengths2, int P1, int P2, int D,
                                                            int64_t total, float* __restrict__ n1, float* __restrict__ n2,
                                                            unsigned* __restrict__ n2max) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int64_t rows = (int64_t)P1 + P2;
  const int n = (int)(t / rows);
  const int64_t r = t - (int64_t)n * rows;
  if (r < P1) {
    const int64_t row = (int64_t)n * P1 + r;
    n1[row] = screen_norm(p1 + row * D, D);
  } else {
    const int64_t j = r - P1, row = (int64_t)n * P2 + j;
    const float v = screen_norm(p2 + row * D, D);
    n2[row] = v;
    if (j < clamped_length<int64_t>(lengths2, n, P2)) atomicMax(n2max + n, __float_as_uint(v));
  }
}

__device__ __forceinline__ bool pair_less(float ra, int ja, float rb, int jb) {
  return ra < rb || (ra == rb && ja < jb);
}

// Workgroups of 64 or 256 lanes (blockDim.x): 32 queries per wave.  `idxs` null: the introspection entry (nothing is
// written but s_out / E_out).
template <int DH>
__global__ __launch_bounds__(256) void feature_screen_kernel(
    const float* __restrict__ p1, const float* __restrict__ p2, const int64_t* __restrict__ lengths1,
    const int64_t* __restrict__ lengths2, int P1, int P2, int D, int K, int tiles_per_cloud,
    const float* __restrict__ n1, const float* __restrict__ n2, const unsigned* __restrict__ n2max,
    int* __restrict__ qlist, int* __restrict__ qcount, int64_t* __restrict__ idxs, float* __restrict__ dists,
    float* __restrict__ s_out, float* __restrict__ E_out) {
  constexpr int STRIDE = 2 * DH + 1;
  __shared__ float s_t[kMatchTile * STRIDE];
  __shared__ float s_n2[kMatchTile];
  const int n = blockIdx.x / tiles_per_cloud;  // wave-uniform
  const int tile = blockIdx.x - n * tiles_per_cloud;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  const int q = (tile * ((int)blockDim.x >> 6) + wave) * 32 + c;
  const int len1 = clamped_length<int>(lengths1, n, P1), len2 = clamped_length<int>(lengths2, n, P2);
  const bool qin = q < P1;
  const float* __restrict__ a = p1 + ((int64_t)n * P1 + (qin ? q : 0)) * D;
  const float* __restrict__ tgt = p2 + (int64_t)n * P2 * D;

  float bq[DH];  // B[k = 2 kk + h][j = c]
#pragma unroll
  for (int kk = 0; kk < DH; ++kk) {
    const int k = 2 * kk + h;
    bq[kk] = (qin && k < D) ? a[k] : 0.0f;
  }
  const float n1q = qin ? n1[(int64_t)n * P1 + q] : 0.0f;

  for (int f = tid; f < kMatchTile * STRIDE; f += (int)blockDim.x) s_t[f] = 0.0f;  // (the columns past D stay zero)
  __syncthreads();

  TopK<kScreenM> top;
  top.init();
  // element f = tid + m blockDim of a tile is (row, d) = (f / D, f % D): stepped without a division per element
  const int step_r = (int)blockDim.x / D, step_d = (int)blockDim.x - step_r * D;
  for (int t0 = 0; t0 < len2; t0 += kMatchTile) {
    const int rows = min(kMatchTile, len2 - t0);
    {
      const float* __restrict__ src = tgt + (int64_t)t0 * D;
      int row = tid / D, d = tid - row * D;
      while (row < kMatchTile) {
        s_t[row * STRIDE + d] = row < rows ? src[row * D + d] : 0.0f;
        row += step_r;
        d += step_d;
        if (d >= D) {
          d -= D;
          ++row;
        }
      }
      if (tid < kMatchTile) s_n2[tid] = tid < rows ? n2[(int64_t)n * P2 + t0 + tid] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int blk = 0; blk < kMatchTile / 32; ++blk) {
      if (blk * 32 < rows) {  // (workgroup-uniform)
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float* __restrict__ arow = s_t + (blk * 32 + c) * STRIDE + h;  // A[i = c][k = 2 kk + h]
#pragma unroll
        for (int kk = 0; kk < DH; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * kk], bq[kk], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int trow = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const int j = t0 + trow;
          const float s = screen_value(n1q, s_n2[trow], acc[r]);
          if (j < len2) {
            if (s < top.worst()) top.insert(s, j);
            if (s_out != nullptr && q < len1) s_out[((int64_t)n * P1 + q) * P2 + j] = s;
          }
        }
      }
    }
    __syncthreads();
  }

  // exact distances of this lane's collected targets (a filled slot holds a key below +inf); its two smallest (r, j)
  float r0 = __builtin_inff(), r1 = __builtin_inff();
  int j0 = INT_MAX, j1 = INT_MAX;
  if (idxs != nullptr) {
#pragma unroll
    for (int k = 0; k < kScreenM; ++k) {
      if (qin && top.dk[k] < __builtin_inff()) {
        const int j = top.ik[k];
        const float r = exact_distance(a, tgt + (int64_t)j * D, D);
        if (pair_less(r, j, r0, j0)) {
          r1 = r0, j1 = j0;
          r0 = r, j0 = j;
        } else if (pair_less(r, j, r1, j1)) {
          r1 = r, j1 = j;
        }
      }
    }
  }
  // the other half wave's lane of the same query
  const float pr0 = __shfl_xor(r0, 32), pr1 = __shfl_xor(r1, 32);
  const int pj0 = __shfl_xor(j0, 32), pj1 = __shfl_xor(j1, 32);
  const float s_cut = fminf(top.worst(), __shfl_xor(top.worst(), 32));
  if (h != 0 || !qin) return;
  // (r0, j0) <= (r1, j1) and (pr0, pj0) <= (pr1, pj1): the two smallest of the four
  float b0, b1;
  int i0, i1;
  if (pair_less(pr0, pj0, r0, j0)) {
    b0 = pr0, i0 = pj0;
    const bool second_theirs = pair_less(pr1, pj1, r0, j0);
    b1 = second_theirs ? pr1 : r0, i1 = second_theirs ? pj1 : j0;
  } else {
    b0 = r0, i0 = j0;
    const bool second_theirs = pair_less(pr0, pj0, r1, j1);
    b1 = second_theirs ? pr0 : r1, i1 = second_theirs ? pj0 : j1;
  }
  const bool live = q < len1 && len2 > 0;
  const float n2m = __uint_as_float(n2max[n]);
  const float E = live ? screen_bound(D, n1q, n2m) : 0.0f;
  if (E_out != nullptr) E_out[(int64_t)n * P1 + q] = E;
  if (idxs == nullptr) return;
  const int64_t row = (int64_t)n * P1 + q;
  if (live && !screen_certified(D, n1q, n2m, len2, K == 1 ? b0 : b1, E, s_cut)) {
    qlist[(int64_t)n * P1 + atomicAdd(qcount + n, 1)] = q;
    return;
  }
  const int kvalid = live ? min(K, len2) : 0;
  idxs[row * K] = kvalid > 0 ? (int64_t)i0 : 0;
  dists[row * K] = kvalid > 0 ? b0 : 0.0f;
  if (K > 1) {
    idxs[row * K + 1] = kvalid > 1 ? (int64_t)i1 : 0;
    dists[row * K + 1] = kvalid > 1 ? b1 : 0.0f;
  }
}

__global__ __launch_bounds__(256) void feature_stats_kernel(const int64_t* __restrict__ lengths1,
                                                            const int64_t* __restrict__ lengths2, int P1, int P2, int N,
                                                            const int* __restrict__ qcount, int32_t* __restrict__ stats) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int live = clamped_length<int>(lengths2, n, P2) > 0 ? clamped_length<int>(lengths1, n, P1) : 0;
  const int listed = qcount != nullptr ? qcount[n] : 0;
  stats[4 * n] = qcount != nullptr ? 1 : 0;
  stats[4 * n + 1] = qcount != nullptr ? live - listed : 0;
  stats[4 * n + 2] = listed;
  stats[4 * n + 3] = 0;
}

static bool match_shape_ok(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  return N >= 0 && N < (1LL << 31) && P1 >= 0 && P1 < (1LL << 31) && P2 >= 0 && P2 < (1LL << 31) && D >= 1 &&
         D < (1LL << 16) && K >= 1 && K <= 2;
}

// Default dispatch, from profiles/match_bench.jsonl (MI355X, search alone, exact over screen): the screen wins at
// 8 x 65536 rows (1.84x at D = 32, 1.57x at 33, 5.53x at 128) and at 16 x 131072 (1.7 - 1.8x), both on 256-lane
// workgroups, and loses at every measured shape of up to 16384 targets (0.28x - 0.60x; 8 x 4096 at D = 128 ties), all
// of which run 64-lane workgroups.  So a call takes the screen from the smallest target count at which it was measured
// faster, in the workgroup shape it was measured in; nothing between 16384 and 65536 targets has been timed, and such
// calls stay on the exact search.
constexpr int64_t kMatchMinTargets = 65536;
constexpr int kMatchMinDim = 9;          // D <= 8: the exact search has its register scan and its grid
constexpr int64_t kMatchWideGroups = 1024;  // 128-query workgroups from this many on: 256 lanes each
static bool match_uses_screen(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  if (N <= 0 || P1 <= 0 || P2 <= 0 || D > kMatchMaxDim || !knn_wide_supported(D, K)) return false;
  const long force = debug_knob("match_screen", -1);
  if (force == 0) return false;
  return force == 1 || (D >= kMatchMinDim && P2 >= kMatchMinTargets && N * ceil_div(P1, 128) >= kMatchWideGroups);
}

struct MatchLayout {
  char* knn;        // the exact search's own workspace
  float* n1;        // (N, P1)
  float* n2;        // (N, P2)
  unsigned* n2max;  // (N,) bits, then qcount (N,): one memset
  int* qcount;
  int* qlist;       // (N, P1)
  size_t knn_bytes, bytes;
};

// one layout for both paths: which one a call takes may depend on a debug knob, its workspace does not
static MatchLayout match_layout(void* ws, int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  Carver c(ws);
  MatchLayout l;
  l.knn_bytes = pointops_knn_workspace_bytes(N, P1, P2, D, K, -1);
  l.knn = c.take(l.knn_bytes);
  const bool screen = D <= kMatchMaxDim && knn_wide_supported(D, K);
  l.n1 = (float*)c.take(screen ? sizeof(float) * (size_t)(N * P1) : 0);
  l.n2 = (float*)c.take(screen ? sizeof(float) * (size_t)(N * P2) : 0);
  l.n2max = (unsigned*)c.take(screen ? sizeof(int) * 2 * (size_t)N : 0);
  l.qcount = l.n2max ? (int*)(l.n2max + N) : nullptr;
  l.qlist = (int*)c.take(screen ? sizeof(int) * (size_t)(N * P1) : 0);
  l.bytes = c.off;
  return l;
}

// the screen over every query: `wg` lanes per workgroup
static int launch_screen(const float* p1, const float* p2, const int64_t* l1, const int64_t* l2, int64_t N, int64_t P1,
                         int64_t P2, int64_t D, int64_t K, const float* n1, const float* n2, const unsigned* n2max,
                         int* qlist, int* qcount, int64_t* idxs, float* dists, float* s_out, float* E_out,
                         hipStream_t stream) {
  const int wg = N * ceil_div(P1, 128) >= kMatchWideGroups ? 256 : 64;  // a small batch: four times the workgroups
  const int64_t tiles = ceil_div(P1, wg / 2);
  POINTOPS_REQUIRE(N * tiles < (1LL << 31), "feature_knn: grid too large");
  with_bucket(kMatchDH, (int)ceil_div(D, 2), [&](auto DH) {
    hipLaunchKernelGGL(feature_screen_kernel<DH>, dim3((unsigned)(N * tiles)), dim3(wg), 0, stream, p1, p2, l1, l2,
                       (int)P1, (int)P2, (int)D, (int)K, (int)tiles, n1, n2, n2max, qlist, qcount, idxs, dists, s_out,
                       E_out);
  });
  return POINTOPS_OK;
}

static void launch_norms(const float* p1, const float* p2, const int64_t* l2, int64_t N, int64_t P1, int64_t P2, int64_t D,
                         float* n1, float* n2, unsigned* n2max, hipStream_t stream) {
  const int64_t total = N * (P1 + P2);
  hipLaunchKernelGGL(feature_norms_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream, p1, p2, l2,
                     (int)P1, (int)P2, (int)D, total, n1, n2, n2max);
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_feature_knn_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  if (!match_shape_ok(N, P1, P2, D, K) || N == 0 || P1 == 0) return 0;
  return match_layout(nullptr, N, P1, P2, D, K).bytes;
}

extern "C" int pointops_feature_knn(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                                    int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K, int64_t* idxs, float* dists,
                                    int32_t* stats, void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(match_shape_ok(N, P1, P2, D, K),
                   "feature_knn: need 0 <= N, P1, P2 < 2^31, 1 <= D < 2^16 and K in {1, 2}");
  if (N == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE(lengths1 && lengths2 && stats, "feature_knn: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  if (P1 == 0) {
    hipLaunchKernelGGL(feature_stats_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, stream, lengths1, lengths2,
                       (int)P1, (int)P2, (int)N, (const int*)nullptr, stats);
    return check_launch("feature_knn");
  }
  POINTOPS_REQUIRE(p1 && idxs && dists && (p2 || P2 == 0), "feature_knn: null pointer");
  const MatchLayout l = match_layout(workspace, N, P1, P2, D, K);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "feature_knn: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  if (!match_uses_screen(N, P1, P2, D, K)) {
    const int rc = pointops_knn_points_idx(p1, p2 ? p2 : p1, lengths1, lengths2, N, P1, P2, D, 2, K, -1, idxs, dists,
                                           l.knn, l.knn_bytes, stream_);
    if (rc != POINTOPS_OK) return rc;
    hipLaunchKernelGGL(feature_stats_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, stream, lengths1, lengths2,
                       (int)P1, (int)P2, (int)N, (const int*)nullptr, stats);
    return check_launch("feature_knn");
  }
  if (hipMemsetAsync(l.n2max, 0, sizeof(int) * 2 * (size_t)N, stream) != hipSuccess) return check_launch("feature_knn");
  launch_norms(p1, p2, lengths2, N, P1, P2, D, l.n1, l.n2, l.n2max, stream);
  int rc = launch_screen(p1, p2, lengths1, lengths2, N, P1, P2, D, K, l.n1, l.n2, l.n2max, l.qlist, l.qcount, idxs,
                         dists, nullptr, nullptr, stream);
  if (rc != POINTOPS_OK) return rc;
  KnnArgs a = make_knn_args(p1, p2, lengths1, lengths2, N, P1, P2, D, K, (int)ceil_div(P1, kKnnBlock), idxs, dists, stream);
  a.qlist = l.qlist;
  a.qcount = l.qcount;
  rc = launch_knn_wide(a, 2, 1, nullptr);  // the listed rows, whole clouds (no p2 slices: they would write every row)
  if (rc != POINTOPS_OK) return rc;
  hipLaunchKernelGGL(feature_stats_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, stream, lengths1, lengths2,
                     (int)P1, (int)P2, (int)N, (const int*)l.qcount, stats);
  return check_launch("feature_knn");
}

extern "C" int pointops_feature_screen_values(const float* p1, const float* p2, const int64_t* lengths1,
                                              const int64_t* lengths2, int64_t N, int64_t P1, int64_t P2, int64_t D,
                                              float* s, float* n1, float* n2, float* n2max, float* E, void* stream_) {
  POINTOPS_REQUIRE(N >= 0 && N < 65536 && P1 >= 1 && P1 <= 1024 && P2 >= 1 && P2 <= 1024 && D >= 1 && D <= kMatchMaxDim,
                   "feature_screen_values: need 0 <= N < 65536, 1 <= P1, P2 <= 1024 and 1 <= D <= %d", kMatchMaxDim);
  if (N == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE(p1 && p2 && lengths1 && lengths2 && s && n1 && n2 && n2max && E, "feature_screen_values: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  if (hipMemsetAsync(s, 0, sizeof(float) * (size_t)(N * P1 * P2), stream) != hipSuccess ||
      hipMemsetAsync(n2max, 0, sizeof(float) * (size_t)N, stream) != hipSuccess)
    return check_launch("feature_screen_values");
  launch_norms(p1, p2, lengths2, N, P1, P2, D, n1, n2, (unsigned*)n2max, stream);
  const int rc = launch_screen(p1, p2, lengths1, lengths2, N, P1, P2, D, 1, n1, n2, (const unsigned*)n2max, nullptr,
                               nullptr, nullptr, nullptr, s, E, stream);
  if (rc != POINTOPS_OK) return rc;
  return check_launch("feature_screen_values");
}

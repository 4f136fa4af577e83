// feature_topk.hip -- the K nearest rows of a descriptor table for every row of another, K <= 32 on the MFMA screen
// (C ABI: pointops_feature_topk; device half of functions/knn_features.py).  The definition is the FEATURE TOP-K block
// of include/pointops_amd.h; the list geometry, the merge and the certificate are feature_topk.h, the screen value and
// its error bound feature_screen.h, which the host tests compile alone.
//
// The results are pointops_knn_points_idx's, byte for byte.  feature_match.hip has the idea (order the targets by the
// product form of the distance on the matrix cores, spend the reference's unfused sum only on the collected targets,
// certify each row, send the rest through the exact kernel); this file gives it the geometry that K <= 32 and small
// batches need:
//   split     a 256-lane workgroup of 4 waves owns 128 / S queries, S in {1, 4}.  Wave w holds the fragment of query
//             group w / S (32 queries, on the COLUMN side of v_mfma_f32_32x32x2_f32, DH = ceil(D / 2) registers) and
//             takes the 32-row target blocks b with b mod S = w mod S.  S = 1: a tile is reused by 128 queries.  S = 4:
//             the same queries get four times the waves -- what a small batch lacks.
//   tile      128 target rows in LDS, odd row stride 2 DH + 1 words (the A operand read of a half wave hits 32 banks);
//             every wave reads every tile.
//   lists     the accumulator lane (query j, half h) of wave w offers its 16 targets of a block, in index order, to a
//             sorted register list of M = 16 keys: list t = 2 (w mod S) + h of the query (topk_list_of).
//   rescore   each lane computes exact_distance of its <= 16 targets, sorts the (r bits, j) keys in registers (the
//             60-comparator network on the FP64 pipe, sort_net.h) and writes them into the LDS the tile occupied,
//             key-major so that the lanes of a half wave write consecutive words.
//   merge     one lane per query merges its 2 S lists for the first K keys (topk_merge), reads r_K and s_cut, and
//             evaluates the certificate (topk_certified); an uncertified row is appended to the cloud's list (integer
//             atomicAdd: the ORDER of the list varies, no result depends on it).
//   store     the merged rows of a workgroup are one contiguous span of the outputs: all 256 lanes write it from LDS,
//             skipping the listed rows.
//   fallback  launch_knn_wide in its qlist / qcount mode over the listed rows: always enqueued, ends on the count.
// A fixed sequence of five launches on the caller's stream (clear, norms, screen, fallback, stats); nothing is read back.
#include <limits.h>

#include "debug.h"
#include "feature_match.h"
#include "feature_topk.h"
#include "knn_common.h"
#include "knn_grid.h"
#include "sort_net.h"

namespace pointops {

constexpr int kTopkMaxDim = 128;  // the query fragment's register budget: 64 VGPRs
constexpr int kTopkTile = 128;    // targets per LDS tile: four 32 x 32 blocks
constexpr int kTopkWg = 256;
constexpr Ints<8, 16, 17, 32, 64> kTopkDH{};  // k-steps of the instances (D <= 16, 32, 34, 64, 128)

// LDS of the tail (bytes from the start; the tile and its norms occupy the same memory during the scan)
constexpr int kTopkLdsLists = kTopkM * 2 * 128 * 8;      // 2 S lists x 128 / S queries x M keys
constexpr int kTopkLdsCut = kTopkLdsLists;               // the M-th screen key of every list: 2 S x 128 / S floats
constexpr int kTopkLdsFlag = kTopkLdsCut + 2 * 128 * 4;  // one int per query
constexpr int kTopkLdsOut = kTopkLdsFlag + 128 * 4;      // the merged keys: 128 / S x K
constexpr size_t kTopkLdsMax = 68 * 1024;                // above the largest instance (DH = 64; S = 1 at K = 32)

static size_t topk_lds_bytes(int DH, int S, int64_t K) {
  const size_t scan = sizeof(float) * (size_t)(kTopkTile * (2 * DH + 1) + kTopkTile);
  const size_t tail = (size_t)kTopkLdsOut + (size_t)(128 / S) * (size_t)K * 8;
  return scan > tail ? scan : tail;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void feature_topk_clear_kernel(unsigned* __restrict__ words, int64_t count) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < count) words[t] = 0u;
}

// rows [t0, t0 + rows) of a cloud into the tile (rows past `rows` as zeros) and their norms; element f = tid + m 256 of a
// tile is (row, d) = (f / D, f % D), stepped without a division per element
template <int STRIDE>
__device__ __forceinline__ void topk_load_tile(float* __restrict__ s_t, float* __restrict__ s_n2,
                                               const float* __restrict__ src, const float* __restrict__ n2, int rows,
                                               int D, int tid) {
  const int step_r = kTopkWg / D, step_d = kTopkWg - step_r * D;
  int row = tid / D, d = tid - row * D;
  while (row < kTopkTile) {
    s_t[row * STRIDE + d] = row < rows ? src[row * D + d] : 0.0f;
    row += step_r;
    d += step_d;
    if (d >= D) {
      d -= D;
      ++row;
    }
  }
  if (tid < kTopkTile) s_n2[tid] = tid < rows ? n2[tid] : 0.0f;
}

// one 32 x 32 block: g = the k-ordered fmaf chain over the DH steps; A[i = c][k = 2 kk + h] from the tile row,
// B[k = 2 kk + h][j = c] from the lane's fragment
template <int DH>
__device__ __forceinline__ f32x16 topk_mfma_block(const float* __restrict__ arow, const float (&bq)[DH]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int kk = 0; kk < DH; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * kk], bq[kk], acc, 0, 0, 0);
  return acc;
}

// the lane's 16 targets of a block, rows (r & 3) + 8 (r >> 2) + 4 h in ascending order of r, offered to its list
__device__ __forceinline__ void topk_offer_block(TopK<kTopkM>& top, const f32x16& acc, const float* __restrict__ s_n2,
                                                 float n1q, int row0, int h, int j0, int len2) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int trow = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
    const int j = j0 + trow;
    const float s = screen_value(n1q, s_n2[trow], acc[r]);
    if (j < len2 && s < top.worst()) top.insert(s, j);
  }
}

template <int DH, int S>
__global__ __launch_bounds__(256) void feature_topk_kernel(
    const float* __restrict__ p1, const float* __restrict__ p2, const int64_t* __restrict__ lengths1,
    const int64_t* __restrict__ lengths2, int P1, int P2, int D, int K, int tiles_per_cloud,
    const float* __restrict__ n1, const float* __restrict__ n2, const unsigned* __restrict__ n2max,
    int* __restrict__ qlist, int* __restrict__ qcount, int64_t* __restrict__ idxs, float* __restrict__ dists) {
  constexpr int STRIDE = 2 * DH + 1, LISTS = 2 * S, QPG = 128 / S;
  extern __shared__ double s_topk[];  // (8-byte aligned: the keys)
  float* s_t = (float*)s_topk;
  float* s_n2 = s_t + kTopkTile * STRIDE;
  const int n = blockIdx.x / tiles_per_cloud;  // wave-uniform
  const int tile = blockIdx.x - n * tiles_per_cloud;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  const int sub = wave % S;            // which blocks of a tile this wave takes
  const int ql = (wave / S) * 32 + c;  // the query within the workgroup
  const int q = tile * QPG + ql;
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

  for (int f = tid; f < kTopkTile * STRIDE; f += kTopkWg) s_t[f] = 0.0f;  // (the columns past D stay zero)
  __syncthreads();

  TopK<kTopkM> top;
  top.init();
  for (int t0 = 0; t0 < len2; t0 += kTopkTile) {
    const int rows = min(kTopkTile, len2 - t0);
    topk_load_tile<STRIDE>(s_t, s_n2, tgt + (int64_t)t0 * D, n2 + (int64_t)n * P2 + t0, rows, D, tid);
    __syncthreads();
#pragma unroll
    for (int blk = 0; blk < kTopkTile / 32; ++blk) {
      if (blk % S == sub && blk * 32 < rows) {  // (wave-uniform)
        const f32x16 acc = topk_mfma_block<DH>(s_t + (blk * 32 + c) * STRIDE + h, bq);
        topk_offer_block(top, acc, s_n2, n1q, blk * 32, h, t0, len2);
      }
    }
    __syncthreads();
  }

  // the reference's distance of this lane's collected targets (a filled slot holds a key below +inf), sorted by (r, j)
  const bool live = q < len1 && len2 > 0;
  double key[kTopkM];
#pragma unroll
  for (int k = 0; k < kTopkM; ++k) {
    key[k] = __hiloint2double(0x7f800000, 0x7fffffff);
    if (live && top.dk[k] < __builtin_inff()) {
      const int j = top.ik[k];
      key[k] = __hiloint2double(__float_as_int(exact_distance(a, tgt + (int64_t)j * D, D)), j);
    }
  }
  bitonic_sort(key);

  // (the scan's last barrier is behind every read of the tile)
  double* s_keys = s_topk;                                 // [k][t][ql]
  float* s_cut = (float*)((char*)s_topk + kTopkLdsCut);    // [t][ql]
  int* s_flag = (int*)((char*)s_topk + kTopkLdsFlag);      // [ql]: 0 nothing to store, 1 a row of zeros, 2 the merged row
  unsigned long long* s_out = (unsigned long long*)((char*)s_topk + kTopkLdsOut);  // [ql][K]
  const int t = 2 * sub + h;
#pragma unroll
  for (int k = 0; k < kTopkM; ++k) s_keys[(k * LISTS + t) * QPG + ql] = key[k];
  s_cut[t * QPG + ql] = top.worst();
  __syncthreads();

  if (sub == 0 && h == 0) {  // one lane per query
    int flag = 0;
    if (qin) {
      flag = 1;
      if (live) {
        float cut = __builtin_inff();
#pragma unroll
        for (int u = 0; u < LISTS; ++u) cut = fminf(cut, s_cut[u * QPG + ql]);
        const unsigned long long* keys = (const unsigned long long*)s_keys;
        unsigned long long* out = s_out + ql * K;
        const float rK = topk_merge<LISTS>(
            K, [&](int u, int k) { return (uint64_t)keys[(k * LISTS + u) * QPG + ql]; },
            [&](int k, uint64_t v) { out[k] = v; });
        const float n2m = __uint_as_float(n2max[n]);
        flag = 2;
        if (!topk_certified(D, n1q, n2m, len2, rK, screen_bound(D, n1q, n2m), cut)) {
          qlist[(int64_t)n * P1 + atomicAdd(qcount + n, 1)] = q;
          flag = 0;
        }
      }
    }
    s_flag[ql] = flag;
  }
  __syncthreads();

  // rows tile QPG .. of the cloud are one span of idxs and of dists
  const int kvalid = min(K, len2);
  const int64_t base = ((int64_t)n * P1 + (int64_t)tile * QPG) * K;
  for (int e = tid; e < QPG * K; e += kTopkWg) {
    const int qe = e / K, k = e - qe * K;
    const int flag = s_flag[qe];
    if (flag == 0) continue;
    const bool ok = flag == 2 && k < kvalid;
    const unsigned long long v = ok ? s_out[e] : 0ull;
    idxs[base + e] = (int64_t)(unsigned)v;
    dists[base + e] = __uint_as_float((unsigned)(v >> 32));
  }
}

static bool topk_shape_ok(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  return N >= 0 && N < (1LL << 31) && P1 >= 0 && P1 < (1LL << 31) && P2 >= 0 && P2 < (1LL << 31) && D >= 1 &&
         D < (1LL << 16) && K >= 1 && K < (1LL << 31);
}

// the shapes the screen can take at all: the range of knn_wide's register-list instances, its fallback
static bool topk_screen_possible(int64_t D, int64_t K) {
  return D <= kTopkMaxDim && K <= kTopkMaxK && knn_wide_supported(D, K);
}

// Default dispatch, from profiles/feature_topk_bench.jsonl (MI355X, unit-norm rows, exact over screen, HIP-event medians
// of 5 alternated rounds, spread below 1 %): the screen is taken only where that table has it faster than the exact
// search by more than the spread, in the split it was measured in.
//   8 x 65536 rows  D = 64: 3.34x (K = 8), 1.57x (16), 1.36x (20), 1.04x (32);  D = 128: 3.64x, 1.93x, 1.06x, 1.06x;
//                   D = 32: 1.59x at K = 8, and 0.91x / 0.84x / 0.70x at K = 16 / 20 / 32
//   16 x 4096 and 32 x 1024 rows: 0.22x - 0.93x everywhere but D = 128, K = 8 at 16 x 4096 (1.51x, next to 0.64x at
//                   K = 16): one point is no range, these batches stay on the exact search
// So: at least 65536 targets and the 4096 groups of 128 queries of the measured batch; D >= 64 with 8 <= K <= 32, or
// D >= 32 with K = 8.  Everything else, K < 8 included (never timed; K <= 2 has feature_knn), is the exact search.
constexpr int64_t kTopkMinTargets = 65536;
constexpr int64_t kTopkMinGroups = 4096;
static bool topk_uses_screen(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  if (N <= 0 || P1 <= 0 || P2 <= 0 || !topk_screen_possible(D, K)) return false;
  const long force = debug_knob("topk_screen", -1);
  if (force == 0) return false;
  if (force == 1) return true;
  if (P2 < kTopkMinTargets || N * ceil_div(P1, 128) < kTopkMinGroups) return false;
  return D >= 64 ? K >= 8 : (D >= 32 && K == 8);
}

// S: K > 16 needs the 8 lists of S = 4 (two lists of 16 keys leave no room to certify 17 nearest).  Up to K = 16 the
// same table has S = 1 ahead of S = 4 at every shape, the small batches included (32 x 1024, D = 32, K = 8: 0.57 ms
// against 0.99 ms): four times the waves do not pay for a tile that serves a quarter of the queries.
static int topk_split(int64_t K) {
  const long force = debug_knob("topk_split", 0);
  if (force == 1 || force == 4) return (int)force;
  return K > kTopkM ? 4 : 1;
}

struct TopkLayout {
  char* knn;        // the exact search's own workspace
  float* n1;        // (N, P1)
  float* n2;        // (N, P2)
  unsigned* n2max;  // (N,) bits, then qcount (N,): one clear
  int* qcount;
  int* qlist;       // (N, P1)
  size_t knn_bytes, bytes;
};

// one layout for both paths: which one a call takes may depend on a debug knob, its workspace does not
static TopkLayout topk_layout(void* ws, int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  Carver c(ws);
  TopkLayout l;
  l.knn_bytes = pointops_knn_workspace_bytes(N, P1, P2, D, K, -1);
  l.knn = c.take(l.knn_bytes);
  const bool screen = topk_screen_possible(D, K);
  l.n1 = (float*)c.take(screen ? sizeof(float) * (size_t)(N * P1) : 0);
  l.n2 = (float*)c.take(screen ? sizeof(float) * (size_t)(N * P2) : 0);
  l.n2max = (unsigned*)c.take(screen ? sizeof(int) * 2 * (size_t)N : 0);
  l.qcount = l.n2max ? (int*)(l.n2max + N) : nullptr;
  l.qlist = (int*)c.take(screen ? sizeof(int) * (size_t)(N * P1) : 0);
  l.bytes = c.off;
  return l;
}

template <int DH, int S>
static int launch_topk(const KnnArgs& a, const TopkLayout& l) {
  auto kern = feature_topk_kernel<DH, S>;
  static bool attr_set[64] = {false};  // per instantiation and DEVICE (a process may drive several GPUs)
  int dev = -1;
  const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;  // (unknown: set it on every call)
  if (!known || !attr_set[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kTopkLdsMax) != hipSuccess)
      return check_launch("feature_topk(attribute)");
    if (known) attr_set[dev] = true;
  }
  const int64_t tiles = ceil_div(a.P1, 128 / S);
  POINTOPS_REQUIRE(a.N * tiles < (1LL << 31), "feature_topk: grid too large");
  const size_t lds = topk_lds_bytes(DH, S, a.K);
  POINTOPS_REQUIRE(lds <= kTopkLdsMax, "feature_topk: %zu bytes of LDS", lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.N * tiles)), dim3(kTopkWg), lds, a.stream, a.p1, a.p2, a.l1, a.l2, a.P1, a.P2,
                     a.D, a.K, (int)tiles, l.n1, l.n2, l.n2max, l.qlist, l.qcount, a.idxs, a.dists);
  return POINTOPS_OK;
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_feature_topk_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  if (!topk_shape_ok(N, P1, P2, D, K) || N == 0 || P1 == 0) return 0;
  return topk_layout(nullptr, N, P1, P2, D, K).bytes;
}

extern "C" int pointops_feature_topk(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                                     int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K, int64_t* idxs, float* dists,
                                     int32_t* stats, void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(topk_shape_ok(N, P1, P2, D, K), "feature_topk: need 0 <= N, P1, P2 < 2^31, 1 <= D < 2^16 and K >= 1");
  if (N == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE(lengths1 && lengths2 && stats, "feature_topk: null pointer");
  hipStream_t stream = (hipStream_t)stream_;
  if (P1 == 0) {
    launch_feature_stats(lengths1, lengths2, N, P1, P2, nullptr, 0, stats, stream);
    return check_launch("feature_topk");
  }
  POINTOPS_REQUIRE(p1 && idxs && dists && (p2 || P2 == 0), "feature_topk: null pointer");
  const TopkLayout l = topk_layout(workspace, N, P1, P2, D, K);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "feature_topk: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  if (!topk_uses_screen(N, P1, P2, D, K)) {
    const int rc = pointops_knn_points_idx(p1, p2 ? p2 : p1, lengths1, lengths2, N, P1, P2, D, 2, K, -1, idxs, dists,
                                           l.knn, l.knn_bytes, stream_);
    if (rc != POINTOPS_OK) return rc;
    launch_feature_stats(lengths1, lengths2, N, P1, P2, nullptr, 0, stats, stream);
    return check_launch("feature_topk");
  }
  // (a kernel, not a memset node: the sequence is the same eager and captured)
  hipLaunchKernelGGL(feature_topk_clear_kernel, dim3((unsigned)ceil_div(2 * N, 256)), dim3(256), 0, stream, l.n2max,
                     2 * N);
  launch_feature_norms(p1, p2, lengths2, N, P1, P2, D, l.n1, l.n2, l.n2max, stream);
  KnnArgs a = make_knn_args(p1, p2, lengths1, lengths2, N, P1, P2, D, K, (int)ceil_div(P1, kKnnBlock), idxs, dists, stream);
  const int S = topk_split(K);
  int rc = with_bucket(kTopkDH, (int)ceil_div(D, 2), [&](auto DH) {
    return S == 4 ? launch_topk<DH, 4>(a, l) : launch_topk<DH, 1>(a, l);
  });
  if (rc != POINTOPS_OK) return rc;
  a.qlist = l.qlist;
  a.qcount = l.qcount;
  rc = launch_knn_wide(a, 2, 1, nullptr);  // the listed rows, whole clouds (no p2 slices: they would write every row)
  if (rc != POINTOPS_OK) return rc;
  launch_feature_stats(lengths1, lengths2, N, P1, P2, l.qcount, 2 * S, stats, stream);
  return check_launch("feature_topk");
}

// fpfh.hip -- point-pair features, SPFH and FPFH descriptors of a neighbour table, in two fused passes.
//
// Device half of functions/fpfh.py; the definition is the comment block of pointops_spfh / pointops_fpfh in
// include/pointops_amd.h.  The torch composition it replaces materialises several (N,P,K,3) tensors, an atan2, three
// scatter_adds and a (N,P,K,33) gather; here the histogram of a point never leaves the workgroup.
//
// Pass 1 (spfh_kernel<G>): a workgroup of 256 lanes owns 256 / G consecutive points, G lanes per point striding over
// the slots k.  A lane gathers the neighbour's point and normal, computes (f1, f2, f3, d), writes them as one 16-byte
// store (optional output) and adds 1 to three of the point's 33 INTEGER counters in LDS (ds_add: integer adds commute,
// so the lane order cannot show).  After the barrier the workgroup's rows -- one contiguous run of 33 floats per
// point -- are scaled by 100 / m and stored coalesced.  G = 1 is the lane-per-point form (each lane walks its own
// index row, 128 B and more apart from its neighbour's); G = 8 reads a row's indices and writes its pair features as
// runs of 64 / 128 contiguous bytes.  The entry picks G = 8 from K >= 8 on (DESIGN.md has the measurement);
// POINTOPS_DEBUG="spfh_lanes=1|8" forces one (results do not depend on it).
//
// Pass 2 (fpfh_kernel): 7 points x 33 lanes per workgroup, lane = bin, so each gathered SPFH row (132 contiguous
// bytes) is one coalesced read and the 7 output rows one contiguous store.  The slots of the 7 points are resolved
// once into LDS (neighbour index or -1, and d2) instead of 33 times; the three group sums go through LDS in bin order.
// No atomics on global memory, no workspace, a fixed summation order.
#include "common.h"
#include "debug.h"
#include "small_solvers.h"

namespace pointops {

constexpr int kFpfhBins = 33;
constexpr int kFpfhGroup = 11;
constexpr int kFpfhMaxK = 255;
constexpr int kSpfhBlock = 256;
constexpr int kSpfhLanes = 8;       // G of the striding form
constexpr int kSpfhLanesMinK = 8;   // ... used from this K on
constexpr int kFpfhBlock = 256;
constexpr int kFpfhPts = 7;         // 7 x 33 = 231 of 256 lanes
constexpr float kPiF = 3.14159265358979323846f;
constexpr float kC1F = (float)(11.0 / (2.0 * 3.14159265358979323846));

// clamp(floorf((f + off) * scale), 0, 10), clamped in floating point: fmaxf(NaN, 0) = 0, so any value lands in a bin
__device__ __forceinline__ int fpfh_bin(float f, float off, float scale) {
  const float x = floorf((f + off) * scale);
  return (int)fminf(fmaxf(x, 0.0f), 10.0f);
}

template <int G>
__global__ __launch_bounds__(kSpfhBlock) void spfh_kernel(const float* __restrict__ points,
                                                          const float* __restrict__ normals,
                                                          const int64_t* __restrict__ idx,
                                                          const int64_t* __restrict__ lengths, int P, int K,
                                                          float4* __restrict__ pair, float* __restrict__ spfh) {
  constexpr int PTS = kSpfhBlock / G;
  __shared__ unsigned s_cnt[PTS * kFpfhBins];
  __shared__ float s_scale[PTS];
  const int n = blockIdx.y;
  const int i0 = blockIdx.x * PTS;
  const int rows = min(PTS, P - i0);
  const int len = clamped_length(lengths, n, P);
  for (int e = threadIdx.x; e < PTS * kFpfhBins; e += kSpfhBlock) s_cnt[e] = 0u;
  __syncthreads();

  const int p = threadIdx.x / G, g = threadIdx.x % G;
  if (p < rows) {
    const int i = i0 + p;
    const bool row_live = i < len;
    const float* __restrict__ pts = points + (int64_t)n * P * 3;
    const float* __restrict__ nrm = normals + (int64_t)n * P * 3;
    float pi[3] = {0.0f, 0.0f, 0.0f}, ni[3] = {0.0f, 0.0f, 0.0f};
    if (row_live) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        pi[d] = pts[(int64_t)i * 3 + d];
        ni[d] = nrm[(int64_t)i * 3 + d];
      }
    }
    const int64_t slot0 = ((int64_t)n * P + i) * K;
    unsigned* __restrict__ cnt = s_cnt + p * kFpfhBins;
    for (int k = g; k < K; k += G) {
      float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (row_live) {
        const int64_t j = idx[slot0 + k];
        if (j >= 0 && j < len && j != i) {
          float dp[3], nj[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            dp[d] = pts[j * 3 + d] - pi[d];
            nj[d] = nrm[j * 3 + d];
          }
          const float d2 = dot3f(dp, dp);
          if (d2 > 0.0f) {
            const float dist = sqrtf(d2);
            const float a1 = dot3f(ni, dp) / dist, a2 = dot3f(nj, dp) / dist;
            const bool swap = fabsf(a1) < fabsf(a2);
            float ns[3], nt[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              ns[d] = swap ? nj[d] : ni[d];
              nt[d] = swap ? ni[d] : nj[d];
              dp[d] = swap ? -dp[d] : dp[d];
            }
            const float f3 = swap ? -a2 : a1;
            float v[3], w[3];
            cross3f(dp, ns, v);
            const float vn = sqrtf(dot3f(v, v));
            if (vn > 0.0f) {
#pragma unroll
              for (int d = 0; d < 3; ++d) v[d] /= vn;
              cross3f(ns, v, w);
              const float f2 = dot3f(v, nt);
              const float f1 = atan2f(dot3f(w, nt), dot3f(ns, nt));
              out = make_float4(f1, f2, f3, dist);
              atomicAdd(cnt + fpfh_bin(f1, kPiF, kC1F), 1u);
              atomicAdd(cnt + kFpfhGroup + fpfh_bin(f2, 1.0f, 5.5f), 1u);
              atomicAdd(cnt + 2 * kFpfhGroup + fpfh_bin(f3, 1.0f, 5.5f), 1u);
            }
          }
        }
      }
      if (pair != nullptr) pair[slot0 + k] = out;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < PTS) {  // every group of 11 holds the row's m counted slots
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < kFpfhGroup; ++b) m += s_cnt[threadIdx.x * kFpfhBins + b];
    s_scale[threadIdx.x] = m > 0 ? 100.0f / (float)m : 0.0f;
  }
  __syncthreads();
  float* __restrict__ out = spfh + ((int64_t)n * P + i0) * kFpfhBins;
  for (int e = threadIdx.x; e < rows * kFpfhBins; e += kSpfhBlock) out[e] = (float)s_cnt[e] * s_scale[e / kFpfhBins];
}

__global__ __launch_bounds__(kFpfhBlock) void fpfh_kernel(const float* __restrict__ points,
                                                          const int64_t* __restrict__ idx,
                                                          const int64_t* __restrict__ lengths,
                                                          const float* __restrict__ spfh, int P, int K,
                                                          float* __restrict__ fpfh) {
  extern __shared__ __attribute__((aligned(16))) int s_slots[];  // [kFpfhPts][K] neighbour or -1, then [kFpfhPts][K] d2
  __shared__ float s_acc[kFpfhPts * kFpfhBins];
  int* __restrict__ s_j = s_slots;
  float* __restrict__ s_d2 = reinterpret_cast<float*>(s_slots + kFpfhPts * K);
  const int n = blockIdx.y;
  const int i0 = blockIdx.x * kFpfhPts;
  const int rows = min(kFpfhPts, P - i0);
  const int len = clamped_length(lengths, n, P);
  const float* __restrict__ pts = points + (int64_t)n * P * 3;
  const int64_t* __restrict__ idx0 = idx + ((int64_t)n * P + i0) * K;
  for (int e = threadIdx.x; e < rows * K; e += kFpfhBlock) {
    const int i = i0 + e / K;
    int jj = -1;
    float d2 = 0.0f;
    if (i < len) {
      const int64_t j = idx0[e];
      if (j >= 0 && j < len && j != i) {
        float dp[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) dp[d] = pts[j * 3 + d] - pts[(int64_t)i * 3 + d];
        d2 = dot3f(dp, dp);
        if (d2 > 0.0f) jj = (int)j;
      }
    }
    s_j[e] = jj;
    s_d2[e] = d2;
  }
  __syncthreads();

  const int p = threadIdx.x / kFpfhBins, b = threadIdx.x - p * kFpfhBins;
  const bool active = (int)threadIdx.x < rows * kFpfhBins;
  const bool row_live = active && i0 + p < len;
  float acc = 0.0f, own = 0.0f;
  if (row_live) {
    const float* __restrict__ sp = spfh + (int64_t)n * P * kFpfhBins;
    const int* __restrict__ js = s_j + p * K;
    const float* __restrict__ ds = s_d2 + p * K;
    for (int k = 0; k < K; ++k) {
      const int j = js[k];
      if (j >= 0) acc += sp[(int64_t)j * kFpfhBins + b] / ds[k];
    }
    own = sp[(int64_t)(i0 + p) * kFpfhBins + b];
  }
  if (threadIdx.x < kFpfhPts * kFpfhBins) s_acc[threadIdx.x] = acc;
  __syncthreads();
  if (active) {
    float r = 0.0f;
    if (row_live) {
      const float* __restrict__ grp = s_acc + p * kFpfhBins + (b / kFpfhGroup) * kFpfhGroup;
      float S = 0.0f;
#pragma unroll
      for (int q = 0; q < kFpfhGroup; ++q) S += grp[q];
      r = (S > 0.0f ? acc * 100.0f / S : 0.0f) + own;
    }
    fpfh[((int64_t)n * P + i0) * kFpfhBins + threadIdx.x] = r;
  }
}

static int fpfh_check_shape(const char* what, int64_t N, int64_t P, int64_t K) {
  POINTOPS_REQUIRE(N >= 0 && P >= 0 && K >= 1 && K <= kFpfhMaxK, "%s: need N, P >= 0 and 1 <= K <= 255", what);
  POINTOPS_REQUIRE(N < 65536 && P < (1LL << 30), "%s: need N < 65536 and P < 2^30", what);
  return POINTOPS_OK;
}

}  // namespace pointops

using namespace pointops;

extern "C" int pointops_spfh(const float* points, const float* normals, const int64_t* idx, const int64_t* lengths,
                             int64_t N, int64_t P, int64_t K, float* pair_features, float* spfh, void* stream_) {
  if (int rc = fpfh_check_shape("spfh", N, P, K)) return rc;
  if (N == 0 || P == 0) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const int lanes = (int)debug_knob("spfh_lanes", K >= kSpfhLanesMinK ? kSpfhLanes : 1);
  with_exact<1>(Ints<kSpfhLanes>{}, lanes, [&](auto G) {
    constexpr int g = decltype(G)::value;
    const dim3 grid((unsigned)ceil_div(P, kSpfhBlock / g), (unsigned)N);
    hipLaunchKernelGGL((spfh_kernel<g>), grid, dim3(kSpfhBlock), 0, stream, points, normals, idx, lengths, (int)P,
                       (int)K, reinterpret_cast<float4*>(pair_features), spfh);
  });
  return check_launch("spfh");
}

extern "C" int pointops_fpfh(const float* points, const int64_t* idx, const int64_t* lengths, const float* spfh,
                             int64_t N, int64_t P, int64_t K, float* fpfh, void* stream_) {
  if (int rc = fpfh_check_shape("fpfh", N, P, K)) return rc;
  if (N == 0 || P == 0) return POINTOPS_OK;
  const dim3 grid((unsigned)ceil_div(P, kFpfhPts), (unsigned)N);
  const size_t lds = (size_t)kFpfhPts * (size_t)K * (sizeof(int) + sizeof(float));
  hipLaunchKernelGGL(fpfh_kernel, grid, dim3(kFpfhBlock), lds, (hipStream_t)stream_, points, idx, lengths, spfh,
                     (int)P, (int)K, fpfh);
  return check_launch("fpfh");
}

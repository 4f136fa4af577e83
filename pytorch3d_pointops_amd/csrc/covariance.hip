// covariance.hip -- per-point covariance of a gathered K-neighbourhood, fused.
//
// Device half of get_point_covariances (reference: functions/utils.py:111-153), which builds the
// result from torch ops and materialises a (N,P,K,D,D) tensor of outer products (576 bytes per point
// at K = 16, D = 3) next to the centred copy of the neighbourhood:
//     m = mean_k x_k ;  cov[a][b] = mean_k (x_k[a] - m[a]) (x_k[b] - m[b]).
// Here one lane owns one point: the K x D neighbourhood row (contiguous, K*D*4 bytes) is read
// twice (mean pass, covariance pass), the D x D accumulators live in registers, and only the
// (N,P,D,D) result is written.  Backward (closed form):  grad_x_k = (G + G^T) (x_k - m) / K.
// The three passes are neighbourhood_sums.h's, which local_frames.hip calls as well; this file is
// where a lane's row lives and how it gets there.
// fp32 throughout; sums run in k order (the torch reduction order is unspecified: parity within 1e-5).
#include "common.h"
#include "neighbourhood_sums.h"

namespace pointops {

constexpr int kCovBlock = 256;  // rows per workgroup of the direct form
constexpr int kCovMaxD = 8;
// Staged form for K * D <= 64: a 128-lane workgroup loads its 128 neighbourhood rows COALESCED into
// LDS (row stride K*D + 1 words: conflict-free for the per-lane walk), then every lane makes both
// passes over its own row from LDS; the backward writes its results back in place, so that the global
// store is coalesced as well.  The direct form reads one 4..256-byte row per lane from L1/L2 with
// 64 cache lines per wave instruction (0.26 ms for 8 x 65536 x 16 x 3, no faster than the five
// torch kernels it replaces).
constexpr int kCovTile = 128;
constexpr int kCovStageMax = 64;  // floats per row

template <int DT, bool BACKWARD, bool STAGED>  // DT = compile-time D (2, 3) or 0 = runtime D <= kCovMaxD
__global__ __launch_bounds__(STAGED ? kCovTile : kCovBlock) void covariance_kernel(const float* __restrict__ knn,
                                                                                  const float* __restrict__ grad_cov,
                                                                                  int64_t rows, int K, int Drt,
                                                                                  float* __restrict__ out) {
  extern __shared__ float s_x[];  // STAGED: [kCovTile][K*D + 1]
  constexpr int DM = DT > 0 ? DT : kCovMaxD;
  constexpr int kRows = STAGED ? kCovTile : kCovBlock;
  const int D = DT > 0 ? DT : Drt;
  const int T = STAGED ? K * D : 0, stride = T + 1;  // floats of a staged row (K * D <= kCovStageMax) and its stride
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int nrows = (int)min((int64_t)kRows, rows - row0);
  if constexpr (STAGED) {
    const float* __restrict__ src = knn + row0 * T;
    for (int f = threadIdx.x; f < nrows * T; f += kCovTile) {
      const int r = f / T;
      s_x[r * stride + (f - r * T)] = src[f];
    }
    __syncthreads();
  }
  const bool active = (int)threadIdx.x < nrows;
  if (!(STAGED && BACKWARD) && !active) return;  // the staged backward has one more barrier: every lane must reach it
  if (active) {
    const int64_t r = row0 + threadIdx.x;
    // the lane's LDS row, read by the passes and written in place by the backward (formed but never used when direct)
    float* mine = s_x + threadIdx.x * stride;
    const float* x = STAGED ? mine : knn + r * K * D;
    auto row = [&](int k) { return x + k * D; };
    if constexpr (!BACKWARD) {
      float c[DM][DM];
      nb_covariance<DM>(row, K, D, c);
      float* __restrict__ o = out + r * D * D;
#pragma unroll
      for (int a = 0; a < DM; ++a)
#pragma unroll
        for (int b = 0; b < DM; ++b)
          if (a < D && b < D) o[a * D + b] = c[a][b];
    } else {
      nb_covariance_backward<DM>(row, K, D, grad_cov + r * D * D, STAGED ? mine : out + r * K * D);
    }
  }
  if constexpr (STAGED && BACKWARD) {
    __syncthreads();
    float* __restrict__ dst = out + row0 * T;
    for (int f = threadIdx.x; f < nrows * T; f += kCovTile) {
      const int rr = f / T;
      dst[f] = s_x[rr * stride + (f - rr * T)];
    }
  }
}

// out = cov (N,P,D,D) of the forward, grad_knn (N,P,K,D) of the backward
template <bool BACKWARD>
static int covariance_launch(const char* what, const float* knn, const float* grad_cov, int64_t N, int64_t P, int64_t K,
                             int64_t D, float* out, void* stream_) {
  POINTOPS_REQUIRE(N >= 0 && P >= 0 && K >= 1 && D >= 1 && D <= kCovMaxD && K < (1LL << 31),
                   "%s: need K >= 1 and 1 <= D <= %d", what, kCovMaxD);
  const int64_t rows = N * P;
  if (rows == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE(ceil_div(rows, kCovBlock) < (1LL << 31), "%s: grid too large", what);
  hipStream_t stream = (hipStream_t)stream_;
  const bool staged = K * D <= kCovStageMax;
  const dim3 grid((unsigned)ceil_div(rows, staged ? kCovTile : kCovBlock)), block(staged ? kCovTile : kCovBlock);
  const size_t lds = staged ? sizeof(float) * (size_t)kCovTile * (size_t)(K * D + 1) : 0;
  with_exact<0>(Ints<3, 2>{}, (int)D, [&](auto DT) {
    if (staged) {
      hipLaunchKernelGGL((covariance_kernel<DT, BACKWARD, true>), grid, block, lds, stream, knn, grad_cov, rows, (int)K,
                         (int)D, out);
    } else {
      hipLaunchKernelGGL((covariance_kernel<DT, BACKWARD, false>), grid, block, lds, stream, knn, grad_cov, rows,
                         (int)K, (int)D, out);
    }
  });
  return check_launch(what);
}

}  // namespace pointops

using namespace pointops;

extern "C" int pointops_point_covariances(const float* knn, int64_t N, int64_t P, int64_t K, int64_t D, float* cov,
                                          void* stream_) {
  return covariance_launch<false>("point_covariances", knn, nullptr, N, P, K, D, cov, stream_);
}

extern "C" int pointops_point_covariances_backward(const float* knn, const float* grad_cov, int64_t N, int64_t P,
                                                   int64_t K, int64_t D, float* grad_knn, void* stream_) {
  return covariance_launch<true>("point_covariances_backward", knn, grad_cov, N, P, K, D, grad_knn, stream_);
}

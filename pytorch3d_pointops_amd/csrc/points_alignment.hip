// points_alignment.hip -- weighted Umeyama / Kabsch alignment of corresponding points and one ICP iteration, fused.
//
// Device half of corresponding_points_alignment / iterative_closest_point (functions/points_alignment.py; PyTorch3D's
// ops/points_alignment.py).  The torch composition it replaces gathers Y through the K=1 neighbour table into an
// (N,P,1,d) tensor, forms two weighted means, two centred copies, a batched d x d product, a batched SVD, a
// determinant, the transformed cloud, a residual and a read-back: about twenty launch-bound kernels per iteration.
// All of it is one pass over the points into 3 + 4d + d^2 per-cloud moments plus one d x d problem per cloud:
//
//   1. alignment_moments_kernel   grid (nb, N): every thread walks rows i = b*256 + t + k*nb*256 of its cloud, reads
//      x = X[n,i], y = Y[n,i] or Y[n, idx[n,i]] (the 12-byte gather is the only uncoalesced access) and w, and
//      accumulates in fp64, about a per-cloud pivot (row 0 of X and of Y, so that clouds far from the origin lose
//      nothing to cancellation):  Sw, Sw2, Swx, Swy, Sw2x, Sw2y, Sw2 x y^T, Sw2 |x|^2   (w2 = w*w).
//      Wave sums go through DPP, the four waves of a block through LDS, and the block's partial to the workspace.
//   2. alignment_solve_kernel     one wave per cloud: lane m sums partial m over the blocks in ascending order (no
//      floating-point atomics anywhere: results are bit-reproducible), then lane 0 shifts the raw moments to the
//      centred ones in fp64 -- C = (Sxy - xm Sw2y^T - Sw2x ym^T + Sw2 xm ym^T) / W -- and factors C = U S V^T with a
//      ONE-SIDED Jacobi on C itself (the condition number is never squared), completes U by a perpendicular / cross
//      product where a singular value is negligible, fixes the determinant, and rounds R, T, s to fp32.
//   3. icp_apply_kernel           Xt = s X R + T in fp32 (zero rows past the length) and the block partials of
//      sum |Xt - Y[idx]|^2 in fp64;  icp_finish_kernel turns them into rmse, the relative change and one int32
//      "every cloud converged" word.
//
// pointops_icp_iteration chains the K=1 search (pointops_knn_points_idx_reuse on the caller's workspace, so that the
// grid over the unmodified target cloud is built once per ICP run) with 1-3.  The backward of the alignment is the
// elementwise alignment_backward_kernel: the gradient of the moments (from the host's float64 autograd of the N tiny
// solves) pushed to X, Y and the weights.
#include "block_sum.h"
#include "common.h"
#include "small_solvers.h"

namespace pointops {

template <int D>
__global__ __launch_bounds__(kPaBlock) void alignment_moments_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ idx,
    const int64_t* __restrict__ lengths, const float* __restrict__ weights, int P, int P2,
    double* __restrict__ partials) {
  using S = PaSlot<D>;
  constexpr int M = S::kCount;
  __shared__ double s_part[kPaWaves][M];
  const int n = blockIdx.y, nb = gridDim.x;
  const int64_t len = clamped_length<int64_t>(lengths, n, P);
  double px[D], py[D];
  pa_pivots<D>(X, Y, n, P, P2, len, px, py);
  const float* __restrict__ xs = X + (int64_t)n * P * D;
  const float* __restrict__ ys = Y + (int64_t)n * P2 * D;
  double acc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kPaBlock + threadIdx.x; i < len; i += (int64_t)nb * kPaBlock) {
    int64_t j = i;
    if (idx != nullptr) {
      j = idx[(int64_t)n * P + i];
      j = j < 0 ? 0 : (j >= P2 ? P2 - 1 : j);
    }
    const double w = weights != nullptr ? (double)weights[(int64_t)n * P + i] : 1.0;
    double x[D], y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      x[d] = (double)xs[i * D + d] - px[d];
      y[d] = (P2 > 0 ? (double)ys[j * D + d] : 0.0) - py[d];
    }
    pa_accumulate<D>(acc, w, x, y);
  }
  pa_block_sum<M>(acc, s_part, partials + ((int64_t)n * nb + blockIdx.x) * M);
}

template <int D>
__global__ __launch_bounds__(kWave) void alignment_solve_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ lengths, int P, int P2,
    int nb, const double* __restrict__ partials, int estimate_scale, int allow_reflection, double eps,
    float* __restrict__ R, float* __restrict__ T, float* __restrict__ s, double* __restrict__ moments,
    float* __restrict__ sing) {
  constexpr int M = PaSlot<D>::kCount;
  __shared__ double s_mom[M];
  const int n = blockIdx.x;
  pa_sum_partials<M>(partials + (int64_t)n * nb * M, nb, true, s_mom,
                     moments != nullptr ? moments + (int64_t)n * M : nullptr);
  if (threadIdx.x != 0) return;
  double px[D], py[D], Rd[D][D], Td[D], sd, sg[D];
  pa_pivots<D>(X, Y, n, P, P2, clamped_length<int64_t>(lengths, n, P), px, py);
  pa_solve<D>(s_mom, px, py, estimate_scale != 0, allow_reflection != 0, eps, Rd, Td, sd, sg);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    T[(int64_t)n * D + a] = (float)Td[a];
    if (sing != nullptr) sing[(int64_t)n * D + a] = (float)sg[a];
#pragma unroll
    for (int b = 0; b < D; ++b) R[((int64_t)n * D + a) * D + b] = (float)Rd[a][b];
  }
  s[n] = (float)sd;
}

// Xt = s X R + T (fp32; zero rows past the length) and the block partials of sum_valid |Xt - Y[idx]|^2 (fp64).
template <int D>
__global__ __launch_bounds__(kPaBlock) void icp_apply_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ idx,
    const int64_t* __restrict__ lengths, const float* __restrict__ R, const float* __restrict__ T,
    const float* __restrict__ s, int P, int P2, float* __restrict__ Xt, double* __restrict__ partials) {
  __shared__ double s_part[kPaWaves][1];
  const int n = blockIdx.y, nb = gridDim.x;
  const int64_t len = clamped_length<int64_t>(lengths, n, P);
  float r[D][D], t[D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    t[a] = T[(int64_t)n * D + a];
#pragma unroll
    for (int b = 0; b < D; ++b) r[a][b] = R[((int64_t)n * D + a) * D + b];
  }
  const float sc = s[n];
  const float* __restrict__ xs = X + (int64_t)n * P * D;
  const float* __restrict__ ys = Y + (int64_t)n * P2 * D;
  float* __restrict__ xt = Xt + (int64_t)n * P * D;
  double acc[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * kPaBlock + threadIdx.x; i < P; i += (int64_t)nb * kPaBlock) {
    if (i >= len) {
#pragma unroll
      for (int d = 0; d < D; ++d) xt[i * D + d] = 0.0f;
      continue;
    }
    float x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = xs[i * D + d];
    int64_t j = idx[(int64_t)n * P + i];
    j = j < 0 ? 0 : (j >= P2 ? P2 - 1 : j);
#pragma unroll
    for (int b = 0; b < D; ++b) {
      float v = x[0] * r[0][b];
#pragma unroll
      for (int a = 1; a < D; ++a) v += x[a] * r[a][b];
      v = sc * v + t[b];
      xt[i * D + b] = v;
      const double e = (double)v - (P2 > 0 ? (double)ys[j * D + b] : 0.0);
      acc[0] += e * e;
    }
  }
  pa_block_sum<1>(acc, s_part, partials + (int64_t)n * nb + blockIdx.x);
}

// rmse[n] = sqrt(sum / max(len, 1e-9)); relative change against the previous rmse (1 on the first iteration, 0 where
// the previous rmse is 0: an empty or exactly matched cloud has nothing left to gain); converged = every cloud's
// change <= thr.  One block.
__global__ __launch_bounds__(kPaBlock) void icp_finish_kernel(const double* __restrict__ partials,
                                                              const int64_t* __restrict__ lengths, int N, int P,
                                                              int nb, int first, float thr, float* __restrict__ rmse,
                                                              int* __restrict__ converged) {
  int bad = 0;
  for (int n = threadIdx.x; n < N; n += kPaBlock) {
    double v = 0.0;
    for (int b = 0; b < nb; ++b) v += partials[(int64_t)n * nb + b];
    const double len = (double)clamped_length<int64_t>(lengths, n, P);
    const float cur = (float)sqrt(v / (len > 1e-9 ? len : 1e-9));
    const float prev = rmse[n];
    const float rel = first ? 1.0f : (prev > 0.0f ? (prev - cur) / prev : 0.0f);
    rmse[n] = cur;
    bad |= !(rel <= thr);
  }
  const int any_bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) converged[0] = any_bad ? 0 : 1;
}

// Gradient of the moments pushed to the points: one thread per row.
template <int D>
__global__ __launch_bounds__(kPaBlock) void alignment_backward_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ lengths,
    const float* __restrict__ weights, const double* __restrict__ grad_moments, int64_t rows, int P,
    float* __restrict__ grad_X, float* __restrict__ grad_Y, float* __restrict__ grad_w) {
  using S = PaSlot<D>;
  const int64_t row = (int64_t)blockIdx.x * kPaBlock + threadIdx.x;
  if (row >= rows) return;
  const int n = (int)(row / P);
  const int64_t i = row - (int64_t)n * P;
  const int64_t len = clamped_length<int64_t>(lengths, n, P);
  if (i >= len) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      grad_X[row * D + d] = 0.0f;
      grad_Y[row * D + d] = 0.0f;
    }
    if (grad_w != nullptr) grad_w[row] = 0.0f;
    return;
  }
  double px[D], py[D];
  pa_pivots<D>(X, Y, n, P, P, len, px, py);
  const double* __restrict__ g = grad_moments + (int64_t)n * S::kCount;
  const double w = weights != nullptr ? (double)weights[row] : 1.0;
  const double w2 = w * w;
  double x[D], y[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = (double)X[row * D + d] - px[d];
    y[d] = (double)Y[row * D + d] - py[d];
  }
  double gw1 = g[S::kSw], gw2 = g[S::kSw2];  // d/dw = gw1 + 2 w gw2
  double xx = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double gxy_y = 0.0, gxy_x = 0.0;
#pragma unroll
    for (int b = 0; b < D; ++b) {
      gxy_y += g[S::kSxy + a * D + b] * y[b];
      gxy_x += g[S::kSxy + b * D + a] * x[b];
    }
    grad_X[row * D + a] = (float)(w * g[S::kSwx + a] + w2 * (g[S::kSw2x + a] + gxy_y + 2.0 * g[S::kSxx] * x[a]));
    grad_Y[row * D + a] = (float)(w * g[S::kSwy + a] + w2 * (g[S::kSw2y + a] + gxy_x));
    gw1 += g[S::kSwx + a] * x[a] + g[S::kSwy + a] * y[a];
    gw2 += g[S::kSw2x + a] * x[a] + g[S::kSw2y + a] * y[a] + x[a] * gxy_y;
    xx += x[a] * x[a];
  }
  gw2 += g[S::kSxx] * xx;
  if (grad_w != nullptr) grad_w[row] = (float)(gw1 + 2.0 * w * gw2);
}

// ------------------------------------------------------------------------------------------------ host side
struct AlignmentLayout {
  double* partials;  // (N, nb, moments)
  double* residual;  // (N, nb): ICP only
  size_t bytes;
};

static AlignmentLayout alignment_layout(void* ws, int64_t N, int64_t P, int64_t D, bool icp) {
  Carver c(ws);
  AlignmentLayout l;
  const size_t nb = (size_t)pa_blocks(P);
  l.partials = (double*)c.take(sizeof(double) * (size_t)N * nb * (size_t)pa_moments((int)D));
  l.residual = icp ? (double*)c.take(sizeof(double) * (size_t)N * nb) : nullptr;
  l.bytes = c.off;
  return l;
}

static bool alignment_shape_ok(int64_t N, int64_t P, int64_t P2, int64_t D) {
  return N >= 0 && N < 65536 && P >= 0 && P < (1LL << 30) && P2 >= 0 && P2 < (1LL << 30) && (D == 2 || D == 3);
}

static int alignment_launch(const float* X, const float* Y, const int64_t* idx, const int64_t* lengths,
                            const float* weights, int64_t N, int64_t P, int64_t P2, int64_t D, int estimate_scale,
                            int allow_reflection, double eps, float* R, float* T, float* s, double* moments,
                            float* sing, const AlignmentLayout& l, hipStream_t stream) {
  const int nb = pa_blocks(P);
  with_exact<3>(Ints<2>{}, (int)D, [&](auto Dc) {
    constexpr int kD = decltype(Dc)::value;
    hipLaunchKernelGGL((alignment_moments_kernel<kD>), dim3((unsigned)nb, (unsigned)N), dim3(kPaBlock), 0, stream, X,
                       Y, idx, lengths, weights, (int)P, (int)P2, l.partials);
    hipLaunchKernelGGL((alignment_solve_kernel<kD>), dim3((unsigned)N), dim3(kWave), 0, stream, X, Y, lengths, (int)P,
                       (int)P2, nb, (const double*)l.partials, estimate_scale, allow_reflection, eps, R, T, s, moments,
                       sing);
  });
  return check_launch("points_alignment");
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_points_alignment_workspace_bytes(int64_t N, int64_t P, int64_t D) {
  if (!alignment_shape_ok(N, P, P, D)) return 0;
  return alignment_layout(nullptr, N, P, D, false).bytes;
}

extern "C" int pointops_points_alignment(const float* X, const float* Y, const int64_t* idx, const int64_t* lengths,
                                         const float* weights, int64_t N, int64_t P, int64_t P2, int64_t D,
                                         int estimate_scale, int allow_reflection, double eps, float* R, float* T,
                                         float* s, double* moments, float* singular_values, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(alignment_shape_ok(N, P, P2, D),
                   "points_alignment: need 0 <= N < 65536, 0 <= P, P2 < 2^30 and D in {2, 3}");
  POINTOPS_REQUIRE(idx != nullptr || P2 == P, "points_alignment: without idx, Y must have P rows per cloud");
  if (N == 0) return POINTOPS_OK;
  const AlignmentLayout l = alignment_layout(workspace, N, P, D, false);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "points_alignment: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  return alignment_launch(X, Y, idx, lengths, weights, N, P, P2, D, estimate_scale, allow_reflection, eps, R, T, s,
                          moments, singular_values, l, (hipStream_t)stream_);
}

extern "C" int pointops_points_alignment_backward(const float* X, const float* Y, const int64_t* lengths,
                                                  const float* weights, const double* grad_moments, int64_t N,
                                                  int64_t P, int64_t D, float* grad_X, float* grad_Y,
                                                  float* grad_weights, void* stream_) {
  POINTOPS_REQUIRE(alignment_shape_ok(N, P, P, D),
                   "points_alignment_backward: need 0 <= N < 65536, 0 <= P < 2^30 and D in {2, 3}");
  const int64_t rows = N * P;
  if (rows == 0) return POINTOPS_OK;
  const int64_t blocks = ceil_div(rows, kPaBlock);
  POINTOPS_REQUIRE(blocks < (1LL << 31), "points_alignment_backward: grid too large");
  with_exact<3>(Ints<2>{}, (int)D, [&](auto Dc) {
    hipLaunchKernelGGL((alignment_backward_kernel<decltype(Dc)::value>), dim3((unsigned)blocks), dim3(kPaBlock), 0,
                       (hipStream_t)stream_, X, Y, lengths, weights, grad_moments, rows, (int)P, grad_X, grad_Y,
                       grad_weights);
  });
  return check_launch("points_alignment_backward");
}

extern "C" size_t pointops_icp_workspace_bytes(int64_t N, int64_t P1, int64_t D) {
  if (!alignment_shape_ok(N, P1, P1, D)) return 0;
  return alignment_layout(nullptr, N, P1, D, true).bytes;
}

extern "C" int pointops_icp_iteration(const float* X_init, float* Xt, const float* Y, const int64_t* lengths_x,
                                      const int64_t* lengths_y, int64_t N, int64_t P1, int64_t P2, int64_t D,
                                      int estimate_scale, int allow_reflection, int first, int reuse,
                                      float relative_rmse_thr, int64_t* idx, float* dists, float* R, float* T,
                                      float* s, float* rmse, int32_t* converged, void* knn_workspace,
                                      size_t knn_workspace_bytes, void* workspace, size_t workspace_bytes,
                                      void* stream_) {
  POINTOPS_REQUIRE(alignment_shape_ok(N, P1, P2, D),
                   "icp_iteration: need 0 <= N < 65536, 0 <= P1, P2 < 2^30 and D in {2, 3}");
  POINTOPS_REQUIRE(N >= 1 && P1 >= 1 && P2 >= 1, "icp_iteration: need N, P1, P2 >= 1");
  POINTOPS_REQUIRE(lengths_x != nullptr && lengths_y != nullptr, "icp_iteration: lengths are required");
  POINTOPS_REQUIRE(reuse >= -1 && reuse <= 1, "icp_iteration: reuse is -1 (idx is given), 0 or 1");
  hipStream_t stream = (hipStream_t)stream_;
  const AlignmentLayout l = alignment_layout(workspace, N, P1, D, true);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "icp_iteration: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  if (reuse >= 0) {
    const int rc = pointops_knn_points_idx_reuse(Xt, Y, lengths_x, lengths_y, N, P1, P2, D, 2, 1, -1, idx, dists,
                                                 knn_workspace, knn_workspace_bytes, reuse, stream_);
    if (rc != POINTOPS_OK) return rc;
  }
  int rc = alignment_launch(X_init, Y, idx, lengths_x, nullptr, N, P1, P2, D, estimate_scale, allow_reflection, 1e-9,
                            R, T, s, nullptr, nullptr, l, stream);
  if (rc != POINTOPS_OK) return rc;
  const int nb = pa_blocks(P1);
  with_exact<3>(Ints<2>{}, (int)D, [&](auto Dc) {
    hipLaunchKernelGGL((icp_apply_kernel<decltype(Dc)::value>), dim3((unsigned)nb, (unsigned)N), dim3(kPaBlock), 0,
                       stream, X_init, Y, (const int64_t*)idx, lengths_x, (const float*)R, (const float*)T,
                       (const float*)s, (int)P1, (int)P2, Xt, l.residual);
  });
  hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(kPaBlock), 0, stream, (const double*)l.residual, lengths_x,
                     (int)N, (int)P1, nb, first, relative_rmse_thr, rmse, converged);
  return check_launch("icp_iteration");
}

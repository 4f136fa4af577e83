// local_frames.hip -- per-point curvatures and local coordinate frames of a K-neighbourhood, fused.
//
// Device half of estimate_pointcloud_local_coord_frames / estimate_pointcloud_normals
// (functions/points_normals.py).  The torch composition it replaces writes the gathered (N,P,K,3) neighbourhood,
// reads it back for the covariance, hands (N*P) 3x3 matrices to a batched eigensolver and reads the neighbourhood a
// third time for the sign disambiguation.  Here one lane owns one query point i of cloud n:
//   1. the K neighbour rows x_k = points[n, idx[n,i,k]] (zero where k >= lengths[n] or idx is out of range, like
//      gather_neighbors with lengths);
//   2. m = mean_k x_k, C = mean_k (x_k - m)(x_k - m)^T in fp32, by the functions of neighbourhood_sums.h that
//      covariance.hip calls: C is bit-equal to point_covariances(gather_neighbors(points, idx, lengths));
//   3. cyclic Jacobi in fp64 on C, eigenpairs sorted ascending (stable: a zero C gives the identity frame), rounded
//      to fp32 -- curvatures = eigenvalues, frame columns = eigenvectors (v0, v1, v2);
//   4. with `disambiguate`: v0 -> n and v2 -> z are flipped when fewer than K/2 neighbours have (x_k - x_i).v > 0,
//      and the frame becomes (n, n x z, z).
// Rows i >= lengths[n] are zero.  No atomics, no workspace, no allocation: deterministic and graph-capturable.
//
// The staged form (K <= kLfStageMaxK) gathers the workgroup's neighbourhoods into LDS once: the index rows of its
// 64 queries are one contiguous run of 64*K int64 values, read coalesced, and each neighbour row is gathered once;
// every pass then walks the lane's own LDS row.  Larger K reads the lane's index row and re-gathers per pass
// (L1/L2 hits).
//
// Backward (closed form, one lane per point): with y = n x z folded into n and z first (g_n += z x g_y,
// g_z += g_y x n, g_v1 = 0), grad_C = sum_i g_lambda_i v_i v_i^T + sum_{i != j} (v_j . g_v_i) / (lambda_i - lambda_j)
// v_j v_i^T -- the eigh backward; the flips are piecewise constant.  Coincident eigenvalues divide by zero, as
// torch.linalg.eigh's backward does.  The rest of the chain (gather, covariance backward, scatter) is existing code.
#include "common.h"
#include "neighbourhood_sums.h"
#include "small_solvers.h"

namespace pointops {

constexpr int kLfTile = 64;           // queries (lanes) per workgroup of the forward
constexpr int kLfStageMaxK = 64;      // staged form: 64 rows of (3K | 1) floats <= 49.4 KiB of LDS
constexpr int kLfBwdBlock = 256;

template <bool STAGED>
__global__ __launch_bounds__(kLfTile) void local_frames_kernel(const float* __restrict__ points,
                                                               const int64_t* __restrict__ lengths,
                                                               const int64_t* __restrict__ idx, int P, int K,
                                                               int disambiguate, float* __restrict__ curv,
                                                               float* __restrict__ frames) {
  extern __shared__ __attribute__((aligned(16))) float s_x[];  // STAGED: [kLfTile][stride]
  const int n = blockIdx.y;
  const int i0 = blockIdx.x * kLfTile;
  const int nrows = min(kLfTile, P - i0);
  const int64_t len = lengths[n];
  const float* __restrict__ pts = points + (int64_t)n * P * 3;
  const int64_t* __restrict__ idx0 = idx + ((int64_t)n * P + i0) * K;
  const int stride = (3 * K) | 1;  // odd row stride: the per-lane walk is free of bank conflicts
  if constexpr (STAGED) {
    const int live = (int)max((int64_t)0, min((int64_t)nrows, len - i0));  // rows i >= len are not gathered
#pragma unroll 4
    for (int f = threadIdx.x; f < live * K; f += kLfTile) {
      const int r = f / K, k = f - r * K;
      const int64_t j = idx0[f];
      const bool ok = j >= 0 && j < P && (int64_t)k < len;
      const float* __restrict__ src = pts + (ok ? j : 0) * 3;
      const float x0 = src[0], x1 = src[1], x2 = src[2];
      float* __restrict__ dst = s_x + r * stride + 3 * k;
      dst[0] = ok ? x0 : 0.0f;
      dst[1] = ok ? x1 : 0.0f;
      dst[2] = ok ? x2 : 0.0f;
    }
    __syncthreads();  // the only barrier: lanes may leave after it
  }
  if ((int)threadIdx.x >= nrows) return;
  const int i = i0 + threadIdx.x;
  const int64_t row = (int64_t)n * P + i;
  float* __restrict__ oc = curv + row * 3;
  float* __restrict__ of = frames + row * 9;
  if ((int64_t)i >= len) {
#pragma unroll
    for (int e = 0; e < 3; ++e) oc[e] = 0.0f;
#pragma unroll
    for (int e = 0; e < 9; ++e) of[e] = 0.0f;
    return;
  }
  const float* __restrict__ sx = s_x + threadIdx.x * stride;
  const int64_t* __restrict__ my_idx = idx0 + (int64_t)threadIdx.x * K;
  auto neighbour = [&](int k) {
    NbRow<3> x;
    if constexpr (STAGED) {
#pragma unroll
      for (int d = 0; d < 3; ++d) x.v[d] = sx[3 * k + d];
    } else {
      const int64_t j = my_idx[k];
      const bool ok = j >= 0 && j < P && (int64_t)k < len;
      const float* __restrict__ src = pts + (ok ? j : 0) * 3;
#pragma unroll
      for (int d = 0; d < 3; ++d) x.v[d] = ok ? src[d] : 0.0f;
    }
    return x;
  };

  // mean and covariance: neighbourhood_sums.h's, the functions covariance.hip calls
  float c[3][3];
  nb_covariance<3>(neighbour, K, 3, c);

  float lam[3], f[3][3];  // f[a][j] = component a of eigenvector j
  sym3_eigen(c, lam, f);

  if (disambiguate) {
    float xi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) xi[d] = pts[(int64_t)i * 3 + d];
    int pos0 = 0, pos2 = 0;
    for (int k = 0; k < K; ++k) {
      const NbRow<3> x = neighbour(k);
      float dx[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) dx[d] = x[d] - xi[d];
      const float p0 = dx[0] * f[0][0] + dx[1] * f[1][0] + dx[2] * f[2][0];
      const float p2 = dx[0] * f[0][2] + dx[1] * f[1][2] + dx[2] * f[2][2];
      pos0 += p0 > 0.0f;
      pos2 += p2 > 0.0f;
    }
    // flip when pos < 0.5 * K
    const float s0 = 2 * pos0 < K ? -1.0f : 1.0f, s2 = 2 * pos2 < K ? -1.0f : 1.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      f[d][0] *= s0;
      f[d][2] *= s2;
    }
    // y = n x z
    f[0][1] = f[1][0] * f[2][2] - f[2][0] * f[1][2];
    f[1][1] = f[2][0] * f[0][2] - f[0][0] * f[2][2];
    f[2][1] = f[0][0] * f[1][2] - f[1][0] * f[0][2];
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) oc[e] = lam[e];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) of[a * 3 + b] = f[a][b];
}

__global__ __launch_bounds__(kLfBwdBlock) void local_frames_backward_kernel(
    const float* __restrict__ curv, const float* __restrict__ frames, const float* __restrict__ grad_curv,
    const float* __restrict__ grad_frames, const int64_t* __restrict__ lengths, int64_t rows, int64_t P,
    int disambiguate, float* __restrict__ grad_cov) {
  const int64_t r = (int64_t)blockIdx.x * kLfBwdBlock + threadIdx.x;
  if (r >= rows) return;
  const int64_t n = r / P, i = r - n * P;
  float* __restrict__ o = grad_cov + r * 9;
  if (i >= lengths[n]) {
#pragma unroll
    for (int e = 0; e < 9; ++e) o[e] = 0.0f;
    return;
  }
  float lam[3], gl[3], v[3][3], gv[3][3];  // v[j] = frame column j, gv[j] = its gradient
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    lam[j] = curv[r * 3 + j];
    gl[j] = grad_curv[r * 3 + j];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[j][a] = frames[r * 9 + a * 3 + j];
      gv[j][a] = grad_frames[r * 9 + a * 3 + j];
    }
  }
  if (disambiguate) {  // y = n x z: g_n += z x g_y, g_z += g_y x n
    float t0[3], t2[3];
    cross3f(v[2], gv[1], t0);
    cross3f(gv[1], v[0], t2);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      gv[0][a] += t0[a];
      gv[2][a] += t2[a];
      gv[1][a] = 0.0f;
    }
  }
  float w[3][3];  // grad_C = sum_{j,i} w[j][i] v_j v_i^T
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (j == q) {
        w[j][q] = gl[q];
      } else {
        const float dot = v[j][0] * gv[q][0] + v[j][1] * gv[q][1] + v[j][2] * gv[q][2];
        w[j][q] = dot / (lam[q] - lam[j]);
      }
    }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) acc += w[j][q] * v[j][a] * v[q][b];
      o[a * 3 + b] = acc;
    }
}

}  // namespace pointops

using namespace pointops;

extern "C" int pointops_local_frames(const float* points, const int64_t* lengths, const int64_t* idx, int64_t N,
                                     int64_t P, int64_t K, int disambiguate, float* curvatures, float* frames,
                                     void* stream_) {
  POINTOPS_REQUIRE(N >= 0 && P >= 0 && K >= 1, "local_frames: need N, P >= 0 and K >= 1");
  POINTOPS_REQUIRE(N < 65536 && P < (1LL << 30) && K < (1LL << 20),
                   "local_frames: need N < 65536, P < 2^30 and K < 2^20");
  if (N == 0 || P == 0) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)ceil_div(P, kLfTile), (unsigned)N), block(kLfTile);
  const bool staged = K <= kLfStageMaxK;
  const size_t lds = staged ? sizeof(float) * (size_t)kLfTile * (size_t)((3 * K) | 1) : 0;
  with_exact<0>(Ints<1>{}, (int)staged, [&](auto S) {
    hipLaunchKernelGGL((local_frames_kernel<decltype(S)::value == 1>), grid, block, lds, stream, points, lengths, idx,
                       (int)P, (int)K, disambiguate, curvatures, frames);
  });
  return check_launch("local_frames");
}

extern "C" int pointops_local_frames_backward(const float* curvatures, const float* frames,
                                              const float* grad_curvatures, const float* grad_frames,
                                              const int64_t* lengths, int64_t N, int64_t P, int disambiguate,
                                              float* grad_cov, void* stream_) {
  POINTOPS_REQUIRE(N >= 0 && P >= 0, "local_frames_backward: need N, P >= 0");
  const int64_t rows = N * P;
  if (rows == 0) return POINTOPS_OK;
  const int64_t blocks = ceil_div(rows, kLfBwdBlock);
  POINTOPS_REQUIRE(blocks < (1LL << 31), "local_frames_backward: grid too large");
  hipLaunchKernelGGL(local_frames_backward_kernel, dim3((unsigned)blocks), dim3(kLfBwdBlock), 0,
                     (hipStream_t)stream_, curvatures, frames, grad_curvatures, grad_frames, lengths, rows, P,
                     disambiguate, grad_cov);
  return check_launch("local_frames_backward");
}

// registration.hip -- one step of registration_icp: trimmed point-to-plane / point-to-point ICP, fused.
//
// Device half of functions/registration.py (Open3D's registration_icp with TransformationEstimationPointToPlane /
// PointToPoint; PCL's IterativeClosestPoint with setMaxCorrespondenceDistance).  The contract -- every stage of a step,
// exactly enough for the numpy checker of tests/registration_ref.py -- is the REGISTRATION block of
// include/pointops_amd.h; in short, per cloud and step:
//
//   search    K=1, L2 search of Xt in Y (pointops_knn_points_idx_reuse on the caller's workspace: the grid over the
//             unmodified target is built once per run) -> idx, d2; or, with search_version =
//             POINTOPS_REGISTRATION_SEARCH_BOUNDED, the K=1 pointops_knn_in_radius with radius r_max: (-1, 0) on the
//             rows with nothing inside the radius, the same idx, d2 elsewhere
//   inliers   row r counts iff r < len_x, len_y > 0, idx >= 0 and d2 < fl32(r_max * r_max)        (ball_query's rule)
//   evaluate  c = inliers, fitness = fl32(c / max(len_x, 1)), inlier_rmse = fl32(sqrt(sum d2 / max(c, 1)))
//   freeze    status 0 when both moved less than the thresholds since the previous step; else
//   update    point-to-plane: A = sum J^T J, b = -sum J rho over the inliers about the pivot c0 = Xt[0], one fp64
//             Cholesky (icp_plane.h), the exact rotation of the three angles, composed onto the fp64 transform;
//             point-to-point: pa_solve (small_solvers.h) of the ORIGINAL rows onto Y[idx], weights 1 / 0;
//             too few inliers or a degenerate pivot freeze the cloud with status 1 and leave its transform alone
//   write     history entry = fl32(R, T); Xt = X_init R + T in fp32 (icp_apply_kernel's arithmetic), zero past len_x
//
// Kernels of a step (after the search):
//   1. registration_moments_kernel   grid (nb, N), 256 threads: every thread walks rows i = b*256 + t + k*nb*256, writes
//      correspondences[i] and accumulates 29 fp64 sums (A 21, b 6, c, sum d2; or the 24 alignment moments, c, sum d2).
//      The 12-byte gathers of Y[idx] and normals[idx] are the only uncoalesced reads.  Wave sums go through DPP, the
//      four waves through LDS, the block's partial to the workspace (block_sum.h).  No floating-point atomics.
//   2. registration_solve_kernel     one wave per cloud: lane m sums partial m over the blocks in ascending order; lane 0
//      evaluates, decides, solves, composes and writes the history entry and the per-cloud state.
//   3. registration_apply_kernel     Xt of the clouds whose transform moved.
//   4. registration_frozen_kernel    one block: the "every cloud frozen" word.
// A frozen cloud costs a block exit in 1 and 3 and repeats its history entry in 2: enqueueing more steps than a run
// needs is legal, which is what makes the loop capturable into a HIP graph.  `first` runs registration_init_kernel
// before the search: the per-cloud state from the initial transform, and Xt.
#include "block_sum.h"
#include "common.h"
#include "debug.h"
#include "icp_plane.h"
#include "small_solvers.h"

namespace pointops {

constexpr int kRegMoments = 29;   // fp64 sums per cloud
constexpr int kRegMomentsOut = 35;  // the optional `moments` output: the sums, then the solved x (6)
constexpr int kRegCount = 27;     // slot of c
constexpr int kRegSumD2 = 28;     // slot of sum d2
constexpr int kRegState = 16;     // fp64 words of a cloud's state: R (9), T (3), prev_fitness, prev_rmse, 2 spare
constexpr int kRegRunning = 2;    // status of a cloud that is not frozen
static_assert(PaSlot<3>::kCount <= kRegCount && kIcpUpper + 6 == kRegCount, "c and sum d2 follow the moments");

enum { kRegPointToPoint = 0, kRegPointToPlane = 1 };

__device__ __forceinline__ void reg_apply_row(const float* __restrict__ xs, float* __restrict__ xt, int64_t i,
                                              int64_t len, const float (&r)[3][3], const float (&t)[3]) {
  if (i >= len) {
#pragma unroll
    for (int d = 0; d < 3; ++d) xt[i * 3 + d] = 0.0f;
    return;
  }
  const float x[3] = {xs[i * 3], xs[i * 3 + 1], xs[i * 3 + 2]};
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    float v = x[0] * r[0][b];
    v += x[1] * r[1][b];
    v += x[2] * r[2][b];
    xt[i * 3 + b] = v + t[b];
  }
}

// state, status, iterations from the initial transform (NULL: the identity) and Xt = X_init R0 + T0
__global__ __launch_bounds__(kPaBlock) void registration_init_kernel(
    const float* __restrict__ X_init, const int64_t* __restrict__ lengths_x, const float* __restrict__ R0,
    const float* __restrict__ T0, int P1, float* __restrict__ Xt, double* __restrict__ state,
    int32_t* __restrict__ status, int32_t* __restrict__ iterations) {
  const int n = blockIdx.y, nb = gridDim.x;
  const int64_t len = clamped_length<int64_t>(lengths_x, n, P1);
  float r[3][3], t[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t[a] = T0 != nullptr ? T0[(int64_t)n * 3 + a] : 0.0f;
#pragma unroll
    for (int b = 0; b < 3; ++b) r[a][b] = R0 != nullptr ? R0[((int64_t)n * 3 + a) * 3 + b] : (a == b ? 1.0f : 0.0f);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double* __restrict__ st = state + (int64_t)n * kRegState;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      st[9 + a] = (double)t[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) st[a * 3 + b] = (double)r[a][b];
    }
#pragma unroll
    for (int k = 12; k < kRegState; ++k) st[k] = 0.0;
    status[n] = kRegRunning;
    iterations[n] = 0;
  }
  const float* __restrict__ xs = X_init + (int64_t)n * P1 * 3;
  float* __restrict__ xt = Xt + (int64_t)n * P1 * 3;
  for (int64_t i = (int64_t)blockIdx.x * kPaBlock + threadIdx.x; i < P1; i += (int64_t)nb * kPaBlock)
    reg_apply_row(xs, xt, i, len, r, t);
}

template <int EST>
__global__ __launch_bounds__(kPaBlock) void registration_moments_kernel(
    const float* __restrict__ X_init, const float* __restrict__ Xt, const float* __restrict__ Y,
    const float* __restrict__ normals, const int64_t* __restrict__ idx, const float* __restrict__ d2s,
    const int64_t* __restrict__ lengths_x, const int64_t* __restrict__ lengths_y,
    const int32_t* __restrict__ status, int P1, int P2, float r2, int64_t* __restrict__ correspondences,
    double* __restrict__ partials) {
  constexpr int M = kRegMoments;
  __shared__ double s_part[kPaWaves][M];
  const int n = blockIdx.y, nb = gridDim.x;
  if (status[n] != kRegRunning) return;  // (the whole block: a frozen cloud leaves everything as it is)
  const int64_t len = clamped_length<int64_t>(lengths_x, n, P1);
  const bool has_y = clamped_length<int64_t>(lengths_y, n, P2) > 0;
  const float* __restrict__ src = (EST == kRegPointToPlane ? Xt : X_init) + (int64_t)n * P1 * 3;
  const float* __restrict__ ys = Y + (int64_t)n * P2 * 3;
  const float* __restrict__ ns = EST == kRegPointToPlane ? normals + (int64_t)n * P2 * 3 : nullptr;
  // the pivots: row 0 of the transformed cloud (plane), rows 0 of the original cloud and of the target (point)
  double px[3], py[3];
  pa_pivots<3>(EST == kRegPointToPlane ? Xt : X_init, Y, n, P1, P2, len, px, py);
  double acc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kPaBlock + threadIdx.x; i < P1; i += (int64_t)nb * kPaBlock) {
    const int64_t at = (int64_t)n * P1 + i;
    bool in = false;
    int64_t j = 0;
    float d2 = 0.0f;
    if (i < len && has_y) {
      d2 = d2s[at];
      j = idx[at];
      in = j >= 0 && d2 < r2;  // (j < 0: the bounded search's "nothing inside the radius")
      j = j < 0 ? 0 : (j >= P2 ? P2 - 1 : j);
    }
    correspondences[at] = in ? j : -1;
    if (!in) continue;
    acc[kRegCount] += 1.0;
    acc[kRegSumD2] += (double)d2;
    const double x[3] = {(double)src[i * 3], (double)src[i * 3 + 1], (double)src[i * 3 + 2]};
    const double q[3] = {(double)ys[j * 3], (double)ys[j * 3 + 1], (double)ys[j * 3 + 2]};
    if constexpr (EST == kRegPointToPlane) {
      const double nr[3] = {(double)ns[j * 3], (double)ns[j * 3 + 1], (double)ns[j * 3 + 2]};
      const double p[3] = {x[0] - px[0], x[1] - px[1], x[2] - px[2]};
      const double rho = ((x[0] - q[0]) * nr[0] + (x[1] - q[1]) * nr[1]) + (x[2] - q[2]) * nr[2];
      const double J[6] = {p[1] * nr[2] - p[2] * nr[1], p[2] * nr[0] - p[0] * nr[2], p[0] * nr[1] - p[1] * nr[0],
                           nr[0], nr[1], nr[2]};
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) acc[icp_upper(r, c)] += J[r] * J[c];
        acc[kIcpUpper + r] -= J[r] * rho;
      }
    } else {
      const double xc[3] = {x[0] - px[0], x[1] - px[1], x[2] - px[2]};
      const double yc[3] = {q[0] - py[0], q[1] - py[1], q[2] - py[2]};
      pa_accumulate<3>(acc, 1.0, xc, yc);  // weights 1 / 0: every product by 1.0 is exact
    }
  }
  pa_block_sum<M>(acc, s_part, partials + ((int64_t)n * nb + blockIdx.x) * M);
}

template <int EST>
__global__ __launch_bounds__(kWave) void registration_solve_kernel(
    const float* __restrict__ X_init, const float* __restrict__ Xt, const float* __restrict__ Y,
    const int64_t* __restrict__ lengths_x, int P1, int P2, int nb, const double* __restrict__ partials, int update,
    int first, double relative_fitness, double relative_rmse, double* __restrict__ state,
    int32_t* __restrict__ status, int32_t* __restrict__ iterations, int32_t* __restrict__ updated,
    float* __restrict__ R, float* __restrict__ T, float* __restrict__ fitness, float* __restrict__ inlier_rmse,
    int64_t* __restrict__ num_correspondences, double* __restrict__ moments) {
  constexpr int M = kRegMoments;
  __shared__ double s_mom[M];
  const int n = blockIdx.x;
  const bool live = status[n] == kRegRunning;
  pa_sum_partials<M>(partials + (int64_t)n * nb * M, nb, live, s_mom,
                     moments != nullptr ? moments + (int64_t)n * kRegMomentsOut : nullptr);
  if (threadIdx.x != 0) return;
  double* __restrict__ st = state + (int64_t)n * kRegState;
  double Rd[3][3], Td[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    Td[a] = st[9 + a];
#pragma unroll
    for (int b = 0; b < 3; ++b) Rd[a][b] = st[a * 3 + b];
  }
  int moved = 0;
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the solved (alpha, beta, gamma, t): zeros where nothing was solved
  if (live) {
    const int64_t len = clamped_length<int64_t>(lengths_x, n, P1);
    const int64_t c = (int64_t)s_mom[kRegCount];
    const float fit = (float)((double)c / (double)(len > 1 ? len : 1));
    const float rmse = (float)sqrt(s_mom[kRegSumD2] / (double)(c > 1 ? c : 1));
    const bool settled = !first && fabs((double)fit - st[12]) < relative_fitness &&
                         fabs((double)rmse - st[13]) < relative_rmse;
    st[12] = (double)fit;
    st[13] = (double)rmse;
    num_correspondences[n] = c;
    if (settled) {
      status[n] = 0;
    } else if (update) {
      bool ok = c >= (EST == kRegPointToPlane ? kIcpMinPlane : kIcpMinPoint);
      if constexpr (EST == kRegPointToPlane) {
        ok = ok && icp_cholesky_solve6(s_mom, s_mom + kIcpUpper, x);
        if (ok) {
          const float* __restrict__ row0 = Xt + (int64_t)n * P1 * 3;
          const double c0[3] = {(double)row0[0], (double)row0[1], (double)row0[2]};  // (c >= 6: the cloud has rows)
          const double t[3] = {x[3], x[4], x[5]};
          double Rs[3][3];
          icp_rotation(x[0], x[1], x[2], Rs);
          icp_compose(Rd, Td, Rs, c0, t);
        }
      } else if (ok) {
        double px[3], py[3], s, sg[3];
        // pa_pivots' values (c >= 3: the cloud has rows), read unconditionally: the call costs this kernel 6 VGPRs and a
        // wave of occupancy
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          px[d] = (double)X_init[(int64_t)n * P1 * 3 + d];
          py[d] = (double)Y[(int64_t)n * P2 * 3 + d];
        }
        pa_solve<3>(s_mom, px, py, false, false, 1e-9, Rd, Td, s, sg);
      }
      if (ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          st[9 + a] = Td[a];
#pragma unroll
          for (int b = 0; b < 3; ++b) st[a * 3 + b] = Rd[a][b];
        }
        iterations[n] += 1;
        moved = 1;
      } else {
        status[n] = 1;
      }
    }
  }
  updated[n] = moved;
  if (moments != nullptr) {
#pragma unroll
    for (int k = 0; k < 6; ++k) moments[(int64_t)n * kRegMomentsOut + kRegMoments + k] = moved ? x[k] : 0.0;
  }
  fitness[n] = (float)st[12];
  inlier_rmse[n] = (float)st[13];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    T[(int64_t)n * 3 + a] = (float)Td[a];
#pragma unroll
    for (int b = 0; b < 3; ++b) R[((int64_t)n * 3 + a) * 3 + b] = (float)Rd[a][b];
  }
}

// Xt = X_init R + T (fp32; zero rows past the length) of the clouds whose transform this step moved
__global__ __launch_bounds__(kPaBlock) void registration_apply_kernel(
    const float* __restrict__ X_init, const int64_t* __restrict__ lengths_x, const int32_t* __restrict__ updated,
    const float* __restrict__ R, const float* __restrict__ T, int P1, float* __restrict__ Xt) {
  const int n = blockIdx.y, nb = gridDim.x;
  if (!updated[n]) return;
  const int64_t len = clamped_length<int64_t>(lengths_x, n, P1);
  float r[3][3], t[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t[a] = T[(int64_t)n * 3 + a];
#pragma unroll
    for (int b = 0; b < 3; ++b) r[a][b] = R[((int64_t)n * 3 + a) * 3 + b];
  }
  const float* __restrict__ xs = X_init + (int64_t)n * P1 * 3;
  float* __restrict__ xt = Xt + (int64_t)n * P1 * 3;
  for (int64_t i = (int64_t)blockIdx.x * kPaBlock + threadIdx.x; i < P1; i += (int64_t)nb * kPaBlock)
    reg_apply_row(xs, xt, i, len, r, t);
}

// all_frozen[0] = no cloud is still running.  One block.
__global__ __launch_bounds__(kPaBlock) void registration_frozen_kernel(const int32_t* __restrict__ status, int N,
                                                                       int32_t* __restrict__ all_frozen) {
  int running = 0;
  for (int n = threadIdx.x; n < N; n += kPaBlock) running |= status[n] == kRegRunning;
  const int any = __syncthreads_or(running);
  if (threadIdx.x == 0) all_frozen[0] = any ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------ host side
struct RegistrationLayout {
  double* partials;   // (N, nb, kRegMoments)
  int32_t* updated;   // (N,)
  size_t bytes;
};

static RegistrationLayout registration_layout(void* ws, int64_t N, int64_t P1) {
  Carver c(ws);
  RegistrationLayout l;
  l.partials = (double*)c.take(sizeof(double) * (size_t)N * (size_t)pa_blocks(P1) * kRegMoments);
  l.updated = (int32_t*)c.take(sizeof(int32_t) * (size_t)N);
  l.bytes = c.off;
  return l;
}

static bool registration_shape_ok(int64_t N, int64_t P1, int64_t P2) {
  return N >= 1 && N < 65536 && P1 >= 1 && P1 < (1LL << 30) && P2 >= 1 && P2 < (1LL << 30);
}

}  // namespace pointops

using namespace pointops;

// the `search_version` a run passes to every one of its steps: knn_points' own choice by shape, or (POINTOPS_DEBUG
// registration_grid=1, tests) the grid family whatever the size.  A run asks ONCE, so that a change of the environment
// between two steps cannot send a step to a workspace built for another family
extern "C" int pointops_registration_search_version(void) {
  return debug_knob("registration_grid", -1) == 1 ? 3 : -1;
}

extern "C" size_t pointops_registration_workspace_bytes(int64_t N, int64_t P1) {
  if (!registration_shape_ok(N, P1, 1)) return 0;
  return registration_layout(nullptr, N, P1).bytes;
}

extern "C" int pointops_registration_step(
    const float* X_init, const float* Y, const float* target_normals, const int64_t* lengths_x,
    const int64_t* lengths_y, const float* R_init, const float* T_init, int64_t N, int64_t P1, int64_t P2,
    float max_correspondence_distance, double relative_fitness, double relative_rmse, int estimation, int update,
    int first, int reuse, int search_version, float* Xt, double* state, int32_t* status, int32_t* iterations, int64_t* idx, float* dists,
    int64_t* correspondences, int64_t* num_correspondences, float* R, float* T, float* fitness, float* inlier_rmse,
    int32_t* all_frozen, double* moments, void* knn_workspace, size_t knn_workspace_bytes, void* workspace,
    size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(registration_shape_ok(N, P1, P2), "registration_step: need 1 <= N < 65536 and 1 <= P1, P2 < 2^30");
  POINTOPS_REQUIRE(lengths_x != nullptr && lengths_y != nullptr, "registration_step: lengths are required");
  POINTOPS_REQUIRE(estimation == kRegPointToPoint || estimation == kRegPointToPlane,
                   "registration_step: estimation is 0 (point to point) or 1 (point to plane)");
  POINTOPS_REQUIRE(estimation != kRegPointToPlane || target_normals != nullptr,
                   "registration_step: point to plane needs target_normals");
  POINTOPS_REQUIRE(reuse == 0 || reuse == 1, "registration_step: reuse is 0 or 1");
  POINTOPS_REQUIRE(max_correspondence_distance > 0.0f && max_correspondence_distance <= 3.4028234663852886e38f,
                   "registration_step: max_correspondence_distance must be finite and > 0");
  hipStream_t stream = (hipStream_t)stream_;
  const RegistrationLayout l = registration_layout(workspace, N, P1);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "registration_step: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  const bool bounded = search_version == POINTOPS_REGISTRATION_SEARCH_BOUNDED;
  POINTOPS_REQUIRE(bounded || search_version == -1 || pointops_knn_check_version(search_version, 3, 1),
                   "registration_step: search_version is -1, a version of knn_points valid for D = 3, K = 1, or "
                   "POINTOPS_REGISTRATION_SEARCH_BOUNDED");
  const int version = search_version;
  const size_t knn_need = bounded ? pointops_knn_in_radius_workspace_bytes(N, P1, P2, 3, 1)
                                  : pointops_knn_workspace_bytes(N, P1, P2, 3, 1, version);
  // (before anything is launched)
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(knn_workspace, knn_workspace_bytes, knn_need),
                             "registration_step: search workspace of %zu bytes, need %zu", knn_workspace_bytes,
                             knn_need);
  const int nb = pa_blocks(P1);
  const dim3 rows((unsigned)nb, (unsigned)N);
  if (first) {
    hipLaunchKernelGGL(registration_init_kernel, rows, dim3(kPaBlock), 0, stream, X_init, lengths_x, R_init, T_init,
                       (int)P1, Xt, state, status, iterations);
  }
  int rc = bounded ? pointops_knn_in_radius(Xt, Y, lengths_x, lengths_y, N, P1, P2, 3, 1, max_correspondence_distance,
                                            idx, dists, nullptr, knn_workspace, knn_workspace_bytes, reuse, stream_)
                   : pointops_knn_points_idx_reuse(Xt, Y, lengths_x, lengths_y, N, P1, P2, 3, 2, 1, version, idx, dists,
                                                   knn_workspace, knn_workspace_bytes, reuse, stream_);
  if (rc != POINTOPS_OK) return rc;
  const float r2 = max_correspondence_distance * max_correspondence_distance;
  with_exact<kRegPointToPlane>(Ints<kRegPointToPoint>{}, estimation, [&](auto Ec) {
    constexpr int kE = decltype(Ec)::value;
    hipLaunchKernelGGL((registration_moments_kernel<kE>), rows, dim3(kPaBlock), 0, stream, X_init, (const float*)Xt,
                       Y, target_normals, (const int64_t*)idx, (const float*)dists, lengths_x, lengths_y,
                       (const int32_t*)status, (int)P1, (int)P2, r2, correspondences, l.partials);
    hipLaunchKernelGGL((registration_solve_kernel<kE>), dim3((unsigned)N), dim3(kWave), 0, stream, X_init,
                       (const float*)Xt, Y, lengths_x, (int)P1, (int)P2, nb, (const double*)l.partials, update, first,
                       relative_fitness, relative_rmse, state, status, iterations, l.updated, R, T, fitness,
                       inlier_rmse, num_correspondences, moments);
  });
  if (update) {
    hipLaunchKernelGGL(registration_apply_kernel, rows, dim3(kPaBlock), 0, stream, X_init, lengths_x,
                       (const int32_t*)l.updated, (const float*)R, (const float*)T, (int)P1, Xt);
  }
  hipLaunchKernelGGL(registration_frozen_kernel, dim3(1), dim3(kPaBlock), 0, stream, (const int32_t*)status, (int)N,
                     all_frozen);
  return check_launch("registration_step");
}

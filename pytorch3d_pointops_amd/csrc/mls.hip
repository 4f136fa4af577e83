// mls.hip -- moving-least-squares smoothing of a batch of clouds (C ABI: pointops_mls_smooth; device half of
// functions/mls.py).  The definition is the comment block of the entry in include/pointops_amd.h: the support of a point
// is ball query's `dist2 < r * r`, every member carries the quartic weight (1 - d2 / r2)^4 quantized to 12 bits, the
// weighted moments of the quantized offsets are summed in INTEGERS (so the sum does not depend on the order of the
// walk), the plane comes from sym3_eigen_f64 of their covariance, and the point moves along the plane's normal onto it.
//
// A fixed sequence of launches per pass, stream-ordered, nothing read back, no atomics beyond grid_build's:
//   prepare   radius_walk_prepare with cell_radius = r over the pass's input: the lengths clamped into [0, P], and for
//             clouds of 512 points and more a grid (the points move between passes, so every pass builds its own)
//   smooth    one lane per point in cell order, one full walk: per hit the weight, three quantized offsets and eleven
//             int64 accumulators; then offset, covariance, eigenvectors, status, projection -> every output at the
//             point's own index
// Pass k of `iterations` reads what pass k - 1 wrote: the passes ping-pong between points_out and one workspace buffer
// such that the last one writes points_out; normals, curvature, num_neighbors, status (and moments) are rewritten by
// every pass, so the last one's stay.  Padding rows are written by the smooth launch itself.  A lane without
// radius_walk.h's certificate, a refused grid and a small cloud walk all pairs, which never changes a result.
// POINTOPS_DEBUG=mls_grid=0|1 forces either path.
#include <limits.h>

#include "mls_fit.h"
#include "radius_walk.h"
#include "small_solvers.h"

namespace pointops {

struct MlsParams {
  double s;  // mls_scale(r)
  int min_neighbors;
};

// Six waves per SIMD: 80 VGPRs without scratch, 2-3 % faster than the compiler's own 90 VGPRs / five waves at
// 16 x 131072 points in alternating runs; eight waves would spill (profiles/mls_resources.txt).
constexpr int kMlsWavesPerSimd = 6;

__global__ __launch_bounds__(kWalkBlock, kMlsWavesPerSimd) void mls_smooth_kernel(
    WalkView v, MlsParams p, float* __restrict__ points_out, float* __restrict__ normals, float* __restrict__ curvature,
    int64_t* __restrict__ num_neighbors, uint8_t* __restrict__ status, int64_t* __restrict__ moments) {
  const WalkItem it = walk_item(v);
  if (it.t >= v.P) return;
  const int64_t base = (int64_t)it.n * v.P;
  if (it.t >= it.len) {  // padding rows
    float* const po = points_out + (base + it.t) * 3;
    float* const no = normals + (base + it.t) * 3;
    po[0] = po[1] = po[2] = 0.0f;
    no[0] = no[1] = no[2] = 0.0f;
    curvature[base + it.t] = 0.0f;
    num_neighbors[base + it.t] = 0;
    status[base + it.t] = 0;
    if (moments != nullptr)
      for (int k = 0; k < kMlsMoments; ++k) moments[(base + it.t) * kMlsMoments + k] = 0;
    return;
  }
  const WalkLane<3> L = walk_lane<3>(v, it);
  MlsSums sum;
  radius_walk_records<3>(v, it, L, [&](int, const float4& c, int) {
    // (the walk's own distance, formed again by the same expression: the compiler keeps one)
    mls_accumulate(sum, mls_weight(point_dist<3, 2>(L.x, L.y, L.z, c), v.r2), iss_quantize(c.x, L.x, p.s),
                   iss_quantize(c.y, L.y, p.s), iss_quantize(c.z, L.z, p.s));
    return true;
  });
  const float x[3] = {L.x, L.y, L.z};
  float po[3] = {L.x, L.y, L.z}, no[3] = {0.0f, 0.0f, 0.0f}, curv = 0.0f;
  uint8_t st = 1;
  if (sum.n >= p.min_neighbors) {
    double C[6], a[3][3], l[3], vec[3][3], delta[3];
    iss_covariance(sum.M1, sum.M2, sum.W, p.s, C);
    a[0][0] = C[0], a[0][1] = a[1][0] = C[1], a[0][2] = a[2][0] = C[2];
    a[1][1] = C[3], a[1][2] = a[2][1] = C[4], a[2][2] = C[5];
    sym3_eigen_f64(a, l, vec);
    st = mls_status(sum.n, p.min_neighbors, l);
    if (st == 0) {
      mls_offset(sum.M1, sum.W, p.s, delta);
      mls_project(x, delta, l, vec, po, no, curv);
    }
  }
  const int64_t row = base + L.i;
  points_out[row * 3 + 0] = po[0], points_out[row * 3 + 1] = po[1], points_out[row * 3 + 2] = po[2];
  normals[row * 3 + 0] = no[0], normals[row * 3 + 1] = no[1], normals[row * 3 + 2] = no[2];
  curvature[row] = curv;
  num_neighbors[row] = sum.n;
  status[row] = st;
  if (moments != nullptr) {
    int64_t* const m = moments + row * kMlsMoments;
    m[0] = sum.W;
    for (int k = 0; k < 3; ++k) m[1 + k] = sum.M1[k];
    for (int k = 0; k < 6; ++k) m[4 + k] = sum.M2[k];
  }
}

static bool mls_shape_ok(int64_t N, int64_t P, int64_t iterations) {
  // (a cloud is a grid's y coordinate; 2^20 hits keep the int64 moments below 2^63: mls_fit.h)
  return N >= 0 && N < 65536 && P >= 0 && P <= kMlsMaxPoints && iterations >= 1 && iterations <= 65536;
}

struct MlsLayout {
  WalkLayout walk;
  float* moved;  // (N, P, 3) the other end of the ping-pong; absent for one pass
  size_t bytes;
};

static MlsLayout mls_layout(void* ws, int64_t N, int64_t P, int64_t iterations) {
  Carver c(ws);
  MlsLayout l;
  l.walk = radius_walk_carve(c, "mls_grid", N, P);
  l.moved = (float*)c.take(iterations > 1 ? sizeof(float) * 3 * (size_t)N * (size_t)P : 0);
  l.bytes = c.off;
  return l;
}

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_mls_workspace_bytes(int64_t N, int64_t P, int64_t iterations) {
  if (!mls_shape_ok(N, P, iterations) || N == 0) return 0;
  return mls_layout(nullptr, N, P, iterations).bytes;
}

extern "C" int pointops_mls_smooth(const float* points, const int64_t* lengths, int64_t N, int64_t P, float radius,
                                   int64_t min_neighbors, int64_t iterations, float* points_out, float* normals,
                                   float* curvature, int64_t* num_neighbors, uint8_t* status, int64_t* moments,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(mls_shape_ok(N, P, iterations),
                   "mls_smooth: need 0 <= N < 65536, 0 <= P <= 2^20 and 1 <= iterations <= 65536");
  POINTOPS_REQUIRE(radius > 0.0f && radius <= FLT_MAX, "mls_smooth: need a finite radius > 0");
  POINTOPS_REQUIRE(min_neighbors >= 0, "mls_smooth: need min_neighbors >= 0");
  if (N == 0) return POINTOPS_OK;
  const MlsLayout l = mls_layout(workspace, N, P, iterations);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "mls_smooth: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  MlsParams p;
  p.s = mls_scale(radius);
  p.min_neighbors = (int)(min_neighbors > INT_MAX ? INT_MAX : min_neighbors);
  const dim3 pgrid((unsigned)ceil_div(P, kWalkBlock), (unsigned)N);
  const float* src = points;
  for (int64_t pass = 0; pass < iterations; ++pass) {
    // the last pass writes points_out, the one before it the workspace buffer, and so on back
    float* const dst = (iterations - 1 - pass) % 2 == 0 ? points_out : l.moved;
    WalkView v;
    const int rc = radius_walk_prepare(l.walk, src, lengths, N, P, 3, radius, stream, &v);
    if (rc != POINTOPS_OK) return rc;
    if (P == 0) return check_launch("mls_smooth");
    v.r2 = radius * radius;  // an fp32 product, as ball query's radius2
    hipLaunchKernelGGL(mls_smooth_kernel, pgrid, dim3(kWalkBlock), 0, stream, v, p, dst, normals, curvature,
                       num_neighbors, status, moments);
    src = dst;
  }
  return check_launch("mls_smooth");
}

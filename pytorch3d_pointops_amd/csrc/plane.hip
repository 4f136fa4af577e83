// plane.hip -- RANSAC plane extraction: the dominant plane of every cloud (floor, road, table, wall), found from
// thousands of three-point hypotheses scored against every valid point, the winner refitted on its inliers.  Device
// half of functions/plane.py; the definition is the comment of pointops_segment_plane in include/pointops_amd.h.
//
// The torch composition it replaces builds an (N, H, P) residual tensor.  Here nothing of that size exists:
//
//   1. compaction (consensus.h over PlaneRows)   the valid rows of a cloud, in ascending order, as 16-byte records
//      (x, y, z, row), and their number M_n.
//   2. plane_hypotheses_kernel   one lane per (cloud, hypothesis): draws three distinct records (or reads the caller's
//      rows) and forms the plane in fp64 with its validity tests (plane_hypothesis.h).
//   3. plane_score_kernel        the hot path, H M residuals per cloud.  One lane = HPL hypotheses with (a, b, c, d) in
//      4 VGPRs each and an integer counter.  Every lane of a wave consumes the SAME record, whose address is built from
//      blockIdx and the loop counter only, so the records arrive through the scalar path (s_load_dwordx4 into SGPRs) and
//      feed the VALU as scalar operands -- or, the form the entry launches, through an LDS tile the workgroup fills once
//      and every lane reads at the same address.  blockIdx.y splits the records of a cloud into chunks of kPlaneChunk;
//      each (chunk, hypothesis) writes one int32.  POINTOPS_DEBUG="plane_lds=0|1" picks the path, "plane_hpl=1|2" the
//      hypotheses per lane (default 2 above 256 hypotheses): the A/B of DESIGN 4.10.
//   4. selection (consensus.h)    the largest count at the lowest index; plane_select_kernel copies the winning plane
//      into the candidate.
//   5. plane_evaluate_kernel / plane_finish_kernel   mask, count, fp64 block partials of sum r^2 and of the moments of
//      the inliers about a pivot; one finishing block per cloud applies the accept rule (consensus.h), writes the
//      public outputs and solves the next candidate from the moments (ph_refit: covariance, sym3_eigen_f64, sign rule).
//
// No atomics, no host read-back: bit-reproducible and capturable into a HIP graph.
#include "common.h"
#include "consensus.h"
#include "debug.h"
#include "plane_hypothesis.h"

namespace pointops {

constexpr int kPlaneChunk = 512;  // records per scoring block (exported: pointops_plane_chunk)
constexpr int kPlPart = kPlaneMoments;  // doubles per evaluation partial: sum r^2, S q (3), S q q^T (6)

__device__ __forceinline__ bool pl_row_valid(const uint8_t* __restrict__ mask, int n, int P, int64_t i, int len) {
  return i >= 0 && i < len && (mask == nullptr || mask[(int64_t)n * P + i] != 0);
}

// ---------------------------------------------------------------------------------------------------- 1. compaction
// The row source of the compaction: a valid row's key is 0.
struct PlaneRows {
  using Record = float4;
  const float* points;
  const int64_t* lengths;
  const uint8_t* mask;
  int P, len;
  __device__ __forceinline__ void enter(int n) { len = clamped_length(lengths, n, P); }
  __device__ __forceinline__ int key(int n, int i) const { return pl_row_valid(mask, n, P, i, len) ? 0 : -1; }
  __device__ __forceinline__ void store(float4* __restrict__ out, int at, int n, int i, int) const {
    const float* __restrict__ p = points + (int64_t)n * P * 3 + (int64_t)i * 3;
    out[at] = make_float4(p[0], p[1], p[2], __int_as_float(i));
  }
};

// ---------------------------------------------------------------------------------------------------- 2. hypotheses
__global__ __launch_bounds__(kCsBlock) void plane_hypotheses_kernel(
    const float* __restrict__ points, const int64_t* __restrict__ lengths, const uint8_t* __restrict__ mask,
    const int64_t* __restrict__ samples_in, int P, int H, int64_t seed, int64_t first_cloud, PlaneCone cone,
    const float4* __restrict__ records, const int* __restrict__ num_valid, float4* __restrict__ ws_plane,
    int* __restrict__ ws_valid, float* __restrict__ hyp_planes, int64_t* __restrict__ samples_out) {
  const int n = blockIdx.y;
  const int h = blockIdx.x * kCsBlock + (int)threadIdx.x;
  if (h >= H) return;
  const int64_t slot = (int64_t)n * H + h;
  float p[3][3];
  int64_t rows[3] = {-1, -1, -1};
  bool valid;
  if (samples_in != nullptr) {
    const int len = clamped_length(lengths, n, P);
    valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      rows[k] = samples_in[slot * 3 + k];
      const bool ok = pl_row_valid(mask, n, P, rows[k], len);
      valid = valid && ok;
#pragma unroll
      for (int d = 0; d < 3; ++d) p[k][d] = ok ? points[((int64_t)n * P + rows[k]) * 3 + d] : 0.0f;
    }
    valid = valid && rows[0] != rows[1] && rows[0] != rows[2] && rows[1] != rows[2];
  } else {
    const int M = num_valid[n];
    valid = M >= 3;
    uint32_t at[3] = {0u, 0u, 0u};
    if (valid) rh_draw(seed, first_cloud + n, h, (uint32_t)M, at);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (valid) {
        r = records[(int64_t)n * P + at[k]];
        rows[k] = __float_as_int(r.w);
      }
      p[k][0] = r.x;
      p[k][1] = r.y;
      p[k][2] = r.z;
    }
  }
  float plane[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (valid) valid = ph_plane(p, cone, plane);
  ws_valid[slot] = valid ? 1 : 0;
  ws_plane[slot] = make_float4(plane[0], plane[1], plane[2], plane[3]);
  if (hyp_planes != nullptr) ((float4*)hyp_planes)[slot] = make_float4(plane[0], plane[1], plane[2], plane[3]);
  if (samples_out != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) samples_out[slot * 3 + k] = rows[k];
  }
}

// ---------------------------------------------------------------------------------------------------- 3. scoring
// LDS = false (POINTOPS_DEBUG="plane_lds=0"): the scalar path.  LDS = true, the default: the workgroup copies its chunk
// into an LDS tile and every lane reads the same address (a broadcast).  HPL hypotheses per lane: lane t of tile b owns hypotheses
// (b HPL + k) 256 + t, so every record fetched feeds HPL residuals per lane.  The results are the same in every form.
template <bool LDS, int HPL>
__global__ __launch_bounds__(kCsBlock) void plane_score_kernel(
    const float4* __restrict__ records, const int* __restrict__ num_valid, const float4* __restrict__ ws_plane,
    const int* __restrict__ ws_valid, int P, int H, int S, float thr, int* __restrict__ partials) {
  __shared__ float4 s_rec[LDS ? kPlaneChunk : 1];
  const int n = blockIdx.z, chunk = blockIdx.y;  // wave-uniform
  const int M = num_valid[n];
  const int beg = chunk * kPlaneChunk;
  if (beg >= M) return;  // (workgroup-uniform; count reads the chunks below ceil(M / chunk) only)
  const int end = min(beg + kPlaneChunk, M);
  const float4* __restrict__ rec = records + (int64_t)n * P;
  if constexpr (LDS) {
    for (int t = threadIdx.x; t < end - beg; t += kCsBlock) s_rec[t] = rec[beg + t];
    __syncthreads();
  }
  int h[HPL];
  bool valid[HPL], any = false;
#pragma unroll
  for (int k = 0; k < HPL; ++k) {
    h[k] = (blockIdx.x * HPL + k) * kCsBlock + (int)threadIdx.x;
    valid[k] = h[k] < H && ws_valid[(int64_t)n * H + h[k]] != 0;
    any = any || valid[k];
  }
  int* __restrict__ out = partials + ((int64_t)n * S + chunk) * H;
  if (__ballot(any) == 0ull) {  // the whole wave is invalid
#pragma unroll
    for (int k = 0; k < HPL; ++k)
      if (h[k] < H) out[h[k]] = -1;
    return;
  }
  float4 pl[HPL];
  int count[HPL];
#pragma unroll
  for (int k = 0; k < HPL; ++k) {
    pl[k] = valid[k] ? ws_plane[(int64_t)n * H + h[k]] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    count[k] = 0;
  }
  if constexpr (LDS) {
#pragma unroll 8
    for (int j = 0; j < end - beg; ++j) {
      const float4 r = s_rec[j];
#pragma unroll
      for (int k = 0; k < HPL; ++k)
        count[k] += fabsf(ph_residual(pl[k].x, pl[k].y, pl[k].z, pl[k].w, r.x, r.y, r.z)) <= thr ? 1 : 0;
    }
  } else {
#pragma unroll 8
    for (int j = beg; j < end; ++j) {  // a uniform address: the record arrives in SGPRs
      const float4 r = rec[j];
#pragma unroll
      for (int k = 0; k < HPL; ++k)
        count[k] += fabsf(ph_residual(pl[k].x, pl[k].y, pl[k].z, pl[k].w, r.x, r.y, r.z)) <= thr ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < HPL; ++k)
    if (h[k] < H) out[h[k]] = valid[k] ? count[k] : -1;
}

// ---------------------------------------------------------------------------------------------------- 4. selection
__global__ __launch_bounds__(kCsBlock) void plane_select_kernel(
    const unsigned long long* __restrict__ tile_keys, int tiles, const float4* __restrict__ ws_plane, int H,
    int64_t* __restrict__ best, float4* __restrict__ cand_plane, int* __restrict__ cand_ok) {
  const int n = blockIdx.x;
  const int64_t b = cs_best(tile_keys, tiles, n);
  if (threadIdx.x != 0) return;
  best[n] = b;
  cand_ok[n] = b < 0 ? 0 : 1;
  cand_plane[n] = b < 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : ws_plane[(int64_t)n * H + b];
}

// ---------------------------------------------------------------------------------------------------- 5. evaluation
// Mask (one byte per row), count, sum of r^2 and -- MOMENTS: a refit follows -- the moments about the pivot over the
// inliers of the candidate plane of every cloud.  The pivot is the cloud's first valid row (record 0).
template <bool MOMENTS>
__global__ __launch_bounds__(kCsBlock) void plane_evaluate_kernel(
    const float* __restrict__ points, const int64_t* __restrict__ lengths, const uint8_t* __restrict__ mask,
    const float4* __restrict__ cand_plane, const int* __restrict__ cand_ok, const float4* __restrict__ records,
    const int* __restrict__ num_valid, const int* __restrict__ stopped, int first, int P, float thr,
    uint8_t* __restrict__ cand_mask, double* __restrict__ part, int* __restrict__ part_count) {
  constexpr int kSums = MOMENTS ? kPlPart : 1;
  const int n = blockIdx.y, nb = gridDim.x;
  const int len = clamped_length(lengths, n, P);
  // a cloud that has stopped keeps the mask it accepted: its candidate is not evaluated and nothing is written over
  const bool skip = !first && stopped[n] != 0;
  const bool none = skip || cand_ok[n] == 0 || num_valid[n] == 0;
  const float4 pl = cand_plane[n];
  float4 pivot = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (MOMENTS && !none) pivot = records[(int64_t)n * P];
  const float* __restrict__ ps = points + (int64_t)n * P * 3;
  double sum[kSums];
#pragma unroll
  for (int m = 0; m < kSums; ++m) sum[m] = 0.0;
  int cnt = 0;
  for (int i = blockIdx.x * kCsBlock + (int)threadIdx.x; i < P; i += nb * kCsBlock) {
    bool in = false;
    if (!none && pl_row_valid(mask, n, P, i, len)) {
      const float x = ps[(int64_t)i * 3], y = ps[(int64_t)i * 3 + 1], z = ps[(int64_t)i * 3 + 2];
      const float r = ph_residual(pl.x, pl.y, pl.z, pl.w, x, y, z);
      in = fabsf(r) <= thr;
      if (in) {
        sum[0] += (double)r * (double)r;
        if constexpr (MOMENTS) {
          const double q0 = (double)x - (double)pivot.x, q1 = (double)y - (double)pivot.y,
                       q2 = (double)z - (double)pivot.z;
          sum[1] += q0;
          sum[2] += q1;
          sum[3] += q2;
          sum[4] += q0 * q0;
          sum[5] += q0 * q1;
          sum[6] += q0 * q2;
          sum[7] += q1 * q1;
          sum[8] += q1 * q2;
          sum[9] += q2 * q2;
        }
      }
    }
    cnt += in ? 1 : 0;
    if (!skip) cand_mask[(int64_t)n * P + i] = in ? 1 : 0;
  }
  const int64_t slot = (int64_t)n * nb + blockIdx.x;
  cs_block_partials(sum, cnt, nb, part + (int64_t)n * kPlPart * nb + blockIdx.x, part_count + slot);
}

// One block per cloud: the accept rule and -- on acceptance -- the public plane, count and rmse and the buffer that
// holds the accepted mask; with `more` (another refit follows) thread 0 then solves the next candidate from the moments
// of the mask it has just accepted.
__global__ __launch_bounds__(kCsBlock) void plane_finish_kernel(
    const double* __restrict__ part, const int* __restrict__ part_count, int nb, int first, int more,
    const int64_t* __restrict__ best, float4* __restrict__ cand_plane, int* __restrict__ cand_ok,
    int buffer, const float4* __restrict__ records, const int* __restrict__ num_valid, int P, PlaneCone cone,
    int* __restrict__ stopped, int* __restrict__ which, float* __restrict__ planes, int64_t* __restrict__ num_inliers,
    float* __restrict__ rmse) {
  __shared__ double s_part[kCsMaxBlocks * kPlPart];  // (one load per thread instead of nb dependent rounds in thread 0)
  const int n = blockIdx.x;
  if (more) {
    for (int t = threadIdx.x; t < nb * kPlPart; t += kCsBlock) s_part[t] = part[(int64_t)n * nb * kPlPart + t];
  }
  int cnt;
  double sum;  // (the barrier of cs_accept also completes s_part; cand_ok is read before thread 0 writes it)
  const bool usable = cand_ok[n] != 0;
  const double* __restrict__ sums = part + (int64_t)n * kPlPart * nb;  // (of r^2: row 0 of the cloud's partials)
  if (!cs_accept(sums, part_count, nb, n, first, usable, stopped, num_inliers, cnt, sum)) return;
  if (threadIdx.x == 0) {
    cs_publish(n, first, best, cnt, sum, stopped, num_inliers, rmse);
    which[n] = buffer;
    const float4 pl = cand_plane[n];
    ((float4*)planes)[n] = pl;
    if (more) {
      double mom[kPlaneMoments];
      mom[0] = (double)cnt;
#pragma unroll
      for (int m = 1; m < kPlaneMoments; ++m) mom[m] = 0.0;
      for (int b = 0; b < nb; ++b) {
#pragma unroll
        for (int m = 1; m < kPlaneMoments; ++m) mom[m] += s_part[m * nb + b];
      }
      float next[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      bool ok = false;
      if (num_valid[n] > 0) {
        const float4 pv = records[(int64_t)n * P];
        const double pivot[3] = {(double)pv.x, (double)pv.y, (double)pv.z};
        ok = ph_refit(mom, pivot, cone, next);
      }
      cand_plane[n] = make_float4(next[0], next[1], next[2], next[3]);
      cand_ok[n] = ok ? 1 : 0;
    }
  }
}

// The public mask: the candidate mask of the evaluation each cloud accepted last (which[n] names its buffer).
__global__ __launch_bounds__(kCsBlock) void plane_mask_kernel(
    const uint8_t* __restrict__ cand_mask, const int* __restrict__ which, int64_t N, int P, uint8_t* __restrict__ mask) {
  const int n = blockIdx.y;
  const uint8_t* __restrict__ src = cand_mask + ((int64_t)which[n] * N + n) * P;
  uint8_t* __restrict__ dst = mask + (int64_t)n * P;
  const int stride = gridDim.x * kCsBlock, at = blockIdx.x * kCsBlock + (int)threadIdx.x;
  if ((P & 15) == 0 && (((uintptr_t)mask | (uintptr_t)cand_mask) & 15) == 0) {  // sixteen rows per access
    for (int i = at; i < P / 16; i += stride) ((uint4*)dst)[i] = ((const uint4*)src)[i];
    return;
  }
  for (int i = at; i < P; i += stride) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------------ host side
struct PlaneLayout : CsLayout {
  float4* records;      // (N, P)
  float4* hyp_plane;    // (N, H)
  float4* cand_plane;   // (N,)
  int* cand_ok;         // (N,)
  uint8_t* cand_mask;   // (2, N, P): the evaluations alternate, so an accepted mask outlives the next candidate
  int* which;           // (N,) the buffer of the accepted mask
  double* part;         // (N, kPlPart, nb)
  size_t bytes;
};

static PlaneLayout plane_layout(void* ws, int64_t N, int64_t P, int64_t H) {
  Carver c(ws);
  PlaneLayout l;
  static_cast<CsLayout&>(l) = cs_layout(c, N, P, H, kPlaneChunk);
  const size_t n = (size_t)N, p = (size_t)P, h = (size_t)H;
  l.records = (float4*)c.take(sizeof(float4) * n * p);
  l.hyp_plane = (float4*)c.take(sizeof(float4) * n * h);
  l.cand_plane = (float4*)c.take(sizeof(float4) * n);
  l.cand_ok = (int*)c.take(sizeof(int) * n);
  l.cand_mask = (uint8_t*)c.take(2 * n * p);
  l.which = (int*)c.take(sizeof(int) * n);
  l.part = (double*)c.take(sizeof(double) * n * (size_t)cs_eval_blocks(P) * kPlPart);
  l.bytes = c.off;
  return l;
}

static bool plane_shape_ok(int64_t N, int64_t P, int64_t H) { return cs_shape_ok(N, P, H, kPlaneChunk); }

template <bool LDS, int HPL>
static void plane_launch_score(const PlaneLayout& l, int64_t N, int64_t P, int64_t H, unsigned S, float thr,
                               hipStream_t stream) {
  const unsigned tiles = (unsigned)ceil_div(H, (int64_t)kCsBlock * HPL);
  hipLaunchKernelGGL((plane_score_kernel<LDS, HPL>), dim3(tiles, S, (unsigned)N), dim3(kCsBlock), 0, stream,
                     (const float4*)l.records, (const int*)l.num_valid, (const float4*)l.hyp_plane,
                     (const int*)l.hyp_valid, (int)P, (int)H, (int)S, thr, l.partials);
}

}  // namespace pointops

using namespace pointops;

extern "C" int64_t pointops_plane_chunk(void) { return kPlaneChunk; }

extern "C" size_t pointops_plane_workspace_bytes(int64_t N, int64_t P, int64_t H) {
  if (!plane_shape_ok(N, P, H)) return 0;
  return plane_layout(nullptr, N, P, H).bytes;
}

extern "C" int pointops_segment_plane(
    const float* points, const int64_t* lengths, const uint8_t* mask, const int64_t* samples_in, int64_t N, int64_t P,
    int64_t H, int64_t seed, int64_t first_cloud, float distance_threshold, int use_axis, float axis_x, float axis_y,
    float axis_z, float cos_max_angle, int refine_steps, float* planes, uint8_t* inlier_mask, int64_t* num_inliers,
    float* rmse, int64_t* best, int32_t* counts, float* hyp_planes, int64_t* samples_out, void* workspace,
    size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(plane_shape_ok(N, P, H), "segment_plane: need 0 <= N < 65536, 0 <= P <= 65535 * 512 and 1 <= H <= 2^24");
  POINTOPS_REQUIRE(distance_threshold >= 0.0f && distance_threshold < INFINITY,
                   "segment_plane: need a finite distance_threshold >= 0");
  POINTOPS_REQUIRE(refine_steps >= 0 && first_cloud >= 0, "segment_plane: need refine_steps >= 0, first_cloud >= 0");
  if (use_axis) {
    const float sq = (axis_x * axis_x + axis_y * axis_y) + axis_z * axis_z;
    POINTOPS_REQUIRE(sq > 0.999f && sq < 1.001f && cos_max_angle >= 0.0f && cos_max_angle <= 1.0f,
                     "segment_plane: need a unit axis and 0 <= cos_max_angle <= 1");
  }
  if (N == 0) return POINTOPS_OK;
  const PlaneLayout l = plane_layout(workspace, N, P, H);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, l.bytes),
                             "segment_plane: workspace of %zu bytes, need %zu", workspace_bytes, l.bytes);
  hipStream_t stream = (hipStream_t)stream_;
  const float thr = distance_threshold;
  PlaneCone cone;
  cone.use = use_axis ? 1 : 0;
  cone.a[0] = use_axis ? axis_x : 0.0f;
  cone.a[1] = use_axis ? axis_y : 0.0f;
  cone.a[2] = use_axis ? axis_z : 0.0f;
  cone.cos_max = use_axis ? cos_max_angle : 0.0f;
  const CsGrid g(N, P, H, kPlaneChunk);
  const dim3 block(kCsBlock);
  const unsigned S = g.S;

  cs_launch_compact(PlaneRows{points, lengths, mask, (int)P, 0}, g, l, P, l.records, stream);
  hipLaunchKernelGGL(plane_hypotheses_kernel, g.hyp, block, 0, stream, points, lengths, mask, samples_in, (int)P,
                     (int)H, seed, first_cloud, cone, (const float4*)l.records, (const int*)l.num_valid, l.hyp_plane,
                     l.hyp_valid, hyp_planes, samples_out);
  if (S > 0) {
    // (the defaults are the winners of the A/B of DESIGN 4.10; a tile of hypotheses is 256 HPL wide)
    const bool lds = debug_knob("plane_lds", 1) != 0;
    const long hpl = debug_knob("plane_hpl", H > kCsBlock ? 2 : 1);
    if (lds && hpl == 2) plane_launch_score<true, 2>(l, N, P, H, S, thr, stream);
    else if (lds) plane_launch_score<true, 1>(l, N, P, H, S, thr, stream);
    else if (hpl == 2) plane_launch_score<false, 2>(l, N, P, H, S, thr, stream);
    else plane_launch_score<false, 1>(l, N, P, H, S, thr, stream);
  }
  cs_launch_count<kPlaneChunk>(g, l, H, counts, stream);
  hipLaunchKernelGGL(plane_select_kernel, g.cloud, block, 0, stream, (const unsigned long long*)l.tile_keys,
                     (int)g.tiles, (const float4*)l.hyp_plane, (int)H, best, l.cand_plane, l.cand_ok);
  int rc = check_launch("segment_plane");
  const int refits = P == 0 ? 0 : refine_steps;  // (no row, nothing to refit)
  for (int step = 0; step <= refits && rc == POINTOPS_OK; ++step) {
    const int more = step < refits ? 1 : 0;
    auto* evaluate = more ? plane_evaluate_kernel<true> : plane_evaluate_kernel<false>;
    hipLaunchKernelGGL(evaluate, g.eval, block, 0, stream, points, lengths, mask, (const float4*)l.cand_plane,
                       (const int*)l.cand_ok, (const float4*)l.records, (const int*)l.num_valid, (const int*)l.stopped,
                       step == 0 ? 1 : 0, (int)P, thr, l.cand_mask + (size_t)(step & 1) * (size_t)N * (size_t)P, l.part,
                       l.part_count);
    hipLaunchKernelGGL(plane_finish_kernel, g.cloud, block, 0, stream, (const double*)l.part,
                       (const int*)l.part_count, g.nb, step == 0 ? 1 : 0, more, (const int64_t*)best, l.cand_plane,
                       l.cand_ok, step & 1, (const float4*)l.records, (const int*)l.num_valid, (int)P, cone, l.stopped,
                       l.which, planes, num_inliers, rmse);
    rc = check_launch("segment_plane");
  }
  if (rc == POINTOPS_OK && P > 0) {
    hipLaunchKernelGGL(plane_mask_kernel, g.eval, block, 0, stream,
                       (const uint8_t*)l.cand_mask, (const int*)l.which, N, (int)P, inlier_mask);
    rc = check_launch("segment_plane");
  }
  return rc;
}

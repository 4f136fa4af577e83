// neighbor_attention.hip -- NEIGHBOUR ATTENTION (gfx950): softmax attention of every query row over the K rows its
// neighbour table names, per head, without the two (N, L, K, C) tensors of knn_gather(k), knn_gather(v), and its
// backward.  The definition is the NEIGHBOUR ATTENTION block of include/pointops_amd.h; neighbor_attention.h has the
// split of the heads over the lanes.
//
// Like neighbor_reduce.hip the work is a gather bound by memory traffic: every query has its own K rows of k and of v,
// each used once, so there is no operand a matrix instruction could reuse and nothing to keep in LDS but the table and
// the bias.  What the kernels are built for is 16-byte traffic, loads in flight, and per-head sums that stay in a wave:
//   forward   a group of G lanes per query row, a head on Gh = D / 4 consecutive lanes, Hg = G / Gh heads at a time.
//             The 256 / G rows of a workgroup own CONSECUTIVE table entries: the workgroup reads them once, coalesced,
//             checks them and leaves int32 sources (-1 = masked) and the bias of the heads in flight in LDS.  The slot
//             loop is unrolled by kNaUnroll: the k row and the v row of four slots are requested (eight 16-byte loads)
//             before the first dot.  Per slot: the per-head dot (4 products per lane, then wave_sum<Gh>), the running
//             maximum, one rescale of the running sum and of the accumulator, p v added.  One division per channel at
//             the end, 16-byte stores, lse by the first lane of a head.  Nothing of size K C ever exists.
//   grad A    the same split and staging, one pass: delta = g . out up front, per slot p = exp(s - lse), dP = g . v,
//             ds = p (dP - delta), grad_q += ds k_row with the k row already in registers.  p and ds go out per
//             (row, slot, head): ds straight into grad_bias when that is wanted, else into the workspace.
//   grad B    the table is inverted (backward_det.h); a group per TARGET row walks its segment in table order, reads
//             p and ds of the lane's head and 16 bytes of g[row] and q[row] per entry, and writes its rows of grad_v
//             and grad_k once.  No float atomics, no zero fill.  A hub row is walked by one group alone.
#include <math.h>

#include "backward_det.h"
#include "dispatch.h"
#include "neighbor_attention.h"
#include "wave.h"

namespace pointops {

__device__ __forceinline__ void na_load(const float* __restrict__ p, float (&v)[kNaVec]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
}
__device__ __forceinline__ void na_store(float* __restrict__ p, const float (&v)[kNaVec]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void na_zero(float (&v)[kNaVec]) { v[0] = v[1] = v[2] = v[3] = 0.0f; }

// sum over the D channels of a head of a b: the lane's four products in ascending order, then the butterfly over the
// Gh lanes of the head.  Every lane of the wave takes part (idle ones with zeros).
template <int GH>
__device__ __forceinline__ float na_head_dot(const float (&a)[kNaVec], const float (&b)[kNaVec]) {
  float d = a[0] * b[0];
  d = d + a[1] * b[1];
  d = d + a[2] * b[2];
  d = d + a[3] * b[3];
  return wave_sum<GH>(d);
}

// Stage slots [k0, k0 + kt) of the workgroup's R rows: s_src [R][tile] the source row (-1 = masked), and with a bias
// s_b [R][tile][HG] the bias of heads [h0, h0 + HG) (0 beyond `heads`).  Call from workgroup-uniform control flow.
template <int G, int GH>
__device__ __forceinline__ void na_stage(int* s_src, float* s_b, const int64_t* __restrict__ idx,
                                         const int64_t* __restrict__ lengths, const float* __restrict__ bias,
                                         int64_t row0, int64_t rows, int L, int K, int M, int heads, int h0, int tile,
                                         int k0, int kt, bool sources) {
  constexpr int R = kNaBlock / G, HG = G / GH;
  __syncthreads();
  if (sources) {
    for (int i = threadIdx.x; i < R * kt; i += kNaBlock) {
      const int r = i / kt, kk = i - r * kt;
      const int64_t rr = row0 + r;
      int s = -1;
      if (rr < rows) {
        // (every load is in bounds whatever the slot holds: no branch on the loaded values)
        const int64_t m = idx[rr * K + k0 + kk];
        const int64_t len = lengths == nullptr ? INT64_MAX : lengths[rr / L];
        s = (m >= 0 && m < M && k0 + kk < len) ? (int)m : -1;
      }
      s_src[r * tile + kk] = s;
    }
  }
  if (bias != nullptr) {
    for (int i = threadIdx.x; i < R * kt * HG; i += kNaBlock) {
      const int e = i / HG, hh = i - e * HG;
      const int r = e / kt, kk = e - r * kt;
      const int64_t rr = row0 + r;
      float b = 0.0f;
      if (rr < rows && h0 + hh < heads) b = bias[(rr * K + k0 + kk) * heads + h0 + hh];
      s_b[(r * tile + kk) * HG + hh] = b;
    }
  }
  __syncthreads();
}

// Dynamic LDS: na_lds_bytes.  G lanes per row, GH lanes per head.
template <int G, int GH>
__global__ __launch_bounds__(kNaBlock) void na_forward_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths, const float* __restrict__ bias, int64_t rows,
    int L, int K, int M, int heads, int tile, float scale, float* __restrict__ out, float* __restrict__ lse) {
  extern __shared__ int s_na[];
  constexpr int R = kNaBlock / G, HG = G / GH, U = kNaUnroll, D = GH * kNaVec;
  int* s_src = s_na;
  float* s_b = reinterpret_cast<float*>(s_na + (size_t)R * tile);
  const int grp = threadIdx.x / G, j = threadIdx.x % G, hl = j / GH, jl = j % GH;
  const int64_t row0 = (int64_t)blockIdx.x * R, row = row0 + grp;
  const bool live = row < rows;
  const int C = heads * D;
  const int64_t base = (live ? row / L : 0) * (int64_t)M * C;
  const int chunks = (heads + HG - 1) / HG, ntiles = (K + tile - 1) / tile;
  const bool has_bias = bias != nullptr;

  for (int c = 0; c < chunks; ++c) {  // (more than one only with G = 64)
    const int h = c * HG + hl;
    const bool on = live && h < heads;
    const int ch = h * D + jl * kNaVec;
    float qv[kNaVec], acc[kNaVec];
    na_zero(qv), na_zero(acc);
    if (on) na_load(q + row * C + ch, qv);
    float m = -INFINITY, l = 0.0f;
    for (int t = 0; t < ntiles; ++t) {
      const int k0 = t * tile, kt = min(tile, K - k0);
      if (ntiles > 1 || c == 0 || has_bias)  // (workgroup-uniform)
        na_stage<G, GH>(s_src, s_b, idx, lengths, bias, row0, rows, L, K, M, heads, c * HG, tile, k0, kt,
                        ntiles > 1 || c == 0);
      for (int kb = 0; kb < kt; kb += U) {
        int s[U];
        float b[U], kr[U][kNaVec], vr[U][kNaVec];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool in = kb + u < kt;
          s[u] = in ? s_src[grp * tile + kb + u] : -1;
          b[u] = (has_bias && in) ? s_b[(grp * tile + kb + u) * HG + hl] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // the loads, all issued before the first dot
          if (on && s[u] >= 0) {
            na_load(k + base + (int64_t)s[u] * C + ch, kr[u]);
            na_load(v + base + (int64_t)s[u] * C + ch, vr[u]);
          } else {
            na_zero(kr[u]), na_zero(vr[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // ascending k; branch-free, every lane of the wave is in the butterfly
          const float sk = scale * na_head_dot<GH>(qv, kr[u]) + b[u];
          const bool ok = s[u] >= 0 && sk > -INFINITY;
          const float mn = ok ? fmaxf(m, sk) : m;
          const float alpha = mn == -INFINITY ? 1.0f : expf(m - mn);  // (m = -inf, mn finite: exp(-inf) = 0)
          const float p = ok ? expf(sk - mn) : 0.0f;
          l = l * alpha + p;
#pragma unroll
          for (int x = 0; x < kNaVec; ++x) acc[x] = acc[x] * alpha + p * vr[u][x];
          m = mn;
        }
      }
    }
    if (!on) continue;
    const bool any = l > 0.0f;
#pragma unroll
    for (int x = 0; x < kNaVec; ++x) acc[x] = any ? acc[x] / l : 0.0f;
    na_store(out + row * C + ch, acc);
    if (jl == 0) lse[row * heads + h] = any ? m + logf(l) : -INFINITY;
  }
}

// grad_q[row,:] and the planes p, ds [(row K + k) heads + h] (0 for a slot that does not count); grad_q may be null
template <int G, int GH>
__global__ __launch_bounds__(kNaBlock) void na_grad_q_kernel(
    const float* __restrict__ g, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ out, const float* __restrict__ lse, const int64_t* __restrict__ idx,
    const int64_t* __restrict__ lengths, const float* __restrict__ bias, int64_t rows, int L, int K, int M, int heads,
    int tile, float scale, float* __restrict__ grad_q, float* __restrict__ plane_p, float* __restrict__ plane_ds) {
  extern __shared__ int s_na[];
  constexpr int R = kNaBlock / G, HG = G / GH, U = kNaUnroll, D = GH * kNaVec;
  int* s_src = s_na;
  float* s_b = reinterpret_cast<float*>(s_na + (size_t)R * tile);
  const int grp = threadIdx.x / G, j = threadIdx.x % G, hl = j / GH, jl = j % GH;
  const int64_t row0 = (int64_t)blockIdx.x * R, row = row0 + grp;
  const bool live = row < rows;
  const int C = heads * D;
  const int64_t base = (live ? row / L : 0) * (int64_t)M * C;
  const int chunks = (heads + HG - 1) / HG, ntiles = (K + tile - 1) / tile;
  const bool has_bias = bias != nullptr;

  for (int c = 0; c < chunks; ++c) {
    const int h = c * HG + hl;
    const bool on = live && h < heads;
    const int ch = h * D + jl * kNaVec;
    float qv[kNaVec], gv[kNaVec], ov[kNaVec], gq[kNaVec];
    na_zero(qv), na_zero(gv), na_zero(ov), na_zero(gq);
    float ls = -INFINITY;
    if (on) {
      na_load(q + row * C + ch, qv);
      na_load(g + row * C + ch, gv);
      na_load(out + row * C + ch, ov);
      ls = lse[row * heads + h];
    }
    const float delta = na_head_dot<GH>(gv, ov);
    for (int t = 0; t < ntiles; ++t) {
      const int k0 = t * tile, kt = min(tile, K - k0);
      if (ntiles > 1 || c == 0 || has_bias)  // (workgroup-uniform)
        na_stage<G, GH>(s_src, s_b, idx, lengths, bias, row0, rows, L, K, M, heads, c * HG, tile, k0, kt,
                        ntiles > 1 || c == 0);
      for (int kb = 0; kb < kt; kb += U) {
        int s[U];
        float b[U], kr[U][kNaVec], vr[U][kNaVec];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool in = kb + u < kt;
          s[u] = in ? s_src[grp * tile + kb + u] : -1;
          b[u] = (has_bias && in) ? s_b[(grp * tile + kb + u) * HG + hl] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (on && s[u] >= 0) {
            na_load(k + base + (int64_t)s[u] * C + ch, kr[u]);
            na_load(v + base + (int64_t)s[u] * C + ch, vr[u]);
          } else {
            na_zero(kr[u]), na_zero(vr[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float sk = scale * na_head_dot<GH>(qv, kr[u]) + b[u];  // the forward's logit, operation by operation
          const float dp = na_head_dot<GH>(gv, vr[u]);
          const bool ok = s[u] >= 0 && sk > -INFINITY && ls > -INFINITY;
          const float p = ok ? expf(sk - ls) : 0.0f;
          const float ds = p * (dp - delta);
#pragma unroll
          for (int x = 0; x < kNaVec; ++x) gq[x] = gq[x] + ds * kr[u][x];
          if (on && jl == 0 && kb + u < kt) {
            const int64_t at = (row * K + k0 + kb + u) * heads + h;
            plane_p[at] = p;
            plane_ds[at] = ds;
          }
        }
      }
    }
    if (!on || grad_q == nullptr) continue;
#pragma unroll
    for (int x = 0; x < kNaVec; ++x) gq[x] = scale * gq[x];
    na_store(grad_q + row * C + ch, gq);
  }
}

// grad_v[r,:] = sum over the entries e = (n L + l) K + k of target row r, in table order, of p[e,h] g[n,l,:];
// grad_k[r,:] = scale times the same sum of ds[e,h] q[n,l,:].  Either may be null.
template <int G, int GH>
__global__ __launch_bounds__(kNaBlock) void na_grad_kv_kernel(
    const float* __restrict__ g, const float* __restrict__ q, const float* __restrict__ plane_p,
    const float* __restrict__ plane_ds, const unsigned* __restrict__ vals, const int* __restrict__ seg_start,
    const int* __restrict__ seg_end, int64_t targets, int K, int heads, float scale, float* __restrict__ grad_k,
    float* __restrict__ grad_v) {
  constexpr int R = kNaBlock / G, HG = G / GH, U = kNaUnroll, D = GH * kNaVec;
  const int grp = threadIdx.x / G, j = threadIdx.x % G, hl = j / GH, jl = j % GH;
  const int64_t r = (int64_t)blockIdx.x * R + grp;
  if (r >= targets) return;  // (no barrier and no cross-lane step below)
  const int t0 = seg_start[r], t1 = seg_end[r];
  const int C = heads * D, chunks = (heads + HG - 1) / HG;
  const bool want_k = grad_k != nullptr, want_v = grad_v != nullptr;
  for (int c = 0; c < chunks; ++c) {
    const int h = c * HG + hl;
    if (h >= heads) continue;
    const int ch = h * D + jl * kNaVec;
    float ak[kNaVec], av[kNaVec];
    na_zero(ak), na_zero(av);
    for (int tb = t0; tb < t1; tb += U) {
      bool in[U];
      float p[U], ds[U], gv[U][kNaVec], qv[U][kNaVec];
#pragma unroll
      for (int u = 0; u < U; ++u) {  // the entry, its weights, its rows of g and q: loads before the first add
        in[u] = tb + u < t1;
        p[u] = ds[u] = 0.0f;
        na_zero(gv[u]), na_zero(qv[u]);
        if (!in[u]) continue;
        const unsigned e = vals[tb + u];
        const int64_t row = e / (unsigned)K;
        if (want_v) {
          p[u] = plane_p[(int64_t)e * heads + h];
          na_load(g + row * C + ch, gv[u]);
        }
        if (want_k) {
          ds[u] = plane_ds[(int64_t)e * heads + h];
          na_load(q + row * C + ch, qv[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {  // the adds, in segment order
        if (!in[u]) continue;
#pragma unroll
        for (int x = 0; x < kNaVec; ++x) {
          av[x] = av[x] + p[u] * gv[u][x];
          ak[x] = ak[x] + ds[u] * qv[u][x];
        }
      }
    }
    if (want_v) na_store(grad_v + r * C + ch, av);
    if (want_k) {
#pragma unroll
      for (int x = 0; x < kNaVec; ++x) ak[x] = scale * ak[x];
      na_store(grad_k + r * C + ch, ak);
    }
  }
}

struct NaWs {
  DetWs det;
  float *p, *ds;  // (N L K heads) planes of kernel A for kernel B
};

// the inverted table of backward_det.h, then the two planes
static size_t na_carve(NaWs* ws, void* base, int64_t N, int64_t L, int64_t K, int64_t M, int64_t heads) {
  NaWs w;
  Carver c(base);
  w.det.keys_in = nullptr;
  c.off = det_carve(base ? &w.det : nullptr, base, N, L, K, M);
  const size_t plane = sizeof(float) * (size_t)(N * L * K * heads > 0 ? N * L * K * heads : 1);
  w.p = (float*)c.take(plane);
  w.ds = (float*)c.take(plane);
  if (ws) *ws = w;
  return c.off;
}

static bool na_sizes_ok(int64_t N, int64_t L, int64_t M, int64_t K, int64_t heads, int64_t D) {
  return N >= 0 && M >= 0 && L >= 0 && K >= 0 && heads >= 1 && na_head_ok(D) && heads <= kNaMaxC / D &&
         N < (1LL << 31) && M < (1LL << 31) && L < (1LL << 31) && K < (1LL << 31) && N * L < (1LL << 31) &&
         N * L * K < (1LL << 31) && N * L * K * heads < (1LL << 31) && N * M < (1LL << 31) - 1;
}

static bool na_aligned(const void* a, const void* b, const void* c, const void* d, const void* e) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) % 16) == 0;
}

constexpr Ints<2, 4, 8, 16, 32, 64> kNaHeadLanes{};  // (fallback: 1)
constexpr Ints<1, 2, 4, 8, 16, 32, 64> kNaGroups{};

// f(G, GH) for the plan's instance; the instances are the pairs with GH <= G
template <class F>
static void na_with_instance(const NaPlan& plan, F&& f) {
  with_exact<1>(kNaHeadLanes, plan.Gh, [&](auto GH) {
    with_bucket(kNaGroups, plan.G, [&](auto G) {
      if constexpr (decltype(G)::value >= decltype(GH)::value) f(G, GH);
    });
  });
}

}  // namespace pointops

using namespace pointops;

#define NA_BAD_SIZES \
  ": bad sizes (D in {4, 8, ..., 256}, heads D <= 65536; N L K heads must be below 2^31 and N M below 2^31 - 1)"

extern "C" size_t pointops_neighbor_attention_backward_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M,
                                                                       int64_t heads) {
  if (!na_sizes_ok(N, L, M, K, heads, kNaVec)) return 0;
  return na_carve(nullptr, nullptr, N, L, K, M, heads);
}

extern "C" int pointops_neighbor_attention(const float* q, const float* k, const float* v, const int64_t* idx,
                                           const int64_t* lengths, const float* bias, int64_t N, int64_t L, int64_t M,
                                           int64_t K, int64_t heads, int64_t D, float scale, float* out, float* lse,
                                           void* stream_) {
  POINTOPS_REQUIRE(na_sizes_ok(N, L, M, K, heads, D), "neighbor_attention" NA_BAD_SIZES);
  const int64_t rows = N * L;
  if (rows == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE(q != nullptr && out != nullptr && lse != nullptr && (K == 0 || idx != nullptr) &&
                       ((k != nullptr && v != nullptr) || N * M == 0),
                   "neighbor_attention: null pointer");
  POINTOPS_REQUIRE(na_aligned(q, k, v, out, nullptr), "neighbor_attention: q, k, v and out must be 16-byte aligned");
  const NaPlan plan = na_plan(heads, D, K);
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned blocks = (unsigned)ceil_div(rows, plan.rows);
  na_with_instance(plan, [&](auto G, auto GH) {
    hipLaunchKernelGGL((na_forward_kernel<decltype(G)::value, decltype(GH)::value>), dim3(blocks), dim3(kNaBlock),
                       na_lds_bytes(plan), stream, q, k, v, idx, lengths, bias, rows, (int)L, (int)K, (int)M,
                       (int)heads, plan.tile, scale, out, lse);
  });
  return check_launch("neighbor_attention");
}

extern "C" int pointops_neighbor_attention_backward(const float* grad_out, const float* q, const float* k,
                                                    const float* v, const float* out, const float* lse,
                                                    const int64_t* idx, const int64_t* lengths, const float* bias,
                                                    int64_t N, int64_t L, int64_t M, int64_t K, int64_t heads,
                                                    int64_t D, float scale, float* grad_q, float* grad_k,
                                                    float* grad_v, float* grad_bias, void* workspace,
                                                    size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(na_sizes_ok(N, L, M, K, heads, D), "neighbor_attention_backward" NA_BAD_SIZES);
  if (N == 0) return POINTOPS_OK;
  const int64_t rows = N * L, targets = N * M;
  POINTOPS_REQUIRE(rows == 0 || (grad_out != nullptr && q != nullptr && out != nullptr && lse != nullptr &&
                                 (K == 0 || idx != nullptr) && ((k != nullptr && v != nullptr) || targets == 0)),
                   "neighbor_attention_backward: null pointer");
  POINTOPS_REQUIRE(na_aligned(grad_out, q, k, v, out) && na_aligned(grad_q, grad_k, grad_v, nullptr, nullptr),
                   "neighbor_attention_backward: grad_out, q, k, v, out, grad_q, grad_k and grad_v must be 16-byte "
                   "aligned");
  NaWs ws;
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, na_carve(&ws, workspace, N, L, K, M, heads)),
                             "neighbor_attention_backward: workspace too small");
  const bool want_kv = (grad_k != nullptr || grad_v != nullptr) && targets > 0;
  if (grad_q == nullptr && grad_bias == nullptr && !want_kv) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const NaPlan plan = na_plan(heads, D, K);
  float* plane_ds = grad_bias != nullptr ? grad_bias : ws.ds;
  if (rows > 0) {
    const unsigned blocks = (unsigned)ceil_div(rows, plan.rows);
    na_with_instance(plan, [&](auto G, auto GH) {
      hipLaunchKernelGGL((na_grad_q_kernel<decltype(G)::value, decltype(GH)::value>), dim3(blocks), dim3(kNaBlock),
                         na_lds_bytes(plan), stream, grad_out, q, k, v, out, lse, idx, lengths, bias, rows, (int)L,
                         (int)K, (int)M, (int)heads, plan.tile, scale, grad_q, ws.p, plane_ds);
    });
  }
  if (want_kv) {
    const int rc = det_invert(ws.det, idx, nullptr, lengths, N, L, K, M, stream);
    if (rc != POINTOPS_OK) return rc;
    const unsigned blocks = (unsigned)ceil_div(targets, plan.rows);
    na_with_instance(plan, [&](auto G, auto GH) {
      hipLaunchKernelGGL((na_grad_kv_kernel<decltype(G)::value, decltype(GH)::value>), dim3(blocks), dim3(kNaBlock), 0,
                         stream, grad_out, q, ws.p, plane_ds, ws.det.vals_out, ws.det.seg_start, ws.det.seg_end,
                         targets, (int)(K > 0 ? K : 1), (int)heads, scale, grad_k, grad_v);
    });
  }
  return check_launch("neighbor_attention_backward");
}

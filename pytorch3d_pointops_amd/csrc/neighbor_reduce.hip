// neighbor_reduce.hip -- NEIGHBOUR REDUCE (gfx950): out[n,l,:] = sum / mean / max over k of x[n, idx[n,l,k], :] without
// the (N, L, K, C) tensor of knn_gather, and the two pull backward passes.  The definition is the NEIGHBOUR REDUCE block
// of include/pointops_amd.h; neighbor_reduce.h has the split of a row over the lanes.
//
// The work is a gather bound by memory traffic: a gathered row is used once, so there is nothing for the matrix cores
// to reuse and nothing to keep in LDS but the table.  What the kernels are built for is 16-byte traffic and loads in
// flight:
//   forward   a group of G lanes per query row, V = 4 channels per lane (global_load_dwordx4 / store_dwordx4; V = 1 when
//             C % 4 != 0).  The 256 / G rows of a workgroup own CONSECUTIVE table entries, so the workgroup reads them
//             once with coalesced loads, checks them (idx in [0, M), k < lengths[n]) and leaves int32 sources (-1 =
//             masked) and weights in LDS; every lane then reads its row's slots as LDS broadcasts.  The slot loop is
//             unrolled by kNrUnroll: four independent row loads are issued before the first add, the adds follow in
//             ascending k.  `max` keeps best and slot in registers and stores the four slots of a lane as one dword.
//   grad_x    the table is inverted (backward_det.h: stable sort, segments in table order); a group of G lanes per
//             TARGET row walks its segment, loads g[n,l,:] 16 bytes at a time (for `max` the four arg bytes as one
//             dword, compared with k), adds in segment order and writes its row once.  No atomics, no zero fill.  A hub
//             row referenced by thousands of entries is walked by one group alone (DESIGN.md states the cost).
//   grad_w    a group per query row; per slot the lane's partial dot over its channels (chunks ascending, the V channels
//             ascending), then wave_sum<G> (wave.h): a fixed tree, so the order depends on C alone.
#include "backward_det.h"
#include "neighbor_reduce.h"
#include "wave.h"

namespace pointops {

template <int V>
__device__ __forceinline__ void nr_load(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void nr_store(float* __restrict__ p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// the slots of cloud n that lengths leaves: k < nr_length(lengths, n)
__device__ __forceinline__ int64_t nr_length(const int64_t* __restrict__ lengths, int n) {
  return lengths == nullptr ? INT64_MAX : lengths[n];
}
// a slot counts: the NEIGHBOUR REDUCE mask (knn_gather's and masked_gather's together, and idx < M)
__device__ __forceinline__ bool nr_valid(int64_t m, int k, int M, int64_t len) { return m >= 0 && m < M && k < len; }

// MODE: kNrSum / kNrMean / kNrMax; W: `sum` with weights.  Dynamic LDS: nr_lds_bytes.
template <int V, int G, int MODE, bool W>
__global__ __launch_bounds__(kNrBlock) void nr_forward_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths,
    const float* __restrict__ weights, int64_t rows, int L, int K, int M, int C, int tile, float* __restrict__ out,
    uint8_t* __restrict__ arg) {
  extern __shared__ int s_nr[];
  constexpr int R = kNrBlock / G, U = kNrUnroll;
  int* s_src = s_nr;                                           // [R][tile] source row of x, -1 = masked
  float* s_w = reinterpret_cast<float*>(s_nr + (size_t)R * tile);  // [R][tile] (W only)
  const int grp = threadIdx.x / G, j = threadIdx.x % G;
  const int64_t row0 = (int64_t)blockIdx.x * R, row = row0 + grp;
  const bool live = row < rows;
  const float* xn = x + (live ? row / L : 0) * (int64_t)M * C;
  const int chunks = (C + V * G - 1) / (V * G), ntiles = (K + tile - 1) / tile;

  for (int c = 0; c < chunks; ++c) {  // (more than one only with G = 64)
    const int ch = (c * G + j) * V;
    const bool on = live && ch < C;
    float acc[V];
    int slot[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = 0.0f, slot[q] = 255;
    int count = 0;
    for (int t = 0; t < ntiles; ++t) {
      const int k0 = t * tile, kt = min(tile, K - k0);
      if (ntiles > 1 || c == 0) {  // (workgroup-uniform) stage the tile: one coalesced pass over the table
        __syncthreads();
        for (int i = threadIdx.x; i < R * kt; i += kNrBlock) {
          const int r = i / kt, kk = i - r * kt;
          const int64_t rr = row0 + r;
          int s = -1;
          float w = 0.0f;
          if (rr < rows) {
            // (every load is in bounds whatever the slot holds: no branch on the loaded values)
            const int64_t e = rr * K + k0 + kk;
            const int64_t m = idx[e];
            s = nr_valid(m, k0 + kk, M, nr_length(lengths, (int)(rr / L))) ? (int)m : -1;
            if (W) w = weights[e];
          }
          s_src[r * tile + kk] = s;
          if (W) s_w[r * tile + kk] = w;
        }
        __syncthreads();
      }
      for (int kb = 0; kb < kt; kb += U) {
        int s[U];
        float w[U], v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool in = kb + u < kt;
          s[u] = in ? s_src[grp * tile + kb + u] : -1;
          w[u] = (W && in) ? s_w[grp * tile + kb + u] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // the loads, all issued before the first add
          if (on && s[u] >= 0) {
            nr_load<V>(xn + (int64_t)s[u] * C + ch, v[u]);
          } else {
#pragma unroll
            for (int q = 0; q < V; ++q) v[u][q] = 0.0f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // the adds, ascending k
          if (s[u] < 0) continue;
#pragma unroll
          for (int q = 0; q < V; ++q) {
            if (MODE == kNrMax) {
              if (count == 0 || v[u][q] > acc[q]) acc[q] = v[u][q], slot[q] = k0 + kb + u;
            } else {
              const float p = W ? w[u] * v[u][q] : v[u][q];
              acc[q] = acc[q] + p;
            }
          }
          ++count;
        }
      }
    }
    if (!on) continue;
    if (MODE == kNrMean) {
      const float den = (float)(count > 1 ? count : 1);
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] = acc[q] / den;
    }
    nr_store<V>(out + row * C + ch, acc);
    if (MODE == kNrMax) {
      if constexpr (V == 4) {
        *reinterpret_cast<uint32_t*>(arg + row * C + ch) =
            (uint32_t)slot[0] | ((uint32_t)slot[1] << 8) | ((uint32_t)slot[2] << 16) | ((uint32_t)slot[3] << 24);
      } else {
        arg[row * C + ch] = (uint8_t)slot[0];
      }
    }
  }
}

// inv[row] = fl(1 / max(count, 1)), count = the valid slots of the query row: the factor of the `mean` backward
__global__ __launch_bounds__(kNrBlock) void nr_inv_count_kernel(const int64_t* __restrict__ idx,
                                                                const int64_t* __restrict__ lengths, int64_t rows,
                                                                int L, int K, int M, float* __restrict__ inv) {
  const int64_t row = (int64_t)blockIdx.x * kNrBlock + threadIdx.x;
  if (row >= rows) return;
  const int64_t len = nr_length(lengths, (int)(row / L));
  int count = 0;
  for (int k = 0; k < K; ++k) count += nr_valid(idx[row * K + k], k, M, len) ? 1 : 0;
  inv[row] = 1.0f / (float)(count > 1 ? count : 1);
}

// grad_x[r,:] = sum over the entries e = (n L + l) K + k of target row r, in table order, of fl(f g[n,l,:]): f the
// weight of the entry (W), inv[n L + l] (`mean`) or none; `max` takes the channels with arg[n,l,c] == k only
template <int V, int G, int MODE, bool W>
__global__ __launch_bounds__(kNrBlock) void nr_grad_x_kernel(
    const float* __restrict__ g, const float* __restrict__ weights, const float* __restrict__ inv,
    const uint8_t* __restrict__ arg, const unsigned* __restrict__ vals, const int* __restrict__ seg_start,
    const int* __restrict__ seg_end, int64_t targets, int K, int C, float* __restrict__ grad_x) {
  constexpr int R = kNrBlock / G, U = kNrUnroll;
  const int grp = threadIdx.x / G, j = threadIdx.x % G;
  const int64_t r = (int64_t)blockIdx.x * R + grp;
  if (r >= targets) return;  // (no barrier and no cross-lane step below)
  const int t0 = seg_start[r], t1 = seg_end[r];
  const int chunks = (C + V * G - 1) / (V * G);
  for (int c = 0; c < chunks; ++c) {
    const int ch = (c * G + j) * V;
    if (ch >= C) break;
    float acc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = 0.0f;
    for (int tb = t0; tb < t1; tb += U) {
      bool in[U];
      int k[U];
      float f[U], v[U][V];
      uint32_t a[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {  // the entry, its row of g (and of arg): loads before the first add
        in[u] = tb + u < t1;
        k[u] = 0, f[u] = 0.0f, a[u] = 0;
#pragma unroll
        for (int q = 0; q < V; ++q) v[u][q] = 0.0f;
        if (!in[u]) continue;
        const unsigned e = vals[tb + u];
        const unsigned row = e / (unsigned)K;
        k[u] = (int)(e - row * (unsigned)K);
        if (W) f[u] = weights[e];
        if (MODE == kNrMean) f[u] = inv[row];
        nr_load<V>(g + (int64_t)row * C + ch, v[u]);
        if (MODE == kNrMax) {
          if constexpr (V == 4) a[u] = *reinterpret_cast<const uint32_t*>(arg + (int64_t)row * C + ch);
          else a[u] = arg[(int64_t)row * C + ch];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {  // the adds, in segment order
        if (!in[u]) continue;
#pragma unroll
        for (int q = 0; q < V; ++q) {
          if (MODE == kNrMax && (int)((a[u] >> (8 * q)) & 255u) != k[u]) continue;
          const float p = (W || MODE == kNrMean) ? f[u] * v[u][q] : v[u][q];
          acc[q] = acc[q] + p;
        }
      }
    }
    nr_store<V>(grad_x + r * C + ch, acc);
  }
}

// grad_w[n,l,k] = sum over c of g[n,l,c] x[n,idx,c] for a valid slot, else 0
template <int V, int G>
__global__ __launch_bounds__(kNrBlock) void nr_grad_w_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                             const int64_t* __restrict__ idx,
                                                             const int64_t* __restrict__ lengths, int64_t rows, int L,
                                                             int K, int M, int C, float* __restrict__ grad_w) {
  constexpr int R = kNrBlock / G;
  const int grp = threadIdx.x / G, j = threadIdx.x % G;
  const int64_t row = (int64_t)blockIdx.x * R + grp;
  const bool live = row < rows;  // (a dead group stays for the cross-lane sums of its wave)
  const int n = live ? (int)(row / L) : 0;
  const float* xn = x + (int64_t)n * M * C;
  const float* gr = g + (live ? row : 0) * C;
  const int64_t len = nr_length(lengths, n);
  const int chunks = (C + V * G - 1) / (V * G);
  for (int k = 0; k < K; ++k) {
    const int64_t m = live ? idx[row * K + k] : -1;
    const bool ok = live && nr_valid(m, k, M, len);
    float acc = 0.0f;
    for (int c = 0; c < chunks; ++c) {
      const int ch = (c * G + j) * V;
      if (!ok || ch >= C) continue;
      float gv[V], xv[V];
      nr_load<V>(gr + ch, gv);
      nr_load<V>(xn + m * C + ch, xv);
#pragma unroll
      for (int q = 0; q < V; ++q) acc = acc + gv[q] * xv[q];
    }
    acc = wave_sum<G>(acc);
    if (live && j == 0) grad_w[row * K + k] = ok ? acc : 0.0f;
  }
}

struct NrWs {
  DetWs det;
  float* inv;  // (N L) factors of the `mean` backward
};

// the inverted table of backward_det.h, then the factors
static size_t nr_carve(NrWs* ws, void* base, int64_t N, int64_t L, int64_t K, int64_t M) {
  NrWs w;
  Carver c(base);
  w.det.keys_in = nullptr;
  c.off = det_carve(base ? &w.det : nullptr, base, N, L, K, M);
  w.inv = (float*)c.take(sizeof(float) * (size_t)(N * L > 0 ? N * L : 1));
  if (ws) *ws = w;
  return c.off;
}

static bool nr_sizes_ok(int64_t N, int64_t M, int64_t C, int64_t L, int64_t K) {
  return N >= 0 && M >= 0 && L >= 0 && K >= 0 && C >= 1 && C <= kNrMaxC && N < (1LL << 31) && M < (1LL << 31) &&
         L < (1LL << 31) && K < (1LL << 31) && N * L < (1LL << 31) && N * L * K < (1LL << 31) &&
         N * M < (1LL << 31) - 1;
}

// the rows of C channels behind these pointers can be moved V channels at a time (arg: the four slots of a lane)
static bool nr_aligned(int V, const void* a, const void* b, const void* c, const void* arg) {
  if (V == 1) return true;
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16) == 0 && ((uintptr_t)arg % 4) == 0;
}

constexpr Ints<1, 2, 4, 8, 16, 32, 64> kNrGroups{};

}  // namespace pointops

using namespace pointops;

extern "C" size_t pointops_neighbor_reduce_backward_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M) {
  if (!nr_sizes_ok(N, M, 1, L, K)) return 0;
  return nr_carve(nullptr, nullptr, N, L, K, M);
}

extern "C" int pointops_neighbor_reduce(const float* x, const int64_t* idx, const int64_t* lengths,
                                        const float* weights, int64_t N, int64_t M, int64_t C, int64_t L, int64_t K,
                                        int reduce, float* out, uint8_t* arg, void* stream_) {
  POINTOPS_REQUIRE(reduce == kNrSum || reduce == kNrMean || reduce == kNrMax,
                   "neighbor_reduce: reduce must be 0 (sum), 1 (mean) or 2 (max)");
  POINTOPS_REQUIRE(nr_sizes_ok(N, M, C, L, K),
                   "neighbor_reduce: bad sizes (C in [1, 65536]; the neighbour table must have fewer than 2^31 entries)");
  POINTOPS_REQUIRE(weights == nullptr || reduce == kNrSum, "neighbor_reduce: weights go with sum only");
  POINTOPS_REQUIRE(reduce != kNrMax || (K <= kNrMaxK && (arg != nullptr || N * L == 0)),
                   "neighbor_reduce: max needs K <= 255 and the arg output");
  const int64_t rows = N * L;
  if (rows == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE(out != nullptr && (K == 0 || idx != nullptr) && (x != nullptr || N * M == 0),
                   "neighbor_reduce: null pointer");
  const NrPlan plan = nr_plan(C, K);
  POINTOPS_REQUIRE(nr_aligned(plan.V, x, out, nullptr, arg),
                   "neighbor_reduce: x and out must be 16-byte aligned when C is a multiple of 4");
  hipStream_t stream = (hipStream_t)stream_;
  const int mode = weights != nullptr ? 3 : reduce;
  const unsigned blocks = (unsigned)ceil_div(rows, plan.rows);
  with_exact<1>(Ints<4>{}, plan.V, [&](auto V) {
    with_bucket(kNrGroups, plan.G, [&](auto G) {
      with_exact<kNrSum>(Ints<kNrMean, kNrMax, 3>{}, mode, [&](auto MODE) {
        constexpr int mode_c = decltype(MODE)::value;
        constexpr bool W = mode_c == 3;
        hipLaunchKernelGGL((nr_forward_kernel<decltype(V)::value, decltype(G)::value, W ? kNrSum : mode_c, W>), dim3(blocks), dim3(kNrBlock),
                           nr_lds_bytes(plan, W), stream, x, idx, lengths, weights, rows, (int)L, (int)K, (int)M, (int)C,
                           plan.tile, out, arg);
      });
    });
  });
  return check_launch("neighbor_reduce");
}

extern "C" int pointops_neighbor_reduce_backward(const float* grad_out, const float* x, const int64_t* idx,
                                                 const int64_t* lengths, const float* weights, const uint8_t* arg,
                                                 int64_t N, int64_t M, int64_t C, int64_t L, int64_t K, int reduce,
                                                 float* grad_x, float* grad_w, void* workspace, size_t workspace_bytes,
                                                 void* stream_) {
  POINTOPS_REQUIRE(reduce == kNrSum || reduce == kNrMean || reduce == kNrMax,
                   "neighbor_reduce_backward: reduce must be 0 (sum), 1 (mean) or 2 (max)");
  POINTOPS_REQUIRE(nr_sizes_ok(N, M, C, L, K),
                   "neighbor_reduce_backward: bad sizes (C in [1, 65536]; the neighbour table must have fewer than 2^31 "
                   "entries)");
  POINTOPS_REQUIRE(weights == nullptr || reduce == kNrSum, "neighbor_reduce_backward: weights go with sum only");
  POINTOPS_REQUIRE(grad_w == nullptr || (weights != nullptr && x != nullptr) || N * L * K == 0 || N * M == 0,
                   "neighbor_reduce_backward: grad_w needs weights and x");
  POINTOPS_REQUIRE(reduce != kNrMax || (K <= kNrMaxK && (arg != nullptr || N * L == 0)),
                   "neighbor_reduce_backward: max needs K <= 255 and the forward's arg");
  if (N == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE((grad_out != nullptr || N * L == 0) && (idx != nullptr || N * L * K == 0),
                   "neighbor_reduce_backward: null pointer");
  const NrPlan plan = nr_plan(C, K);
  POINTOPS_REQUIRE(nr_aligned(plan.V, grad_out, x, grad_x, arg),
                   "neighbor_reduce_backward: grad_out, x and grad_x must be 16-byte aligned when C is a multiple of 4");
  NrWs ws;
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, nr_carve(&ws, workspace, N, L, K, M)),
                             "neighbor_reduce_backward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t rows = N * L, targets = N * M;
  if (grad_x != nullptr && targets > 0) {
    const int rc = det_invert(ws.det, idx, nullptr, lengths, N, L, K, M, stream);
    if (rc != POINTOPS_OK) return rc;
    if (reduce == kNrMean && rows > 0)
      hipLaunchKernelGGL(nr_inv_count_kernel, dim3((unsigned)ceil_div(rows, kNrBlock)), dim3(kNrBlock), 0, stream, idx,
                         lengths, rows, (int)L, (int)K, (int)M, ws.inv);
    const int mode = weights != nullptr ? 3 : reduce;
    const unsigned blocks = (unsigned)ceil_div(targets, plan.rows);
    with_exact<1>(Ints<4>{}, plan.V, [&](auto V) {
      with_bucket(kNrGroups, plan.G, [&](auto G) {
        with_exact<kNrSum>(Ints<kNrMean, kNrMax, 3>{}, mode, [&](auto MODE) {
          constexpr int mode_c = decltype(MODE)::value;
        constexpr bool W = mode_c == 3;
          hipLaunchKernelGGL((nr_grad_x_kernel<decltype(V)::value, decltype(G)::value, W ? kNrSum : mode_c, W>), dim3(blocks), dim3(kNrBlock), 0,
                             stream, grad_out, weights, ws.inv, arg, ws.det.vals_out, ws.det.seg_start, ws.det.seg_end,
                             targets, (int)(K > 0 ? K : 1), (int)C, grad_x);
        });
      });
    });
  }
  if (grad_w != nullptr && rows * K > 0) {
    const unsigned blocks = (unsigned)ceil_div(rows, plan.rows);
    with_exact<1>(Ints<4>{}, plan.V, [&](auto V) {
      with_bucket(kNrGroups, plan.G, [&](auto G) {
        hipLaunchKernelGGL((nr_grad_w_kernel<decltype(V)::value, decltype(G)::value>), dim3(blocks), dim3(kNrBlock), 0, stream, grad_out, x, idx, lengths,
                           rows, (int)L, (int)K, (int)M, (int)C, grad_w);
      });
    });
  }
  return check_launch("neighbor_reduce_backward");
}

// neighbor_mlp.hip -- NEIGHBOUR MLP-MAX (gfx950): out[n,l,:] = max over k of relu(x[n,idx[n,l,k],:] + center[n,l,:]) weight
// + bias, the second layer of a PointNet++ set abstraction or EdgeConv block, without the two (N, L, K, C) tensors of
// knn_gather + add + relu + matmul + amax, and its backward.  The definition is the NEIGHBOUR MLP-MAX block of
// include/pointops_amd.h.
//
// weight is ONE matrix for every edge, so unlike neighbor_conv.hip the B operand never moves:
//   forward   the M side of a v_mfma_f32_32x32x2_f32 block is 32 QUERY ROWS AT THE SAME SLOT k, and the kernel loops
//             over k: the running best and its slot live in registers of the accumulator's shape and are updated
//             elementwise, so the max over K needs no cross-lane step.  A 256-lane workgroup owns R = 32 RT rows; its
//             waves split (row tile rt) x (32-column block cb), RT NB <= 4 with NB = 1, 2, 4 column blocks (C2 <= 32,
//             64, 128): 128, 64, 32 rows.  (C2 <= 32 with C1 > 64 takes 64 rows and two of its waves only gather: 128
//             rows of 129 floats do not fit the 64 KiB of static LDS.)  A wave keeps the B-fragments of its column
//             block in KS = C1 / 2 (bucketed 8, 16, 32, 64) registers for the whole kernel.  Per slot the R rows are
//             gathered 16 bytes per lane INTO REGISTERS (the loads of slot k + 1 are issued before the MFMAs of slot
//             k), center added and the ReLU applied on the way to ONE LDS tile of odd row stride 2 KS + 1.  The
//             sources of 32 slots of every row are staged at a time (int32, -1 = masked, no branch on loaded values),
//             with a 32-bit validity mask per (slot, row tile) that the update reads as an LDS broadcast.
//   grad_c    a half wave per query row, 4 channels i per lane.  Per valid slot the columns with arg == k are found by
//             four ballots over the half wave (a lane compares the four arg bytes it holds) and walked ascending:
//             e = fmaf(gy[c], weight^T[c, i..i+3], e), gy[c] by one shuffle, weight^T (a transposed copy in the
//             workspace) 16 bytes per lane from cache.  Masked by the recomputed a > 0, summed in ascending k.
//   grad_x    the table is inverted (backward_det.h); a half wave per TARGET row walks its segment in table order and
//             recomputes the same e per entry (the target's own row of x is loaded once).  No atomics, every row
//             written once.  A hub row is walked by one half wave alone.
//   grad_w/b  workgroups (row chunk, 32-column block); a group of G >= C1 / 4 lanes per column keeps
//             acc[i..i+3][c] in registers over the rows of its chunk (row = chunk, chunk + chunks, ...), fetching the
//             row of the winning slot of (row, c); row C1 of the partial is grad_bias.  One partial per chunk in the
//             workspace, added in ascending chunk order by nm_sum_partials_kernel.
// Nothing here is sized by K C1 or K C2.  Fixed launch sequences, nothing is read back.
#include "neighbor_mlp.h"

namespace pointops {

constexpr int kNmTileFloats = 128 * 65;    // the LDS tile: 128 rows of C1 <= 64, 64 rows of C1 <= 128
constexpr int kNmMaxC = 128;

constexpr int nm_row_tiles(int NB, int KS) { return (4 / NB) * 32 * (2 * KS + 1) <= kNmTileFloats ? 4 / NB : 2 / NB; }

__device__ __forceinline__ float4 nm_ld4(const float* __restrict__ p) { return *reinterpret_cast<const float4*>(p); }

template <int NB, int KS, bool CENTER>
__global__ __launch_bounds__(kNmBlock) void nm_forward_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths,
    const float* __restrict__ center, const float* __restrict__ weight, const float* __restrict__ bias, int64_t rows,
    int L, int K, int M, int C1, int C2, int relu_out, float* __restrict__ out, uint8_t* __restrict__ arg) {
  constexpr int RT = nm_row_tiles(NB, KS), R = 32 * RT, STRIDE = 2 * KS + 1, G4 = KS / 2;
  constexpr int UNITS = R * G4, Q = (UNITS + kNmBlock - 1) / kNmBlock;  // 16-byte pieces of the tile, per lane
  __shared__ float s_A[R * STRIDE];
  __shared__ int s_src[kNmWin * R];  // [slot][row]
  __shared__ uint32_t s_mask[kNmWin * RT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5, c = lane & 31;
  const int cb = wave % NB, rt = (wave / NB) % RT;
  const bool mma = wave < NB * RT;  // (wave-uniform)
  const int oc = cb * 32 + c;
  const bool col = oc < C2;
  const int64_t row0 = (int64_t)blockIdx.x * R;

  float b[KS];  // B[k = 2 kk + h][o = oc], resident
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) b[kk] = (col && 2 * kk < C1) ? weight[(int64_t)(2 * kk + h) * C2 + oc] : 0.0f;
  const float bv = (col && bias != nullptr) ? bias[oc] : 0.0f;

  int ur[Q], uc[Q];
  bool uon[Q];
  float4 cen[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int u = t + kNmBlock * q;
    ur[q] = u / G4, uc[q] = (u % G4) * 4;
    uon[q] = u < UNITS && uc[q] < C1;
    cen[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (CENTER && uon[q] && row0 + ur[q] < rows) cen[q] = nm_ld4(center + (row0 + ur[q]) * C1 + uc[q]);
  }

  float best[16];
  int slot[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) best[r] = 0.0f, slot[r] = 255;
  uint32_t seen = 0;

  for (int k0 = 0; k0 < K; k0 += kNmWin) {
    const int kt = min(kNmWin, K - k0);
    nm_stage<R, RT>(idx, lengths, row0, rows, L, K, M, k0, kt, s_src, s_mask);

    float4 v[Q];
    auto gather = [&](int kk) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int s = uon[q] ? s_src[kk * R + ur[q]] : -1;
        v[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (s >= 0) v[q] = nm_ld4(x + (int64_t)s * C1 + uc[q]);
      }
    };
    gather(0);
    for (int kk = 0; kk < kt; ++kk) {
      __syncthreads();  // the MFMAs of the slot before have read the tile (first slot: the masks are written)
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!uon[q]) continue;
        float a[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
        const float ce[4] = {cen[q].x, cen[q].y, cen[q].z, cen[q].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (CENTER) a[j] = a[j] + ce[j];
          s_A[ur[q] * STRIDE + uc[q] + j] = a[j] > 0.0f ? a[j] : 0.0f;
        }
      }
      __syncthreads();
      if (kk + 1 < kt) gather(kk + 1);  // in flight during the MFMAs
      if (!mma) continue;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = bv;
      const float* a = s_A + (rt * 32 + c) * STRIDE + h;  // A[i = c][k = 2 kk + h]
#pragma unroll
      for (int q = 0; q < KS; ++q)
        if (2 * q < C1) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * q], b[q], acc, 0, 0, 0);
      const uint32_t m = s_mask[kk * RT + rt];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rb = (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool take = ((m >> rb) & 1u) && (!((seen >> rb) & 1u) || acc[r] > best[r]);
        best[r] = take ? acc[r] : best[r];
        slot[r] = take ? k0 + kk : slot[r];
      }
      seen |= m;
    }
  }
  if (!mma || !col) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (row >= rows) continue;
    out[row * C2 + oc] = (relu_out && !(best[r] > 0.0f)) ? 0.0f : best[r];
    arg[row * C2 + oc] = (uint8_t)slot[r];
  }
}

// wT[c C1 + i] = weight[i C2 + c]
__global__ __launch_bounds__(256) void nm_transpose_kernel(const float* __restrict__ weight, int C1, int C2,
                                                           float* __restrict__ wT) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o < C1 * C2) wT[o] = weight[(o % C1) * C2 + o / C1];
}

// gy of the lane's four columns ch .. ch + 3 of `row` (ch < C2)
__device__ __forceinline__ void nm_gy(const float* __restrict__ g, const float* __restrict__ out, int64_t row, int C2,
                                      int ch, int relu_out, float (&gy)[4]) {
  const float4 gv = nm_ld4(g + row * C2 + ch), ov = nm_ld4(out + row * C2 + ch);
  gy[0] = (relu_out && !(ov.x > 0.0f)) ? 0.0f : gv.x;
  gy[1] = (relu_out && !(ov.y > 0.0f)) ? 0.0f : gv.y;
  gy[2] = (relu_out && !(ov.z > 0.0f)) ? 0.0f : gv.z;
  gy[3] = (relu_out && !(ov.w > 0.0f)) ? 0.0f : gv.w;
}

// e[:] = the chain from +0.0f, over the columns c ascending whose arg byte is k, of fmaf(gy[c], wT[c, ch .. ch + 3], e).
// A half wave (32 lanes) per row: lane j holds the arg bytes (argw) and gy of columns 4 j .. 4 j + 3 (argw = ~0 past C2).
// Call with the whole half wave; returns whether any column matched.
__device__ __forceinline__ bool nm_edge_grad(uint32_t argw, const float (&gy)[4], int k, const float* __restrict__ wT,
                                             int C1, int ch, bool on, float (&e)[4]) {
  const int half = (threadIdx.x & 63) >> 5;
  uint32_t m[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) m[q] = (uint32_t)(__ballot((int)((argw >> (8 * q)) & 255u) == k) >> (32 * half));
  e[0] = e[1] = e[2] = e[3] = 0.0f;
  uint32_t any = m[0] | m[1] | m[2] | m[3];
  const bool hit = any != 0;
  while (any != 0) {
    const int jj = __ffs(any) - 1;
    any &= any - 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!((m[q] >> jj) & 1u)) continue;  // (uniform over the half wave)
      const float gyc = __shfl(gy[q], jj, 32);
      if (on) {
        const float4 w = nm_ld4(wT + (int64_t)(4 * jj + q) * C1 + ch);
        e[0] = __builtin_fmaf(gyc, w.x, e[0]), e[1] = __builtin_fmaf(gyc, w.y, e[1]);
        e[2] = __builtin_fmaf(gyc, w.z, e[2]), e[3] = __builtin_fmaf(gyc, w.w, e[3]);
      }
    }
  }
  return hit;
}

// acc[:] += (a > 0 ? e : 0), a = fl(x + center)
__device__ __forceinline__ void nm_masked_add(const float4 xv, const float4 cv, const float (&e)[4], float (&acc)[4]) {
  const float a[4] = {xv.x + cv.x, xv.y + cv.y, xv.z + cv.z, xv.w + cv.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = acc[j] + (a[j] > 0.0f ? e[j] : 0.0f);
}

// grad_center[row, :] = sum over the valid slots, ascending, of d
__global__ __launch_bounds__(kNmBlock) void nm_grad_center_kernel(
    const float* __restrict__ g, const float* __restrict__ out, const uint8_t* __restrict__ arg,
    const float* __restrict__ x, const float* __restrict__ center, const int64_t* __restrict__ idx,
    const int64_t* __restrict__ lengths, const float* __restrict__ wT, int64_t rows, int L, int K, int M, int C1,
    int C2, int relu_out, float* __restrict__ grad_center) {
  const int j = threadIdx.x & 31, ch = 4 * j;
  const int64_t row = (int64_t)blockIdx.x * (kNmBlock / 32) + (threadIdx.x >> 5);
  if (row >= rows) return;  // (a whole half wave; no barrier below)
  const bool on = ch < C1;
  uint32_t argw = ~0u;
  float gy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (ch < C2) {
    argw = *reinterpret_cast<const uint32_t*>(arg + row * C2 + ch);
    nm_gy(g, out, row, C2, ch, relu_out, gy);
  }
  const float4 cv = on ? nm_ld4(center + row * C1 + ch) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int64_t n = row / L;
  const int64_t len = lengths == nullptr ? INT64_MAX : lengths[n];
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < K; ++k) {
    const int64_t m = idx[row * K + k];
    if (!(m >= 0 && m < M && k < len)) continue;  // (uniform over the half wave)
    float e[4];
    if (!nm_edge_grad(argw, gy, k, wT, C1, ch, on, e) || !on) continue;
    nm_masked_add(nm_ld4(x + (n * M + m) * C1 + ch), cv, e, acc);
  }
  if (on) *reinterpret_cast<float4*>(grad_center + row * C1 + ch) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// grad_x[r, :] = sum over the entries of target row r, in table order, of d
template <bool CENTER>
__global__ __launch_bounds__(kNmBlock) void nm_grad_x_kernel(
    const float* __restrict__ g, const float* __restrict__ out, const uint8_t* __restrict__ arg,
    const float* __restrict__ x, const float* __restrict__ center, const float* __restrict__ wT,
    const unsigned* __restrict__ vals, const int* __restrict__ seg_start, const int* __restrict__ seg_end,
    int64_t targets, int K, int C1, int C2, int relu_out, float* __restrict__ grad_x) {
  const int j = threadIdx.x & 31, ch = 4 * j;
  const int64_t r = (int64_t)blockIdx.x * (kNmBlock / 32) + (threadIdx.x >> 5);
  if (r >= targets) return;  // (a whole half wave; no barrier below)
  const bool on = ch < C1;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int t0 = seg_start[r], t1 = seg_end[r];
  const float4 xv = (on && t0 < t1) ? nm_ld4(x + r * C1 + ch) : zero;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = t0; t < t1; ++t) {
    const unsigned en = vals[t];
    const int64_t row = en / (unsigned)K;
    const int k = (int)(en - (unsigned)row * (unsigned)K);
    uint32_t argw = ~0u;
    float gy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ch < C2) {
      argw = *reinterpret_cast<const uint32_t*>(arg + row * C2 + ch);
      nm_gy(g, out, row, C2, ch, relu_out, gy);
    }
    const float4 cv = (CENTER && on) ? nm_ld4(center + row * C1 + ch) : zero;
    float e[4];
    if (nm_edge_grad(argw, gy, k, wT, C1, ch, on, e)) nm_masked_add(xv, cv, e, acc);
  }
  if (on) *reinterpret_cast<float4*>(grad_x + r * C1 + ch) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// partial[(chunk (C1 + 1) + i) C2 + c] = sum over the rows chunk, chunk + chunks, ... of gy[c] h_i(slot arg[c]); row
// i = C1: the sum of gy[c].  G lanes (4 channels each) per column; a workgroup of min(32 G, 256) lanes.
template <int G, bool CENTER>
__global__ __launch_bounds__(kNmBlock) void nm_grad_w_kernel(
    const float* __restrict__ g, const float* __restrict__ out, const uint8_t* __restrict__ arg,
    const float* __restrict__ x, const float* __restrict__ center, const int64_t* __restrict__ idx,
    const int64_t* __restrict__ lengths, int64_t rows, int L, int K, int M, int C1, int C2, int relu_out,
    float* __restrict__ partial) {
  constexpr int GR = kNmBlock / G >= 32 ? 32 : kNmBlock / G, CP = 32 / GR;  // column groups, columns per group
  const int grp = threadIdx.x / G, ch = (threadIdx.x % G) * 4;
  if (ch >= C1) return;  // (the workgroup is GR G lanes; no barrier and no cross-lane step below)
  const int c0 = blockIdx.y * 32 + grp * CP;
  float acc[CP][4], bacc[CP];
#pragma unroll
  for (int p = 0; p < CP; ++p) acc[p][0] = acc[p][1] = acc[p][2] = acc[p][3] = bacc[p] = 0.0f;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t n = row / L;
    const int64_t len = lengths == nullptr ? INT64_MAX : lengths[n];
    float4 cv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (CENTER) cv = nm_ld4(center + row * C1 + ch);
    int k[CP];
    float gy[CP];
    int64_t m[CP];
#pragma unroll
    for (int p = 0; p < CP; ++p) {  // the loads of every column before the first fmaf
      const int c = c0 + p;
      k[p] = 255, gy[p] = 0.0f, m[p] = -1;
      if (c < C2) {
        k[p] = arg[row * C2 + c];
        gy[p] = (relu_out && !(out[row * C2 + c] > 0.0f)) ? 0.0f : g[row * C2 + c];
      }
      if (k[p] < K) m[p] = idx[row * K + k[p]];
      if (!(m[p] >= 0 && m[p] < M && k[p] < len)) m[p] = -1;  // (a slot the forward cannot have chosen is not followed)
    }
    float4 xv[CP];
#pragma unroll
    for (int p = 0; p < CP; ++p) xv[p] = m[p] >= 0 ? nm_ld4(x + (n * M + m[p]) * C1 + ch) : cv;
#pragma unroll
    for (int p = 0; p < CP; ++p) {
      if (m[p] < 0) continue;
      const float a[4] = {xv[p].x + cv.x, xv[p].y + cv.y, xv[p].z + cv.z, xv[p].w + cv.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_fmaf(gy[p], a[q] > 0.0f ? a[q] : 0.0f, acc[p][q]);
      bacc[p] = bacc[p] + gy[p];
    }
  }
  float* __restrict__ dst = partial + (int64_t)blockIdx.x * (C1 + 1) * C2;
#pragma unroll
  for (int p = 0; p < CP; ++p) {
    const int c = c0 + p;
    if (c >= C2) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[(ch + q) * C2 + c] = acc[p][q];
    if (ch == 0) dst[C1 * C2 + c] = bacc[p];
  }
}

struct NmWs {
  DetWs det;
  float* wT;       // (C2, C1)
  float* partial;  // (chunks, C1 + 1, C2)
};

// the inverted table of backward_det.h, then the transposed weight and the partial sums: nothing grows with K C1 or K C2
static size_t nm_carve(NmWs* ws, void* base, int64_t N, int64_t L, int64_t K, int64_t M, int64_t C1, int64_t C2) {
  NmWs w;
  Carver c(base);
  w.det.keys_in = nullptr;
  c.off = det_carve(base ? &w.det : nullptr, base, N, L, K, M);
  w.wT = (float*)c.take(sizeof(float) * (size_t)(C1 * C2));
  w.partial = (float*)c.take(sizeof(float) * (size_t)(nm_chunks(N * L) * (C1 + 1) * C2));
  if (ws) *ws = w;
  return c.off;
}

static bool nm_sizes_ok(int64_t N, int64_t L, int64_t M, int64_t K, int64_t C1, int64_t C2) {
  return nm_index_ok(N, L, M, K) && C1 >= 4 && C1 <= kNmMaxC && C1 % 4 == 0 && C2 >= 4 && C2 <= kNmMaxC && C2 % 4 == 0;
}

constexpr Ints<1, 2, 4> kNmBlocks{};        // 32-column blocks: the smallest NB >= ceil(C2 / 32)
constexpr Ints<8, 16, 32, 64> kNmSteps{};   // k-step pairs: the smallest KS >= C1 / 2
constexpr Ints<1, 2, 4, 8, 16, 32> kNmGroups{};  // grad_w: lanes per column, the smallest G >= C1 / 4

}  // namespace pointops

using namespace pointops;

#define NM_BAD_SIZES \
  ": bad sizes (C1 and C2 multiples of 4 in [4, 128], 1 <= K <= 255; N L K must be below 2^31 and N M below 2^31 - 1)"

extern "C" size_t pointops_neighbor_mlp_max_backward_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M,
                                                                     int64_t C1, int64_t C2) {
  if (!nm_sizes_ok(N, L, M, K, C1, C2)) return 0;
  return nm_carve(nullptr, nullptr, N, L, K, M, C1, C2);
}

extern "C" int pointops_neighbor_mlp_max(const float* x, const int64_t* idx, const int64_t* lengths,
                                         const float* center, const float* weight, const float* bias, int64_t N,
                                         int64_t L, int64_t M, int64_t K, int64_t C1, int64_t C2, int relu_out,
                                         float* out, uint8_t* arg, void* stream_) {
  POINTOPS_REQUIRE(nm_sizes_ok(N, L, M, K, C1, C2), "neighbor_mlp_max" NM_BAD_SIZES);
  const int64_t rows = N * L;
  if (rows == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE(idx != nullptr && weight != nullptr && out != nullptr && arg != nullptr && (x != nullptr || N * M == 0),
                   "neighbor_mlp_max: null pointer");
  POINTOPS_REQUIRE(nm_aligned(x, center, nullptr, nullptr), "neighbor_mlp_max: x and center must be 16-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  with_bucket(kNmBlocks, (int)ceil_div(C2, 32), [&](auto NB) {
    with_bucket(kNmSteps, (int)(C1 / 2), [&](auto KS) {
      with_exact<0>(Ints<1>{}, center != nullptr ? 1 : 0, [&](auto CEN) {
        constexpr int nb = decltype(NB)::value, ks = decltype(KS)::value;
        constexpr int R = 32 * nm_row_tiles(nb, ks);
        hipLaunchKernelGGL((nm_forward_kernel<nb, ks, decltype(CEN)::value != 0>), dim3((unsigned)ceil_div(rows, R)),
                           dim3(kNmBlock), 0, stream, x, idx, lengths, center, weight, bias, rows, (int)L, (int)K, (int)M,
                           (int)C1, (int)C2, relu_out, out, arg);
      });
    });
  });
  return check_launch("neighbor_mlp_max");
}

extern "C" int pointops_neighbor_mlp_max_backward(const float* grad_out, const float* x, const int64_t* idx,
                                                  const int64_t* lengths, const float* center, const float* weight,
                                                  const float* out, const uint8_t* arg, int64_t N, int64_t L, int64_t M,
                                                  int64_t K, int64_t C1, int64_t C2, int relu_out, float* grad_x,
                                                  float* grad_center, float* grad_weight, float* grad_bias,
                                                  void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(nm_sizes_ok(N, L, M, K, C1, C2), "neighbor_mlp_max_backward" NM_BAD_SIZES);
  POINTOPS_REQUIRE(grad_center == nullptr || center != nullptr, "neighbor_mlp_max_backward: grad_center needs center");
  const int64_t rows = N * L, targets = N * M;
  POINTOPS_REQUIRE(weight != nullptr && (rows == 0 || (grad_out != nullptr && idx != nullptr && out != nullptr &&
                                                       arg != nullptr)) &&
                       (x != nullptr || targets == 0 || rows == 0),
                   "neighbor_mlp_max_backward: null pointer");
  POINTOPS_REQUIRE(nm_aligned(grad_out, x, center, out) && nm_aligned(grad_x, grad_center, nullptr, nullptr) &&
                       (uintptr_t)arg % 4 == 0,
                   "neighbor_mlp_max_backward: grad_out, x, center, out and the row gradients must be 16-byte aligned, "
                   "arg 4-byte");
  NmWs ws;
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, nm_carve(&ws, workspace, N, L, K, M, C1, C2)),
                             "neighbor_mlp_max_backward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const bool rowwise = (grad_x != nullptr && targets > 0) || (grad_center != nullptr && rows > 0);
  if (rowwise)
    hipLaunchKernelGGL(nm_transpose_kernel, dim3((unsigned)ceil_div(C1 * C2, 256)), dim3(256), 0, stream, weight,
                       (int)C1, (int)C2, ws.wT);
  if (grad_x != nullptr && targets > 0) {
    const int rc = det_invert(ws.det, idx, nullptr, lengths, N, L, K, M, stream);
    if (rc != POINTOPS_OK) return rc;
    with_exact<0>(Ints<1>{}, center != nullptr ? 1 : 0, [&](auto CEN) {
      hipLaunchKernelGGL((nm_grad_x_kernel<decltype(CEN)::value != 0>), dim3((unsigned)ceil_div(targets, kNmBlock / 32)),
                         dim3(kNmBlock), 0, stream, grad_out, out, arg, x, center, ws.wT, ws.det.vals_out,
                         ws.det.seg_start, ws.det.seg_end, targets, (int)K, (int)C1, (int)C2, relu_out, grad_x);
    });
  }
  if (grad_center != nullptr && rows > 0)
    hipLaunchKernelGGL(nm_grad_center_kernel, dim3((unsigned)ceil_div(rows, kNmBlock / 32)), dim3(kNmBlock), 0, stream,
                       grad_out, out, arg, x, center, idx, lengths, ws.wT, rows, (int)L, (int)K, (int)M, (int)C1,
                       (int)C2, relu_out, grad_center);
  if (grad_weight != nullptr || grad_bias != nullptr) {
    const int64_t chunks = nm_chunks(rows);  // (no rows: every lane writes its zeros)
    with_bucket(kNmGroups, (int)(C1 / 4), [&](auto G) {
      with_exact<0>(Ints<1>{}, center != nullptr ? 1 : 0, [&](auto CEN) {
        constexpr int g = decltype(G)::value, lanes = 32 * g < kNmBlock ? 32 * g : kNmBlock;  // 32 columns of G lanes
        hipLaunchKernelGGL((nm_grad_w_kernel<g, decltype(CEN)::value != 0>),
                           dim3((unsigned)chunks, (unsigned)ceil_div(C2, 32)), dim3(lanes), 0, stream, grad_out, out,
                           arg, x, center, idx, lengths, rows, (int)L, (int)K, (int)M, (int)C1, (int)C2, relu_out,
                           ws.partial);
      });
    });
    hipLaunchKernelGGL(nm_sum_partials_kernel<float>, dim3((unsigned)ceil_div((C1 + 1) * C2, 256)), dim3(256), 0, stream,
                       ws.partial, (int)chunks, (int)C1, (int)C2, grad_weight, grad_bias);
  }
  return check_launch("neighbor_mlp_max_backward");
}

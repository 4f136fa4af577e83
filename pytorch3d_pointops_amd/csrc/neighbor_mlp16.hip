// neighbor_mlp16.hip -- NEIGHBOUR MLP-MAX on bfloat16 / float16 features (gfx950), on the 16-deep matrix instructions
// v_mfma_f32_32x32x16_bf16 / _f16 with fp32 accumulation.  The definition is the "16-bit features" part of the NEIGHBOUR
// MLP-MAX block of include/pointops_amd.h; the slot staging, the chunks and the summing of partials are neighbor_mlp.h's,
// shared with the float32 kernels of neighbor_mlp.hip, and the instruction wrapper is mfma16.h's.  T is __bf16 or _Float16.
//
//   pack      weight is rewritten once per call into wT[ceil32(C2)][Kp = ceil16(C1)] of T, zero-padded: the B-fragment of
//             a 16-deep step (k = 16 s + 8 h + [0, 8) of column c) is one 16-byte load with no tail predicate, and the
//             backward's e chain reads wT[c][i .. i + 7] as 16 bytes per lane.
//   forward   as neighbor_mlp.hip, 32 query rows at the same slot are the M side and the kernel loops over slots; a wave
//             keeps the ceil(C1 / 16) B-fragments of its 32-column block in KS (bucketed 1, 2, 4, 8, 16) x 4 registers.
//             The matrix stage is 8 times shorter than the float32 one, so ONE barrier pair serves S slots: the tile
//             holds S slots of the workgroup's R rows, R S = 128 (row, slot) pairs for C1 <= 128 and 64 above, with
//             R = 128, 64, 32 for NB = 1, 2, 4 column blocks (C1 > 128: R = 64, 64, 32).  The pairs are gathered 16 bytes
//             = 8 channels per lane INTO REGISTERS (the loads of the next group are issued before the MFMAs of this one),
//             widened, center (in registers per pair) added, ReLU, rounded ONCE to T and written to the tile, whose row
//             stride 16 KS + 8 elements is an odd number of 16-byte units: the A-fragment of a step is one conflict-free
//             16-byte LDS read.  A wave runs its S accumulators one after another and applies the max update S times in
//             ascending k.  C2 > 128 takes a second grid dimension over 128-column slices (the rows are gathered once
//             per slice).
//   grad_c    a half wave per query row, 8 channels i per lane (256 fit).  A lane holds CPL = 4 (C2 <= 128) or 8 columns:
//             CPL ballots per valid slot find the columns with arg == k, walked ascending, e = fmaf(gy[c], wT[c][i..i+7],
//             e) in fp32.  h is recomputed and rounded as the forward does; the mask is h > 0; one rounding at the store.
//   grad_x    the inverted table of backward_det.h, a half wave per TARGET row, the same e per entry.
//   grad_w/b  workgroups (row chunk, 32-column block), G >= C1 / 8 lanes per column with acc[8 channels] in fp32; the
//             per-chunk partials are added in ascending order and rounded once (nm_sum_partials_kernel<T>).
// No float atomics; every output element is written once.  Fixed launch sequences, nothing is read back.
#include "mfma16.h"
#include "neighbor_mlp.h"

namespace pointops {

constexpr int kNm16MaxC = 256;
constexpr int kNm16Pad = 8;                                      // elements: one 16-byte unit
constexpr int kNm16Slice = 128;                                  // columns of a forward workgroup
constexpr int64_t kNm16MaxPartial = (int64_t)1024 * 129 * 128;  // floats: the float32 path's largest partial plane

constexpr int nm16_pairs(int KS) { return KS > 8 ? 64 : 128; }  // (row, slot) pairs of a tile
constexpr int nm16_rows(int NB, int KS) { return NB == 1 ? nm16_pairs(KS) : (NB == 2 ? 64 : 32); }
static inline int nm16_up(int64_t v, int to) { return (int)((v + to - 1) / to * to); }

inline int64_t nm16_chunks(int64_t rows, int64_t C1, int64_t C2) {
  const int64_t c = nm_chunks(rows), most = kNm16MaxPartial / ((C1 + 1) * C2);
  return c < most ? c : most;
}

// wT[o Kp + k] = weight[k C2 + o], 0 past C1 or C2
template <class T>
__global__ __launch_bounds__(256) void nm16_pack_kernel(const T* __restrict__ weight, int C1, int C2, int Kp, int Op,
                                                        T* __restrict__ wT) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Op * Kp) return;
  const int o = i / Kp, k = i - o * Kp;
  wT[i] = (o < C2 && k < C1) ? weight[k * C2 + o] : (T)0.0f;
}

template <class T, int NB, int KS, bool CENTER>
__global__ __launch_bounds__(kNmBlock) void nm16_forward_kernel(
    const T* __restrict__ x, const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths,
    const T* __restrict__ center, const T* __restrict__ wT, const T* __restrict__ bias, int64_t rows, int L, int K,
    int M, int C1, int C2, int relu_out, T* __restrict__ out, uint8_t* __restrict__ arg) {
  typedef typename Nc16<T>::V V;
  constexpr int R = nm16_rows(NB, KS), S = nm16_pairs(KS) / R, RT = R / 32, STRIDE = 16 * KS + kNm16Pad, G8 = 2 * KS;
  constexpr int UNITS = R * S * G8, Q = UNITS / kNmBlock;  // 16-byte pieces of the tile, per lane
  static_assert(UNITS % kNmBlock == 0 && (STRIDE / 8) % 2 == 1, "whole units per lane, odd stride in 16-byte units");
  __shared__ uint4 s_tile[R * S * STRIDE / 8];  // [slot of the group][row][STRIDE] of T
  __shared__ int s_src[kNmWin * R];             // [slot][row]
  __shared__ uint32_t s_mask[kNmWin * RT];
  T* s_A = reinterpret_cast<T*>(s_tile);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5, c = lane & 31;
  const int cb = wave % NB, rt = (wave / NB) % RT;
  const int Kp = (C1 + 15) & ~15, Op = (C2 + 31) & ~31;
  const int oc = blockIdx.y * kNm16Slice + cb * 32 + c;
  const bool mma = wave < NB * RT && oc - c < Op;  // (wave-uniform; a column block past the pack does nothing)
  const bool col = oc < C2;
  const int64_t row0 = (int64_t)blockIdx.x * R;

  V b[KS];  // B[k = 16 q + 8 h + j][o = oc], resident
#pragma unroll
  for (int q = 0; q < KS; ++q)
    b[q] = (mma && 16 * q < Kp) ? *reinterpret_cast<const V*>(wT + (int64_t)oc * Kp + 16 * q + 8 * h) : nc16_zero<T>();
  const float bv = (col && bias != nullptr) ? (float)bias[oc] : 0.0f;

  int up[Q], uc[Q];  // the unit's pair = (slot of the group) R + row: its tile row, and its source past the group's first
  V cen[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int u = t + kNmBlock * q;
    up[q] = u / G8, uc[q] = (u % G8) * 8;
    cen[q] = nc16_zero<T>();
    const int64_t row = row0 + up[q] % R;
    if (CENTER && uc[q] < C1 && row < rows) cen[q] = *reinterpret_cast<const V*>(center + row * C1 + uc[q]);
  }

  float best[16];
  int slot[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) best[r] = 0.0f, slot[r] = 255;
  uint32_t seen = 0;

  for (int k0 = 0; k0 < K; k0 += kNmWin) {
    const int kt = min(kNmWin, K - k0);
    nm_stage<R, RT>(idx, lengths, row0, rows, L, K, M, k0, kt, s_src, s_mask);

    V v[Q];
    auto gather = [&](int g0) {  // slots g0 .. g0 + S - 1 of the window; past kt: zeros
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int at = g0 * R + up[q];
        const int s = (uc[q] < C1 && at < kt * R) ? s_src[at] : -1;
        v[q] = nc16_zero<T>();
        if (s >= 0) v[q] = *reinterpret_cast<const V*>(x + (int64_t)s * C1 + uc[q]);
      }
    };
    gather(0);
    for (int g0 = 0; g0 < kt; g0 += S) {
      __syncthreads();  // the MFMAs of the group before have read the tile (first group: the masks are written)
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (uc[q] >= Kp) continue;  // (units in [C1, Kp) write the zeros of the k padding)
        V hv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float a = (float)v[q][j];
          if (CENTER) a = a + (float)cen[q][j];
          hv[j] = (T)(a > 0.0f ? a : 0.0f);
        }
        *reinterpret_cast<V*>(s_A + up[q] * STRIDE + uc[q]) = hv;
      }
      __syncthreads();
      if (g0 + S < kt) gather(g0 + S);  // in flight during the MFMAs
      if (!mma) continue;
#pragma unroll
      for (int sl = 0; sl < S; ++sl) {
        const int kk = g0 + sl;
        if (kk >= kt) break;  // (uniform: the last group of a window may be partial)
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bv;
        const T* a = s_A + (sl * R + rt * 32 + c) * STRIDE + 8 * h;  // A[i = c][k = 16 q + 8 h + j]
#pragma unroll
        for (int q = 0; q < KS; ++q)
          if (16 * q < Kp) acc = Nc16<T>::mfma(*reinterpret_cast<const V*>(a + 16 * q), b[q], acc);
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
  }
  if (!mma || !col) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (row >= rows) continue;
    out[row * C2 + oc] = (T)((relu_out && !(best[r] > 0.0f)) ? 0.0f : best[r]);
    arg[row * C2 + oc] = (uint8_t)slot[r];
  }
}

// the arg bytes (argw, ~0 past C2) and gy of the lane's CPL columns cc .. cc + CPL - 1 of `row`
template <class T, int CPL>
__device__ __forceinline__ void nm16_gy(const T* __restrict__ g, const T* __restrict__ out,
                                        const uint8_t* __restrict__ arg, int64_t row, int C2, int cc, int relu_out,
                                        uint32_t (&argw)[CPL / 4], float (&gy)[CPL]) {
  typedef T VT __attribute__((ext_vector_type(CPL)));
#pragma unroll
  for (int w = 0; w < CPL / 4; ++w) argw[w] = ~0u;
#pragma unroll
  for (int q = 0; q < CPL; ++q) gy[q] = 0.0f;
  if (cc >= C2) return;
  const VT gv = *reinterpret_cast<const VT*>(g + row * C2 + cc), ov = *reinterpret_cast<const VT*>(out + row * C2 + cc);
#pragma unroll
  for (int w = 0; w < CPL / 4; ++w) argw[w] = *reinterpret_cast<const uint32_t*>(arg + row * C2 + cc + 4 * w);
#pragma unroll
  for (int q = 0; q < CPL; ++q) gy[q] = (relu_out && !((float)ov[q] > 0.0f)) ? 0.0f : (float)gv[q];
}

// e[:] = the chain from +0.0f, over the columns c ascending whose arg byte is k, of fmaf(gy[c], wT[c][ch .. ch + 7], e).
// A half wave (32 lanes) per row: lane j holds the arg bytes and gy of columns CPL j .. CPL j + CPL - 1.  Call with the
// whole half wave; returns whether any column matched.
template <class T, int CPL>
__device__ __forceinline__ bool nm16_edge_grad(const uint32_t (&argw)[CPL / 4], const float (&gy)[CPL], int k,
                                               const T* __restrict__ wT, int Kp, int ch, bool on, float (&e)[8]) {
  typedef typename Nc16<T>::V V;
  const int half = (threadIdx.x & 63) >> 5;
  uint32_t m[CPL], any = 0;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    m[q] = (uint32_t)(__ballot((int)((argw[q >> 2] >> (8 * (q & 3))) & 255u) == k) >> (32 * half));
    any |= m[q];
  }
#pragma unroll
  for (int x = 0; x < 8; ++x) e[x] = 0.0f;
  const bool hit = any != 0;
  while (any != 0) {
    const int jj = __ffs(any) - 1;
    any &= any - 1;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      if (!((m[q] >> jj) & 1u)) continue;  // (uniform over the half wave)
      const float gyc = __shfl(gy[q], jj, 32);
      if (on) {
        const V w = *reinterpret_cast<const V*>(wT + (int64_t)(CPL * jj + q) * Kp + ch);
#pragma unroll
        for (int x = 0; x < 8; ++x) e[x] = __builtin_fmaf(gyc, (float)w[x], e[x]);
      }
    }
  }
  return hit;
}

// h_j = rnd_T(relu(fl32(x_j + c_j))), as the forward writes it to its tile
template <class T>
__device__ __forceinline__ float nm16_hidden(T xv, T cv) {
  const float a = (float)xv + (float)cv;
  return (float)(T)(a > 0.0f ? a : 0.0f);
}

// acc[:] += (h > 0 ? e : 0)
template <class T>
__device__ __forceinline__ void nm16_masked_add(typename Nc16<T>::V xv, typename Nc16<T>::V cv, const float (&e)[8],
                                                float (&acc)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = acc[j] + (nm16_hidden<T>(xv[j], cv[j]) > 0.0f ? e[j] : 0.0f);
}

template <class T>
__device__ __forceinline__ void nm16_store(T* __restrict__ dst, const float (&acc)[8]) {
  typename Nc16<T>::V o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (T)acc[j];
  *reinterpret_cast<typename Nc16<T>::V*>(dst) = o;
}

// grad_center[row, :] = sum over the valid slots, ascending, of d
template <class T, int CPL>
__global__ __launch_bounds__(kNmBlock) void nm16_grad_center_kernel(
    const T* __restrict__ g, const T* __restrict__ out, const uint8_t* __restrict__ arg, const T* __restrict__ x,
    const T* __restrict__ center, const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths,
    const T* __restrict__ wT, int64_t rows, int L, int K, int M, int C1, int C2, int relu_out,
    T* __restrict__ grad_center) {
  typedef typename Nc16<T>::V V;
  const int j = threadIdx.x & 31, ch = 8 * j, Kp = (C1 + 15) & ~15;
  const int64_t row = (int64_t)blockIdx.x * (kNmBlock / 32) + (threadIdx.x >> 5);
  if (row >= rows) return;  // (a whole half wave; no barrier below)
  const bool on = ch < C1;
  uint32_t argw[CPL / 4];
  float gy[CPL];
  nm16_gy<T, CPL>(g, out, arg, row, C2, CPL * j, relu_out, argw, gy);
  const V cv = on ? *reinterpret_cast<const V*>(center + row * C1 + ch) : nc16_zero<T>();
  const int64_t n = row / L;
  const int64_t len = lengths == nullptr ? INT64_MAX : lengths[n];
  float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < K; ++k) {
    const int64_t m = idx[row * K + k];
    if (!(m >= 0 && m < M && k < len)) continue;  // (uniform over the half wave)
    float e[8];
    if (!nm16_edge_grad<T, CPL>(argw, gy, k, wT, Kp, ch, on, e) || !on) continue;
    nm16_masked_add<T>(*reinterpret_cast<const V*>(x + (n * M + m) * C1 + ch), cv, e, acc);
  }
  if (on) nm16_store<T>(grad_center + row * C1 + ch, acc);
}

// grad_x[r, :] = sum over the entries of target row r, in table order, of d
template <class T, int CPL, bool CENTER>
__global__ __launch_bounds__(kNmBlock) void nm16_grad_x_kernel(
    const T* __restrict__ g, const T* __restrict__ out, const uint8_t* __restrict__ arg, const T* __restrict__ x,
    const T* __restrict__ center, const T* __restrict__ wT, const unsigned* __restrict__ vals,
    const int* __restrict__ seg_start, const int* __restrict__ seg_end, int64_t targets, int K, int C1, int C2,
    int relu_out, T* __restrict__ grad_x) {
  typedef typename Nc16<T>::V V;
  const int j = threadIdx.x & 31, ch = 8 * j, Kp = (C1 + 15) & ~15;
  const int64_t r = (int64_t)blockIdx.x * (kNmBlock / 32) + (threadIdx.x >> 5);
  if (r >= targets) return;  // (a whole half wave; no barrier below)
  const bool on = ch < C1;
  const int t0 = seg_start[r], t1 = seg_end[r];
  const V xv = (on && t0 < t1) ? *reinterpret_cast<const V*>(x + r * C1 + ch) : nc16_zero<T>();
  float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = t0; t < t1; ++t) {
    const unsigned en = vals[t];
    const int64_t row = en / (unsigned)K;
    const int k = (int)(en - (unsigned)row * (unsigned)K);
    uint32_t argw[CPL / 4];
    float gy[CPL];
    nm16_gy<T, CPL>(g, out, arg, row, C2, CPL * j, relu_out, argw, gy);
    const V cv = (CENTER && on) ? *reinterpret_cast<const V*>(center + row * C1 + ch) : nc16_zero<T>();
    float e[8];
    if (nm16_edge_grad<T, CPL>(argw, gy, k, wT, Kp, ch, on, e)) nm16_masked_add<T>(xv, cv, e, acc);
  }
  if (on) nm16_store<T>(grad_x + r * C1 + ch, acc);
}

// partial[(chunk (C1 + 1) + i) C2 + c] = sum over the rows chunk, chunk + chunks, ... of gy[c] h_i(slot arg[c]); row
// i = C1: the sum of gy[c].  G lanes (8 channels each) per column; a workgroup of min(32 G, 256) lanes.
template <class T, int G, bool CENTER>
__global__ __launch_bounds__(kNmBlock) void nm16_grad_w_kernel(
    const T* __restrict__ g, const T* __restrict__ out, const uint8_t* __restrict__ arg, const T* __restrict__ x,
    const T* __restrict__ center, const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths, int64_t rows,
    int L, int K, int M, int C1, int C2, int relu_out, float* __restrict__ partial) {
  typedef typename Nc16<T>::V V;
  constexpr int GR = kNmBlock / G >= 32 ? 32 : kNmBlock / G, CP = 32 / GR;  // column groups, columns per group
  const int grp = threadIdx.x / G, ch = (threadIdx.x % G) * 8;
  if (ch >= C1) return;  // (the workgroup is GR G lanes; no barrier and no cross-lane step below)
  const int c0 = blockIdx.y * 32 + grp * CP;
  float acc[CP][8], bacc[CP];
#pragma unroll
  for (int p = 0; p < CP; ++p) {
    bacc[p] = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[p][q] = 0.0f;
  }
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t n = row / L;
    const int64_t len = lengths == nullptr ? INT64_MAX : lengths[n];
    V cv = nc16_zero<T>();
    if (CENTER) cv = *reinterpret_cast<const V*>(center + row * C1 + ch);
    int k[CP];
    float gy[CP];
    int64_t m[CP];
#pragma unroll
    for (int p = 0; p < CP; ++p) {  // the loads of every column before the first fmaf
      const int c = c0 + p;
      k[p] = 255, gy[p] = 0.0f, m[p] = -1;
      if (c < C2) {
        k[p] = arg[row * C2 + c];
        gy[p] = (relu_out && !((float)out[row * C2 + c] > 0.0f)) ? 0.0f : (float)g[row * C2 + c];
      }
      if (k[p] < K) m[p] = idx[row * K + k[p]];
      if (!(m[p] >= 0 && m[p] < M && k[p] < len)) m[p] = -1;  // (a slot the forward cannot have chosen is not followed)
    }
    V xv[CP];
#pragma unroll
    for (int p = 0; p < CP; ++p) xv[p] = m[p] >= 0 ? *reinterpret_cast<const V*>(x + (n * M + m[p]) * C1 + ch) : cv;
#pragma unroll
    for (int p = 0; p < CP; ++p) {
      if (m[p] < 0) continue;
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[p][q] = __builtin_fmaf(gy[p], nm16_hidden<T>(xv[p][q], cv[q]), acc[p][q]);
      bacc[p] = bacc[p] + gy[p];
    }
  }
  float* __restrict__ dst = partial + (int64_t)blockIdx.x * (C1 + 1) * C2;
#pragma unroll
  for (int p = 0; p < CP; ++p) {
    const int c = c0 + p;
    if (c >= C2) continue;
#pragma unroll
    for (int q = 0; q < 8; ++q) dst[(ch + q) * C2 + c] = acc[p][q];
    if (ch == 0) dst[C1 * C2 + c] = bacc[p];
  }
}

struct Nm16Ws {
  DetWs det;
  void* wT;        // (ceil32(C2), ceil16(C1)) of T
  float* partial;  // (chunks, C1 + 1, C2)
};

// forward: the pack; backward: the inverted table of backward_det.h, the pack and the partial sums -- beyond the table,
// nothing depends on K
static size_t nm16_carve(Nm16Ws* ws, void* base, bool backward, int64_t N, int64_t L, int64_t K, int64_t M, int64_t C1,
                         int64_t C2) {
  Nm16Ws w;
  Carver c(base);
  w.det.keys_in = nullptr;
  w.partial = nullptr;
  if (backward) c.off = det_carve(base ? &w.det : nullptr, base, N, L, K, M);
  w.wT = c.take((size_t)2 * nm16_up(C2, 32) * nm16_up(C1, 16));
  if (backward) w.partial = (float*)c.take(sizeof(float) * (size_t)(nm16_chunks(N * L, C1, C2) * (C1 + 1) * C2));
  if (ws) *ws = w;
  return c.off;
}

static bool nm16_sizes_ok(int64_t N, int64_t L, int64_t M, int64_t K, int64_t C1, int64_t C2) {
  return nm_index_ok(N, L, M, K) && C1 >= 8 && C1 <= kNm16MaxC && C1 % 8 == 0 && C2 >= 8 && C2 <= kNm16MaxC &&
         C2 % 8 == 0;
}

constexpr Ints<1, 2, 4> kNm16Blocks{};               // 32-column blocks of a slice: the smallest NB >= ceil(C2 / 32)
constexpr Ints<1, 2, 4, 8, 16> kNm16Steps{};         // 16-deep steps: the smallest KS >= ceil(C1 / 16)
constexpr Ints<1, 2, 4, 8, 16, 32> kNm16Groups{};    // grad_w: lanes per column, the smallest G >= C1 / 8

template <class T>
static void nm16_pack(const void* weight, int64_t C1, int64_t C2, const Nm16Ws& ws, hipStream_t stream) {
  const int Kp = nm16_up(C1, 16), Op = nm16_up(C2, 32);
  hipLaunchKernelGGL(nm16_pack_kernel<T>, dim3((unsigned)ceil_div(Op * Kp, 256)), dim3(256), 0, stream, (const T*)weight,
                     (int)C1, (int)C2, Kp, Op, (T*)ws.wT);
}

template <class T>
static int nm16_forward(const void* x, const int64_t* idx, const int64_t* lengths, const void* center,
                        const void* weight, const void* bias, int64_t N, int64_t L, int64_t M, int64_t K, int64_t C1,
                        int64_t C2, int relu_out, void* out, uint8_t* arg, const Nm16Ws& ws, hipStream_t stream) {
  const int64_t rows = N * L;
  nm16_pack<T>(weight, C1, C2, ws, stream);
  const int64_t slices = ceil_div(C2, kNm16Slice);
  with_bucket(kNm16Blocks, (int)ceil_div(slices > 1 ? kNm16Slice : C2, 32), [&](auto NB) {
    with_bucket(kNm16Steps, (int)ceil_div(C1, 16), [&](auto KS) {
      with_exact<0>(Ints<1>{}, center != nullptr ? 1 : 0, [&](auto CEN) {
        constexpr int nb = decltype(NB)::value, ks = decltype(KS)::value;
        hipLaunchKernelGGL((nm16_forward_kernel<T, nb, ks, decltype(CEN)::value != 0>),
                           dim3((unsigned)ceil_div(rows, nm16_rows(nb, ks)), (unsigned)slices), dim3(kNmBlock), 0, stream,
                           (const T*)x, idx, lengths, (const T*)center, (const T*)ws.wT, (const T*)bias, rows, (int)L,
                           (int)K, (int)M, (int)C1, (int)C2, relu_out, (T*)out, arg);
      });
    });
  });
  return check_launch("neighbor_mlp_max16");
}

template <class T>
static int nm16_backward(const void* grad_out_, const void* x_, const int64_t* idx, const int64_t* lengths,
                         const void* center_, const void* weight, const void* out_, const uint8_t* arg, int64_t N,
                         int64_t L, int64_t M, int64_t K, int64_t C1, int64_t C2, int relu_out, void* grad_x,
                         void* grad_center, void* grad_weight, void* grad_bias, const Nm16Ws& ws, hipStream_t stream) {
  const T *grad_out = (const T*)grad_out_, *x = (const T*)x_, *center = (const T*)center_, *out = (const T*)out_;
  const T* wT = (const T*)ws.wT;
  const int64_t rows = N * L, targets = N * M;
  const bool need_x = grad_x != nullptr && targets > 0, need_c = grad_center != nullptr && rows > 0;
  if (need_x || need_c) nm16_pack<T>(weight, C1, C2, ws, stream);
  if (need_x) {
    const int rc = det_invert(ws.det, idx, nullptr, lengths, N, L, K, M, stream);
    if (rc != POINTOPS_OK) return rc;
    with_exact<4>(Ints<8>{}, C2 > 128 ? 8 : 4, [&](auto CPL) {
      with_exact<0>(Ints<1>{}, center != nullptr ? 1 : 0, [&](auto CEN) {
        hipLaunchKernelGGL((nm16_grad_x_kernel<T, decltype(CPL)::value, decltype(CEN)::value != 0>),
                           dim3((unsigned)ceil_div(targets, kNmBlock / 32)), dim3(kNmBlock), 0, stream, grad_out, out, arg,
                           x, center, wT, ws.det.vals_out, ws.det.seg_start, ws.det.seg_end, targets, (int)K, (int)C1,
                           (int)C2, relu_out, (T*)grad_x);
      });
    });
  }
  if (need_c)
    with_exact<4>(Ints<8>{}, C2 > 128 ? 8 : 4, [&](auto CPL) {
      hipLaunchKernelGGL((nm16_grad_center_kernel<T, decltype(CPL)::value>), dim3((unsigned)ceil_div(rows, kNmBlock / 32)),
                         dim3(kNmBlock), 0, stream, grad_out, out, arg, x, center, idx, lengths, wT, rows, (int)L, (int)K,
                         (int)M, (int)C1, (int)C2, relu_out, (T*)grad_center);
    });
  if (grad_weight != nullptr || grad_bias != nullptr) {
    const int64_t chunks = nm16_chunks(rows, C1, C2);  // (no rows: every lane writes its zeros)
    with_bucket(kNm16Groups, (int)(C1 / 8), [&](auto G) {
      with_exact<0>(Ints<1>{}, center != nullptr ? 1 : 0, [&](auto CEN) {
        constexpr int gl = decltype(G)::value, lanes = 32 * gl < kNmBlock ? 32 * gl : kNmBlock;  // 32 columns of G lanes
        hipLaunchKernelGGL((nm16_grad_w_kernel<T, gl, decltype(CEN)::value != 0>),
                           dim3((unsigned)chunks, (unsigned)ceil_div(C2, 32)), dim3(lanes), 0, stream, grad_out, out, arg,
                           x, center, idx, lengths, rows, (int)L, (int)K, (int)M, (int)C1, (int)C2, relu_out, ws.partial);
      });
    });
    hipLaunchKernelGGL(nm_sum_partials_kernel<T>, dim3((unsigned)ceil_div((C1 + 1) * C2, 256)), dim3(256), 0, stream,
                       ws.partial, (int)chunks, (int)C1, (int)C2, (T*)grad_weight, (T*)grad_bias);
  }
  return check_launch("neighbor_mlp_max16_backward");
}

}  // namespace pointops

using namespace pointops;

#define NM16_BAD_SIZES                                                                                               \
  ": bad sizes (dtype 0 or 1, C1 and C2 multiples of 8 in [8, 256], 1 <= K <= 255; N L K must be below 2^31 and N M " \
  "below 2^31 - 1)"

static bool nm16_dtype_ok(int dtype) { return dtype == POINTOPS_DTYPE_BF16 || dtype == POINTOPS_DTYPE_F16; }

extern "C" size_t pointops_neighbor_mlp_max16_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M, int64_t C1,
                                                              int64_t C2) {
  if (!nm16_sizes_ok(N, L, M, K, C1, C2)) return 0;
  return nm16_carve(nullptr, nullptr, false, N, L, K, M, C1, C2);
}

extern "C" size_t pointops_neighbor_mlp_max16_backward_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M,
                                                                       int64_t C1, int64_t C2) {
  if (!nm16_sizes_ok(N, L, M, K, C1, C2)) return 0;
  return nm16_carve(nullptr, nullptr, true, N, L, K, M, C1, C2);
}

extern "C" int pointops_neighbor_mlp_max16(const void* x, const int64_t* idx, const int64_t* lengths, const void* center,
                                           const void* weight, const void* bias, int dtype, int64_t N, int64_t L,
                                           int64_t M, int64_t K, int64_t C1, int64_t C2, int relu_out, void* out,
                                           uint8_t* arg, void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(nm16_dtype_ok(dtype) && nm16_sizes_ok(N, L, M, K, C1, C2), "neighbor_mlp_max16" NM16_BAD_SIZES);
  const int64_t rows = N * L;
  POINTOPS_REQUIRE(weight != nullptr && (rows == 0 || (idx != nullptr && out != nullptr && arg != nullptr)) &&
                       (x != nullptr || N * M == 0 || rows == 0),
                   "neighbor_mlp_max16: null pointer");
  POINTOPS_REQUIRE(nm_aligned(x, center, nullptr, nullptr), "neighbor_mlp_max16: x and center must be 16-byte aligned");
  Nm16Ws ws;
  POINTOPS_REQUIRE_WORKSPACE(
      workspace_fits(workspace, workspace_bytes, nm16_carve(&ws, workspace, false, N, L, K, M, C1, C2)),
      "neighbor_mlp_max16: workspace too small");
  if (rows == 0) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  return dtype == POINTOPS_DTYPE_BF16 ? nm16_forward<__bf16>(x, idx, lengths, center, weight, bias, N, L, M, K, C1, C2,
                                                             relu_out, out, arg, ws, stream)
                                      : nm16_forward<_Float16>(x, idx, lengths, center, weight, bias, N, L, M, K, C1, C2,
                                                               relu_out, out, arg, ws, stream);
}

extern "C" int pointops_neighbor_mlp_max16_backward(const void* grad_out, const void* x, const int64_t* idx,
                                                    const int64_t* lengths, const void* center, const void* weight,
                                                    const void* out, const uint8_t* arg, int dtype, int64_t N, int64_t L,
                                                    int64_t M, int64_t K, int64_t C1, int64_t C2, int relu_out,
                                                    void* grad_x, void* grad_center, void* grad_weight, void* grad_bias,
                                                    void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(nm16_dtype_ok(dtype) && nm16_sizes_ok(N, L, M, K, C1, C2),
                   "neighbor_mlp_max16_backward" NM16_BAD_SIZES);
  POINTOPS_REQUIRE(grad_center == nullptr || center != nullptr, "neighbor_mlp_max16_backward: grad_center needs center");
  const int64_t rows = N * L, targets = N * M;
  POINTOPS_REQUIRE(weight != nullptr && (rows == 0 || (grad_out != nullptr && idx != nullptr && out != nullptr &&
                                                       arg != nullptr)) &&
                       (x != nullptr || targets == 0 || rows == 0),
                   "neighbor_mlp_max16_backward: null pointer");
  POINTOPS_REQUIRE(nm_aligned(grad_out, x, center, out) && nm_aligned(grad_x, grad_center, nullptr, nullptr) &&
                       (uintptr_t)arg % 4 == 0,
                   "neighbor_mlp_max16_backward: grad_out, x, center, out and the row gradients must be 16-byte aligned, "
                   "arg 4-byte");
  Nm16Ws ws;
  POINTOPS_REQUIRE_WORKSPACE(
      workspace_fits(workspace, workspace_bytes, nm16_carve(&ws, workspace, true, N, L, K, M, C1, C2)),
      "neighbor_mlp_max16_backward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  return dtype == POINTOPS_DTYPE_BF16
             ? nm16_backward<__bf16>(grad_out, x, idx, lengths, center, weight, out, arg, N, L, M, K, C1, C2, relu_out,
                                     grad_x, grad_center, grad_weight, grad_bias, ws, stream)
             : nm16_backward<_Float16>(grad_out, x, idx, lengths, center, weight, out, arg, N, L, M, K, C1, C2, relu_out,
                                       grad_x, grad_center, grad_weight, grad_bias, ws, stream);
}

// neighbor_mlp2_16.hip -- NEIGHBOUR MLP-MAX with a second hidden layer, on bfloat16 / float16 features (gfx950):
//   h1 = rnd_T(relu(x[j] + center)),  h2 = rnd_T(relu(h1 @ weight + bias)),  out = rnd_T(act(max_k h2 @ weight2 + bias2))
// on v_mfma_f32_32x32x16_bf16 / _f16 with fp32 accumulation.  The definition is the "two layers" part of the NEIGHBOUR
// MLP-MAX block of include/pointops_amd.h; the slot staging and the summing of partials are neighbor_mlp.h's, the
// instruction wrapper is mfma16.h's.  T is __bf16 or _Float16.  C1, C2 <= 128, C3 <= 256.
//
//   pack      one kernel rewrites a matrix into B-fragment order dst[ceil32(columns)][ceil16(k)], zero-padded, so that a
//             fragment of a 16-deep step is one 16-byte load without a tail predicate.  The forward packs weight and
//             weight2 TRANSPOSED (k = the input channel); the backward's transposed products e3 @ weight2^T and
//             e2 @ weight^T have k = the OUTPUT channel, so their packs are the matrices as they lie, padded.
//   forward   a tile is 128 (row, slot) pairs: R = 64 rows x 2 slots (C3 <= 64) or 32 rows x 4 slots.  Rows are
//             gathered 16 bytes per lane into registers while the MFMAs of the tile before run, center added in fp32,
//             ReLU, rounded to T into LDS tile A1 (stride 16 KS1 + 8: an odd number of 16-byte units).
//             stage 1: the 4 pair tiles x NB1 column blocks of h1 @ weight are dealt so that a wave always has the same
//             column block of weight: its fragments stay in registers.  bias, ReLU and the ONE rounding to T are applied
//             in the accumulator's layout and written to LDS tile A2 (same odd stride).
//             stage 2, after one barrier: wave (column group, row tile) reads A2 as A-fragments against its resident
//             fragments of weight2 (two column blocks per wave for C3 > 128) and updates the running maximum and its
//             slot elementwise, S times in ascending k.  Two barriers per tile.
//   backward  one query-order kernel, workgroups persistent over tiles of 32 rows x 2 slots.  Per tile: h1 -> A1 and
//             e3 (gy where arg == k) -> E3; h2 = the forward's stage 1 and e2 = (E3 @ weight2^T) (h2 > 0) in the SAME
//             accumulator positions -> A2 and E2 (T); e1 = ((E2 + E2L) @ weight^T) (h1 > 0), E2L what the rounding of e2 dropped, summed over k in registers for
//             grad_center and written in T to the e1 workspace; grad_weight += A1^T (E2 + E2L) and grad_weight2 += (A2 + A2L)^T E3 with
//             the pair index as k (fragments read down the tiles' columns), in accumulators that live as long as the
//             workgroup and leave as per-workgroup partials, summed afterwards in ascending order
//             (nm_sum_partials_kernel).  grad_x is a pull of e1 over the inverted table of backward_det.h.
// No float atomics; every output element is written once.  Fixed launch sequences, nothing is read back.
#include "mfma16.h"
#include "neighbor_mlp.h"

namespace pointops {

constexpr int kNm2MaxC = 128;      // C1, C2
constexpr int kNm2MaxC3 = 256;
constexpr int kNm2MaxChunks = 256;  // backward workgroups: one set of weight-gradient partials each

static inline int nm2_up(int64_t v, int to) { return (int)((v + to - 1) / to * to); }
static inline int nm2_bucket(int64_t blocks) { return blocks <= 1 ? 1 : (blocks <= 2 ? 2 : 4); }
__device__ __forceinline__ int nm2_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }  // accumulator element r

// dst[o Kp + k] = src[o so + k sk], 0 past O or Kd
template <class T>
__global__ __launch_bounds__(256) void nm2_pack_kernel(const T* __restrict__ src, int O, int Kd, int so, int sk, int Op,
                                                       int Kp, T* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Op * Kp) return;
  const int o = i / Kp, k = i - o * Kp;
  dst[i] = (o < O && k < Kd) ? src[(int64_t)o * so + (int64_t)k * sk] : (T)0.0f;
}

template <class T, int NBW, int CB, int KS1, int KS2>
__global__ __launch_bounds__(kNmBlock) void nm2_forward_kernel(
    const T* __restrict__ x, const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths,
    const T* __restrict__ center, const T* __restrict__ wT, const T* __restrict__ bias, const T* __restrict__ w2T,
    const T* __restrict__ bias2, int64_t rows, int L, int K, int M, int C1, int C2, int C3, int relu_out,
    T* __restrict__ out, uint8_t* __restrict__ arg) {
  typedef typename Nc16<T>::V V;
  constexpr int RT = 4 / NBW, R = 32 * RT, S = 128 / R, NB1 = KS2 / 2, PT1 = 4 / NB1;
  constexpr int ST1 = 16 * KS1 + 8, ST2 = 16 * KS2 + 8, G8 = 2 * KS1, Q = 128 * G8 / kNmBlock;
  static_assert((ST1 / 8) % 2 == 1 && (ST2 / 8) % 2 == 1 && 128 * G8 % kNmBlock == 0, "odd strides, whole units per lane");
  __shared__ uint4 s_t1[128 * ST1 / 8];  // A1[slot of the group][row][ST1] of T
  __shared__ uint4 s_t2[128 * ST2 / 8];  // A2, the same pairs
  __shared__ int s_src[kNmWin * R];      // [slot][row]
  __shared__ uint32_t s_mask[kNmWin * RT];
  T* s_A1 = reinterpret_cast<T*>(s_t1);
  T* s_A2 = reinterpret_cast<T*>(s_t2);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5, c = lane & 31;
  const int Kp1 = (C1 + 15) & ~15, Kp2 = (C2 + 15) & ~15, Op1 = (C2 + 31) & ~31, Op2 = (C3 + 31) & ~31;
  const int64_t row0 = (int64_t)blockIdx.x * R;

  // stage 1: column block cb1 of weight for the pair tiles pt1, pt1 + PT1, ...
  const int cb1 = wave % NB1, pt1 = wave / NB1, oc1 = cb1 * 32 + c;
  const bool mma1 = cb1 * 32 < Op1;  // (wave-uniform)
  V b1[KS1];
#pragma unroll
  for (int q = 0; q < KS1; ++q)
    b1[q] = (mma1 && 16 * q < Kp1) ? *reinterpret_cast<const V*>(wT + (int64_t)oc1 * Kp1 + 16 * q + 8 * h) : nc16_zero<T>();
  const float bv1 = (oc1 < C2 && bias != nullptr) ? (float)bias[oc1] : 0.0f;

  // stage 2: row tile rt, column blocks cbw, cbw + NBW
  const int cbw = wave % NBW, rt = wave / NBW;
  V b2[CB][KS2];
  float bv2[CB];
  bool mma2[CB];
  int oc2[CB];
#pragma unroll
  for (int e = 0; e < CB; ++e) {
    oc2[e] = (cbw + NBW * e) * 32 + c;
    mma2[e] = oc2[e] - c < Op2;
#pragma unroll
    for (int q = 0; q < KS2; ++q)
      b2[e][q] = (mma2[e] && 16 * q < Kp2) ? *reinterpret_cast<const V*>(w2T + (int64_t)oc2[e] * Kp2 + 16 * q + 8 * h)
                                           : nc16_zero<T>();
    bv2[e] = (oc2[e] < C3 && bias2 != nullptr) ? (float)bias2[oc2[e]] : 0.0f;
  }

  // unit q of a lane is 16 bytes of pair up0 + UP q at channel uc: G8 divides the workgroup, so the channel is the lane's
  // own and the pairs' rows repeat after NC units -- NC center vectors stay in registers
  constexpr int UP = kNmBlock / G8, NC = R / UP > 0 ? (R / UP < Q ? R / UP : Q) : 1;
  static_assert(kNmBlock % G8 == 0 && (R % UP == 0 || UP % R == 0), "a lane's units share a channel; rows repeat");
  const int up0 = t / G8, uc = (t % G8) * 8;
  V cen[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    cen[q] = nc16_zero<T>();
    const int64_t row = row0 + (up0 + UP * q) % R;
    if (center != nullptr && uc < C1 && row < rows) cen[q] = *reinterpret_cast<const V*>(center + row * C1 + uc);
  }

  float best[CB][16];
  int slot[CB][16];
#pragma unroll
  for (int e = 0; e < CB; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) best[e][r] = 0.0f, slot[e][r] = 255;
  uint32_t seen = 0;

  for (int k0 = 0; k0 < K; k0 += kNmWin) {
    const int kt = min(kNmWin, K - k0);
    nm_stage<R, RT>(idx, lengths, row0, rows, L, K, M, k0, kt, s_src, s_mask);

    V v[Q];
    auto gather = [&](int g0) {  // slots g0 .. g0 + S - 1 of the window; past kt or masked: zeros
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int at = g0 * R + up0 + UP * q;
        const int s = (uc < C1 && at < kt * R) ? s_src[at] : -1;
        v[q] = nc16_zero<T>();
        if (s >= 0) v[q] = *reinterpret_cast<const V*>(x + (int64_t)s * C1 + uc);
      }
    };
    gather(0);
    for (int g0 = 0; g0 < kt; g0 += S) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {  // (stage 1 of the group before is behind its second barrier)
        if (uc >= Kp1) continue;  // (units in [C1, Kp1) write the zeros of the k padding)
        V hv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float a = (float)v[q][j] + (float)cen[q % NC][j];
          hv[j] = (T)(a > 0.0f ? a : 0.0f);
        }
        *reinterpret_cast<V*>(s_A1 + (up0 + UP * q) * ST1 + uc) = hv;
      }
      __syncthreads();  // A1 is written; stage 2 of the group before has read A2; the masks are written
      if (g0 + S < kt) gather(g0 + S);  // in flight during the MFMAs
      if (mma1) {
#pragma unroll
        for (int i = 0; i < NB1; ++i) {
          const int pt = pt1 + PT1 * i;
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = bv1;
          const T* a = s_A1 + (pt * 32 + c) * ST1 + 8 * h;
#pragma unroll
          for (int q = 0; q < KS1; ++q)
            if (16 * q < Kp1) acc = Nc16<T>::mfma(*reinterpret_cast<const V*>(a + 16 * q), b1[q], acc);
#pragma unroll
          for (int r = 0; r < 16; ++r)  // columns in [C2, Op1) get exact zeros: the k padding of stage 2
            s_A2[(pt * 32 + nm2_row(r, h)) * ST2 + oc1] = (T)(acc[r] > 0.0f ? acc[r] : 0.0f);
        }
      }
      __syncthreads();  // A2 is written; A1 is read
#pragma unroll
      for (int sl = 0; sl < S; ++sl) {
        const int kk = g0 + sl;
        if (kk >= kt) break;  // (uniform: the last group of a window may be partial)
        const uint32_t m = s_mask[kk * RT + rt];
        const T* a = s_A2 + (sl * R + rt * 32 + c) * ST2 + 8 * h;
#pragma unroll
        for (int e = 0; e < CB; ++e) {
          if (!mma2[e]) continue;
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = bv2[e];
#pragma unroll
          for (int q = 0; q < KS2; ++q)
            if (16 * q < Kp2) acc = Nc16<T>::mfma(*reinterpret_cast<const V*>(a + 16 * q), b2[e][q], acc);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rb = nm2_row(r, h);
            const bool take = ((m >> rb) & 1u) && (!((seen >> rb) & 1u) || acc[r] > best[e][r]);
            best[e][r] = take ? acc[r] : best[e][r];
            slot[e][r] = take ? k0 + kk : slot[e][r];
          }
        }
        seen |= m;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < CB; ++e) {
    if (!mma2[e] || oc2[e] >= C3) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + rt * 32 + nm2_row(r, h);
      if (row >= rows) continue;
      out[row * C3 + oc2[e]] = (T)((relu_out && !(best[e][r] > 0.0f)) ? 0.0f : best[e][r]);
      arg[row * C3 + oc2[e]] = (uint8_t)slot[e][r];
    }
  }
}

// the fragment of a 16-deep step whose k runs DOWN a tile: rows p0 .. p0 + 7 of column col
template <class T>
__device__ __forceinline__ typename Nc16<T>::V nm2_column(const T* tile, int stride, int p0, int col, bool on) {
  typename Nc16<T>::V f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = on ? tile[(p0 + j) * stride + col] : (T)0.0f;
  return f;
}

// The query-order backward.  BIG: C1, C2 <= 128 and C3 <= 256, else C1, C2 <= 64 and C3 <= 128 (smaller tiles).
// partial1[(workgroup KSP1 + g)(C1 + 1) C2 + ...]: rows i < C1 grad_weight, row C1 grad_bias (g = 0; zeros for g > 0);
// partial2 likewise with (C2 + 1) C3, whose row C2 nm2_bias2_kernel writes.  KSP = 4 / (waves over the M side).
template <class T, bool BIG>
__global__ __launch_bounds__(kNmBlock) void nm2_backward_kernel(
    const T* __restrict__ g, const T* __restrict__ out, const uint8_t* __restrict__ arg, const T* __restrict__ x,
    const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths, const T* __restrict__ center,
    const T* __restrict__ wT, const T* __restrict__ bias, const T* __restrict__ wN, const T* __restrict__ w2N,
    int64_t rows, int L, int K, int M, int C1, int C2, int C3, int relu_out, int nbi1, int nbi2,
    T* __restrict__ grad_center, T* __restrict__ e1ws, float* __restrict__ partial1, float* __restrict__ partial2) {
  typedef typename Nc16<T>::V V;
  constexpr int MAXC = BIG ? 128 : 64, MAXC3 = BIG ? 256 : 128, ST = MAXC + 8, ST3 = MAXC3 + 8;
  constexpr int J1 = MAXC / 32, J2 = MAXC3 / 32, P = 64;  // pairs of a tile: 32 rows x 2 slots
  static_assert((ST / 8) % 2 == 1 && (ST3 / 8) % 2 == 1, "odd strides in 16-byte units");
  __shared__ uint4 s_t1[P * ST / 8], s_t2[P * ST / 8], s_t3[P * ST / 8], s_t4[P * ST3 / 8], s_t5[P * ST / 8], s_t6[P * ST / 8];
  __shared__ int s_src[kNmWin * 32];
  __shared__ uint32_t s_mask[kNmWin];
  T *s_A1 = reinterpret_cast<T*>(s_t1), *s_A2 = reinterpret_cast<T*>(s_t2), *s_E2 = reinterpret_cast<T*>(s_t3);
  T *s_E3 = reinterpret_cast<T*>(s_t4), *s_E2L = reinterpret_cast<T*>(s_t5);  // E2L, A2L: what the roundings of E2 and A2 dropped
  T* s_A2L = reinterpret_cast<T*>(s_t6);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, h = lane >> 5, c = lane & 31;
  const int Kp1 = (C1 + 15) & ~15, Kp2 = (C2 + 15) & ~15, Kp3 = (C3 + 15) & ~15;
  const int Op1 = (C1 + 31) & ~31, Op2 = (C2 + 31) & ~31, Op3 = (C3 + 31) & ~31;
  const int G1 = Kp1 / 8, G3 = Op3 / 8;
  const int ksp1 = 4 / nbi1, ksp2 = 4 / nbi2;
  const int i1 = wave % nbi1, grp1 = wave / nbi1, i2 = wave % nbi2, grp2 = wave / nbi2;

  f32x16 gw[J1], gw2[J2];
  float gbacc[J1 / 2];
#pragma unroll
  for (int j = 0; j < J1; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) gw[j][r] = 0.0f;
#pragma unroll
  for (int j = 0; j < J2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) gw2[j][r] = 0.0f;
#pragma unroll
  for (int i = 0; i < J1 / 2; ++i) gbacc[i] = 0.0f;

  const int64_t tiles = (rows + 31) / 32;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 32;
    float gc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) gc[r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kNmWin) {
      const int kt = min(kNmWin, K - k0);
      nm_stage<32, 1>(idx, lengths, row0, rows, L, K, M, k0, kt, s_src, s_mask);
      for (int g0 = 0; g0 < kt; g0 += 2) {
        __syncthreads();  // the products of the group before have read the tiles; s_src is written
        for (int u = t; u < P * G1; u += kNmBlock) {  // A1 = h1, zeros in masked pairs and in the k padding
          const int p = u / G1, ch = (u - p * G1) * 8, kk = g0 + (p >> 5);
          const int s = (ch < C1 && kk < kt) ? s_src[kk * 32 + (p & 31)] : -1;
          V hv = nc16_zero<T>();
          if (s >= 0) {
            const V xv = *reinterpret_cast<const V*>(x + (int64_t)s * C1 + ch);
            V cv = nc16_zero<T>();
            if (center != nullptr) cv = *reinterpret_cast<const V*>(center + (row0 + (p & 31)) * C1 + ch);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float a = (float)xv[j] + (float)cv[j];
              hv[j] = (T)(a > 0.0f ? a : 0.0f);
            }
          }
          *reinterpret_cast<V*>(s_A1 + p * ST + ch) = hv;
        }
        for (int u = t; u < P * G3; u += kNmBlock) {  // E3 = gy where arg is the pair's slot
          const int p = u / G3, ch = (u - p * G3) * 8, kk = g0 + (p >> 5);
          const bool on = ch < C3 && kk < kt && s_src[kk * 32 + (p & 31)] >= 0;
          V ev = nc16_zero<T>();
          if (on) {
            const int64_t at = (row0 + (p & 31)) * C3 + ch;
            const V gv = *reinterpret_cast<const V*>(g + at);
            const uint32_t a0 = *reinterpret_cast<const uint32_t*>(arg + at);
            const uint32_t a1 = *reinterpret_cast<const uint32_t*>(arg + at + 4);
            V ov = gv;
            if (relu_out) ov = *reinterpret_cast<const V*>(out + at);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int ak = (int)(((j < 4 ? a0 : a1) >> (8 * (j & 3))) & 255u);
              const bool hit = ak == k0 + kk && (!relu_out || (float)ov[j] > 0.0f);
              ev[j] = hit ? gv[j] : (T)0.0f;
            }
          }
          *reinterpret_cast<V*>(s_E3 + p * ST3 + ch) = ev;
        }
        __syncthreads();
        {  // h2 and e2 of pair tile (wave & 1), column blocks (wave >> 1) + 2 i of C2
          const int pt = wave & 1;
#pragma unroll
          for (int i = 0; i < J1 / 2; ++i) {
            const int jb = (wave >> 1) + 2 * i, oc = jb * 32 + c;
            if (jb * 32 >= Op2) continue;  // (uniform)
            f32x16 a1, a2;
            const float bv = (oc < C2 && bias != nullptr) ? (float)bias[oc] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) a1[r] = bv, a2[r] = 0.0f;
            const T* pa = s_A1 + (pt * 32 + c) * ST + 8 * h;
            const T* pb = wT + (int64_t)oc * Kp1 + 8 * h;
            for (int q = 0; q < Kp1; q += 16)
              a1 = Nc16<T>::mfma(*reinterpret_cast<const V*>(pa + q), *reinterpret_cast<const V*>(pb + q), a1);
            const T* pe = s_E3 + (pt * 32 + c) * ST3 + 8 * h;
            const T* pw = w2N + (int64_t)oc * Kp3 + 8 * h;
            for (int q = 0; q < Kp3; q += 16)
              a2 = Nc16<T>::mfma(*reinterpret_cast<const V*>(pe + q), *reinterpret_cast<const V*>(pw + q), a2);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float h2f = a1[r] > 0.0f ? a1[r] : 0.0f;
              const T h2 = (T)h2f;
              const float e2f = (float)h2 > 0.0f ? a2[r] : 0.0f;
              const T e2 = (T)e2f;
              const int at = (pt * 32 + nm2_row(r, h)) * ST + oc;
              s_A2[at] = h2, s_E2[at] = e2, s_E2L[at] = (T)(e2f - (float)e2), s_A2L[at] = (T)(h2f - (float)h2);
              gbacc[i] = gbacc[i] + e2f;
            }
          }
        }
        __syncthreads();
        if (wave * 32 < Op1) {  // e1 of column block `wave` of C1, slots ascending
          const int oc = wave * 32 + c;
          for (int pt = 0; pt < 2 && g0 + pt < kt; ++pt) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            const T* pa = s_E2 + (pt * 32 + c) * ST + 8 * h;
            const T* pl = s_E2L + (pt * 32 + c) * ST + 8 * h;
            const T* pb = wN + (int64_t)oc * Kp2 + 8 * h;
            for (int q = 0; q < Kp2; q += 16) {  // e2 as the pair (E2, E2L): the chain to e1 sees it to 16 bits
              const V b = *reinterpret_cast<const V*>(pb + q);
              acc = Nc16<T>::mfma(*reinterpret_cast<const V*>(pl + q), b, acc);
              acc = Nc16<T>::mfma(*reinterpret_cast<const V*>(pa + q), b, acc);
            }
            if (oc < C1) {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int rr = nm2_row(r, h);
                const float e1 = (float)s_A1[(pt * 32 + rr) * ST + oc] > 0.0f ? acc[r] : 0.0f;
                gc[r] = gc[r] + e1;
                if (e1ws != nullptr && row0 + rr < rows)
                  e1ws[((row0 + rr) * K + k0 + g0 + pt) * C1 + oc] = (T)e1;
              }
            }
          }
        }
        if (i1 * 32 < Op1) {  // grad_weight block row i1: A1^T E2 over the pairs of steps grp1, grp1 + ksp1, ...
          for (int s = grp1; s < P / 16; s += ksp1) {
            const V a = nm2_column<T>(s_A1, ST, 16 * s + 8 * h, i1 * 32 + c, i1 * 32 + c < Kp1);
#pragma unroll
            for (int j = 0; j < J1; ++j)
              if (j * 32 < Op2) {
                gw[j] = Nc16<T>::mfma(a, nm2_column<T>(s_E2L, ST, 16 * s + 8 * h, j * 32 + c, true), gw[j]);
                gw[j] = Nc16<T>::mfma(a, nm2_column<T>(s_E2, ST, 16 * s + 8 * h, j * 32 + c, true), gw[j]);
              }
          }
        }
        if (i2 * 32 < Op2) {  // grad_weight2 block row i2: A2^T E3
          for (int s = grp2; s < P / 16; s += ksp2) {
            const V a = nm2_column<T>(s_A2, ST, 16 * s + 8 * h, i2 * 32 + c, true);
            const V al = nm2_column<T>(s_A2L, ST, 16 * s + 8 * h, i2 * 32 + c, true);
#pragma unroll
            for (int j = 0; j < J2; ++j)
              if (j * 32 < Op3) {
                const V b = nm2_column<T>(s_E3, ST3, 16 * s + 8 * h, j * 32 + c, true);
                gw2[j] = Nc16<T>::mfma(al, b, gw2[j]);
                gw2[j] = Nc16<T>::mfma(a, b, gw2[j]);
              }
          }
        }
      }
    }
    if (grad_center != nullptr && wave * 32 + c < C1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = row0 + nm2_row(r, h);
        if (row < rows) grad_center[row * C1 + wave * 32 + c] = (T)gc[r];
      }
    }
  }

  const int64_t n1 = (int64_t)(C1 + 1) * C2, n2 = (int64_t)(C2 + 1) * C3;
  if (i1 * 32 < Op1) {
    float* dst = partial1 + ((int64_t)blockIdx.x * ksp1 + grp1) * n1;
#pragma unroll
    for (int j = 0; j < J1; ++j) {
      const int n = j * 32 + c;
      if (n >= C2) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = i1 * 32 + nm2_row(r, h);
        if (m < C1) dst[(int64_t)m * C2 + n] = gw[j][r];
      }
    }
  }
  if (i2 * 32 < Op2) {
    float* dst = partial2 + ((int64_t)blockIdx.x * ksp2 + grp2) * n2;
#pragma unroll
    for (int j = 0; j < J2; ++j) {
      const int n = j * 32 + c;
      if (n >= C3) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = i2 * 32 + nm2_row(r, h);
        if (m < C2) dst[(int64_t)m * C3 + n] = gw2[j][r];
      }
    }
  }
  // grad_bias: the lanes' column sums of e2, added in the fixed order (pair tile, half)
  __syncthreads();
  float* s_red = reinterpret_cast<float*>(s_t4);  // [wave][half][MAXC]
#pragma unroll
  for (int i = 0; i < J1 / 2; ++i) s_red[(wave * 2 + h) * MAXC + ((wave >> 1) + 2 * i) * 32 + c] = gbacc[i];
  __syncthreads();
  if (t < C2) {
    const int w0 = 2 * ((t >> 5) & 1);
    float s = 0.0f;
    for (int q = 0; q < 4; ++q) s = s + s_red[((w0 + (q >> 1)) * 2 + (q & 1)) * MAXC + t];
    for (int gq = 0; gq < ksp1; ++gq)
      partial1[((int64_t)blockIdx.x * ksp1 + gq) * n1 + (int64_t)C1 * C2 + t] = gq == 0 ? s : 0.0f;
  }
}

// row C2 of partial2: the sums of gy over the rows chunk, chunk + chunks, ... (plane 0 of the chunk; zeros in the others)
template <class T>
__global__ __launch_bounds__(256) void nm2_bias2_kernel(const T* __restrict__ g, const T* __restrict__ out,
                                                        const uint8_t* __restrict__ arg, int64_t rows, int C2, int C3,
                                                        int relu_out, int ksp2, float* __restrict__ partial2) {
  const int cc = threadIdx.x;
  if (cc >= C3) return;
  float s8[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // eight rows in flight, added in a fixed tree
  for (int64_t row = blockIdx.x; row < rows; row += 8 * (int64_t)gridDim.x) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t at = (row + q * (int64_t)gridDim.x) * C3 + cc;
      if (row + q * (int64_t)gridDim.x >= rows) continue;
      const bool on = arg[at] != 255 && (!relu_out || (float)out[at] > 0.0f);
      s8[q] = s8[q] + (on ? (float)g[at] : 0.0f);
    }
  }
  const float s = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
  const int64_t n2 = (int64_t)(C2 + 1) * C3;
  for (int gq = 0; gq < ksp2; ++gq)
    partial2[((int64_t)blockIdx.x * ksp2 + gq) * n2 + (int64_t)C2 * C3 + cc] = gq == 0 ? s : 0.0f;
}

// grad_x[r, :] = the sum over the entries of target row r, in table order, of e1 as stored; 16 lanes per row
template <class T>
__global__ __launch_bounds__(kNmBlock) void nm2_grad_x_kernel(const T* __restrict__ e1ws, const unsigned* __restrict__ vals,
                                                              const int* __restrict__ seg_start,
                                                              const int* __restrict__ seg_end, int64_t targets, int C1,
                                                              T* __restrict__ grad_x) {
  typedef typename Nc16<T>::V V;
  const int ch = (threadIdx.x & 15) * 8;
  const int64_t r = (int64_t)blockIdx.x * (kNmBlock / 16) + (threadIdx.x >> 4);
  if (r >= targets || ch >= C1) return;
  float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const int t1 = seg_end[r];
  for (int t = seg_start[r]; t < t1; ++t) {
    const V e = *reinterpret_cast<const V*>(e1ws + (int64_t)vals[t] * C1 + ch);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] + (float)e[j];
  }
  V o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (T)acc[j];
  *reinterpret_cast<V*>(grad_x + r * C1 + ch) = o;
}

struct Nm2Ws {
  DetWs det;
  void *wT, *w2T;   // forward order: (ceil32(C2), ceil16(C1)) and (ceil32(C3), ceil16(C2)) of T
  void *wN, *w2N;   // as they lie: (ceil32(C1), ceil16(C2)) and (ceil32(C2), ceil16(C3))
  float *partial1, *partial2;
  void* e1;         // (N, L, K, C1) of T
};

inline int64_t nm2_chunks(int64_t rows) {
  const int64_t c = ceil_div(rows, 32);
  return c < 1 ? 1 : (c < kNm2MaxChunks ? c : kNm2MaxChunks);
}

static size_t nm2_carve(Nm2Ws* ws, void* base, bool backward, int64_t N, int64_t L, int64_t K, int64_t M, int64_t C1,
                        int64_t C2, int64_t C3) {
  Nm2Ws w = {};
  Carver c(base);
  if (backward) c.off = det_carve(base ? &w.det : nullptr, base, N, L, K, M);
  w.wT = c.take((size_t)2 * nm2_up(C2, 32) * nm2_up(C1, 16));
  if (!backward) w.w2T = c.take((size_t)2 * nm2_up(C3, 32) * nm2_up(C2, 16));
  if (backward) {
    const int64_t chunks = nm2_chunks(N * L);
    w.wN = c.take((size_t)2 * nm2_up(C1, 32) * nm2_up(C2, 16));
    w.w2N = c.take((size_t)2 * nm2_up(C2, 32) * nm2_up(C3, 16));
    w.partial1 = (float*)c.take(sizeof(float) * (size_t)(chunks * (4 / nm2_bucket(ceil_div(C1, 32))) * (C1 + 1) * C2));
    w.partial2 = (float*)c.take(sizeof(float) * (size_t)(chunks * (4 / nm2_bucket(ceil_div(C2, 32))) * (C2 + 1) * C3));
    w.e1 = c.take((size_t)2 * (size_t)(N * L * K * C1));
  }
  if (ws) *ws = w;
  return c.off;
}

static bool nm2_sizes_ok(int64_t N, int64_t L, int64_t M, int64_t K, int64_t C1, int64_t C2, int64_t C3) {
  return nm_index_ok(N, L, M, K) && C1 >= 8 && C1 <= kNm2MaxC && C1 % 8 == 0 && C2 >= 8 && C2 <= kNm2MaxC &&
         C2 % 8 == 0 && C3 >= 8 && C3 <= kNm2MaxC3 && C3 % 8 == 0;
}

constexpr Ints<2, 4, 8> kNm2Steps{};  // 16-deep steps: the smallest KS >= ceil(C / 16)

template <class T>
static void nm2_pack(const void* src, int64_t O, int64_t Kd, int64_t so, int64_t sk, void* dst, hipStream_t stream) {
  const int Op = nm2_up(O, 32), Kp = nm2_up(Kd, 16);
  hipLaunchKernelGGL(nm2_pack_kernel<T>, dim3((unsigned)ceil_div(Op * Kp, 256)), dim3(256), 0, stream, (const T*)src,
                     (int)O, (int)Kd, (int)so, (int)sk, Op, Kp, (T*)dst);
}

template <class T>
static int nm2_forward(const void* x, const int64_t* idx, const int64_t* lengths, const void* center,
                       const void* weight, const void* bias, const void* weight2, const void* bias2, int64_t N,
                       int64_t L, int64_t M, int64_t K, int64_t C1, int64_t C2, int64_t C3, int relu_out, void* out,
                       uint8_t* arg, const Nm2Ws& ws, hipStream_t stream) {
  const int64_t rows = N * L;
  nm2_pack<T>(weight, C2, C1, 1, C2, ws.wT, stream);    // wT[c2][c1]
  nm2_pack<T>(weight2, C3, C2, 1, C3, ws.w2T, stream);  // w2T[c3][c2]
  auto launch = [&](auto NBW, auto CBK) {
    with_bucket(kNm2Steps, (int)ceil_div(C1, 16), [&](auto KS1) {
      with_bucket(kNm2Steps, (int)ceil_div(C2, 16), [&](auto KS2) {
        constexpr int nbw = decltype(NBW)::value, cb = decltype(CBK)::value;
        hipLaunchKernelGGL((nm2_forward_kernel<T, nbw, cb, decltype(KS1)::value, decltype(KS2)::value>),
                           dim3((unsigned)ceil_div(rows, 128 / nbw)), dim3(kNmBlock), 0, stream, (const T*)x, idx, lengths,
                           (const T*)center, (const T*)ws.wT, (const T*)bias, (const T*)ws.w2T, (const T*)bias2, rows,
                           (int)L, (int)K, (int)M, (int)C1, (int)C2, (int)C3, relu_out, (T*)out, arg);
      });
    });
  };
  if (C3 <= 64) launch(IntC<2>{}, IntC<1>{});
  else if (C3 <= 128) launch(IntC<4>{}, IntC<1>{});
  else launch(IntC<4>{}, IntC<2>{});
  return check_launch("neighbor_mlp2_max16");
}

template <class T>
static int nm2_backward(const void* grad_out, const void* x, const int64_t* idx, const int64_t* lengths,
                        const void* center, const void* weight, const void* bias, const void* weight2, const void* out,
                        const uint8_t* arg, int64_t N, int64_t L, int64_t M, int64_t K, int64_t C1, int64_t C2,
                        int64_t C3, int relu_out, void* grad_x, void* grad_center, void* grad_weight, void* grad_bias,
                        void* grad_weight2, void* grad_bias2, const Nm2Ws& ws, hipStream_t stream) {
  const int64_t rows = N * L, targets = N * M, chunks = nm2_chunks(rows);
  const bool need_x = grad_x != nullptr && targets > 0;
  const int nbi1 = nm2_bucket(ceil_div(C1, 32)), nbi2 = nm2_bucket(ceil_div(C2, 32));
  nm2_pack<T>(weight, C2, C1, 1, C2, ws.wT, stream);    // wT[c2][c1]
  nm2_pack<T>(weight, C1, C2, C2, 1, ws.wN, stream);    // wN[c1][c2]
  nm2_pack<T>(weight2, C2, C3, C3, 1, ws.w2N, stream);  // w2N[c2][c3]
  with_exact<0>(Ints<1>{}, (C1 > 64 || C2 > 64 || C3 > 128) ? 1 : 0, [&](auto BIG) {
    hipLaunchKernelGGL((nm2_backward_kernel<T, decltype(BIG)::value != 0>), dim3((unsigned)chunks), dim3(kNmBlock), 0,
                       stream, (const T*)grad_out, (const T*)out, arg, (const T*)x, idx, lengths, (const T*)center,
                       (const T*)ws.wT, (const T*)bias, (const T*)ws.wN, (const T*)ws.w2N, rows, (int)L, (int)K, (int)M,
                       (int)C1, (int)C2, (int)C3, relu_out, nbi1, nbi2, (T*)grad_center, need_x ? (T*)ws.e1 : (T*)nullptr,
                       ws.partial1, ws.partial2);
  });
  if (grad_weight != nullptr || grad_bias != nullptr)
    hipLaunchKernelGGL(nm_sum_partials_kernel<T>, dim3((unsigned)ceil_div((C1 + 1) * C2, 256)), dim3(256), 0, stream,
                       ws.partial1, (int)(chunks * (4 / nbi1)), (int)C1, (int)C2, (T*)grad_weight, (T*)grad_bias);
  if (grad_weight2 != nullptr || grad_bias2 != nullptr) {
    hipLaunchKernelGGL(nm2_bias2_kernel<T>, dim3((unsigned)chunks), dim3(256), 0, stream, (const T*)grad_out,
                       (const T*)out, arg, rows, (int)C2, (int)C3, relu_out, 4 / nbi2, ws.partial2);
    hipLaunchKernelGGL(nm_sum_partials_kernel<T>, dim3((unsigned)ceil_div((C2 + 1) * C3, 256)), dim3(256), 0, stream,
                       ws.partial2, (int)(chunks * (4 / nbi2)), (int)C2, (int)C3, (T*)grad_weight2, (T*)grad_bias2);
  }
  if (need_x) {
    const int rc = det_invert(ws.det, idx, nullptr, lengths, N, L, K, M, stream);
    if (rc != POINTOPS_OK) return rc;
    hipLaunchKernelGGL(nm2_grad_x_kernel<T>, dim3((unsigned)ceil_div(targets, kNmBlock / 16)), dim3(kNmBlock), 0, stream,
                       (const T*)ws.e1, ws.det.vals_out, ws.det.seg_start, ws.det.seg_end, targets, (int)C1, (T*)grad_x);
  }
  return check_launch("neighbor_mlp2_max16_backward");
}

}  // namespace pointops

using namespace pointops;

#define NM2_BAD_SIZES                                                                                                   \
  ": bad sizes (dtype 0 or 1, C1 and C2 multiples of 8 in [8, 128], C3 a multiple of 8 in [8, 256], 1 <= K <= 255; N L " \
  "K must be below 2^31 and N M below 2^31 - 1)"

static bool nm2_dtype_ok(int dtype) { return dtype == POINTOPS_DTYPE_BF16 || dtype == POINTOPS_DTYPE_F16; }

extern "C" size_t pointops_neighbor_mlp2_max16_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M, int64_t C1,
                                                               int64_t C2, int64_t C3) {
  if (!nm2_sizes_ok(N, L, M, K, C1, C2, C3)) return 0;
  return nm2_carve(nullptr, nullptr, false, N, L, K, M, C1, C2, C3);
}

extern "C" size_t pointops_neighbor_mlp2_max16_backward_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M,
                                                                        int64_t C1, int64_t C2, int64_t C3) {
  if (!nm2_sizes_ok(N, L, M, K, C1, C2, C3)) return 0;
  return nm2_carve(nullptr, nullptr, true, N, L, K, M, C1, C2, C3);
}

extern "C" int pointops_neighbor_mlp2_max16(const void* x, const int64_t* idx, const int64_t* lengths,
                                            const void* center, const void* weight, const void* bias,
                                            const void* weight2, const void* bias2, int dtype, int64_t N, int64_t L,
                                            int64_t M, int64_t K, int64_t C1, int64_t C2, int64_t C3, int relu_out,
                                            void* out, uint8_t* arg, void* workspace, size_t workspace_bytes,
                                            void* stream_) {
  POINTOPS_REQUIRE(nm2_dtype_ok(dtype) && nm2_sizes_ok(N, L, M, K, C1, C2, C3), "neighbor_mlp2_max16" NM2_BAD_SIZES);
  const int64_t rows = N * L;
  POINTOPS_REQUIRE(weight != nullptr && weight2 != nullptr &&
                       (rows == 0 || (idx != nullptr && out != nullptr && arg != nullptr)) &&
                       (x != nullptr || N * M == 0 || rows == 0),
                   "neighbor_mlp2_max16: null pointer");
  POINTOPS_REQUIRE(nm_aligned(x, center, nullptr, nullptr), "neighbor_mlp2_max16: x and center must be 16-byte aligned");
  Nm2Ws ws;
  POINTOPS_REQUIRE_WORKSPACE(
      workspace_fits(workspace, workspace_bytes, nm2_carve(&ws, workspace, false, N, L, K, M, C1, C2, C3)),
      "neighbor_mlp2_max16: workspace too small");
  if (rows == 0) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  return dtype == POINTOPS_DTYPE_BF16
             ? nm2_forward<__bf16>(x, idx, lengths, center, weight, bias, weight2, bias2, N, L, M, K, C1, C2, C3,
                                   relu_out, out, arg, ws, stream)
             : nm2_forward<_Float16>(x, idx, lengths, center, weight, bias, weight2, bias2, N, L, M, K, C1, C2, C3,
                                     relu_out, out, arg, ws, stream);
}

extern "C" int pointops_neighbor_mlp2_max16_backward(
    const void* grad_out, const void* x, const int64_t* idx, const int64_t* lengths, const void* center,
    const void* weight, const void* bias, const void* weight2, const void* out, const uint8_t* arg, int dtype, int64_t N,
    int64_t L, int64_t M, int64_t K, int64_t C1, int64_t C2, int64_t C3, int relu_out, void* grad_x, void* grad_center,
    void* grad_weight, void* grad_bias, void* grad_weight2, void* grad_bias2, void* workspace, size_t workspace_bytes,
    void* stream_) {
  POINTOPS_REQUIRE(nm2_dtype_ok(dtype) && nm2_sizes_ok(N, L, M, K, C1, C2, C3),
                   "neighbor_mlp2_max16_backward" NM2_BAD_SIZES);
  POINTOPS_REQUIRE(grad_center == nullptr || center != nullptr, "neighbor_mlp2_max16_backward: grad_center needs center");
  const int64_t rows = N * L, targets = N * M;
  POINTOPS_REQUIRE(weight != nullptr && weight2 != nullptr &&
                       (rows == 0 || (grad_out != nullptr && idx != nullptr && out != nullptr && arg != nullptr)) &&
                       (x != nullptr || targets == 0 || rows == 0),
                   "neighbor_mlp2_max16_backward: null pointer");
  POINTOPS_REQUIRE(nm_aligned(grad_out, x, center, out) && nm_aligned(grad_x, nullptr, nullptr, nullptr) &&
                       (uintptr_t)arg % 4 == 0,
                   "neighbor_mlp2_max16_backward: grad_out, x, center, out and grad_x must be 16-byte aligned, arg 4-byte");
  Nm2Ws ws;
  POINTOPS_REQUIRE_WORKSPACE(
      workspace_fits(workspace, workspace_bytes, nm2_carve(&ws, workspace, true, N, L, K, M, C1, C2, C3)),
      "neighbor_mlp2_max16_backward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  return dtype == POINTOPS_DTYPE_BF16
             ? nm2_backward<__bf16>(grad_out, x, idx, lengths, center, weight, bias, weight2, out, arg, N, L, M, K, C1,
                                    C2, C3, relu_out, grad_x, grad_center, grad_weight, grad_bias, grad_weight2,
                                    grad_bias2, ws, stream)
             : nm2_backward<_Float16>(grad_out, x, idx, lengths, center, weight, bias, weight2, out, arg, N, L, M, K, C1,
                                      C2, C3, relu_out, grad_x, grad_center, grad_weight, grad_bias, grad_weight2,
                                      grad_bias2, ws, stream);
}

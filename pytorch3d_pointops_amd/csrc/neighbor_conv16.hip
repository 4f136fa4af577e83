// neighbor_conv16.hip -- NEIGHBOUR CONVOLUTION on bfloat16 / float16 features (gfx950), on the 16-deep matrix
// instructions v_mfma_f32_32x32x16_bf16 / _f16 with fp32 accumulation.  The definition is the "16-bit features" part of
// the NEIGHBOUR CONVOLUTION block of include/pointops_amd.h; the row lists and their staging are neighbor_conv.h's, shared
// with the float32 kernels of neighbor_conv.hip.  T is __bf16 or _Float16 throughout.
//
//   pack      weight[p] is rewritten once per call into B-fragment order wp[p][k / 8][o][8], k zero-padded to a multiple
//             of 16 (Kp) and o to a multiple of 32 (Op): a lane's eight k-values of its column are one 16-byte load, a
//             half-wave reads 512 contiguous bytes, and the matrix stage has no tail predicates.  The planes follow each
//             other, so the pack is ONE (P Kp / 8, Op, 8) array and a chunk of planes is a linear range of 16-deep steps.
//             With swapped strides the same kernel writes the transposed pack (k = Cout, o = Cin) of grad_x and grad_coeff.
//   gather    a group of G = pow2 >= C / 8 lanes per row (at least 4), 16 bytes = 8 channels per lane and entry,
//             kNcUnroll row loads in flight before the first fmaf, fp32 acc[rows per lane][PC][8] with
//             PC = 8, 4, 2 for G <= 8, 16, 32: 64 registers, PC Kp <= 512.  Entries are staged by nc_stage.
//   A tile    ALL planes of a chunk are rounded to T (once, to nearest even) and written, 16 bytes per lane, to one LDS
//             tile [rows][PC Kp + 8]: one barrier pair per CHUNK.  The row stride is an ODD number of 16-byte units
//             (PC Kp is a multiple of 16 elements = 2 units, + 1 unit of pad): LDS has 64 banks of 4 bytes = 16 units,
//             so the 16-byte reads of 16 consecutive rows at the same k start in 16 different units and cover every bank
//             once, where an even stride would fold them onto 8 units or fewer (the argument of feature_match.hip's odd
//             float stride, in units of the access width).
//   matrix    a step is one 16-byte LDS read (A), one 16-byte global read of the pack (B) and one MFMA; the B loads of
//             four steps are issued ahead of their MFMAs.  Lane (c = lane & 31, h = lane >> 5) holds, for BOTH operands,
//             the k-values 16 s + 8 h + [0, 8) of step s: the instruction multiplies A and B element by element over
//             (h, j) and sums, so the product does not depend on which k the hardware believes a lane holds -- only on
//             A and B agreeing, which one expression (8 h + j) guarantees.  ONE accumulator per output block is carried
//             across all steps of all chunks and written once, rounded to T.  The order inside a step is the
//             hardware's: two calls give the same bytes.
//   waves     Co <= 64: the workgroup owns 64 rows, gathered as two 32-row halves into the tile, and the four waves
//             cover (row half x column block); Co <= 128: 32 rows, one column block per wave; Co > 128: two per wave.
//   grad_w    workgroups (row chunk, p, 64 channels of Cin): A_p is rebuilt in T by the same gather (G = 8, PC = 1) and
//             written TRANSPOSED, g's tile beside it, both [channel][32 rows + 8] (5 units: odd); A_p^T g is two 16-deep
//             steps per tile, up to four blocks per wave; fp32 partials, summed in ascending chunk order, rounded once.
//   grad_c    per row tile and p, T_p = g_tile weight[p]^T from the transposed pack, kept in fp32 in LDS; the lane groups
//             dot it with the gathered rows: the lane's eight products ascending, then wave_sum<G>; rounded once.
// No float atomics; every output element is written once.  Fixed launch sequences, nothing is read back.
#include "mfma16.h"
#include "neighbor_conv.h"

namespace pointops {

constexpr int kNc16MaxC = 256;
constexpr int kNc16Pad = 8;         // elements: one 16-byte unit
constexpr int kNc16Ahead = 4;       // B loads in flight
constexpr int kNc16GwChannels = 64; // channels of Cin per grad_w workgroup: 32 rows x 8 lanes x 8 channels
constexpr int kNc16GwStride = kNcRows + kNc16Pad;
constexpr size_t kNc16LdsMax = (size_t)2 * kNcRows * (512 + kNc16Pad) * 2;  // the 64-row tile at PC Kp = 512

constexpr int nc16_pc(int G) { return G >= 32 ? 2 : (G >= 16 ? 4 : 8); }
constexpr int nc16_rpl(int G) { return G >= 8 ? G / 8 : 1; }  // rows of a 32-row tile a lane works on
static inline int nc16_up(int64_t v, int to) { return (int)((v + to - 1) / to * to); }

// wp[((p Kp / 8 + kb) Op + o) 8 + j] = w(p, k = 8 kb + j, o) = weight[p Ck Co + k wk + o wo], 0 past Ck or Co
template <class T>
__global__ __launch_bounds__(256) void nc16_pack_kernel(const T* __restrict__ weight, int P, int Ck, int Co, int wk,
                                                        int wo, int Kp, int Op, T* __restrict__ wp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, kbs = Kp / 8;
  if (i >= (int64_t)P * kbs * Op) return;
  const int o = (int)(i % Op), kb = (int)(i / Op % kbs), p = (int)(i / Op / kbs);
  typename Nc16<T>::V v = nc16_zero<T>();
  if (o < Co) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * kb + j;
      if (k < Ck) v[j] = weight[(int64_t)p * Ck * Co + (int64_t)k * wk + (int64_t)o * wo];
    }
  }
  *reinterpret_cast<typename Nc16<T>::V*>(wp + i * 8) = v;
}

// acc[i][p][:] = the lane's eight channels of A[row grp + i GR][p0 + p] over the row's list, in list order from +0.0f;
// rows of `src` are ldc apart and C wide.  Call from workgroup-uniform control flow.
template <class T, int G, int PC>
__device__ __forceinline__ void nc16_gather(float (&acc)[nc16_rpl(G)][PC][8], const NcList& ls,
                                            const T* __restrict__ src, int ldc, const T* __restrict__ coeff,
                                            int64_t row0, int64_t rows, int C, int P, int p0, int* s_src, int* s_ent,
                                            int* s_cnt) {
  typedef typename Nc16<T>::V V;
  constexpr int GR = kNcBlock / G, RPL = nc16_rpl(G), U = kNcUnroll;
  const int grp = threadIdx.x / G, ch = (threadIdx.x % G) * 8;
  __syncthreads();
  if (threadIdx.x < kNcRows) s_cnt[threadIdx.x] = nc_count(ls, row0 + threadIdx.x, rows);
  __syncthreads();
  int longest = 0;
  for (int r = 0; r < kNcRows; ++r) longest = max(longest, s_cnt[r]);
#pragma unroll
  for (int i = 0; i < RPL; ++i)
#pragma unroll
    for (int p = 0; p < PC; ++p)
#pragma unroll
      for (int x = 0; x < 8; ++x) acc[i][p][x] = 0.0f;

  for (int t0 = 0; t0 < longest; t0 += kNcWin) {
    nc_stage(ls, row0, rows, t0, s_src, s_ent);
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
      const int r = grp + i * GR;
      if (r >= kNcRows) continue;
      const int nent = min(kNcWin, s_cnt[r] - t0);
      for (int jb = 0; jb < nent; jb += U) {
        int s[U], e[U];
        V v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool in = jb + u < nent;
          s[u] = in ? s_src[r * kNcWin + jb + u] : -1;
          e[u] = in ? s_ent[r * kNcWin + jb + u] : 0;
          if (coeff == nullptr) {  // one-hot: the entry belongs to one p
            const int pe = e[u] % ls.K;
            if (pe < p0 || pe >= p0 + PC) s[u] = -1;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // the loads, all issued before the first multiply
          v[u] = nc16_zero<T>();
          if (s[u] >= 0 && ch < C) v[u] = *reinterpret_cast<const V*>(src + (int64_t)s[u] * ldc + ch);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // list order
          if (s[u] < 0) continue;
          const int pe = e[u] % ls.K;
#pragma unroll
          for (int p = 0; p < PC; ++p) {
            if (p0 + p >= P) continue;  // (workgroup-uniform)
            if (coeff != nullptr) {
              const float cf = (float)coeff[(int64_t)e[u] * P + p0 + p];
#pragma unroll
              for (int x = 0; x < 8; ++x) acc[i][p][x] = __builtin_fmaf(cf, (float)v[u][x], acc[i][p][x]);
            } else if (pe == p0 + p) {
#pragma unroll
              for (int x = 0; x < 8; ++x) acc[i][p][x] = acc[i][p][x] + (float)v[u][x];
            }
          }
        }
      }
    }
  }
}

// out[row,:] (Co wide) = the MFMA sum over p, c of A[row][p][c] w(p, c, o), w in the pack `wp` (Kp x Op per plane);
// A over the row list `ls` of rows Ck wide in `src`.  A workgroup owns 32 NH rows; with NB == 2, NH is 1.
template <class T, int G, int NB>
__global__ __launch_bounds__(kNcBlock) void nc16_conv_kernel(NcList ls, const T* __restrict__ src,
                                                             const T* __restrict__ coeff, const T* __restrict__ wp,
                                                             int64_t rows, int Ck, int Co, int P, int NH,
                                                             T* __restrict__ out) {
  typedef typename Nc16<T>::V V;
  constexpr int PC = nc16_pc(G), GR = kNcBlock / G, RPL = nc16_rpl(G), AH = kNc16Ahead;
  extern __shared__ uint4 s_nc16[];  // the A tile [32 NH][PC Kp + 8] of T (16-byte aligned)
  T* s_A = reinterpret_cast<T*>(s_nc16);
  __shared__ int s_src[kNcRows * kNcWin], s_ent[kNcRows * kNcWin], s_cnt[kNcRows];
  const int Kp = (Ck + 15) & ~15, Op = (Co + 31) & ~31, stride = PC * Kp + kNc16Pad;
  const int64_t row0 = (int64_t)blockIdx.x * kNcRows * NH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int grp = threadIdx.x / G, ch = (threadIdx.x % G) * 8;
  const int rb = wave % NH;  // the wave's row half; its column blocks are (wave + 4 q) / NH
  int cb[NB];
  bool act[NB];  // (wave-uniform)
  f32x16 o16[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    cb[q] = (wave + 4 * q) / NH;
    act[q] = cb[q] * 32 < Op;
#pragma unroll
    for (int r = 0; r < 16; ++r) o16[q][r] = 0.0f;
  }
  const int64_t bstep = (int64_t)2 * Op * 8;  // elements of the pack per 16-deep step

  for (int p0 = 0; p0 < P; p0 += PC) {
    const int pcnt = min(PC, P - p0);
    for (int half = 0; half < NH; ++half) {
      float acc[RPL][PC][8];
      // (the first barrier of the gather is also the one that ends the previous chunk's matrix stage)
      nc16_gather<T, G, PC>(acc, ls, src, Ck, coeff, row0 + half * kNcRows, rows, Ck, P, p0, s_src, s_ent, s_cnt);
#pragma unroll
      for (int i = 0; i < RPL; ++i) {
        const int r = grp + i * GR;
        if (r < kNcRows && ch < Kp) {  // (lanes in [Ck, Kp) hold the zeros of the k padding)
#pragma unroll
          for (int p = 0; p < PC; ++p) {
            if (p >= pcnt) continue;
            V t;
#pragma unroll
            for (int x = 0; x < 8; ++x) t[x] = (T)acc[i][p][x];
            *reinterpret_cast<V*>(s_A + (half * kNcRows + r) * stride + p * Kp + ch) = t;
          }
        }
      }
    }
    __syncthreads();
    const int nsteps = pcnt * Kp / 16;
    const T* a = s_A + (rb * kNcRows + c) * stride + 8 * h;  // A[i = c][k = 16 s + 8 h + j]
    const T* __restrict__ b[NB];                            // B[k = 16 s + 8 h + j][o = 32 cb + c]
#pragma unroll
    for (int q = 0; q < NB; ++q)
      b[q] = wp + ((int64_t)(p0 * Kp / 8 + h) * Op + (act[q] ? cb[q] : 0) * 32 + c) * 8;
    int s = 0;
    for (; s + AH <= nsteps; s += AH) {
      V bv[NB][AH];
#pragma unroll
      for (int u = 0; u < AH; ++u)
#pragma unroll
        for (int q = 0; q < NB; ++q)
          if (act[q]) bv[q][u] = *reinterpret_cast<const V*>(b[q] + (s + u) * bstep);
#pragma unroll
      for (int u = 0; u < AH; ++u) {
        const V av = *reinterpret_cast<const V*>(a + 16 * (s + u));
#pragma unroll
        for (int q = 0; q < NB; ++q)
          if (act[q]) o16[q] = Nc16<T>::mfma(av, bv[q][u], o16[q]);
      }
    }
    for (; s < nsteps; ++s) {
      const V av = *reinterpret_cast<const V*>(a + 16 * s);
#pragma unroll
      for (int q = 0; q < NB; ++q)
        if (act[q]) o16[q] = Nc16<T>::mfma(av, *reinterpret_cast<const V*>(b[q] + s * bstep), o16[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int oc = cb[q] * 32 + c;
    if (!act[q] || oc >= Co) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + rb * kNcRows + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (row < rows) out[row * Co + oc] = (T)o16[q][r];
    }
  }
}

// partial[(chunk P + p) Cin Cout + ci Cout + o] = sum over the rows of the chunk's tiles, ascending, of
// A[row][p][ci] g[row][o] for the channels ci in [64 z, 64 z + 64)
template <class T>
__global__ __launch_bounds__(kNcBlock) void nc16_grad_w_kernel(NcList ls, const T* __restrict__ x,
                                                               const T* __restrict__ coeff, const T* __restrict__ g,
                                                               int64_t rows, int Cin, int Cout, int P,
                                                               float* __restrict__ partial) {
  typedef typename Nc16<T>::V V;
  constexpr int G = 8, S = kNc16GwStride, CZ = kNc16GwChannels;
  __shared__ __attribute__((aligned(16))) T s_At[CZ * S], s_Gt[kNc16MaxC * S];  // [channel][row]: the rows are k
  __shared__ int s_src[kNcRows * kNcWin], s_ent[kNcRows * kNcWin], s_cnt[kNcRows];
  const int p = blockIdx.y, c0 = blockIdx.z * CZ, Cz = min(CZ, Cin - c0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int grp = threadIdx.x / G, ch = (threadIdx.x % G) * 8;
  const int nco = (Cout + 31) / 32;
  for (int i = threadIdx.x; i < CZ * S; i += kNcBlock) s_At[i] = (T)0.0f;  // (channels past Cz and Cout stay 0)
  for (int i = threadIdx.x; i < kNc16MaxC * S; i += kNcBlock) s_Gt[i] = (T)0.0f;
  f32x16 o16[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) o16[q][r] = 0.0f;

  const int64_t ntiles = (rows + kNcRows - 1) / kNcRows;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kNcRows;
    float acc[1][1][8];
    // (the gather's barriers end the zero fill and the previous tile's matrix stage)
    nc16_gather<T, G, 1>(acc, ls, x + c0, Cin, coeff, row0, rows, Cz, P, p, s_src, s_ent, s_cnt);
    if (ch < Cz) {
#pragma unroll
      for (int xx = 0; xx < 8; ++xx) s_At[(ch + xx) * S + grp] = (T)acc[0][0][xx];
    }
    for (int i = threadIdx.x; i < kNcRows * Cout; i += kNcBlock) {
      const int r = i / Cout, o = i - r * Cout;
      s_Gt[o * S + r] = row0 + r < rows ? g[(row0 + r) * Cout + o] : (T)0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int blk = wave + 4 * q, cib = blk & 1, cob = blk >> 1;
      if (cob < nco && cib * 32 < Cz) {  // (wave-uniform)
#pragma unroll
        for (int s = 0; s < kNcRows / 16; ++s) {
          const V av = *reinterpret_cast<const V*>(s_At + (cib * 32 + c) * S + 16 * s + 8 * h);
          const V bv = *reinterpret_cast<const V*>(s_Gt + (cob * 32 + c) * S + 16 * s + 8 * h);
          o16[q] = Nc16<T>::mfma(av, bv, o16[q]);
        }
      }
    }
  }
  float* __restrict__ dst = partial + ((int64_t)blockIdx.x * P + p) * Cin * Cout;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int blk = wave + 4 * q, cib = blk & 1, cob = blk >> 1, o = cob * 32 + c;
    if (cob >= nco || cib * 32 >= Cz || o >= Cout) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = cib * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ci < Cz) dst[(int64_t)(c0 + ci) * Cout + o] = o16[q][r];
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void nc16_sum_partials_kernel(const float* __restrict__ partial, int chunks,
                                                                int64_t count, T* __restrict__ grad_w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float s = 0.0f;
  for (int ch = 0; ch < chunks; ++ch) s = s + partial[(int64_t)ch * count + i];
  grad_w[i] = (T)s;
}

// grad_coeff[e,p] = x[n,idx[e],:] . (g[n,l,:] weight[p]^T) for a valid slot, else 0; wpt: the transposed pack
template <class T, int G>
__global__ __launch_bounds__(kNcBlock) void nc16_grad_c_kernel(NcList ls, const T* __restrict__ x,
                                                               const T* __restrict__ g, const T* __restrict__ wpt,
                                                               int64_t rows, int Cin, int Cout, int P,
                                                               T* __restrict__ grad_c) {
  typedef typename Nc16<T>::V V;
  constexpr int GR = kNcBlock / G, RPL = nc16_rpl(G), U = kNcUnroll;
  __shared__ __attribute__((aligned(16))) T s_G[kNcRows * (kNc16MaxC + kNc16Pad)];
  __shared__ float s_T[kNcRows * (kNc16MaxC + 1)];
  __shared__ int s_src[kNcRows * kNcWin], s_ent[kNcRows * kNcWin];
  const int64_t row0 = (int64_t)blockIdx.x * kNcRows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int grp = threadIdx.x / G, j = threadIdx.x % G, ch = j * 8;
  const int Kp = (Cout + 15) & ~15, Op = (Cin + 31) & ~31, gs = Kp + kNc16Pad, ts = Cin + 1;
  const int K = ls.K, nwin = (K + kNcWin - 1) / kNcWin;
  for (int i = threadIdx.x; i < kNcRows * Kp; i += kNcBlock) {
    const int r = i / Kp, o = i - r * Kp;
    s_G[r * gs + o] = row0 + r < rows && o < Cout ? g[(row0 + r) * Cout + o] : (T)0.0f;
  }
  for (int p = 0; p < P; ++p) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int cb = wave + 4 * q, ci = cb * 32 + c;
      if (cb * 32 >= Op) continue;  // (wave-uniform)
      f32x16 t16;
#pragma unroll
      for (int r = 0; r < 16; ++r) t16[r] = 0.0f;
      const T* a = s_G + c * gs + 8 * h;                                               // A[i = c][k = 16 s + 8 h + j]
      const T* __restrict__ b = wpt + ((int64_t)(p * Kp / 8 + h) * Op + ci) * 8;  // B[k][o = ci] = w[p][ci][k]
      for (int s = 0; s < Kp / 16; ++s)
        t16 = Nc16<T>::mfma(*reinterpret_cast<const V*>(a + 16 * s),
                            *reinterpret_cast<const V*>(b + (int64_t)s * 2 * Op * 8), t16);
      if (ci < Cin) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_T[((r & 3) + 8 * (r >> 2) + 4 * h) * ts + ci] = t16[r];
      }
    }
    __syncthreads();
    for (int w = 0; w < nwin; ++w) {
      const int t0 = w * kNcWin, nent = min(kNcWin, K - t0);  // (every row of the forward list has K entries)
      if (nwin > 1 || p == 0) nc_stage(ls, row0, rows, t0, s_src, s_ent);
#pragma unroll
      for (int i = 0; i < RPL; ++i) {
        const int r = grp + i * GR;
        if (r >= kNcRows) continue;  // (whole groups, and with G < 8 whole xor ranges of wave_sum)
        float tv[8];
#pragma unroll
        for (int xx = 0; xx < 8; ++xx) tv[xx] = ch < Cin ? s_T[r * ts + ch + xx] : 0.0f;
        for (int jb = 0; jb < nent; jb += U) {
          int s[U], e[U];
          V v[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const bool in = jb + u < nent;
            s[u] = in ? s_src[r * kNcWin + jb + u] : -1;
            e[u] = in ? s_ent[r * kNcWin + jb + u] : 0;
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            v[u] = nc16_zero<T>();
            if (s[u] >= 0 && ch < Cin) v[u] = *reinterpret_cast<const V*>(x + (int64_t)s[u] * Cin + ch);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (jb + u >= nent) continue;  // (workgroup-uniform)
            float d = tv[0] * (float)v[u][0];
#pragma unroll
            for (int xx = 1; xx < 8; ++xx) d = d + tv[xx] * (float)v[u][xx];
            d = wave_sum<G>(d);
            if (j == 0 && row0 + r < rows) grad_c[(int64_t)e[u] * P + p] = s[u] >= 0 ? (T)d : (T)0.0f;
          }
        }
      }
    }
  }
}

struct Nc16Ws {
  DetWs det;
  float* partial;  // (chunks P Cin Cout) of nc16_grad_w_kernel
  void* pack;      // forward: (P, Kp(Cin) / 8, Op(Cout), 8); backward: the transposed one, (P, Kp(Cout) / 8, Op(Cin), 8)
};

static size_t nc16_pack_bytes(int64_t P, int64_t Ck, int64_t Co) { return (size_t)(P * nc16_up(Ck, 16) * nc16_up(Co, 32) * 2); }

static size_t nc16_carve(Nc16Ws* ws, void* base, bool backward, int64_t N, int64_t L, int64_t K, int64_t M, int64_t P,
                         int64_t Cin, int64_t Cout) {
  Nc16Ws w;
  Carver c(base);
  w.det.keys_in = nullptr;
  w.partial = nullptr;
  if (backward) {
    c.off = det_carve(base ? &w.det : nullptr, base, N, L, K, M);
    const int64_t chunks = nc_chunks(N * L, P);
    w.partial = (float*)c.take(sizeof(float) * (size_t)((chunks > 0 ? chunks : 1) * P * Cin * Cout));
  }
  w.pack = c.take(backward ? nc16_pack_bytes(P, Cout, Cin) : nc16_pack_bytes(P, Cin, Cout));
  if (ws) *ws = w;
  return c.off;
}

static bool nc16_sizes_ok(int64_t N, int64_t L, int64_t M, int64_t K, int64_t P, int64_t Cin, int64_t Cout) {
  return N >= 0 && M >= 0 && L >= 0 && K >= 1 && K <= kNcMaxK && P >= 1 && P <= kNcMaxP && Cin >= 8 &&
         Cin <= kNc16MaxC && Cin % 8 == 0 && Cout >= 8 && Cout <= kNc16MaxC && Cout % 8 == 0 && N < (1LL << 31) &&
         M < (1LL << 31) && L < (1LL << 31) && N * L < (1LL << 31) && N * L * K < (1LL << 31) &&
         N * M < (1LL << 31) - 1;
}

static bool nc16_aligned(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) % 16) == 0; }

constexpr Ints<4, 8, 16, 32> kNc16Groups{};  // lanes per row: the smallest G >= C / 8

template <class T>
static void nc16_pack(const T* weight, int64_t P, int64_t Ck, int64_t Co, int64_t wk, int64_t wo, T* wp,
                      hipStream_t stream) {
  const int Kp = nc16_up(Ck, 16), Op = nc16_up(Co, 32);
  hipLaunchKernelGGL(nc16_pack_kernel<T>, dim3((unsigned)ceil_div(P * (Kp / 8) * Op, 256)), dim3(256), 0, stream, weight,
                     (int)P, (int)Ck, (int)Co, (int)wk, (int)wo, Kp, Op, wp);
}

// the row-list kernel over `rows` rows Ck wide into Co columns; false: the LDS attribute could not be raised
template <class T, int G, int NB>
static bool nc16_launch_conv(const NcList& ls, const T* src, const T* coeff, const T* wp, int64_t rows, int64_t Ck,
                             int64_t Co, int64_t P, int NH, T* out, hipStream_t stream) {
  auto kern = nc16_conv_kernel<T, G, NB>;
  static bool attr_set[64] = {false};  // per instantiation and DEVICE (a process may drive several GPUs)
  int dev = -1;
  const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;  // (unknown: set it on every call)
  if (!known || !attr_set[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kNc16LdsMax) != hipSuccess)
      return false;
    if (known) attr_set[dev] = true;
  }
  const size_t lds = (size_t)NH * kNcRows * (nc16_pc(G) * nc16_up(Ck, 16) + kNc16Pad) * sizeof(T);
  hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(rows, kNcRows * NH)), dim3(kNcBlock), lds, stream, ls, src, coeff, wp,
                     rows, (int)Ck, (int)Co, (int)P, NH, out);
  return true;
}

template <class T>
static bool nc16_conv(const NcList& ls, const T* src, const T* coeff, const T* wp, int64_t rows, int64_t Ck, int64_t Co,
                      int64_t P, T* out, hipStream_t stream) {
  return with_bucket(kNc16Groups, (int)(Ck / 8), [&](auto G) {
    constexpr int g = decltype(G)::value;
    if (Co > 128) return nc16_launch_conv<T, g, 2>(ls, src, coeff, wp, rows, Ck, Co, P, 1, out, stream);
    return nc16_launch_conv<T, g, 1>(ls, src, coeff, wp, rows, Ck, Co, P, Co <= 64 ? 2 : 1, out, stream);
  });
}

template <class T>
static int nc16_forward(const void* x, const int64_t* idx, const int64_t* lengths, const void* coeff, const void* weight,
                        int64_t N, int64_t L, int64_t M, int64_t K, int64_t P, int64_t Cin, int64_t Cout, void* out,
                        const Nc16Ws& ws, hipStream_t stream) {
  nc16_pack<T>((const T*)weight, P, Cin, Cout, Cout, 1, (T*)ws.pack, stream);
  if (!nc16_conv<T>(nc_forward_list(idx, lengths, L, K, M), (const T*)x, (const T*)coeff, (const T*)ws.pack, N * L, Cin,
                    Cout, P, (T*)out, stream))
    return check_launch("neighbor_conv16(attribute)");
  return check_launch("neighbor_conv16");
}

template <class T>
static int nc16_backward(const void* grad_out, const void* x, const int64_t* idx, const int64_t* lengths,
                         const void* coeff, const void* weight, int64_t N, int64_t L, int64_t M, int64_t K, int64_t P,
                         int64_t Cin, int64_t Cout, void* grad_x, void* grad_weight, void* grad_coeff, const Nc16Ws& ws,
                         hipStream_t stream) {
  const int64_t rows = N * L, targets = N * M;
  const NcList fwd = nc_forward_list(idx, lengths, L, K, M);
  const bool need_x = grad_x != nullptr && targets > 0, need_c = grad_coeff != nullptr && rows > 0;
  if (need_x || need_c)  // w(p, k = o, o' = c) = weight[p][c][o]
    nc16_pack<T>((const T*)weight, P, Cout, Cin, 1, Cout, (T*)ws.pack, stream);
  if (need_x) {
    const int rc = det_invert(ws.det, idx, nullptr, lengths, N, L, K, M, stream);
    if (rc != POINTOPS_OK) return rc;
    const NcList inv{nullptr, nullptr, ws.det.vals_out, ws.det.seg_start, ws.det.seg_end, 1, (int)K, (int)M};
    if (!nc16_conv<T>(inv, (const T*)grad_out, (const T*)coeff, (const T*)ws.pack, targets, Cout, Cin, P, (T*)grad_x,
                      stream))  // the source rows are g's: Cout wide
      return check_launch("neighbor_conv16_backward(attribute)");
  }
  if (grad_weight != nullptr) {
    const int64_t chunks = nc_chunks(rows, P), count = P * Cin * Cout;
    if (chunks > 0)
      hipLaunchKernelGGL(nc16_grad_w_kernel<T>,
                         dim3((unsigned)chunks, (unsigned)P, (unsigned)ceil_div(Cin, kNc16GwChannels)), dim3(kNcBlock), 0,
                         stream, fwd, (const T*)x, (const T*)coeff, (const T*)grad_out, rows, (int)Cin, (int)Cout,
                         (int)P, ws.partial);
    hipLaunchKernelGGL(nc16_sum_partials_kernel<T>, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, stream,
                       ws.partial, (int)chunks, count, (T*)grad_weight);
  }
  if (need_c) {
    with_bucket(kNc16Groups, (int)(Cin / 8), [&](auto G) {
      hipLaunchKernelGGL((nc16_grad_c_kernel<T, decltype(G)::value>), dim3((unsigned)ceil_div(rows, kNcRows)),
                         dim3(kNcBlock), 0, stream, fwd, (const T*)x, (const T*)grad_out, (const T*)ws.pack, rows,
                         (int)Cin, (int)Cout, (int)P, (T*)grad_coeff);
    });
  }
  return check_launch("neighbor_conv16_backward");
}

}  // namespace pointops

using namespace pointops;

#define NC16_BAD_SIZES                                                                                                \
  ": bad sizes (dtype 0 or 1, Cin and Cout multiples of 8 in [8, 256], 1 <= P <= 32, 1 <= K <= 255; N L K must be " \
  "below 2^31 and N M below 2^31 - 1)"

static bool nc16_dtype_ok(int dtype) { return dtype == POINTOPS_DTYPE_BF16 || dtype == POINTOPS_DTYPE_F16; }

extern "C" size_t pointops_neighbor_conv16_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M, int64_t P,
                                                           int64_t Cin, int64_t Cout) {
  if (!nc16_sizes_ok(N, L, M, K, P, Cin, Cout)) return 0;
  return nc16_carve(nullptr, nullptr, false, N, L, K, M, P, Cin, Cout);
}

extern "C" size_t pointops_neighbor_conv16_backward_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M,
                                                                    int64_t P, int64_t Cin, int64_t Cout) {
  if (!nc16_sizes_ok(N, L, M, K, P, Cin, Cout)) return 0;
  return nc16_carve(nullptr, nullptr, true, N, L, K, M, P, Cin, Cout);
}

extern "C" int pointops_neighbor_conv16(const void* x, const int64_t* idx, const int64_t* lengths, const void* coeff,
                                        const void* weight, int dtype, int64_t N, int64_t L, int64_t M, int64_t K,
                                        int64_t P, int64_t Cin, int64_t Cout, void* out, void* workspace,
                                        size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(nc16_dtype_ok(dtype) && nc16_sizes_ok(N, L, M, K, P, Cin, Cout), "neighbor_conv16" NC16_BAD_SIZES);
  POINTOPS_REQUIRE(coeff != nullptr || P == K, "neighbor_conv16: without coeff, P must be K");
  const int64_t rows = N * L;
  POINTOPS_REQUIRE(weight != nullptr && (rows == 0 || (idx != nullptr && out != nullptr)) &&
                       (x != nullptr || N * M == 0 || rows == 0),
                   "neighbor_conv16: null pointer");
  POINTOPS_REQUIRE(nc16_aligned(x, nullptr), "neighbor_conv16: x must be 16-byte aligned");
  Nc16Ws ws;
  POINTOPS_REQUIRE_WORKSPACE(
      workspace_fits(workspace, workspace_bytes, nc16_carve(&ws, workspace, false, N, L, K, M, P, Cin, Cout)),
      "neighbor_conv16: workspace too small");
  if (rows == 0) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  return dtype == POINTOPS_DTYPE_BF16
             ? nc16_forward<__bf16>(x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout, out, ws, stream)
             : nc16_forward<_Float16>(x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout, out, ws, stream);
}

extern "C" int pointops_neighbor_conv16_backward(const void* grad_out, const void* x, const int64_t* idx,
                                                 const int64_t* lengths, const void* coeff, const void* weight,
                                                 int dtype, int64_t N, int64_t L, int64_t M, int64_t K, int64_t P,
                                                 int64_t Cin, int64_t Cout, void* grad_x, void* grad_weight,
                                                 void* grad_coeff, void* workspace, size_t workspace_bytes,
                                                 void* stream_) {
  POINTOPS_REQUIRE(nc16_dtype_ok(dtype) && nc16_sizes_ok(N, L, M, K, P, Cin, Cout),
                   "neighbor_conv16_backward" NC16_BAD_SIZES);
  POINTOPS_REQUIRE(coeff != nullptr || P == K, "neighbor_conv16_backward: without coeff, P must be K");
  POINTOPS_REQUIRE(grad_coeff == nullptr || coeff != nullptr, "neighbor_conv16_backward: grad_coeff needs coeff");
  const int64_t rows = N * L, targets = N * M;
  POINTOPS_REQUIRE(weight != nullptr && (rows == 0 || (grad_out != nullptr && idx != nullptr)) &&
                       (x != nullptr || targets == 0 || rows == 0),
                   "neighbor_conv16_backward: null pointer");
  POINTOPS_REQUIRE(nc16_aligned(grad_out, x), "neighbor_conv16_backward: grad_out and x must be 16-byte aligned");
  Nc16Ws ws;
  POINTOPS_REQUIRE_WORKSPACE(
      workspace_fits(workspace, workspace_bytes, nc16_carve(&ws, workspace, true, N, L, K, M, P, Cin, Cout)),
      "neighbor_conv16_backward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  return dtype == POINTOPS_DTYPE_BF16
             ? nc16_backward<__bf16>(grad_out, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout, grad_x,
                                     grad_weight, grad_coeff, ws, stream)
             : nc16_backward<_Float16>(grad_out, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout, grad_x,
                                       grad_weight, grad_coeff, ws, stream);
}

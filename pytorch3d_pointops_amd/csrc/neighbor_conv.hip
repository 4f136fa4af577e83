// neighbor_conv.hip -- NEIGHBOUR CONVOLUTION (gfx950): out[n,l,:] = sum_p (sum_k coeff[n,l,k,p] x[n,idx[n,l,k],:]) weight[p]
// over a neighbour table (KPConv, PointConv, interpolated kernels; with coeff NULL the submanifold sparse convolution
// whose slot k is kernel offset k), and its backward, without the (N, L, K, Cin) and (N, L, P, Cin) tensors of
// knn_gather + einsum + matmul.  The definition is the NEIGHBOUR CONVOLUTION block of include/pointops_amd.h.
//
// Unlike neighbor_attention.hip there IS an operand to reuse: weight[p] is shared by every row, so the inner product is
// a GEMM (M = rows, k = P Cin, N = Cout) and runs on v_mfma_f32_32x32x2_f32, which feature_screen.h shows to be a
// k-ordered fmaf chain.  A 256-lane workgroup owns a tile of 32 rows of a ROW LIST:
//   forward   row (n,l), entries e = (n L + l) K + k, source x[n, idx[e]], coefficients coeff[e,:] or one-hot(k)
//   grad_x    target row (n,m), entries vals[seg_start .. seg_end) of the inverted table (backward_det.h), source
//             g[e / K], coefficients coeff[e,:] or one-hot(e % K), weights indexed transposed (no transposed copy)
//   gather    a group of G >= Cin / 4 lanes per row, 16 bytes per lane and entry, kNcUnroll row loads in flight before
//             the first multiply (neighbor_reduce.hip).  The entries of the tile are staged 32 per row at a time in LDS
//             (int32 source rows, -1 = masked), read coalesced.  A lane keeps acc[rows per lane][PC][4] for PC
//             consecutive p (PC = 16, 8, 4 for G <= 8, 16, 32: 64 registers); P > PC walks the lists once per chunk of
//             PC, the re-read rows coming from L2.  Without coeff an entry is only loaded in the chunk that holds its p:
//             every row is fetched once.  A tile walks to its longest list: a hub row serialises its tile.
//   matrix    for p ascending the A_p tile (32 x Cin) goes from the registers to LDS with the odd row stride Cin + 1
//             (the bank argument of feature_match.hip); wave w owns output columns [32 w, 32 w + 32) and ONE
//             accumulator block carried across all p, written once.  B[k = 2 kk + h][o = lane & 31] is read straight
//             from global memory, coalesced for the forward (weight is at most 2 MiB: cache-resident); columns past
//             Cout are zero-filled.  Cout <= 64 leaves waves idle in this stage.
//   grad_w    workgroups (row chunk, p): the same gather with PC = 1 rebuilds A_p, then A_p^T g on the MFMA with the
//             rows on the k side, up to four 32 x 32 blocks per wave accumulated over the chunk's tiles; one partial
//             per workgroup in the workspace, added in ascending chunk order by nc_sum_partials_kernel.
//   grad_c    per row tile and p, T_p = g_tile weight[p]^T on the MFMA into LDS, then the lane groups dot T_p[row] with
//             the gathered x row of every slot: the lane's four products ascending, then wave_sum<G>.
// No float atomics; every output row is written once.  Fixed launch sequences, nothing is read back.
#include "neighbor_conv.h"

namespace pointops {

constexpr int kNcMaxC = 128;

constexpr int nc_pc(int G) { return G >= 32 ? 4 : (G >= 16 ? 8 : 16); }
constexpr int nc_rpl(int G) { return G >= 8 ? G / 8 : 1; }  // rows of the tile a lane works on

// acc[i][p][:] = the lane's four channels of A[row grp + i GR][p0 + p] over the row's list, in list order from +0.0f.
// Call from workgroup-uniform control flow.
template <int G, int PC>
__device__ __forceinline__ void nc_gather(float (&acc)[nc_rpl(G)][PC][4], const NcList& ls,
                                          const float* __restrict__ src, const float* __restrict__ coeff, int64_t row0,
                                          int64_t rows, int C, int P, int p0, int* s_src, int* s_ent, int* s_cnt) {
  constexpr int GR = kNcBlock / G, RPL = nc_rpl(G), U = kNcUnroll;
  const int grp = threadIdx.x / G, ch = (threadIdx.x % G) * 4;
  __syncthreads();
  if (threadIdx.x < kNcRows) s_cnt[threadIdx.x] = nc_count(ls, row0 + threadIdx.x, rows);
  __syncthreads();
  int longest = 0;
  for (int r = 0; r < kNcRows; ++r) longest = max(longest, s_cnt[r]);
#pragma unroll
  for (int i = 0; i < RPL; ++i)
#pragma unroll
    for (int p = 0; p < PC; ++p) acc[i][p][0] = acc[i][p][1] = acc[i][p][2] = acc[i][p][3] = 0.0f;

  for (int t0 = 0; t0 < longest; t0 += kNcWin) {
    nc_stage(ls, row0, rows, t0, s_src, s_ent);
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
      const int r = grp + i * GR;
      if (r >= kNcRows) continue;
      const int nent = min(kNcWin, s_cnt[r] - t0);
      for (int jb = 0; jb < nent; jb += U) {
        int s[U], e[U];
        float v[U][4];
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
          float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (s[u] >= 0 && ch < C) t = *reinterpret_cast<const float4*>(src + (int64_t)s[u] * C + ch);
          v[u][0] = t.x, v[u][1] = t.y, v[u][2] = t.z, v[u][3] = t.w;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // list order
          if (s[u] < 0) continue;
          const int pe = e[u] % ls.K;
#pragma unroll
          for (int p = 0; p < PC; ++p) {
            if (p0 + p >= P) continue;  // (workgroup-uniform)
            if (coeff != nullptr) {
              const float cf = coeff[(int64_t)e[u] * P + p0 + p];
#pragma unroll
              for (int x = 0; x < 4; ++x) acc[i][p][x] = __builtin_fmaf(cf, v[u][x], acc[i][p][x]);
            } else if (pe == p0 + p) {
#pragma unroll
              for (int x = 0; x < 4; ++x) acc[i][p][x] = acc[i][p][x] + v[u][x];
            }
          }
        }
      }
    }
  }
}

// the lane's channels of plane p of acc -> the tile in LDS, row stride `stride`.  Barriers are the caller's.
template <int G, int PC>
__device__ __forceinline__ void nc_put(const float (&acc)[nc_rpl(G)][PC][4], int p, float* s_A, int stride, int C) {
  constexpr int GR = kNcBlock / G, RPL = nc_rpl(G);
  const int grp = threadIdx.x / G, ch = (threadIdx.x % G) * 4;
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const int r = grp + i * GR;
    if (r < kNcRows && ch < C) {
#pragma unroll
      for (int x = 0; x < 4; ++x) s_A[r * stride + ch + x] = acc[i][p][x];
    }
  }
}

// out[row,:] (Co wide) = sum over p, c ascending of A[row][p][c] w(p, c, o), w(p, c, o) = weight[p Ck Co + c wk + o wo];
// A over the row list `ls` of rows Ck wide in `src`.
template <int G>
__global__ __launch_bounds__(kNcBlock) void nc_conv_kernel(NcList ls, const float* __restrict__ src,
                                                           const float* __restrict__ coeff,
                                                           const float* __restrict__ weight, int64_t rows, int Ck,
                                                           int Co, int P, int wk, int wo, float* __restrict__ out) {
  constexpr int PC = nc_pc(G);
  __shared__ float s_A[kNcRows * (kNcMaxC + 1)];
  __shared__ int s_src[kNcRows * kNcWin], s_ent[kNcRows * kNcWin], s_cnt[kNcRows];
  const int64_t row0 = (int64_t)blockIdx.x * kNcRows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int stride = Ck + 1, oc = wave * 32 + c;
  const bool block = wave * 32 < Co, col = oc < Co;  // (block: wave-uniform)
  f32x16 o16;
#pragma unroll
  for (int r = 0; r < 16; ++r) o16[r] = 0.0f;

  for (int p0 = 0; p0 < P; p0 += PC) {
    float acc[nc_rpl(G)][PC][4];
    nc_gather<G, PC>(acc, ls, src, coeff, row0, rows, Ck, P, p0, s_src, s_ent, s_cnt);
#pragma unroll
    for (int p = 0; p < PC; ++p) {
      if (p0 + p < P) {  // (workgroup-uniform)
        __syncthreads();
        nc_put<G, PC>(acc, p, s_A, stride, Ck);
        __syncthreads();
        if (block) {
          const float* a = s_A + c * stride + h;  // A[i = c][k = 2 kk + h]
          const float* __restrict__ b = weight + (int64_t)(p0 + p) * Ck * Co + (int64_t)h * wk + (int64_t)(col ? oc : 0) * wo;
          int kk = 0;
          for (; kk + 8 <= Ck / 2; kk += 8) {  // eight B loads in flight, then the eight steps in k order
            float bv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) bv[q] = col ? b[(int64_t)2 * (kk + q) * wk] : 0.0f;  // B[k = 2 kk + h][o = oc]
#pragma unroll
            for (int q = 0; q < 8; ++q) o16 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * (kk + q)], bv[q], o16, 0, 0, 0);
          }
          for (; kk < Ck / 2; ++kk) {
            const float bv = col ? b[(int64_t)2 * kk * wk] : 0.0f;
            o16 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * kk], bv, o16, 0, 0, 0);
          }
        }
      }
    }
  }
  if (!col) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (row < rows) out[row * Co + oc] = o16[r];
  }
}

// partial[(chunk P + p) Cin Cout + c Cout + o] = sum over the rows of the chunk's tiles, ascending, of A[row][p][c] g[row][o]
template <int G>
__global__ __launch_bounds__(kNcBlock) void nc_grad_w_kernel(NcList ls, const float* __restrict__ x,
                                                             const float* __restrict__ coeff,
                                                             const float* __restrict__ g, int64_t rows, int Cin,
                                                             int Cout, int P, float* __restrict__ partial) {
  __shared__ float s_A[kNcRows * (kNcMaxC + 1)], s_G[kNcRows * kNcMaxC];
  __shared__ int s_src[kNcRows * kNcWin], s_ent[kNcRows * kNcWin], s_cnt[kNcRows];
  const int p = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int stride = Cin + 1, nco = (Cout + 31) / 32, nblk = ((Cin + 31) / 32) * nco;
  f32x16 o16[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) o16[q][r] = 0.0f;

  const int64_t ntiles = (rows + kNcRows - 1) / kNcRows;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kNcRows;
    float acc[nc_rpl(G)][1][4];
    nc_gather<G, 1>(acc, ls, x, coeff, row0, rows, Cin, P, p, s_src, s_ent, s_cnt);
    __syncthreads();
    nc_put<G, 1>(acc, 0, s_A, stride, Cin);
    for (int i = threadIdx.x; i < kNcRows * Cout; i += kNcBlock)
      s_G[i] = row0 * Cout + i < rows * Cout ? g[row0 * Cout + i] : 0.0f;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int blk = wave + 4 * q;
      if (blk < nblk) {  // (wave-uniform)
        const int ci = (blk / nco) * 32 + c, o = (blk % nco) * 32 + c;
#pragma unroll 4
        for (int kk = 0; kk < kNcRows / 2; ++kk) {  // the rows are the k side
          const int row = 2 * kk + h;
          const float av = ci < Cin ? s_A[row * stride + ci] : 0.0f;
          const float bv = o < Cout ? s_G[row * Cout + o] : 0.0f;
          o16[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, o16[q], 0, 0, 0);
        }
      }
    }
  }
  float* __restrict__ dst = partial + ((int64_t)blockIdx.x * P + p) * Cin * Cout;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int blk = wave + 4 * q;
    if (blk >= nblk) continue;
    const int o = (blk % nco) * 32 + c;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = (blk / nco) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ci < Cin && o < Cout) dst[ci * Cout + o] = o16[q][r];
    }
  }
}

__global__ __launch_bounds__(256) void nc_sum_partials_kernel(const float* __restrict__ partial, int chunks,
                                                              int64_t count, float* __restrict__ grad_w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float s = 0.0f;
  for (int ch = 0; ch < chunks; ++ch) s = s + partial[(int64_t)ch * count + i];
  grad_w[i] = s;
}

// grad_coeff[e,p] = x[n,idx[e],:] . (g[n,l,:] weight[p]^T) for a valid slot, else 0
template <int G>
__global__ __launch_bounds__(kNcBlock) void nc_grad_c_kernel(NcList ls, const float* __restrict__ x,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ weight, int64_t rows, int Cin,
                                                             int Cout, int P, float* __restrict__ grad_c) {
  constexpr int GR = kNcBlock / G, RPL = nc_rpl(G), U = kNcUnroll;
  __shared__ float s_G[kNcRows * (kNcMaxC + 1)], s_T[kNcRows * (kNcMaxC + 1)];
  __shared__ int s_src[kNcRows * kNcWin], s_ent[kNcRows * kNcWin];
  const int64_t row0 = (int64_t)blockIdx.x * kNcRows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
  const int grp = threadIdx.x / G, j = threadIdx.x % G, ch = j * 4;
  const int gs = Cout + 1, ts = Cin + 1, ci = wave * 32 + c;
  const bool block = wave * 32 < Cin, col = ci < Cin;
  const int K = ls.K, nwin = (K + kNcWin - 1) / kNcWin;
  for (int i = threadIdx.x; i < kNcRows * Cout; i += kNcBlock) {
    const int r = i / Cout, o = i - r * Cout;
    s_G[r * gs + o] = row0 + r < rows ? g[(row0 + r) * Cout + o] : 0.0f;
  }
  for (int p = 0; p < P; ++p) {
    __syncthreads();
    if (block) {
      f32x16 t16;
#pragma unroll
      for (int r = 0; r < 16; ++r) t16[r] = 0.0f;
      const float* a = s_G + c * gs + h;  // A[i = c][k = 2 kk + h]
      const float* __restrict__ b = weight + ((int64_t)p * Cin + (col ? ci : 0)) * Cout + h;  // B[k][o = ci] = w[p][ci][k]
#pragma unroll 8
      for (int kk = 0; kk < Cout / 2; ++kk)
        t16 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * kk], col ? b[2 * kk] : 0.0f, t16, 0, 0, 0);
      if (col) {
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
        float tv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ch < Cin) {
#pragma unroll
          for (int xx = 0; xx < 4; ++xx) tv[xx] = s_T[r * ts + ch + xx];
        }
        for (int jb = 0; jb < nent; jb += U) {
          int s[U], e[U];
          float v[U][4];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const bool in = jb + u < nent;
            s[u] = in ? s_src[r * kNcWin + jb + u] : -1;
            e[u] = in ? s_ent[r * kNcWin + jb + u] : 0;
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s[u] >= 0 && ch < Cin) t = *reinterpret_cast<const float4*>(x + (int64_t)s[u] * Cin + ch);
            v[u][0] = t.x, v[u][1] = t.y, v[u][2] = t.z, v[u][3] = t.w;
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (jb + u >= nent) continue;  // (workgroup-uniform)
            float d = tv[0] * v[u][0];
            d = d + tv[1] * v[u][1];
            d = d + tv[2] * v[u][2];
            d = d + tv[3] * v[u][3];
            d = wave_sum<G>(d);
            if (j == 0 && row0 + r < rows) grad_c[(int64_t)e[u] * P + p] = s[u] >= 0 ? d : 0.0f;
          }
        }
      }
    }
  }
}

struct NcWs {
  DetWs det;
  float* partial;  // (chunks P Cin Cout) of nc_grad_w_kernel
};

static size_t nc_carve(NcWs* ws, void* base, int64_t N, int64_t L, int64_t K, int64_t M, int64_t P, int64_t Cin,
                       int64_t Cout) {
  NcWs w;
  Carver c(base);
  w.det.keys_in = nullptr;
  c.off = det_carve(base ? &w.det : nullptr, base, N, L, K, M);
  const int64_t chunks = nc_chunks(N * L, P);
  w.partial = (float*)c.take(sizeof(float) * (size_t)((chunks > 0 ? chunks : 1) * P * Cin * Cout));
  if (ws) *ws = w;
  return c.off;
}

static bool nc_sizes_ok(int64_t N, int64_t L, int64_t M, int64_t K, int64_t P, int64_t Cin, int64_t Cout) {
  return N >= 0 && M >= 0 && L >= 0 && K >= 1 && K <= kNcMaxK && P >= 1 && P <= kNcMaxP && Cin >= 4 &&
         Cin <= kNcMaxC && Cin % 4 == 0 && Cout >= 4 && Cout <= kNcMaxC && Cout % 4 == 0 && N < (1LL << 31) &&
         M < (1LL << 31) && L < (1LL << 31) && N * L < (1LL << 31) && N * L * K < (1LL << 31) &&
         N * M < (1LL << 31) - 1;
}

static bool nc_aligned(const void* a, const void* b, const void* c) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16) == 0;
}

constexpr Ints<1, 2, 4, 8, 16, 32> kNcGroups{};  // lanes per row: the smallest G >= C / 4

}  // namespace pointops

using namespace pointops;

#define NC_BAD_SIZES                                                                                                  \
  ": bad sizes (Cin and Cout multiples of 4 in [4, 128], 1 <= P <= 32, 1 <= K <= 255; N L K must be below 2^31 and " \
  "N M below 2^31 - 1)"

extern "C" size_t pointops_neighbor_conv_backward_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M, int64_t P,
                                                                  int64_t Cin, int64_t Cout) {
  if (!nc_sizes_ok(N, L, M, K, P, Cin, Cout)) return 0;
  return nc_carve(nullptr, nullptr, N, L, K, M, P, Cin, Cout);
}

extern "C" int pointops_neighbor_conv(const float* x, const int64_t* idx, const int64_t* lengths, const float* coeff,
                                      const float* weight, int64_t N, int64_t L, int64_t M, int64_t K, int64_t P,
                                      int64_t Cin, int64_t Cout, float* out, void* stream_) {
  POINTOPS_REQUIRE(nc_sizes_ok(N, L, M, K, P, Cin, Cout), "neighbor_conv" NC_BAD_SIZES);
  POINTOPS_REQUIRE(coeff != nullptr || P == K, "neighbor_conv: without coeff, P must be K");
  const int64_t rows = N * L;
  if (rows == 0) return POINTOPS_OK;
  POINTOPS_REQUIRE(idx != nullptr && weight != nullptr && out != nullptr && (x != nullptr || N * M == 0),
                   "neighbor_conv: null pointer");
  POINTOPS_REQUIRE(nc_aligned(x, nullptr, nullptr), "neighbor_conv: x must be 16-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  const NcList ls = nc_forward_list(idx, lengths, L, K, M);
  with_bucket(kNcGroups, (int)(Cin / 4), [&](auto G) {
    hipLaunchKernelGGL((nc_conv_kernel<decltype(G)::value>), dim3((unsigned)ceil_div(rows, kNcRows)), dim3(kNcBlock), 0,
                       stream, ls, x, coeff, weight, rows, (int)Cin, (int)Cout, (int)P, (int)Cout, 1, out);
  });
  return check_launch("neighbor_conv");
}

extern "C" int pointops_neighbor_conv_backward(const float* grad_out, const float* x, const int64_t* idx,
                                               const int64_t* lengths, const float* coeff, const float* weight,
                                               int64_t N, int64_t L, int64_t M, int64_t K, int64_t P, int64_t Cin,
                                               int64_t Cout, float* grad_x, float* grad_weight, float* grad_coeff,
                                               void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(nc_sizes_ok(N, L, M, K, P, Cin, Cout), "neighbor_conv_backward" NC_BAD_SIZES);
  POINTOPS_REQUIRE(coeff != nullptr || P == K, "neighbor_conv_backward: without coeff, P must be K");
  POINTOPS_REQUIRE(grad_coeff == nullptr || coeff != nullptr, "neighbor_conv_backward: grad_coeff needs coeff");
  const int64_t rows = N * L, targets = N * M;
  POINTOPS_REQUIRE(weight != nullptr && (rows == 0 || (grad_out != nullptr && idx != nullptr)) &&
                       (x != nullptr || targets == 0 || rows == 0),
                   "neighbor_conv_backward: null pointer");
  POINTOPS_REQUIRE(nc_aligned(grad_out, x, nullptr), "neighbor_conv_backward: grad_out and x must be 16-byte aligned");
  NcWs ws;
  POINTOPS_REQUIRE_WORKSPACE(
      workspace_fits(workspace, workspace_bytes, nc_carve(&ws, workspace, N, L, K, M, P, Cin, Cout)),
      "neighbor_conv_backward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const NcList fwd = nc_forward_list(idx, lengths, L, K, M);
  const unsigned tiles = (unsigned)ceil_div(rows, kNcRows);
  if (grad_x != nullptr && targets > 0) {
    const int rc = det_invert(ws.det, idx, nullptr, lengths, N, L, K, M, stream);
    if (rc != POINTOPS_OK) return rc;
    const NcList inv{nullptr, nullptr, ws.det.vals_out, ws.det.seg_start, ws.det.seg_end, 1, (int)K, (int)M};
    with_bucket(kNcGroups, (int)(Cout / 4), [&](auto G) {  // the source rows are g's: Cout wide
      hipLaunchKernelGGL((nc_conv_kernel<decltype(G)::value>), dim3((unsigned)ceil_div(targets, kNcRows)),
                         dim3(kNcBlock), 0, stream, inv, grad_out, coeff, weight, targets, (int)Cout, (int)Cin, (int)P,
                         1, (int)Cout, grad_x);
    });
  }
  if (grad_weight != nullptr) {
    const int64_t chunks = nc_chunks(rows, P);
    if (chunks > 0) {
      with_bucket(kNcGroups, (int)(Cin / 4), [&](auto G) {
        hipLaunchKernelGGL((nc_grad_w_kernel<decltype(G)::value>), dim3((unsigned)chunks, (unsigned)P), dim3(kNcBlock),
                           0, stream, fwd, x, coeff, grad_out, rows, (int)Cin, (int)Cout, (int)P, ws.partial);
      });
    }
    const int64_t count = P * Cin * Cout;
    hipLaunchKernelGGL(nc_sum_partials_kernel, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, stream, ws.partial,
                       (int)chunks, count, grad_weight);
  }
  if (grad_coeff != nullptr && rows > 0) {
    with_bucket(kNcGroups, (int)(Cin / 4), [&](auto G) {
      hipLaunchKernelGGL((nc_grad_c_kernel<decltype(G)::value>), dim3(tiles), dim3(kNcBlock), 0, stream, fwd, x,
                         grad_out, weight, rows, (int)Cin, (int)Cout, (int)P, grad_coeff);
    });
  }
  return check_launch("neighbor_conv_backward");
}

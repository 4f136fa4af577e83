// neighbor_mlp.h -- what the float32 kernels (neighbor_mlp.hip) and the 16-bit kernels (neighbor_mlp16.hip) of the
// NEIGHBOUR MLP-MAX share: the staging of a window of slots, the chunks of grad_weight / grad_bias and the summing of
// their partials, and the index and alignment checks.
#pragma once
#include "backward_det.h"
#include "dispatch.h"
#include "wave.h"

namespace pointops {

constexpr int kNmBlock = 256;
constexpr int kNmWin = 32;          // slots of a row staged at a time
constexpr int kNmMaxK = 255;
constexpr int kNmMaxChunks = 1024;  // grad_weight / grad_bias: partial sums at the most

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline int64_t nm_chunks(int64_t rows) {
  const int64_t c = ceil_div(rows, 32);
  return c < 1 ? 1 : (c < kNmMaxChunks ? c : kNmMaxChunks);
}

// Slots [k0, k0 + kt) of the R = 32 RT rows from row0: s_src[slot][row] the flat source row (int32, -1 = masked, so no
// branch on loaded values), s_mask[slot][row tile] the validity bits of the tile's 32 rows.  Call from workgroup-uniform
// control flow; the masks are visible after the caller's next barrier.
template <int R, int RT>
__device__ __forceinline__ void nm_stage(const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths,
                                         int64_t row0, int64_t rows, int L, int K, int M, int k0, int kt, int* s_src,
                                         uint32_t* s_mask) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int i = t; i < R * kt; i += kNmBlock) {  // one coalesced pass over the table
    const int r = i / kt, kk = i - r * kt;
    const int64_t row = row0 + r;
    int s = -1;
    if (row < rows) {
      const int64_t n = row / L, m = idx[row * K + k0 + kk];
      const int64_t len = lengths == nullptr ? INT64_MAX : lengths[n];
      if (m >= 0 && m < M && k0 + kk < len) s = (int)(n * M + m);
    }
    s_src[kk * R + r] = s;
  }
  __syncthreads();
  for (int i = t; i < kt * RT; i += kNmBlock) {
    const int kk = i / RT, tile = i - kk * RT;
    uint32_t m = 0;
    for (int r = 0; r < 32; ++r) m |= (s_src[kk * R + tile * 32 + r] >= 0 ? 1u : 0u) << r;
    s_mask[i] = m;
  }
}

// the chunks' partial sums in ascending chunk order, each result rounded once to T (float: as it is): rows i < C1 to
// grad_weight, row C1 to grad_bias (either may be null)
template <class T>
__global__ __launch_bounds__(256) void nm_sum_partials_kernel(const float* __restrict__ partial, int chunks, int C1,
                                                              int C2, T* __restrict__ grad_w, T* __restrict__ grad_b) {
  const int i = blockIdx.x * 256 + threadIdx.x, count = (C1 + 1) * C2;
  if (i >= count) return;
  float s = 0.0f;
  for (int ch = 0; ch < chunks; ++ch) s = s + partial[(int64_t)ch * count + i];
  if (i < C1 * C2) {
    if (grad_w != nullptr) grad_w[i] = (T)s;
  } else if (grad_b != nullptr) {
    grad_b[i - C1 * C2] = (T)s;
  }
}

// the index limits of every entry: the table fits int32 entries and the inverted table's keys
inline bool nm_index_ok(int64_t N, int64_t L, int64_t M, int64_t K) {
  return N >= 0 && M >= 0 && L >= 0 && K >= 1 && K <= kNmMaxK && N < (1LL << 31) && M < (1LL << 31) &&
         L < (1LL << 31) && N * L < (1LL << 31) && N * L * K < (1LL << 31) && N * M < (1LL << 31) - 1;
}

inline bool nm_aligned(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) % 16) == 0;
}

}  // namespace pointops

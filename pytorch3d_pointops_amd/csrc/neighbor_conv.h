// neighbor_conv.h -- what the float32 kernels (neighbor_conv.hip) and the 16-bit kernels (neighbor_conv16.hip) of the
// NEIGHBOUR CONVOLUTION share: the row list (the forward table, or det_invert's inverted table), its staging in LDS,
// and the chunks of grad_weight.
#pragma once
#include "backward_det.h"
#include "dispatch.h"
#include "wave.h"

namespace pointops {

constexpr int kNcBlock = 256;  // lanes of a workgroup
constexpr int kNcRows = 32;    // rows of a tile: the M side of one MFMA block
constexpr int kNcWin = 32;     // entries of a row staged at a time
constexpr int kNcUnroll = 4;   // row loads in flight
constexpr int kNcMaxP = 32, kNcMaxK = 255;
constexpr int kNcTargetGroups = 1024;  // grad_w: about this many workgroups (row chunks x P)

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct NcList {
  const int64_t* idx;  // forward list: the table and its lengths
  const int64_t* lengths;
  const unsigned* vals;  // inverted list (non-null selects it): det_invert's entries and segments
  const int* seg_start;
  const int* seg_end;
  int L, K, M;
};

__device__ __forceinline__ int nc_count(const NcList& ls, int64_t row, int64_t rows) {
  if (row >= rows) return 0;
  return ls.vals != nullptr ? ls.seg_end[row] - ls.seg_start[row] : ls.K;
}

// Entries [t0, t0 + kNcWin) of the tile's rows: s_src the flat source row (-1: masked or past the list), s_ent the
// entry e.  Call from workgroup-uniform control flow.
__device__ __forceinline__ void nc_stage(const NcList& ls, int64_t row0, int64_t rows, int t0, int* s_src, int* s_ent) {
  __syncthreads();
  for (int i = threadIdx.x; i < kNcRows * kNcWin; i += kNcBlock) {
    const int r = i / kNcWin, t = t0 + i % kNcWin;
    const int64_t row = row0 + r;
    int s = -1, e = 0;
    if (row < rows) {
      if (ls.vals != nullptr) {
        const int at = ls.seg_start[row] + t;
        if (at < ls.seg_end[row]) {
          e = (int)ls.vals[at];
          s = e / ls.K;
        }
      } else if (t < ls.K) {
        e = (int)(row * ls.K + t);
        const int64_t n = row / ls.L, m = ls.idx[e];
        const int64_t len = ls.lengths == nullptr ? INT64_MAX : ls.lengths[n];
        if (m >= 0 && m < ls.M && t < len) s = (int)(n * ls.M + m);
      }
    }
    s_src[i] = s;
    s_ent[i] = e;
  }
  __syncthreads();
}

inline int64_t nc_chunks(int64_t rows, int64_t P) {
  const int64_t tiles = ceil_div(rows, kNcRows), most = kNcTargetGroups / P > 1 ? kNcTargetGroups / P : 1;
  return tiles < most ? tiles : most;
}

inline NcList nc_forward_list(const int64_t* idx, const int64_t* lengths, int64_t L, int64_t K, int64_t M) {
  return NcList{idx, lengths, nullptr, nullptr, nullptr, (int)(L > 0 ? L : 1), (int)K, (int)M};
}

}  // namespace pointops

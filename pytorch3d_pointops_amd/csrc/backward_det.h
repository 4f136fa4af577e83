// backward_det.h -- the neighbour-table inversion of backward_det.hip for the other pull backward passes
// (neighbor_reduce.hip): the workspace layout, and the stable sort that leaves every target row's entries together in
// table order.  The bodies are backward_det.hip's.
#pragma once
#include "common.h"

namespace pointops {

struct DetWs {
  unsigned *keys_in, *keys_out, *vals_in, *vals_out;
  int *seg_start, *seg_end;  // per target row (+ the slot of masked entries)
  void* sort_tmp;
  size_t sort_tmp_bytes;
};

// the table of N L K entries (at least one) keyed by the N M target rows: the bytes of the layout; with a non-null
// `ws`, its arrays inside `base`
size_t det_carve(DetWs* ws, void* base, int64_t N, int64_t L, int64_t K, int64_t M);

// keys, stable sort, segments; afterwards entries vals_out[seg_start[r] .. seg_end[r]) are those of target row
// r = n M + idx, e = (n L + i) K + k ascending.  Masked: k >= min(lengths2[n], K) (lengths2 may be null),
// i >= lengths1[n] (lengths1 may be null), idx outside [0, M).  Needs N L K < 2^31 and N M < 2^31 - 1.
int det_invert(const DetWs& ws, const int64_t* idx, const int64_t* lengths1, const int64_t* lengths2, int64_t N,
               int64_t L, int64_t K, int64_t M, hipStream_t stream);

}  // namespace pointops

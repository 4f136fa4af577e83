// feature_match.h -- the launches of feature_match.hip that the K <= 32 screen (feature_topk.hip) shares with it.
#pragma once
#include "common.h"

namespace pointops {

// n1 (N,P1), n2 (N,P2): screen_norm of every row; n2max (N,) (cleared by the caller): the bits of the largest n2 over
// j < lengths2[n], by integer atomicMax (a NaN or +inf norm wins it, which marks the cloud)
void launch_feature_norms(const float* p1, const float* p2, const int64_t* l2, int64_t N, int64_t P1, int64_t P2,
                          int64_t D, float* n1, float* n2, unsigned* n2max, hipStream_t stream);

// stats (N,4): screened, certified, listed, `lists`; `qcount` null: the exact search, all 0
void launch_feature_stats(const int64_t* l1, const int64_t* l2, int64_t N, int64_t P1, int64_t P2, const int* qcount,
                          int lists, int32_t* stats, hipStream_t stream);

}  // namespace pointops

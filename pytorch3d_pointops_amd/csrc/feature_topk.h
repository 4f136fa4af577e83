// feature_topk.h -- the scalar definitions of the K <= 32 feature screen (feature_topk.hip; C ABI: pointops_feature_topk,
// whose FEATURE TOP-K block in include/pointops_amd.h is the definition of the operator).  __host__ __device__ and free
// of HIP types, on top of feature_screen.h alone: tests/native/feature_topk_main.cpp compiles the two headers and holds
// the merge, r_K and the certificate to a brute-force top K.
//
// List geometry.  A query keeps 2 S lists (S in {1, 4}) of M = 16 keys.  Target j of a cloud belongs to list
//   t(j) = 2 ((j >> 5) mod S) + ((j >> 2) & 1)                                                   topk_list_of
// -- the wave of the workgroup that sees its 32-row block, and the half of the accumulator map of
// v_mfma_f32_32x32x2_f32 that holds its row.  Each list keeps the M smallest (s, j) of its targets (s: screen_value).
//
// After the scan every collected target gets the reference's distance r (exact_distance) and a 64-bit key
// (r bits << 32 | j): for r >= +0 and not NaN the unsigned order of the keys is the (r, j) order of the operator.  The
// lists are sorted by key and merged for the first K keys (topk_merge); r_K is the distance of the K-th, +inf when
// fewer than K targets were collected (the empty key is (+inf, INT_MAX)).
//
// The certificate (topk_certified) is feature_screen.h's with "two lanes" replaced by "2 S lists".  Every target j a
// list drops has (s_j, j) >= that list's M-th key, so s_j >= s_cut, the smallest M-th key over the 2 S lists (+inf for a
// list that never filled), and r_j >= s_cut - E.  fl(r_K + E) < s_cut implies r_K + E < s_cut (rounding to nearest is
// monotone, s_cut is a float), hence r_j > r_K for every dropped j: the K nearest are among the collected targets and no
// tie crosses the cut.  A cloud of at most M targets is collected whole by any geometry.  Rows whose norms fail
// screen_row_finite are never certified.
#pragma once
#include "feature_screen.h"

namespace pointops {

constexpr int kTopkM = 16;        // keys per list
constexpr int kTopkMaxK = 32;     // the screen's largest K
constexpr int kTopkMaxLists = 8;  // 2 S, S = 4
constexpr uint64_t kTopkEmpty = 0x7f8000007fffffffULL;  // (+inf, INT_MAX)

POINTOPS_SCREEN_HD int topk_list_of(int64_t j, int S) { return 2 * (int)((j >> 5) % S) + (int)((j >> 2) & 1); }

POINTOPS_SCREEN_HD uint64_t topk_key(float r, int j) {
  uint32_t bits;
  memcpy(&bits, &r, sizeof(bits));
  return ((uint64_t)bits << 32) | (uint32_t)j;
}

POINTOPS_SCREEN_HD float topk_key_dist(uint64_t key) {
  const uint32_t bits = (uint32_t)(key >> 32);
  float r;
  memcpy(&r, &bits, sizeof(r));
  return r;
}

// The first K keys of LISTS sorted lists of kTopkM keys, ascending; returns r_K.  load(t, k): key k of list t;
// store(k, key): the k-th merged key.  Keys of different lists differ (a target is in one list) except the empty key,
// where any choice gives the same output.  The list index stays a compile-time constant: everything is in registers.
template <int LISTS, class Load, class Store>
POINTOPS_SCREEN_HD float topk_merge(int K, Load load, Store store) {
  uint64_t head[LISTS];
  int at[LISTS];
#pragma unroll
  for (int t = 0; t < LISTS; ++t) {
    head[t] = load(t, 0);
    at[t] = 0;
  }
  uint64_t best = kTopkEmpty;
  for (int k = 0; k < K; ++k) {
    best = head[0];
    int win = 0;
#pragma unroll
    for (int t = 1; t < LISTS; ++t) {
      if (head[t] < best) {
        best = head[t];
        win = t;
      }
    }
    store(k, best);
#pragma unroll
    for (int t = 0; t < LISTS; ++t) {
      if (t == win) {
        ++at[t];
        head[t] = at[t] < kTopkM ? load(t, at[t]) : kTopkEmpty;
      }
    }
  }
  return topk_key_dist(best);
}

// The certificate of one row.  rK: topk_merge's; s_cut: the smallest M-th screen key over the 2 S lists.
POINTOPS_SCREEN_HD bool topk_certified(int D, float n1, float n2max, int len2, float rK, float E, float s_cut) {
  if (!screen_row_finite(D, n1, n2max)) return false;
  if (len2 <= kTopkM) return true;
  const float lhs = rK + E;
  return lhs < s_cut;
}

}  // namespace pointops

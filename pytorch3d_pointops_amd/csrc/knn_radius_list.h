// knn_radius_list.h -- the per-lane result list of knn_in_radius (knn_in_radius.hip): the KC smallest 64-bit keys
// (d2 bits << 32 | j) seen so far, ascending.  d2 is a non-negative fp32 that is not a NaN, so the order of its bit
// patterns is the order of its values, and two candidates of equal distance are ordered by their index: the list order
// IS the header's (d2, j) order, and no two keys are equal.  __host__ __device__ and free of HIP types:
// tests/native/knn_in_radius_list_main.cpp compiles this header alone and fuzzes it against std::sort.
//
// Every loop has constant bounds and every slot a constant index, so the list of a kernel instance lives in registers
// (two per slot); a dynamically indexed slot would move the whole list to scratch memory.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define POINTOPS_LIST_HD __host__ __device__ inline
#else
#define POINTOPS_LIST_HD inline
#endif

namespace pointops {

constexpr uint64_t kRadiusListEmpty = ~(uint64_t)0;  // above every key: the upper half of a key is never a NaN's bits

POINTOPS_LIST_HD uint32_t radius_list_bits(float d2) {
  uint32_t b;
  memcpy(&b, &d2, sizeof(b));
  return b;
}
POINTOPS_LIST_HD uint64_t radius_list_key(float d2, uint32_t j) { return ((uint64_t)radius_list_bits(d2) << 32) | j; }
POINTOPS_LIST_HD float radius_list_d2(uint64_t key) {
  const uint32_t b = (uint32_t)(key >> 32);
  float d2;
  memcpy(&d2, &b, sizeof(d2));
  return d2;
}
POINTOPS_LIST_HD uint32_t radius_list_index(uint64_t key) { return (uint32_t)key; }

template <int KC>
struct RadiusList {
  uint64_t top[KC];  // ascending; kRadiusListEmpty behind the keys held

  POINTOPS_LIST_HD void clear() {
#if defined(__HIPCC__) || defined(__HIP__)
#pragma unroll
#endif
    for (int t = 0; t < KC; ++t) top[t] = kRadiusListEmpty;
  }

  // a key at or above it cannot enter the list
  POINTOPS_LIST_HD uint64_t worst() const { return top[KC - 1]; }

  // Inserts `key` where it belongs and drops the largest: slot t becomes max(top[t - 1], min(key, top[t])) -- the old
  // neighbour below when the key sorts below that, the key when it falls between the two, else what it held.
  POINTOPS_LIST_HD void insert(uint64_t key) {
    if (!(key < top[KC - 1])) return;
#if defined(__HIPCC__) || defined(__HIP__)
#pragma unroll
#endif
    for (int t = KC - 1; t > 0; --t) {
      const uint64_t lo = key < top[t] ? key : top[t];
      top[t] = top[t - 1] > lo ? top[t - 1] : lo;
    }
    top[0] = key < top[0] ? key : top[0];
  }
};

}  // namespace pointops

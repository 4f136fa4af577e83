// mfma16.h -- the 16-deep matrix instructions v_mfma_f32_32x32x16_bf16 / _f16 behind one name, for the 16-bit kernels
// (neighbor_conv16.hip, neighbor_mlp16.hip).  T is __bf16 or _Float16; V is eight of them, one 16-byte load.
// Lane (c = lane & 31, h = lane >> 5) holds, for BOTH operands, the k-values 16 s + 8 h + [0, 8) of step s (row c of A,
// column c of B), and accumulator element r is row (r & 3) + 8 (r >> 2) + 4 h of column c.
#pragma once
#include "common.h"

namespace pointops {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <class T>
struct Nc16;
template <>
struct Nc16<__bf16> {
  typedef bf16x8 V;
  static __device__ __forceinline__ f32x16 mfma(V a, V b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Nc16<_Float16> {
  typedef f16x8 V;
  static __device__ __forceinline__ f32x16 mfma(V a, V b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

template <class T>
__device__ __forceinline__ typename Nc16<T>::V nc16_zero() {
  typename Nc16<T>::V z;
#pragma unroll
  for (int x = 0; x < 8; ++x) z[x] = (T)0.0f;
  return z;
}

}  // namespace pointops

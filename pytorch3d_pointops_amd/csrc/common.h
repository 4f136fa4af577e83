// common.h -- shared host/device helpers for libpointops_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/pointops_amd.h"
#include "dispatch.h"

// Parity rule: every distance is an UNFUSED fp32
// multiply followed by an add.  hipcc's default -ffp-contract=fast would fuse
// them into v_fma/v_fmac and change the last bit, hence this pragma in every
// translation unit (the build also passes -ffp-contract=off).
#pragma clang fp contract(off)

namespace pointops {

constexpr int kWave = 64;  // CDNA wavefront width

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return POINTOPS_ELAUNCH;
  }
  return POINTOPS_OK;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the rows of cloud n that count: P without `lengths`, else lengths[n] clamped to [0, P] (T: the caller's index width)
template <class T = int>
__device__ __forceinline__ T clamped_length(const int64_t* __restrict__ lengths, int n, int P) {
  if (lengths == nullptr) return P;
  const int64_t l = lengths[n];
  return (T)(l < 0 ? 0 : (l > P ? P : l));
}
// len[n] = clamped_length(lengths, n, P) for the N clouds, on `stream` (radius_walk.hip): for the operators whose every
// pass reads the lengths, and whose grid_build needs them as an array
void clamp_lengths_async(const int64_t* lengths, int64_t N, int64_t P, int64_t* len, hipStream_t stream);

// Lays a workspace out as consecutive 256-byte aligned arrays.  With a null base it only sizes (take() returns null):
// one layout function serves both an operator's *_workspace_bytes query and its entry.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  char* take(size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  }
};

// a caller's workspace of `bytes` holds a layout of `need` bytes (null only when nothing is needed)
inline bool workspace_fits(const void* ws, size_t bytes, size_t need) {
  return bytes >= need && (ws != nullptr || need == 0);
}

}  // namespace pointops

#define POINTOPS_REQUIRE(cond, ...)        \
  do {                                     \
    if (!(cond)) {                         \
      pointops::set_error(__VA_ARGS__);    \
      return POINTOPS_EINVAL;              \
    }                                      \
  } while (0)

// the same for a caller's workspace (workspace_fits): the header's code for "workspace too small"
#define POINTOPS_REQUIRE_WORKSPACE(cond, ...) \
  do {                                        \
    if (!(cond)) {                            \
      pointops::set_error(__VA_ARGS__);       \
      return POINTOPS_EWORKSPACE;             \
    }                                         \
  } while (0)

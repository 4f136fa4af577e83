// zero_fill.hip -- stream-ordered zeroing of device buffers (zero_fill.h).
#include "zero_fill.h"

namespace pointops {

constexpr int kZeroBlock = 256;
constexpr int64_t kZeroMaxBlocks = 4096;

// 16-byte stores where the buffer allows them (base 16-byte aligned, whole uint4s), 4-byte stores otherwise
template <typename T>
__global__ __launch_bounds__(kZeroBlock) void zero_fill_kernel(T* __restrict__ p, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * kZeroBlock;
  for (int64_t i = (int64_t)blockIdx.x * kZeroBlock + threadIdx.x; i < n; i += stride) p[i] = T{};
}

int zero_words_async(void* p, int64_t words, hipStream_t stream, const char* what) {
  if (words <= 0) return POINTOPS_OK;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && (words & 3) == 0) {
    const int64_t n = words / 4;
    const int64_t blocks = ceil_div(n, kZeroBlock) < kZeroMaxBlocks ? ceil_div(n, kZeroBlock) : kZeroMaxBlocks;
    hipLaunchKernelGGL(zero_fill_kernel<uint4>, dim3((unsigned)blocks), dim3(kZeroBlock), 0, stream, (uint4*)p, n);
  } else {
    const int64_t blocks = ceil_div(words, kZeroBlock) < kZeroMaxBlocks ? ceil_div(words, kZeroBlock) : kZeroMaxBlocks;
    hipLaunchKernelGGL(zero_fill_kernel<uint32_t>, dim3((unsigned)blocks), dim3(kZeroBlock), 0, stream, (uint32_t*)p,
                       words);
  }
  return check_launch(what);
}

}  // namespace pointops

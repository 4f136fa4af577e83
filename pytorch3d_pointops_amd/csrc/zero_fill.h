// zero_fill.h -- stream-ordered zeroing of device buffers with a kernel.
//
// Not hipMemsetAsync: every launch of this library may be captured into a HIP graph (graphs.py), and a captured
// memset node stops writing zeros from the graph's second launch on (ROCm 7.0, MI355X: the first three quarters of
// the buffer receive a repeated 16-byte record that holds the buffer's own address, the last quarter is not written).
// Kernel nodes replay correctly.
#pragma once
#include "common.h"

namespace pointops {

// Zeroes `words` 32-bit words at `p` (4-byte aligned) on `stream`; `what` names the caller in the error string.
int zero_words_async(void* p, int64_t words, hipStream_t stream, const char* what);

}  // namespace pointops

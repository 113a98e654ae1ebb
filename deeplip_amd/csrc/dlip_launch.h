// Launch-side helpers shared by the element-wise files (host code).
#pragma once
#include "dlip_common.h"

// Workgroups of 256 threads for a grid-stride pass over n items: ceil(n / 256) clamped to [1, cap].  The cap is the caller's: it
// differs per file (how many workgroups per CU its kernels want resident) and shows at the call.
inline unsigned dlip_grid1d(long long n, long long cap) {
  const long long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// float4 / 128-bit access needs this
inline bool dlip_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline hipStream_t dlip_hip_stream(dlip_stream_t stream) { return static_cast<hipStream_t>(stream); }

// Launch-side helpers shared by the element-wise files (host code).
#pragma once
#include "dlip_common.h"

// Workgroups of 256 threads for a grid-stride pass over n items: ceil(n / 256) clamped to [1, cap].  The cap is the caller's: it
// differs per file (how many workgroups per CU its kernels want resident) and shows at the call.
inline unsigned dlip_grid1d(long long n, long long cap) {
  const long long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Every one of the pointers is a multiple of BYTES (a power of two).  A null pointer is aligned: whether it may be null is the caller's
// own condition.
template <unsigned BYTES, class... P>
inline bool dlip_aligned(const P*... p) {
  static_assert(BYTES > 0 && (BYTES & (BYTES - 1)) == 0, "a power of two");
  return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & (BYTES - 1)) == 0;
}
// float4 / 128-bit access needs the first; the split-format images (whole 128-byte blocks of 32 hi | 32 lo halves) the second
template <class... P>
inline bool dlip_aligned16(const P*... p) { return dlip_aligned<16>(p...); }
template <class... P>
inline bool dlip_aligned128(const P*... p) { return dlip_aligned<128>(p...); }

inline hipStream_t dlip_hip_stream(dlip_stream_t stream) { return static_cast<hipStream_t>(stream); }

// keep_power of the reverberation routes (wave_augment_ops.hip): y *= sqrt(Px / Py) per reverberated row, the sums taken per
// DLIP_FIR_TILE tile in the FIR kernel's order; `part` holds two doubles per (row, tile).  Called by wave_reverb_fft_ops.hip.
__attribute__((visibility("hidden"))) void dlip_wave_reverb_keep_power(const float* x, const int32_t* lengths, const int32_t* rir_idx,
                                                                       float* y, double* part, int B, int S, hipStream_t stream);

// Ragged batches through stride-2 stages (the ResNet speech encoder): utterance frames valid on a W-frame time axis that `shift`
// stride-2 convolutions (kernel 3, padding 1: L -> (L - 1) / 2 + 1) stand in front of, from the INPUT length `len` -- clamped to
// [1, W << shift], so the result lies in [1, W] whatever the vector holds.  Device code of layout_ops / pool_ops.
__host__ __device__ __forceinline__ int dlip_time_valid(int len, int shift, int W) {
  const long long cap = (long long)W << shift;
  const long long l = len < 1 ? 1 : (len > cap ? cap : (long long)len);
  return (int)((l - 1) >> shift) + 1;
}

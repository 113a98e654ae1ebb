// Wave and workgroup reductions shared by the element-wise and loss kernels.  dlip_wave_sum / dlip_wave_sum_f64 live in
// dlip_common.h (a source of the dominant kernel's translation unit, which this header must not touch); the rest is here.
// Every butterfly runs over the full 64-lane wave in the order 32, 16, .., 1: all lanes end with the same value.
#pragma once
#include "dlip_common.h"

__device__ __forceinline__ int dlip_wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float dlip_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ unsigned dlip_wave_max(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off, 64));
  return v;
}

// Sum over a workgroup of FOUR waves (256 threads, all of them call): butterflies within a wave, then the four wave totals meet in
// red[4] and every thread returns ((r0 + r1) + r2) + r3 -- wave order, the same bits on every run.  It ENDS AFTER THE READ of
// red[]: a caller that writes red[] (or anything else these barriers are meant to close) again puts its own __syncthreads() behind.
template <typename T>
__device__ __forceinline__ T dlip_block_meet4(T wave_total, T* red) {
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double dlip_block_sum4(double v, double* red) { return dlip_block_meet4(dlip_wave_sum_f64(v), red); }
__device__ __forceinline__ int dlip_block_sum4(int v, int* red) { return dlip_block_meet4(dlip_wave_sum_i32(v), red); }
// The same meeting for a maximum (exact in any order).
__device__ __forceinline__ float dlip_block_max4(float v, float* red) {
  v = dlip_wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

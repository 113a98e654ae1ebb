// Statistics pooling of the ResNet speech encoder (deeplip_amd/audio_resnet.py, `pooling: statistic | attentive_statistic`) on its
// channels-last map [N,H,W,C] (H = frequency, W = time): per (h, c) the mean and the eps-floored unbiased standard deviation over
// the utterance's valid frames, read straight from the map; the backward; the [N,H,W,C] <-> [N,W,H,C] copy in front of the attentive
// pooling's GEMM; the valid frame counts of a ragged batch.  HBM-bound: one float4 of channels per lane, fp64 sums in a fixed
// order, no atomics.
#include "dlip_launch.h"

namespace {

// y[n, h C + c] = mean_{w < Wb} x[n,h,w,c];  y[n, H C + h C + c] = sqrt( sum_{w < Wb} (x - mean)^2 / (Wb - 1) + eps )
// One workgroup per (utterance, h, 64-channel block), as meanstd_kernel (pool_ops.hip): 16 lanes x float4 span the block, 16 frame
// groups split Wb (each ascending), sums and sums of squares in fp64 (the inputs are fp32, so sum x^2 - (sum x)^2 / Wb loses nothing a
// two-pass fp32 result has), the 16 partial rows meet in LDS in a fixed order.  Wb = dlip_time_valid(len[n], shift, W), or W without
// `len`; the frames w >= Wb are never loaded.  The map's last operation is a ReLU: a feature that is constant over time (zero, most
// often) is ordinary there, and eps > 0 under the root keeps its std -- and the backward's divisor -- away from zero.  Wb == 1
// (a device length vector only: host lengths are validated) gives std = sqrt(eps), not NaN.
__global__ __launch_bounds__(256) void statpool_nhwc_kernel(const float* __restrict__ x, const int32_t* __restrict__ len, int shift,
                                                            float eps, float* __restrict__ y, int H, int W, int C) {
  __shared__ double part[16][64][2];
  const int n = blockIdx.z, h = blockIdx.y, c0 = blockIdx.x * 64;
  const int Wb = len != nullptr ? dlip_time_valid(len[n], shift, W) : W;
  const int lx = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = c0 + lx * 4;
  double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
  if (c < C) {   // C % 4 == 0: a float4 is all inside or all outside
    const float* p = x + (((long long)n * H + h) * W) * C + c;
    for (int t = g; t < Wb; t += 16) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + (long long)t * C);
#pragma unroll
      for (int k = 0; k < 4; ++k) { s[k] += (double)v[k]; q[k] += (double)v[k] * (double)v[k]; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { part[g][lx * 4 + k][0] = s[k]; part[g][lx * 4 + k][1] = q[k]; }
  __syncthreads();
  if (threadIdx.x < 64 && c0 + (int)threadIdx.x < C) {
    double ss = 0.0, qq = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) { ss += part[i][threadIdx.x][0]; qq += part[i][threadIdx.x][1]; }
    const double mean = ss / (double)Wb;
    double var = Wb > 1 ? (qq - ss * mean) / (double)(Wb - 1) : 0.0;
    if (var < 0.0) var = 0.0;
    const long long D = (long long)H * C;
    float* yn = y + (long long)n * 2 * D + (long long)h * C + c0 + threadIdx.x;
    yn[0] = (float)mean;
    yn[D] = (float)sqrt(var + (double)eps);
  }
}

// dx[n,h,w,c] = dmean / W + dstd (x - mean) / ((W - 1) std), mean and std read from y (std >= sqrt(eps) > 0: no 0/0 at a feature that
// is constant over time).  Element-wise, one float4 per thread, every element of dx written; the coefficient arithmetic in fp64.
__global__ __launch_bounds__(256) void statpool_nhwc_bwd_kernel(const f32x4* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ dy, f32x4* __restrict__ dx, long long total,
                                                                int H, int W, int C4) {
  const long long D = (long long)H * C4 * 4;
  const double inv_w = 1.0 / (double)W, inv_w1 = 1.0 / (double)(W - 1);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    const long long r = i / C4 / W;      // n H + h
    const int h = (int)(r % H);
    const long long o = (r / H) * 2 * D + ((long long)h * C4 + c4) * 4;
    const f32x4 mean = *reinterpret_cast<const f32x4*>(y + o), sd = *reinterpret_cast<const f32x4*>(y + o + D);
    const f32x4 dm = *reinterpret_cast<const f32x4*>(dy + o), ds = *reinterpret_cast<const f32x4*>(dy + o + D);
    const f32x4 v = x[i];
    f32x4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      out[k] = (float)((double)dm[k] * inv_w + (double)ds[k] * ((double)v[k] - (double)mean[k]) * inv_w1 / (double)sd[k]);
    dx[i] = out;
  }
}

// y[n, b, a, :] = x[n, a, b, :]  (float4 of channels per thread; reads and writes are both whole C-rows)
__global__ __launch_bounds__(256) void swap_axes_nhwc_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ y, long long total, int A,
                                                             int B, int C4) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    long long p = i / C4;
    const int a = (int)(p % A); p /= A;
    const int b = (int)(p % B);
    const long long n = p / B;
    y[i] = x[((n * A + a) * B + b) * C4 + c4];
  }
}

__global__ __launch_bounds__(256) void time_valid_lengths_kernel(const int32_t* __restrict__ len, int shift, int W,
                                                                 int32_t* __restrict__ out, int N) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n < N) out[n] = dlip_time_valid(len[n], shift, W);
}

constexpr int kGridCap = 256 * 8;  // 8 workgroups per CU, grid-stride the rest

}  // namespace

extern "C" int dlip_statpool_nhwc_f32(const float* x, const int32_t* lengths, int32_t shift, float eps, float* y, int32_t N, int32_t H,
                                      int32_t W, int32_t C, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && N > 0 && N <= 65535 && H > 0 && H <= 65535 && W > 0 && C > 0 && (C & 3) == 0);
  DLIP_CHECK_ARG(shift >= 0 && shift <= 16 && W <= (0x7fffffff >> shift) && eps > 0.f);
  DLIP_CHECK_ARG(dlip_aligned16(x));
  hipLaunchKernelGGL(statpool_nhwc_kernel, dim3((C + 63) / 64, H, N), dim3(256), 0, dlip_hip_stream(stream), x, lengths, shift, eps, y,
                     H, W, C);
  return dlip_launch_status();
}

extern "C" int dlip_statpool_nhwc_bwd_f32(const float* x, const float* y, const float* dy, float eps, float* dx, int32_t N, int32_t H,
                                          int32_t W, int32_t C, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && dy && dx && N > 0 && H > 0 && W > 1 && C > 0 && (C & 3) == 0);
  DLIP_CHECK_ARG(eps > 0.f);   // what keeps the std read from y away from zero: the entry point has no eps = 0 form
  DLIP_CHECK_ARG(dlip_aligned16(x, y, dy, dx));
  const long long total = (long long)N * H * W * (C / 4);
  hipLaunchKernelGGL(statpool_nhwc_bwd_kernel, dim3(dlip_grid1d(total, kGridCap)), dim3(256), 0, dlip_hip_stream(stream),
                     reinterpret_cast<const f32x4*>(x), y, dy, reinterpret_cast<f32x4*>(dx), total, H, W, C / 4);
  return dlip_launch_status();
}

extern "C" int dlip_swap_axes_nhwc_f32(const float* x, float* y, int32_t N, int32_t A, int32_t B, int32_t C, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && x != y && N > 0 && A > 0 && B > 0 && C > 0 && (C & 3) == 0);
  DLIP_CHECK_ARG(dlip_aligned16(x, y));
  const long long total = (long long)N * A * B * (C / 4);
  hipLaunchKernelGGL(swap_axes_nhwc_kernel, dim3(dlip_grid1d(total, kGridCap)), dim3(256), 0, dlip_hip_stream(stream),
                     reinterpret_cast<const f32x4*>(x), reinterpret_cast<f32x4*>(y), total, A, B, C / 4);
  return dlip_launch_status();
}

extern "C" int dlip_time_valid_lengths_i32(const int32_t* lengths, int32_t shift, int32_t W, int32_t* valid, int32_t N,
                                           dlip_stream_t stream) {
  DLIP_CHECK_ARG(lengths && valid && N > 0 && W > 0 && shift >= 0 && shift <= 16 && W <= (0x7fffffff >> shift));
  hipLaunchKernelGGL(time_valid_lengths_kernel, dim3((N + 255) / 256), dim3(256), 0, dlip_hip_stream(stream), lengths, shift, W, valid,
                     N);
  return dlip_launch_status();
}

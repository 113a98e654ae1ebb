// HBM-bound reductions on channels-last activations: max-pool, global average pool, (masked)
// temporal mean, clip-group mean, mean + unbiased-std statistics pooling.  One thread owns one
// channel (or a float4 of channels) so every wave access is a contiguous 256 B - 1 KiB segment;
// statistics accumulate in fp64 (torch's CPU reductions accumulate float inputs in double).
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

// MaxPool3d((1,3,3), s(1,2,2), p(0,1,1)) == per-frame MaxPool2d(3, 2, 1); padding never wins.
template <bool OSPLIT>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ y,
                                                           int N, int H, int W, int C4, int Ho, int Wo, DlipRange status) {
  const long long total = (long long)N * Ho * Wo * C4;
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C4);
    long long p = i / C4;
    const int wo = (int)(p % Wo); p /= Wo;
    const int ho = (int)(p % Ho);
    const int n = (int)(p / Ho);
    const float ninf = -__builtin_inff();
    f32x4 m = {ninf, ninf, ninf, ninf};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int hi = 2 * ho - 1 + r;
      if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int wi = 2 * wo - 1 + s;
        if ((unsigned)wi >= (unsigned)W) continue;
        const f32x4 v = x[((long long)(n * H + hi) * W + wi) * C4 + c];
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
      }
    }
    if constexpr (OSPLIT) {   // (hi, lo) fp16 pairs per 32-channel block for the split-fp16 conv kernels
      typedef _Float16 h4 __attribute__((ext_vector_type(4)));
      h4 hi, lo;
#pragma unroll
      for (int k = 0; k < 4; ++k) { hi[k] = (_Float16)m[k]; lo[k] = (_Float16)(m[k] - (float)hi[k]); amax = fmaxf(amax, fabsf(m[k])); }
      float* b = reinterpret_cast<float*>(y) + (i >> 3) * 32;
      const int q = (int)(i & 7);
      *reinterpret_cast<h4*>(b + q * 2) = hi;
      *reinterpret_cast<h4*>(b + 16 + q * 2) = lo;
    } else {
      y[i] = m;
    }
  }
  if constexpr (OSPLIT) dlip_report_range_block(amax, status);
}

// y[n,c] = mean over hw of x[n,hw,c]   (sequential fp32 sum, then one divide: AdaptiveAvgPool2d(1))
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                      int N, int HW, int C) {
  const long long total = (long long)N * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long long n = i / C;
    const float* p = x + n * HW * C + c;
    float s = 0.f;
    for (int h = 0; h < HW; ++h) s += p[(long long)h * C];
    y[i] = s / (float)HW;
  }
}

__global__ __launch_bounds__(256) void time_mean_kernel(const float* __restrict__ x, const DlipLen len,
                                                        float* __restrict__ y, int B, int T, int C, int ldx) {
  const long long total = (long long)B * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int b = (int)(i / C);
    const int L = dlip_valid_rows(len, b, T);
    const float* p = x + (long long)b * T * ldx + c;
    double s = 0.0;
    for (int t = 0; t < L; ++t) s += (double)p[(long long)t * ldx];
    y[i] = (float)(s / (double)L);
  }
}

__global__ __launch_bounds__(256) void group_mean_kernel(const float* __restrict__ x, const int32_t* __restrict__ ptr,
                                                         float* __restrict__ y, int U, int C) {
  const long long total = (long long)U * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int u = (int)(i / C);
    const int g0 = ptr[u], g1 = ptr[u + 1];
    float s = 0.f;  // the reference accumulates the clip means in fp32 (`em += ...`, train_fusion.py:274)
    for (int g = g0; g < g1; ++g) s += x[(long long)g * C + c];
    y[i] = s / (float)(g1 - g0);
  }
}

// y[b, c] = mean_t x[b,t,c];  y[b, C + c] = sqrt( sum_t (x - mean)^2 / (T - 1) )
// One workgroup per (utterance, 64-channel block): 16 lanes x float4 span the block, 16 row groups
// split T, so every thread streams T/16 independent 16-B loads; sums and sums of squares are kept
// in fp64 (the inputs are fp32, so sum x^2 - (sum x)^2 / T loses nothing a two-pass fp32 result has)
// and the 16 partial rows meet in LDS.  SPLIT writes the [B, ldy] result as (hi, lo) fp16 pairs (the
// split activation format; ldy = 2C rounded up to 32, padding zeroed) for the LDS-DMA GEMM behind it.
// `len` (ragged batches: utterance b is valid for its first len[b] + len_add of the T frames, the rest is padding): the
// statistics cover the valid frames only, as the reference's one-utterance-at-a-time loop computes them (train_fusion.py:334-338).
// (ABI 48) BN: x is the RAW output z of the last TDNN convolution and every loaded value becomes lrelu((z - mean) invstd gamma + beta, slope)
// first (bn_fwd_apply_kernel's expression: the same bits) -- the train-mode BatchNorm + LeakyReLU in front of the pooling, whose activated
// tensor ([B,T,1500]: 460 MB at B = 256) is then never stored.
struct PoolBn {
  const float* mean = nullptr;
  const float* invstd = nullptr;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  float slope = 1.f;
};
template <bool SPLIT, bool BN = false>
__global__ __launch_bounds__(256) void meanstd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                      int Tpad, int C, int ldy, const DlipLen len, DlipRange status, const PoolBn bn = PoolBn{}) {
  __shared__ double part[16][64][2];
  const int b = blockIdx.y, c0 = blockIdx.x * 64;
  const int T = dlip_valid_rows(len, b, Tpad);
  const int lx = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = c0 + lx * 4;
  float amax = 0.f;
  double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
  if (c < C) {   // C % 4 == 0: a float4 is all inside or all outside
    const float* p = x + (long long)b * Tpad * C + c;
    f32x4 mu = {0, 0, 0, 0}, is = mu, ga = mu, be = mu;
    if constexpr (BN) {
      mu = *reinterpret_cast<const f32x4*>(bn.mean + c); is = *reinterpret_cast<const f32x4*>(bn.invstd + c);
      ga = *reinterpret_cast<const f32x4*>(bn.gamma + c); be = *reinterpret_cast<const f32x4*>(bn.beta + c);
    }
    for (int t = g; t < T; t += 16) {
      f32x4 v = *reinterpret_cast<const f32x4*>(p + (long long)t * C);
      if constexpr (BN) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float u = (v[k] - mu[k]) * is[k] * ga[k] + be[k];
          v[k] = u >= 0.f ? u : u * bn.slope;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) { s[k] += (double)v[k]; q[k] += (double)v[k] * (double)v[k]; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { part[g][lx * 4 + k][0] = s[k]; part[g][lx * 4 + k][1] = q[k]; }
  __syncthreads();
  if (threadIdx.x < 64 && c0 + (int)threadIdx.x < C) {
    const int cc = c0 + threadIdx.x;
    double ss = 0.0, qq = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) { ss += part[i][threadIdx.x][0]; qq += part[i][threadIdx.x][1]; }
    const double mean = ss / (double)T;
    double var = (qq - ss * mean) / (double)(T - 1);   // T == 1 -> NaN, as torch.std
    if (var < 0.0) var = 0.0;
    const float out[2] = {(float)mean, (float)sqrt(var)};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int col = h * C + cc;
      if (SPLIT) {
        const _Float16 hi = (_Float16)out[h], lo = (_Float16)(out[h] - (float)hi);
        _Float16* blk = reinterpret_cast<_Float16*>(y + (long long)b * ldy + (col & ~31));
        blk[col & 31] = hi;
        blk[32 + (col & 31)] = lo;
        amax = fmaxf(amax, fabsf(out[h]));
        if (!(fabsf(out[h]) < DLIP_F16_OVERFLOW)) amax = __builtin_inff();   // (a NaN too: fmaxf would drop it)
      } else {
        y[(long long)b * ldy + col] = out[h];
      }
    }
  }
  if (SPLIT && blockIdx.x == 0 && (int)threadIdx.x < ldy - 2 * C) {   // zero the channel padding (< 32 values)
    const int col = 2 * C + threadIdx.x;
    _Float16* blk = reinterpret_cast<_Float16*>(y + (long long)b * ldy + (col & ~31));
    blk[col & 31] = (_Float16)0.f;
    blk[32 + (col & 31)] = (_Float16)0.f;
  }
  if (SPLIT) dlip_report_range(amax, status);
}

// y[n, c] = mean over h < H, w < Lk of x[n, h, w, c], Lk = dlip_time_valid(len[n], shift, W): AdaptiveAvgPool2d(1) of utterance n
// alone, taken from its row of a zero-padded batch (divisor H Lk, not H W).  One workgroup per (utterance, 64-channel block) as
// meanstd_kernel: 16 lanes x float4 span the block, 16 position groups split the H Lk valid positions (ascending), fp64 sums, the
// 16 partial rows meet in LDS in a fixed order -- no atomics, the same bits on every run.
__global__ __launch_bounds__(256) void avgpool_time_ragged_kernel(const float* __restrict__ x, const int32_t* __restrict__ len,
                                                                  int shift, float* __restrict__ y, int H, int W, int C) {
  __shared__ double part[16][64];
  const int n = blockIdx.y, c0 = blockIdx.x * 64;
  const int Lk = dlip_time_valid(len[n], shift, W);
  const int lx = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = c0 + lx * 4;
  double s[4] = {0, 0, 0, 0};
  if (c < C) {   // C % 4 == 0: a float4 is all inside or all outside
    const float* p = x + (long long)n * H * W * C + c;
    const int P = H * Lk;
    for (int i = g; i < P; i += 16) {
      const int h = i / Lk, w = i - h * Lk;
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + ((long long)h * W + w) * C);
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += (double)v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) part[g][lx * 4 + k] = s[k];
  __syncthreads();
  if (threadIdx.x < 64 && c0 + (int)threadIdx.x < C) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) ss += part[i][threadIdx.x];
    y[(long long)n * C + c0 + threadIdx.x] = (float)(ss / ((double)H * (double)Lk));
  }
}

constexpr int kGridCap = 256 * 8;  // 8 workgroups per CU, grid-stride the rest

}  // namespace

extern "C" int dlip_maxpool3x3s2_nhwc_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C,
                                          int32_t out_split, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && (!out_split || (C & 31) == 0));
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const long long total = (long long)N * Ho * Wo * (C / 4);
  if (out_split)
    hipLaunchKernelGGL(maxpool3x3s2_kernel<true>, dim3(dlip_grid1d(total, kGridCap)), dim3(256), 0, dlip_hip_stream(stream),
                       reinterpret_cast<const f32x4*>(x), reinterpret_cast<f32x4*>(y), N, H, W, C / 4, Ho, Wo,
                       dlip_range_for(DLIP_ST_PACK));
  else
    hipLaunchKernelGGL(maxpool3x3s2_kernel<false>, dim3(dlip_grid1d(total, kGridCap)), dim3(256), 0, dlip_hip_stream(stream),
                       reinterpret_cast<const f32x4*>(x), reinterpret_cast<f32x4*>(y), N, H, W, C / 4, Ho, Wo, DlipRange{});
  return dlip_launch_status();
}

extern "C" int dlip_avgpool_nhwc_f32(const float* x, float* y, int32_t N, int32_t HW, int32_t C,
                                     dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && N > 0 && HW > 0 && C > 0);
  hipLaunchKernelGGL(avgpool_kernel, dim3(dlip_grid1d((long long)N * C, kGridCap)), dim3(256), 0,
                     dlip_hip_stream(stream), x, y, N, HW, C);
  return dlip_launch_status();
}

extern "C" int dlip_time_mean_f32(const float* x, const int32_t* len, int32_t len_add, float* y, int32_t B, int32_t T, int32_t C,
                                  int32_t ldx, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && B > 0 && T > 0 && C > 0 && ldx >= C);
  DlipLen l; l.len = len; l.mul = 1; l.add = len_add;
  hipLaunchKernelGGL(time_mean_kernel, dim3(dlip_grid1d((long long)B * C, kGridCap)), dim3(256), 0,
                     dlip_hip_stream(stream), x, l, y, B, T, C, ldx);
  return dlip_launch_status();
}

extern "C" int dlip_avgpool_time_ragged_f32(const float* x, const int32_t* lengths, int32_t shift, float* y, int32_t N, int32_t H,
                                            int32_t W, int32_t C, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && lengths && y && N > 0 && N <= 65535 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && shift >= 0 && shift <= 16);
  DLIP_CHECK_ARG((long long)H * W <= 0x7fffffffLL && W <= (0x7fffffff >> shift));
  DLIP_CHECK_ARG(dlip_aligned16(x));
  hipLaunchKernelGGL(avgpool_time_ragged_kernel, dim3((C + 63) / 64, N), dim3(256), 0, dlip_hip_stream(stream), x, lengths, shift, y,
                     H, W, C);
  return dlip_launch_status();
}

extern "C" int dlip_group_mean_f32(const float* x, const int32_t* group_ptr, float* y, int32_t U, int32_t C,
                                   dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && group_ptr && y && U > 0 && C > 0);
  hipLaunchKernelGGL(group_mean_kernel, dim3(dlip_grid1d((long long)U * C, kGridCap)), dim3(256), 0,
                     dlip_hip_stream(stream), x, group_ptr, y, U, C);
  return dlip_launch_status();
}

extern "C" int dlip_meanstd_pool_f32(const float* x, const int32_t* len, int32_t len_add, float* y, int32_t B, int32_t T, int32_t C,
                                     int32_t out_split, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && B > 0 && B <= 65535 && T > 0 && C > 0 && (C & 3) == 0);
  DLIP_CHECK_ARG(dlip_aligned16(x));
  const dim3 grid((C + 63) / 64, B);
  DlipLen l; l.len = len; l.mul = 1; l.add = len_add;
  if (out_split)
    hipLaunchKernelGGL(meanstd_kernel<true>, grid, dim3(256), 0, dlip_hip_stream(stream), x, y, T, C,
                       (2 * C + 31) / 32 * 32, l, dlip_range_for(DLIP_ST_POOL));
  else
    hipLaunchKernelGGL(meanstd_kernel<false>, grid, dim3(256), 0, dlip_hip_stream(stream), x, y, T, C, 2 * C, l,
                       DlipRange{});
  return dlip_launch_status();
}

extern "C" int dlip_meanstd_pool_bn_f32(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                        float slope, float* y, int32_t B, int32_t T, int32_t C, dlip_stream_t stream) {
  DLIP_CHECK_ARG(z && mean && invstd && gamma && beta && y && B > 0 && B <= 65535 && T > 0 && C > 0 && (C & 3) == 0);
  DLIP_CHECK_ARG(dlip_aligned16(z));
  DlipLen l; l.len = nullptr; l.mul = 1; l.add = 0;
  PoolBn bn; bn.mean = mean; bn.invstd = invstd; bn.gamma = gamma; bn.beta = beta; bn.slope = slope;
  hipLaunchKernelGGL((meanstd_kernel<false, true>), dim3((C + 63) / 64, B), dim3(256), 0, dlip_hip_stream(stream), z, y, T, C, 2 * C, l,
                     DlipRange{}, bn);
  return dlip_launch_status();
}

namespace {
// Finisher of the pooled convolution epilogue (conv_igemm_f16x3_dma.hip, EPI 2): partials [tiles_m][4][Kp] fp64 =
// per tile the column sums {sum, sumsq} of the rows before the tile's group boundary (segment 0) and after it
// (segment 1).  Group g = rows [g Gs, (g+1) Gs) touches tiles g Gs / BM .. ((g+1) Gs - 1) / BM; in each it is
// segment 0 if the tile's first row belongs to g, else segment 1.  Tiles are added in row order.
template <int MODE, bool SPLIT>
__global__ __launch_bounds__(256) void pool_finish_kernel(const double* __restrict__ part, float* __restrict__ y, long long M,
                                                          int K, int Kp, int BM, int Gs, int G, int ldy, const DlipLen len,
                                                          DlipRange status) {
  const long long total = (long long)G * K;
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % K);
    const long long g = i / K;
    const long long r0 = g * Gs;
    long long r1 = r0 + Gs;
    if (r1 > M) r1 = M;
    double s = 0.0, q = 0.0;
    for (long long tm = r0 / BM; tm <= (r1 - 1) / BM; ++tm) {
      const int seg = (tm * BM) / Gs == g ? 0 : 1;
      const double* p = part + ((size_t)tm * 4 + 2 * seg) * Kp + k;
      s += p[0];
      q += p[Kp];
    }
    const double n = (double)dlip_valid_rows(len, g, (int)(r1 - r0));   // ragged: the epilogue summed the group's valid rows only
    const double mean = s / n;
    if (MODE == 0) {
      y[g * ldy + k] = (float)mean;
    } else {
      double var = (q - s * mean) / (n - 1.0);   // n == 1 -> NaN, as torch.std
      if (var < 0.0) var = 0.0;
      const float out[2] = {(float)mean, (float)sqrt(var)};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int col = h * K + k;
        if (SPLIT) {
          const _Float16 hi = (_Float16)out[h], lo = (_Float16)(out[h] - (float)hi);
          _Float16* blk = reinterpret_cast<_Float16*>(y + g * ldy + (col & ~31));
          blk[col & 31] = hi;
          blk[32 + (col & 31)] = lo;
          amax = fmaxf(amax, fabsf(out[h]));
        } else {
          y[g * ldy + col] = out[h];
        }
      }
    }
  }
  if (SPLIT) {
    const long long pad_total = (long long)G * (ldy - 2 * K);   // zero the channel padding (< 32 values per row)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pad_total; i += (long long)gridDim.x * 256) {
      const long long g = i / (ldy - 2 * K);
      const int col = 2 * K + (int)(i % (ldy - 2 * K));
      _Float16* blk = reinterpret_cast<_Float16*>(y + g * ldy + (col & ~31));
      blk[col & 31] = (_Float16)0.f;
      blk[32 + (col & 31)] = (_Float16)0.f;
    }
    dlip_report_range_block(amax, status);
  }
}
}  // namespace

extern "C" int dlip_pool_finish_f32(const double* partials, int64_t M, int32_t K, int32_t tile_rows, int32_t group_rows,
                                    const int32_t* group_len, int32_t len_mul, int32_t len_add,
                                    int32_t mode, int32_t out_split, float* y, dlip_stream_t stream) {
  DLIP_CHECK_ARG(partials && y && M > 0 && K > 0 && tile_rows > 0 && group_rows >= tile_rows && (mode == 0 || mode == 1));
  DLIP_CHECK_ARG(!(out_split && mode == 0));
  const int Kp = (K + 127) / 128 * 128;   // the pooled epilogue exists on the 128-column tiles only
  const long long G = (M + group_rows - 1) / group_rows;
  DLIP_CHECK_ARG(G <= 0x7FFFFFFF);
  hipStream_t st = dlip_hip_stream(stream);
  const unsigned grid = dlip_grid1d(G * K, kGridCap);
  const DlipRange status = (mode == 1 && out_split) ? dlip_range_for(DLIP_ST_POOL) : DlipRange{};   // only a split output is a producer
  DlipLen l; l.len = group_len; l.mul = len_mul; l.add = len_add;
  if (mode == 0)
    hipLaunchKernelGGL((pool_finish_kernel<0, false>), dim3(grid), dim3(256), 0, st, partials, y, (long long)M, K, Kp, tile_rows,
                       group_rows, (int)G, K, l, status);
  else if (out_split)
    hipLaunchKernelGGL((pool_finish_kernel<1, true>), dim3(grid), dim3(256), 0, st, partials, y, (long long)M, K, Kp, tile_rows,
                       group_rows, (int)G, (2 * K + 31) / 32 * 32, l, status);
  else
    hipLaunchKernelGGL((pool_finish_kernel<1, false>), dim3(grid), dim3(256), 0, st, partials, y, (long long)M, K, Kp, tile_rows,
                       group_rows, (int)G, 2 * K, l, status);
  return dlip_launch_status();
}

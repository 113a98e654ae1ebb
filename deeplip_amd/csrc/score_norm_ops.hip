// Cohort score normalisation (Z-/T-/S-norm and adaptive S-norm) behind the trial scoring of score_ops.hip.
//   topk_stats_kernel : per row of a score matrix, mean and population deviation of its K largest values -- exact selection
//                       (radix select over order-preserving keys held in LDS), fp64 statistics, one rounding to fp32.
//   score_norm_kernel : per trial, (s - mu) / max(sd, eps) through the trial's two utterance indices.
// One 256-thread workgroup owns a row: the row is read from HBM once and everything else happens on the LDS copy.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int TOPK_MAX_N = 32768;   // 128 KiB of keys + the histogram fit the 160 KiB of a CU

// float -> uint32 whose unsigned order is the float order (-0.0 just below +0.0; NaNs at the two ends: still a total order)
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__global__ __launch_bounds__(256) void topk_stats_kernel(const float* __restrict__ s, int N, long long ld, int K,
                                                         float* __restrict__ mean, float* __restrict__ sd) {
  extern __shared__ uint32_t keys[];          // [N]
  __shared__ int hist[256];
  __shared__ int wave_tot[4];
  __shared__ int pick[2];                     // the bin that holds the K-th largest key, and the rank left inside it
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = s + (long long)blockIdx.x * ld;
  for (int i = tid; i < N; i += 256) keys[i] = key_of(row[i]);

  // Radix select, most significant byte first: after the four passes `prefix` is the K-th largest key T and `want` the number
  // of copies of T that belong to the top K (K minus the count of keys above T).  K == N takes the whole row: nothing to select.
  uint32_t prefix = 0, mask = 0;
  int want = K;
  const bool all = K == N;
  for (int shift = 24; shift >= 0 && !all; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();                          // also orders the key writes above before the first pass reads them
    for (int i = tid; i < N; i += 256) {
      const uint32_t k = keys[i];
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1);
    }
    __syncthreads();
    // thread t looks at bin 255 - t: an inclusive scan over t counts the candidates in that bin and every bin above it
    const int c = hist[255 - tid];
    int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += wave_tot[w];
    if (incl - c < want && want <= incl) {    // exactly one thread: the counts are non-decreasing and end at >= want
      pick[0] = 255 - tid;
      pick[1] = want - (incl - c);
    }
    __syncthreads();
    prefix |= (uint32_t)pick[0] << shift;
    mask |= 255u << shift;
    want = pick[1];
    // the next pass zeroes hist[] and overwrites pick[] only behind its own barriers; wave_tot is rewritten behind two of them
  }
  if (all) {
    want = 0;
    __syncthreads();
  }
  const uint32_t T = prefix;
  const double vT = all ? 0.0 : (double)value_of(T);   // K == N: no threshold (key 0 is a NaN's), and no copies of it to add

  double acc = 0.0;
  for (int i = tid; i < N; i += 256) {
    const uint32_t k = keys[i];
    if (all || k > T) acc += (double)value_of(k);
  }
  double tot = dlip_block_sum4(acc, red) + (double)want * vT;
  const double mu = tot / (double)K;
  __syncthreads();                            // red[] is written again below
  acc = 0.0;
  for (int i = tid; i < N; i += 256) {
    const uint32_t k = keys[i];
    if (all || k > T) {
      const double d = (double)value_of(k) - mu;
      acc += d * d;
    }
  }
  const double q = dlip_block_sum4(acc, red) + (double)want * (vT - mu) * (vT - mu);
  if (tid == 0) {
    mean[blockIdx.x] = (float)mu;
    sd[blockIdx.x] = (float)sqrt(q / (double)K);
  }
}

__global__ __launch_bounds__(256) void score_norm_kernel(const float* __restrict__ s, const int32_t* __restrict__ ia,
                                                         const int32_t* __restrict__ ib, int n, const float* __restrict__ mu,
                                                         const float* __restrict__ sd, int U, int mode, float eps, float weight,
                                                         int accumulate, float* __restrict__ out) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int a = ia[i], b = ib[i];
    float r;
    if ((unsigned)a >= (unsigned)U || (unsigned)b >= (unsigned)U) {
      r = __builtin_nanf("");
    } else {
      const double v = (double)s[i];
      const double za = (v - (double)mu[a]) / (double)fmaxf(sd[a], eps);
      const double zb = (v - (double)mu[b]) / (double)fmaxf(sd[b], eps);
      const double z = mode == 0 ? za : (mode == 1 ? zb : 0.5 * (za + zb));
      r = (float)(accumulate ? (double)out[i] + (double)weight * z : (double)weight * z);
    }
    out[i] = r;
  }
}

}  // namespace

extern "C" int dlip_topk_stats_f32(const float* s, int32_t R, int32_t N, int64_t ld, int32_t K, float* mean, float* sd,
                                   dlip_stream_t stream) {
  DLIP_CHECK_ARG(s && mean && sd && R > 0);
  DLIP_CHECK_ARG(N >= 1 && N <= TOPK_MAX_N && K >= 1 && K <= N && ld >= (int64_t)N);
  const size_t lds = (size_t)N * sizeof(uint32_t);
  auto kern = topk_stats_kernel;
  static DlipKernelState ks;   // the dynamic-LDS limit is raised once per device and size
  if (lds > 48 * 1024) {
    const int e = ks.ensure_lds(reinterpret_cast<const void*>(kern), lds);
    if (e != DLIP_OK) return e;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)R), dim3(256), lds, dlip_hip_stream(stream), s, N, (long long)ld, K, mean, sd);
  return dlip_launch_status();
}

extern "C" int dlip_score_norm_f32(const float* s, const int32_t* idx_a, const int32_t* idx_b, int32_t n, const float* mu,
                                   const float* sd, int32_t U, int32_t mode, float eps, float weight, int32_t accumulate,
                                   float* out, dlip_stream_t stream) {
  DLIP_CHECK_ARG(s && idx_a && idx_b && mu && sd && out && n > 0 && U > 0 && mode >= 0 && mode <= 2);
  hipLaunchKernelGGL(score_norm_kernel, dim3(dlip_grid1d(n, 2048)), dim3(256), 0, dlip_hip_stream(stream), s, idx_a, idx_b, n, mu,
                     sd, U, mode, eps, weight, accumulate, out);
  return dlip_launch_status();
}

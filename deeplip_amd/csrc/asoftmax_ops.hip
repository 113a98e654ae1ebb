// A-Softmax (SphereFace, Liu et al. 2017) on cosine logits (ABI 66): `ASoftmax` is an empty stub upstream (models/audio_models/loss.py:53-59)
// that conf/audio_config.yaml:130 nevertheless lists, so the definition is the build's own:
//   z_bj = r_b c_bj (j != y_b),   z_by = r_b (lambda c + psi(c)) / (1 + lambda),   psi(c) = (-1)^k T_m(c) - 2k,
//   k = #{ j in 1 .. m-1 : c <= cos(j pi / m) },  c clamped to [-1, 1],  T_m the Chebyshev polynomial, m = 1 .. 4,
// r_b = max(|x_b|, eps) exactly as dlip_l2_normalize_f32 forms it.  lambda is READ FROM DEVICE MEMORY by both modes: a recorded step
// follows the annealing schedule without being recorded again.  psi is continuous and psi' = (-1)^k m U_{m-1}(c) vanishes at every
// branch point, so a k chosen differently by one rounding moves neither value nor gradient.  The target column (one element per row)
// is evaluated in fp64; every sum runs in a fixed order (no atomics): a replayed step equals the eager one bit for bit.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

struct ASoftmaxCuts { float c1, c2, c3; };      // cos(j pi / m), j = 1 .. m-1 (unused ones: -2, never reached by c in [-1, 1])

__device__ __forceinline__ int asoftmax_k(float c, const ASoftmaxCuts& cuts) {
  return (c <= cuts.c1 ? 1 : 0) + (c <= cuts.c2 ? 1 : 0) + (c <= cuts.c3 ? 1 : 0);
}

// T_m(c) and m U_{m-1}(c) = T_m'(c)
__device__ __forceinline__ double asoftmax_cheb(double c, int m) {
  const double c2 = c * c;
  return m == 1 ? c : (m == 2 ? 2.0 * c2 - 1.0 : (m == 3 ? (4.0 * c2 - 3.0) * c : (8.0 * c2 - 8.0) * c2 + 1.0));
}
__device__ __forceinline__ double asoftmax_cheb_d(double c, int m) {
  const double c2 = c * c;
  return m == 1 ? 1.0 : (m == 2 ? 4.0 * c : (m == 3 ? 12.0 * c2 - 3.0 : (32.0 * c2 - 16.0) * c));
}

// the target logit's factor (lambda c + psi(c)) / (1 + lambda) and its derivative (lambda + psi'(c)) / (1 + lambda)
__device__ __forceinline__ double asoftmax_target(float cf, double lam, int m, const ASoftmaxCuts& cuts) {
  const float cc = fminf(fmaxf(cf, -1.f), 1.f);
  const int k = asoftmax_k(cc, cuts);
  const double psi = ((k & 1) ? -1.0 : 1.0) * asoftmax_cheb((double)cc, m) - 2.0 * k;
  return (lam * (double)cc + psi) / (1.0 + lam);
}
__device__ __forceinline__ double asoftmax_target_d(float cf, double lam, int m, const ASoftmaxCuts& cuts) {
  // (outside [-1, 1] the clamp's own derivative is 0 for psi and for the lambda c term alike; cosines of unit vectors leave the
  // interval by a rounding only, where psi' = 0 anyway)
  if (cf < -1.f || cf > 1.f) return 0.0;
  const int k = asoftmax_k(cf, cuts);
  return (lam + ((k & 1) ? -1.0 : 1.0) * asoftmax_cheb_d((double)cf, m)) / (1.0 + lam);
}

// One workgroup per row, 256 columns per step.  mode 0: out = z.  mode 1: out = dc, dr[b] = sum_j dz_bj z_bj / r_b in fp64 (lane-strided
// partials, shuffle tree, wave order), 0 on a row whose norm sits at the clamp (r <= r_floor: the clamp's derivative).
__global__ __launch_bounds__(256) void asoftmax_logits_kernel(const float* __restrict__ c, const float* __restrict__ r,
                                                              const long long* __restrict__ labels, const float* __restrict__ lambda,
                                                              const float* __restrict__ dz, float* __restrict__ out,
                                                              float* __restrict__ dr, int K, int m, ASoftmaxCuts cuts, float r_floor,
                                                              int mode) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  const float rb = r[b];
  const double lam = (double)lambda[0];
  const long long y = labels[b];
  const float* pc = c + (long long)b * K;
  float* po = out + (long long)b * K;
  if (mode == 0) {
    for (int j = threadIdx.x; j < K; j += 256)
      po[j] = j == y ? (float)((double)rb * asoftmax_target(pc[j], lam, m, cuts)) : rb * pc[j];
    return;
  }
  const float* pg = dz + (long long)b * K;
  double s = 0.0;
  for (int j = threadIdx.x; j < K; j += 256) {
    const float g = pg[j], cj = pc[j];
    if (j == y) {
      po[j] = (float)((double)rb * (double)g * asoftmax_target_d(cj, lam, m, cuts));
      s += (double)g * asoftmax_target(cj, lam, m, cuts);
    } else {
      po[j] = rb * g;
      s += (double)g * (double)cj;
    }
  }
  s = dlip_block_sum4(s, red);      // = sum_j dz_bj z_bj / r_b
  if (threadIdx.x == 0) dr[b] = rb > r_floor ? (float)s : 0.f;
}

// r = max(|x|, eps): the sum, its order and the rounding of dlip_l2_normalize_f32 (one wave per row, fp64, shuffle tree) -- the same bits
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ x, float* __restrict__ r, int U, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= U) return;
  const float* p = x + (long long)row * D;
  double s = 0.0;
  for (int i = lane; i < D; i += 64) s += (double)p[i] * (double)p[i];
  const float nrm = fmaxf((float)sqrt(dlip_wave_sum_f64(s)), eps);
  if (lane == 0) r[row] = nrm;
}

// dx = dr x / r; a row at the clamp (r <= eps) gets zeros
__global__ __launch_bounds__(256) void row_norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ r,
                                                           const float* __restrict__ dr, float* __restrict__ dx, int U, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= U) return;
  const float rr = r[row];
  const float f = rr > eps ? dr[row] / rr : 0.f;
  for (int i = lane; i < D; i += 64) dx[(long long)row * D + i] = rr > eps ? f * x[(long long)row * D + i] : 0.f;
}

}  // namespace

extern "C" int dlip_asoftmax_logits_f32(const float* c, const float* r, const int64_t* labels, const float* lambda, const float* dz,
                                        float* out, float* dr, int32_t B, int32_t K, int32_t m, float r_floor, int32_t backward,
                                        dlip_stream_t stream) {
  DLIP_CHECK_ARG(c && r && labels && lambda && out && B > 0 && K > 0 && m >= 1 && m <= 4);
  DLIP_CHECK_ARG(!backward || (dz && dr));
  ASoftmaxCuts cuts = {-2.f, -2.f, -2.f};
  float* cv[3] = {&cuts.c1, &cuts.c2, &cuts.c3};
  for (int j = 1; j < m; ++j) *cv[j - 1] = (float)cos((double)j * 3.14159265358979323846 / (double)m);
  hipLaunchKernelGGL(asoftmax_logits_kernel, dim3((unsigned)B), dim3(256), 0, dlip_hip_stream(stream), c, r,
                     reinterpret_cast<const long long*>(labels), lambda, dz, out, dr, K, m, cuts, r_floor, backward ? 1 : 0);
  return dlip_launch_status();
}

extern "C" int dlip_row_norm_f32(const float* x, float* r, int32_t U, int32_t D, float eps, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && r && U > 0 && D > 0);
  hipLaunchKernelGGL(row_norm_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, dlip_hip_stream(stream), x, r, U, D, eps);
  return dlip_launch_status();
}

extern "C" int dlip_row_norm_bwd_f32(const float* x, const float* r, const float* dr, float* dx, int32_t U, int32_t D, float eps,
                                     dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && r && dr && dx && U > 0 && D > 0);
  hipLaunchKernelGGL(row_norm_bwd_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, dlip_hip_stream(stream), x, r, dr, dx, U, D, eps);
  return dlip_launch_status();
}

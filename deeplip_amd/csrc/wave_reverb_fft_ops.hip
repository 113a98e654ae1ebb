// Reverberation with long room responses: the definition of wave_augment_ops.hip's FIR kernel,
// y[t] = sum_k h[k] x[t + d - k], 0 <= t < n, x zero outside [0, n) (train_audio.py:454, the 'reverb' kind), computed as a uniformly
// partitioned overlap-save convolution in fp32.  P = DLIP_OLS_BLOCK new samples per step, transform length N = 2P.  Every partition
// boundary is anchored at sample 0 of the row and at tap 0 of the response, so a row's arithmetic depends on (x[:n], h, d) alone.
//
//   H[r, p]  = FFT_N(h_r[pP : (p + 1)P), zero-padded) / P        p < ceil(len_r / P)          once per bank  (rir_spectra_kernel)
//   X[b, k]  = FFT_N(x_b[(k - 1)P : (k + 1)P))                   (k - 1)P < n                 per call       (input_spectra_kernel)
//   Y[b, k]  = sum_p X[b, k - p] H[r, p], p ascending;  the last P samples of the inverse transform are the convolution indices
//              [kP, (k + 1)P);  index j goes to y[j - d]                                      per call       (accumulate_kernel)
//
// THE FFT CORE.  A real block of N = 2P samples is transformed as ONE complex transform of M = P points on z[j] = x[2j] + i x[2j + 1]
// and split into the half spectrum X[0 .. M] afterwards (X[k] = E[k] + w^k O[k], E / O the transforms of the even / odd samples,
// w = exp(-2 pi i / N)); bins 0 and M are real and share slot 0 as (X[0], X[M]), so a spectrum is exactly M complex words.  The forward
// transform is decimation in frequency (natural order in, bit-reversed out), the inverse decimation in time (bit-reversed in, natural
// out): no reordering pass, the split / unsplit steps address the bit-reversed positions directly.  Passes are radix-4 held in
// registers -- two radix-2 stages on four elements per lane, one LDS round trip -- with one radix-2 pass when log2(M) is odd.  The
// data lie in LDS as interleaved (re, im) pairs, one 8-byte access per element, with one pad word per 32 elements: the four elements
// of a butterfly are four separate accesses whose lanes run over consecutive elements while the quarter span is >= 32
// (conflict-free); in the narrow passes the lanes address short runs a power of two apart, which the pad shifts by one element per
// 32 (at 2^11 points: quarter span 8 four-way, 2 two-way, the closing radix-2 pass conflict-free).  Twiddles exp(-2 pi i k / N), k < M, are formed once with sincospi in fp64, rounded once to
// fp32, and kept at the head of the spectra block; each workgroup copies them into LDS.
#include "dlip_launch.h"

namespace {

constexpr int kM = DLIP_OLS_BLOCK;               // new samples per step P = points of the complex transform
constexpr int kThreads = 256;
constexpr int kPer = kM / kThreads;              // spectrum bins per lane
constexpr int kLg = kM == 1024 ? 10 : 11;
static_assert((kM == 1024 || kM == 2048) && DLIP_OLS_MAX_TAPS % kM == 0, "the passes below are written for 2^10 or 2^11 points");
constexpr int kZWords = kM + kM / 32;            // the padded data array, in complex words

__device__ __forceinline__ int row_len(const int32_t* lengths, long long b, int S) {
  if (lengths == nullptr) return S;
  const int v = lengths[b];
  return v < 1 ? 1 : (v > S ? S : v);
}

__device__ __forceinline__ int at(int i) { return i + (i >> 5); }
__device__ __forceinline__ int brev(int k) { return (int)(__brev((unsigned)k) >> (32 - kLg)); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)

__device__ __forceinline__ void radix2_pass(float2* z) {
  for (int t = threadIdx.x; t < kM / 2; t += kThreads) {
    const float2 a = z[at(2 * t)], b = z[at(2 * t + 1)];
    z[at(2 * t)] = cadd(a, b);
    z[at(2 * t + 1)] = csub(a, b);
  }
  __syncthreads();
}

// z (natural order) := DFT_M(z) in bit-reversed order.  tw[k] = exp(-2 pi i k / 2M).  Ends behind a barrier.
__device__ __forceinline__ void fft_dif(float2* z, const float2* tw) {
  int L = kM;
  for (; L >= 4; L >>= 2) {
    const int q = L >> 2, ts = 2 * kM / L;
    for (int t = threadIdx.x; t < kM / 4; t += kThreads) {
      const int j = t & (q - 1), i = ((t - j) << 2) + j;
      const float2 a = z[at(i)], b = z[at(i + q)], c = z[at(i + 2 * q)], d = z[at(i + 3 * q)];
      const float2 w1 = tw[j * ts], w2 = tw[2 * j * ts];
      const float2 a1 = cadd(a, c), c1 = cmul(csub(a, c), w1);
      const float2 b1 = cadd(b, d), u = cmul(csub(b, d), w1);
      const float2 d1 = make_float2(u.y, -u.x);                    // the twiddle a quarter turn on: -i w1
      z[at(i)] = cadd(a1, b1);
      z[at(i + q)] = cmul(csub(a1, b1), w2);
      z[at(i + 2 * q)] = cadd(c1, d1);
      z[at(i + 3 * q)] = cmul(csub(c1, d1), w2);
    }
    __syncthreads();
  }
  if (L == 2) radix2_pass(z);
}

// z (bit-reversed order) := M IDFT_M(z) in natural order: the passes of fft_dif undone back to front.  Ends behind a barrier.
__device__ __forceinline__ void ifft_dit(float2* z, const float2* tw) {
  if (kLg & 1) radix2_pass(z);
  for (int L = (kLg & 1) ? 8 : 4; L <= kM; L <<= 2) {
    const int q = L >> 2, ts = 2 * kM / L;
    for (int t = threadIdx.x; t < kM / 4; t += kThreads) {
      const int j = t & (q - 1), i = ((t - j) << 2) + j;
      const float2 a = z[at(i)], b = z[at(i + q)], c = z[at(i + 2 * q)], d = z[at(i + 3 * q)];
      const float2 w1 = tw[j * ts], w2 = tw[2 * j * ts];
      const float2 tb = cmulc(b, w2), td = cmulc(d, w2);
      const float2 a1 = cadd(a, tb), b1 = csub(a, tb), c1 = cadd(c, td), d1 = csub(c, td);
      const float2 tc = cmulc(c1, w1), u = cmulc(d1, w1);
      const float2 te = make_float2(-u.y, u.x);                    // i conj(w1)
      z[at(i)] = cadd(a1, tc);
      z[at(i + 2 * q)] = csub(a1, tc);
      z[at(i + q)] = cadd(b1, te);
      z[at(i + 3 * q)] = csub(b1, te);
    }
    __syncthreads();
  }
}

// Half spectrum of the 2M real samples whose packed transform fft_dif left in z: bin k of the lane's own kPer bins.
__device__ __forceinline__ float2 split_bin(const float2* z, const float2* tw, int k) {
  const float2 a = z[at(brev(k))];
  if (k == 0) return make_float2(a.x + a.y, a.x - a.y);            // (X[0], X[M]), both real
  const float2 m = z[at(brev(kM - k))];
  const float2 e = make_float2(0.5f * (a.x + m.x), 0.5f * (a.y - m.y));        // E = (Z[k] + conj Z[M - k]) / 2
  const float2 o = make_float2(0.5f * (a.y + m.y), -0.5f * (a.x - m.x));       // O = -i (Z[k] - conj Z[M - k]) / 2
  return cadd(e, cmul(o, tw[k]));
}

// ------------------------------------------------------------------------------------------------------------- response spectra
// One workgroup per (partition, response).  Forms the twiddle table itself (fp64 sincospi, rounded once); workgroup (0, 0) also
// leaves it at the head of the spectra block for the per-call kernels.
__global__ __launch_bounds__(kThreads) void rir_spectra_kernel(const float* __restrict__ rir, const int32_t* __restrict__ rir_len,
                                                                float2* __restrict__ spectra, int Lmax, int pmax) {
  __shared__ float2 z[kZWords];
  __shared__ float2 tw[kM];
  const int p = blockIdx.x, r = blockIdx.y;
  int len = rir_len[r];
  len = len < 1 ? 1 : (len > Lmax ? Lmax : len);
  if (p * kM >= len) return;                                       // past the response's own partitions (blockIdx alone: no barrier yet)
  const float* h = rir + (long long)r * Lmax + (long long)p * kM;
  const int cnt = len - p * kM < kM ? len - p * kM : kM;
  for (int j = threadIdx.x; j < kM; j += kThreads) {
    double s, c;
    sincospi(-(double)j / (double)kM, &s, &c);                     // exp(-2 pi i j / 2M)
    tw[j] = make_float2((float)c, (float)s);
    z[at(j)] = make_float2(2 * j < cnt ? h[2 * j] : 0.f, 2 * j + 1 < cnt ? h[2 * j + 1] : 0.f);
  }
  __syncthreads();
  if (p == 0 && r == 0)
    for (int j = threadIdx.x; j < kM; j += kThreads) spectra[j] = tw[j];
  fft_dif(z, tw);
  float2* out = spectra + kM + ((long long)r * pmax + p) * kM;
  const float scale = 1.f / (float)kM;                             // the inverse transform's 1 / M, a power of two
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int k = u * kThreads + (int)threadIdx.x;
    const float2 v = split_bin(z, tw, k);
    out[k] = make_float2(v.x * scale, v.y * scale);
  }
}

// ---------------------------------------------------------------------------------------------------------------- input spectra
// X[b, kb] of the reverberated rows: samples [(kb - 1)P, (kb + 1)P) of the row, zeros outside [0, n) (never read).  Blocks that lie
// wholly past the row's end are never read by accumulate_kernel and are not written.
__global__ __launch_bounds__(kThreads) void input_spectra_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                                  const int32_t* __restrict__ rir_idx, const float2* __restrict__ twg,
                                                                  float2* __restrict__ X, int S, int kx) {
  __shared__ float2 z[kZWords];
  __shared__ float2 tw[kM];
  const long long b = blockIdx.y;
  const int kb = blockIdx.x;
  const int n = row_len(lengths, b, S);
  const long long s0 = ((long long)kb - 1) * kM;
  if (rir_idx[b] < 0 || s0 >= n) return;                           // both depend on blockIdx alone and sit before the first barrier
  const float* xb = x + b * S;
  for (int j = threadIdx.x; j < kM; j += kThreads) {
    tw[j] = twg[j];
    const long long s = s0 + 2 * j;
    z[at(j)] = make_float2((s >= 0 && s < n) ? xb[s] : 0.f, (s + 1 >= 0 && s + 1 < n) ? xb[s + 1] : 0.f);
  }
  __syncthreads();
  fft_dif(z, tw);
  float2* out = X + (b * kx + kb) * kM;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int k = u * kThreads + (int)threadIdx.x;
    out[k] = split_bin(z, tw, k);
  }
}

// ---------------------------------------------------------------------------------------------------------- accumulate and invert
// One workgroup per (row, output block k): the outputs t = j - d of the convolution indices j in [kP, (k + 1)P).
__global__ __launch_bounds__(kThreads) void accumulate_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                               const float2* __restrict__ spectra, const int32_t* __restrict__ rir_len,
                                                               const int32_t* __restrict__ rir_peak, const int32_t* __restrict__ rir_idx,
                                                               const float2* __restrict__ X, float* __restrict__ y, int S, int R, int Lmax,
                                                               int pmax, int kx) {
  __shared__ float2 z[kZWords];
  __shared__ float2 tw[kM];
  const long long b = blockIdx.y;
  const int k = blockIdx.x;
  const int n = row_len(lengths, b, S);
  const float* xb = x + b * S;
  float* yb = y + b * S;
  int ri = rir_idx[b];
  // every exit below depends on blockIdx alone (the whole workgroup takes it) and sits in front of the first barrier
  if (ri < 0) {                                                    // pass-through rows: the input bit for bit, the zero tail
    for (long long t = (long long)k * kM + threadIdx.x; t < (long long)(k + 1) * kM && t < S; t += kThreads) yb[t] = t < n ? xb[t] : 0.f;
    return;
  }
  ri = ri < R ? ri : R - 1;
  int len = rir_len[ri];
  len = len < 1 ? 1 : (len > Lmax ? Lmax : len);
  int d = rir_peak[ri];
  d = d < 0 ? 0 : (d >= len ? len - 1 : d);
  const long long lo = (long long)k * kM - d, hi = lo + kM;        // the outputs t of this block: [lo, hi)
  if (hi <= 0 || lo >= S) return;
  if (lo >= n) {                                                   // past the row's end: zeros
    for (long long t = lo + threadIdx.x; t < hi && t < S; t += kThreads) yb[t] = 0.f;
    return;
  }
  for (int j = threadIdx.x; j < kM; j += kThreads) tw[j] = spectra[j];
  const int parts = (len + kM - 1) / kM;                           // the response's own partition count
  const int kbmax = (n - 1) / kM + 1;                              // the last input block that holds a sample of the row
  const int p0 = k - kbmax > 0 ? k - kbmax : 0, p1 = parts - 1 < k ? parts - 1 : k;
  const float2* Hr = spectra + kM + (long long)ri * pmax * kM;
  const float2* Xb = X + b * kx * kM;
  float2 acc[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) acc[u] = make_float2(0.f, 0.f);
  for (int p = p0; p <= p1; ++p) {                                 // p ascending, whatever the geometry
    const float2* Hp = Hr + (long long)p * kM + threadIdx.x;
    const float2* Xp = Xb + (long long)(k - p) * kM + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const float2 xv = Xp[u * kThreads], hv = Hp[u * kThreads];
      if (u == 0 && threadIdx.x == 0) {                            // slot 0 holds the two real bins 0 and M
        acc[u].x = fmaf(xv.x, hv.x, acc[u].x);
        acc[u].y = fmaf(xv.y, hv.y, acc[u].y);
      } else {
        acc[u].x = fmaf(xv.x, hv.x, fmaf(-xv.y, hv.y, acc[u].x));
        acc[u].y = fmaf(xv.x, hv.y, fmaf(xv.y, hv.x, acc[u].y));
      }
    }
  }
  // the half spectrum Y back to the packed transform Z[k] = E[k] + i O[k], at the bit-reversed positions ifft_dit starts from
#pragma unroll
  for (int u = 0; u < kPer; ++u) z[at(u * kThreads + (int)threadIdx.x)] = acc[u];
  __syncthreads();
  float2 zk[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int kk = u * kThreads + (int)threadIdx.x;
    const float2 a = acc[u];
    if (kk == 0) {
      zk[u] = make_float2(0.5f * (a.x + a.y), 0.5f * (a.x - a.y));
    } else {
      const float2 m = z[at(kM - kk)];
      const float2 e = make_float2(0.5f * (a.x + m.x), 0.5f * (a.y - m.y));    // (Y[k] + conj Y[M - k]) / 2
      const float2 g = make_float2(0.5f * (a.x - m.x), 0.5f * (a.y + m.y));    // (Y[k] - conj Y[M - k]) / 2
      const float2 o = cmulc(g, tw[kk]);
      zk[u] = make_float2(e.x - o.y, e.y + o.x);                               // E + i O
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kPer; ++u) z[at(brev(u * kThreads + (int)threadIdx.x))] = zk[u];
  __syncthreads();
  ifft_dit(z, tw);
  // the last P real samples = complex words M / 2 .. M - 1: convolution index kP + 2 (j - M / 2) + {0, 1}
  for (int j = kM / 2 + threadIdx.x; j < kM; j += kThreads) {
    const float2 v = z[at(j)];
    const long long t = lo + 2 * (j - kM / 2);
    if (t >= 0 && t < S) yb[t] = t < n ? v.x : 0.f;
    if (t + 1 >= 0 && t + 1 < S) yb[t + 1] = t + 1 < n ? v.y : 0.f;
  }
}

inline int parts_of(int32_t Lmax) { return (Lmax + kM - 1) / kM; }
inline int64_t x_blocks(int64_t S) { return (S - 1) / kM + 2; }     // input blocks a row of S samples can hold a sample in
inline bool sizes_ok(int64_t B, int64_t S) { return B > 0 && B <= 65535 && S > 0 && S <= 0x7fffffffll - 4 * (int64_t)DLIP_OLS_MAX_TAPS; }

}  // namespace

extern "C" int64_t dlip_wave_rir_spectra_bytes(int32_t R, int32_t Lmax) {
  if (R <= 0 || R > 65535 || Lmax <= 0 || Lmax > DLIP_OLS_MAX_TAPS) return DLIP_EINVAL;
  return ((int64_t)kM + (int64_t)R * parts_of(Lmax) * kM) * (int64_t)sizeof(float2);
}

extern "C" int dlip_wave_rir_spectra_f32(const float* rir, const int32_t* rir_len, void* spectra, int64_t spectra_bytes, int32_t R,
                                         int32_t Lmax, dlip_stream_t stream) {
  DLIP_CHECK_ARG(rir && rir_len && spectra && dlip_aligned<8>(spectra));
  const int64_t need = dlip_wave_rir_spectra_bytes(R, Lmax);
  DLIP_CHECK_ARG(need > 0 && spectra_bytes >= need);
  const int pmax = parts_of(Lmax);
  hipLaunchKernelGGL(rir_spectra_kernel, dim3(pmax, R), dim3(kThreads), 0, dlip_hip_stream(stream), rir, rir_len,
                     static_cast<float2*>(spectra), Lmax, pmax);
  return dlip_launch_status();
}

// [B tiles(S)] pairs of doubles (the power partials of keep_power) | X [B, x_blocks(S), P] complex
extern "C" int64_t dlip_wave_reverb_fft_workspace_bytes(int64_t B, int64_t S, int32_t Lmax) {
  if (!sizes_ok(B, S) || Lmax <= 0 || Lmax > DLIP_OLS_MAX_TAPS) return DLIP_EINVAL;
  const int64_t part = dlip_wave_reverb_workspace_bytes(B, S);
  if (part <= 0) return DLIP_EINVAL;
  return part + B * x_blocks(S) * kM * (int64_t)sizeof(float2);
}

extern "C" int dlip_wave_reverb_fft_f32(const float* x, const int32_t* lengths, const void* spectra, const int32_t* rir_len,
                                        const int32_t* rir_peak, const int32_t* rir_idx, float* y, void* workspace,
                                        int64_t workspace_bytes, int32_t B, int32_t S, int32_t R, int32_t Lmax, int32_t keep_power,
                                        dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && spectra && rir_len && rir_peak && rir_idx && y && x != y && R > 0 && R <= 65535 && Lmax > 0 &&
                 Lmax <= DLIP_OLS_MAX_TAPS);
  const int64_t need = dlip_wave_reverb_fft_workspace_bytes(B, S, Lmax);
  DLIP_CHECK_ARG(need > 0 && workspace && dlip_aligned<8>(workspace, spectra) && workspace_bytes >= need);
  const int64_t part_bytes = dlip_wave_reverb_workspace_bytes(B, S);
  double* part = static_cast<double*>(workspace);
  float2* X = reinterpret_cast<float2*>(static_cast<char*>(workspace) + part_bytes);
  const float2* sp = static_cast<const float2*>(spectra);
  const int kx = (int)x_blocks(S), pmax = parts_of(Lmax);
  const int kout = (int)(((int64_t)S + Lmax - 2) / kM + 1);        // output blocks: t = j - d up to S - 1 with d up to Lmax - 1
  hipLaunchKernelGGL(input_spectra_kernel, dim3(kx, B), dim3(kThreads), 0, dlip_hip_stream(stream), x, lengths, rir_idx, sp, X, S, kx);
  hipLaunchKernelGGL(accumulate_kernel, dim3(kout, B), dim3(kThreads), 0, dlip_hip_stream(stream), x, lengths, sp, rir_len, rir_peak,
                     rir_idx, X, y, S, R, Lmax, pmax, kx);
  if (keep_power) dlip_wave_reverb_keep_power(x, lengths, rir_idx, y, part, B, S, dlip_hip_stream(stream));
  return dlip_launch_status();
}

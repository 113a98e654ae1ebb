// The SincNet front layer of `arch: sincnet` (Ravanelli & Bengio 2018): F learnable band-pass filters of L taps on
// the raw waveform, squared, averaged per frame and logged -- from the waveform to frame-level log energies in ONE launch, the stride-1
// filter output z [B, F, S] never stored.  Nothing upstream defines the layer: include/deeplip_hip.h with DESIGN.md 4l is the definition.
//
//   taps      low_hz_, band_hz_ [F] -> g [F, L], formed in fp64 and rounded once; g is even (the half m >= 0 is computed, then mirrored)
//   features  a 256-lane workgroup owns (row, a tile of TF frames, FT filters).  The tile's samples + L - 1 halo sit in LDS, zero outside
//             [0, len): a row never reads its neighbour or the padding.  A lane owns a position p of a 256-position chunk and forms the
//             pair sum s = x[p - m] + x[p + m] ONCE per tap m for all FT filters: (L + 1) / 2 fma per filter and position, the taps
//             staged in LDS in chunks and read as broadcasts.  z^2 goes to LDS and lane (frame, filter) adds its frame's positions in
//             ascending order in fp64; only y = log(e + eps) leaves.  Exact fp32 fma chains on the vector ALUs, m ascending.
//   backward  the same tiling, workgroups walking (row, tile) items in a fixed stride: z is recomputed, dz = z (2 / frame_len) sum_t dy
//             exp(-y) over the tile's frames that hold p (1 / (e + eps) = exp(-y)), and the folded tap gradient D[f, m] = sum_p dz (x[p - m]
//             + x[p + m]) is accumulated in registers -- lane (m, position group) -- over all of a workgroup's items; one partial per
//             workgroup goes to the caller's workspace and a second launch adds the partials in workgroup order in fp64.  No atomics:
//             two runs have the same bits.
// What a lane computes for a frame depends on the row's own samples, its length and the frame index alone: a row has the same bits alone,
// in a batch, under any padding.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kXCap = DLIP_SINC_LDS_SAMPLES;      // floats of a tile's samples + halo
constexpr int kTapChunk = 64;                     // taps staged per pass of the inner loop
constexpr int kBwdGroups = 512;                   // workgroups (per filter pass) of the backward at most: two per compute unit

__device__ __forceinline__ int sinc_row_len(const int32_t* lengths, int b, int S) {
  if (lengths == nullptr) return S;
  const int v = lengths[b];
  return v < 1 ? 1 : (v > S ? S : v);
}

__host__ __device__ __forceinline__ int sinc_frames(int n, int flen, int step) {      // sigproc.framesig's count
  return n <= flen ? 1 : 1 + (int)(((long long)n - flen + step - 1) / step);
}

__device__ __forceinline__ long long sinc_out_index(int layout, long long b, int t, int f, int F, int Fp, int NF) {
  return layout ? (b * NF + t) * Fp + f : (b * F + f) * NF + t;
}

// ---- taps: one workgroup, fp64 inside
__device__ __forceinline__ void sinc_edges(const float* low, const float* band, int f, double rate, double min_low, double min_band,
                                           double& f1, double& f2, bool& open) {
  f1 = min_low + fabs((double)low[f]);
  const double raw = f1 + min_band + fabs((double)band[f]);
  open = raw >= min_low && raw <= 0.5 * rate;       // (torch.clamp: the gradient passes on the closed interval)
  f2 = raw < min_low ? min_low : (raw > 0.5 * rate ? 0.5 * rate : raw);
}

constexpr double kPi = 3.14159265358979323846;

__global__ __launch_bounds__(kThreads) void sinc_taps_kernel(const float* __restrict__ low, const float* __restrict__ band,
                                                              float* __restrict__ g, int F, int L, double rate, double min_low,
                                                              double min_band) {
  const int H = (L - 1) / 2;
  for (int i = threadIdx.x; i < F * (H + 1); i += kThreads) {
    const int f = i / (H + 1), m = i - f * (H + 1);
    double v = 1.0;
    if (m > 0) {
      double f1, f2;
      bool open;
      sinc_edges(low, band, f, rate, min_low, min_band, f1, f2, open);
      const double n = (double)m / rate;
      const double w = 0.54 - 0.46 * cos(2.0 * kPi * (double)(H + m) / (double)(L - 1));
      v = w * (sin(2.0 * kPi * f2 * n) - sin(2.0 * kPi * f1 * n)) / ((kPi * n) * 2.0 * (f2 - f1));
    }
    g[(long long)f * L + H + m] = (float)v;
    g[(long long)f * L + H - m] = (float)v;
  }
}

// d low_hz_[f], d band_hz_[f] from dg [F, L]: the chain rule through the tap formula, summed over l in a fixed order (lane-strided,
// wave butterflies, waves in order), fp64
__global__ __launch_bounds__(kThreads) void sinc_taps_bwd_kernel(const float* __restrict__ low, const float* __restrict__ band,
                                                                  const float* __restrict__ dg, float* __restrict__ dlow,
                                                                  float* __restrict__ dband, int F, int L, double rate, double min_low,
                                                                  double min_band) {
  __shared__ double red[4];
  const int H = (L - 1) / 2;
  for (int f = 0; f < F; ++f) {
    double f1, f2;
    bool open;
    sinc_edges(low, band, f, rate, min_low, min_band, f1, f2, open);
    const double D = f2 - f1;
    double a1 = 0.0, a2 = 0.0;      // sum dg dg/df1, sum dg dg/df2
    for (int l = threadIdx.x; l < L; l += kThreads) {
      const int m = l < H ? H - l : l - H;
      if (m == 0) continue;
      const double n = (double)m / rate;
      const double w = 0.54 - 0.46 * cos(2.0 * kPi * (double)(H + m) / (double)(L - 1));
      const double q = (sin(2.0 * kPi * f2 * n) - sin(2.0 * kPi * f1 * n)) / (2.0 * kPi * n * D * D);
      const double d = (double)dg[(long long)f * L + l];
      a1 += d * w * (q - cos(2.0 * kPi * f1 * n) / D);
      a2 += d * w * (cos(2.0 * kPi * f2 * n) / D - q);
    }
    a1 = dlip_block_sum4(a1, red);
    __syncthreads();
    a2 = dlip_block_sum4(a2, red);
    __syncthreads();
    if (threadIdx.x == 0) {
      const double lo = (double)low[f], bd = (double)band[f];
      const double slo = lo > 0.0 ? 1.0 : (lo < 0.0 ? -1.0 : 0.0), sbd = bd > 0.0 ? 1.0 : (bd < 0.0 ? -1.0 : 0.0);
      const double through = open ? a2 : 0.0;       // a clamped f2 has zero derivative
      dlow[f] = (float)(slo * (a1 + through));
      dband[f] = (float)(sbd * through);
    }
  }
}

// ---- what forward and backward share: a tile's samples in LDS, and z of one position for FT filters
struct SincTile {
  int len, nf, t0, tv, span;      // row length, its frames, the tile's first frame, its frames with content, its positions with content
};

__device__ __forceinline__ SincTile sinc_tile(const int32_t* lengths, int b, int S, int tile, int TF, int flen, int step) {
  SincTile t;
  t.len = sinc_row_len(lengths, b, S);
  t.nf = sinc_frames(t.len, flen, step);
  t.t0 = tile * TF;
  t.tv = t.nf - t.t0 < TF ? t.nf - t.t0 : TF;
  t.span = 0;
  if (t.tv > 0) {
    const long long p0 = (long long)t.t0 * step;
    long long sp = (long long)(t.tv - 1) * step + flen;
    if (sp > (long long)t.len - p0) sp = (long long)t.len - p0;
    t.span = sp > 0 ? (int)sp : 0;
  }
  return t;
}

// xs[i] = x~[p0 - H + i], i < span + 2 H: zero outside the row's own samples
__device__ __forceinline__ void sinc_stage_samples(float* xs, const float* __restrict__ row, const SincTile& t, int step, int H) {
  const long long p0 = (long long)t.t0 * step;
  for (int i = threadIdx.x; i < t.span + 2 * H; i += kThreads) {
    const long long q = p0 - H + i;
    xs[i] = (q >= 0 && q < t.len) ? row[q] : 0.f;
  }
}

// z[f] of local position pl (xs index of its centre: pl + H) for filters f0 .. f0 + FT - 1; gl is restaged per kTapChunk taps.  All lanes call.
template <int FT>
__device__ __forceinline__ void sinc_filter(float (&acc)[FT], const float* xs, float* gl, const float* __restrict__ g, int pl, int f0, int F,
                                            int L, int H) {
#pragma unroll
  for (int f = 0; f < FT; ++f) acc[f] = 0.f;
  for (int mc = 0; mc <= H; mc += kTapChunk) {
    __syncthreads();
    for (int i = threadIdx.x; i < kTapChunk * FT; i += kThreads) {
      const int mm = i / FT, f = i - mm * FT, m = mc + mm;
      gl[i] = (m <= H && f0 + f < F) ? g[(long long)(f0 + f) * L + H + m] : 0.f;
    }
    __syncthreads();
    const int mend = H + 1 - mc < kTapChunk ? H + 1 - mc : kTapChunk;
    const float* c = xs + pl + H;
    for (int mm = 0; mm < mend; ++mm) {
      const int m = mc + mm;
      const float s = c[-m] + (m ? c[m] : 0.f);
      const float* gr = gl + mm * FT;
#pragma unroll
      for (int f = 0; f < FT; ++f) acc[f] = fmaf(gr[f], s, acc[f]);
    }
  }
}

template <int FT>
__global__ __launch_bounds__(kThreads) void sinc_features_kernel(const float* __restrict__ wave, const int32_t* __restrict__ lengths,
                                                                  const float* __restrict__ g, float* __restrict__ y,
                                                                  int32_t* __restrict__ frame_lengths, int S, int F, int L, int flen, int step,
                                                                  int NF, int TF, int layout, int Fp, float eps) {
  __shared__ __attribute__((aligned(16))) float xs[kXCap];
  __shared__ __attribute__((aligned(16))) float gl[kTapChunk * FT];
  __shared__ float zz[kThreads * (FT + 1)];
  const int b = blockIdx.y, f0 = blockIdx.z * FT, H = (L - 1) / 2;
  const SincTile t = sinc_tile(lengths, b, S, blockIdx.x, TF, flen, step);
  if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0 && frame_lengths != nullptr) frame_lengths[b] = t.nf;
  const int tn = NF - t.t0 < TF ? NF - t.t0 : TF;          // the tile's frames in the tensor
  // frames at or past the row's count, and (channels-last) the padding channels: zeros
  for (int i = threadIdx.x; i < tn * FT; i += kThreads) {
    const int tl = i / FT, f = i - tl * FT;
    if (t.t0 + tl >= t.nf && f0 + f < F) y[sinc_out_index(layout, b, t.t0 + tl, f0 + f, F, Fp, NF)] = 0.f;
  }
  if (layout && blockIdx.z == 0 && Fp > F)
    for (int i = threadIdx.x; i < tn * (Fp - F); i += kThreads) {
      const int tl = i / (Fp - F), k = i - tl * (Fp - F);
      y[((long long)b * NF + t.t0 + tl) * Fp + F + k] = 0.f;
    }
  if (t.tv <= 0) return;
  sinc_stage_samples(xs, wave + (long long)b * S, t, step, H);
  const int tl = threadIdx.x / FT, fl = threadIdx.x - tl * FT;       // the lane's (frame, filter) of the tile
  double e = 0.0;
  for (int c0 = 0; c0 < t.span; c0 += kThreads) {
    const bool valid = c0 + (int)threadIdx.x < t.span;
    const int pl = valid ? c0 + threadIdx.x : t.span - 1;
    float acc[FT];
    sinc_filter<FT>(acc, xs, gl, g, pl, f0, F, L, H);
#pragma unroll
    for (int f = 0; f < FT; ++f) zz[threadIdx.x * (FT + 1) + f] = valid ? acc[f] * acc[f] : 0.f;
    __syncthreads();
    if (tl < t.tv) {
      const int nv = t.span - c0 < kThreads ? t.span - c0 : kThreads;
      int lo = tl * step - c0, hi = tl * step + flen - c0;
      lo = lo < 0 ? 0 : lo;
      hi = hi > nv ? nv : hi;
      for (int p = lo; p < hi; ++p) e += (double)zz[p * (FT + 1) + fl];
    }
    // (the next chunk writes zz behind sinc_filter's barriers)
  }
  if (tl < t.tv && f0 + fl < F)
    y[sinc_out_index(layout, b, t.t0 + tl, f0 + fl, F, Fp, NF)] = (float)log(e / (double)flen + (double)eps);
}

// grid (n_groups, passes); workgroup w walks items w, w + n_groups, ... of (row, tile), row-major.  MS = 1 << ms_log2 lanes run along the
// folded taps m, the 256 / MS position groups share a chunk's positions; H + 1 <= 2 MS.
template <int FT>
__global__ __launch_bounds__(kThreads) void sinc_features_bwd_kernel(const float* __restrict__ wave, const int32_t* __restrict__ lengths,
                                                                      const float* __restrict__ g, const float* __restrict__ y,
                                                                      const float* __restrict__ dy, float* __restrict__ part, int B, int S, int F,
                                                                      int L, int flen, int step, int NF, int TF, int layout, int Fp, int tiles,
                                                                      int ms_log2) {
  __shared__ __attribute__((aligned(16))) float xs[kXCap];
  __shared__ __attribute__((aligned(16))) float gl[kTapChunk * FT];
  __shared__ __attribute__((aligned(16))) float zz[kThreads * FT];
  __shared__ float cw[32 * FT];                               // (TF <= 32) dy exp(-y) 2 / frame_len of the tile's frames
  const int f0 = blockIdx.y * FT, H = (L - 1) / 2;
  const int MS = 1 << ms_log2, G = kThreads >> ms_log2;
  const int mi = threadIdx.x & (MS - 1), pg = threadIdx.x >> ms_log2;
  float dacc[2][FT];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int f = 0; f < FT; ++f) dacc[k][f] = 0.f;
  const long long items = (long long)B * tiles;
  const float scale = 2.0f / (float)flen;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int b = (int)(it / tiles), tile = (int)(it - (long long)b * tiles);
    const SincTile t = sinc_tile(lengths, b, S, tile, TF, flen, step);
    if (t.tv <= 0 || t.span <= 0) continue;                   // (the same branch for the whole workgroup)
    __syncthreads();                                          // the previous item's readers of xs, cw and zz are done
    sinc_stage_samples(xs, wave + (long long)b * S, t, step, H);
    for (int i = threadIdx.x; i < TF * FT; i += kThreads) {
      const int tl = i / FT, f = i - tl * FT;
      float v = 0.f;
      if (tl < t.tv && f0 + f < F) {
        const long long o = sinc_out_index(layout, b, t.t0 + tl, f0 + f, F, Fp, NF);
        v = dy[o] * expf(-y[o]) * scale;
      }
      cw[i] = v;
    }
    for (int c0 = 0; c0 < t.span; c0 += kThreads) {
      const int q = c0 + threadIdx.x;
      const bool valid = q < t.span;
      float acc[FT];
      sinc_filter<FT>(acc, xs, gl, g, valid ? q : t.span - 1, f0, F, L, H);     // (its barriers also publish xs and cw)
      float w[FT];
#pragma unroll
      for (int f = 0; f < FT; ++f) w[f] = 0.f;
      if (valid) {
        const int tlo = q < flen ? 0 : (q - flen) / step + 1;
        const int thi = q / step < t.tv - 1 ? q / step : t.tv - 1;
        for (int tl = tlo; tl <= thi; ++tl)
#pragma unroll
          for (int f = 0; f < FT; ++f) w[f] += cw[tl * FT + f];
      }
#pragma unroll
      for (int f = 0; f < FT; ++f) zz[threadIdx.x * FT + f] = acc[f] * w[f];
      __syncthreads();
      const int nv = t.span - c0 < kThreads ? t.span - c0 : kThreads;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int m = mi + k * MS;
        if (m <= H && (k == 0 || G == 1)) {
          const float* c = xs + c0 + H;
          for (int p = pg; p < nv; p += G) {
            const float s = c[p - m] + (m ? c[p + m] : 0.f);
            const float* zr = zz + p * FT;
#pragma unroll
            for (int f = 0; f < FT; ++f) dacc[k][f] = fmaf(zr[f], s, dacc[k][f]);
          }
        }
      }
      // (the next chunk writes zz behind sinc_filter's barriers)
    }
  }
  // the position groups meet in group order; one partial [FT, H + 1] per workgroup
  float* out = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * FT * (H + 1);
  __syncthreads();
#pragma unroll
  for (int f = 0; f < FT; ++f) zz[threadIdx.x * FT + f] = dacc[0][f];
  __syncthreads();
  if (pg == 0 && mi <= H) {
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      float v = zz[mi * FT + f];
      for (int gi = 1; gi < G; ++gi) v += zz[(gi * MS + mi) * FT + f];
      out[f * (H + 1) + mi] = v;
    }
  }
  if (G == 1 && mi + MS <= H) {
#pragma unroll
    for (int f = 0; f < FT; ++f) out[f * (H + 1) + mi + MS] = dacc[1][f];
  }
}

// dg[f, H - m] = dg[f, H + m] = D[f, m] / 2 (m > 0), dg[f, H] = D[f, 0]; D = the partials added in workgroup order, fp64
__global__ __launch_bounds__(kThreads) void sinc_dg_finish_kernel(const float* __restrict__ part, float* __restrict__ dg, int F, int L, int FT,
                                                                   int groups) {
  const int H = (L - 1) / 2;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= F * (H + 1)) return;
  const int f = i / (H + 1), m = i - f * (H + 1);
  const int z = f / FT, fl = f - z * FT;
  double acc = 0.0;
  for (int w = 0; w < groups; ++w) acc += (double)part[(((long long)z * groups + w) * FT + fl) * (H + 1) + m];
  if (m == 0) {
    dg[(long long)f * L + H] = (float)acc;
  } else {
    const float v = (float)(0.5 * acc);
    dg[(long long)f * L + H - m] = v;
    dg[(long long)f * L + H + m] = v;
  }
}

struct SincPlan {
  int FT, passes, TF, tiles, groups, ms_log2;
};

inline bool sinc_sizes_ok(long long B, long long S, long long F, long long L, long long flen, long long step) {
  return B >= 1 && B <= 65535 && S >= 1 && S <= 0x7fffffffll - 4096 && F >= 1 && F <= DLIP_SINC_MAX_FILTERS && L >= 3 &&
         L <= DLIP_SINC_MAX_TAPS && (L & 1) == 1 && flen >= 1 && step >= 1 && flen + (L - 1) <= kXCap;
}

inline SincPlan sinc_plan(int B, int S, int F, int L, int flen, int step) {
  SincPlan p;
  p.FT = F <= 8 ? 8 : 24;
  p.passes = (F + p.FT - 1) / p.FT;
  const int tf_lanes = kThreads / p.FT;                            // a lane per (frame, filter): 32 | 10
  const int tf_lds = (kXCap - (L - 1) - flen) / step + 1;          // span + halo fits the LDS block
  p.TF = tf_lanes < tf_lds ? tf_lanes : tf_lds;
  const int NF = sinc_frames(S, flen, step);
  p.tiles = (NF + p.TF - 1) / p.TF;
  const long long items = (long long)B * p.tiles;
  p.groups = (int)(items < kBwdGroups ? items : kBwdGroups);
  const int H1 = (L + 1) / 2;
  p.ms_log2 = 0;
  while ((1 << p.ms_log2) < H1 && p.ms_log2 < 8) ++p.ms_log2;
  return p;
}

}  // namespace

extern "C" int dlip_sinc_taps_f32(const float* low_hz, const float* band_hz, float* g, int32_t F, int32_t L, double rate, double min_low_hz,
                                  double min_band_hz, dlip_stream_t stream) {
  DLIP_CHECK_ARG(low_hz && band_hz && g && F >= 1 && F <= DLIP_SINC_MAX_FILTERS && L >= 3 && L <= DLIP_SINC_MAX_TAPS && (L & 1) == 1);
  DLIP_CHECK_ARG(rate > 0.0 && min_low_hz >= 0.0 && min_band_hz >= 0.0 && min_low_hz <= 0.5 * rate);     // (a NaN fails the comparisons)
  hipLaunchKernelGGL(sinc_taps_kernel, dim3(1), dim3(kThreads), 0, dlip_hip_stream(stream), low_hz, band_hz, g, F, L, rate, min_low_hz,
                     min_band_hz);
  return dlip_launch_status();
}

extern "C" int dlip_sinc_taps_bwd_f32(const float* low_hz, const float* band_hz, const float* dg, float* dlow, float* dband, int32_t F, int32_t L,
                                      double rate, double min_low_hz, double min_band_hz, dlip_stream_t stream) {
  DLIP_CHECK_ARG(low_hz && band_hz && dg && dlow && dband && F >= 1 && F <= DLIP_SINC_MAX_FILTERS && L >= 3 && L <= DLIP_SINC_MAX_TAPS &&
                 (L & 1) == 1);
  DLIP_CHECK_ARG(rate > 0.0 && min_low_hz >= 0.0 && min_band_hz >= 0.0 && min_low_hz <= 0.5 * rate);
  hipLaunchKernelGGL(sinc_taps_bwd_kernel, dim3(1), dim3(kThreads), 0, dlip_hip_stream(stream), low_hz, band_hz, dg, dlow, dband, F, L, rate,
                     min_low_hz, min_band_hz);
  return dlip_launch_status();
}

extern "C" int dlip_sinc_features_f32(const float* wave, const int32_t* lengths, const float* g, float* y, int32_t* frame_lengths, int32_t B,
                                      int32_t S, int32_t F, int32_t L, int32_t frame_len, int32_t frame_step, int32_t NF, int32_t layout,
                                      int32_t Fp, float eps, dlip_stream_t stream) {
  DLIP_CHECK_ARG(sinc_sizes_ok(B, S, F, L, frame_len, frame_step));
  DLIP_CHECK_ARG(wave && g && y && NF == sinc_frames(S, frame_len, frame_step) && eps > 0.f);
  DLIP_CHECK_ARG((layout == 0 && Fp == F) || (layout == 1 && Fp >= F && Fp <= F + 31));
  DLIP_CHECK_ARG(dlip_aligned<4>(wave, lengths, g, y, frame_lengths));
  const SincPlan p = sinc_plan(B, S, F, L, frame_len, frame_step);
  const dim3 grid((unsigned)p.tiles, (unsigned)B, (unsigned)p.passes);
#define DLIP_SINC_FWD(FT)                                                                                                             \
  hipLaunchKernelGGL(sinc_features_kernel<FT>, grid, dim3(kThreads), 0, dlip_hip_stream(stream), wave, lengths, g, y, frame_lengths, S, F, L, \
                     frame_len, frame_step, NF, p.TF, layout, Fp, eps)
  if (p.FT == 8) DLIP_SINC_FWD(8);
  else DLIP_SINC_FWD(24);
#undef DLIP_SINC_FWD
  return dlip_launch_status();
}

extern "C" int64_t dlip_sinc_features_bwd_workspace_bytes(int32_t B, int32_t S, int32_t F, int32_t L, int32_t frame_len, int32_t frame_step) {
  if (!sinc_sizes_ok(B, S, F, L, frame_len, frame_step)) return DLIP_EINVAL;
  const SincPlan p = sinc_plan(B, S, F, L, frame_len, frame_step);
  return (int64_t)p.passes * p.groups * p.FT * ((L + 1) / 2) * (int64_t)sizeof(float);
}

extern "C" int dlip_sinc_features_bwd_f32(const float* wave, const int32_t* lengths, const float* g, const float* y, const float* dy, float* dg,
                                          void* workspace, int64_t workspace_bytes, int32_t B, int32_t S, int32_t F, int32_t L,
                                          int32_t frame_len, int32_t frame_step, int32_t NF, int32_t layout, int32_t Fp, dlip_stream_t stream) {
  DLIP_CHECK_ARG(sinc_sizes_ok(B, S, F, L, frame_len, frame_step));
  DLIP_CHECK_ARG(wave && g && y && dy && dg && workspace && NF == sinc_frames(S, frame_len, frame_step));
  DLIP_CHECK_ARG((layout == 0 && Fp == F) || (layout == 1 && Fp >= F && Fp <= F + 31));
  DLIP_CHECK_ARG(dlip_aligned<4>(wave, lengths, g, y, dy, dg) && dlip_aligned16(workspace));
  DLIP_CHECK_ARG(workspace_bytes >= dlip_sinc_features_bwd_workspace_bytes(B, S, F, L, frame_len, frame_step));
  const SincPlan p = sinc_plan(B, S, F, L, frame_len, frame_step);
  float* part = static_cast<float*>(workspace);
  hipStream_t st = dlip_hip_stream(stream);
  const dim3 grid((unsigned)p.groups, (unsigned)p.passes);
#define DLIP_SINC_BWD(FT)                                                                                                          \
  hipLaunchKernelGGL(sinc_features_bwd_kernel<FT>, grid, dim3(kThreads), 0, st, wave, lengths, g, y, dy, part, B, S, F, L, frame_len, \
                     frame_step, NF, p.TF, layout, Fp, p.tiles, p.ms_log2)
  if (p.FT == 8) DLIP_SINC_BWD(8);
  else DLIP_SINC_BWD(24);
#undef DLIP_SINC_BWD
  int rc = dlip_launch_status();
  if (rc != DLIP_OK) return rc;
  const int outs = F * ((L + 1) / 2);
  hipLaunchKernelGGL(sinc_dg_finish_kernel, dim3((unsigned)((outs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, dg, F, L, p.FT,
                     p.groups);
  return dlip_launch_status();
}

// SpecAugment on the feature batch (ABI 67, added): a time warp, then frequency masks, then time masks (Park et
// al. 2019) on x [B, C, NF] (features by frames, frames contiguous) + optional frame counts.  Nothing upstream defines the stage:
// include/deeplip_hip.h with DESIGN.md 4j is the definition.  The host draws LENGTH-FREE 31-bit integers (`draws` [B,
// DLIP_SPECAUG_DRAWS]); the device resolves them against the row's own length n with pick(r, m) = (int64(r) m) >> 31, so the stage runs
// behind lengths the host never reads and replays in a recorded plan with new lengths and new draws.
//
// A 256-lane workgroup owns a tile of frames of one row (consecutive lanes consecutive frames, VEC frames per lane: one 4-byte or one
// 16-byte access) and a contiguous range of features.  A lane resolves its frames ONCE -- source index i, fraction a (one fp64 division
// per frame), time-mask bit -- and reuses them for every feature of the range; the frequency masks are wave-uniform.  Every output is
// one select / one fmaf of values the row alone decides: a row has the same bits whatever B, NF, the feature split, the tile and its
// neighbours are.  fill = 1 (the row's mean) is a first launch of DLIP_SPECAUG_MEAN_PARTS fp64 partial sums per row into the workspace
// (feature f in part f mod PARTS, per lane features then frames ascending, lanes meeting in wave order: (C, n) alone decide the
// order), added up part-ascending by every workgroup of the row.  Frames t >= n of x are never loaded.  No atomics.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMasks = DLIP_SPECAUG_MAX_MASKS;
constexpr int kParts = DLIP_SPECAUG_MEAN_PARTS;

__device__ __forceinline__ int row_len(const int32_t* lengths, long long b, long long NF) {
  if (lengths == nullptr) return (int)NF;
  const int v = lengths[b];
  return v < 1 ? 1 : (v > NF ? (int)NF : v);
}

// a 31-bit draw onto [0, m): negatives count as 0
__device__ __forceinline__ int pick(int r, int m) { return (int)(((long long)(r < 0 ? 0 : r) * m) >> 31); }

__global__ __launch_bounds__(kThreads) void specaug_mean_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                                 double* __restrict__ part, int C, long long NF) {
  __shared__ double red[4];
  const long long b = blockIdx.y;
  const int g = blockIdx.x;
  const int n = row_len(lengths, b, NF);
  const float* xb = x + b * C * NF;
  double acc = 0.0;
  for (int f = g; f < C; f += kParts) {
    const float* xr = xb + (long long)f * NF;
    for (int t = threadIdx.x; t < n; t += kThreads) acc += (double)xr[t];
  }
  const double tot = dlip_block_sum4(acc, red);
  if (threadIdx.x == 0) part[b * kParts + g] = tot;
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void specaug_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                            const int32_t* __restrict__ draws, float* __restrict__ y,
                                                            const double* __restrict__ part, int C, long long NF, int cper, int warp,
                                                            int n_freq, int freq_width, int n_time, int time_width, double time_ratio,
                                                            int fill) {
  constexpr int kTile = kThreads * VEC;
  const long long b = blockIdx.z;
  const int n = row_len(lengths, b, NF);
  const int fa = blockIdx.y * cper;
  const int fb = fa + cper < C ? fa + cper : C;
  const long long t0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * VEC;      // the lane's first frame
  const float* xb = x + b * C * NF;
  float* yb = y + b * C * NF;
  // VEC == 4 runs only where NF % 4 == 0 and both bases are 16-byte aligned: t0 < NF then means t0 + 3 < NF, every row base a multiple of 16
  if ((long long)blockIdx.x * kTile >= n) {                       // the zero tail of the row (the same branch for the whole workgroup)
    if (t0 < NF)
      for (int f = fa; f < fb; ++f) {
        float* yr = yb + (long long)f * NF + t0;
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(yr) = make_float4(0.f, 0.f, 0.f, 0.f);
        else *yr = 0.f;
      }
    return;
  }
  const int32_t* dr = draws + b * DLIP_SPECAUG_DRAWS;
  // ---- the row's choices: the same words in every lane
  const int We = n >= 3 ? (warp < (n - 3) / 2 ? warp : (n - 3) / 2) : 0;
  int c = 0, cp = 0;
  bool warped = false;
  if (We >= 1) {
    c = We + 1 + pick(dr[0], n - 2 - 2 * We);
    cp = c + pick(dr[1], 2 * We + 1) - We;
    warped = cp != c;                                             // d == 0: the row stays as it is, bit for bit
  }
  int fm0[kMasks], fm1[kMasks], tm0[kMasks], tm1[kMasks];
  const int fcap = freq_width < C ? freq_width : C;
  const int tr = (int)floor(time_ratio * (double)n);
  const int tcap = time_width < tr ? time_width : tr;
#pragma unroll
  for (int j = 0; j < kMasks; ++j) {
    fm0[j] = fm1[j] = tm0[j] = tm1[j] = 0;
    if (j < n_freq) {
      const int w = pick(dr[2 + 2 * j], fcap + 1);
      fm0[j] = pick(dr[3 + 2 * j], C - w + 1);
      fm1[j] = fm0[j] + w;
    }
    if (j < n_time) {
      const int w = pick(dr[2 + 2 * kMasks + 2 * j], tcap + 1);
      tm0[j] = pick(dr[3 + 2 * kMasks + 2 * j], n - w + 1);
      tm1[j] = tm0[j] + w;
    }
  }
  float fillv = 0.f;
  if (fill == 1) {
    double tot = 0.0;
#pragma unroll
    for (int g = 0; g < kParts; ++g) tot += part[b * kParts + g];
    fillv = (float)(tot / ((double)C * (double)n));
  }
  // ---- the lane's frames, resolved once for every feature
  bool valid[VEC], tmask[VEC];
  int src[VEC];
  float a[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const long long t = t0 + k;
    valid[k] = t < n;
    const int ti = valid[k] ? (int)t : 0;
    bool m = false;
#pragma unroll
    for (int j = 0; j < kMasks; ++j) m = m || (ti >= tm0[j] && ti < tm1[j]);
    tmask[k] = m;
    src[k] = ti;
    a[k] = 0.f;
    if (warped && valid[k]) {
      // s = (t c) / c' up to c', c + ((t - c')(n - 1 - c)) / (n - 1 - c') behind it: 64-bit products, one fp64 division
      const bool left = ti <= cp;
      const long long num = left ? (long long)ti * c : (long long)(ti - cp) * (n - 1 - c);
      const int den = left ? cp : n - 1 - cp;                     // both >= 1: 1 <= c' <= n - 2
      const double s = (left ? 0.0 : (double)c) + (double)num / (double)den;
      int i = (int)s;
      i = i < n - 2 ? i : n - 2;
      src[k] = i;
      a[k] = (float)(s - (double)i);
    }
  }
  if (t0 >= NF) return;
  const bool whole = VEC == 4 && valid[VEC - 1];
  for (int f = fa; f < fb; ++f) {
    bool fm = false;
#pragma unroll
    for (int j = 0; j < kMasks; ++j) fm = fm || (f >= fm0[j] && f < fm1[j]);
    const float* xr = xb + (long long)f * NF;
    float v[VEC];
    if (fm) {                                                     // a masked feature: nothing of it is loaded
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = fillv;
    } else if (!warped) {
      if constexpr (VEC == 4) {
        if (whole) {
          const float4 q = *reinterpret_cast<const float4*>(xr + t0);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) v[k] = valid[k] ? xr[t0 + k] : 0.f;
        }
      } else {
        v[0] = valid[0] ? xr[t0] : 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        v[k] = 0.f;
        if (valid[k] && !tmask[k]) {
          const float x0 = xr[src[k]];
          const float x1 = xr[src[k] + 1];                        // src + 1 <= n - 1
          // a == 0 and a == 1 (frame n - 1) take the sample itself: frames 0, c' and n - 1 hold their sources' bits
          v[k] = a[k] == 0.f ? x0 : (a[k] == 1.f ? x1 : fmaf(a[k], x1 - x0, x0));
        }
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = !valid[k] ? 0.f : (tmask[k] ? fillv : v[k]);
    float* yr = yb + (long long)f * NF + t0;
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(yr) = make_float4(v[0], v[1], v[2], v[3]);
    else *yr = v[0];
  }
}

inline bool sizes_ok(long long B, long long C, long long NF) {
  return B >= 1 && B <= 65535 && C >= 1 && C <= (1ll << 30) && NF >= 1 && NF <= 0x7fffffffll - 4 * kThreads;
}

}  // namespace

extern "C" int64_t dlip_spec_augment_workspace_bytes(int32_t B, int32_t C, int32_t NF) {
  if (!sizes_ok(B, C, NF)) return DLIP_EINVAL;
  return (int64_t)B * kParts * (int64_t)sizeof(double);
}

extern "C" int dlip_spec_augment_f32(const float* x, const int32_t* lengths, const int32_t* draws, float* y, void* workspace,
                                     int64_t workspace_bytes, int32_t B, int32_t C, int32_t NF, int32_t warp, int32_t n_freq,
                                     int32_t freq_width, int32_t n_time, int32_t time_width, double time_ratio, int32_t fill,
                                     dlip_stream_t stream) {
  DLIP_CHECK_ARG(sizes_ok(B, C, NF));
  DLIP_CHECK_ARG(x && draws && y && x != y);
  DLIP_CHECK_ARG(warp >= 0 && freq_width >= 0 && time_width >= 0 && n_freq >= 0 && n_freq <= kMasks && n_time >= 0 && n_time <= kMasks);
  DLIP_CHECK_ARG(time_ratio >= 0.0 && time_ratio <= 1.0 && (fill == 0 || fill == 1));      // (a NaN ratio fails both comparisons)
  DLIP_CHECK_ARG(workspace && dlip_aligned<8>(workspace) && workspace_bytes >= dlip_spec_augment_workspace_bytes(B, C, NF));
  double* part = static_cast<double*>(workspace);
  hipStream_t st = dlip_hip_stream(stream);
  if (fill == 1) hipLaunchKernelGGL(specaug_mean_kernel, dim3(kParts, B), dim3(kThreads), 0, st, x, lengths, part, C, (long long)NF);
  const bool wide = NF % 4 == 0 && dlip_aligned16(x, y);
  const int tile = kThreads * (wide ? 4 : 1);
  const int tiles = (int)(((long long)NF + tile - 1) / tile);
  // about eight workgroups per compute unit: the features of a row are dealt out in contiguous ranges until the grid is that large
  long long split = (2048 + (long long)tiles * B - 1) / ((long long)tiles * B);
  split = split < 1 ? 1 : (split > C ? C : split);
  int cper = (int)((C + split - 1) / split);
  if ((C + cper - 1) / cper > 65535) cper = (C + 65534) / 65535;
  const dim3 grid(tiles, (C + cper - 1) / cper, B);
#define DLIP_SPECAUG_LAUNCH(VEC)                                                                                                   \
  hipLaunchKernelGGL(specaug_kernel<VEC>, grid, dim3(kThreads), 0, st, x, lengths, draws, y, part, C, (long long)NF, cper, warp, n_freq, \
                     freq_width, n_time, time_width, time_ratio, fill)
  if (wide) DLIP_SPECAUG_LAUNCH(4);
  else DLIP_SPECAUG_LAUNCH(1);
#undef DLIP_SPECAUG_LAUNCH
  return dlip_launch_status();
}

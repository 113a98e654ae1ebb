// Kaldi-style sliding-window CMN and energy-VAD frame selection on ragged feature batches (ABI 62).
//
// The reference's speech pipeline feeds its encoder and its PLDA back-end through
//     apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ... | select-voiced-frames ... vad.scp
// (conf/audio_config.yaml:21 `plda_input`, :25 `nn_input`).  It ships no source for these tools and Kaldi is not a dependency: the
// definition is the one restated in include/deeplip_hip.h and DESIGN.md from Kaldi's published SlidingWindowCmn and ComputeVadEnergy.
//
// x [B, C, NF] fp32 (time contiguous, the front-end's output) + one frame count per row, every row computed as if it were alone:
//   vad_select_kernel   one workgroup per row: fp64 mean of the log-energy -> threshold -> context vote -> exclusive scan of the mask
//                       over the row's n frames (chunks of 1024 with a carry) -> pos [B, NF] (destination column, -1 = dropped),
//                       out_len [B], fallback [B];
//   cmn_sliding_kernel  one workgroup per tile of DLIP_CMN_TILE frames of one (b, c) row: the tile and its window halo go through LDS
//                       once, the workgroup forms their fp64 prefix sums there (a window sum is then the difference of two of them:
//                       what a frame costs does not grow with the window; windows of <= kDirect frames are summed frame by
//                       frame), each thread owns kRun consecutive frames; stores go to
//                       y[b, c, pos[t]] and the row's tail leaves as zeros.  kMode 0 is the selection alone (a gather of x, no LDS).
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int kRun = DLIP_CMN_TILE / 256;                       // consecutive frames per thread
constexpr int kVadRun = 4;                                      // frames a thread decides per chunk of the VAD's scan
constexpr int kDirect = 16;                                     // windows up to this long are summed frame by frame
static_assert(DLIP_CMN_TILE % 256 == 0 && kRun == 4, "one float4 per thread");
static_assert(DLIP_CMN_TILE >= DLIP_CMN_MAX_WINDOW, "tile_span below: behind the first tile min_window no longer reaches forward");

__host__ __device__ __forceinline__ int clamp_len(int v, int hi) { return v < 1 ? 1 : (v > hi ? hi : v); }
// LDS images of a tile and its halo.  Floats: one pad word per 32; doubles: one pad entry per 16 -- consecutive lanes, a few frames
// apart, then fall on different banks.
__host__ __device__ __forceinline__ int pad(int a) { return a + (a >> 5); }
__host__ __device__ __forceinline__ int padd(int a) { return a + (a >> 4); }
// the frames one tile's windows reach over at most (tile_span below), a multiple of 32, and the LDS bytes of that many
__host__ __device__ __forceinline__ int tile_span(int window, int center, int min_window) {
  const int w = (!center && min_window > window) ? min_window : window;
  return (DLIP_CMN_TILE + 2 * w + 31) & ~31;
}
__host__ __device__ __forceinline__ int prefix_entries(int span) { return padd(span) + 1; }
inline size_t lds_bytes(int span, bool vars) { return sizeof(double) * prefix_entries(span) * (vars ? 2 : 1) + sizeof(float) * (pad(span) + 1); }

// The window of frame t of an n-frame row (Kaldi SlidingWindowCmn): [b, e), 0 <= b <= t < e <= n.  b and e never decrease with t.
__device__ __forceinline__ void window_bounds(int t, int n, int window, int center, int min_window, int& b, int& e) {
  if (center) {
    b = t - window / 2;
    e = b + window;
  } else {
    b = t - window;
    e = t + 1;
  }
  if (b < 0) {
    e -= b;
    b = 0;
  }
  if (!center && e > t) e = max(t + 1, min_window);
  if (e > n) {
    b -= e - n;
    e = n;
    if (b < 0) b = 0;
  }
}

// e [B rows, e_stride apart]: the log-energy; mask [B, NF]: an external decision instead (then e is not read).
__global__ __launch_bounds__(256) void vad_select_kernel(const float* __restrict__ e, long long e_stride, const uint8_t* __restrict__ mask,
                                                         const int32_t* __restrict__ lengths, double thr0, double mean_scale, int ctx,
                                                         float proportion, int min_keep, int32_t* __restrict__ pos,
                                                         int32_t* __restrict__ out_len, int32_t* __restrict__ fallback, int NF) {
#pragma clang fp contract(off)
  __shared__ double redd[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;
  const int n = lengths ? clamp_len(lengths[b], NF) : NF;
  const float* er = e ? e + b * e_stride : nullptr;
  const uint8_t* mr = mask ? mask + b * NF : nullptr;
  int32_t* pr = pos + b * NF;
  float thr = (float)thr0;
  if (!mr && mean_scale != 0.0) {
    // thread i sums frames i, i + 256, .. front to back, the 256 partial sums meet in lane and wave order: n alone decides the order
    double s = 0.0;
    for (int t = tid; t < n; t += 256) s += (double)er[t];
    s = dlip_block_sum4(s, redd);
    thr = (float)(thr0 + mean_scale * (s / n));
  }
  if (ctx > NF) ctx = NF;                                       // (t + ctx stays an int)
  // the scan walks the row in chunks of 256 * kVadRun frames with a carry: a thread decides kVadRun consecutive frames, the
  // workgroup scans the threads' counts (within the wave, then over the four wave totals)
  int carry = 0;
  for (int base = 0; base < n; base += 256 * kVadRun) {
    const int ts = base + tid * kVadRun;
    int v[kVadRun], cnt = 0;
#pragma unroll
    for (int j = 0; j < kVadRun; ++j) {
      const int t = ts + j;
      v[j] = 0;
      if (t < n) {
        if (mr) {
          v[j] = mr[t] != 0;
        } else {
          const int lo = max(0, t - ctx), hi = min(n - 1, t + ctx);
          int num = 0;
          for (int u = lo; u <= hi; ++u) num += er[u] > thr ? 1 : 0;
          v[j] = (float)num >= (float)(hi - lo + 1) * proportion ? 1 : 0;      // Kaldi's BaseFloat product
        }
      }
      cnt += v[j];
    }
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) redi[wave] = incl;
    __syncthreads();
    int p = carry + incl - cnt;                                  // the column of the thread's first kept frame
    for (int w = 0; w < wave; ++w) p += redi[w];
    carry += redi[0] + redi[1] + redi[2] + redi[3];
#pragma unroll
    for (int j = 0; j < kVadRun; ++j) {
      if (ts + j < n) pr[ts + j] = v[j] ? p : -1;
      p += v[j];
    }
    __syncthreads();                                             // redi is written again by the next chunk
  }
  // select-voiced-frames drops an utterance without voiced frames; a batch cannot drop a row: below min_keep the row keeps all n
  const bool fb = carry < min_keep;
  if (fb)                                                        // (each thread rewrites the entries it wrote itself)
    for (int base = 0; base < n; base += 256 * kVadRun)
      for (int t = base + tid * kVadRun; t < min(base + (tid + 1) * kVadRun, n); ++t) pr[t] = t;
  for (int t = n + tid; t < NF; t += 256) pr[t] = -1;
  if (tid == 0) {
    out_len[b] = fb ? n : carry;
    fallback[b] = fb ? 1 : 0;
  }
}

// Exclusive prefix of one double per thread over the workgroup, in thread order: within the wave by doubling steps, the wave totals
// front to back.  red[4]; ends after its reads of red[] (a caller that writes it again puts a barrier behind).
__device__ __forceinline__ double block_exclusive_scan(double v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) red[wave] = incl;
  double excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 0.0;
  __syncthreads();
  double base = 0.0;
  for (int w = 0; w < wave; ++w) base += red[w];
  return base + excl;
}

// kMode 0: the selection alone (values copied), 1: sliding mean, 2: sliding mean and variance (--norm-vars).
// kVec: NF % 4 == 0 and 16-byte aligned tensors -- the tile is loaded (and, without a selection, stored) in float4; whole quads
// only, so no load ever touches a frame >= the last window's end <= n.
// span (kMode > 0): the capacity of the dynamic LDS in frames, tile_span() of the options.
template <int kMode, bool kVec>
__global__ __launch_bounds__(256) void cmn_sliding_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                          const int32_t* __restrict__ pos, const int32_t* __restrict__ out_len,
                                                          float* __restrict__ y, int C, int NF, int tiles, int window, int center,
                                                          int min_window, int span) {
#pragma clang fp contract(off)
  extern __shared__ double lds[];
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const long long row = blockIdx.x / tiles, b = row / C;
  const int t0 = (int)(blockIdx.x % tiles) * DLIP_CMN_TILE;
  const int n = lengths ? clamp_len(lengths[b], NF) : NF;
  const int ol = pos ? min(max(out_len[b], 0), n) : n;
  const int t1 = min(t0 + DLIP_CMN_TILE, n);                     // this tile computes frames [t0, t1)
  const float* xr = x + row * NF;
  float* yr = y + row * NF;
  const int ts = t0 + tid * kRun;
  float r[kRun];
#pragma unroll
  for (int j = 0; j < kRun; ++j) r[j] = 0.f;
  if (kMode == 0) {
    if (kVec && ts + kRun <= t1) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xr + ts);
#pragma unroll
      for (int j = 0; j < kRun; ++j) r[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < kRun; ++j)
        if (ts + j < t1) r[j] = xr[ts + j];
    }
  } else if (t0 < n) {
    double* P = lds;                                             // P[a] = sum of the tile image's first a frames; Q: of their squares
    double* Q = lds + prefix_entries(span);
    float* sx = reinterpret_cast<float*>(lds + (kMode == 2 ? 2 : 1) * prefix_entries(span));
    // tile_span: window bounds never decrease with t, so the tile reads [begin(t0), end(t1 - 1)): at most `window` frames in front of
    // t0 and max(window, min_window) behind t1 - 1 (the first tile of a non-centred row: max(tile, min_window) frames in all)
    int lo, hi, unused;
    window_bounds(t0, n, window, center, min_window, lo, unused);
    window_bounds(t1 - 1, n, window, center, min_window, unused, hi);
    const int cnt = hi - lo;
    if (cnt > span) return;                                      // (cannot happen; keeps the LDS images in bounds whatever the arguments)
    if (kVec) {
      const int qlo = min((lo + 3) & ~3, hi), qhi = max(hi & ~3, qlo);
      for (int a = lo + tid; a < qlo; a += 256) sx[pad(a - lo)] = xr[a];
      for (int q = qlo + 4 * tid; q < qhi; q += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + q);
#pragma unroll
        for (int k = 0; k < 4; ++k) sx[pad(q + k - lo)] = v[k];
      }
      for (int a = qhi + tid; a < hi; a += 256) sx[pad(a - lo)] = xr[a];
    } else {
      for (int a = lo + tid; a < hi; a += 256) sx[pad(a - lo)] = xr[a];
    }
    __syncthreads();
    // prefix sums over the image, fp64: thread k sums its `per` consecutive frames front to back, the 256 totals are scanned in thread
    // order, the thread walks its frames again from its base.  The order is fixed by (lo, hi) = by (tile of t, n, options) alone.
    // What is summed is x - pivot, pivot = the image's first frame: mean and variance do not move with it, and the prefixes stay
    // the size of the signal's variation, not of its offset, so the difference of two of them keeps the digits the variance needs.
    const double pivot = (double)sx[0];
    const int per = (cnt + 255) / 256;
    const int a0 = min(tid * per, cnt), a1 = min(a0 + per, cnt);
    double s = 0.0, q = 0.0;
    for (int a = a0; a < a1; ++a) {
      const double v = (double)sx[pad(a)] - pivot;
      s += v;
      if (kMode == 2) q += v * v;
    }
    s = block_exclusive_scan(s, red);
    if (kMode == 2) q = block_exclusive_scan(q, red + 4);
    for (int a = a0; a < a1; ++a) {
      P[padd(a)] = s;
      if (kMode == 2) Q[padd(a)] = q;
      const double v = (double)sx[pad(a)] - pivot;
      s += v;
      if (kMode == 2) q += v * v;
    }
    if (a0 < a1 && a1 == cnt) {                                  // the thread that owns the image's last frame closes the arrays
      P[padd(cnt)] = s;
      if (kMode == 2) Q[padd(cnt)] = q;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      const int t = ts + j;
      if (t < t1) {
        int wb, we;
        window_bounds(t, n, window, center, min_window, wb, we);
        const int w = we - wb;
        double c = pivot, sum, sq = 0.0;
        if (w <= kDirect) {                                      // a short window: its frames themselves, front to back
          c = 0.0, sum = 0.0;
          for (int u = wb; u < we; ++u) {
            const double v = (double)sx[pad(u - lo)];
            sum += v;
            if (kMode == 2) sq += v * v;
          }
        } else {
          sum = P[padd(we - lo)] - P[padd(wb - lo)];
          if (kMode == 2) sq = Q[padd(we - lo)] - Q[padd(wb - lo)];
        }
        const double mean = sum / w;                             // of x - c
        double d = ((double)sx[pad(t - lo)] - c) - mean;
        if (kMode == 2) d = w == 1 ? 0.0 : d * (1.0 / sqrt(fmax(sq / w - mean * mean, 1e-10)));
        r[j] = (float)d;
      }
    }
  }
  if (!pos) {
    // in place: frames [t0, t1) hold values, the rest of the tile's columns (t >= n) zeros
    if (kVec) {
      if (ts < NF) *reinterpret_cast<f32x4*>(yr + ts) = f32x4{r[0], r[1], r[2], r[3]};
    } else {
#pragma unroll
      for (int j = 0; j < kRun; ++j)
        if (ts + j < NF) yr[ts + j] = r[j];
    }
    return;
  }
  const int32_t* pr = pos + b * NF;
#pragma unroll
  for (int j = 0; j < kRun; ++j) {
    if (ts + j < t1) {
      const int p = pr[ts + j];
      if (p >= 0 && p < ol) yr[p] = r[j];                         // kept columns lie below out_len, the zeros below at and above it
    }
  }
  for (int c = max(t0, ol) + tid; c < min(t0 + DLIP_CMN_TILE, NF); c += 256) yr[c] = 0.f;
}

}  // namespace

extern "C" int dlip_vad_energy_select_i32(const float* log_energy, int64_t energy_stride, const uint8_t* voiced, const int32_t* lengths,
                                          double energy_threshold, double energy_mean_scale, int32_t context, float proportion_threshold,
                                          int32_t min_keep, int32_t* pos, int32_t* out_len, int32_t* fallback, int32_t B, int32_t NF,
                                          dlip_stream_t stream) {
  DLIP_CHECK_ARG((log_energy || voiced) && pos && out_len && fallback && B > 0 && NF > 0 && NF <= (1 << 30));
  DLIP_CHECK_ARG(voiced || energy_stride >= NF);
  DLIP_CHECK_ARG(context >= 0 && min_keep >= 1 && proportion_threshold >= 0.f && proportion_threshold <= 1.f);
  DLIP_CHECK_ARG(energy_threshold == energy_threshold && energy_mean_scale == energy_mean_scale);      // (no NaN)
  hipLaunchKernelGGL(vad_select_kernel, dim3((unsigned)B), dim3(256), 0, dlip_hip_stream(stream), log_energy, (long long)energy_stride,
                     voiced, lengths, energy_threshold, energy_mean_scale, context, proportion_threshold, min_keep, pos, out_len, fallback,
                     NF);
  return dlip_launch_status();
}

extern "C" int dlip_cmn_sliding_select_f32(const float* x, const int32_t* lengths, const int32_t* pos, const int32_t* out_len, float* y,
                                           int32_t B, int32_t C, int32_t NF, int32_t window, int32_t center, int32_t min_window,
                                           int32_t norm_vars, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && x != y && B > 0 && C > 0 && NF > 0 && (pos == nullptr) == (out_len == nullptr));
  DLIP_CHECK_ARG(window >= 0 && window <= DLIP_CMN_MAX_WINDOW && min_window >= 1 && min_window <= DLIP_CMN_MAX_WINDOW);
  const long long rows = (long long)B * C;
  const int tiles = (NF + DLIP_CMN_TILE - 1) / DLIP_CMN_TILE;
  DLIP_CHECK_ARG(rows * tiles < (1ll << 31));
  const bool vec = NF % 4 == 0 && dlip_aligned16(x, y);
  const int mode = window == 0 ? 0 : (norm_vars ? 2 : 1);
  const int span = mode ? tile_span(window, center != 0, min_window) : 0;
  const size_t lds = mode ? lds_bytes(span, mode == 2) : 0;      // <= 54 KiB at the caps: inside the 64 KiB a launch may ask for
  auto kernel = mode == 0 ? (vec ? cmn_sliding_kernel<0, true> : cmn_sliding_kernel<0, false>)
              : mode == 1 ? (vec ? cmn_sliding_kernel<1, true> : cmn_sliding_kernel<1, false>)
                          : (vec ? cmn_sliding_kernel<2, true> : cmn_sliding_kernel<2, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(rows * tiles)), dim3(256), lds, dlip_hip_stream(stream), x, lengths, pos, out_len, y, C, NF,
                     tiles, window, center != 0, min_window, span);
  return dlip_launch_status();
}

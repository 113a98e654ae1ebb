// Waveform resampling in front of the audio front-end (ABI 63): rate conversion of a file whose rate differs
// from the configured one (models/audio_models/datasets.py:459-463, librosa.resample(data, rate, self.rate)) and the speed
// perturbation of an x-vector recipe (sox `speed 0.9 / 1.0 / 1.1`) are one operation, a rational polyphase FIR resampler
//
//   y[m] = sum_i x[i] h[c + m down - i up],  0 <= m < n_out = ceil(n up / down),  x zero outside [0, n), h zero outside [0, L)
//        = sum_{j < K} tab[r][j] x[i_hi - j],  q = c + m down, r = q mod up, i_hi = q div up, tab[r][j] = h[r + j up], K = ceil(L / up)
//
// on a batch wave [B, S] + optional sample counts, each row with the ratio `ratio_idx` names in a bank of Q ratios (-1: the row passes
// through).  A row leaves with a different length, written to out_lengths on the device and never read on the host.  Exact fp32 on the
// vector ALUs: one fmaf per product, j ascending from an accumulator of 0.f, for every output alike -- a row has the same bits whatever
// B, S, S_out, Q, the tile length and its neighbours are.  Every index product (m down, n up, q) is formed in 64 bits.
//
// A 256-lane workgroup owns tiles of `tile` consecutive outputs of one row (consecutive lanes consecutive outputs, tile / 256 per lane)
// and walks the row's tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the row's polyphase table (up x Kp words, the phase stride
// Kp = K | 1 odd so that lanes on different phases spread over the LDS banks; up = 1 has one phase and takes its taps as wave-uniform
// loads instead) is staged in LDS once per workgroup, the input span of each tile (ceil((tile - 1) down / up) + K words at most, zero-filled outside the row) once per tile.
#include "dlip_launch.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ int row_len(const int32_t* lengths, long long b, long long S) {
  if (lengths == nullptr) return (int)S;
  const int v = lengths[b];
  return v < 1 ? 1 : (v > S ? (int)S : v);
}

// words of input a tile of `tile` outputs reaches over: i_hi moves by at most ceil((tile - 1) down / up) within it, K taps behind it
__host__ __device__ __forceinline__ long long span_of(long long up, long long down, long long K, long long tile) {
  return ((tile - 1) * down + up - 1) / up + K;
}

template <int PER>
__global__ __launch_bounds__(kThreads) void resample_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                             const float* __restrict__ tabs, const int32_t* __restrict__ bank,
                                                             const int32_t* __restrict__ ratio_idx, float* __restrict__ y,
                                                             int32_t* __restrict__ out_lengths, long long S, long long S_out, int Q,
                                                             int tab_stride, int span_words, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kTile = PER * kThreads;
  const long long b = blockIdx.y;
  const int tid = (int)threadIdx.x;
  const int n = row_len(lengths, b, S);
  const float* xb = x + b * S;
  float* yb = y + b * S_out;
  // every branch below depends on blockIdx and on words the whole workgroup reads alike: the barriers are met by all lanes or none
  int ri = ratio_idx[b];
  bool live = ri >= 0;
  int up = 1, down = 1, c = 0, K = 1;
  if (live) {
    ri = ri < Q ? ri : Q - 1;
    up = bank[4 * ri];
    down = bank[4 * ri + 1];
    c = bank[4 * ri + 2];
    K = bank[4 * ri + 3];
    // a descriptor the launch's LDS split cannot hold is not trusted: the row passes through
    live = up >= 1 && up <= DLIP_RESAMPLE_MAX_FACTOR && down >= 1 && down <= DLIP_RESAMPLE_MAX_FACTOR && c >= 0 && K >= 1 &&
           K <= span_words && (long long)up * (K | 1) <= tab_stride && span_of(up, down, K, kTile) <= span_words;
  }
  long long n_out = live ? ((long long)n * up + down - 1) / down : (long long)n;
  n_out = n_out < S_out ? n_out : S_out;
  if (blockIdx.x == 0 && tid == 0) out_lengths[b] = (int32_t)n_out;
  if (!live) {
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
#pragma unroll
      for (int p = 0; p < PER; ++p) {
        const long long m = (long long)tile * kTile + p * kThreads + tid;
        if (m < S_out) yb[m] = m < n_out ? xb[m] : 0.f;
      }
    return;
  }
  const int Kp = K | 1;
  float* tab = lds;
  float* win = lds + tab_stride;
  const float* tb = tabs + (long long)ri * tab_stride;
  if (up > 1 && (long long)blockIdx.x * kTile < n_out)
    for (int i = tid; i < up * Kp; i += kThreads) tab[i] = tb[i];
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m0 = (long long)tile * kTile;
    if (m0 >= n_out) {                                            // the zero tail of the row
#pragma unroll
      for (int p = 0; p < PER; ++p) {
        const long long m = m0 + p * kThreads + tid;
        if (m < S_out) yb[m] = 0.f;
      }
      continue;
    }
    const int act = n_out - m0 < kTile ? (int)(n_out - m0) : kTile;  // outputs of this tile inside the row
    const long long q0 = (long long)c + m0 * down;
    const long long i0 = q0 / up;
    const unsigned r0 = (unsigned)(q0 - i0 * up);
    const long long lo = i0 - (K - 1);                            // the row sample that window word 0 holds
    const int cnt = (int)((r0 + (unsigned)(act - 1) * (unsigned)down) / (unsigned)up) + K;   // <= span_of(up, down, K, kTile)
    __syncthreads();                                              // the tile before has been read
    for (int w = tid; w < cnt; w += kThreads) {
      const long long s = lo + w;
      win[w] = (s >= 0 && s < n) ? xb[s] : 0.f;
    }
    __syncthreads();                                              // (the first one covers the table as well)
    // output d of the tile: t = r0 + d down < 2^23, phase t mod up, newest sample at window word t div up + K - 1
    unsigned e[PER], rk[PER];
    float acc[PER];
#pragma unroll
    for (int p = 0; p < PER; ++p) {
      int d = p * kThreads + tid;
      d = d < act ? d : act - 1;                                  // lanes past the row compute a staged output and drop it
      const unsigned t = r0 + (unsigned)d * (unsigned)down;
      const unsigned qd = t / (unsigned)up;
      e[p] = qd + (unsigned)(K - 1);
      rk[p] = (t - qd * (unsigned)up) * (unsigned)Kp;
      acc[p] = 0.f;
    }
    if (up == 1) {
      // one phase: the tap is the same word for every lane -- a wave-uniform load instead of an LDS read (same products, same order)
      for (int j = 0; j < K; ++j) {
        const float hj = tb[j];
#pragma unroll
        for (int p = 0; p < PER; ++p) acc[p] = fmaf(hj, win[e[p] - j], acc[p]);
      }
    } else {
      for (int j = 0; j < K; ++j)
#pragma unroll
        for (int p = 0; p < PER; ++p) acc[p] = fmaf(tab[rk[p] + j], win[e[p] - j], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < PER; ++p) {
      const int d = p * kThreads + tid;
      const long long m = m0 + d;
      if (m < S_out) yb[m] = d < act ? acc[p] : 0.f;
    }
  }
}

inline bool tile_ok(int tile) { return tile == 256 || tile == 512 || tile == 1024; }

}  // namespace

extern "C" int64_t dlip_wave_resample_span_words(int32_t up, int32_t down, int32_t K, int32_t tile) {
  if (up < 1 || up > DLIP_RESAMPLE_MAX_FACTOR || down < 1 || down > DLIP_RESAMPLE_MAX_FACTOR || K < 1 || !tile_ok(tile) ||
      tile > DLIP_RESAMPLE_TILE)
    return DLIP_EINVAL;
  return span_of(up, down, K, tile);
}

extern "C" int32_t dlip_wave_resample_fits(int32_t up, int32_t down, int32_t L) {
  if (up < 1 || up > DLIP_RESAMPLE_MAX_FACTOR || down < 1 || down > DLIP_RESAMPLE_MAX_FACTOR || L < 1) return 0;
  const long long K = ((long long)L + up - 1) / up;
  const long long table = (long long)up * (K | 1);
  for (int tile = DLIP_RESAMPLE_TILE; tile >= 256; tile >>= 1)
    if (table + span_of(up, down, K, tile) <= DLIP_RESAMPLE_LDS_WORDS) return tile;
  return 0;
}

extern "C" int dlip_wave_resample_f32(const float* wave, const int32_t* lengths, const float* tabs, const int32_t* bank,
                                      const int32_t* ratio_idx, float* out, int32_t* out_lengths, int32_t B, int64_t S, int64_t S_out,
                                      int32_t Q, int32_t tab_stride, int32_t span_words, int32_t tile, dlip_stream_t stream) {
  DLIP_CHECK_ARG(wave && tabs && bank && ratio_idx && out && out_lengths && wave != out);
  DLIP_CHECK_ARG(B > 0 && B <= 65535 && Q > 0 && tile_ok(tile) && tile <= DLIP_RESAMPLE_TILE);
  DLIP_CHECK_ARG(S > 0 && S <= 0x7fffffffll - tile && S_out > 0 && S_out <= 0x7fffffffll - tile);
  DLIP_CHECK_ARG(tab_stride > 0 && span_words > 0 && (long long)tab_stride + span_words <= DLIP_RESAMPLE_LDS_WORDS);
  const int ntiles = (int)((S_out + tile - 1) / tile);
  // about eight workgroups per compute unit over the batch; a workgroup stages its row's table once for the tiles it walks, and
  // the row's tiles are dealt out evenly: no more workgroups than the longest walk needs
  const int cap = (2048 + B - 1) / B;
  const int walk = (ntiles + cap - 1) / cap;
  const dim3 grid((ntiles + walk - 1) / walk, B);
  const size_t lds = ((size_t)tab_stride + span_words) * sizeof(float);
#define DLIP_RESAMPLE_LAUNCH(PER)                                                                                                  \
  hipLaunchKernelGGL(resample_kernel<PER>, grid, dim3(kThreads), lds, dlip_hip_stream(stream), wave, lengths, tabs, bank, ratio_idx, \
                     out, out_lengths, (long long)S, (long long)S_out, Q, tab_stride, span_words, ntiles)
  if (tile == 1024) DLIP_RESAMPLE_LAUNCH(4);
  else if (tile == 512) DLIP_RESAMPLE_LAUNCH(2);
  else DLIP_RESAMPLE_LAUNCH(1);
#undef DLIP_RESAMPLE_LAUNCH
  return dlip_launch_status();
}

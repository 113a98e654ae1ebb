// GPU-side preprocessing at the entrance of the hot path.
//
// Audio: the reference extracts MFCC / (log-)fbank features per utterance on CPU workers with the
// third-party python_speech_features package (models/audio_models/datasets.py:65-83: mfcc(winlen 0.025,
// winstep 0.01, numcep 24) with that package's defaults nfilt 26, nfft 512, preemph 0.97,
// ceplifter 22, appendEnergy, rectangular window; then per-utterance mean/variance normalisation,
// datasets.py:52-53).  Here the chain is: framing + pre-emphasis (this file) -> 512-point real DFT as
// ONE fp32 MFMA GEMM against a [514 x 512] cos/sin matrix -> power spectrum + frame energy (this
// file) -> mel filterbank GEMM -> log -> DCT-II(+lifter) GEMM -> c0 := log energy -> CMVN (this file).
// The GEMMs reuse dlip_conv_nhwc_f32 (host side: deeplip_amd/frontend.py).
//
// Video: uint8 gray or RGB frames -> centre crop -> /255 -> (x - 0.421)/0.165
// (models/video_models/dataloaders.py:11-22: Normalize(0,255), CenterCrop(88), Normalize(0.421,0.165)).
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

// RAGGED WAVEFORM BATCHES.  The kernels below that carry a `kRagged` switch serve two entry points each: <false> is the rectangular
// kernel (no length is read, every row is whole), <true> reads one length per row of a zero-padded batch and computes each row as if
// it had been run alone -- the reference's loop extracts one utterance at a time (train_fusion.py:334-349, train_audio.py:343-373).
// sigproc.framesig's frame count of an s-sample signal: 1 + ceil((s - L) / step) above one frame length, else 1.
__device__ __forceinline__ int wave_frames(long long s, int L, int step) {
  return s <= L ? 1 : 1 + (int)((s - L + step - 1) / step);
}
__device__ __forceinline__ long long clamp_len(int v, long long hi) { return v < 1 ? 1 : (v > hi ? hi : v); }

// sample lengths [B] -> frame lengths [B] on the device: a recorded plan follows whatever lengths its buffer holds at replay time
__global__ __launch_bounds__(256) void wave_frame_lengths_kernel(const int32_t* __restrict__ slen, int32_t* __restrict__ flen, int B,
                                                                 long long S, int L, int step) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) flen[b] = wave_frames(clamp_len(slen[b], S), L, step);
}

// frames[b*NF + f][j] = (j < L ? pre(b, f*step + j) : 0), pre(n) = x[n] - coef*x[n-1] (x[-1] -> x[0] alone,
// samples beyond the signal are zero padding as python_speech_features.sigproc.framesig does).
// kRagged: row b ends at S_b = clamp(slen[b], 1, S).  The reference pre-emphasises the S_b-sample signal and framesig zero-pads
// AFTERWARDS, so position S_b holds 0 and not -coef * x[S_b - 1]; samples >= S_b are never read (the caller's padding may hold
// anything) and frames f >= NF_b are all zero.
template <bool kRagged>
__global__ __launch_bounds__(256) void frame_preemph_kernel(const float* __restrict__ x, const int32_t* __restrict__ slen,
                                                            float* __restrict__ y, int S, int NF, int L, int step, int nfft, float coef,
                                                            long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int j = (int)(i % nfft);
    const long long r = i / nfft;
    const int f = (int)(r % NF);
    const long long b = r / NF;
    float v = 0.f;
    const int n = f * step + j;
    int Sb = S;
    bool live = true;
    if (kRagged) {
      Sb = (int)clamp_len(slen[b], S);
      live = f < wave_frames(Sb, L, step);
    }
    if (live && j < L && n < Sb) {
      const float* xb = x + b * S;
      v = n == 0 ? xb[0] : xb[n] - coef * xb[n - 1];
    }
    y[i] = v;
  }
}

// spec [R, 2*NB] = (re_0..re_{NB-1}, im_0..im_{NB-1}) -> pow [R, NBp] = (re^2 + im^2)/nfft (zero padded to NBp),
// energy[r] = sum_k pow (0 -> eps), as python_speech_features.sigproc.powspec / base.fbank.
__global__ __launch_bounds__(256) void powspec_kernel(const float* __restrict__ spec, float* __restrict__ pw,
                                                      float* __restrict__ energy, int R, int NB, int NBp, float inv_nfft) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* s = spec + (long long)r * 2 * NB;
  double e = 0.0;
  for (int k = lane; k < NBp; k += 64) {
    float p = 0.f;
    if (k < NB) {
      p = (s[k] * s[k] + s[NB + k] * s[NB + k]) * inv_nfft;
      e += (double)p;
    }
    pw[(long long)r * NBp + k] = p;
  }
  e = dlip_wave_sum_f64(e);
  if (lane == 0) energy[r] = e == 0.0 ? 2.220446049250313e-16f : (float)e;
}

// Power spectrum with the DFT carried in fp64 (numpy's rfft, which python_speech_features calls, runs in double): one
// workgroup per frame, the frame and the nfft twiddles (cos, sin of 2 pi j / nfft) in LDS, one thread per bin.  For banks
// whose lowest filters sit on bins holding ~1e-9 of the spectrum (80 bands at nfft = 512) the fp32-GEMM DFT's rounding
// noise is the signal; this path holds 1e-4 there too (nfft a power of two, <= 1024).
__global__ __launch_bounds__(256) void powspec_dft64_kernel(const float* __restrict__ frames, float* __restrict__ pw,
                                                            float* __restrict__ energy, int NB, int NBp, int nfft) {
  extern __shared__ double sh[];          // [nfft] frame | [nfft] cos | [nfft] sin | [4] wave sums
  double* fr = sh;
  double* cs = sh + nfft;
  double* sn = sh + 2 * nfft;
  double* part = sh + 3 * nfft;
  const int r = blockIdx.x;
  for (int j = threadIdx.x; j < nfft; j += 256) {
    fr[j] = (double)frames[(long long)r * nfft + j];
    double s, c;
    sincospi(2.0 * (double)j / (double)nfft, &s, &c);
    cs[j] = c;
    sn[j] = s;
  }
  __syncthreads();
  double e = 0.0;
  for (int k = threadIdx.x; k < NBp; k += 256) {
    float p = 0.f;
    if (k < NB) {
      double re = 0.0, im = 0.0;
      for (int n = 0; n < nfft; ++n) {
        const int idx = (k * n) & (nfft - 1);
        re += fr[n] * cs[idx];
        im -= fr[n] * sn[idx];
      }
      const double pp = (re * re + im * im) / (double)nfft;
      p = (float)pp;
      e += pp;
    }
    pw[(long long)r * NBp + k] = p;
  }
  const double t = dlip_block_sum4(e, part);
  if (threadIdx.x == 0) energy[r] = t == 0.0 ? 2.220446049250313e-16f : (float)t;
}

// THE FFT CORE of the two waveform kernels below (power spectrum, log-magnitude STFT): sample j of the frame, an fp64 value that
// `sample(j)` forms, goes into LDS at the bit-reversed position (imaginary part 0), the nfft / 2 twiddles exp(-2 pi i j / nfft) into a
// table (sincospi), and log2(nfft) radix-2 decimation-in-time stages of nfft / 2 butterflies (one per thread and stage at nfft / 2
// threads) leave the spectrum in re / im in natural order.  Every thread of the workgroup calls it; it ends behind a barrier.
template <class Sample>
__device__ __forceinline__ void fft64_frame_lds(double* re, double* im, double* cs, double* sn, int nfft, int lg, Sample sample) {
  const int half = nfft >> 1;
  for (int j = threadIdx.x; j < nfft; j += blockDim.x) {
    const double v = sample(j);
    const int br = (int)(__brev((unsigned)j) >> (32 - lg));
    re[br] = v;
    im[br] = 0.0;
    if (j < half) {
      double s, c;
      sincospi(-2.0 * (double)j / (double)nfft, &s, &c);       // exp(-2 pi i j / nfft)
      cs[j] = c;
      sn[j] = s;
    }
  }
  __syncthreads();
  for (int st = 1; st <= lg; ++st) {
    const int len = 1 << st, hl = len >> 1, tw = nfft >> st;
    for (int t = threadIdx.x; t < half; t += blockDim.x) {
      const int pos = t & (hl - 1), i0 = ((t >> (st - 1)) << st) + pos, i1 = i0 + hl;
      const double wr = cs[pos * tw], wi = sn[pos * tw];
      const double br_ = re[i1] * wr - im[i1] * wi, bi_ = re[i1] * wi + im[i1] * wr;
      const double ar = re[i0], ai = im[i0];
      re[i0] = ar + br_; im[i0] = ai + bi_;
      re[i1] = ar - br_; im[i1] = ai - bi_;
    }
    __syncthreads();
  }
}

// Power spectrum STRAIGHT FROM THE WAVEFORM, in the reference's own precision: python_speech_features pre-emphasises, frames and
// transforms in fp64 (numpy), so a band that holds 1e-12 of a frame's energy -- the lowest one-bin mel filter next to DC in a frame where
// pre-emphasis leaves nothing -- is still resolved there, while fp32 pre-emphasis alone puts rounding noise at -143 dB of the frame under
// it (tools/probes/frontend_fuzz.py: such elements came out 0.3 .. 1 % off in energy).  One workgroup per frame: the frame's samples are
// pre-emphasised in fp64 (coefficient a double: 0.97, not 0.97f) into LDS in bit-reversed order, a radix-2 decimation-in-time FFT of
// nfft points runs there (log2(nfft) stages of nfft / 2 butterflies, one per thread and stage; twiddles from an LDS table of
// sincospi), and the first NB bins leave as |.|^2 / nfft in fp32 together with the frame's energy (summed in fp64).
// kRagged: as frame_preemph_kernel -- the row ends at S_b = clamp(slen[b], 1, S); a frame f >= NF_b runs no FFT and leaves a zero
// power-spectrum row and a zero energy (the dense mel / log / DCT products behind see finite values; the ragged CMVN does not read
// them).  That exit depends on blockIdx alone, so the whole workgroup takes it, and it sits in front of the first barrier.
template <bool kRagged>
__global__ __launch_bounds__(512) void powspec_wave_fft64_kernel(const float* __restrict__ x, const int32_t* __restrict__ slen,
                                                                 float* __restrict__ pw, float* __restrict__ energy,
                                                                 long long S, int NF, int L, int step, int nfft, int lg, double coef, int NB,
                                                                 int NBp) {
  extern __shared__ double sh[];          // [nfft] re | [nfft] im | [nfft / 2] cos | [nfft / 2] sin | [8] wave sums
  double* re = sh;
  double* im = sh + nfft;
  double* cs = sh + 2 * nfft;
  double* sn = cs + nfft / 2;
  double* part = sn + nfft / 2;
  const long long r = blockIdx.x;
  const int f = (int)(r % NF);
  const float* xb = x + (r / NF) * S;
  if (kRagged) {
    S = clamp_len(slen[r / NF], S);
    if (f >= wave_frames(S, L, step)) {
      for (int k = threadIdx.x; k < NBp; k += blockDim.x) pw[r * NBp + k] = 0.f;
      if (threadIdx.x == 0) energy[r] = 0.f;
      return;
    }
  }
  fft64_frame_lds(re, im, cs, sn, nfft, lg, [&](int j) {
    const long long n = (long long)f * step + j;
    double v = 0.0;
    if (j < L && n < S) v = n == 0 ? (double)xb[0] : (double)xb[n] - coef * (double)xb[n - 1];
    return v;
  });
  double e = 0.0;
  for (int k = threadIdx.x; k < NBp; k += blockDim.x) {
    float p = 0.f;
    if (k < NB) {
      const double pp = (re[k] * re[k] + im[k] * im[k]) / (double)nfft;
      p = (float)pp;
      e += pp;
    }
    pw[r * NBp + k] = p;
  }
  e = dlip_wave_sum_f64(e);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) t += part[w];
    energy[r] = t == 0.0 ? 2.220446049250313e-16f : (float)t;
  }
}

// LOG-MAGNITUDE SPECTROGRAM straight from the waveform: the loaders' `stft` feature type (models/audio_models/datasets.py:72-76:
// librosa.stft(y, n_fft, hop_length, win_length) -> magphase -> log1p, with librosa's defaults center=True, pad_mode="reflect",
// window="hann").  The geometry is the loader's: hop and win truncate rate * win_shift / rate * win_len (datasets.py:73), a signal of
// s samples has 1 + s / hop frames, and frame t covers the reflect-padded signal from t hop - nfft / 2 on.
__device__ __forceinline__ long long stft_clamp_len(int v, int nfft, long long hi) {
  const long long lo = (nfft >> 1) + 1;           // one reflection per side reaches every sample of a frame: the host checks S >= lo
  return v < lo ? lo : (v > hi ? hi : v);
}

__global__ __launch_bounds__(256) void stft_frame_lengths_kernel(const int32_t* __restrict__ slen, int32_t* __restrict__ flen, int B,
                                                                 long long S, int nfft, int hop) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) flen[b] = 1 + (int)(stft_clamp_len(slen[b], nfft, S) / hop);
}

// One workgroup per (row, frame), as powspec_wave_fft64_kernel and through the same FFT core, fp64 inside: sample j of frame f is
// y[reflect(f hop + j - nfft / 2)] (about 0 and about S - 1, the edge sample not repeated) times the periodic Hann window of `win`
// points centred in the nfft-point frame (0.5 - 0.5 cos(2 pi k / win) at j = lp + k, lp = (nfft - win) / 2, zero elsewhere; cospi, so
// the value is the fp64 one); bins k < F leave as (float)log1p(sqrt(re^2 + im^2)), the one rounding to fp32 of the pipeline; the pad
// columns F .. Fp - 1 are zeros.  The reflected index stays inside the row: f hop <= S (the host checks NF == 1 + S / hop) and
// S >= nfft / 2 + 1 give 0 <= n < S after one reflection.
// kRagged: the row ends at S_b = clamp(slen[b], nfft / 2 + 1, S), has 1 + S_b / hop frames and is reflected about ITS OWN end; samples
// >= S_b are never read.  A frame past the row's count leaves a zero row; that exit depends on blockIdx alone and sits in front of the
// first barrier.
template <bool kRagged>
__global__ __launch_bounds__(512) void stft_logmag_wave_kernel(const float* __restrict__ x, const int32_t* __restrict__ slen,
                                                               float* __restrict__ out, long long S, int NF, int win, int hop, int nfft,
                                                               int lg, int F, int Fp) {
  extern __shared__ double sh[];          // [nfft] re | [nfft] im | [nfft / 2] cos | [nfft / 2] sin
  double* re = sh;
  double* im = sh + nfft;
  double* cs = sh + 2 * nfft;
  double* sn = cs + nfft / 2;
  const long long r = blockIdx.x;
  const int f = (int)(r % NF);
  const float* xb = x + (r / NF) * S;
  if (kRagged) {
    S = stft_clamp_len(slen[r / NF], nfft, S);
    if (f >= 1 + (int)(S / hop)) {
      for (int k = threadIdx.x; k < Fp; k += blockDim.x) out[r * Fp + k] = 0.f;
      return;
    }
  }
  const int lp = (nfft - win) >> 1;
  const long long start = (long long)f * hop - (nfft >> 1);
  fft64_frame_lds(re, im, cs, sn, nfft, lg, [&](int j) {
    const int k = j - lp;
    double v = 0.0;
    if (k >= 0 && k < win) {
      long long n = start + j;
      if (n < 0) n = -n;
      else if (n >= S) n = 2 * (S - 1) - n;
      v = (double)xb[n] * (0.5 - 0.5 * cospi(2.0 * (double)k / (double)win));
    }
    return v;
  });
  for (int k = threadIdx.x; k < Fp; k += blockDim.x)
    out[r * Fp + k] = k < F ? (float)log1p(sqrt(re[k] * re[k] + im[k] * im[k])) : 0.f;
}

// y = log(x == 0 ? eps : x) elementwise (base.logfbank / base.mfcc)
__global__ __launch_bounds__(256) void log_floor_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = x[i];
    y[i] = logf(v == 0.f ? 2.220446049250313e-16f : v);
  }
}

// feat [B, NF, C] (c0 optionally replaced by log(energy)) -> CMVN over the NF frames of each utterance:
// (x - mean)/(std_biased + 2e-12) (datasets.py:52-53), written channel-first [B, C, NF] like the
// reference loaders (datasets.py:135).  One thread per (b, c), fp64 statistics.
// kRagged: the statistics run over the row's own n = clamp(flen[b], 1, NF) frames, summed front to back by one thread -- an order
// that n alone decides, so a row depends neither on its neighbours nor on the padded width NF -- and columns t >= n leave as exact
// zeros.  n = 1: std 0, (x - x) / 2e-12 = 0, as numpy gives.
template <bool kRagged>
__global__ __launch_bounds__(256) void cmvn_kernel(const float* __restrict__ feat, const float* __restrict__ energy,
                                                   const int32_t* __restrict__ flen, float* __restrict__ y, int B, int NF, int C, int ldf,
                                                   int normalize) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * C) return;
  const int c = (int)(i % C);
  const long long b = i / C;
  const int n = kRagged ? (int)clamp_len(flen[b], NF) : NF;
  const float* p = feat + b * NF * ldf + c;
  const float* en = (energy && c == 0) ? energy + b * NF : nullptr;
  double s = 0.0;
  for (int f = 0; f < n; ++f) s += (double)(en ? logf(en[f]) : p[(long long)f * ldf]);
  const double mean = s / n;
  double q = 0.0;
  for (int f = 0; f < n; ++f) {
    const double d = (double)(en ? logf(en[f]) : p[(long long)f * ldf]) - mean;
    q += d * d;
  }
  const float mu = normalize ? (float)mean : 0.f;
  const float den = normalize ? (float)sqrt(q / n) + 2e-12f : 1.f;
  float* o = y + (b * C + c) * NF;
  for (int f = 0; f < n; ++f) o[f] = ((en ? logf(en[f]) : p[(long long)f * ldf]) - mu) / den;
  for (int f = n; f < NF; ++f) o[f] = 0.f;
}

// python_speech_features.delta as SpkTrainDataset._delta applies it (datasets.py:55-63): x [B, C, NF] (channel first, as
// the loaders hold features) -> y [B, (1 + order) C, NF] = [x | delta(x, N=1) | delta(x, N=2)] -- BOTH differences are
// taken of the base features (the reference does not difference the deltas again):
//   delta(x, N)[t] = sum_{n=-N..N} n x[clamp(t + n)] / (2 sum_{n=1..N} n^2)        (edge padding)
// kRagged: the edge padding repeats the row's own last frame n - 1 (n = clamp(flen[b], 1, NF)), not column NF - 1, and columns
// t >= n are zeros in all 1 + order blocks.
template <bool kRagged>
__global__ __launch_bounds__(256) void delta_kernel(const float* __restrict__ x, const int32_t* __restrict__ flen, float* __restrict__ y,
                                                    long long rows, int C, int NF, int order) {
  const long long total = rows * NF;                 // rows = B * C
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int t = (int)(i % NF);
    const long long r = i / NF;
    const long long b = r / C;
    const int c = (int)(r - b * C);
    const float* p = x + r * NF;
    const int n = kRagged ? (int)clamp_len(flen[b], NF) : NF;
    float* o = y + (b * (1 + order) * C + c) * NF + t;
    if (kRagged && t >= n) {
      for (int k = 0; k <= order; ++k) o[(long long)k * C * NF] = 0.f;
      continue;
    }
    auto at = [&](int u) { return p[u < 0 ? 0 : (u >= n ? n - 1 : u)]; };
    o[0] = p[t];
    if (order >= 1) o[(long long)C * NF] = (at(t + 1) - at(t - 1)) / 2.0f;
    if (order >= 2) o[(long long)2 * C * NF] = (2.0f * at(t + 2) + at(t + 1) - at(t - 1) - 2.0f * at(t - 2)) / 10.0f;
  }
}

// uint8 frames [N, CH, H, W] (CH = 1 gray or 3 RGB; N = B clips of T frames) -> crop [N, CS, CS] float, normalised.
//   clip_params == NULL: the "val" pipeline's CenterCrop (preprocess.py:89-90: the margin halved and rounded DOWN);
//   clip_params [B][4] = (oy, ox, flip, 0): the "train" pipeline's RandomCrop origin + HorizontalFlip coin of each clip
//     (preprocess.py:95-138, dataloaders.py:13-17), drawn by the host; a flipped clip reads column ox + CS - 1 - cx;
//   lengths [B]: frames t >= lengths[b] are the zero padding of pad_packed_collate -- zeros of the NORMALISED clip
//     (dataset.py:117,130-134: the clip is normalised first, padded second).
__global__ __launch_bounds__(256) void crop_norm_kernel(const uint8_t* __restrict__ x, float* __restrict__ y,
                                                        long long N, int CH, int H, int W, int CS, int T,
                                                        const int32_t* __restrict__ clip_params, const int32_t* __restrict__ lengths) {
  const long long total = N * CS * CS;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    int cx = (int)(i % CS);
    const int cy = (int)((i / CS) % CS);
    const long long n = i / ((long long)CS * CS);
    const int b = (int)(n / T);
    if (lengths != nullptr && (int)(n - (long long)b * T) >= lengths[b]) { y[i] = 0.f; continue; }
    int oy = (H - CS) / 2, ox = (W - CS) / 2;
    if (clip_params != nullptr) {
      oy = min(max(clip_params[4 * b], 0), H - CS);
      ox = min(max(clip_params[4 * b + 1], 0), W - CS);
      if (clip_params[4 * b + 2] != 0) cx = CS - 1 - cx;
    }
    const uint8_t* p = x + (n * CH * H + (oy + cy)) * W + ox + cx;
    float g;
    if (CH == 3) g = dlip_gray601((float)p[0], (float)p[(long long)H * W], (float)p[2LL * H * W]);
    else g = (float)p[0];
    y[i] = dlip_pixel_norm(g);
  }
}

constexpr int kGridCap = 2048;

}  // namespace

// Each pair of entry points (rectangular | ragged) shares one launch: lengths == NULL picks the kernel that reads none.
static int frame_preemph(const float* x, const int32_t* slen, float* frames, int32_t B, int32_t S, int32_t NF, int32_t frame_len,
                         int32_t frame_step, int32_t nfft, float preemph, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && frames && B > 0 && S > 0 && NF > 0 && frame_len > 0 && frame_step > 0 && nfft >= frame_len);
  const long long total = (long long)B * NF * nfft;
  hipLaunchKernelGGL(slen ? frame_preemph_kernel<true> : frame_preemph_kernel<false>, dim3(dlip_grid1d(total, kGridCap)), dim3(256), 0,
                     dlip_hip_stream(stream), x, slen, frames, S, NF, frame_len, frame_step, nfft, preemph, total);
  return dlip_launch_status();
}

extern "C" int dlip_frame_preemph_f32(const float* x, float* frames, int32_t B, int32_t S, int32_t NF, int32_t frame_len,
                                      int32_t frame_step, int32_t nfft, float preemph, dlip_stream_t stream) {
  return frame_preemph(x, nullptr, frames, B, S, NF, frame_len, frame_step, nfft, preemph, stream);
}

extern "C" int dlip_frame_preemph_ragged_f32(const float* x, const int32_t* sample_len, float* frames, int32_t B, int32_t S, int32_t NF,
                                             int32_t frame_len, int32_t frame_step, int32_t nfft, float preemph, dlip_stream_t stream) {
  DLIP_CHECK_ARG(sample_len);
  return frame_preemph(x, sample_len, frames, B, S, NF, frame_len, frame_step, nfft, preemph, stream);
}

extern "C" int dlip_wave_frame_lengths_i32(const int32_t* sample_len, int32_t* frame_lengths, int32_t B, int64_t S, int32_t frame_len,
                                           int32_t frame_step, dlip_stream_t stream) {
  DLIP_CHECK_ARG(sample_len && frame_lengths && B > 0 && S > 0 && frame_len > 0 && frame_step > 0);
  hipLaunchKernelGGL(wave_frame_lengths_kernel, dim3((B + 255) / 256), dim3(256), 0, dlip_hip_stream(stream), sample_len, frame_lengths,
                     B, (long long)S, frame_len, frame_step);
  return dlip_launch_status();
}

extern "C" int dlip_powspec_f32(const float* spec, float* pw, float* energy, int32_t R, int32_t NB, int32_t NBp,
                                int32_t nfft, dlip_stream_t stream) {
  DLIP_CHECK_ARG(spec && pw && energy && R > 0 && NB > 0 && NBp >= NB && nfft > 0);
  hipLaunchKernelGGL(powspec_kernel, dim3((R + 3) / 4), dim3(256), 0, dlip_hip_stream(stream), spec, pw, energy,
                     R, NB, NBp, 1.0f / (float)nfft);
  return dlip_launch_status();
}

extern "C" int dlip_powspec_dft64_f32(const float* frames, float* pw, float* energy, int32_t R, int32_t NB, int32_t NBp,
                                      int32_t nfft, dlip_stream_t stream) {
  DLIP_CHECK_ARG(frames && pw && energy && R > 0 && NB > 0 && NBp >= NB && nfft >= 2 && nfft <= 1024 && (nfft & (nfft - 1)) == 0);
  DLIP_CHECK_ARG(NB <= nfft / 2 + 1);
  hipLaunchKernelGGL(powspec_dft64_kernel, dim3(R), dim3(256), (size_t)(3 * nfft + 4) * sizeof(double),
                     dlip_hip_stream(stream), frames, pw, energy, NB, NBp, nfft);
  return dlip_launch_status();
}

static int powspec_wave_fft64(const float* x, const int32_t* slen, float* pw, float* energy, int64_t B, int64_t S, int32_t NF,
                              int32_t frame_len, int32_t frame_step, int32_t nfft, double preemph, int32_t NB, int32_t NBp,
                              dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && pw && energy && B > 0 && S > 0 && NF > 0 && frame_len > 0 && frame_step > 0 && nfft >= frame_len);
  DLIP_CHECK_ARG(nfft >= 128 && nfft <= 1024 && (nfft & (nfft - 1)) == 0 && NB > 0 && NB <= nfft / 2 + 1 && NBp >= NB);
  DLIP_CHECK_ARG(B * (long long)NF < (1ll << 31));
  int lg = 0;
  while ((1 << lg) < nfft) ++lg;
  const int threads = nfft / 2;            // 64 .. 512: one butterfly per thread and stage
  const size_t lds = (size_t)(3 * nfft + 8) * sizeof(double);
  hipLaunchKernelGGL(slen ? powspec_wave_fft64_kernel<true> : powspec_wave_fft64_kernel<false>, dim3((unsigned)(B * NF)),
                     dim3((unsigned)threads), lds, dlip_hip_stream(stream), x, slen, pw, energy, (long long)S, NF, frame_len, frame_step,
                     nfft, lg, preemph, NB, NBp);
  return dlip_launch_status();
}

extern "C" int dlip_powspec_wave_fft64_f32(const float* x, float* pw, float* energy, int64_t B, int64_t S, int32_t NF, int32_t frame_len,
                                           int32_t frame_step, int32_t nfft, double preemph, int32_t NB, int32_t NBp, dlip_stream_t stream) {
  return powspec_wave_fft64(x, nullptr, pw, energy, B, S, NF, frame_len, frame_step, nfft, preemph, NB, NBp, stream);
}

extern "C" int dlip_powspec_wave_fft64_ragged_f32(const float* x, const int32_t* sample_len, float* pw, float* energy, int64_t B, int64_t S,
                                                  int32_t NF, int32_t frame_len, int32_t frame_step, int32_t nfft, double preemph, int32_t NB,
                                                  int32_t NBp, dlip_stream_t stream) {
  DLIP_CHECK_ARG(sample_len);
  return powspec_wave_fft64(x, sample_len, pw, energy, B, S, NF, frame_len, frame_step, nfft, preemph, NB, NBp, stream);
}

static bool stft_geometry_ok(int64_t S, int32_t n_fft, int32_t hop) {
  return n_fft >= 128 && n_fft <= 1024 && (n_fft & (n_fft - 1)) == 0 && hop >= 1 && S >= n_fft / 2 + 1;
}

static int stft_logmag_wave(const float* x, const int32_t* slen, float* out, int64_t B, int64_t S, int32_t NF, int32_t win, int32_t hop,
                            int32_t n_fft, int32_t F, int32_t Fp, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && out && B > 0 && stft_geometry_ok(S, n_fft, hop) && win >= 1 && win <= n_fft);
  DLIP_CHECK_ARG((int64_t)NF == 1 + S / hop && F == n_fft / 2 + 1 && Fp >= F);
  DLIP_CHECK_ARG(B * (long long)NF < (1ll << 31));
  int lg = 0;
  while ((1 << lg) < n_fft) ++lg;
  const int threads = n_fft / 2;           // 64 .. 512: one butterfly per thread and stage
  const size_t lds = (size_t)(3 * n_fft) * sizeof(double);
  hipLaunchKernelGGL(slen ? stft_logmag_wave_kernel<true> : stft_logmag_wave_kernel<false>, dim3((unsigned)(B * NF)),
                     dim3((unsigned)threads), lds, dlip_hip_stream(stream), x, slen, out, (long long)S, NF, win, hop, n_fft, lg, F, Fp);
  return dlip_launch_status();
}

extern "C" int dlip_stft_logmag_wave_f32(const float* x, float* out, int64_t B, int64_t S, int32_t NF, int32_t win, int32_t hop,
                                         int32_t n_fft, int32_t F, int32_t Fp, dlip_stream_t stream) {
  return stft_logmag_wave(x, nullptr, out, B, S, NF, win, hop, n_fft, F, Fp, stream);
}

extern "C" int dlip_stft_logmag_wave_ragged_f32(const float* x, const int32_t* sample_len, float* out, int64_t B, int64_t S, int32_t NF,
                                                int32_t win, int32_t hop, int32_t n_fft, int32_t F, int32_t Fp, dlip_stream_t stream) {
  DLIP_CHECK_ARG(sample_len);
  return stft_logmag_wave(x, sample_len, out, B, S, NF, win, hop, n_fft, F, Fp, stream);
}

extern "C" int dlip_stft_frame_lengths_i32(const int32_t* sample_len, int32_t* frame_lengths, int32_t B, int64_t S, int32_t n_fft,
                                           int32_t hop, dlip_stream_t stream) {
  DLIP_CHECK_ARG(sample_len && frame_lengths && B > 0 && stft_geometry_ok(S, n_fft, hop));
  hipLaunchKernelGGL(stft_frame_lengths_kernel, dim3((B + 255) / 256), dim3(256), 0, dlip_hip_stream(stream), sample_len, frame_lengths,
                     B, (long long)S, n_fft, hop);
  return dlip_launch_status();
}

extern "C" int dlip_log_floor_f32(const float* x, float* y, int64_t n, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && n > 0);
  hipLaunchKernelGGL(log_floor_kernel, dim3(dlip_grid1d(n, kGridCap)), dim3(256), 0, dlip_hip_stream(stream), x, y, (long long)n);
  return dlip_launch_status();
}

static int cmvn_nct(const float* feat, const float* energy, const int32_t* flen, float* y, int32_t B, int32_t NF, int32_t C, int32_t ldf,
                    int32_t normalize, dlip_stream_t stream) {
  DLIP_CHECK_ARG(feat && y && B > 0 && NF > 0 && C > 0 && ldf >= C);
  hipLaunchKernelGGL(flen ? cmvn_kernel<true> : cmvn_kernel<false>, dim3((unsigned)(((long long)B * C + 255) / 256)), dim3(256), 0,
                     dlip_hip_stream(stream), feat, energy, flen, y, B, NF, C, ldf, normalize);
  return dlip_launch_status();
}

extern "C" int dlip_cmvn_nct_f32(const float* feat, const float* energy, float* y, int32_t B, int32_t NF, int32_t C,
                                 int32_t ldf, int32_t normalize, dlip_stream_t stream) {
  return cmvn_nct(feat, energy, nullptr, y, B, NF, C, ldf, normalize, stream);
}

extern "C" int dlip_cmvn_nct_ragged_f32(const float* feat, const float* energy, const int32_t* frame_lengths, float* y, int32_t B, int32_t NF,
                                        int32_t C, int32_t ldf, int32_t normalize, dlip_stream_t stream) {
  DLIP_CHECK_ARG(frame_lengths);
  return cmvn_nct(feat, energy, frame_lengths, y, B, NF, C, ldf, normalize, stream);
}

static int delta_nct(const float* x, const int32_t* flen, float* y, int32_t B, int32_t C, int32_t NF, int32_t order, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && B > 0 && C > 0 && NF > 0 && (order == 1 || order == 2));
  const long long rows = (long long)B * C;
  hipLaunchKernelGGL(flen ? delta_kernel<true> : delta_kernel<false>, dim3(dlip_grid1d(rows * NF, kGridCap)), dim3(256), 0,
                     dlip_hip_stream(stream), x, flen, y, rows, C, NF, order);
  return dlip_launch_status();
}

extern "C" int dlip_delta_nct_f32(const float* x, float* y, int32_t B, int32_t C, int32_t NF, int32_t order,
                                  dlip_stream_t stream) {
  return delta_nct(x, nullptr, y, B, C, NF, order, stream);
}

extern "C" int dlip_delta_nct_ragged_f32(const float* x, const int32_t* frame_lengths, float* y, int32_t B, int32_t C, int32_t NF,
                                         int32_t order, dlip_stream_t stream) {
  DLIP_CHECK_ARG(frame_lengths);
  return delta_nct(x, frame_lengths, y, B, C, NF, order, stream);
}

extern "C" int dlip_crop_normalize_u8(const uint8_t* x, const int32_t* clip_params, const int32_t* lengths, int32_t T, float* y,
                                      int64_t n_frames, int32_t channels, int32_t H, int32_t W, int32_t crop, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && n_frames > 0 && (channels == 1 || channels == 3) && crop > 0 && H >= crop && W >= crop);
  DLIP_CHECK_ARG(T > 0 && n_frames % T == 0);
  hipLaunchKernelGGL(crop_norm_kernel, dim3(dlip_grid1d(n_frames * crop * crop, kGridCap)), dim3(256), 0,
                     dlip_hip_stream(stream), x, y, (long long)n_frames, channels, H, W, crop, T, clip_params, lengths);
  return dlip_launch_status();
}

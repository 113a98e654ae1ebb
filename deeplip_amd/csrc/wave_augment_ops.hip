// Waveform augmentation in front of the audio front-end: reverberation (an FIR
// filter with a room response, Kaldi's 'reverb' kind named by the reference's training lists, train_audio.py:454), additive noise at a
// drawn SNR (models/video_models/preprocess.py:150-179 AddNoise; Kaldi's 'music' / 'babble' / 'noise' kinds) and per-utterance
// normalisation (preprocess.py:141-147 NormalizeUtterance) on a batch wave [B, S] + optional sample counts.  Row b holds
// n = clamp(lengths[b], 1, S) samples (S without lengths) and is computed as if it were alone: every sum that decides a row's values
// (powers, mean, variance) is taken in fp64 per TILE of DLIP_FIR_TILE samples in one fixed order and the tile results are met
// front to back over the row's own ceil(n / TILE) tiles -- no atomics, nothing depends on B, S or the neighbours.  Samples t >= n of
// every output row are written as zeros; samples t >= n of the input are never read.
//
// Workspace (dlip_wave_reverb_workspace_bytes): two doubles per (row, tile); each entry point fills and reads it within its own
// launches, so one block serves the three calls in turn.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int kTile = DLIP_FIR_TILE;             // consecutive outputs of one row per workgroup
constexpr int kChunk = DLIP_FIR_TAP_CHUNK;       // taps per staged input window
constexpr int kThreads = 256;
constexpr int kPer = kTile / kThreads;           // consecutive outputs per lane of the FIR kernel; elements per lane elsewhere
static_assert(kPer == 8 && kChunk % 16 == 0 && kChunk >= 16, "the FIR kernel's register window is written for 8 outputs per lane");

__device__ __forceinline__ int row_len(const int32_t* lengths, long long b, int S) {
  if (lengths == nullptr) return S;
  const int v = lengths[b];
  return v < 1 ? 1 : (v > S ? S : v);
}

// out[t0 .. t0 + kTile) of one row := in (t < n) | 0 (n <= t < S): pass-through rows bit for bit, and the zero tail of every row
__device__ __forceinline__ void copy_tile(const float* __restrict__ in, float* __restrict__ out, int t0, int n, int S) {
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = t0 + j * kThreads + (int)threadIdx.x;
    if (t < S) out[t] = t < n ? in[t] : 0.f;
  }
}

// ((sum_a, sum_b) over the workgroup) in fp64: lane-local sums come in, butterflies within a wave, the four waves in wave order
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
  a = dlip_wave_sum_f64(a);
  b = dlip_wave_sum_f64(b);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = a;
    red[4 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  a = ((red[0] + red[1]) + red[2]) + red[3];
  b = ((red[4] + red[5]) + red[6]) + red[7];
}

// The row's two sums: its tiles' partials met front to back (every thread walks the same words: scalar loads)
__device__ __forceinline__ void row_sums(const double* __restrict__ part, int n, double& a, double& b) {
  const int nt = (n + kTile - 1) / kTile;
  a = 0.0;
  b = 0.0;
  for (int i = 0; i < nt; ++i) {
    a += part[2 * i];
    b += part[2 * i + 1];
  }
}

// ---------------------------------------------------------------------------------------------------------------- reverberation
// y[t] = sum_{k < len} h[k] x[t + d - k], 0 <= t < n, x zero outside [0, n): exact fp32 on the vector ALUs, one fmaf per product,
// taps in ascending order whatever the geometry.  A workgroup owns kTile consecutive outputs of one row, a lane kPer = 8
// consecutive ones.  The taps are walked in chunks of kChunk: per chunk the input window the tile needs (kTile + kChunk - 1 samples,
// zero-filled outside the row) is staged in LDS; within a chunk the taps go in blocks of 8, for which a lane needs 15 consecutive
// window words -- 7 of them it holds from the block before (the window slides DOWN as the tap index rises), 8 it reads as two
// 16-byte LDS words -- and the 8 taps, the same for every lane, come as wave-uniform loads: 8 LDS words + 8 taps feed 64 FMAs.
// Partial sums of x^2 and y^2 over the tile leave in fp64 for keep_power.
__device__ __forceinline__ void fir_block(const float (&lo)[8], const float (&hi)[8], const float (&hk)[8], float (&acc)[kPer]) {
  // window word m = j - u + 7 (output j, tap u of the block): m < 8 in lo, else in hi[m - 8]
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int m = j - u + 7;
      acc[j] = fmaf(hk[u], m < 8 ? lo[m] : hi[m - 8], acc[j]);
    }
}

__device__ __forceinline__ void load_taps(const float* __restrict__ h, int k, int len, float (&hk)[8]) {
  if (k + 8 <= len) {
#pragma unroll
    for (int u = 0; u < 8; ++u) hk[u] = h[k + u];
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u) hk[u] = k + u < len ? h[k + u] : 0.f;
  }
}

__device__ __forceinline__ void load8(const float* __restrict__ win, int p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(win + p);
  const f32x4 b = *reinterpret_cast<const f32x4*>(win + p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__global__ __launch_bounds__(kThreads) void fir_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                        const float* __restrict__ rir, const int32_t* __restrict__ rir_len,
                                                        const int32_t* __restrict__ rir_peak, const int32_t* __restrict__ rir_idx,
                                                        float* __restrict__ y, double* __restrict__ part, int S, int R, int Lmax,
                                                        int ntiles) {
  __shared__ __attribute__((aligned(16))) float win[kTile + kChunk];
  __shared__ double red[8];
  const long long b = blockIdx.y;
  const int t0 = (int)blockIdx.x * kTile;
  const int n = row_len(lengths, b, S);
  const float* xb = x + b * S;
  float* yb = y + b * S;
  int ri = rir_idx[b];
  // both exits depend on blockIdx alone (the whole workgroup takes them) and sit in front of the first barrier
  if (t0 >= n || ri < 0) {
    copy_tile(xb, yb, t0, n, S);
    return;
  }
  ri = ri < R ? ri : R - 1;
  int len = rir_len[ri];
  len = len < 1 ? 1 : (len > Lmax ? Lmax : len);
  int d = rir_peak[ri];
  d = d < 0 ? 0 : (d >= len ? len - 1 : d);
  const float* h = rir + (long long)ri * Lmax;
  const int lb = (int)threadIdx.x * kPer;
  float acc[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) acc[j] = 0.f;
  for (int k0 = 0; k0 < len; k0 += kChunk) {
    const int wb = t0 + d - k0 - (kChunk - 1);                    // the row sample that window word 0 holds
    if (k0) __syncthreads();                                      // the chunk before has been read
    for (int i = threadIdx.x; i < kTile + kChunk; i += kThreads) {
      const int s = wb + i;
      win[i] = (s >= 0 && s < n) ? xb[s] : 0.f;
    }
    __syncthreads();
    const int kc = len - k0 < kChunk ? len - k0 : kChunk;
    // output j of the lane takes tap k0 + kk from window word lb + j + (kChunk - 1) - kk
    float wa[8], wc[8], hk[8];
    load8(win, lb + kChunk, wc);                                  // words 8 .. 15 of the first block (the 16th is never used)
    for (int kk = 0; kk < kc; kk += 16) {                         // two blocks per turn: the halves of the window change roles
      load8(win, lb + kChunk - 8 - kk, wa);
      load_taps(h, k0 + kk, len, hk);
      fir_block(wa, wc, hk, acc);
      load8(win, lb + kChunk - 16 - kk, wc);
      load_taps(h, k0 + kk + 8, len, hk);
      fir_block(wc, wa, hk, acc);
    }
  }
  double px = 0.0, py = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = t0 + lb + j;
    if (t < S) yb[t] = t < n ? acc[j] : 0.f;
    if (t < n) {
      const double xv = (double)xb[t];
      px += xv * xv;
      py += (double)acc[j] * (double)acc[j];
    }
  }
  block_sum2(px, py, red);
  if (threadIdx.x == 0) {
    double* p = part + (b * ntiles + blockIdx.x) * 2;
    p[0] = px;
    p[1] = py;
  }
}

// keep_power: y *= sqrt(Px / Py) over the row's own samples (gain 1 when Py == 0); pass-through rows and tiles past n are left alone
__global__ __launch_bounds__(kThreads) void reverb_gain_kernel(float* __restrict__ y, const int32_t* __restrict__ lengths,
                                                                const int32_t* __restrict__ rir_idx, const double* __restrict__ part,
                                                                int S, int ntiles) {
  const long long b = blockIdx.y;
  const int t0 = (int)blockIdx.x * kTile;
  const int n = row_len(lengths, b, S);
  if (t0 >= n || rir_idx[b] < 0) return;
  double px, py;
  row_sums(part + b * ntiles * 2, n, px, py);
  if (py == 0.0) return;
  const float g = (float)sqrt(px / py);
  float* yb = y + b * S;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = t0 + j * kThreads + (int)threadIdx.x;
    if (t < n) yb[t] *= g;
  }
}

// The FIR kernel's power partials for a y that another kernel made (the transform route, wave_reverb_fft_ops.hip): the same lanes own
// the same samples and the sums meet in the same order, so keep_power is one computation whichever route convolved.
__global__ __launch_bounds__(kThreads) void reverb_power_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                                 const int32_t* __restrict__ rir_idx, const float* __restrict__ y,
                                                                 double* __restrict__ part, int S, int ntiles) {
  __shared__ double red[8];
  const long long b = blockIdx.y;
  const int t0 = (int)blockIdx.x * kTile;
  const int n = row_len(lengths, b, S);
  if (t0 >= n || rir_idx[b] < 0) return;
  const float* xb = x + b * S;
  const float* yb = y + b * S;
  const int lb = (int)threadIdx.x * kPer;
  double px = 0.0, py = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = t0 + lb + j;
    if (t < n) {
      const double xv = (double)xb[t], yv = (double)yb[t];
      px += xv * xv;
      py += yv * yv;
    }
  }
  block_sum2(px, py, red);
  if (threadIdx.x == 0) {
    double* p = part + (b * ntiles + blockIdx.x) * 2;
    p[0] = px;
    p[1] = py;
  }
}

// ------------------------------------------------------------------------------------------------------------------------ noise
// The slice of row b: bank[st .. st + n), st = clamp(start[b], 0, max(bank_len - n, 0)); words past the bank's end read as zero.
__device__ __forceinline__ long long noise_start(const int64_t* __restrict__ start, long long b, long long bank_len, int n) {
  const long long hi = bank_len - n > 0 ? bank_len - n : 0;
  const long long s = start[b];
  return s < 0 ? 0 : (s > hi ? hi : s);
}

__global__ __launch_bounds__(kThreads) void noise_power_kernel(const float* __restrict__ y, const int32_t* __restrict__ lengths,
                                                                const float* __restrict__ bank, long long bank_len,
                                                                const int64_t* __restrict__ start, const float* __restrict__ snr_db,
                                                                double* __restrict__ part, int S, int ntiles) {
  __shared__ double red[8];
  const long long b = blockIdx.y;
  const int t0 = (int)blockIdx.x * kTile;
  const int n = row_len(lengths, b, S);
  if (t0 >= n || !(snr_db[b] < 9999.f)) return;
  const long long st = noise_start(start, b, bank_len, n);
  const float* yb = y + b * S;
  double py = 0.0, pc = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = t0 + j * kThreads + (int)threadIdx.x;
    if (t < n) {
      const double yv = (double)yb[t];
      const double cv = st + t < bank_len ? (double)bank[st + t] : 0.0;
      py += yv * yv;
      pc += cv * cv;
    }
  }
  block_sum2(py, pc, red);
  if (threadIdx.x == 0) {
    double* p = part + (b * ntiles + blockIdx.x) * 2;
    p[0] = py;
    p[1] = pc;
  }
}

// z = y + c sqrt((Py / Pc) / 10^(snr / 10)) (preprocess.py:175-178); rows at the sentinel and rows whose slice has Pc == 0 pass through
__global__ __launch_bounds__(kThreads) void noise_mix_kernel(const float* __restrict__ y, const int32_t* __restrict__ lengths,
                                                              const float* __restrict__ bank, long long bank_len,
                                                              const int64_t* __restrict__ start, const float* __restrict__ snr_db,
                                                              const double* __restrict__ part, float* __restrict__ z, int S, int ntiles) {
  const long long b = blockIdx.y;
  const int t0 = (int)blockIdx.x * kTile;
  const int n = row_len(lengths, b, S);
  const float* yb = y + b * S;
  float* zb = z + b * S;
  const float snr = snr_db[b];
  double py = 0.0, pc = 0.0;
  const bool live = t0 < n && snr < 9999.f;
  if (live) row_sums(part + b * ntiles * 2, n, py, pc);
  if (!live || pc == 0.0) {
    copy_tile(yb, zb, t0, n, S);
    return;
  }
  const float g = (float)sqrt((py / pc) / pow(10.0, (double)snr / 10.0));
  const long long st = noise_start(start, b, bank_len, n);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = t0 + j * kThreads + (int)threadIdx.x;
    if (t < S) {
      float v = 0.f;
      if (t < n) {
        const float c = st + t < bank_len ? bank[st + t] : 0.f;
        v = yb[t] + c * g;
      }
      zb[t] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- normalisation
// Per tile: (mean, sum of squared deviations from that mean) of its samples, two passes over registers; the apply kernel joins the
// tiles front to back (the pairwise update of Chan et al.).  A constant row has every deviation exactly 0, hence std 0 and zeros.
__global__ __launch_bounds__(kThreads) void norm_stats_kernel(const float* __restrict__ z, const int32_t* __restrict__ lengths,
                                                               double* __restrict__ part, int S, int ntiles) {
  __shared__ double red[8];
  const long long b = blockIdx.y;
  const int t0 = (int)blockIdx.x * kTile;
  const int n = row_len(lengths, b, S);
  if (t0 >= n) return;
  const float* zb = z + b * S;
  const int cnt = n - t0 < kTile ? n - t0 : kTile;
  float v[kPer];
  double s = 0.0, unused = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = j * kThreads + (int)threadIdx.x;
    v[j] = t < cnt ? zb[t0 + t] : 0.f;
    s += (double)v[j];
  }
  block_sum2(s, unused, red);
  const double mean = s / cnt;
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = j * kThreads + (int)threadIdx.x;
    const double dv = (double)v[j] - mean;
    if (t < cnt) q += dv * dv;
  }
  __syncthreads();                                                // red[] has been read by everyone
  block_sum2(q, unused, red);
  if (threadIdx.x == 0) {
    double* p = part + (b * ntiles + blockIdx.x) * 2;
    p[0] = mean;
    p[1] = q;
  }
}

__global__ __launch_bounds__(kThreads) void norm_apply_kernel(const float* __restrict__ z, const int32_t* __restrict__ lengths,
                                                               const double* __restrict__ part, float* __restrict__ out, int S,
                                                               int ntiles) {
  const long long b = blockIdx.y;
  const int t0 = (int)blockIdx.x * kTile;
  const int n = row_len(lengths, b, S);
  const float* zb = z + b * S;
  float* ob = out + b * S;
  double mean = 0.0, m2 = 0.0;
  if (t0 < n) {
    const double* p = part + b * ntiles * 2;
    const int nt = (n + kTile - 1) / kTile;
    mean = p[0];
    m2 = p[1];
    for (int i = 1; i < nt; ++i) {
      const double na = (double)i * kTile;
      const double nb = (double)(n - i * kTile < kTile ? n - i * kTile : kTile);
      const double delta = p[2 * i] - mean;
      mean += delta * nb / (na + nb);
      m2 += p[2 * i + 1] + delta * delta * na * nb / (na + nb);
    }
  }
  const double sd = sqrt(m2 / n);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = t0 + j * kThreads + (int)threadIdx.x;
    if (t < S) ob[t] = (t < n && sd != 0.0) ? (float)(((double)zb[t] - mean) / sd) : 0.f;
  }
}

inline int tiles_of(int64_t S) { return (int)((S + kTile - 1) / kTile); }

}  // namespace

extern "C" int64_t dlip_wave_reverb_workspace_bytes(int64_t B, int64_t S) {
  if (B <= 0 || S <= 0 || B > 65535 || S > 0x7fffffffll - kTile) return DLIP_EINVAL;
  return B * tiles_of(S) * 2 * (int64_t)sizeof(double);
}

#define DLIP_WAVE_ARGS(B, S, ws, ws_bytes)                                                                  \
  DLIP_CHECK_ARG((B) > 0 && (B) <= 65535 && (S) > 0 && (S) <= 0x7fffffffll - kTile);                        \
  DLIP_CHECK_ARG((ws) && dlip_aligned<8>(ws) && (ws_bytes) >= dlip_wave_reverb_workspace_bytes((B), (S)))

extern "C" int dlip_wave_reverb_f32(const float* x, const int32_t* lengths, const float* rir, const int32_t* rir_len,
                                    const int32_t* rir_peak, const int32_t* rir_idx, float* y, void* workspace, int64_t workspace_bytes,
                                    int32_t B, int32_t S, int32_t R, int32_t Lmax, int32_t keep_power, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && rir && rir_len && rir_peak && rir_idx && y && x != y && R > 0 && Lmax > 0 && Lmax <= DLIP_FIR_MAX_TAPS);
  DLIP_WAVE_ARGS(B, S, workspace, workspace_bytes);
  const int nt = tiles_of(S);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(fir_kernel, dim3(nt, B), dim3(kThreads), 0, dlip_hip_stream(stream), x, lengths, rir, rir_len, rir_peak, rir_idx, y,
                     part, S, R, Lmax, nt);
  if (keep_power)
    hipLaunchKernelGGL(reverb_gain_kernel, dim3(nt, B), dim3(kThreads), 0, dlip_hip_stream(stream), y, lengths, rir_idx, part, S, nt);
  return dlip_launch_status();
}

// keep_power behind the transform route (declared in dlip_launch.h): the partials of (x, y), then the gain.  Two launches.
void dlip_wave_reverb_keep_power(const float* x, const int32_t* lengths, const int32_t* rir_idx, float* y, double* part, int B, int S,
                                 hipStream_t stream) {
  const int nt = tiles_of(S);
  hipLaunchKernelGGL(reverb_power_kernel, dim3(nt, B), dim3(kThreads), 0, stream, x, lengths, rir_idx, y, part, S, nt);
  hipLaunchKernelGGL(reverb_gain_kernel, dim3(nt, B), dim3(kThreads), 0, stream, y, lengths, rir_idx, part, S, nt);
}

extern "C" int dlip_wave_add_noise_f32(const float* y, const int32_t* lengths, const float* bank, int64_t bank_len,
                                       const int64_t* noise_start, const float* snr_db, float* z, void* workspace,
                                       int64_t workspace_bytes, int32_t B, int32_t S, dlip_stream_t stream) {
  DLIP_CHECK_ARG(y && bank && bank_len > 0 && noise_start && snr_db && z);
  DLIP_WAVE_ARGS(B, S, workspace, workspace_bytes);
  const int nt = tiles_of(S);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(noise_power_kernel, dim3(nt, B), dim3(kThreads), 0, dlip_hip_stream(stream), y, lengths, bank, (long long)bank_len,
                     noise_start, snr_db, part, S, nt);
  hipLaunchKernelGGL(noise_mix_kernel, dim3(nt, B), dim3(kThreads), 0, dlip_hip_stream(stream), y, lengths, bank, (long long)bank_len,
                     noise_start, snr_db, part, z, S, nt);
  return dlip_launch_status();
}

extern "C" int dlip_wave_normalize_f32(const float* z, const int32_t* lengths, float* out, void* workspace, int64_t workspace_bytes,
                                       int32_t B, int32_t S, dlip_stream_t stream) {
  DLIP_CHECK_ARG(z && out);
  DLIP_WAVE_ARGS(B, S, workspace, workspace_bytes);
  const int nt = tiles_of(S);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(norm_stats_kernel, dim3(nt, B), dim3(kThreads), 0, dlip_hip_stream(stream), z, lengths, part, S, nt);
  hipLaunchKernelGGL(norm_apply_kernel, dim3(nt, B), dim3(kThreads), 0, dlip_hip_stream(stream), z, lengths, part, out, S, nt);
  return dlip_launch_status();
}

// Attentive statistics pooling (`pooling: attentive_statistic` is n = 1, ABI 67; `pooling: multi_head_attention`, ABI 64)
// on channels-last activations: n attention heads of their own hidden width over one frame tensor x [B,T,C], y [B, n 2C] =
// cat_h [mean_h | std_h].  Head h owns the columns off[h] .. off[h+1] of hidden [B,T,S] (ONE GEMM for all heads, in front of these
// kernels) and of v; the offsets travel as a device int32 [n+1] array and are clamped to [0, S] where they are read, so no column index
// leaves a hidden row whatever it holds.  One head needs no array: a null pointer means the columns [0, S).
//
// x is read once in the forward and twice in the backward for ALL heads, dx is written once, and every pass over x is spread over
// (channel block | row range, utterance) workgroups:
//   forward   mh_energy (one wave per frame: segmented dot products)  ->  mh_softmax (grid (head, utterance), parallel max and sum)
//             ->  mh_stat (grid (C / 64, utterance) as meanstd_kernel; alpha staged in LDS chunk by chunk; 2n accumulators per channel)
//   backward  mh_dalpha (grid (row range, utterance); dm | g_q | m of all heads in LDS)  ->  mh_softmax_bwd (grid (head, utterance))
//             ->  mh_dx (grid (C / 64, utterance); the heads' coefficients in registers)  ->  mh_dhidden (one wave per frame)
// Exact fp32 data; fp64 wherever a sum runs over frames, channels or hidden units; no atomics, fixed orders: the same bits on every run.
// Padding frames (t >= L_b) of x and hidden are never loaded; alpha, dx, dhidden, rde and de are written as zeros there.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int kMaxHeads = 8;
constexpr int kAlphaChunk = 256;                // frames of alpha staged in LDS per pass (a multiple of the 16 row groups)
constexpr size_t kMaxLds = 160 * 1024;          // LDS of one gfx950 workgroup
constexpr int kRowGridCap = 256 * 16;           // workgroups of the one-wave-per-frame passes, grid-stride the rest

// columns [lo, hi) of head h, inside [0, S] whatever the array holds; no array (n == 1 only, the entry points see to it): [0, S)
__device__ __forceinline__ void mh_head_range(const int32_t* __restrict__ off, int h, int S, int& lo, int& hi) {
  if (off == nullptr) { lo = 0; hi = S; return; }
  const int a = off[h], b = off[h + 1];
  lo = a < 0 ? 0 : (a > S ? S : a);
  hi = b < lo ? lo : (b > S ? S : b);
}

// e[b,h,t] = relu(hidden[b,t,off_h:off_{h+1}]) . v[off_h:off_{h+1}] + k[h] for t < L_b, 0 behind.  One wave per frame: the row's S
// contiguous floats are read once, head segment by head segment (coalesced inside a segment), one fp64 butterfly per head.
__global__ __launch_bounds__(256) void mh_energy_kernel(const float* __restrict__ hidden, const float* __restrict__ v,
                                                        const float* __restrict__ kk, const int32_t* __restrict__ off,
                                                        float* __restrict__ e, int B, int Tpad, int S, int n, const DlipLen len) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long rows = (long long)B * Tpad;
  for (long long r = (long long)blockIdx.x * 4 + wave; r < rows; r += (long long)gridDim.x * 4) {
    const int b = (int)(r / Tpad), t = (int)(r - (long long)b * Tpad);
    const int L = dlip_valid_rows(len, b, Tpad);
    if (t >= L) {
      if (lane < n) e[((long long)b * n + lane) * Tpad + t] = 0.f;
      continue;
    }
    const float* hr = hidden + r * S;
    for (int h = 0; h < n; ++h) {
      int lo, hi;
      mh_head_range(off, h, S, lo, hi);
      double s = 0.0;
      for (int j = lo + lane; j < hi; j += 64) s += (double)fmaxf(hr[j], 0.f) * (double)v[j];
      s = dlip_wave_sum_f64(s);
      if (lane == 0) e[((long long)b * n + h) * Tpad + t] = (float)s + kk[h];
    }
  }
}

// alpha[b,h,:] = softmax over t < L_b of e[b,h,:], in place; zeros behind L_b.  One workgroup per (head, utterance): the maximum and the
// fp64 sum of exponentials meet over the four waves (dlip_block_max4 / dlip_block_sum4).  Every thread reads and writes its own frames only.
__global__ __launch_bounds__(256) void mh_softmax_kernel(float* __restrict__ alpha, int Tpad, int n, const DlipLen len) {
  __shared__ float redf[4];
  __shared__ double redd[4];
  const int h = blockIdx.x, b = blockIdx.y;
  const int L = dlip_valid_rows(len, b, Tpad);
  float* a = alpha + ((long long)b * n + h) * Tpad;
  float mx = -__builtin_inff();
  for (int t = threadIdx.x; t < L; t += 256) mx = fmaxf(mx, a[t]);
  mx = dlip_block_max4(mx, redf);
  double se = 0.0;
  for (int t = threadIdx.x; t < L; t += 256) se += exp((double)(a[t] - mx));
  se = dlip_block_sum4(se, redd);
  for (int t = threadIdx.x; t < Tpad; t += 256) a[t] = t < L ? (float)(exp((double)(a[t] - mx)) / se) : 0.f;
}

// frames [t0, t0 + nt) of alpha[b, 0:NH, :] -> sa (all 256 threads call; barriers in front and behind)
template <int NH>
__device__ __forceinline__ void mh_stage_alpha(float (*sa)[kAlphaChunk], const float* __restrict__ ab, int Tpad, int t0, int nt) {
  __syncthreads();                 // the previous chunk has been consumed
#pragma unroll
  for (int h = 0; h < NH; ++h)
    for (int t = threadIdx.x; t < nt; t += 256) sa[h][t] = ab[(long long)h * Tpad + t0 + t];
  __syncthreads();
}

// y[b, h 2C + c] = m_h[c] = sum_t alpha[b,h,t] x[b,t,c];  y[b, h 2C + C + c] = sqrt(max(sum_t alpha x^2 - m_h^2, 0) + eps), or with
// eps == 0 the reference's unfloored sqrt(sum_t alpha x^2 - m_h^2) (pooling.py:106), NaN where rounding takes the difference below zero.
// One workgroup per (64-channel block, utterance) as meanstd_kernel: 16 lanes x float4 span the block, 16 row groups split the frames;
// every x element is loaded once and feeds the 2 NH fp64 accumulators of all heads; the 16 partial rows meet in LDS head by head.
template <int NH>
__global__ __launch_bounds__(256) void mh_stat_kernel(const float* __restrict__ x, const float* __restrict__ alpha, float* __restrict__ y,
                                                      int Tpad, int C, const DlipLen len, float eps) {
  __shared__ float sa[NH][kAlphaChunk];
  __shared__ double part[16][64][2];
  const int b = blockIdx.y, c0 = blockIdx.x * 64;
  const int L = dlip_valid_rows(len, b, Tpad);
  const int lx = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = c0 + lx * 4;
  const bool active = c < C;       // C % 4 == 0: a float4 is all inside or all outside
  const float* p = x + (long long)b * Tpad * C + (active ? c : 0);
  const float* ab = alpha + (long long)b * NH * Tpad;
  double m[NH][4], q[NH][4];
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int k = 0; k < 4; ++k) { m[h][k] = 0.0; q[h][k] = 0.0; }
  for (int t0 = 0; t0 < L; t0 += kAlphaChunk) {
    const int nt = L - t0 < kAlphaChunk ? L - t0 : kAlphaChunk;
    mh_stage_alpha<NH>(sa, ab, Tpad, t0, nt);
    if (active) {
      for (int t = g; t < nt; t += 16) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(p + (long long)(t0 + t) * C);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double xd = (double)xv[k], x2 = xd * xd;
#pragma unroll
          for (int h = 0; h < NH; ++h) {
            const double a = (double)sa[h][t];
            m[h][k] += a * xd;
            q[h][k] += a * x2;
          }
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    __syncthreads();               // the previous head's partials have been read
#pragma unroll
    for (int k = 0; k < 4; ++k) { part[g][lx * 4 + k][0] = m[h][k]; part[g][lx * 4 + k][1] = q[h][k]; }
    __syncthreads();
    if (threadIdx.x < 64 && c0 + (int)threadIdx.x < C) {
      double mm = 0.0, qq = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) { mm += part[i][threadIdx.x][0]; qq += part[i][threadIdx.x][1]; }
      float* yb = y + ((long long)b * NH + h) * 2 * C + c0 + threadIdx.x;
      yb[0] = (float)mm;
      yb[C] = (float)(eps == 0.f ? sqrt(qq - mm * mm) : sqrt(fmax(qq - mm * mm, 0.0) + (double)eps));
    }
  }
}

// dalpha[b,h,t] = sum_c x (dm_h[c] + g_q,h[c] (x - 2 m_h[c])),  g_q = ds / (2 s): the first backward pass over x, for all heads.
// One workgroup of eight waves per (row range, utterance); dm | g_q | m of every head are staged in LDS once (3 NH C floats, read from
// y and dy) and each wave takes a frame at a time: the row is loaded once (float4) and feeds NH fp64 sums, one butterfly per head.
template <int NH>
__global__ __launch_bounds__(512) void mh_dalpha_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                        float* __restrict__ dal, int Tpad, int C, int rows_per_wg, const DlipLen len) {
  extern __shared__ __attribute__((aligned(16))) float coef[];      // [NH][3][C]
  const int b = blockIdx.y;
  const int L = dlip_valid_rows(len, b, Tpad);
  const int t_begin = blockIdx.x * rows_per_wg;
  if (t_begin >= L) return;        // (workgroup-uniform: nobody reaches the barrier)
  const int t_end = t_begin + rows_per_wg < L ? t_begin + rows_per_wg : L;
  for (int i = threadIdx.x; i < NH * C; i += 512) {
    const int h = i / C, c = i - h * C;
    const long long o = ((long long)b * NH + h) * 2 * C + c;
    const double s = y[o + C], ds = dy[o + C];
    coef[(h * 3 + 0) * C + c] = dy[o];
    coef[(h * 3 + 1) * C + c] = (float)(ds / (2.0 * s));
    coef[(h * 3 + 2) * C + c] = y[o];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* xb = x + (long long)b * Tpad * C;
  for (int t = t_begin + wave; t < t_end; t += 8) {
    double a[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) a[h] = 0.0;
    for (int c = lane * 4; c < C; c += 256) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xb + (long long)t * C + c);
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const f32x4 dm = *reinterpret_cast<const f32x4*>(coef + (h * 3 + 0) * C + c);
        const f32x4 gq = *reinterpret_cast<const f32x4*>(coef + (h * 3 + 1) * C + c);
        const f32x4 mm = *reinterpret_cast<const f32x4*>(coef + (h * 3 + 2) * C + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double xd = (double)xv[k];
          a[h] += xd * ((double)dm[k] + (double)gq[k] * (xd - 2.0 * (double)mm[k]));
        }
      }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const double s = dlip_wave_sum_f64(a[h]);
      if (lane == 0) dal[((long long)b * NH + h) * Tpad + t] = (float)s;
    }
  }
}

// de[b,h,t] = alpha (dalpha - sum_t' alpha dalpha) over the valid frames, in place over dalpha; zeros behind (dalpha is not read there).
// dek[b,h] = sum_t de[b,h,t] (the rows of dk).  One workgroup per (head, utterance).
__global__ __launch_bounds__(256) void mh_softmax_bwd_kernel(const float* __restrict__ alpha, float* __restrict__ de, float* __restrict__ dek,
                                                             int Tpad, int n, const DlipLen len) {
  __shared__ double red[4];
  const int h = blockIdx.x, b = blockIdx.y;
  const int L = dlip_valid_rows(len, b, Tpad);
  const float* a = alpha + ((long long)b * n + h) * Tpad;
  float* d = de + ((long long)b * n + h) * Tpad;
  double dot = 0.0;
  for (int t = threadIdx.x; t < L; t += 256) dot += (double)a[t] * (double)d[t];
  dot = dlip_block_sum4(dot, red);
  __syncthreads();                 // red[] is written again below
  double tot = 0.0;
  for (int t = threadIdx.x; t < Tpad; t += 256) {
    const float o = t < L ? (float)((double)a[t] * ((double)d[t] - dot)) : 0.f;
    d[t] = o;
    tot += (double)o;
  }
  tot = dlip_block_sum4(tot, red);
  if (threadIdx.x == 0) dek[(long long)b * n + h] = (float)tot;
}

// dx[b,t,c] = sum_h alpha[b,h,t] (dm_h[c] + 2 g_q,h[c] (x - m_h[c])) for t < L_b, 0 behind: the second backward pass over x, summed
// over the heads in fp64 and written once.  Grid and thread layout of mh_stat_kernel; a thread keeps the coefficients of its four
// channels for all heads in registers and alpha arrives through LDS chunk by chunk.
template <int NH>
__global__ __launch_bounds__(256) void mh_dx_kernel(const float* __restrict__ x, const float* __restrict__ alpha, const float* __restrict__ y,
                                                    const float* __restrict__ dy, float* __restrict__ dx, int Tpad, int C, const DlipLen len) {
  __shared__ float sa[NH][kAlphaChunk];
  const int b = blockIdx.y, c0 = blockIdx.x * 64;
  const int L = dlip_valid_rows(len, b, Tpad);
  const int lx = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = c0 + lx * 4;
  const bool active = c < C;
  const long long xo = (long long)b * Tpad * C + (active ? c : 0);
  const float* ab = alpha + (long long)b * NH * Tpad;
  f32x4 dm[NH], g2[NH], mm[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    dm[h] = f32x4{0, 0, 0, 0}; g2[h] = dm[h]; mm[h] = dm[h];
    if (active) {
      const long long o = ((long long)b * NH + h) * 2 * C + c;
      dm[h] = *reinterpret_cast<const f32x4*>(dy + o);
      mm[h] = *reinterpret_cast<const f32x4*>(y + o);
      const f32x4 s = *reinterpret_cast<const f32x4*>(y + o + C), ds = *reinterpret_cast<const f32x4*>(dy + o + C);
#pragma unroll
      for (int k = 0; k < 4; ++k) g2[h][k] = (float)((double)ds[k] / (2.0 * (double)s[k]));
    }
  }
  for (int t0 = 0; t0 < Tpad; t0 += kAlphaChunk) {
    const int nt = Tpad - t0 < kAlphaChunk ? Tpad - t0 : kAlphaChunk;
    const int nv = L - t0 < 0 ? 0 : (L - t0 < nt ? L - t0 : nt);      // valid frames of the chunk
    mh_stage_alpha<NH>(sa, ab, Tpad, t0, nv);
    if (active) {
      for (int t = g; t < nt; t += 16) {
        f32x4 o = {0, 0, 0, 0};
        if (t < nv) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(x + xo + (long long)(t0 + t) * C);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double xd = (double)xv[k];
            double s = 0.0;
#pragma unroll
            for (int h = 0; h < NH; ++h)
              s += (double)sa[h][t] * ((double)dm[h][k] + 2.0 * (double)g2[h][k] * (xd - (double)mm[h][k]));
            o[k] = (float)s;
          }
        }
        *reinterpret_cast<f32x4*>(dx + xo + (long long)(t0 + t) * C) = o;
      }
    }
  }
}

// dhidden[b,t,j] = de[b,h(j),t] v[j] [hidden > 0],  rde[b,t,j] = de[b,h(j),t] relu(hidden[b,t,j]);  zeros in padding frames (hidden is
// not read there) and in any column no head owns.  One wave per frame, head segment by head segment, as mh_energy_kernel.
__global__ __launch_bounds__(256) void mh_dhidden_kernel(const float* __restrict__ hidden, const float* __restrict__ v,
                                                         const float* __restrict__ de, const int32_t* __restrict__ off,
                                                         float* __restrict__ dhidden, float* __restrict__ rde, int B, int Tpad, int S,
                                                         int n, const DlipLen len) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long rows = (long long)B * Tpad;
  for (long long r = (long long)blockIdx.x * 4 + wave; r < rows; r += (long long)gridDim.x * 4) {
    const int b = (int)(r / Tpad), t = (int)(r - (long long)b * Tpad);
    const int L = dlip_valid_rows(len, b, Tpad);
    const float* hr = hidden + r * S;
    float* dr = dhidden + r * S;
    float* rr = rde + r * S;
    if (t >= L) {
      for (int j = lane; j < S; j += 64) { dr[j] = 0.f; rr[j] = 0.f; }
      continue;
    }
    int first, last, unused;
    mh_head_range(off, 0, S, first, unused);
    mh_head_range(off, n - 1, S, unused, last);
    for (int j = lane; j < first; j += 64) { dr[j] = 0.f; rr[j] = 0.f; }
    for (int j = last + lane; j < S; j += 64) { dr[j] = 0.f; rr[j] = 0.f; }
    for (int h = 0; h < n; ++h) {
      int lo, hi;
      mh_head_range(off, h, S, lo, hi);
      const float d = de[((long long)b * n + h) * Tpad + t];
      for (int j = lo + lane; j < hi; j += 64) {
        const float hv = hr[j];
        dr[j] = hv > 0.f ? d * v[j] : 0.f;
        rr[j] = d * fmaxf(hv, 0.f);
      }
    }
  }
}

inline unsigned mh_row_grid(long long rows) {
  const long long g = (rows + 3) / 4;
  return (unsigned)(g < 1 ? 1 : (g > kRowGridCap ? kRowGridCap : g));
}

template <int NH>
int mh_stat_launch(const float* x, const float* alpha, float* y, int B, int T, int C, const DlipLen l, float eps, hipStream_t st) {
  hipLaunchKernelGGL(mh_stat_kernel<NH>, dim3((C + 63) / 64, B), dim3(256), 0, st, x, alpha, y, T, C, l, eps);
  return dlip_launch_status();
}

template <int NH>
int mh_bwd_launch(const float* x, const float* alpha, const float* y, const float* dy, float* dx, float* de, int B, int T, int C,
                  const DlipLen l, hipStream_t st, int phase) {
  if (phase == 0) {
    const size_t lds = (size_t)3 * NH * C * sizeof(float);
    auto kern = mh_dalpha_kernel<NH>;
    static DlipKernelState ks;     // the dynamic-LDS limit is raised once per device and size
    if (lds > 48 * 1024) {
      const int e = ks.ensure_lds(reinterpret_cast<const void*>(kern), lds);
      if (e != DLIP_OK) return e;
    }
    // row ranges: at least ~512 workgroups on the device while a range keeps >= 32 frames (the staging costs 3 NH frames' worth of loads)
    int splits = (512 + B - 1) / B;
    const int most = (T + 31) / 32;
    if (splits > most) splits = most;
    if (splits < 1) splits = 1;
    const int rows_per_wg = (T + splits - 1) / splits;
    hipLaunchKernelGGL(kern, dim3((T + rows_per_wg - 1) / rows_per_wg, B), dim3(512), lds, st, x, y, dy, de, T, C, rows_per_wg, l);
  } else {
    hipLaunchKernelGGL(mh_dx_kernel<NH>, dim3((C + 63) / 64, B), dim3(256), 0, st, x, alpha, y, dy, dx, T, C, l);
  }
  return dlip_launch_status();
}

#define MH_DISPATCH(n, CALL)        \
  switch (n) {                      \
    case 1: return CALL(1);         \
    case 2: return CALL(2);         \
    case 3: return CALL(3);         \
    case 4: return CALL(4);         \
    case 5: return CALL(5);         \
    case 6: return CALL(6);         \
    case 7: return CALL(7);         \
    case 8: return CALL(8);         \
    default: return DLIP_EINVAL;    \
  }

int mh_stat_dispatch(int n, const float* x, const float* alpha, float* y, int B, int T, int C, const DlipLen l, float eps, hipStream_t st) {
#define MH_CALL(N) mh_stat_launch<N>(x, alpha, y, B, T, C, l, eps, st)
  MH_DISPATCH(n, MH_CALL)
#undef MH_CALL
}

int mh_bwd_dispatch(int n, const float* x, const float* alpha, const float* y, const float* dy, float* dx, float* de, int B, int T, int C,
                    const DlipLen l, hipStream_t st, int phase) {
#define MH_CALL(N) mh_bwd_launch<N>(x, alpha, y, dy, dx, de, B, T, C, l, st, phase)
  MH_DISPATCH(n, MH_CALL)
#undef MH_CALL
}

}  // namespace

extern "C" int dlip_mh_attn_scores_f32(const float* hidden, const float* v, const float* k, const int32_t* head_off, const int32_t* len,
                                       int32_t len_add, float* alpha, int32_t B, int32_t T, int32_t S, int32_t n, dlip_stream_t stream) {
  DLIP_CHECK_ARG(hidden && v && k && (head_off || n == 1) && alpha);
  DLIP_CHECK_ARG(n >= 1 && n <= kMaxHeads && B > 0 && B <= 65535 && T > 0 && T <= 16000 && S >= n);
  DlipLen l; l.len = len; l.mul = 1; l.add = len_add;
  hipStream_t st = dlip_hip_stream(stream);
  hipLaunchKernelGGL(mh_energy_kernel, dim3(mh_row_grid((long long)B * T)), dim3(256), 0, st, hidden, v, k, head_off, alpha, B, T, S, n, l);
  int e = dlip_launch_status();
  if (e != DLIP_OK) return e;
  hipLaunchKernelGGL(mh_softmax_kernel, dim3(n, B), dim3(256), 0, st, alpha, T, n, l);
  return dlip_launch_status();
}

extern "C" int dlip_mh_attn_stat_pool_f32(const float* x, const float* alpha, const int32_t* len, int32_t len_add, float eps, float* y,
                                          int32_t B, int32_t T, int32_t C, int32_t n, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && alpha && y);
  DLIP_CHECK_ARG(n >= 1 && n <= kMaxHeads && B > 0 && B <= 65535 && T > 0 && T <= 16000 && C > 0 && (C & 3) == 0 && eps >= 0.f);
  DLIP_CHECK_ARG((size_t)3 * n * C * sizeof(float) <= kMaxLds);       // the backward's bound: what it could not differentiate is refused here
  DLIP_CHECK_ARG(dlip_aligned16(x));
  DlipLen l; l.len = len; l.mul = 1; l.add = len_add;
  return mh_stat_dispatch(n, x, alpha, y, B, T, C, l, eps, dlip_hip_stream(stream));
}

extern "C" int dlip_mh_attn_stat_pool_bwd_f32(const float* x, const float* hidden, const float* v, const int32_t* head_off,
                                              const float* alpha, const float* y, const float* dy, const int32_t* len, int32_t len_add,
                                              float eps, float* dx, float* dhidden, float* rde, float* de, float* dek, int32_t B,
                                              int32_t T, int32_t C, int32_t S, int32_t n, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && hidden && v && (head_off || n == 1) && alpha && y && dy && dx && dhidden && rde && de && dek);
  DLIP_CHECK_ARG(n >= 1 && n <= kMaxHeads && B > 0 && B <= 65535 && T > 0 && T <= 16000 && C > 0 && (C & 3) == 0 && S >= n);
  DLIP_CHECK_ARG(eps >= 0.f);      // > 0 keeps the std read from y away from zero; 0: the reference's 0 / 0 at a frame-constant feature
  DLIP_CHECK_ARG((size_t)3 * n * C * sizeof(float) <= kMaxLds);
  DLIP_CHECK_ARG(dlip_aligned16(x, y, dy, dx));
  DlipLen l; l.len = len; l.mul = 1; l.add = len_add;
  hipStream_t st = dlip_hip_stream(stream);
  int e = mh_bwd_dispatch(n, x, alpha, y, dy, dx, de, B, T, C, l, st, 0);
  if (e != DLIP_OK) return e;
  hipLaunchKernelGGL(mh_softmax_bwd_kernel, dim3(n, B), dim3(256), 0, st, alpha, de, dek, T, n, l);
  e = dlip_launch_status();
  if (e != DLIP_OK) return e;
  e = mh_bwd_dispatch(n, x, alpha, y, dy, dx, de, B, T, C, l, st, 1);
  if (e != DLIP_OK) return e;
  hipLaunchKernelGGL(mh_dhidden_kernel, dim3(mh_row_grid((long long)B * T)), dim3(256), 0, st, hidden, v, de, head_off, dhidden, rde, B, T, S,
                     n, l);
  return dlip_launch_status();
}

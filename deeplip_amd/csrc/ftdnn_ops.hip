// The factorized TDNN speech encoder, `arch: ftdnn` (conf/audio_config.yaml:84-92 names the architecture, upstream ships no source for
// it: include/deeplip_hip.h and DESIGN.md 4k are the definition).  Two things the TDNN kernels do not already serve:
//   (a) the SEMI-ORTHOGONAL STEP on every factor matrix M [rows, cols] (Povey et al. 2018; Kaldi's ConstrainOrthonormalInternal with a
//       floating scale), one launch pair for all matrices of a model, gated by a step counter that lives on the device;
//   (b) the BYPASS y[b, t, :] += s x[b, t + shift, :] of a block whose widths agree, forward (fp32 or split activation format on either
//       side) and backward (scattered into the data gradient of the factor convolution, in place).
// Every product is an fp32 fma on the vector ALUs, every sum runs in an order the shapes alone decide: a replayed step equals the eager one
// bit for bit, and a row of the bypass has the same bits whatever batch it sits in.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int kRows = DLIP_SEMI_ORTH_MAX_ROWS;        // 128: P = M M^T is at most 64 KB of LDS in the update kernel
constexpr int kSplits = DLIP_SEMI_ORTH_SPLITS;        // workgroups that share the columns of one matrix in the Gram kernel
constexpr int kPanel = DLIP_SEMI_ORTH_PANEL;          // columns one workgroup of the update kernel rewrites
constexpr int kGramElems = kRows * kRows;

struct SemiOrthMat {       // one row of the device table (16 bytes): the matrix, row-major, row pitch = cols
  float* M;
  int32_t rows, cols;
};
static_assert(sizeof(SemiOrthMat) == 16, "the device table's row");

__device__ __forceinline__ bool semi_orth_ok(const SemiOrthMat& m, int max_rows, int max_cols) {
  return m.M != nullptr && m.rows >= 1 && m.rows <= max_rows && m.rows <= kRows && m.cols >= m.rows && m.cols <= max_cols;
}

// columns per split of a matrix with `cols` columns (whole 32-column tiles), and how many splits then hold any
__device__ __forceinline__ int semi_orth_chunk(int cols) { return ((cols + kSplits - 1) / kSplits + 31) / 32 * 32; }

// The hand-off of the convolution kernels' split and of the column reductions (encoder_train_ops.hip): shares are
// written through (agent-scope relaxed stores), every storing wave drains them, ONE ticket per workgroup; the workgroup that takes the
// last of `n` re-zeroes the word for the next launch and drops its stale cache lines.  No workgroup waits for another.
__device__ __forceinline__ void so_publish(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ bool so_last_arrival(int* word, int n) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = __hip_atomic_fetch_add(word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == n - 1;
    if (s_last) __hip_atomic_store(word, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const bool last = s_last != 0;
  if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return last;
}

// Phase 1, grid (kSplits, n_mats): P = M M^T as a split-K reduction.  Workgroup (s, m) multiplies its chunk of columns -- 32-column tiles
// through LDS, thread (ty, tx) of 16 x 16 the entries (ty + 16 i, tx + 16 j) -- and publishes the partial; the last to arrive adds the
// partials in split order and leaves P.  counter[0] = optimizer steps so far; the step is due on step n = counter[0] + 1 when
// every > 0 and n % every == 0.  Nobody writes counter[0] here (phase 2 advances it); counter[1] hands `due` to phase 2.
__global__ __launch_bounds__(256) void semi_orth_gram_kernel(const SemiOrthMat* __restrict__ table, int max_rows, int max_cols,
                                                             int32_t* __restrict__ counter, int every, int* __restrict__ tickets,
                                                             float* __restrict__ ws) {
  __shared__ float tile[32][kRows + 1];
  const long long n1 = (long long)counter[0] + 1;
  const bool due = every > 0 && n1 % every == 0;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) counter[1] = due ? 1 : 0;
  if (!due) return;
  const SemiOrthMat m = table[blockIdx.y];
  if (!semi_orth_ok(m, max_rows, max_cols)) return;
  const int R = m.rows, Cn = m.cols;
  const int chunk = semi_orth_chunk(Cn);
  const int n_active = (Cn + chunk - 1) / chunk;
  if ((int)blockIdx.x >= n_active) return;
  const int c0 = blockIdx.x * chunk, c1 = min(Cn, c0 + chunk);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int ni = (R + 15) >> 4;                      // 16-row groups that hold any row
  float acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  const int lk = threadIdx.x & 31, lr = threadIdx.x >> 5;
  for (int cb = c0; cb < c1; cb += 32) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = lr + 8 * i, c = cb + lk;
      tile[lk][r] = (r < R && c < c1) ? m.M[(long long)r * Cn + c] : 0.f;
    }
    __syncthreads();
    for (int kk = 0; kk < 32; ++kk) {
      float a[8], b[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { a[i] = tile[kk][ty + 16 * i]; b[i] = tile[kk][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i < ni) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
      }
    }
  }
  float* base = ws + (long long)blockIdx.y * (kSplits + 1) * kGramElems;
  float* part = base + (long long)blockIdx.x * kGramElems;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = ty + 16 * i, c = tx + 16 * j;
      if (r < R && c < R) so_publish(part + r * R + c, acc[i][j]);
    }
  if (!so_last_arrival(tickets + blockIdx.y, n_active)) return;
  float* P = base + (long long)kSplits * kGramElems;
  for (int e = threadIdx.x; e < R * R; e += 256) {
    float p = base[e];
    for (int s = 1; s < n_active; ++s) p += base[(long long)s * kGramElems + e];
    P[e] = p;
  }
}

// Phase 2, grid (ceil(max_cols / kPanel), n_mats), dynamic LDS: [8 doubles | P, R x R | a panel of M, R x kPanel].  Every workgroup derives
// tp = tr P and tpp = |P|_F^2 itself, in fp64 and in one fixed order (thread-strided, wave butterflies, waves in order), hence the same
// alpha2 and nu in all of them, and rewrites its panel:  M <- M - (4 nu / alpha2) (P M - alpha2 M).  A matrix with tr P = 0 is left alone.
// Workgroup (0, 0) advances the counter: no workgroup of this kernel reads counter[0].
__global__ __launch_bounds__(256) void semi_orth_update_kernel(const SemiOrthMat* __restrict__ table, int max_rows, int max_cols,
                                                               int32_t* __restrict__ counter, const float* __restrict__ ws) {
  extern __shared__ float so_lds[];
  const bool due = counter[1] != 0;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) counter[0] = counter[0] + 1;
  if (!due) return;
  const SemiOrthMat m = table[blockIdx.y];
  if (!semi_orth_ok(m, max_rows, max_cols)) return;
  const int R = m.rows, Cn = m.cols;
  const int c0 = blockIdx.x * kPanel;
  if (c0 >= Cn) return;
  double* red = reinterpret_cast<double*>(so_lds);
  float* Ps = so_lds + 16;
  float* Mp = Ps + R * R;
  const float* P = ws + ((long long)blockIdx.y * (kSplits + 1) + kSplits) * kGramElems;
  for (int e = threadIdx.x; e < R * R; e += 256) Ps[e] = P[e];
  for (int e = threadIdx.x; e < R * kPanel; e += 256) {
    const int r = e / kPanel, c = c0 + (e % kPanel);
    Mp[e] = c < Cn ? m.M[(long long)r * Cn + c] : 0.f;
  }
  __syncthreads();
  double tp = 0.0, tpp = 0.0;
  for (int e = threadIdx.x; e < R * R; e += 256) {
    const double v = (double)Ps[e];
    tpp += v * v;
    if (e / R == e % R) tp += v;
  }
  tp = dlip_block_sum4(tp, red);
  __syncthreads();
  tpp = dlip_block_sum4(tpp, red);
  if (!(tp > 0.0)) return;
  const double alpha2 = tpp / tp;
  const double ratio = tpp * (double)R / (tp * tp);
  double nu = 0.125;
  if (ratio > 1.02) nu *= 0.5;
  if (ratio > 1.1) nu *= 0.5;
  const float a2 = (float)alpha2, cf = (float)(4.0 * nu / alpha2);
  const int col = threadIdx.x & (kPanel - 1), g = threadIdx.x >> 6;       // a wave = one row group, 64 consecutive columns
  float acc[kRows / 4];
#pragma unroll
  for (int i = 0; i < kRows / 4; ++i) acc[i] = 0.f;
  for (int k = 0; k < R; ++k) {
    const float mv = Mp[k * kPanel + col];
#pragma unroll
    for (int i = 0; i < kRows / 4; ++i) {
      const int r = g + 4 * i;
      if (r < R) acc[i] = fmaf(Ps[r * R + k], mv, acc[i]);
    }
  }
  if (c0 + col < Cn) {
#pragma unroll
    for (int i = 0; i < kRows / 4; ++i) {
      const int r = g + 4 * i;
      if (r < R) {
        const float mv = Mp[r * kPanel + col];
        m.M[(long long)r * Cn + c0 + col] = mv - cf * (acc[i] - a2 * mv);
      }
    }
  }
}

typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// four channels of a [rows, C] tensor at float4 index i (C % 32 == 0 in the split format: 8 float4 per 128-byte block of 32 hi | 32 lo halves)
__device__ __forceinline__ f32x4 load4(const float* p, long long i, bool split) {
  if (!split) return reinterpret_cast<const f32x4*>(p)[i];
  const float* b = p + (i >> 3) * 32;
  const int q = (int)(i & 7);
  const h4 hi = *reinterpret_cast<const h4*>(b + q * 2), lo = *reinterpret_cast<const h4*>(b + 16 + q * 2);
  f32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (float)hi[k] + (float)lo[k];
  return v;
}

// out[b, t, :] = y[b, t, :] + s x[b, t + shift, :]; y fp32 [B, Tp, C], x [B, T, C] and out [B, Tp, C] fp32 or split.  One lane per four
// channels; what a lane computes depends on its own (b, t, c) alone.
__global__ __launch_bounds__(256) void ftdnn_bypass_kernel(const float* __restrict__ y, const float* __restrict__ x, float* __restrict__ out,
                                                           long long n4, int T, int Tp, int C4, int shift, float s, int x_split,
                                                           int out_split, DlipRange status) {
  float amax = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const long long row = i / C4;
    const int c4 = (int)(i - row * C4);
    const long long b = row / Tp;
    const int t = (int)(row - b * Tp);
    const f32x4 yv = reinterpret_cast<const f32x4*>(y)[i];
    const f32x4 xv = load4(x, (b * T + t + shift) * C4 + c4, x_split != 0);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fmaf(s, xv[k], yv[k]);
    if (!out_split) {
      reinterpret_cast<f32x4*>(out)[i] = v;
    } else {
      h4 hi, lo;
#pragma unroll
      for (int k = 0; k < 4; ++k) { hi[k] = (_Float16)v[k]; lo[k] = (_Float16)(v[k] - (float)hi[k]); amax = fmaxf(amax, fabsf(v[k])); }
      float* bo = out + (i >> 3) * 32;
      const int q = (int)(i & 7);
      *reinterpret_cast<h4*>(bo + q * 2) = hi;
      *reinterpret_cast<h4*>(bo + 16 + q * 2) = lo;
    }
  }
  if (out_split) dlip_report_range_block(amax, status);      // (kernel-uniform)
}

// dx[b, t + shift, :] += s dy[b, t, :]: the bypass's share of the block input's gradient, added to the factor convolution's data gradient
__global__ __launch_bounds__(256) void ftdnn_bypass_bwd_kernel(const f32x4* __restrict__ dy, f32x4* __restrict__ dx, long long n4, int T, int Tp,
                                                               int C4, int shift, float s) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const long long row = i / C4;
    const int c4 = (int)(i - row * C4);
    const long long b = row / Tp;
    const int t = (int)(row - b * Tp);
    const f32x4 g = dy[i];
    f32x4* p = dx + (b * T + t + shift) * C4 + c4;
    f32x4 v = *p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fmaf(s, g[k], v[k]);
    *p = v;
  }
}

constexpr long long kGridCap = 2048;

}  // namespace

extern "C" int64_t dlip_semi_orth_workspace_bytes(int32_t n_mats) {
  if (n_mats < 1 || n_mats > DLIP_SEMI_ORTH_MAX_MATS) return -1;
  // [ticket words, one per matrix, a whole 256-byte line][per matrix: kSplits partial Gram matrices, then P]
  return 256 + (int64_t)n_mats * (kSplits + 1) * kGramElems * 4;
}

extern "C" int dlip_semi_orth_step_f32(const void* table, int32_t n_mats, int32_t max_rows, int32_t max_cols, int32_t* counter, int32_t every,
                                       void* workspace, int64_t workspace_bytes, dlip_stream_t stream) {
  DLIP_CHECK_ARG(table && counter && workspace && n_mats >= 1 && n_mats <= DLIP_SEMI_ORTH_MAX_MATS && every >= 0);
  DLIP_CHECK_ARG(max_rows >= 1 && max_rows <= kRows && max_cols >= max_rows);
  DLIP_CHECK_ARG(workspace_bytes >= dlip_semi_orth_workspace_bytes(n_mats) && dlip_aligned16(table, workspace) && dlip_aligned<4>(counter));
  static_assert(DLIP_SEMI_ORTH_MAX_MATS * 4 <= 256, "the ticket words' line");
  int* tickets = static_cast<int*>(workspace);
  float* ws = reinterpret_cast<float*>(static_cast<char*>(workspace) + 256);
  const SemiOrthMat* tab = static_cast<const SemiOrthMat*>(table);
  hipStream_t st = dlip_hip_stream(stream);
  static DlipKernelState ks;
  const size_t lds = 64 + ((size_t)max_rows * max_rows + (size_t)max_rows * kPanel) * 4;
  int rc = ks.ensure_lds(reinterpret_cast<const void*>(semi_orth_update_kernel), lds);
  if (rc != DLIP_OK) return rc;
  hipLaunchKernelGGL(semi_orth_gram_kernel, dim3(kSplits, (unsigned)n_mats), dim3(256), 0, st, tab, max_rows, max_cols, counter, every, tickets, ws);
  rc = dlip_launch_status();
  if (rc != DLIP_OK) return rc;
  hipLaunchKernelGGL(semi_orth_update_kernel, dim3((unsigned)((max_cols + kPanel - 1) / kPanel), (unsigned)n_mats), dim3(256), lds, st, tab,
                     max_rows, max_cols, counter, ws);
  return dlip_launch_status();
}

extern "C" int dlip_ftdnn_bypass_f32(const float* y, const float* x, float* out, int32_t B, int32_t T, int32_t Tp, int32_t C, int32_t shift,
                                     float scale, int32_t flags, dlip_stream_t stream) {
  DLIP_CHECK_ARG(y && x && out && B > 0 && T > 0 && Tp > 0 && C > 0 && (C & 3) == 0 && shift >= 0 && (long long)shift + Tp <= T);
  DLIP_CHECK_ARG((flags & ~3) == 0 && (!(flags & 3) || (C & 31) == 0) && out != x && (out != y || !(flags & 2)) && dlip_aligned16(y, x, out));
  const long long n4 = (long long)B * Tp * (C / 4);
  hipLaunchKernelGGL(ftdnn_bypass_kernel, dim3(dlip_grid1d(n4, kGridCap)), dim3(256), 0, dlip_hip_stream(stream), y, x, out, n4, T, Tp, C / 4,
                     shift, scale, flags & 1, (flags >> 1) & 1, dlip_range_for(DLIP_ST_PACK));
  return dlip_launch_status();
}

extern "C" int dlip_ftdnn_bypass_bwd_f32(const float* dy, float* dx, int32_t B, int32_t T, int32_t Tp, int32_t C, int32_t shift, float scale,
                                         dlip_stream_t stream) {
  DLIP_CHECK_ARG(dy && dx && dy != dx && B > 0 && T > 0 && Tp > 0 && C > 0 && (C & 3) == 0 && shift >= 0 && (long long)shift + Tp <= T);
  DLIP_CHECK_ARG(dlip_aligned16(dy, dx));
  const long long n4 = (long long)B * Tp * (C / 4);
  hipLaunchKernelGGL(ftdnn_bypass_bwd_kernel, dim3(dlip_grid1d(n4, kGridCap)), dim3(256), 0, dlip_hip_stream(stream),
                     reinterpret_cast<const f32x4*>(dy), reinterpret_cast<f32x4*>(dx), n4, T, Tp, C / 4, shift, scale);
  return dlip_launch_status();
}

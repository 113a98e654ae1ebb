// Depthwise dilated temporal convolution of the depthwise-separable TCN heads (tcn_dwpw, models/video_models/tcn.py:31-43,155-181),
// exact fp32 on the vector ALUs (no MFMA content: one multiply-add per tap and channel).
//
//   dlip_tcn_dw_fwd_f32     z[b,t,c] = act(sum_j w[j,c] x[b, t - P + j d, c] + bias[c]), zeros outside [0, T)
//   dlip_tcn_dw_dgrad_f32   dx[b,s,c] = sum_branch sum_j w[j,c] dz[b, s + P - j d, c], zeros outside [0, T_out)
//   dlip_tcn_dw_wgrad_f32   dw[j,c] = sum_{b,t} dz[b,t,c] x[b, t - P + j d, c]: fp64 partial sums per row chunk, then a second pass
//                           that adds the chunks in a fixed order (no atomics: a replayed step gives the eager step's bits)
//
// Layout: channels-last [B, T, C] fp32, C % 4 == 0, weights tap-major [k][C].  Every thread owns one channel quad (float4 loads and
// stores along C) of one row; a launch serves up to DW_MAX_BR branches that read the same input (the kernel sizes of one dwpw MS-TCN
// stage), one grid row per branch.
#include "dlip_launch.h"

namespace {

constexpr int DW_MAX_BR = 4;
constexpr int DW_MAX_K = 64;
constexpr int WG_ROWS = 32;  // rows of dz per weight-gradient chunk

struct DwBranch {
  const float* w;      // [k][C]
  const float* bias;   // [C] or NULL (forward)
  const float* slope;  // [C] or NULL = identity (forward)
  float* y;            // forward: [B, t_out, C]; weight gradient: dw [k][C]
  const float* dz;     // [B, t_out, C] (gradients)
  double* ws;          // weight gradient: [chunks][k][C]
  int k, pad, t_out, chunks;
};

struct DwArgs {
  const float* x;  // forward / weight gradient: [B, T, C]
  float* dx;       // data gradient: [B, T, C]
  DwBranch br[DW_MAX_BR];
  int n, B, T, C4, d;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__global__ __launch_bounds__(256) void tcn_dw_fwd_kernel(const DwArgs a) {
  const DwBranch& br = a.br[blockIdx.y];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)a.B * br.t_out * a.C4;
  if (i >= total) return;
  const int c4 = (int)(i % a.C4);
  const long long row = i / a.C4;
  const int t = (int)(row % br.t_out);
  const int b = (int)(row / br.t_out);
  const int C = a.C4 * 4;
  const float* xb = a.x + (size_t)b * a.T * C + c4 * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < br.k; ++j) {
    const int ti = t - br.pad + j * a.d;
    if (ti < 0 || ti >= a.T) continue;
    const f32x4 wv = ld4(br.w + (size_t)j * C + c4 * 4);
    const f32x4 xv = ld4(xb + (size_t)ti * C);
    for (int q = 0; q < 4; ++q) acc[q] = fmaf(wv[q], xv[q], acc[q]);
  }
  if (br.bias) acc += ld4(br.bias + c4 * 4);
  if (br.slope) {
    const f32x4 s = ld4(br.slope + c4 * 4);
    for (int q = 0; q < 4; ++q) acc[q] = acc[q] < 0.f ? acc[q] * s[q] : acc[q];
  }
  *reinterpret_cast<f32x4*>(br.y + (size_t)row * C + c4 * 4) = acc;
}

__global__ __launch_bounds__(256) void tcn_dw_dgrad_kernel(const DwArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)a.B * a.T * a.C4;
  if (i >= total) return;
  const int c4 = (int)(i % a.C4);
  const long long row = i / a.C4;
  const int s = (int)(row % a.T);
  const int b = (int)(row / a.T);
  const int C = a.C4 * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < a.n; ++r) {
    const DwBranch& br = a.br[r];
    const float* gb = br.dz + (size_t)b * br.t_out * C + c4 * 4;
    for (int j = 0; j < br.k; ++j) {
      const int to = s + br.pad - j * a.d;
      if (to < 0 || to >= br.t_out) continue;
      const f32x4 wv = ld4(br.w + (size_t)j * C + c4 * 4);
      const f32x4 gv = ld4(gb + (size_t)to * C);
      for (int q = 0; q < 4; ++q) acc[q] = fmaf(wv[q], gv[q], acc[q]);
    }
  }
  *reinterpret_cast<f32x4*>(a.dx + (size_t)row * C + c4 * 4) = acc;
}

// Pass 1: one wave per (channel block of 64 quads, row chunk, branch); lane = channel quad, the chunk's WG_ROWS rows in order.
__global__ __launch_bounds__(64) void tcn_dw_wgrad_partial_kernel(const DwArgs a) {
  const DwBranch& br = a.br[blockIdx.z];
  const int chunk = blockIdx.y;
  if (chunk >= br.chunks) return;
  const int c4 = blockIdx.x * 64 + threadIdx.x;
  if (c4 >= a.C4) return;
  const int C = a.C4 * 4;
  double* out = br.ws + (size_t)chunk * br.k * C + c4 * 4;
  const long long rows = (long long)a.B * br.t_out;
  const long long r0 = (long long)chunk * WG_ROWS;
  const long long r1 = r0 + WG_ROWS < rows ? r0 + WG_ROWS : rows;
  for (int j0 = 0; j0 < br.k; j0 += 8) {      // taps in blocks of 8: 32 fp64 accumulators per lane
    const int nj = br.k - j0 < 8 ? br.k - j0 : 8;
    double s[8][4];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) s[j][q] = 0.0;
    for (long long r = r0; r < r1; ++r) {
      const int t = (int)(r % br.t_out);
      const int b = (int)(r / br.t_out);
      const f32x4 g = ld4(br.dz + (size_t)r * C + c4 * 4);
      const float* xb = a.x + (size_t)b * a.T * C + c4 * 4;
#pragma unroll
      for (int j = 0; j < 8; ++j) {          // (fully unrolled: the accumulators stay in registers)
        const int ti = t - br.pad + (j0 + j) * a.d;
        if (j < nj && ti >= 0 && ti < a.T) {
          const f32x4 xv = ld4(xb + (size_t)ti * C);
#pragma unroll
          for (int q = 0; q < 4; ++q) s[j][q] = fma((double)g[q], (double)xv[q], s[j][q]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nj)
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(size_t)(j0 + j) * C + q] = s[j][q];
  }
}

// Pass 2: dw[j][c] = sum over chunks in index order (fp64), rounded once to fp32.
__global__ __launch_bounds__(256) void tcn_dw_wgrad_reduce_kernel(const DwArgs a) {
  const DwBranch& br = a.br[blockIdx.y];
  const int C = a.C4 * 4;
  const int i = blockIdx.x * 256 + threadIdx.x;      // (j, c4)
  if (i >= br.k * a.C4) return;
  const int j = i / a.C4, c4 = i % a.C4;
  const size_t stride = (size_t)br.k * C;
  const double* p = br.ws + (size_t)j * C + c4 * 4;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 8
  for (int ch = 0; ch < br.chunks; ++ch) {      // (unrolled: the loads of 8 chunks are in flight together; the sum keeps chunk order)
    const double* q = p + ch * stride;
    s0 += q[0]; s1 += q[1]; s2 += q[2]; s3 += q[3];
  }
  f32x4 v = {(float)s0, (float)s1, (float)s2, (float)s3};
  *reinterpret_cast<f32x4*>(br.y + (size_t)j * C + c4 * 4) = v;
}


// Checks shared by the three entry points; fills the branch table's geometry.
int dw_setup(DwArgs& a, int32_t n, const int32_t* k, const int32_t* pad, const int32_t* t_out, int32_t B, int32_t T, int32_t C,
             int32_t d) {
  DLIP_CHECK_ARG(n >= 1 && n <= DW_MAX_BR && k && pad && t_out);
  DLIP_CHECK_ARG(B > 0 && T > 0 && C > 0 && (C & 3) == 0 && d > 0);
  if ((long long)B * T * C > DLIP_MAX_BUFFER_BYTES / 4) return DLIP_ERANGE;
  a.n = n; a.B = B; a.T = T; a.C4 = C / 4; a.d = d;
  for (int r = 0; r < n; ++r) {
    DLIP_CHECK_ARG(k[r] >= 1 && k[r] <= DW_MAX_K && pad[r] >= 0 && t_out[r] > 0);
    if ((long long)B * t_out[r] * C > DLIP_MAX_BUFFER_BYTES / 4 || (long long)(k[r] - 1) * d > 0x3FFFFFFF ||
        (long long)pad[r] + t_out[r] > 0x3FFFFFFF)
      return DLIP_ERANGE;
    a.br[r] = DwBranch{};
    a.br[r].k = k[r]; a.br[r].pad = pad[r]; a.br[r].t_out = t_out[r];
  }
  return DLIP_OK;
}

}  // namespace

extern "C" int dlip_tcn_dw_fwd_f32(const float* x, int32_t n, const float* const* w, const float* const* bias,
                                   const float* const* slope, float* const* y, const int32_t* k, const int32_t* pad,
                                   const int32_t* t_out, int32_t B, int32_t T, int32_t C, int32_t d, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && w && y && dlip_aligned16(x));
  DwArgs a;
  a.x = x; a.dx = nullptr;
  const int st = dw_setup(a, n, k, pad, t_out, B, T, C, d);
  if (st != DLIP_OK) return st;
  long long most = 0;
  for (int r = 0; r < n; ++r) {
    DLIP_CHECK_ARG(w[r] && y[r] && dlip_aligned16(w[r], y[r]));
    a.br[r].w = w[r];
    a.br[r].bias = bias ? bias[r] : nullptr;
    a.br[r].slope = slope ? slope[r] : nullptr;
    DLIP_CHECK_ARG(dlip_aligned16(a.br[r].bias, a.br[r].slope));
    a.br[r].y = y[r];
    const long long tot = (long long)B * t_out[r] * (C / 4);
    most = tot > most ? tot : most;
  }
  if ((most + 255) / 256 > 0x7FFFFFFFll) return DLIP_ERANGE;
  hipLaunchKernelGGL(tcn_dw_fwd_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)n), dim3(256), 0,
                     dlip_hip_stream(stream), a);
  return dlip_launch_status();
}

extern "C" int dlip_tcn_dw_dgrad_f32(const float* const* dz, int32_t n, const float* const* w, const int32_t* k, const int32_t* pad,
                                     const int32_t* t_out, float* dx, int32_t B, int32_t T, int32_t C, int32_t d,
                                     dlip_stream_t stream) {
  DLIP_CHECK_ARG(dz && w && dx && dlip_aligned16(dx));
  DwArgs a;
  a.x = nullptr; a.dx = dx;
  const int st = dw_setup(a, n, k, pad, t_out, B, T, C, d);
  if (st != DLIP_OK) return st;
  for (int r = 0; r < n; ++r) {
    DLIP_CHECK_ARG(dz[r] && w[r] && dlip_aligned16(dz[r], w[r]));
    a.br[r].dz = dz[r];
    a.br[r].w = w[r];
  }
  const long long total = (long long)B * T * (C / 4);
  hipLaunchKernelGGL(tcn_dw_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, dlip_hip_stream(stream), a);
  return dlip_launch_status();
}

extern "C" int dlip_tcn_dw_wgrad_chunks(int32_t rows) { return rows > 0 ? (rows + WG_ROWS - 1) / WG_ROWS : 0; }

extern "C" int dlip_tcn_dw_wgrad_f32(const float* x, int32_t n, const float* const* dz, float* const* dw, const int32_t* k,
                                     const int32_t* pad, const int32_t* t_out, int32_t B, int32_t T, int32_t C, int32_t d,
                                     double* workspace, int64_t workspace_len, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && dz && dw && workspace && dlip_aligned16(x));
  DwArgs a;
  a.x = x; a.dx = nullptr;
  const int st = dw_setup(a, n, k, pad, t_out, B, T, C, d);
  if (st != DLIP_OK) return st;
  long long off = 0;
  int most_chunks = 0, most_k = 0;
  for (int r = 0; r < n; ++r) {
    DLIP_CHECK_ARG(dz[r] && dw[r] && dlip_aligned16(dz[r], dw[r]));
    a.br[r].dz = dz[r];
    a.br[r].y = dw[r];
    a.br[r].chunks = dlip_tcn_dw_wgrad_chunks(B * t_out[r]);
    a.br[r].ws = workspace + off;
    off += (long long)a.br[r].chunks * k[r] * C;
    most_chunks = a.br[r].chunks > most_chunks ? a.br[r].chunks : most_chunks;
    most_k = k[r] > most_k ? k[r] : most_k;
  }
  DLIP_CHECK_ARG(off <= workspace_len);
  if (most_chunks > 65535) return DLIP_ERANGE;
  hipStream_t s = dlip_hip_stream(stream);
  hipLaunchKernelGGL(tcn_dw_wgrad_partial_kernel, dim3((unsigned)((C / 4 + 63) / 64), (unsigned)most_chunks, (unsigned)n), dim3(64), 0,
                     s, a);
  const int e = dlip_launch_status();
  if (e != DLIP_OK) return e;
  hipLaunchKernelGGL(tcn_dw_wgrad_reduce_kernel, dim3((unsigned)((most_k * (C / 4) + 255) / 256), (unsigned)n), dim3(256), 0, s, a);
  return dlip_launch_status();
}

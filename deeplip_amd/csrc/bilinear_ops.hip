// Low-rank bilinear pooling head (ABI 54): deeplip_amd.fusion.BNBilinear, the class train_fusion.py:84 of the reference asks for
// (LBP.BNBilinear) and LBP.py does not define.  It follows LBP.py:38-44 without the signed square root:
//
//   P = e1 U [B, k o]   Q = e2 V [B, k o]   z[b,j] = mean_{i<k} P[b, j k + i] Q[b, j k + i]   (then F.normalize and BatchNorm1d)
//
// Exact fp32 on v_mfma_f32_16x16x4_f32 under every arithmetic mode; every sum has a fixed order, there is no split of a reduction
// over workgroups and no float atomic: a replayed launch repeats the bits.
//
//   forward : one workgroup owns `opt` pooled outputs (opt k columns of U and V, at most 64 per pass).  The weight columns are
//             staged through LDS in 32-deep chunks (registers hold the next chunk while the MFMAs run on this one); the four waves
//             take one 16-row tile each, so a pass covers 64 batch rows and a larger batch loops over row groups with the same
//             columns.  P and Q meet in registers; their product goes through LDS once to be summed over k.  P and Q are written
//             only when the caller keeps them for the backward pass.
//   bwd (w) : dU = e1^T dP, dV = e2^T dQ with dP = dz/k * Q and dQ = dz/k * P formed on load into LDS; one workgroup owns a 64-column
//             stripe of both gradients and reduces over the batch by itself.
//   bwd (x) : de1 = dP U^T, de2 = dQ V^T; one workgroup per 16 x 16 output tile, its four waves split the k o reduction and are summed
//             in wave order through LDS.
//   finish  : eval mode's F.normalize + folded BatchNorm, one workgroup per row.
//
// MFMA operand maps (16x16x4 f32): lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; a lane loads FOUR
// consecutive floats, and MFMA j of a group takes element j from every lane.  Along the reduction that only permutes the order of
// the sum (the same for both operands); along the columns of B it makes accumulator `cb` of lane l hold column 4 (l & 15) + cb.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int BL_ROWS = 64;     // batch rows of a forward pass: four waves x one 16-row tile
constexpr int BL_COLS = 64;     // columns of a pass (four column blocks per lane)
constexpr int BL_KC = 32;       // depth of a staged weight chunk
constexpr int BL_BWD_ROWS = 96; // batch rows of dP | dQ held in LDS by the weight-gradient kernel

// Four consecutive floats of a row with n elements, from column c on; elements at or beyond n read as zero.  vec: n % 4 == 0, c % 4 == 0 and
// the row 16-byte aligned.
__device__ __forceinline__ f32x4 bl_load4(const float* __restrict__ row, int c, int n, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if (c < n) v = *reinterpret_cast<const f32x4*>(row + c);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < n) v[j] = row[c + j];
  }
  return v;
}

template <bool SAVE>
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const float* __restrict__ e1, const float* __restrict__ e2,
                                                           const float* __restrict__ U, const float* __restrict__ V,
                                                           float* __restrict__ z, float* __restrict__ P, float* __restrict__ Q, int B,
                                                           int d1, int d2, int o, int k, int opt, int vec) {
  // [buffer][U | V][depth][column]; the products of a pass reuse the first 64 x 65 floats once the last chunk has been consumed
  __shared__ __attribute__((aligned(16))) float ws[2 * 2 * BL_KC * BL_COLS];
  __shared__ float zs[BL_ROWS * BL_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kg = lane >> 4;
  const int ko = k * o;
  const int dmax = d1 > d2 ? d1 : d2;
  const int j0 = blockIdx.x * opt;
  const int nj = (o - j0) < opt ? (o - j0) : opt;
  const int start = j0 * k, c_end = (j0 + nj) * k;
  const int c_lo = vec ? (start & ~3) : start;
  const bool v4 = vec != 0;
  const int nchunk = (dmax + BL_KC - 1) / BL_KC;

  for (int m0 = 0; m0 < B; m0 += BL_ROWS) {
    const int arow = m0 + wave * 16 + r;
    const bool a_ok = arow < B;
    const float* pa1 = e1 + (size_t)(a_ok ? arow : 0) * d1;
    const float* pa2 = e2 + (size_t)(a_ok ? arow : 0) * d2;
    for (int c = c_lo; c < c_end; c += BL_COLS) {
      f32x4 accP[4], accQ[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        accP[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        accQ[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      f32x4 wreg[4], a1[2], a2[2];
      // chunk `ch` of both matrices into registers: 32 x 64 x 2 floats = 1024 float4, four per thread
      auto fetch = [&](int ch) {
        const int dbase = ch * BL_KC;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int idx = tid + 256 * q;
          const int mat = idx >> 9, rr = (idx & 511) >> 4, c4 = idx & 15;
          const int d = dbase + rr;
          const float* W = mat ? V : U;
          const int dm = mat ? d2 : d1;
          wreg[q] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (d < dm) wreg[q] = bl_load4(W + (size_t)d * ko, c + 4 * c4, ko, v4);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int d = dbase + 16 * s + 4 * kg;
          a1[s] = f32x4{0.f, 0.f, 0.f, 0.f};
          a2[s] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (a_ok && d < d1) a1[s] = *reinterpret_cast<const f32x4*>(pa1 + d);      // d1 % 4 == 0
          if (a_ok && d < d2) a2[s] = *reinterpret_cast<const f32x4*>(pa2 + d);
        }
      };
      auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int idx = tid + 256 * q;
          *reinterpret_cast<f32x4*>(&ws[buf * (2 * BL_KC * BL_COLS) + 4 * idx]) = wreg[q];     // [mat][rr][4 c4] is idx in float4 units
        }
      };
      fetch(0);
      stash(0);
      __syncthreads();
      for (int ch = 0; ch < nchunk; ++ch) {
        const f32x4 b1[2] = {a1[0], a1[1]}, b2[2] = {a2[0], a2[1]};
        if (ch + 1 < nchunk) fetch(ch + 1);
        const float* wu = &ws[(ch & 1) * (2 * BL_KC * BL_COLS)];
        const float* wv = wu + BL_KC * BL_COLS;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int dd = 16 * s + 4 * kg + j;
            const f32x4 u4 = *reinterpret_cast<const f32x4*>(wu + dd * BL_COLS + 4 * r);
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(wv + dd * BL_COLS + 4 * r);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
              accP[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(b1[s][j], u4[cb], accP[cb], 0, 0, 0);
              accQ[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(b2[s][j], w4[cb], accQ[cb], 0, 0, 0);
            }
          }
        }
        if (ch + 1 < nchunk) stash((ch + 1) & 1);
        __syncthreads();
      }
      // accumulator cb, register i of this lane: row 16 wave + 4 kg + i of the pass, column c + 4 r + cb
      float* pr = ws;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int lr = wave * 16 + kg * 4 + i;
        const int row = m0 + lr;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          const int col = c + 4 * r + cb;
          pr[lr * (BL_COLS + 1) + 4 * r + cb] = accP[cb][i] * accQ[cb][i];
          if (SAVE && row < B && col >= start && col < c_end) {
            P[(size_t)row * ko + col] = accP[cb][i];
            Q[(size_t)row * ko + col] = accQ[cb][i];
          }
        }
      }
      __syncthreads();
      // the sum over k, columns in ascending order; a (row, output) pair stays with one thread over the passes
      for (int idx = tid; idx < BL_ROWS * nj; idx += 256) {
        const int lr = idx / nj, jj = idx - lr * nj;
        const int lo = (j0 + jj) * k, hi = lo + k;
        const int a = lo > c ? lo : c, b = hi < c + BL_COLS ? hi : c + BL_COLS;
        float s = c == c_lo ? 0.f : zs[idx];
        for (int col = a; col < b; ++col) s += pr[lr * (BL_COLS + 1) + (col - c)];
        zs[idx] = s;
      }
      __syncthreads();
    }
    for (int idx = tid; idx < BL_ROWS * nj; idx += 256) {
      const int lr = idx / nj, jj = idx - lr * nj;
      if (m0 + lr < B) z[(size_t)(m0 + lr) * o + j0 + jj] = zs[idx] / (float)k;
    }
  }
}

// One workgroup per 64-column stripe c .. c + 63 of dU [d1, k o] and dV [d2, k o].  The stripe's dP | dQ rows sit in LDS (up to 96
// batch rows at a time; a larger batch adds the later row groups to what the earlier ones stored -- the same thread, a fixed order).
// MFMA: A[row = d][k = b] = e[b][d], B[k = b][col] = dP[b][col].
__global__ __launch_bounds__(256) void bilinear_bwd_w_kernel(const float* __restrict__ e1, const float* __restrict__ e2,
                                                             const float* __restrict__ P, const float* __restrict__ Q,
                                                             const float* __restrict__ dz, float* __restrict__ dU, float* __restrict__ dV,
                                                             int B, int d1, int d2, int o, int k, int vec) {
  __shared__ __attribute__((aligned(16))) float gs[2 * BL_BWD_ROWS * BL_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kg = lane >> 4;
  const int ko = k * o;
  const int c = blockIdx.x * BL_COLS;
  const float fk = (float)k;
  for (int b0 = 0; b0 < B; b0 += BL_BWD_ROWS) {
    const int nb = (B - b0) < BL_BWD_ROWS ? (B - b0) : BL_BWD_ROWS;
    const int nb16 = (nb + 15) / 16 * 16;
    if (b0 > 0) __syncthreads();
    for (int idx = tid; idx < nb16 * BL_COLS; idx += 256) {
      const int rb = idx >> 6, cc = idx & 63;
      const int n = c + cc, b = b0 + rb;
      float gp = 0.f, gq = 0.f;
      if (rb < nb && n < ko) {
        const float g = dz[(size_t)b * o + n / k] / fk;
        gp = g * Q[(size_t)b * ko + n];
        gq = g * P[(size_t)b * ko + n];
      }
      gs[idx] = gp;
      gs[BL_BWD_ROWS * BL_COLS + idx] = gq;
    }
    __syncthreads();
#pragma unroll 1
    for (int mat = 0; mat < 2; ++mat) {
      const float* e = mat ? e2 : e1;
      const int dm = mat ? d2 : d1;
      float* dW = mat ? dV : dU;
      const float* g = gs + mat * (BL_BWD_ROWS * BL_COLS);
      for (int d0 = 16 * wave; d0 < dm; d0 += 64) {
        f32x4 acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bool d_ok = d0 + r < dm;
        for (int bc = 0; bc < nb16; bc += 16) {
          float a[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int b = b0 + bc + 4 * kg + j;
            a[j] = (d_ok && b < B) ? e[(size_t)b * dm + d0 + r] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(g + (bc + 4 * kg + j) * BL_COLS + 4 * r);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], g4[cb], acc[cb], 0, 0, 0);
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int d = d0 + 4 * kg + i;
          if (d >= dm) continue;
          float* out = dW + (size_t)d * ko + c + 4 * r;
          f32x4 v = {acc[0][i], acc[1][i], acc[2][i], acc[3][i]};
          if (vec) {
            if (c + 4 * r < ko) {
              if (b0 > 0) v += *reinterpret_cast<const f32x4*>(out);
              *reinterpret_cast<f32x4*>(out) = v;
            }
          } else {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
              if (c + 4 * r + cb < ko) out[cb] = b0 > 0 ? out[cb] + v[cb] : v[cb];
          }
        }
      }
    }
  }
}

// de [B, dm] = dX W^T, dX[b,n] = dz[b, n / k] / k * X[b,n] formed on load (X = Q with W = U, X = P with W = V: blockIdx.z).  One
// workgroup per 16 x 16 tile; wave w takes the 16-wide pieces w, w + 4, ... of the k o reduction, the four partial tiles are added in
// wave order.  MFMA: A[row = b][k = n], B[k = n][col = d] = W[d][n].
__global__ __launch_bounds__(256) void bilinear_bwd_x_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                             const float* __restrict__ dz, const float* __restrict__ U,
                                                             const float* __restrict__ V, float* __restrict__ de1, float* __restrict__ de2,
                                                             int B, int d1, int d2, int o, int k, int vec) {
  __shared__ float red[4 * 4 * 64];
  const int mat = blockIdx.z;
  const float* X = mat ? P : Q;
  const float* W = mat ? V : U;
  float* de = mat ? de2 : de1;
  const int dm = mat ? d2 : d1;
  const int d0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
  if (de == nullptr || d0 >= dm) return;      // (uniform over the workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kg = lane >> 4;
  const int ko = k * o;
  const bool v4 = vec != 0;
  const float fk = (float)k;
  const int b = m0 + r, d = d0 + r;
  const bool b_ok = b < B, d_ok = d < dm;
  const float* px = X + (size_t)(b_ok ? b : 0) * ko;
  const float* pz = dz + (size_t)(b_ok ? b : 0) * o;
  const float* pw = W + (size_t)(d_ok ? d : 0) * ko;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int n0 = 16 * wave; n0 < ko; n0 += 64) {
    const int n = n0 + 4 * kg;
    f32x4 xv = {0.f, 0.f, 0.f, 0.f}, wv = {0.f, 0.f, 0.f, 0.f};
    if (b_ok) {
      xv = bl_load4(px, n, ko, v4);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (n + j < ko) xv[j] *= pz[(n + j) / k] / fk;
    }
    if (d_ok) wv = bl_load4(pw, n, ko, v4);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[0], wv[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[1], wv[1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[2], wv[2], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[3], wv[3], acc1, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[(wave * 4 + i) * 64 + lane] = acc0[i] + acc1[i];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s = ((red[i * 64 + lane] + red[(4 + i) * 64 + lane]) + red[(8 + i) * 64 + lane]) + red[(12 + i) * 64 + lane];
      const int row = m0 + 4 * kg + i, col = d0 + r;
      if (row < B && col < dm) de[(size_t)row * dm + col] = s;
    }
  }
}

// out[b,j] = z[b,j] / max(|z_b|, eps) * scale[j] + shift[j]: F.normalize(p = 2) and the eval-mode BatchNorm1d folded to scale / shift.
__global__ __launch_bounds__(256) void bilinear_finish_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, float* __restrict__ out, int o, float eps) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  const float* pz = z + (size_t)b * o;
  double s = 0.0;
  for (int j = threadIdx.x; j < o; j += 256) s += (double)pz[j] * (double)pz[j];
  const float norm = fmaxf((float)sqrt(dlip_block_sum4(s, red)), eps);
  for (int j = threadIdx.x; j < o; j += 256) out[(size_t)b * o + j] = pz[j] / norm * scale[j] + shift[j];
}

bool bilinear_shape_ok(int B, int d1, int d2, int o, int k) {
  if (!(B >= 1 && d1 >= 4 && d2 >= 4 && d1 % 4 == 0 && d2 % 4 == 0 && o >= 1 && k >= 1)) return false;
  const long long ko = (long long)k * o;
  const long long dmax = d1 > d2 ? d1 : d2;
  return ko < (1ll << 30) && ko * dmax < (1ll << 31) && ko * B < (1ll << 31) && dmax * B < (1ll << 31);
}

}  // namespace

extern "C" int dlip_bilinear_pool_f32(const float* e1, const float* e2, const float* u, const float* v, float* z, float* p, float* q,
                                      int32_t B, int32_t d1, int32_t d2, int32_t o, int32_t k, dlip_stream_t stream) {
  DLIP_CHECK_ARG(e1 && e2 && u && v && z && bilinear_shape_ok(B, d1, d2, o, k));
  DLIP_CHECK_ARG((p == nullptr) == (q == nullptr));
  DLIP_CHECK_ARG(dlip_aligned16(e1, e2, u, v));
  const int vec = ((long long)k * o) % 4 == 0;
  // outputs per workgroup: their columns (plus the three an aligned start may add in front) fit one 64-column pass when k allows
  const int opt = k <= 61 ? 61 / k : 1;
  hipStream_t st = dlip_hip_stream(stream);
  const dim3 grid((o + opt - 1) / opt);
  if (p)
    hipLaunchKernelGGL(bilinear_fwd_kernel<true>, grid, dim3(256), 0, st, e1, e2, u, v, z, p, q, B, d1, d2, o, k, opt, vec);
  else
    hipLaunchKernelGGL(bilinear_fwd_kernel<false>, grid, dim3(256), 0, st, e1, e2, u, v, z, p, q, B, d1, d2, o, k, opt, vec);
  return dlip_launch_status();
}

extern "C" int dlip_bilinear_pool_bwd_w_f32(const float* e1, const float* e2, const float* p, const float* q, const float* dz, float* du,
                                            float* dv, int32_t B, int32_t d1, int32_t d2, int32_t o, int32_t k, dlip_stream_t stream) {
  DLIP_CHECK_ARG(e1 && e2 && p && q && dz && du && dv && bilinear_shape_ok(B, d1, d2, o, k));
  DLIP_CHECK_ARG(dlip_aligned16(du, dv));
  const int ko = k * o;
  hipStream_t st = dlip_hip_stream(stream);
  hipLaunchKernelGGL(bilinear_bwd_w_kernel, dim3((ko + BL_COLS - 1) / BL_COLS), dim3(256), 0, st, e1, e2, p, q, dz, du, dv, B, d1, d2, o, k,
                     (int)(ko % 4 == 0));
  return dlip_launch_status();
}

extern "C" int dlip_bilinear_pool_bwd_x_f32(const float* p, const float* q, const float* dz, const float* u, const float* v, float* de1,
                                            float* de2, int32_t B, int32_t d1, int32_t d2, int32_t o, int32_t k, dlip_stream_t stream) {
  DLIP_CHECK_ARG(p && q && dz && u && v && (de1 || de2) && bilinear_shape_ok(B, d1, d2, o, k));
  DLIP_CHECK_ARG(dlip_aligned16(p, q, u, v));
  const int ko = k * o;
  const int dmax = d1 > d2 ? d1 : d2;
  hipStream_t st = dlip_hip_stream(stream);
  hipLaunchKernelGGL(bilinear_bwd_x_kernel, dim3((dmax + 15) / 16, (B + 15) / 16, 2), dim3(256), 0, st, p, q, dz, u, v, de1, de2, B, d1, d2, o,
                     k, (int)(ko % 4 == 0));
  return dlip_launch_status();
}

extern "C" int dlip_bilinear_finish_f32(const float* z, const float* scale, const float* shift, float* out, int32_t B, int32_t o, float eps,
                                        dlip_stream_t stream) {
  DLIP_CHECK_ARG(z && scale && shift && out && B >= 1 && o >= 1 && eps > 0.f);
  hipLaunchKernelGGL(bilinear_finish_kernel, dim3(B), dim3(256), 0, dlip_hip_stream(stream), z, scale, shift, out, o, eps);
  return dlip_launch_status();
}

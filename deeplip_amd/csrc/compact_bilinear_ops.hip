// Compact bilinear pooling (ABI 55): deeplip_amd.fusion.CompactBilinearPooling, the third fusion head the reference's trainer names
// (`CompactBilinearPooling(embedding_dim, embedding_dim, 512)`, train_fusion.py:31-32,83) and whose source upstream no longer ships.
//
//   psi1 = x1 . sketch1 [D]   psi2 = x2 . sketch2 [D]        count sketches: row i of a sketch is s[i] = +-1 at column h[i]
//   cbp[k] = D sum_m psi1[m] psi2[(k - m) mod D]             (= irfft(rfft(psi1) rfft(psi2)) D), summed over positions when pooling
//
// Exact fp32 on the vector ALUs under every arithmetic mode: no FFT, no float atomics, every sum in a fixed order (bins gather their
// inputs in ascending channel order, the convolution runs m = 0 .. D-1, positions p = 0 .. P-1), so a replayed launch repeats the
// bits.  Nothing is shared between samples and a sample is a few KB: there is no operand reuse for the MFMA to exploit.
//
//   forward : one workgroup per sample.  Per position it gathers psi1 and psi2 into LDS over the bin-sorted (CSR) lists the host
//             packed -- a bin sums its own inputs, nothing is scattered -- keeping psi2 twice in a row (2 D floats) so that
//             psi2[(k - m) mod D] is wd[k + D - m] for any D, then convolves out of LDS.  With D % 4 == 0 a thread owns four
//             consecutive k and walks m in fours: one broadcast 16-byte read of psi1 and one 16-byte read of the doubled row feed 16
//             FMAs (the seven row values a 4 x 4 block needs are two aligned quads, one kept from the step before).  Any other D takes
//             one k per thread.  The k range is NOT split over workgroups: at B = 60 a sample is two waves of 2048 dependent FMAs
//             per lane, no SIMD is shared, and more workgroups would shorten nothing.
//   backward: one workgroup per (sample, position, input): dpsi1[m] = D sum_k g[k] psi2[(k - m) mod D] (the correlation, same
//             4 x 4 walk), then dx1[i] = s1[i] dpsi1[h1[i]] gathered out of LDS and written in NCHW; the same for dx2 with psi1.
//             Either output may be absent.
//   A workgroup has one thread per element of its longest row (64 .. 1024), so that a row's dependent loads go out in one turn.
//
// The index lists come from deeplip_amd.ops.compact_bilinear_pack, which reads them out of the dense sketch and refuses a sketch
// that is not one +-1 per row; the kernels rely on idx < C, h < D and a monotone rowptr ending at C.
#include "dlip_launch.h"

namespace {

constexpr int CB_MAX_THREADS = 1024;
constexpr int CB_MAX_D = 4096;

__device__ __forceinline__ int cb_pad4(int D) { return (D + 3) & ~3; }

// psi1[k], psi2[k]: each the sum over its bin's inputs (ascending channel) of sgn * x[channel], x read with stride P (NCHW, one
// position).  Both bins are walked together, four inputs a turn, with every load unconditional (a slot past the bin's end reads the
// list's last entry and is dropped by a select): the index loads of a turn are independent of each other and so are its input
// loads, so a bin of n inputs costs 1 + 2 ceil(n / 4) dependent memory round trips, not 1 + 2 n.
__device__ __forceinline__ void cb_bins(const float* __restrict__ x1, const int* __restrict__ rp1, const int* __restrict__ ix1,
                                        const float* __restrict__ sg1, int C1, const float* __restrict__ x2, const int* __restrict__ rp2,
                                        const int* __restrict__ ix2, const float* __restrict__ sg2, int C2, int k, int P, float& s1,
                                        float& s2) {
  int t1 = rp1[k], t2 = rp2[k];
  const int e1 = rp1[k + 1], e2 = rp2[k + 1];
  s1 = 0.f;
  s2 = 0.f;
  while (t1 < e1 || t2 < e2) {
    int i1[4], i2[4];
    float g1[4], g2[4], v1[4], v2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c1 = t1 + j < C1 ? t1 + j : C1 - 1, c2 = t2 + j < C2 ? t2 + j : C2 - 1;
      i1[j] = ix1[c1];
      g1[j] = sg1[c1];
      i2[j] = ix2[c2];
      g2[j] = sg2[c2];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v1[j] = x1[(size_t)i1[j] * P];
      v2[j] = x2[(size_t)i2[j] * P];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s1 += t1 + j < e1 ? g1[j] * v1[j] : 0.f;
      s2 += t2 + j < e2 ? g2[j] * v2[j] : 0.f;
    }
    t1 += 4;
    t2 += 4;
  }
}

// acc[j] += sum_t a4[t] * w[4 + SIGN (j - t)] with w = lo | hi, the eight row values around the block's base index
template <int SIGN>
__device__ __forceinline__ void cb_block(f32x4& acc, const f32x4 a4, const f32x4 lo, const f32x4 hi) {
  const float w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaf(a4[t], w[4 + SIGN * (j - t)], acc[j]);
}

// out[k0 + j] = sum_m a[m] wd[k0 + j + D - m], j < 4; D % 4 == 0, k0 % 4 == 0, a and wd 16-byte aligned.  The operands of the next
// step are read before this step's FMAs (one wave per SIMD: nobody else hides the LDS latency); the last step reads its own again.
__device__ __forceinline__ f32x4 cb_conv4(const float* a, const float* wd, int k0, int D) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* w = wd + k0 + D;      // step m reads w[-m - 4 .. -m + 3]
  f32x4 hi = *reinterpret_cast<const f32x4*>(w);
  f32x4 lo = *reinterpret_cast<const f32x4*>(w - 4);
  f32x4 a4 = *reinterpret_cast<const f32x4*>(a);
#pragma unroll 4
  for (int m = 0; m < D; m += 4) {
    const int mn = m + 4 < D ? m + 4 : m;
    const f32x4 a_n = *reinterpret_cast<const f32x4*>(a + mn);
    const f32x4 lo_n = *reinterpret_cast<const f32x4*>(w - mn - 4);
    cb_block<1>(acc, a4, lo, hi);
    hi = lo;
    lo = lo_n;
    a4 = a_n;
  }
  return acc;
}

// out[m0 + j] = sum_k a[k] wd[k + D - m0 - j], j < 4 (the correlation of the backward pass); same alignment, same read-ahead
__device__ __forceinline__ f32x4 cb_corr4(const float* a, const float* wd, int m0, int D) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* w = wd + D - m0;      // step k reads w[k - 4 .. k + 3]
  f32x4 lo = *reinterpret_cast<const f32x4*>(w - 4);
  f32x4 hi = *reinterpret_cast<const f32x4*>(w);
  f32x4 a4 = *reinterpret_cast<const f32x4*>(a);
#pragma unroll 4
  for (int k = 0; k < D; k += 4) {
    const int kn = k + 4 < D ? k + 4 : k;
    const f32x4 a_n = *reinterpret_cast<const f32x4*>(a + kn);
    const f32x4 hi_n = *reinterpret_cast<const f32x4*>(w + kn);
    cb_block<-1>(acc, a4, lo, hi);
    lo = hi;
    hi = hi_n;
    a4 = a_n;
  }
  return acc;
}

template <bool VEC, bool SAVE>
__global__ __launch_bounds__(CB_MAX_THREADS) void cbp_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                             const int* __restrict__ rp1, const int* __restrict__ ix1,
                                                             const float* __restrict__ sg1, const int* __restrict__ rp2,
                                                             const int* __restrict__ ix2, const float* __restrict__ sg2,
                                                             float* __restrict__ out, float* __restrict__ psi1, float* __restrict__ psi2,
                                                             int C1, int C2, int P, int D, int pool) {
  extern __shared__ __attribute__((aligned(16))) float cb_lds[];
  float* a = cb_lds;                 // psi1 [D]
  float* wd = cb_lds + cb_pad4(D);   // psi2 | psi2 [2 D]
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const float fD = (float)D;
  float* orow = out + (size_t)b * (pool ? 1 : P) * D;
  for (int p = 0; p < P; ++p) {
    if (p > 0) __syncthreads();
    const float* px1 = x1 + (size_t)b * C1 * P + p;
    const float* px2 = x2 + (size_t)b * C2 * P + p;
    for (int k = tid; k < D; k += nt) {
      float s1, s2;
      cb_bins(px1, rp1, ix1, sg1, C1, px2, rp2, ix2, sg2, C2, k, P, s1, s2);
      a[k] = s1;
      wd[k] = s2;
      wd[k + D] = s2;
      if (SAVE) {
        psi1[((size_t)b * P + p) * D + k] = s1;
        psi2[((size_t)b * P + p) * D + k] = s2;
      }
    }
    __syncthreads();
    float* o = pool ? orow : orow + (size_t)p * D;
    const bool add = pool && p > 0;      // positions of a sample in ascending order, each k by the thread that owns it
    if (VEC) {
      for (int k0 = 4 * tid; k0 < D; k0 += 4 * nt) {
        f32x4 v = cb_conv4(a, wd, k0, D) * fD;
        if (add) v += *reinterpret_cast<const f32x4*>(o + k0);
        *reinterpret_cast<f32x4*>(o + k0) = v;
      }
    } else {
      for (int k = tid; k < D; k += nt) {
        float acc = 0.f;
        for (int m = 0; m < D; ++m) acc = fmaf(a[m], wd[k + D - m], acc);
        acc *= fD;
        o[k] = add ? o[k] + acc : acc;
      }
    }
  }
}

// One workgroup per (sample, position, side): side 0 turns g and psi2 into dx1, side 1 g and psi1 into dx2 (blockIdx.y; a launch
// for one output alone has one side).  res[m] = D sum_k g[k] wd[k + D - m], then dx[i] = s[i] res[h[i]].
template <bool VEC>
__global__ __launch_bounds__(CB_MAX_THREADS) void cbp_bwd_kernel(const float* __restrict__ g, const float* __restrict__ psi1,
                                                                 const float* __restrict__ psi2, const int* __restrict__ h1,
                                                                 const float* __restrict__ s1, const int* __restrict__ h2,
                                                                 const float* __restrict__ s2, float* __restrict__ dx1,
                                                                 float* __restrict__ dx2, int C1, int C2, int P, int D, int pool) {
  extern __shared__ __attribute__((aligned(16))) float cb_lds[];
  const int Dp = cb_pad4(D);
  float* a = cb_lds;            // g [D]
  float* wd = cb_lds + Dp;      // the other input's sketch, twice [2 D]
  float* res = wd + 2 * Dp;     // dpsi [D]
  const int side = (dx1 && dx2) ? (int)blockIdx.y : (dx1 ? 0 : 1);      // (uniform: kernel arguments and the block index)
  const float* psi = side ? psi1 : psi2;
  const int* h = side ? h2 : h1;
  const float* s = side ? s2 : s1;
  float* dx = side ? dx2 : dx1;
  const int C = side ? C2 : C1;
  const int bp = blockIdx.x, b = bp / P, p = bp - b * P;
  const int tid = threadIdx.x, nt = blockDim.x;
  const float fD = (float)D;
  const float* grow = g + (size_t)(pool ? b : bp) * D;   // with sum pooling one g serves every position
  const float* prow = psi + (size_t)bp * D;
  for (int k = tid; k < D; k += nt) {
    const float v = prow[k];
    a[k] = grow[k];
    wd[k] = v;
    wd[k + D] = v;
  }
  __syncthreads();
  if (VEC) {
    for (int m0 = 4 * tid; m0 < D; m0 += 4 * nt) *reinterpret_cast<f32x4*>(res + m0) = cb_corr4(a, wd, m0, D) * fD;
  } else {
    for (int m = tid; m < D; m += nt) {
      float acc = 0.f;
      for (int k = 0; k < D; ++k) acc = fmaf(a[k], wd[k + D - m], acc);
      res[m] = acc * fD;
    }
  }
  __syncthreads();
  float* o = dx + (size_t)b * C * P + p;
  for (int i = tid; i < C; i += nt) o[(size_t)i * P] = s[i] * res[h[i]];
}

// threads of a workgroup: one per element of the longest row it loads or gathers, in whole waves
inline int cb_threads(int n) {
  const int t = (n + 63) / 64 * 64;
  return t < 64 ? 64 : (t > CB_MAX_THREADS ? CB_MAX_THREADS : t);
}

bool cbp_shape_ok(int B, int C1, int C2, int P, int D) {
  if (!(B >= 1 && C1 >= 1 && C2 >= 1 && P >= 1 && D >= 1 && D <= CB_MAX_D)) return false;
  const long long cmax = C1 > C2 ? C1 : C2;
  const long long rows = (long long)B * P;
  return rows < (1ll << 31) && rows * D < (1ll << 31) && rows * cmax < (1ll << 31);
}


}  // namespace

extern "C" int dlip_compact_bilinear_f32(const float* x1, const float* x2, const int32_t* rowptr1, const int32_t* idx1, const float* sgn1,
                                         const int32_t* rowptr2, const int32_t* idx2, const float* sgn2, float* out, float* psi1,
                                         float* psi2, int32_t B, int32_t C1, int32_t C2, int32_t P, int32_t D, int32_t sum_pool,
                                         dlip_stream_t stream) {
  DLIP_CHECK_ARG(x1 && x2 && rowptr1 && idx1 && sgn1 && rowptr2 && idx2 && sgn2 && out && cbp_shape_ok(B, C1, C2, P, D));
  DLIP_CHECK_ARG((psi1 == nullptr) == (psi2 == nullptr));
  const bool vec = D % 4 == 0 && dlip_aligned16(out);
  const size_t lds = 3 * (size_t)((D + 3) & ~3) * sizeof(float);      // at most 48 KB
  hipStream_t st = dlip_hip_stream(stream);
  const dim3 grid(B), block(cb_threads(D));
  const int pool = sum_pool != 0;
#define CB_FWD(V, S) \
  hipLaunchKernelGGL((cbp_fwd_kernel<V, S>), grid, block, lds, st, x1, x2, rowptr1, idx1, sgn1, rowptr2, idx2, sgn2, out, psi1, psi2, C1, C2, P, D, pool)
  if (vec) {
    if (psi1) CB_FWD(true, true); else CB_FWD(true, false);
  } else {
    if (psi1) CB_FWD(false, true); else CB_FWD(false, false);
  }
#undef CB_FWD
  return dlip_launch_status();
}

extern "C" int dlip_compact_bilinear_bwd_f32(const float* g, const float* psi1, const float* psi2, const int32_t* h1, const float* s1,
                                             const int32_t* h2, const float* s2, float* dx1, float* dx2, int32_t B, int32_t C1, int32_t C2,
                                             int32_t P, int32_t D, int32_t sum_pool, dlip_stream_t stream) {
  DLIP_CHECK_ARG(g && psi1 && psi2 && h1 && s1 && h2 && s2 && cbp_shape_ok(B, C1, C2, P, D));
  if (!dx1 && !dx2) return DLIP_OK;      // nobody asked for a gradient: nothing launches
  const size_t lds = 4 * (size_t)((D + 3) & ~3) * sizeof(float);      // at most 64 KB
  hipStream_t st = dlip_hip_stream(stream);
  const int cmax = C1 > C2 ? C1 : C2;
  const dim3 grid(B * P, (dx1 && dx2) ? 2 : 1), block(cb_threads(D > cmax ? D : cmax));
  const int pool = sum_pool != 0;
  if (D % 4 == 0)
    hipLaunchKernelGGL(cbp_bwd_kernel<true>, grid, block, lds, st, g, psi1, psi2, h1, s1, h2, s2, dx1, dx2, C1, C2, P, D, pool);
  else
    hipLaunchKernelGGL(cbp_bwd_kernel<false>, grid, block, lds, st, g, psi1, psi2, h1, s1, h2, s2, dx1, dx2, C1, C2, P, D, pool);
  return dlip_launch_status();
}

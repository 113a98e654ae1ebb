// ShuffleNetV2 lip-clip trunk (Lipreading(backbone_type='shufflenet'), models/video_models/model.py:72-78 and
// shufflenetv2.py), eval mode, exact fp32 on v_mfma_f32_16x16x4_f32.
//
//   dlip_shuffle_stem24_f32   Conv3d(1 -> 24, 5x7x7) + folded BN + PReLU/ReLU (the 24-channel frontend3D.0-.2)
//   dlip_shuffle_dwpw_f32     [depthwise 3x3 + folded BN on load ->] 1x1 conv + folded BN + ReLU, output scattered to the
//                             unit's channel-shuffled positions, a stride-1 unit's passthrough half copied by the same epilogue
//   dlip_avgpool3_nhwc_f32    AvgPool2d(3): the top-left 3x3 window of a 3..5 pixel map
//
// Channel layout of a unit's output (deeplip_amd/shufflenet.py): logical channel L of a 2*h-channel output lives at physical
// channel L (L < h) or hp + L - h (L >= h), hp = h rounded up to 4; the pitch is 2*hp and the padding channels hold zeros.
// channel_shuffle (shufflenetv2.py:27-40) sends branch channel j to logical 2j (first branch) or 2j + 1 (second branch).
#include "dlip_launch.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// Stem.  One workgroup = 4 output rows of one frame; the 5 x 13 x (W+6) input window (zero halo) is staged in LDS once.
// 24 channels = two 16-wide MFMA column tiles (the second 8/16 used); wave w takes column tile (w & 1) and half (w >> 1)
// of the row's 16-pixel tiles, with its 248 x 16 filter slice in 62 VGPRs.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int SK = 24, SKP = 32;
constexpr int KT = 5, KH = 7, KW = 7, KTAPS = KT * KH * KW;  // 245
constexpr int KPAD = 248, KSTEPS = KPAD / 4;                  // 62
constexpr int ROWS = 4;
constexpr int PR = 2 * ROWS + 5;                              // 13 input rows

struct Stem24Args {
  const float* x;
  const float* w;  // [248][32]: 245 taps + 3 zero rows, channels 24..31 zero
  const float* bias;
  const float* slope;
  float* y;        // [(B*T), Ho, Wo, 24]
  int T, H, W, Ho, Wo;
  int row_tiles;
  int pwp;         // LDS row pitch (W + 6)
};

template <int MT>
__global__ __launch_bounds__(256) void shuffle_stem24_f32_kernel(const Stem24Args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int plane = PR * a.pwp;
  float* patch = smem;                                          // [5][13][pwp]

  const int rt = blockIdx.x % a.row_tiles;
  const int f = blockIdx.x / a.row_tiles;                       // frame b*T + t
  const int t = f % a.T;
  const int ho0 = rt * ROWS;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int n = (wave & 1) * 16 + li;                           // output channel (< 32)
  const int tile0 = (wave >> 1) * MT;                           // this wave's first 16-pixel tile

  {
    const int hi0 = 2 * ho0 - 3;
    const float* xf = a.x + (size_t)(f - t) * a.H * a.W;        // clip base
    const int w_id = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
    for (int row = w_id; row < KT * PR; row += 4) {
      const int ft = row / PR, pr = row - ft * PR;
      const int tt = t + ft - 2, hi = hi0 + pr;
      const bool rok = (unsigned)tt < (unsigned)a.T && (unsigned)hi < (unsigned)a.H;
      const float* src = xf + ((size_t)(rok ? tt : 0) * a.H + (rok ? hi : 0)) * a.W;
      float* dst = patch + row * a.pwp;
      for (int pc = ln; pc < a.pwp; pc += 64) {
        const int wi = pc - 3;
        dst[pc] = (rok && (unsigned)wi < (unsigned)a.W) ? src[wi] : 0.f;
      }
    }
  }

  float breg[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) breg[ks] = a.w[(4 * ks + kq) * SKP + n];

  int pixoff[MT];
  const int npix = ROWS * a.Wo;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    int p = (tile0 + mt) * 16 + li;
    if (p >= npix) p = 0;
    const int orow = p / a.Wo, ocol = p - orow * a.Wo;
    pixoff[mt] = 2 * orow * a.pwp + 2 * ocol;
  }

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  __syncthreads();

  int kw = kq, kh = 0;
  int ko = kw;                                                  // ktp*plane + kh*pwp + kw
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    const int kk = (4 * ks + kq) < KTAPS ? ko : 0;              // padded taps read offset 0 (their weights are 0)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const float av = patch[kk + pixoff[mt]];
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, breg[ks], acc[mt], 0, 0, 0);
    }
    kw += 4; ko += 4;
    if (kw >= KW) {
      kw -= KW; ko += a.pwp - KW;
      if (++kh == KH) { kh = 0; ko += plane - KH * a.pwp; }
    }
  }

  if (n >= SK) return;
  const float bias = a.bias ? a.bias[n] : 0.f;
  const float slope = a.slope ? a.slope[n] : 1.f;
  float* yf = a.y + (size_t)f * a.Ho * a.Wo * SK;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int p = (tile0 + mt) * 16 + kq * 4 + e;
      const int orow = p / a.Wo, ocol = p - orow * a.Wo;
      if (p < npix && ho0 + orow < a.Ho) {
        float v = acc[mt][e] + bias;
        if (a.slope) v = v >= 0.f ? v : v * slope;
        yf[((size_t)(ho0 + orow) * a.Wo + ocol) * SK + n] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// 1x1 GEMM, optionally with a depthwise 3x3 (pad 1, stride 1 or 2, folded BN, no activation) computed on load.
// Workgroup = 64 output pixels x 16*NT output channels; wave w owns pixels 16w..16w+15 and all NT column tiles, so every
// A element is produced by exactly the lane that feeds it to the MFMA: lane (li, kq) owns pixel li and, in each 32-channel
// reduction slice, the 8 contiguous channels 8kq..8kq+7 (k-step ks of v_mfma_f32_16x16x4_f32 sums channels 8kq + ks over
// the four lane quarters: the reduction order is permuted, the B operand follows the same permutation).  The depthwise
// result is formed in registers from two float4 loads per tap and never stored.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int BM = 64, KC = 32;

struct PwArgs {
  const float* x;     // A source: pixel rows at pitch ldx, Cin channels from the pointer on
  const float* dww;   // [9][Cin] folded depthwise weights (tap-major), NULL: plain 1x1
  const float* dwb;   // [Cin] folded depthwise bias
  const float* w;     // [Cp][Kp] k-major pointwise weights, Cp = Cin rounded up to 32, zero rows beyond Cin
  const float* bias;  // [K]
  const float* xp;    // passthrough source (stride-1 unit: x1 at pitch ldp) or NULL
  float* y;
  int H, W, Ho, Wo, stride;
  int Cin, K, Kp;
  int ldx, ldp, ldy;
  int hp, par;        // hp > 0: shuffled scatter (out channel j -> logical 2j + par of a 2K-channel unit output); 0: plain
  int M;              // N * Ho * Wo
};

__device__ __forceinline__ int shuffle_phys(int L, int K, int hp) { return L < K ? L : L - K + hp; }

template <int NT, bool DW>
__global__ __launch_bounds__(256) void shuffle_dwpw_f32_kernel(const PwArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.x * BM + wave * 16;
  const int n0 = blockIdx.y * (16 * NT);

  // the pixel this lane produces A for
  const int m = m0 + li;
  const bool mok = m < a.M;
  int img = 0, oy = 0, ox = 0;
  if (mok) {
    const int hw = a.Ho * a.Wo;
    img = m / hw;
    const int r = m - img * hw;
    oy = r / a.Wo;
    ox = r - oy * a.Wo;
  }

  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < a.Cin; c0 += KC) {
    const int c = c0 + 8 * kq;                   // this lane's 8 channels: c .. c+7 (Cin % 4 == 0: a float4 is all in or all out)
    const bool in0 = mok && c < a.Cin, in1 = mok && c + 4 < a.Cin;
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
    if (DW) {
      if (in0) v0 = *reinterpret_cast<const f32x4*>(a.dwb + c);
      if (in1) v1 = *reinterpret_cast<const f32x4*>(a.dwb + c + 4);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int iy = oy * a.stride - 1 + r;
        const bool rok = (unsigned)iy < (unsigned)a.H;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int ix = ox * a.stride - 1 + q;
          if (!(rok && (unsigned)ix < (unsigned)a.W)) continue;
          const float* src = a.x + ((size_t)(img * a.H + iy) * a.W + ix) * a.ldx + c;
          const float* wt = a.dww + (r * 3 + q) * a.Cin + c;
          if (in0) v0 += *reinterpret_cast<const f32x4*>(src) * *reinterpret_cast<const f32x4*>(wt);
          if (in1) v1 += *reinterpret_cast<const f32x4*>(src + 4) * *reinterpret_cast<const f32x4*>(wt + 4);
        }
      }
    } else {
      const float* src = a.x + (size_t)m * a.ldx + c;
      if (in0) v0 = *reinterpret_cast<const f32x4*>(src);
      if (in1) v1 = *reinterpret_cast<const f32x4*>(src + 4);
    }
    const float av[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    const float* wrow = a.w + (size_t)c * a.Kp + n0 + li;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float bv = wrow[(size_t)ks * a.Kp + nt * 16];
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], bv, acc[nt], 0, 0, 0);
      }
    }
  }

  // Epilogue.  C/D map of the 16x16 MFMA: column (channel) = li, row (pixel) = 4 kq + e.
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int j = n0 + nt * 16 + li;
    if (j >= a.K) continue;
    const float b = a.bias[j];
    const int pj = a.hp ? shuffle_phys(2 * j + a.par, a.K, a.hp) : j;
    const int pp = a.hp ? shuffle_phys(2 * j + 1 - a.par, a.K, a.hp) : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int mm = m0 + 4 * kq + e;
      if (mm >= a.M) continue;
      float* yrow = a.y + (size_t)mm * a.ldy;
      yrow[pj] = fmaxf(acc[nt][e] + b, 0.f);
      if (a.xp) yrow[pp] = a.xp[(size_t)mm * a.ldp + j];     // the unit's other half (x1), same pixel (stride 1)
    }
  }
  // padding channels of the unit output: zeros, written by the second branch's launch (column block 0)
  if (a.hp && a.par == 1 && blockIdx.y == 0) {
    const int npad = a.hp - a.K;
    for (int i = lane; i < 16 * 2 * npad; i += 64) {
      const int mm = m0 + i / (2 * npad), k = i % (2 * npad);
      if (mm < a.M) a.y[(size_t)mm * a.ldy + (k < npad ? a.K + k : a.hp + a.K + k - npad)] = 0.f;
    }
  }
}

template <int NT>
void launch_dwpw(const PwArgs& a, bool dw, hipStream_t st) {
  const dim3 grid((unsigned)((a.M + BM - 1) / BM), (unsigned)((a.K + 16 * NT - 1) / (16 * NT)));
  if (dw)
    hipLaunchKernelGGL((shuffle_dwpw_f32_kernel<NT, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((shuffle_dwpw_f32_kernel<NT, false>), grid, dim3(256), 0, st, a);
}

// ------------------------------------------------------------------------------------------------------------------------
// AvgPool2d(3) (stride 3, no padding) of an H x W map with 3 <= H, W <= 5: one output pixel, the top-left 3x3 window.
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void avgpool3_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W,
                                                       int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * C) return;
  const int n = (int)(i / C), c = (int)(i - (long long)n * C);
  const float* xf = x + (size_t)n * H * W * C + c;
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) s += xf[(size_t)(r * W + q) * C];
  y[i] = s / 9.f;
}

}  // namespace

extern "C" int dlip_shuffle_stem24_f32(const float* x, const float* w_248x32, const float* bias, const float* slope, float* y,
                                       int32_t B, int32_t T, int32_t H, int32_t W, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && w_248x32 && bias && y && B > 0 && T > 0 && H > 0 && W > 0);
  DLIP_CHECK_ARG((H & 1) == 0 && (W & 1) == 0);
  Stem24Args a;
  a.x = x; a.w = w_248x32; a.bias = bias; a.slope = slope; a.y = y;
  a.T = T; a.H = H; a.W = W; a.Ho = H / 2; a.Wo = W / 2;
  a.row_tiles = (a.Ho + ROWS - 1) / ROWS;
  a.pwp = W + 6;
  const long long grid = (long long)B * T * a.row_tiles;
  if (grid > 0x7FFFFFFFll || (long long)B * T * H * W * 4 > DLIP_MAX_BUFFER_BYTES ||
      (long long)B * T * a.Ho * a.Wo * SK * 4 > DLIP_MAX_BUFFER_BYTES)
    return DLIP_ERANGE;
  const size_t lds = (size_t)(KT * PR * a.pwp) * 4;
  hipStream_t st = dlip_hip_stream(stream);
  const int tiles = (ROWS * a.Wo + 15) / 16;     // split between the two pixel halves of the workgroup
  if (tiles <= 12) {
    hipLaunchKernelGGL(shuffle_stem24_f32_kernel<6>, dim3((unsigned)grid), dim3(256), lds, st, a);
  } else if (tiles <= 16) {
    hipLaunchKernelGGL(shuffle_stem24_f32_kernel<8>, dim3((unsigned)grid), dim3(256), lds, st, a);
  } else {
    return DLIP_EINVAL;  // frames wider than 128 pixels
  }
  return dlip_launch_status();
}

extern "C" int dlip_shuffle_dwpw_f32(const float* x, const float* dw_w, const float* dw_b, const float* w, const float* bias,
                                     const float* xp, float* y, int32_t N, int32_t H, int32_t W, int32_t stride, int32_t Cin,
                                     int32_t K, int32_t Kp, int32_t ldx, int32_t ldp, int32_t ldy, int32_t hp, int32_t par,
                                     dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && w && bias && y && N > 0 && H > 0 && W > 0 && Cin > 0 && K > 0);
  DLIP_CHECK_ARG((dw_w == nullptr) == (dw_b == nullptr));
  DLIP_CHECK_ARG(stride == 1 || (stride == 2 && dw_w));
  DLIP_CHECK_ARG((Cin & 3) == 0 && (ldx & 3) == 0 && ldx >= Cin);
  DLIP_CHECK_ARG(dlip_aligned16(x));
  DLIP_CHECK_ARG(dw_w == nullptr || dlip_aligned16(dw_w, dw_b));
  DLIP_CHECK_ARG(Kp >= K && (Kp & 63) == 0);
  DLIP_CHECK_ARG(hp == 0 || (hp >= K && (par == 0 || par == 1) && ldy >= 2 * hp));   // the padding reaches channel 2hp - 1
  DLIP_CHECK_ARG(hp != 0 || ldy >= K);
  DLIP_CHECK_ARG(xp == nullptr || (hp != 0 && stride == 1 && ldp >= K));
  const int Ho = stride == 1 ? H : (H - 1) / 2 + 1, Wo = stride == 1 ? W : (W - 1) / 2 + 1;
  const long long M = (long long)N * Ho * Wo;
  const long long Cp = (Cin + KC - 1) / KC * KC;
  if (M > 0x7FFFFFFFll / BM || ((long long)N * H * W - 1) * ldx + Cin > DLIP_MAX_BUFFER_BYTES / 4 ||
      (M - 1) * ldy + (hp ? 2 * hp : K) > DLIP_MAX_BUFFER_BYTES / 4 || Cp * Kp > DLIP_MAX_BUFFER_BYTES / 4)
    return DLIP_ERANGE;
  PwArgs a;
  a.x = x; a.dww = dw_w; a.dwb = dw_b; a.w = w; a.bias = bias; a.xp = xp; a.y = y;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.stride = stride;
  a.Cin = Cin; a.K = K; a.Kp = Kp;
  a.ldx = ldx; a.ldp = ldp; a.ldy = ldy;
  a.hp = hp; a.par = par;
  a.M = (int)M;
  // column tile: 64 channels unless K fits a narrower one -- every column block recomputes the depthwise stage of its pixels, so a
  // narrower tile that only trims padding (K = 232: 15 blocks of 16 instead of 4 of 64) measured 2.4x slower per launch
  const int nt = K <= 16 ? 1 : K <= 32 ? 2 : 4;
  hipStream_t st = dlip_hip_stream(stream);
  const bool dw = dw_w != nullptr;
  if (nt == 4) launch_dwpw<4>(a, dw, st);
  else if (nt == 2) launch_dwpw<2>(a, dw, st);
  else launch_dwpw<1>(a, dw, st);
  return dlip_launch_status();
}

extern "C" int dlip_avgpool3_nhwc_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && y && N > 0 && C > 0);
  DLIP_CHECK_ARG(H >= 3 && H <= 5 && W >= 3 && W <= 5);   // AvgPool2d(3) of the map gives exactly one pixel
  const long long total = (long long)N * C;
  if ((long long)N * H * W * C > DLIP_MAX_BUFFER_BYTES / 4) return DLIP_ERANGE;
  hipLaunchKernelGGL(avgpool3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, dlip_hip_stream(stream), x, y, N,
                     H, W, C);
  return dlip_launch_status();
}

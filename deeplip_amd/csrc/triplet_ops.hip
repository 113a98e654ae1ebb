// Online triplet loss with negative mining on the device (ABI 53): models/audio_models/loss.py:18-31 (OnlineTriplet) and the
// selectors of models/audio_models/utils.py:18-142, which copy the embeddings to the host and walk every anchor-positive pair in a
// Python loop.  Here: exact fp32, shapes fixed by B and E alone, nothing read back, no float atomics (the only atomics are
// integer counts in LDS), every sum in a fixed order -- a replayed step equals the eager one bit for bit.
//
//   mine  : G = X X^T (RAW dot products, utils.py:93 -- not cosines although the reference calls it cos_matrix) on
//           v_mfma_f32_16x16x4_f32, rownorm = max(sqrt(G_ii), 1e-8); then one workgroup per anchor row a picks, for every
//           positive p > a of a's label, one negative (or none) into the dense neg[a,p].
//   loss  : one workgroup per anchor row: hinge terms on COSINES G_ij / (rownorm_i rownorm_j), fp64 row sum, row count and the
//           signed integer weights wcount[a,j] = #(active triplets with negative j) - #(active triplets with positive j);
//           then a fixed-order reduction over the rows.
//   bwd   : M_ij = (wcount_ij + wcount_ji) g / (N rownorm_i rownorm_j), M_ii = -sum_j M_ij G_ij / rownorm_i^2, dX = M X (MFMA).
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

enum { TRIPLET_ALL = 0, TRIPLET_HARDEST = 1, TRIPLET_RANDOM = 2, TRIPLET_SEMIHARD = 3 };
constexpr int TRIPLET_MAX_B = 1024;

// C[M,N] = A[M,K] * op(Bm); TB: op(Bm)[k][n] = Bm[n][k] (Bm [N,K], ldb = its row stride), else Bm [K,N].  One wave per 16x16
// tile, four tiles (64 columns) per workgroup.  A lane loads the four consecutive k of its k-group (16 bytes) and MFMA j of a
// 16-wide k-chunk takes element j from every lane: the chunk's 16 products are summed in the order j-major, which is the same for A
// and B, so any consistent assignment gives the product.  Two accumulators (even / odd j) hide the 40-cycle dependent latency; their
// sum is one more fixed-order add.  A rows beyond M, B columns beyond N and B's k beyond K read as zeros; A is read in whole
// 16-byte groups up to lda (lda % 4 == 0, K <= lda, and either lda == K or lda % 16 == 0 with zeros in columns K .. lda).  diag_norm (TB, square): the lanes that hold C_ii also write max(sqrt(C_ii), 1e-8).
template <bool TB>
__global__ __launch_bounds__(256) void triplet_gemm16_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                             float* __restrict__ Cm, float* __restrict__ diag_norm, int M, int N,
                                                             int K, int lda, int ldb, int ldc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.y * 16, n0 = (blockIdx.x * 4 + wave) * 16;
  if (n0 >= N) return;      // (wave-uniform; no barrier in this kernel)
  const int r = lane & 15, kg = lane >> 4;
  const int am = m0 + r, bn = n0 + r;
  const bool a_ok = am < M, b_ok = bn < N;
  const float* pa = A + (long long)(a_ok ? am : 0) * lda;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 16) {
    const int k = k0 + 4 * kg;
    f32x4 av = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
    if (a_ok && k < lda) av = *reinterpret_cast<const f32x4*>(pa + k);    // lda % 4 == 0; columns K .. lda of A hold zeros
    if (TB) {
      if (b_ok && k < K) bv = *reinterpret_cast<const f32x4*>(Bm + (long long)bn * ldb + k);
    } else if (b_ok) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k + j < K) bv[j] = Bm[(long long)(k + j) * ldb + bn];
    }
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[2], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[3], acc1, 0, 0, 0);
  }
  const int col = n0 + (lane & 15);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = m0 + (lane >> 4) * 4 + i;
    if (row < M && col < N) {
      const float v = acc0[i] + acc1[i];
      Cm[(long long)row * ldc + col] = v;
      if (TB && diag_norm != nullptr && row == col) diag_norm[row] = fmaxf(sqrtf(v), 1e-8f);
    }
  }
}

// utils.py:106: cos_matrix[a, negatives] + margin - cos_matrix[a, p], two fp32 roundings in that order
__device__ __forceinline__ float triplet_value(float g_an, float margin, float g_ap) {
#pragma clang fp contract(off)
  return (g_an + margin) - g_ap;
}

__device__ __forceinline__ bool triplet_candidate(float v, float margin, int mode) {
  return mode == TRIPLET_SEMIHARD ? (v > 0.f && v < margin) : v > 0.f;
}

// One workgroup per anchor row a; the row of G and the labels sit in LDS.  Every wave scans the positives p > a in index order
// (ballots) and takes every fourth one.  hardest: wave-wide arg-max with the lower index winning ties (numpy's argmax), kept if
// its value is > 0.  random / semi-hard: count the candidates, pick number floor(u[a,p] * count) in index order.
// neg[a,j] = the chosen negative, -1 where (a,j) is no anchor-positive pair or the pair has no candidate: the whole row is written.
__global__ __launch_bounds__(256) void triplet_mine_kernel(const float* __restrict__ G, const int32_t* __restrict__ labels,
                                                           const float* __restrict__ u, int32_t* __restrict__ neg, int B,
                                                           float margin, int mode) {
  __shared__ float g[TRIPLET_MAX_B];
  __shared__ int32_t lab[TRIPLET_MAX_B];
  const int a = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < B; j += 256) {
    g[j] = G[(long long)a * B + j];
    lab[j] = labels[j];
  }
  __syncthreads();
  const int la = lab[a];
  for (int j = threadIdx.x; j < B; j += 256)
    if (!(j > a && lab[j] == la)) neg[(long long)a * B + j] = -1;
  int ord = 0;
  for (int c0 = (a + 1) & ~63; c0 < B; c0 += 64) {
    const int pl = c0 + lane;
    unsigned long long pm = __builtin_amdgcn_ballot_w64(pl < B && pl > a && lab[pl] == la);
    while (pm != 0ull) {
      const int p = c0 + __builtin_ctzll(pm);
      pm &= pm - 1ull;
      if ((ord++ & 3) != wave) continue;
      const float gap = g[p];
      int res = -1;
      if (mode == TRIPLET_HARDEST) {
        float best = -__builtin_inff();
        int bi = 0x7fffffff;
        for (int n = lane; n < B; n += 64) {
          if (lab[n] != la) {
            const float v = triplet_value(g[n], margin, gap);
            if (v > best) { best = v; bi = n; }
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(best, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (best > 0.f) res = bi;
      } else {
        int count = 0;
        for (int n0 = 0; n0 < B; n0 += 64) {
          const int n = n0 + lane;
          const bool c = n < B && lab[n] != la && triplet_candidate(triplet_value(g[n], margin, gap), margin, mode);
          count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(c));
        }
        if (count > 0) {
          int k = (int)(u[(long long)a * B + p] * (float)count);
          k = k < 0 ? 0 : (k > count - 1 ? count - 1 : k);
          int run = 0;
          for (int n0 = 0; n0 < B; n0 += 64) {
            const int n = n0 + lane;
            const bool c = n < B && lab[n] != la && triplet_candidate(triplet_value(g[n], margin, gap), margin, mode);
            unsigned long long m = __builtin_amdgcn_ballot_w64(c);
            const int pc = __builtin_popcountll(m);
            if (run + pc > k) {
              for (int t = k - run; t > 0; --t) m &= m - 1ull;
              res = n0 + __builtin_ctzll(m);
              break;
            }
            run += pc;
          }
        }
      }
      if (lane == 0) neg[(long long)a * B + p] = res;
    }
  }
}

// loss.py:28-31 for the triplets anchored at row a: relu(cos(a,n) - cos(a,p) + margin), cos = G_ij / (max(|x_i|, 1e-8) max(|x_j|, 1e-8))
// (F.cosine_similarity's clamp).  Every triplet counts towards N; the active ones (hinge > 0) enter the sum and the signed
// weights of row a.  mode all: thread per negative column, loop over the row's positives.
__global__ __launch_bounds__(256) void triplet_loss_rows_kernel(const float* __restrict__ G, const float* __restrict__ rownorm,
                                                                const int32_t* __restrict__ labels, const int32_t* __restrict__ neg,
                                                                double* __restrict__ rowsum, int32_t* __restrict__ rowcnt,
                                                                int32_t* __restrict__ wcount, int B, float margin, int mode) {
  __shared__ float c[TRIPLET_MAX_B];
  __shared__ int32_t lab[TRIPLET_MAX_B];
  __shared__ int32_t wcl[TRIPLET_MAX_B];
  __shared__ int32_t plist[TRIPLET_MAX_B];
  __shared__ double red[4];
  __shared__ int redi[4];
  __shared__ int np_s;
  const int a = blockIdx.x, lane = threadIdx.x & 63;
  const float na = rownorm[a];
  for (int j = threadIdx.x; j < B; j += 256) {
    c[j] = G[(long long)a * B + j] / (na * rownorm[j]);
    lab[j] = labels[j];
    wcl[j] = 0;
  }
  __syncthreads();
  const int la = lab[a];
  double sum = 0.0;
  int cnt = 0;
  if (mode == TRIPLET_ALL) {
    if (threadIdx.x < 64) {       // the row's positives, in index order
      int np = 0;
      for (int c0 = (a + 1) & ~63; c0 < B; c0 += 64) {
        const int p = c0 + lane;
        const bool pos = p < B && p > a && lab[p] == la;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(pos);
        if (pos) plist[np + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = p;
        np += __builtin_popcountll(m);
      }
      if (lane == 0) np_s = np;
    }
    __syncthreads();
    const int np = np_s;
    for (int n = threadIdx.x; n < B; n += 256) {
      if (lab[n] == la) continue;
      int act = 0;
      for (int i = 0; i < np; ++i) {
        const int p = plist[i];
        const float h = (c[n] - c[p]) + margin;
        ++cnt;
        if (h > 0.f) {
          sum += (double)h;
          ++act;
          atomicAdd(&wcl[p], -1);
        }
      }
      if (act) atomicAdd(&wcl[n], act);
    }
  } else {
    for (int p = threadIdx.x; p < B; p += 256) {
      const int n = neg[(long long)a * B + p];
      if (n < 0 || n >= B) continue;
      const float h = (c[n] - c[p]) + margin;
      ++cnt;
      if (h > 0.f) {
        sum += (double)h;
        atomicAdd(&wcl[n], 1);
        atomicAdd(&wcl[p], -1);
      }
    }
  }
  const double s = dlip_block_sum4(sum, red);      // (its barrier also closes the LDS counts)
  __syncthreads();
  const int k = dlip_block_sum4(cnt, redi);
  __syncthreads();
  if (threadIdx.x == 0) {
    rowsum[a] = s;
    rowcnt[a] = k;
  }
  for (int j = threadIdx.x; j < B; j += 256) wcount[(long long)a * B + j] = wcl[j];
}

// loss = sum_a rowsum[a] / N, N = sum_a rowcnt[a]; N == 0: loss = 0 (the reference's fallback, utils.py:114-118, fails instead).
__global__ __launch_bounds__(256) void triplet_loss_finish_kernel(const double* __restrict__ rowsum, const int32_t* __restrict__ rowcnt,
                                                                  float* __restrict__ loss, int32_t* __restrict__ n_triplets, int B) {
  __shared__ double red[4];
  __shared__ int redi[4];
  double s = 0.0;
  int k = 0;
  for (int a = threadIdx.x; a < B; a += 256) {
    s += rowsum[a];
    k += rowcnt[a];
  }
  s = dlip_block_sum4(s, red);
  __syncthreads();
  k = dlip_block_sum4(k, redi);
  __syncthreads();
  if (threadIdx.x == 0) {
    loss[0] = k > 0 ? (float)(s / (double)k) : 0.f;
    n_triplets[0] = k;
  }
}

// Row i of M (leading dimension ldm = B rounded up to 16, the padding written as zeros): the transposed half of the weights is
// READ (wcount[j,i]), nothing is scattered.  A row whose norm sits at the clamp has no correction term (the clamp's derivative is 0).
__global__ __launch_bounds__(256) void triplet_bwd_weights_kernel(const float* __restrict__ G, const float* __restrict__ rownorm,
                                                                  const int32_t* __restrict__ wcount, const int32_t* __restrict__ n_triplets,
                                                                  const float* __restrict__ gscale, float* __restrict__ Mw, int B, int ldm) {
  __shared__ double red[4];
  const int i = blockIdx.x;
  const int N = n_triplets[0];
  const float scale = N > 0 ? (gscale ? gscale[0] : 1.f) / (float)N : 0.f;
  const float ni = rownorm[i];
  double d = 0.0;
  for (int j = threadIdx.x; j < B; j += 256) {
    const int s = wcount[(long long)i * B + j] + wcount[(long long)j * B + i];
    if (s != 0) d += (double)((float)s * scale / (ni * rownorm[j])) * (double)G[(long long)i * B + j];
  }
  d = dlip_block_sum4(d, red);
  __syncthreads();
  const float dii = ni > 1e-8f ? (float)(-d / ((double)ni * (double)ni)) : 0.f;
  for (int j = threadIdx.x; j < ldm; j += 256) {
    float m = 0.f;
    if (j == i) {
      m = dii;
    } else if (j < B) {
      const int s = wcount[(long long)i * B + j] + wcount[(long long)j * B + i];
      if (s != 0) m = (float)s * scale / (ni * rownorm[j]);
    }
    Mw[(long long)i * ldm + j] = m;
  }
}

bool triplet_shape_ok(int B, int E) { return B >= 1 && B <= TRIPLET_MAX_B && E >= 4 && E % 4 == 0; }

}  // namespace

extern "C" int dlip_triplet_mine_f32(const float* x, const int32_t* labels, float margin, int32_t mode, const float* u, float* g,
                                     float* rownorm, int32_t* neg, int32_t B, int32_t E, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && labels && g && rownorm && triplet_shape_ok(B, E) && mode >= TRIPLET_ALL && mode <= TRIPLET_SEMIHARD);
  DLIP_CHECK_ARG(mode == TRIPLET_ALL || neg);
  DLIP_CHECK_ARG((mode != TRIPLET_RANDOM && mode != TRIPLET_SEMIHARD) || u);
  DLIP_CHECK_ARG(dlip_aligned16(x));
  hipStream_t st = dlip_hip_stream(stream);
  hipLaunchKernelGGL(triplet_gemm16_kernel<true>, dim3((B + 63) / 64, (B + 15) / 16), dim3(256), 0, st, x, x, g, rownorm, B, B, E, E, E, B);
  if (mode != TRIPLET_ALL)
    hipLaunchKernelGGL(triplet_mine_kernel, dim3(B), dim3(256), 0, st, g, labels, u, neg, B, margin, mode);
  return dlip_launch_status();
}

extern "C" int dlip_triplet_loss_f32(const float* g, const float* rownorm, const int32_t* labels, const int32_t* neg, float margin,
                                     int32_t mode, double* rowsum, int32_t* rowcnt, int32_t* wcount, float* loss,
                                     int32_t* n_triplets, int32_t B, dlip_stream_t stream) {
  DLIP_CHECK_ARG(g && rownorm && labels && rowsum && rowcnt && wcount && loss && n_triplets && B >= 1 && B <= TRIPLET_MAX_B);
  DLIP_CHECK_ARG(mode >= TRIPLET_ALL && mode <= TRIPLET_SEMIHARD && (mode == TRIPLET_ALL || neg));
  hipStream_t st = dlip_hip_stream(stream);
  hipLaunchKernelGGL(triplet_loss_rows_kernel, dim3(B), dim3(256), 0, st, g, rownorm, labels, neg, rowsum, rowcnt, wcount, B, margin, mode);
  hipLaunchKernelGGL(triplet_loss_finish_kernel, dim3(1), dim3(256), 0, st, rowsum, rowcnt, loss, n_triplets, B);
  return dlip_launch_status();
}

extern "C" int dlip_triplet_loss_bwd_f32(const float* x, const float* g, const float* rownorm, const int32_t* wcount,
                                         const int32_t* n_triplets, const float* gscale, float* mw, float* dx, int32_t B, int32_t E,
                                         dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && g && rownorm && wcount && n_triplets && mw && dx && triplet_shape_ok(B, E));
  DLIP_CHECK_ARG(dlip_aligned16(mw));
  const int ldm = (B + 15) / 16 * 16;
  hipStream_t st = dlip_hip_stream(stream);
  hipLaunchKernelGGL(triplet_bwd_weights_kernel, dim3(B), dim3(256), 0, st, g, rownorm, wcount, n_triplets, gscale, mw, B, ldm);
  hipLaunchKernelGGL(triplet_gemm16_kernel<false>, dim3((E + 63) / 64, (B + 15) / 16), dim3(256), 0, st, mw, x, dx, nullptr, B, E, B, ldm, E, E);
  return dlip_launch_status();
}

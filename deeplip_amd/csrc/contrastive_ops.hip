// Online contrastive loss on cosines with the pairs selected on the device (ABI 66): `Contrastive` is an empty stub upstream
// (models/audio_models/loss.py:69-75) that conf/audio_config.yaml:130 lists; the definition is the build's own: the
// cosine form of adambielski/siamese-triplet's OnlineContrastiveLoss, i.e. torch.nn.CosineEmbeddingLoss on the selected pairs --
//   a positive pair (one label) costs 1 - cos_ij, a negative pair relu(cos_ij - margin), loss = mean over ALL selected pairs,
//   cos_ij = x_i.x_j / (max(|x_i|, 1e-8) max(|x_j|, 1e-8)).
// The cosine matrix is the triplet file's Gram launch (G = X X^T on the fp32 MFMA with rownorm from its diagonal), called through
// dlip_triplet_mine_f32's mode-0 form.  One workgroup per anchor row a then selects among the columns j > a and leaves the signed
// weights w[a,j] (-1 positive pair, +1 selected negative with an active hinge, 0 otherwise) that dlip_triplet_loss_bwd_f32 takes as
// they are.  Exact fp32, nothing read back, no atomics at all, every sum in a fixed order.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

enum { PAIRS_ALL = 0, PAIRS_HARD_NEGATIVE = 1 };
constexpr int PAIRS_MAX_B = 1024;

// mode all: every pair a < j.  mode hard negative: every positive pair, and the min(P_a, #negatives after a) negatives n > a of
// highest cosine, the lower index winning ties -- an EXACT top-K by rank counting: candidate n is taken iff fewer than K candidates
// precede it in the order (cosine descending, index ascending).  Every thread owns the columns j = tid, tid + 256, ..; the inner
// loop reads one LDS word per step, the same for all lanes (a broadcast): O(n^2) compares per row, 1 M at B = 1024.
// w and (when given) sel are written for the whole row: sel = 1 positive pair, 2 selected negative, 0 otherwise.
__global__ __launch_bounds__(256) void contrastive_rows_kernel(const float* __restrict__ G, const float* __restrict__ rownorm,
                                                               const int32_t* __restrict__ labels, double* __restrict__ rowsum,
                                                               int32_t* __restrict__ rowcnt, int32_t* __restrict__ w,
                                                               int32_t* __restrict__ sel, int B, float margin, int mode) {
  __shared__ float c[PAIRS_MAX_B];
  __shared__ int32_t lab[PAIRS_MAX_B];
  __shared__ double red[4];
  __shared__ int redi[4];
  const int a = blockIdx.x;
  const float na = rownorm[a];
  for (int j = threadIdx.x; j < B; j += 256) {
    c[j] = G[(long long)a * B + j] / (na * rownorm[j]);
    lab[j] = labels[j];
  }
  __syncthreads();
  const int la = lab[a];
  int K = 0, nneg = 0;
  if (mode == PAIRS_HARD_NEGATIVE) {
    int np = 0;
    for (int j = a + 1 + threadIdx.x; j < B; j += 256) np += lab[j] == la ? 1 : 0;
    np = dlip_block_sum4(np, redi);
    __syncthreads();
    nneg = B - 1 - a - np;
    K = np < nneg ? np : nneg;
  }
  double sum = 0.0;
  int cnt = 0;
  for (int j = threadIdx.x; j < B; j += 256) {
    int wv = 0, sv = 0;
    if (j > a) {
      const float cj = c[j];
      if (lab[j] == la) {
        wv = -1;
        sv = 1;
        sum += 1.0 - (double)cj;
        ++cnt;
      } else {
        bool take = mode == PAIRS_ALL || (K > 0 && K >= nneg);
        if (!take && K > 0) {
          int rank = 0;
          for (int n = a + 1; n < B; ++n)
            rank += (lab[n] != la && (c[n] > cj || (c[n] == cj && n < j))) ? 1 : 0;
          take = rank < K;
        }
        if (take) {
          sv = 2;
          ++cnt;
          const float h = cj - margin;
          if (h > 0.f) {
            sum += (double)h;
            wv = 1;
          }
        }
      }
    }
    w[(long long)a * B + j] = wv;
    if (sel != nullptr) sel[(long long)a * B + j] = sv;
  }
  const double s = dlip_block_sum4(sum, red);
  const int k = dlip_block_sum4(cnt, redi);
  if (threadIdx.x == 0) {
    rowsum[a] = s;
    rowcnt[a] = k;
  }
}

// loss = sum_a rowsum[a] / N, N = sum_a rowcnt[a] (inactive negatives count); N == 0: loss = 0.  Rows in a fixed order.
__global__ __launch_bounds__(256) void contrastive_finish_kernel(const double* __restrict__ rowsum, const int32_t* __restrict__ rowcnt,
                                                                 float* __restrict__ loss, int32_t* __restrict__ n_pairs, int B) {
  __shared__ double red[4];
  __shared__ int redi[4];
  double s = 0.0;
  int k = 0;
  for (int a = threadIdx.x; a < B; a += 256) {
    s += rowsum[a];
    k += rowcnt[a];
  }
  s = dlip_block_sum4(s, red);
  k = dlip_block_sum4(k, redi);
  if (threadIdx.x == 0) {
    loss[0] = k > 0 ? (float)(s / (double)k) : 0.f;
    n_pairs[0] = k;
  }
}

}  // namespace

extern "C" int dlip_contrastive_loss_f32(const float* x, const int32_t* labels, float margin, int32_t mode, float* g, float* rownorm,
                                         double* rowsum, int32_t* rowcnt, int32_t* w, int32_t* sel, float* loss, int32_t* n_pairs,
                                         int32_t B, int32_t E, dlip_stream_t stream) {
  DLIP_CHECK_ARG(x && labels && g && rownorm && rowsum && rowcnt && w && loss && n_pairs);
  DLIP_CHECK_ARG(B >= 1 && B <= PAIRS_MAX_B && (mode == PAIRS_ALL || mode == PAIRS_HARD_NEGATIVE));
  // G = X X^T and rownorm = max(sqrt(G_ii), 1e-8): the Gram launch alone (mode 0 mines nothing); it checks E and the alignment of x
  const int rc = dlip_triplet_mine_f32(x, labels, 0.f, 0, nullptr, g, rownorm, nullptr, B, E, stream);
  if (rc != DLIP_OK) return rc;
  hipStream_t st = dlip_hip_stream(stream);
  hipLaunchKernelGGL(contrastive_rows_kernel, dim3((unsigned)B), dim3(256), 0, st, g, rownorm, labels, rowsum, rowcnt, w, sel, B, margin, mode);
  hipLaunchKernelGGL(contrastive_finish_kernel, dim3(1), dim3(256), 0, st, rowsum, rowcnt, loss, n_pairs, B);
  return dlip_launch_status();
}

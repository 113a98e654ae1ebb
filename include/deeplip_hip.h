/*
 * deeplip_hip.h -- C ABI of libdeeplip_hip.so: the MI355X (gfx950 / CDNA4) kernels under the
 * DeepLip audio-visual embedding hot path.
 *
 * The reference (DanielMengLiu/DeepLip) has no FFI / operator / plugin layer: its boundary is the
 * Python module API + state-dict schema and all arithmetic is delegated to
 * stock torch.nn layers.  Each entry point below therefore names the reference call site(s) whose
 * torch.nn arithmetic it replaces (paths relative to the reference repo root).  The Python host
 * (the deeplip_amd package, re-exported as the models package) binds these with ctypes; INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (kernels never allocate, free or synchronise), except the parameters marked DLIP_HOST:
 *     descriptors, out-parameters and per-branch arrays the CPU reads or writes during the call;
 *   - this header is the ONE definition of the ABI: deeplip_amd/_lib.py derives its ctypes binding and
 *     the shared constants from it (prototypes, `#define DLIP_X <integer>`, anonymous enums,
 *     dlip_conv_desc), so keep declarations in the plain style used below;
 *   - activations are channels-last (NHWC / N-T-C), fp32; weights are pre-packed by the
 *     caller to [K][R][S][C] ("KRSC", BN already folded in fp64 on the host);
 *   - every call is asynchronous on `stream` (a hipStream_t; NULL = the null stream);
 *   - return value: 0 on success, a positive hipError_t value if the launch failed, or a
 *     negative DLIP_E* code for argument errors detected on the host.  No exceptions, no
 *     global mutable state: every function is re-entrant.
 */
#ifndef DEEPLIP_HIP_H
#define DEEPLIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLIP_ABI_VERSION 67
#define DLIP_HOST              /* marks a pointer parameter that the CPU dereferences during the call (HOST memory, not device) */
#define DLIP_LIFT_BCAST 2048
#define DLIP_LIFT_WORDS 4098   /* a gradient's power-of-two lift: (2^e, 2^-e), then 2^-e repeated DLIP_LIFT_BCAST times (the post_scale
                                  vector of the convolution that consumes the lifted gradient); while it is formed the words behind the
                                  pair hold one maximum per workgroup of the producing pass: 2 + max(4096 maxima, DLIP_LIFT_BCAST) */

#define DLIP_OK 0
#define DLIP_EINVAL (-1)  /* inconsistent shapes / null pointers / unsupported alignment */
#define DLIP_ERANGE (-2)  /* a tensor exceeds the 2 GiB addressing window of one launch */

typedef void* dlip_stream_t; /* hipStream_t */
typedef void* dlip_plan_t;   /* a recorded step (dlip_plan_end) */

int dlip_abi_version(void);
/* sha256 (hex) over the sources and headers this library was built from, stamped at link time by deeplip_amd/build.py: the
 * build check compares it with the tree's own hash, so a stale prebuilt library is rebuilt and a fresh one is proven fresh. */
const char* dlip_source_sha(void);
/* Human-readable text for a code returned by any dlip_* call. */
const char* dlip_error_string(int code);

/* ------------------------------------------------------------------------------------------
 * Generic implicit-GEMM convolution, NHWC fp32, on v_mfma_f32_32x32x2_f32.
 *   y[n,ho,wo,k] = epilogue( sum_{r,s,c} x[n, ho*sh-ph+r*dh, wo*sw-pw+s*dw, c] * w[k,r,s,c] )
 *   epilogue(v)  = v + bias[k]; v += residual[m*ldr + k]; v = v>=0 ? v : v*slope[k];
 *                  v = v*post_scale[k] + post_shift[k]            (each step skipped when NULL)
 * Replaces, with BN folded into (w, bias):
 *   Conv2d 3x3 / 1x1 + BatchNorm2d + PReLU|ReLU + residual add   models/video_models/resnet.py:9-17,55-69
 *   Conv1d(dilated) + BatchNorm1d + LeakyReLU(0.2) (TDNN_Block)   models/audio_models/tdnn.py:23-43
 *   Conv1d + BatchNorm1d + Chomp1d + PReLU, 1x1 residual Conv1d   models/video_models/tcn.py:46-59,87,113-116
 *   nn.Linear (+BatchNorm1d +LeakyReLU)                           models/audio_models/tdnn.py:85-101,
 *                                                                 models/fusion_models/model_fusion.py:19-24,
 *                                                                 models/audio_models/loss.py:14,
 *                                                                 models/video_models/model.py:27
 * Conv1d is H=1; Linear is H=W=R=S=1.  C % 4 == 0 required (pad on pack); ldx/ldy/ldr are pixel
 * strides in floats (>= C / K), so a call may read or write a channel slice of a wider tensor.
 * ------------------------------------------------------------------------------------------ */
typedef struct dlip_conv_desc {
  int32_t N, H, W, C;          /* input  [N,H,W,C]                 */
  int32_t K;                   /* output channels                  */
  int32_t R, S;                /* filter taps (height, width)      */
  int32_t stride_h, stride_w;
  int32_t pad_h, pad_w;
  int32_t dil_h, dil_w;
  int32_t Ho, Wo;              /* output spatial size (validated)  */
  int32_t ldx, ldy, ldr;       /* pixel strides in floats          */
} dlip_conv_desc;

int dlip_conv_nhwc_f32(DLIP_HOST const dlip_conv_desc* d, const float* x, const float* w_krsc,
                       const float* bias, const float* residual, const float* slope,
                       const float* post_scale, const float* post_shift, float* y,
                       dlip_stream_t stream);

/* Split-precision variant of dlip_conv_nhwc_f32: same operation, fp32 in / fp32 out, but every
 * product is evaluated as hi*hi + hi*lo + lo*hi on the f16 matrix core (3 x v_mfma_f32_32x32x16_f16,
 * fp32 accumulate; ~2^-22 relative, see conv_igemm_f16x3.hip).  `w_split` = weights pre-split by the
 * host into (hi, lo) fp16: [K][R][S][C32/32][2][32] halves with C32 = C rounded up to 32 (zero
 * filled), each output channel k pre-multiplied by the power of two `w_scale[k]` (undone exactly in
 * the epilogue).  bias, slope, post_* are fp32.  With flags = 0, x / residual / y are plain fp32 as
 * in dlip_conv_nhwc_f32.  DLIP_SPLIT_IN: x and residual are in the *split activation format* -- per
 * pixel and 32-channel block, 32 hi halves then 32 lo halves (value = hi + lo), i.e. the same 128
 * bytes and the same ld* (counted in fp32 slots) as the fp32 block they replace; C, ldx, ldr (and K
 * when a residual is given) must be multiples of 32.  DLIP_SPLIT_OUT: y is written in that format
 * (K, ldy multiples of 32).  Chains of convolutions then split each activation once, in the
 * producer's epilogue, instead of once per filter tap in every consumer. */
#define DLIP_SPLIT_IN 1
#define DLIP_SPLIT_OUT 2
int dlip_conv_nhwc_f16x3(DLIP_HOST const dlip_conv_desc* d, const float* x, const void* w_split,
                         const float* w_scale, const float* bias, const float* residual,
                         const float* slope, const float* post_scale, const float* post_shift,
                         float* y, int32_t flags, dlip_stream_t stream);

/* dlip_conv_nhwc_f16x3 with a SECOND reduction source: y = epilogue( conv(x, w[:, taps]) + conv1x1_strided(x2, w[:, tail]) ).
 * Replaces conv2 + bn2 and the shortcut's 1x1 stride-2 convolution + BatchNorm of a down-sampling BasicBlock
 * (models/video_models/resnet.py:13-17 downsample_basic_block, :55-69 forward: `out += residual` with
 * residual = self.downsample(x)) in ONE launch: both BatchNorms are folded into the weights, so the sum of the two
 * convolutions is one reduction over [R*S*C32 taps | C2 shortcut channels] (what w_split holds per output channel,
 * under one power-of-two scale w_scale[k]); bias = the sum of the two folded biases.  x2 is [N,H2,W2,C2] in the
 * split activation format (DLIP_SPLIT_IN is mandatory), read at pixel (ho*stride2_h, wo*stride2_w) for output pixel
 * (ho, wo); C2, ldx2 multiples of 32.  residual may still be given (added after both).  Split-format kernel only. */
/* (ABI 43) dlip_conv_nhwc_f16x3 with DLIP_SPLIT_IN, fp32 y, no residual / post-affine, whose epilogue ALSO leaves the column sums of
 * the y it writes: stats [chunks][K][2] fp64 = per chunk of output rows {sum y, sum y^2} -- the batch statistics of the BatchNorm
 * behind a convolution under model.train() (models/audio_models/tdnn.py:35-43: Conv1d -> BatchNorm1d), without the pass over y that
 * dlip_bn_rows_train_fwd_f32 would otherwise make (hand it `stats` as its workspace and `chunks` as ready_chunks).
 * dlip_conv_stats_chunks(d): how many chunks such a launch of `d` writes (two per row tile of its route, dlip_conv_route(d, 3, 3, ..)),
 * or 0 when this shape has no statistics epilogue (today: all but the rows kernel's; the caller then launches the plain convolution).  Within a
 * chunk (half a tile: <= 80 rows) the sums are fp32 in a fixed order; across chunks the finalize kernel adds in fp64. */
int32_t dlip_conv_stats_chunks(DLIP_HOST const dlip_conv_desc* d);
int dlip_conv_nhwc_stats_f16x3(DLIP_HOST const dlip_conv_desc* d, const float* x, const void* w_split, const float* w_scale,
                               const float* bias, const float* slope, float* y, double* stats, int64_t stats_bytes,
                               dlip_stream_t stream);
int dlip_conv2_nhwc_f16x3(DLIP_HOST const dlip_conv_desc* d, const float* x, const float* x2, int32_t H2, int32_t W2,
                          int32_t C2, int32_t ldx2, int32_t stride2_h, int32_t stride2_w, const void* w_split,
                          const float* w_scale, const float* bias, const float* residual, const float* slope,
                          const float* post_scale, const float* post_shift, float* y, int32_t flags,
                          dlip_stream_t stream);

/* dlip_conv_nhwc_f16x3 (DLIP_SPLIT_IN) whose epilogue keeps only POOLED STATISTICS of its output: the rows
 * m = (n, ho, wo) are cut into consecutive groups of `group_rows` (a clip's T*Ho*Wo feature-map pixels; an
 * utterance's T' frames) and every workgroup tile stores, per group segment it contains, the fp64 column sums of
 * y and y^2 -- the [M,K] output itself never reaches memory.  dlip_pool_finish_f32 turns the partial sums into
 *   mode 0: the group means  [G,K]   (AdaptiveAvgPool2d(1) + the temporal mean of the lip-clip features:
 *           models/video_models/resnet.py:125-126, train_fusion.py:274,348 -- a mean of equal-sized means)
 *   mode 1: mean | unbiased std [G,2K] (MeanStdPooling, models/audio_models/pooling.py:24-26), optionally in the
 *           split activation format ([G, 2K rounded up to 32], what fc1's kernel reads).
 * partials: caller-owned, dlip_conv_pool_partial_bytes(d, &tile_rows) bytes (8-byte aligned): the partial bands of the launch's route,
 * dlip_conv_route(d, 3, 2, ..), tile_rows rows each; group_rows must be >= tile_rows (a band then holds at most one group boundary) -- callers fall back to the unfused kernels
 * otherwise.  Sums are formed in a fixed order: results do not depend on scheduling.
 * RAGGED BATCHES (ABI 43).  The reference extracts one utterance / one clip at a time at its own length
 * (train_fusion.py:334-349: audio [1,24,T_i], clips [1,1,T_j,88,88]); a batch of them is the zero-padded tensor +
 * length vector of pad_packed_collate (models/video_models/dataset.py:123-139).  group_len (device int32 [G], NULL =
 * every group is whole): group g is valid for its first clamp(group_len[g] * len_mul + len_add, 0, group_rows) rows, the
 * rest is padding and enters neither sum nor count -- len_mul / len_add turn the caller's unit into pooled rows (lip
 * clips: frames * Ho*Wo of the last convolution; utterances: input frames - the frames the valid convolutions consume),
 * so one length vector in HBM serves the whole step and a recorded plan replays with new lengths.  The valid rows'
 * values equal the unpadded run's (a valid convolution / a per-frame trunk never reads past them; the stem's pre-pass
 * zeroes the padding frames, dlip_stem3d_pool_f16x3).  The speech side starts one stage earlier since ABI 57: a zero-padded batch of
 * waveforms + sample counts goes through the front-end's ragged entry points (dlip_wave_frame_lengths_i32 and the *_ragged_f32
 * kernels further down), which hand the frame counts on as this very length vector. */
int64_t dlip_conv_pool_partial_bytes(DLIP_HOST const dlip_conv_desc* d, DLIP_HOST int32_t* tile_rows);
int dlip_conv_pool_f16x3(DLIP_HOST const dlip_conv_desc* d, const float* x, const void* w_split, const float* w_scale,
                         const float* bias, const float* residual, const float* slope, const float* post_scale,
                         const float* post_shift, double* partials, int64_t partial_bytes, int32_t group_rows,
                         const int32_t* group_len, int32_t len_mul, int32_t len_add, dlip_stream_t stream);
/* M = rows of the pooled convolution, K its channels, tile_rows as reported by dlip_conv_pool_partial_bytes; group_len /
 * len_mul / len_add as given to dlip_conv_pool_f16x3 (the divisor of group g is its valid row count: the masked mean of
 * models/video_models/model.py:16-17, the statistics of one utterance at its own length).
 * y: mode 0 [G,K]; mode 1 [G,2K] or, with out_split != 0, [G, 2K rounded up to 32] split format (padding zeroed). */
int dlip_pool_finish_f32(const double* partials, int64_t M, int32_t K, int32_t tile_rows, int32_t group_rows,
                         const int32_t* group_len, int32_t len_mul, int32_t len_add,
                         int32_t mode, int32_t out_split, float* y, dlip_stream_t stream);

/* Workspace of dlip_conv_nhwc_f16x3's balanced ("stream-K") work split on split-format activations:
 * ticket counters + partial-tile slabs, one block PER STREAM (launches on a stream are ordered and share
 * it).  dlip_conv_workspace_bytes() = size that covers every launch on the current device;
 * dlip_conv_set_workspace registers a caller-owned device block for `stream` (16-byte aligned; its counter
 * words are zeroed asynchronously on that stream; it must stay valid until replaced, unregistered with
 * ptr = NULL, or the stream's work has completed).  A smaller block is legal: launches that need more
 * than it holds run as plain launches.  A stream without a registered block gets a library-owned one on
 * first use (the only allocation the library ever makes). */
int64_t dlip_conv_workspace_bytes(void);
int dlip_conv_set_workspace(void* ptr, int64_t bytes, dlip_stream_t stream);

/* fp32 [rows, C] -> split activation format (and back), C % 32 == 0.  Boundary converters for callers
 * that hold fp32 tensors; inside the encoders the producers write the split format directly. */
int dlip_split_pack_f32(const float* x, float* y, int64_t rows, int32_t C, dlip_stream_t stream);
int dlip_split_unpack_f32(const float* x, float* y, int64_t rows, int32_t C, dlip_stream_t stream);

/* Which kernel and workgroup tile a convolution launch of `d` runs on -- the instance a profiler will show.  Host-only, no launch:
 * the launches execute the answer of the same function (the kernels, the order, every condition).
 *   mode      0 dlip_conv_nhwc_f32, 1 dlip_conv_nhwc_f16x3 on fp32 activations, 3 on split-format activations (DLIP_SPLIT_IN)
 *   epilogue  0 fp32 y, 1 split-format y, 2 pooled partials (dlip_conv_pool_f16x3), 3 y + column sums (DLIP_EINVAL: the shape has none)
 *   C2        channels of dlip_conv2_nhwc_f16x3's second source, or 0;  unaligned != 0: y or the residual is off 16 bytes;  d->ldr
 *             != 0 says that a residual is added (dlip_conv_nhwc_f16x3 goes by the pointer: pass ldr = 0 without one)
 *   *kind     0 LDS-DMA ring, 1 window, 2 rows, 3 register-staged conv_igemm_f16x3_kernel (also: split input with an fp32 y whose K
 *             or ldy is no multiple of 4), 4 conv_igemm_f32_kernel;  *bm, *bn: that instance's tile */
int dlip_conv_route(DLIP_HOST const dlip_conv_desc* d, int32_t mode, int32_t epilogue, int32_t C2, int32_t unaligned,
                    DLIP_HOST int32_t* kind, DLIP_HOST int32_t* bm, DLIP_HOST int32_t* bn);
/* dlip_conv_route(d, split_f16, 0, 0, 0, ..)'s tile: of whichever kernel serves the launch (window, register-staged at K % 4 != 0, ..). */
int dlip_conv_plan(DLIP_HOST const dlip_conv_desc* d, int32_t split_f16, DLIP_HOST int32_t* bm, DLIP_HOST int32_t* bn);
/* dlip_conv_route(d, 3, 0, 0, 0, ..)'s kind where it is 1 (window) or 2 (rows); 0 for every other kernel (so at K % 4 != 0 with an fp32 y). */
int dlip_conv_kernel_kind(DLIP_HOST const dlip_conv_desc* d);

/* ------------------------------------------------------------------------------------------
 * Video stem: Conv3d(1->K, 5x7x7, stride (1,2,2), pad (2,3,3), no bias) + BatchNorm3d + PReLU|ReLU
 * (BN folded into w/bias; slope[k] = PReLU weight or 0 for ReLU), output NDHWC = [(B*T),Ho,Wo,K].
 * Replaces models/video_models/model.py:81-84 (frontend3D.0-.2) and makes threeD_to_2D_tensor
 * (model.py:9-13) a no-op.  x is [B,T,H,W] (the reference's [B,1,T,H,W]); w is [K][5][7][7] padded
 * to [K][248]; H, W even.
 * ------------------------------------------------------------------------------------------ */
int dlip_stem3d_bn_act_f32(const float* x, const float* w_k248, const float* bias, const float* slope,
                           float* y, int32_t B, int32_t T, int32_t H, int32_t W, int32_t K,
                           dlip_stream_t stream);

/* Split-fp16 variant of dlip_stem3d_bn_act_f32 (3 x v_mfma_f32_16x16x32_f16 per product, fp32
 * accumulate; fp32 in / fp32 out).  w_split = 64 x 1184 bytes: per output channel a hi plane [36 kernel
 * rows (kt*7+kh; row 35 zero)][8 taps (kw; tap 7 zero)] of fp16, then the lo plane of the same shape, + 32
 * bytes of padding, pre-multiplied by the power of two w_scale[k] (deeplip_amd.packing.pack_stem3d).  W <= 88. */
int dlip_stem3d_bn_act_f16x3(const float* x, const void* w_split, const float* w_scale, const float* bias,
                             const float* slope, float* y, int32_t B, int32_t T, int32_t H, int32_t W,
                             int32_t K, dlip_stream_t stream);

/* dlip_stem3d_bn_act_f16x3 + MaxPool3d((1,3,3), stride (1,2,2), pad (0,1,1)) (replaces
 * models/video_models/model.py:81-85): the pre-pool activations never reach memory.  y is
 * [(B*T), Hp, Wp, 64] with Hp = (H/2 - 1)/2 + 1, in the split activation format of
 * dlip_conv_nhwc_f16x3 (what the trunk's first layers read).  H, W even, W <= 88.
 * x_split: caller-owned scratch of dlip_stem3d_pool_workspace_bytes(B, T, H, W) bytes, 16-B aligned -- a
 * pre-pass writes the clip there once as (hi, lo) fp16 pairs at the kernel's window row pitch, and the
 * kernel fetches its windows from it by LDS-DMA (two launches on `stream`).
 * lengths (device int32 [B], NULL = every clip has T frames; ABI 43): clip b's frames t >= lengths[b] are padding
 * (pad_packed_collate, models/video_models/dataset.py:123-139) and the pre-pass writes them as ZEROS of the normalised clip
 * whatever x holds there -- for the frames t < lengths[b] that is the Conv3d's own zero padding behind the clip's last frame,
 * so their outputs equal the clip run alone at its own length (train_fusion.py:346-348). */
int64_t dlip_stem3d_pool_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t W);
int dlip_stem3d_pool_f16x3(const float* x, const int32_t* lengths, void* x_split, const void* w_split, const float* w_scale,
                           const float* bias, const float* slope, float* y, int32_t B, int32_t T, int32_t H,
                           int32_t W, int32_t K, dlip_stream_t stream);

/* dlip_stem3d_pool_f16x3 fed with the frames as a loader hands them over: uint8, `channels` = 1 (gray [B,T,Hs,Ws], what the
 * reference's npz mouth crops hold: models/video_models/dataset.py) or 3 (RGB [B,T,3,Hs,Ws], BASELINE.json's input shape).
 * The pre-pass crops H x W at row oy, column ox (CenterCrop, preprocess.py:89-90: oy = (Hs - H) / 2 rounded DOWN) and
 * normalises while it writes the split clip: gray = 0.299 R + 0.587 G + 0.114 B kept in float (preprocess.py:32-46),
 * (gray / 255 - 0.421) / 0.165 (dataloaders.py:11-22), mul / add / IEEE divide in that order, uncontracted -- bit-identical
 * to dlip_ingest_rgb_u8 (or dlip_crop_normalize_u8) followed by dlip_stem3d_pool_f16x3, without the fp32 clip: a quarter of
 * the host-to-device bytes, one HBM write and one read of 4 B per pixel less.  Replaces train_fusion.py:346-348's
 * `.to(device)` of a float clip + model.py:81-85.
 * clip_params (device int32 [B][4], NULL = (oy, ox) for every clip, no flip; ABI 43): per clip (oy_b, ox_b, flip_b, 0) -- the
 * train pipeline's RandomCrop origin and HorizontalFlip coin (preprocess.py:95-138, dataloaders.py:13-17: ONE draw per clip, all
 * of its frames alike; the host draws them from its seeded generator); flip_b != 0 mirrors the cropped frame left-right
 * (pixel w <- column ox_b + W - 1 - w).  Origins are clamped into the frame.  lengths: as dlip_stem3d_pool_f16x3 (here the
 * only way to pad: a zero byte is not a zero of the normalised clip). */
int dlip_stem3d_pool_u8_f16x3(const uint8_t* frames, int32_t channels, int32_t Hs, int32_t Ws, int32_t oy, int32_t ox,
                              const int32_t* clip_params, const int32_t* lengths,
                              void* x_split, const void* w_split, const float* w_scale, const float* bias,
                              const float* slope, float* y, int32_t B, int32_t T, int32_t H, int32_t W, int32_t K,
                              dlip_stream_t stream);

/* Self-test of a hardware behaviour the layer-1 / layer-2 window kernel (conv_win_f16x3.hip) relies on: a ds_read_b128 at an
 * LDS address with bit 18 set (beyond every allocation) returns zeros on gfx950 -- the kernel uses that as the zero
 * padding of taps outside the image, and is selected on gfx950 devices only.  `blocks` workgroups of 256 lanes, 8 KB of
 * LDS each (several per CU), fill their allocation with a pattern and read inside and beyond it; counts (device int32[2])
 * receives [lanes whose in-range read returned the pattern, lanes whose out-of-range reads returned anything non-zero]:
 * expected [256 * blocks, 0]. */
int dlip_selftest_lds_oob(int32_t* counts, int32_t blocks, dlip_stream_t stream);

/* MaxPool3d((1,3,3), stride (1,2,2), pad (0,1,1)) on NHWC: [N,H,W,C] -> [N,Ho,Wo,C],
 * Ho = (H+2-3)/2+1.  Replaces models/video_models/model.py:85.  C % 4 == 0.  out_split != 0 writes y
 * in the split activation format of dlip_conv_nhwc_f16x3 (C % 32 == 0). */
int dlip_maxpool3x3s2_nhwc_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C,
                               int32_t out_split, dlip_stream_t stream);

/* AdaptiveAvgPool2d(1) + flatten on NHWC: [N,HW,C] -> [N,C].  Replaces resnet.py:83,125-126. */
int dlip_avgpool_nhwc_f32(const float* x, float* y, int32_t N, int32_t HW, int32_t C,
                          dlip_stream_t stream);

/* Masked temporal mean: y[b,c] = mean_{t < len[b] + len_add} x[b,t,c]; len == NULL means T for every b.
 * Replaces torch.mean(..., dim=0) over frames (train_fusion.py:274,348) and _average_batch
 * (models/video_models/model.py:16-17).  x [B,T,C] with row stride ldx floats. */
int dlip_time_mean_f32(const float* x, const int32_t* len, int32_t len_add, float* y, int32_t B, int32_t T, int32_t C,
                       int32_t ldx, dlip_stream_t stream);

/* Ragged batches on the paths without a stem pre-pass (exact-fp32 packing, taps): y[b,t,:] = t < len[b] ? x[b,t,:] : 0 for x
 * [B,T,E] -- the padding frames of pad_packed_collate (models/video_models/dataset.py:123-139) as zeros of the normalised
 * clip.  E % 4 == 0, x and y 16-byte aligned (y may be x). */
int dlip_mask_frames_f32(const float* x, const int32_t* len, float* y, int32_t B, int32_t T, int32_t E, dlip_stream_t stream);

/* Segmented mean over clip groups (CSR offsets, G+1 entries): y[u] = sum(x[ptr[u]:ptr[u+1]]) / count.
 * Replaces the per-utterance clip-file average (train_fusion.py:272-275,346-349). */
int dlip_group_mean_f32(const float* x, const int32_t* group_ptr, float* y, int32_t U, int32_t C,
                        dlip_stream_t stream);

/* MeanStdPooling on N-T-C: y[b, 0:C] = mean_t, y[b, C:2C] = unbiased std_t (N-1); sums of x and x^2
 * in fp64.  Replaces models/audio_models/pooling.py:24-26.  C % 4 == 0.  out_split != 0 writes y as
 * [B, 2C rounded up to 32] in the split activation format of dlip_conv_nhwc_f16x3 (padding zeroed).
 * len (device int32 [B], NULL = T for every b; ABI 43): utterance b's statistics cover its first
 * clamp(len[b] + len_add, 0, T) frames -- a zero-padded batch pooled as the reference pools each utterance at its own
 * length (train_fusion.py:334-338); len_add = -(frames the valid convolutions in front consumed) when len counts input frames. */
int dlip_meanstd_pool_f32(const float* x, const int32_t* len, int32_t len_add, float* y, int32_t B, int32_t T, int32_t C,
                          int32_t out_split, dlip_stream_t stream);

/* (AttentiveStatPooling's tail, models/audio_models/pooling.py:87-107, and its backward: the dlip_mh_attn_* entry points below with
 * n = 1 and eps = 0, ABI 67.) */

/* Layout adapters at the API boundary.
 *   dlip_nct_to_ntc_f32: x [B,C,T] (reference layout, tdnn.py:89) -> y [B,T,Cp] zero-padded to Cp>=C.
 *   dlip_ntc_to_nct_f32: y [B,C,T] <- x [B,T,C].
 *   dlip_ingest_rgb_u8 : [B,T,3,H,W] uint8 RGB -> [B,T,H,W] float = ((0.299R+0.587G+0.114B)/255-0.421)/0.165
 *                        (constants: models/video_models/dataloaders.py:12,21-22; build-owned adapter). */
int dlip_nct_to_ntc_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, int32_t Cp,
                        dlip_stream_t stream);
int dlip_ntc_to_nct_f32(const float* x, float* y, int32_t B, int32_t T, int32_t C,
                        dlip_stream_t stream);
/* dlip_nct_to_ntc_f32 + dlip_split_pack_f32 in one pass: y [B,T,Cp] in the split activation format, Cp % 32 == 0. */
int dlip_nct_to_ntc_split_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, int32_t Cp,
                              dlip_stream_t stream);
int dlip_ingest_rgb_u8(const uint8_t* x, float* y, int64_t n_frames, int32_t H, int32_t W,
                       dlip_stream_t stream);

/* Eval-mode BatchNorm1d (as per-channel scale/shift) and LeakyReLU(slope) on [M,C]:
 * order 0: y = lrelu(x*scale + shift)  (bn_first, tdnn.py:92-94,105-107; model_fusion.py:21-22)
 * order 1: y = lrelu(x)*scale + shift  (tdnn.py:96-97,109-110). */
int dlip_affine_act_f32(const float* x, const float* scale, const float* shift, float* y, int64_t M,
                        int32_t C, float slope, int32_t order, dlip_stream_t stream);

/* Per-row z-normalisation with the UNBIASED std (train_fusion.py:233-238) of a [U,Da] and a [U,Dv]
 * table, concatenated into y [U, Da+Dv] (train_fusion.py:353-358).  Either input may be NULL
 * (D = 0) to z-normalise a single table.  biased != 0 selects numpy's biased std
 * (models/fusion_models/utils.py:524-527, feature-fusion scoring). */
int dlip_znorm_cat_f32(const float* a, int32_t Da, const float* v, int32_t Dv, float* y, int32_t U,
                       int32_t biased, dlip_stream_t stream);

/* dlip_znorm_cat_f32 whose second table is the per-clip mean still held as pooled partial sums (dlip_conv_pool_f16x3
 * over groups of T*Ho*Wo rows; M, K, tile_rows, group_rows as for dlip_pool_finish_f32, U = number of groups): the
 * temporal mean of train_fusion.py:348 and the fusion of :353-358 in one launch; bit-identical to
 * dlip_pool_finish_f32 (mode 0) followed by dlip_znorm_cat_f32 (group_len / len_mul / len_add as there). */
int dlip_znorm_cat_pooled_f32(const float* a, int32_t Da, const double* partials, int64_t M, int32_t K,
                              int32_t tile_rows, int32_t group_rows, const int32_t* group_len, int32_t len_mul,
                              int32_t len_add, float* y, int32_t U, int32_t biased, dlip_stream_t stream);

/* y[u,:] = x[u,:] / max(||x[u,:]||_2, eps)   (F.normalize; loss.py:44, train_audio.py:355). */
int dlip_l2_normalize_f32(const float* x, float* y, int32_t U, int32_t D, float eps,
                          dlip_stream_t stream);

/* PLDA trial scoring (eer_plda_lomgrid / eer_plda_grid, models/fusion_models/utils.py:285-329: the `plda`
 * package's model.transform(..., 'D' -> 'U_model') followed by calc_same_diff_log_likelihood_ratio per trial).
 * u [N,D] = the embeddings already mapped to the model's latent space (an affine map: one dlip_conv_nhwc_f32
 * GEMM, deeplip_amd/plda.py), psi [D] = the between-class variances there (within-class covariance = I):
 * score[i] = log p(u_a, u_b | same speaker) - log p(u_a) - log p(u_b). */
int dlip_plda_llr_f32(const float* u, int32_t N, int32_t D, const float* psi, const int32_t* idx_a,
                      const int32_t* idx_b, float* score, int32_t n_trials, dlip_stream_t stream);

/* Trial scoring over an [N,D] embedding table: score[i] = cos(emb[idx_a[i]], emb[idx_b[i]]).
 * mode 0: sklearn cosine_similarity semantics (normalise each row, then dot; utils.py:244,262)
 * mode 1: F.cosine_similarity(eps) semantics  (dot / max(||a||*||b||, eps); utils.py:372).
 * score_io: if accumulate != 0, score[i] = score[i] + weight*cos, else score[i] = weight*cos
 * (score-level fusion 0.5/0.5, utils.py:343-377). */
int dlip_pair_cosine_f32(const float* emb, int32_t N, int32_t D, const int32_t* idx_a,
                         const int32_t* idx_b, float* score, int32_t n_trials, int32_t mode,
                         float eps, float weight, int32_t accumulate, dlip_stream_t stream);

/* (ABI 58) COHORT SCORE NORMALISATION of the trial scores above (Z-/T-/S-norm, adaptive S-norm with a top-K cohort).  The reference
 * scores raw cosines only (models/fusion_models/utils.py:251-283, :331-522); the normalised forms are build-owned, DESIGN.md 3f.
 *
 * dlip_topk_stats_f32: s is a score matrix of R rows with pitch ld (floats): row r is s[r*ld .. r*ld+N), columns [N, ld) are never
 * read (a GEMM's padded output width).  mean[r] / sd[r] = mean and POPULATION deviation (divisor K) of the K largest values of row r,
 * ties at the K-th value counted exactly: the selection is exact (radix select over order-preserving keys of the row held in LDS),
 * both statistics accumulate in fp64 (the deviation centred on the mean, from the on-chip copy) and are rounded to fp32 once.
 * 1 <= K <= N <= 32768 (a 32768-float row is 128 KiB of the CU's 160 KiB LDS), ld >= N; anything else, a null pointer or R <= 0 is
 * DLIP_EINVAL before any launch.  Inputs are taken to be finite; a non-finite value cannot hang or fault the kernel (the keys stay
 * totally ordered), what it yields is unspecified. */
int dlip_topk_stats_f32(const float* s, int32_t R, int32_t N, int64_t ld, int32_t K, float* mean, float* sd,
                        dlip_stream_t stream);

/* out[i] = weight * z(s[i]) (accumulate != 0: out[i] += ...), with za = (s[i] - mu[idx_a[i]]) / max(sd[idx_a[i]], eps), zb likewise
 * through idx_b, and z = za (mode 0, Z-norm), zb (mode 1, T-norm) or (za + zb) / 2 (mode 2, S-norm).  mu / sd [U] are the per-utterance
 * cohort statistics of dlip_topk_stats_f32; weight / accumulate as in dlip_pair_cosine_f32, so the two halves of a score fusion are
 * normalised separately and added.  out may be s.  An index outside [0, U) is the caller's error (its trial comes out NaN, nothing is
 * read out of bounds); hosts that hold the indices validate them first. */
int dlip_score_norm_f32(const float* s, const int32_t* idx_a, const int32_t* idx_b, int32_t n, const float* mu, const float* sd,
                        int32_t U, int32_t mode, float eps, float weight, int32_t accumulate, float* out, dlip_stream_t stream);

/* logits[b,k] =<normalize(e[b]), normalize(W[k])> (cosine logits, loss.py:44) when cosine != 0,
 * else <e[b], W[k]> + bias[k] (loss.py:14); argmax[b] = first index of the row maximum
 * (torch.max(logits,1)[1]; train_fusion.py:296), int64.  K <= 1024. */
int dlip_logits_argmax_f32(const float* e, const float* W, const float* bias, float* logits,
                           int64_t* argmax, int32_t B, int32_t D, int32_t K, int32_t cosine,
                           dlip_stream_t stream);

/* Softmax cross-entropy over margin-adjusted logits (forward value only):
 *   z[b,k] = scale * (logits[b,k] - margin*[k==label[b]]) + 1e-8;  loss = mean_b( lse(z[b]) - z[b,label] )
 * LMCL: scale=s, margin=m (loss.py:45-48); CrossEntropy: scale=1, margin=0 (loss.py:15).
 * loss is one float on the device. */
int dlip_margin_ce_loss_f32(const float* logits, const int64_t* labels, float* loss, int32_t B,
                            int32_t K, float scale, float margin, dlip_stream_t stream);

/* LowFER.forward as shipped (LBP.py:46-50): y = cat[e1, sigmoid(e2), sigmoid(e2)*e1], [B,3D]. */
int dlip_lowfer_cat_f32(const float* e1, const float* e2, float* y, int32_t B, int32_t D,
                        dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GPU-side preprocessing in front of the hot path.  Audio features as
 * the reference computes them with python_speech_features (models/audio_models/datasets.py:65-83,52-53);
 * the DFT / mel / DCT matrix products go through dlip_conv_nhwc_f32 (deeplip_amd/frontend.py).
 * ------------------------------------------------------------------------------------------ */
/* x [B,S] waveform -> frames [B*NF, nfft]: frame f = pre-emphasised samples [f*step, f*step+len), zero
 * padded to nfft and past the end of the signal (sigproc.preemphasis + framesig, rectangular window). */
int dlip_frame_preemph_f32(const float* x, float* frames, int32_t B, int32_t S, int32_t NF, int32_t frame_len,
                           int32_t frame_step, int32_t nfft, float preemph, dlip_stream_t stream);
/* spec [R, 2*NB] (re | im) -> pw [R, NBp] = |.|^2 / nfft (zero padded), energy [R] = row sum (0 -> eps). */
int dlip_powspec_f32(const float* spec, float* pw, float* energy, int32_t R, int32_t NB, int32_t NBp,
                     int32_t nfft, dlip_stream_t stream);
/* frames [R, nfft] (dlip_frame_preemph_f32) -> pw / energy as dlip_powspec_f32, the DFT itself evaluated in fp64 (numpy's
 * rfft under python_speech_features is double): for filterbanks whose lowest bands hold ~1e-9 of the spectrum (80 bands at
 * nfft 512) the fp32-GEMM DFT's rounding noise is larger than the signal.  nfft a power of two <= 1024. */
int dlip_powspec_dft64_f32(const float* frames, float* pw, float* energy, int32_t R, int32_t NB, int32_t NBp,
                           int32_t nfft, dlip_stream_t stream);
/* (ABI 46) x [B,S] waveform -> pw [B*NF, NBp] / energy [B*NF] as above, with pre-emphasis, framing and the DFT (a radix-2 FFT in LDS, one
 * workgroup per frame) ALL in fp64, as python_speech_features computes them (sigproc.preemphasis / framesig / numpy rfft on doubles;
 * features/audio front-end of models/audio_models/datasets.py:60-82).  `preemph` is a double: the reference's 0.97 is.  What the fp32 routes
 * lose: elements holding ~1e-12 of a frame's energy (the lowest mel band of a frame that pre-emphasis empties), 0.3 .. 1 % there.  The
 * default route of deeplip_amd.frontend.AudioFrontend since ABI 46.  nfft a power of two, 128 .. 1024. */
int dlip_powspec_wave_fft64_f32(const float* x, float* pw, float* energy, int64_t B, int64_t S, int32_t NF, int32_t frame_len,
                                int32_t frame_step, int32_t nfft, double preemph, int32_t NB, int32_t NBp, dlip_stream_t stream);
/* y = log(x == 0 ? eps : x). */
int dlip_log_floor_f32(const float* x, float* y, int64_t n, dlip_stream_t stream);
/* feat [B,NF,C] (row stride ldf; channel 0 := log(energy) when energy != NULL) -> per-utterance
 * (x - mean)/(std + 2e-12) when normalize != 0 -> y [B,C,NF] (the reference loaders' layout). */
int dlip_cmvn_nct_f32(const float* feat, const float* energy, float* y, int32_t B, int32_t NF, int32_t C,
                      int32_t ldf, int32_t normalize, dlip_stream_t stream);
/* Delta features as SpkTrainDataset._delta appends them (models/audio_models/datasets.py:55-63, `delta: true`):
 * x [B,C,NF] -> y [B,(1+order)C,NF] = [x | delta(x, N=1) | delta(x, N=2)], python_speech_features.delta with edge
 * padding; order 1 or 2. */
int dlip_delta_nct_f32(const float* x, float* y, int32_t B, int32_t C, int32_t NF, int32_t order, dlip_stream_t stream);
/* uint8 frames [n, channels(1|3), H, W] (n = B clips of T frames) -> crop [n, crop, crop] float = ((gray)/255 - 0.421)/0.165
 * (models/video_models/dataloaders.py:11-22; RGB -> gray with the BT.601 weights).  clip_params NULL: the "val" / "test"
 * pipeline's CenterCrop (preprocess.py:89-90); clip_params (device int32 [B][4] = (oy, ox, flip, 0); ABI 43): the "train"
 * pipeline's RandomCrop + HorizontalFlip (preprocess.py:95-138, dataloaders.py:13-17), one host draw per clip.  lengths
 * (device int32 [B], NULL = whole clips): frames t >= lengths[b] are written as zeros of the normalised clip -- the padding
 * of pad_packed_collate, which pads AFTER the normalisation (dataset.py:117,130-134). */
int dlip_crop_normalize_u8(const uint8_t* x, const int32_t* clip_params, const int32_t* lengths, int32_t T, float* y,
                           int64_t n_frames, int32_t channels, int32_t H, int32_t W, int32_t crop, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Train-mode / backward kernels for the trainable fusion head and criterion (config C5; the
 * encoders stay frozen, train_fusion.py:198-201).  Replace the autograd of
 *   nn.Linear / nn.BatchNorm1d(train) / nn.LeakyReLU   models/fusion_models/model_fusion.py:19-24
 *   F.cross_entropy, F.normalize, F.linear              models/audio_models/loss.py:13-16,43-51
 * ------------------------------------------------------------------------------------------ */
/* y = lrelu_slope(BN_train(x)) on [M,C]: batch mean / biased variance, saves mean and 1/std for the
 * backward, updates running stats (unbiased variance, `momentum`) when the pointers are non-NULL.
 * slope = 1 gives plain BatchNorm1d. */
int dlip_bn1d_train_fwd_f32(const float* x, const float* gamma, const float* beta, float* y,
                            float* save_mean, float* save_invstd, float* running_mean,
                            float* running_var, int32_t M, int32_t C, float momentum, float eps,
                            float slope, dlip_stream_t stream);
int dlip_bn1d_train_bwd_f32(const float* dy, const float* x, const float* save_mean,
                            const float* save_invstd, const float* gamma, float* dx, float* dgamma,
                            float* dbeta, int32_t M, int32_t C, dlip_stream_t stream);
/* dx = dy * (y >= 0 ? 1 : slope)  (LeakyReLU backward from the OUTPUT; slope > 0). */
int dlip_lrelu_bwd_f32(const float* dy, const float* y, float* dx, int64_t n, float slope,
                       dlip_stream_t stream);
/* y[c] = sum_m x[m,c]  (bias gradients). */
int dlip_colsum_f32(const float* x, float* y, int32_t M, int32_t C, dlip_stream_t stream);
/* out[0] = sum |w[i]| (fp64 accumulation, fixed order) -- the L1 regulariser of LMCL, 1e-5 * ||W||_1 (models/audio_models/loss.py:
 * 49-50); dlip_l1_sign_f32: dw[i] = coef * grad_scale_dev[0] * sign(w[i]) (grad_scale_dev NULL: 1), its gradient. */
int dlip_l1_sum_f32(const float* w, float* out, int64_t n, dlip_stream_t stream);
int dlip_l1_sign_f32(const float* w, const float* grad_scale_dev, float* dw, float coef, int64_t n, dlip_stream_t stream);

/* dlogits = grad_scale * grad_scale_dev[0] * d/dlogits mean_b CE(scale*(logits - margin*onehot) + 1e-8, labels);
 * grad_scale_dev = the upstream gradient of the scalar loss as a DEVICE scalar (NULL = 1): autograd's backward
 * does not have to read it back to the host. */
int dlip_margin_ce_bwd_f32(const float* logits, const int64_t* labels, float* dlogits, int32_t B,
                           int32_t K, float scale, float margin, float grad_scale,
                           const float* grad_scale_dev, dlip_stream_t stream);
/* Backward of dlip_l2_normalize_f32. */
int dlip_l2_normalize_bwd_f32(const float* x, const float* dy, float* dx, int32_t U, int32_t D,
                              float eps, dlip_stream_t stream);
/* C[M,N] = op(A)[M,K] * op(B)[K,N], row-major, any sizes (head gradients: dX = dY W, dW = dY^T X). */
int dlip_gemm_small_f32(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K,
                        int32_t trans_a, int32_t trans_b, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Train-mode kernels of the speech encoder (deeplip_amd/csrc/encoder_train_ops.hip).
 * They serve torch.autograd Functions in deeplip_amd/autograd.py that replace what autograd does for
 * SpeakerEmbNet.forward under model.train() (train_audio.py:167-183; models/audio_models/tdnn.py:35-43,
 * 89-111; pooling.py:24-26).  Column reductions over the M = B*T' rows are deterministic (fixed 512-row
 * chunks, fp64 partials in `workspace` = dlip_bn_rows_chunks(M) * C * 2 doubles, added in chunk order).
 * ------------------------------------------------------------------------------------------ */
int32_t dlip_bn_rows_chunks(int32_t M);

/* BatchNorm over rows, training mode, fused with LeakyReLU(slope): x, y [M,C], C % 4 == 0.
 * act_first = 0: y = lrelu(bn(x))  (TDNN_Block bn_first=True, tdnn.py:36-38; bn1/bn2 in tdnn.py:93-94,106-107)
 * act_first = 1: y = bn(lrelu(x))  (bn_first=False, tdnn.py:40-42,96-97,109-110).
 * Batch statistics: biased variance for the normalisation, unbiased for running_var (momentum update,
 * nullable pair), as nn.BatchNorm1d.  save_mean / save_invstd [C] feed the backward. */
/* (ABI 44) y == NULL: statistics only (save_mean, save_invstd, running statistics, the counter) -- the consumer applies the
 * normalisation and the activation on load (dlip_wgrad_operand_split_bn_f32 / dlip_wgrad_chwn_bn_f32) and the activated tensor is
 * never stored.
 * (ABI 44) num_batches_tracked (nullable): the module's int64 counter, incremented by the launch that finishes the statistics
 * (nn.BatchNorm*.forward under model.train(): `self.num_batches_tracked += 1` -- 44 one-element torch launches per lip-clip step).
 * Launch sequence since ABI 44: the finalize steps (partials -> mean / 1/std, -> dgamma / dbeta / dslope, -> the lift of dx) run in
 * the LAST workgroup of the pass before them (a ticket word of the stream's dlip_conv_set_workspace block, when the stream has one)
 * instead of in launches of their own, the parts of a column reduction grow beyond 512 rows so that there are at most 512 of them,
 * and tensors of M <= 4096 rows (the MS-TCN head's, tcn.py:42-43) take ONE launch per direction.  dlip_debug_set(8, 0) restores
 * the ABI 43 sequence.  Results are deterministic either way; the association of the fp64 column sums differs between the two.
 * (ABI 43) ready_chunks > 0 (act_first == 0 only): `workspace` already holds that many partial rows [chunk][C][2] fp64 = {sum x,
 * sum x^2} of x, written by the convolution that produced x (dlip_conv_nhwc_stats_f16x3): the statistics pass over x is skipped. */
int dlip_bn_rows_train_fwd_f32(const float* x, const float* gamma, const float* beta, float* y,
                               float* save_mean, float* save_invstd, float* running_mean,
                               float* running_var, double* workspace, int32_t M, int32_t C, float momentum,
                               float eps, float slope, int32_t act_first, int32_t ready_chunks, int64_t* num_batches_tracked,
                               dlip_stream_t stream);
/* Backward of the above: dy = dL/dy -> dx = dL/dx [M,C], dgamma, dbeta [C].  dx_lift2 (nullable, DLIP_LIFT_WORDS floats: the pair, then per-workgroup scratch): the power-of-two
 * lift of dx, (2^e, 2^-e) with max|dx| * 2^e in [512, 1024] -- what dlip_pow2_scale_f32(dx, ., 1024) would return, formed by the
 * pass that writes dx: the convolution backward that consumes dx needs it and would otherwise read dx once more. */
int dlip_bn_rows_train_bwd_f32(const float* dy, const float* x, const float* gamma, const float* beta,
                               const float* save_mean, const float* save_invstd, float* dx, float* dgamma,
                               float* dbeta, double* workspace, int32_t M, int32_t C, float slope,
                               int32_t act_first, float* dx_lift2, dlip_stream_t stream);
/* BatchNorm (batch statistics) + PReLU with PER-CHANNEL slopes in the same passes: y = prelu(bn(x)) (resnet.py:51-53 bn1 + relu1,
 * tcn.py:42-43, model.py:83-84 under model.train()).  Forward as dlip_bn_rows_train_fwd_f32 with slope[C] applied behind the
 * affine; backward additionally returns dslope[C] = sum over rows of (bn(x) < 0 ? dy * bn(x) : 0) from the SAME pass that
 * forms dgamma / dbeta -- `workspace` holds 2 * dlip_bn_rows_chunks(M) * C * 2 doubles here.  Saves the separate PReLU
 * forward / backward passes and the column sum of its slope terms. */
int dlip_bn_prelu_rows_train_fwd_f32(const float* x, const float* gamma, const float* beta, const float* slope, float* y,
                                     float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                                     double* workspace, int32_t M, int32_t C, float momentum, float eps,
                                     int64_t* num_batches_tracked, dlip_stream_t stream);
int dlip_bn_prelu_rows_train_bwd_f32(const float* dy, const float* x, const float* gamma, const float* beta, const float* slope,
                                     const float* save_mean, const float* save_invstd, float* dx, float* dgamma, float* dbeta,
                                     float* dslope, double* workspace, int32_t M, int32_t C, float* dx_lift2, dlip_stream_t stream);
/* (ABI 44) BatchNorm3d (batch statistics) + PReLU + MaxPool3d((1,3,3),(1,2,2),(0,1,1)) of the stem under model.train()
 * (models/video_models/model.py:83-85) WITHOUT the full-resolution tensors between them: x [N,H,W,C] = the stem convolution's output.
 * (dy_pooled2, nullable: a second gradient of the pooled output, added on the fly -- the first BasicBlock's convolution and its
 * shortcut both consume it.)
 * Forward: statistics of x (workspace as dlip_bn_rows_train_fwd_f32 with M = N H W), then ONE pass writes the pooled y
 * [N,Ho,Wo,C] and the argmax codes idx [N,Ho,Wo,C/4] (dlip_maxpool3x3s2_idx_f32's: tap r*3+s of the first maximum, one byte per
 * channel); prelu(bn(x)) is never stored.  Backward: dy_pooled [N,Ho,Wo,C] -> dx [N,H,W,C], dgamma, dbeta, dslope: both passes form
 * the gradient behind the pooling per input pixel from the <= 4 windows covering it (idx, dy_pooled) instead of reading a scattered
 * full-resolution gradient (workspace: 2 * dlip_bn_rows_chunks(N H W) * C * 2 doubles; dx_lift2 as above).  At B = 32 the stem's
 * train-mode passes move 3.2 GB instead of 5.6 GB. */
int dlip_bn_prelu_maxpool_train_fwd_f32(const float* x, const float* gamma, const float* beta, const float* slope, float* y,
                                        uint32_t* idx, float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                                        double* workspace, int64_t N, int32_t H, int32_t W, int32_t C, float momentum, float eps,
                                        int64_t* num_batches_tracked, dlip_stream_t stream);
int dlip_bn_prelu_maxpool_train_bwd_f32(const float* dy_pooled, const float* dy_pooled2, const uint32_t* idx, const float* x, const float* gamma,
                                        const float* beta, const float* slope, const float* save_mean, const float* save_invstd,
                                        float* dx, float* dgamma, float* dbeta, float* dslope, double* workspace, int64_t N, int32_t H,
                                        int32_t W, int32_t C, float* dx_lift2, dlip_stream_t stream);
/* (ABI 44) The END of a BasicBlock under model.train(): y = prelu(bn2(x) + residual), x = conv2's output
 * (models/video_models/resnet.py:62-69: `out = self.bn2(out); out += residual; out = self.relu2(out)`), rows x [M,C].
 * Forward: statistics of x, then ONE pass writes sum = bn2(x) + residual (kept for the backward) and y; bn2's output is never stored.
 * Backward: dy [M,C] (+ dy2, nullable: a second gradient of y -- the next block's first convolution AND its shortcut both consume y --
 * added on the fly) -> dresidual [M,C] = the gradient behind the PReLU (the shortcut's gradient and bn2's incoming one), dx [M,C],
 * dgamma, dbeta (bn2), dslope (relu2): the first pass forms dresidual, the slope gradient's terms and bn2's two sums from one read of
 * dy, sum and x (was: PReLU backward writing two tensors, a column sum, the BatchNorm's sums pass); the second is the BatchNorm
 * backward's apply pass.  workspace: 2 * dlip_bn_rows_chunks(M) * C * 2 doubles; dx_lift2 as above. */
int dlip_bn_add_prelu_rows_train_fwd_f32(const float* x, const float* residual, const float* gamma, const float* beta,
                                         const float* slope, float* sum, float* y, float* save_mean, float* save_invstd,
                                         float* running_mean, float* running_var, double* workspace, int32_t M, int32_t C,
                                         float momentum, float eps, int64_t* num_batches_tracked, dlip_stream_t stream);
int dlip_bn_add_prelu_rows_train_bwd_f32(const float* dy, const float* dy2, const float* sum, const float* x, const float* gamma,
                                         const float* beta, const float* slope, const float* save_mean, const float* save_invstd,
                                         float* dresidual, float* dx, float* dgamma, float* dbeta, float* dslope, double* workspace,
                                         int32_t M, int32_t C, float* dx_lift2, dlip_stream_t stream);
/* (ABI 44) The apply pass alone: y = act((x - mean) invstd gamma + beta) on [M,C] rows from statistics already formed (a deferred
 * activation -- dlip_bn_rows_train_fwd_f32 with y == NULL -- whose consumer turns out to need the values after all). */
int dlip_bn_apply_rows_f32(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* slope_vec, float slope, float* y, int32_t M, int32_t C, dlip_stream_t stream);
/* y[c] = sum_m x[m,c] (bias gradients), same chunked reduction and workspace. */
int dlip_colsum_rows_f32(const float* x, float* y, double* workspace, int32_t M, int32_t C, dlip_stream_t stream);

/* MeanStdPooling backward (pooling.py:24-26): x [B,T,C], y = forward output [B,2C] (mean | unbiased std),
 * dy [B,2C] -> dx [B,T,C].  C % 4 == 0, T > 1. */
int dlip_meanstd_pool_bwd_f32(const float* x, const float* y, const float* dy, float* dx, int32_t B, int32_t T,
                              int32_t C, dlip_stream_t stream);

/* y = x permuted: x [d0,d1,d2]; output axis i is input axis p_i; flip_axis (-1 = none) reverses one INPUT
 * axis.  Conv1d weight layouts between the reference's [K,C,S], the forward kernel's [K,S,C], the data
 * gradient's flipped [C,S,K] and the weight gradient's [S,C,K]. */
int dlip_permute3_f32(const float* x, float* y, int32_t d0, int32_t d1, int32_t d2, int32_t p0, int32_t p1,
                      int32_t p2, int32_t flip_axis, dlip_stream_t stream);

/* scale2[0] = 2^floor(log2(target / max|x|)), scale2[1] = 1 / scale2[0] (device scalars; 1 if x == 0):
 * the power-of-two that lifts a gradient tensor into fp16's normal range before it is split. */
int dlip_pow2_scale_f32(const float* x, float* scale2, int64_t n, float target, dlip_stream_t stream);
/* The same into a DLIP_LIFT_WORDS buffer (layout above): lift[0] = 2^e, lift[1] = 2^-e, lift[2 .. 2049] = 2^-e. */
int dlip_pow2_lift_f32(const float* x, float* lift, int64_t n, float target, dlip_stream_t stream);
/* dlip_split_pack_f32 of x * scale[0] (device scalar). */
int dlip_split_pack_scaled_f32(const float* x, float* y, const float* scale, int64_t rows, int32_t C,
                               dlip_stream_t stream);
/* The same with each row zero-padded from C (a multiple of 4) to C_pad (a multiple of 32) channels: y [rows, C_pad]. */
int dlip_split_pack_scaled_pad_f32(const float* x, float* y, const float* scale, int64_t rows, int32_t C, int32_t C_pad,
                                   dlip_stream_t stream);
/* Split-fp16 operand image of a weight matrix on the device (what deeplip_amd.packing.split_weights builds on the host at load
 * time; a training step needs it from the CURRENT weights): w [K rows][L], L % 32 == 0 with every 32-channel block intact ->
 * w_split [K][L] (per block 32 hi halves | 32 lo halves of w * w_scale[k]), w_scale[k] = 2^floor(log2(1023 / max|w[k,:]|))
 * (1 for a zero row) -- the w_split / w_scale pair dlip_conv_nhwc_f16x3 takes. */
int dlip_split_weights_rows_f32(const float* w, float* w_split, float* w_scale, int32_t K, int32_t L, dlip_stream_t stream);
/* The same straight from the reference layout w [K, C, T] (T = R*S taps: nn.Conv2d / nn.Conv1d weights), permutation included:
 * mode 0 = the forward operand, K rows of [T][C]; mode 1 = the data-gradient operand, C rows of [T reversed][K] (the flipped,
 * transposed filter).  w_scale has one entry per output row; the row's inner channel count (C resp. K) must be a multiple of 32. */
int dlip_split_weights_perm_f32(const float* w_kct, float* w_split, float* w_scale, int32_t K, int32_t C, int32_t T, int32_t mode,
                                int32_t C_pad, dlip_stream_t stream);
/* C_pad (0 = none): the rows' inner channel count (C in mode 0, K in mode 1) zero-padded to C_pad -- a first layer whose input has
 * 24 feature channels reads its activations padded to 32; the data gradient of a 1500-channel layer reads its gradient padded
 * to 1504 (tdnn.py:52-62 on conf/audio_config.yaml's input_dim / hidden_dim). */
/* (round 4) dlip_split_weights_perm_f32 for MANY weight tensors in ONE launch -- a training step splits the current weights of every
 * convolution twice (forward and data-gradient operand): `descs` is a DEVICE array of dlip_wsplit_desc (one per output tensor),
 * `block_desc` a device int32[n_blocks] naming, for each output row of each tensor in order, its descriptor (row r of descriptor d is
 * block d.row0 + r).  Same result per row as the single-tensor call (mode, C_pad as there). */
typedef struct dlip_wsplit_desc {
  const float* w;       /* [K, C, T] reference layout */
  float* w_split;       /* mode 0: [K][T][C_pad]; mode 1: [C][T reversed][C_pad = K padded] */
  float* w_scale;       /* one per output row */
  int32_t K, C, T, C_pad, mode, row0;
} dlip_wsplit_desc;
/* (ABI 44) max_row_floats: the longest output row of the launch, T * C_pad floats (0: unknown) -- sizes the kernel's staging buffer
 * (dynamic LDS), so that a launch of short rows keeps more workgroups on a CU. */
int dlip_split_weights_multi_f32(const void* descs, const int32_t* block_desc, int32_t n_blocks, int32_t max_row_floats,
                                 dlip_stream_t stream);
/* y[0:n] = src[0] (device scalar broadcast: the per-channel 1/scale vector of the weight-gradient GEMM). */
int dlip_fill_from_scalar_f32(const float* src, float* y, int32_t n, dlip_stream_t stream);

/* Additive angular margin on cosine logits (ArcFace / AAM-softmax: named by the north star; `AAMSoftmax` is an
 * empty stub upstream, models/audio_models/loss.py:62-67 -- parity unpinned, the published recipe is restated):
 * backward == 0: y = logits with the target column cos(theta) replaced by cos(theta + margin) (where cos > cos(pi - m),
 * else cos - m sin(pi - m); easy_margin: only where cos > 0); backward != 0: y = g * d(modified)/d(logits).
 * logits, g, y [B,K]; labels int64 [B]. */
int dlip_aam_margin_f32(const float* logits, const int64_t* labels, const float* g, float* y, int32_t B, int32_t K,
                        float margin, int32_t easy_margin, int32_t backward, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Train-mode kernels of the lip-clip encoder (deeplip_amd/csrc/video_train_ops.hip):
 * what sits around the implicit-GEMM convolutions when torch.autograd's work for Lipreading.forward under
 * model.train() (train_video.py:108-169; models/video_models/model.py:80-105, resnet.py:28-127,
 * tcn.py:28-116) is done by dlip_* launches (deeplip_amd/autograd_video.py).  All tensors NHWC fp32,
 * C % 4 == 0.
 * ------------------------------------------------------------------------------------------ */

/* Rows one filter tap reads: out[j*ldo + 0:C] = x[n, ho*stride_h + off_h, wo*stride_w + off_w, 0:C] (zeros outside
 * the image), j = (n*Ho + ho)*Wo + wo; off = tap * dilation - padding.  With out = base + tap*C and
 * ldo = taps*C the taps land side by side in one [J, taps*C] matrix: the operand of the weight-gradient GEMM
 * of a padded / strided Conv2d / Conv1d (resnet.py:9-16, tcn.py:39-41). */
int dlip_tap_gather_f32(const float* x, float* out, int64_t N, int32_t H, int32_t W, int32_t C, int32_t ldx,
                        int32_t Ho, int32_t Wo, int32_t stride_h, int32_t stride_w, int32_t off_h, int32_t off_w,
                        int32_t ldo, dlip_stream_t stream);

/* One operand of the weight-gradient GEMM of a Conv2d / Conv1d in ONE pass (replaces dlip_tap_gather_f32 + dlip_nct_to_ntc_f32 +
 * dlip_split_pack*_f32 on a matrix R*S times the activation): out is [R*S*C rows][ld_out] floats in the split activation format ALONG
 * THE REDUCTION -- row (tap, c) holds scale * x[n, ho*stride_h + r*dil_h - pad_h, wo*stride_w + s*dil_w - pad_w, c] for j = (n*Ho +
 * ho)*Wo + wo = 0 .. J-1 (zeros outside the image and for j in J .. ld_out-1), 32 consecutive j per 128-byte block (32 hi halves |
 * 32 lo halves).  ld_out: row pitch in floats, a multiple of 32, >= J (an ODD number of 128-byte blocks keeps the rows of a slice
 * off one memory channel).  R = S = 1, no padding, scale = the power-of-two lift of dlip_pow2_scale_f32: the dy operand.
 * out 128-byte aligned; scale a device scalar or NULL (1).  x is [N,H,W,ldx] NHWC (Conv1d: H = 1). */
/* (round 4) The one-tap case with BOTH images of a [J, C] row matrix from ONE read: `out` as above (rows c, positions j along the
 * reduction) and `nhwc_split_out` [J, C] = the same values in the convolution kernels' split activation format (per row and 32
 * channels one 128-byte block) -- the forward convolution's operand of x, or (scale = the lift) the data gradient's of dy, which
 * dlip_split_pack*_f32 formed in a pass of its own.  C % 64 == 0; x 16-byte, both outputs 128-byte aligned. */
int dlip_wgrad_operand_split_f32(const float* x, float* out, int64_t ld_out, int64_t J, int32_t C, const float* scale,
                                 float* nhwc_split_out, dlip_stream_t stream);
int dlip_wgrad_operand_f32(const float* x, float* out, int64_t ld_out, int64_t N, int32_t H, int32_t W, int32_t C, int32_t ldx,
                           int32_t Ho, int32_t Wo, int32_t stride_h, int32_t stride_w, int32_t R, int32_t S, int32_t dil_h,
                           int32_t dil_w, int32_t pad_h, int32_t pad_w, const float* scale, dlip_stream_t stream);
/* Operand of a weight gradient RUN AS A CONVOLUTION: x [N,H,W,C] fp32 (row pitch ldx) -> out [C,H,W,N32] in the split format, the
 * images as the reduction's channels (N32 >= N, a multiple of 32; images beyond N are zeros), times *scale when scale != NULL
 * (the gradient's power-of-two lift).  With x' = this image of the layer input and g' = this image of dy,
 *   dW[c, r, s, k] = dlip_conv_nhwc_f16x3(x' as N = C images of H x W x N32, filter g' = [K, Ho, Wo, N32], stride = the layer's
 *                    dilation, dilation = the layer's stride, padding = the layer's) [c, r, s, k]        (r < R, s < S)
 * -- ONE copy of each tensor instead of the R*S shifted copies of dlip_wgrad_operand_f32; dlip_conv_nhwc_f16x3 accepts filters of
 * more than 32 taps for this (split input, fp32 output, no residual).  train_video.py:129-147 (loss.backward()). */
int dlip_wgrad_chwn_f32(const float* x, float* out, int64_t N, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t N32,
                        const float* scale, int32_t slice_major, float* nhwc_split_out, dlip_stream_t stream);
/* (ABI 44) The two producers above with a train-mode BatchNorm + (Leaky | P)ReLU applied ON LOAD: x is the RAW output z of the
 * previous convolution and every loaded value becomes act((z - mean) invstd gamma + beta) (slope_vec [C] per-channel slopes, or NULL:
 * the scalar `slope`) before it is split -- the convolution behind a conv -> BatchNorm -> activation (tdnn.py:35-43: the next
 * TDNN_Block; resnet.py:51-57: conv2 behind bn1 + relu1) needs its input only as these images, so the activated tensor is never
 * stored (one write and one read of an activation-sized tensor per layer).  Slice-major image layout; C % 64 == 0; the split NHWC
 * copy is mandatory (it is the forward convolution's operand). */
int dlip_wgrad_operand_split_bn_f32(const float* x, float* out, int64_t ld_out, int64_t J, int32_t C, const float* mean,
                                    const float* invstd, const float* gamma, const float* beta, const float* slope_vec, float slope,
                                    float* nhwc_split_out, dlip_stream_t stream);
int dlip_wgrad_chwn_bn_f32(const float* x, float* out, int64_t N, int32_t H, int32_t W, int32_t C, int32_t N32, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, const float* slope_vec, float slope,
                           float* nhwc_split_out, dlip_stream_t stream);
/* (ABI 47) The BACKWARD of a train-mode BatchNorm (+ LeakyReLU) applied ON LOAD, in two parts: (1) dlip_bn_rows_train_bwd_sums_f32 = the first
 * half of dlip_bn_rows_train_bwd_f32 -- dgamma, dbeta -- plus the power-of-two lift of a dx that is never written: from the largest |g| and
 * |xhat| the sums pass sees PER CHANNEL (ABI 50; amax_parts: 2 * C * (dlip_bn_rows_chunks(M) + 1) floats of scratch) and the finished sums,
 * the bound |dx| <= max_c |gamma_c invstd_c| (max|g_c| + |dbeta_c| / M + max|xhat_c| |dgamma_c| / M) is put at 1024 (a lift is exact: another
 * exponent, the same gradients; ABI 47 - 49 took the three maxima over all channels apart and could sit 2^18 above max|dx|); (2) the two operand
 * producers read dy and z and form dx = gamma invstd (g - dbeta / M - xhat dgamma / M) per loaded value (the apply pass's expression, the
 * same bits), times lift[0], straight into the weight gradient's image and the data gradient's split operand (nhwc_split_out, nullable).
 * The convolution in front of a BatchNorm (tdnn.py:35-43 under loss.backward(), train_audio.py:189-191) needs the BatchNorm's input
 * gradient only as these images: one write and one read of an activation-sized fp32 tensor per layer less.  C % 64 == 0. */
/* (ABI 48) MeanStdPooling (pooling.py:24-26) and its backward on the RAW output z of the last TDNN convolution, the train-mode BatchNorm +
 * LeakyReLU in front applied per loaded value (tdnn.py:35-43 -> :96 under model.train()): the activated [B,T,1500] tensor -- 460 MB at
 * B = 256 -- is never stored.  dx of the backward is the gradient with respect to the ACTIVATED values (the BatchNorm's backward follows). */
int dlip_meanstd_pool_bn_f32(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta, float slope,
                             float* y, int32_t B, int32_t T, int32_t C, dlip_stream_t stream);
int dlip_meanstd_pool_bwd_bn_f32(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta, float slope,
                                 const float* y, const float* dy, float* dx, int32_t B, int32_t T, int32_t C, dlip_stream_t stream);
/* (ABI 48) ... and the BatchNorm backward BEHIND that pooling with the pooling's backward formed on load: dy[b,t,c] = dmean / T + dstd (y - mean) /
 * ((T - 1) std) per loaded value from the pooled statistics y_pool [B,2C] and their gradient g_pool [B,2C] (y = the activated value the
 * BatchNorm backward recomputes anyway) -- the pooling's backward writes nothing (its [B,T,C] gradient was one write and two reads).  Otherwise
 * dlip_bn_rows_train_bwd_f32 (conv -> BatchNorm -> LeakyReLU order; M = B T > 4096 rows).  The gradient is A[b,c] + K[b,c] y: the two
 * coefficients per (utterance, channel) -- coef [B,2C] = (A | K) -- come from dlip_meanstd_bwd_coef_f32 (ABI 49), one launch over [B,2C]. */
int dlip_meanstd_bwd_coef_f32(const float* y_pool, const float* g_pool, float* coef, int32_t B, int32_t C, int32_t T, dlip_stream_t stream);
int dlip_bn_rows_train_bwd_ms_f32(const float* ms_coef, int32_t T, const float* x, const float* gamma, const float* beta, const float* save_mean,
                                  const float* save_invstd, float* dx, float* dgamma, float* dbeta, double* workspace, int32_t M, int32_t C,
                                  float slope, float* dx_lift2, dlip_stream_t stream);
int dlip_bn_rows_train_bwd_sums_f32(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                                    const float* save_invstd, float* dgamma, float* dbeta, double* workspace, float* amax_parts, int32_t M,
                                    int32_t C, float slope, int32_t act_first, float* dx_lift2, const float* ms_coef, int32_t ms_T,
                                    dlip_stream_t stream);
/* (ABI 49) both take ms_coef [B,2C] + ms_T (nullable: then as ABI 47): dy is itself formed on load from a MeanStdPooling's coefficients
 * (dlip_bn_rows_train_bwd_ms_f32's rule; dy may be NULL) -- the last TDNN layer's whole backward then reads z alone.  The operand
 * producer also takes a channel count that is no multiple of 64 (C % 4 == 0: the E-TDNN's 1 500) and the row pitch ld_nhwc of its split copy
 * (0 = C; else >= C, a multiple of 32, the padding channels written as zeros). */
int dlip_wgrad_operand_split_bnbwd_f32(const float* dy, const float* z, float* out, int64_t ld_out, int64_t J, int32_t C, const float* mean,
                                       const float* invstd, const float* gamma, const float* beta, const float* dgamma, const float* dbeta,
                                       int64_t M, float slope, int32_t act_first, const float* lift, float* nhwc_split_out, int32_t ld_nhwc,
                                       const float* ms_coef, int32_t ms_T, dlip_stream_t stream);
int dlip_wgrad_chwn_bnbwd_f32(const float* dy, const float* z, float* out, int64_t N, int32_t H, int32_t W, int32_t C, int32_t N32,
                              const float* mean, const float* invstd, const float* gamma, const float* beta, const float* dgamma,
                              const float* dbeta, int64_t M, float slope, int32_t act_first, const float* lift, float* nhwc_split_out,
                              dlip_stream_t stream);
/* nhwc_split_out (nullable; C % 32 == 0): the same tensor (scaled alike) ALSO in the convolution kernels' split activation format
 * [N,H,W,C] -- what dlip_split_pack_f32 / dlip_split_pack_scaled_f32 would write -- from the one read: the forward convolution's
 * operand together with the weight gradient's (x), the data gradient's together with the weight gradient's (dy). */
/* slice_major != 0: the image as [C][N32/32][H][W][32] instead -- one 32-image slice of all pixels of a channel is ONE contiguous
 * plane, so that the filter taps a convolution walks one after the other are adjacent 128-byte lines (pixel-major they are
 * N32 * 4 bytes apart: every piece a DRAM page of its own).  That is the layout dlip_wgrad_conv_f16x3 reads:
 *   dw [C, R', S', K] fp32 = sum over images and output positions, x_img = the layer input's image, g_img = the output gradient's
 *   (lifted), R' = (H + 2 pad - stride (Ho - 1) - 1) / dil + 1 >= R (dW sits in [:, :R, :S, :]); post_scale / post_shift [K]: the
 *   epilogue's affine (2^-e of the lift, 0); unit_scale [K]: ones (the "filter" carries no per-channel scale).
 * stride / pad / dil are the LAYER's. */
int dlip_wgrad_conv_f16x3(const float* x_img, const float* g_img, const float* post_scale, const float* post_shift,
                          const float* unit_scale, float* dw, int32_t C, int32_t H, int32_t W, int32_t K, int32_t Ho, int32_t Wo,
                          int32_t N32, int32_t stride_h, int32_t stride_w, int32_t pad_h, int32_t pad_w, int32_t dil_h, int32_t dil_w,
                          int32_t R, int32_t S, dlip_stream_t stream);
/* R, S (ABI 43; 0, 0 = dw [C, R', S', K] as above): the LAYER's filter extent -- dw is then written in the REFERENCE layout
 * [K, C, R, S] (what Conv2d.weight.grad is: models/video_models/resnet.py:9-16), the positions r' >= R / s' >= S dropped, by the
 * epilogue itself: no [C, R', S', K] tensor, no slice copy and no permute launch behind it (48 launches of a training step). */
/* The stem's input for its weight gradient run as a convolution: the clip x [B,T,H,W] -> out [5][H][W][N32] split format, n = b*T + t,
 * out[dt][h][w][n] = x[b, t + dt - 2, h, w] (zero outside the clip; N32 >= B*T, a multiple of 32): the five temporal taps of
 * Conv3d(1,64,(5,7,7),(1,2,2),(2,3,3)) (model.py:82) as five "images" of ONE 2-D convolution whose filter is the output gradient
 * (dlip_wgrad_chwn_f32 of dy: [64][H/2][W/2][N32]; stride 1, dilation 2, padding 3): dW[k, dt, r, s] = its output [dt, r, s, k]. */
int dlip_stem_wgrad_chwn_f32(const float* x, float* out, int32_t B, int32_t T, int32_t H, int32_t W, int32_t N32, int32_t slice_major,
                             dlip_stream_t stream);
/* out [N,Hu,Wu,C] = dz [N,Ho,Wo,C] with stride-1 zeros inserted (out[n, ho*s, wo*s] = dz[n, ho, wo]): the data
 * gradient of a strided convolution as a stride-1 convolution (resnet.py:9-16 with stride 2). */
int dlip_upsample_zero_f32(const float* dz, float* out, int64_t N, int32_t Ho, int32_t Wo, int32_t Hu, int32_t Wu,
                           int32_t C, int32_t stride_h, int32_t stride_w, dlip_stream_t stream);
/* (ABI 44) The same zero insertion written straight as the lifted split operand of the data-gradient convolution: out_split =
 * dlip_split_pack_scaled_f32(dlip_upsample_zero_f32(dz), scale) without the fp32 tensor in between (C % 32 == 0). */
int dlip_upsample_zero_split_f32(const float* dz, float* out_split, const float* scale, int64_t N, int32_t Ho, int32_t Wo, int32_t Hu,
                                 int32_t Wu, int32_t C, int32_t stride_h, int32_t stride_w, dlip_stream_t stream);
/* nn.PReLU(C) on rows [M,C] (resnet.py:52,66; model.py:84; tcn.py:47,105): y = x >= 0 ? x : slope[c] * x. */
int dlip_prelu_rows_fwd_f32(const float* x, const float* slope, float* y, int64_t M, int32_t C, dlip_stream_t stream);
/* Backward: dx, and dslope_terms [M,C] = (x < 0 ? dy * x : 0) whose column sums (dlip_colsum_rows_f32) are
 * the slope gradient. */
int dlip_prelu_rows_bwd_f32(const float* dy, const float* x, const float* slope, float* dx, float* dslope_terms,
                            int64_t M, int32_t C, dlip_stream_t stream);
/* The end of a residual block in one pass (resnet.py:66-68, tcn.py:114): sum = a + b (the pre-activation dlip_prelu_rows_bwd_f32
 * needs), y = prelu(sum) with per-channel slopes; a, b, sum, y [M,C]. */
int dlip_add_prelu_rows_fwd_f32(const float* a, const float* b, const float* slope, float* sum, float* y, int64_t M, int32_t C,
                                dlip_stream_t stream);
/* MaxPool3d((1,3,3),(1,2,2),(0,1,1)) backward (model.py:85): x [N,H,W,C] = the pooled tensor's input,
 * dy [N,Ho,Wo,C] -> dx; first-maximum tie rule (row-major window scan), deterministic. */
int dlip_maxpool3x3s2_bwd_f32(const float* x, const float* dy, float* dx, int64_t N, int32_t H, int32_t W, int32_t C,
                              dlip_stream_t stream);
/* The training pair that does not re-scan x: the forward also writes, per output element, the tap (r*3+s) of its first maximum
 * as one byte (idx: N*Ho*Wo*C bytes, 4 channels per 32-bit word), the backward reads at most four (byte, dy) pairs per input
 * pixel.  y is bit-identical to dlip_maxpool3x3s2_f32, dx to dlip_maxpool3x3s2_bwd_f32. */
int dlip_maxpool3x3s2_idx_f32(const float* x, float* y, uint32_t* idx, int64_t N, int32_t H, int32_t W, int32_t C, dlip_stream_t stream);
int dlip_maxpool3x3s2_bwd_idx_f32(const uint32_t* idx, const float* dy, float* dx, int64_t N, int32_t H, int32_t W, int32_t C,
                                  dlip_stream_t stream);
/* dx[n, p, :] = dy[n, :] * w, p < P: w = scale (AdaptiveAvgPool2d(1) backward, resnet.py:83: scale = 1/(H W)),
 * or with lengths != NULL w = (p < len[n] ? 1/len[n] : 0) (masked temporal mean backward, model.py:16-17). */
int dlip_row_broadcast_f32(const float* dy, const int32_t* lengths, float* dx, int64_t N, int32_t P, int32_t C,
                           float scale, dlip_stream_t stream);
/* im2col of the stem Conv3d(1,64,(5,7,7),(1,2,2),(2,3,3)) (model.py:82): x [B,T,H,W] -> col [B*T*(H/2)*(W/2), 248]
 * (245 taps + 3 zero columns), the operand of the stem's weight-gradient GEMM. */
int dlip_stem_im2col_f32(const float* x, float* col, int32_t B, int32_t T, int32_t H, int32_t W, dlip_stream_t stream);
/* The same operand WITHOUT the im2col round trip: out [248, ld_out] = the reduction-major split image the weight-gradient GEMM
 * reads (per row and 32 positions one 128-B block: 32 hi halves | 32 lo halves; positions >= J and rows 245..247 zero), written
 * in one pass from the clip x [B,T,H,W].  ld_out >= B*T*(H/2)*(W/2), a multiple of 32; out 128-B aligned.  Reports range like
 * the other split producers.  (train_video.py:129-147: the stem's weight gradient.) */
int dlip_stem_wgrad_operand_f32(const float* x, float* out, int64_t ld_out, int32_t B, int32_t T, int32_t H, int32_t W,
                                dlip_stream_t stream);
/* The stem's CURRENT weights w [K,245] (= [K,1,5,7,7]) -> the split-fp16 weight image of dlip_stem3d_bn_act_f16x3 /
 * dlip_stem3d_pool_f16x3 (K x 1184 B) and its per-channel power-of-two scale [K], on the device: what a training step needs
 * every iteration (the extraction path packs once on the host). */
int dlip_split_stem_weights_f32(const float* w, float* w_img, float* w_scale, int32_t K, dlip_stream_t stream);
/* (ABI 44) nn.Dropout (tcn.py:80,85) with the keep test in the kernel: y = u >= p ? x * scale : 0, u = the uniform draws (the
 * backward applies the same launch to dy with the kept u).  Replaces compare + cast + dlip_mul_mask_f32 behind the generator. */
int dlip_dropout_keep_f32(const float* x, const float* u, float* y, int64_t n, float p, float scale, dlip_stream_t stream);
/* (ABI 44) The end of a multibranch TCN stage in one launch: symmetric chomp (tcn.py:52-59) + concatenation along channels
 * (tcn.py:96-108) of n_branches <= 4 tensors z_j [B, lengths[j], widths[j]] (HOST arrays of pointers / sizes; lengths[j] - T even,
 * widths multiples of 4): cat[b, t, off_j + c] = z_j[b, t + (lengths[j] - T) / 2, c].  backward != 0: the reverse -- `branches` are
 * written from cat (= the gradient of the concatenation), zeros in the chomped rows. */
int dlip_chomp_concat_f32(DLIP_HOST const float* const* branches, DLIP_HOST const int32_t* lengths, DLIP_HOST const int32_t* widths,
                          int32_t n_branches, float* cat, int32_t B, int32_t T, int32_t backward, dlip_stream_t stream);
/* y = x * mask * scale (nn.Dropout forward / backward, tcn.py:80,85). */
int dlip_mul_mask_f32(const float* x, const float* mask, float* y, int64_t n, float scale, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Range status of the split-fp16 ("f16x3") arithmetic.  The reference computes in fp32 end to end
 * (models/video_models/model.py:82-85); the split activation format stores a value as hi + lo fp16, so a value
 * of magnitude >= 65520 becomes infinite.  Every kernel that PRODUCES split-format values (conv epilogues with
 * DLIP_SPLIT_OUT, dlip_split_pack*_f32, the fused stem + pool, pooling with out_split) stores 1 into its word of
 * a caller-owned status block when it meets such a value; the host reads the words (device memory after a
 * synchronisation, or host-pinned device-visible memory at any time), raises, and the documented recourse is to
 * re-pack that model in the exact "f32" mode (same engine).  words = int32[8] {conv, stem, split_pack, pooling, low side (below),
 * 3 reserved}, zeroed by the caller; NULL unregisters (nothing is reported).  One block per process (one process per GPU).
 * ------------------------------------------------------------------------------------------ */
enum { DLIP_ST_CONV = 0, DLIP_ST_STEM = 1, DLIP_ST_PACK = 2, DLIP_ST_POOL = 3, DLIP_ST_LOW = 4, DLIP_ST_COUNT = 8 };   /* the words */
int dlip_set_status_words(int32_t* words);
/* (ABI 45) A status block for the launches of the CALLING THREAD alone: until dlip_status_scope(NULL), every producer this thread
 * launches (and the verdict kernel of a range scope it closes) reports to `words` (int32[8], host-pinned and device-visible, or
 * device memory; zeroed by the caller) instead of the process-wide block.  The address is handed to the kernels per launch, so a step
 * plan recorded inside such a scope reports to ITS block on every replay: the host can tell WHICH recorded batch left the range
 * (deeplip_amd.pipeline: the offending batch is re-run on the exact "f32" pack of the same model, train_fusion.py:338-358 never
 * saw it) where the process-wide block only says that one of the launches since the last look did. */
int dlip_status_scope(int32_t* words);

/* The LOW side of that range.  hi keeps 11 significant bits down to 6.1e-5, but lo = v - hi is a normal fp16 number only while
 * |v| >= 2^-3; below, lo sits on the subnormal grid 2^-24: an absolute error of up to 3e-8 per element, whatever its size.  Measured
 * on a 3-layer chain of Gaussian activations the result is 5.9e-7 off at sigma 1, 2.8e-5 at sigma 1e-3 (largest element 4.5e-3),
 * 3.1e-2 at sigma 1e-6.  A checkpoint whose BatchNorm statistics put a whole layer's activations down there would lose
 * fp32-grade accuracy silently, so a produced tensor whose largest magnitude lies in (0, 2^-2) is reported -- word 4 of the
 * status block (int32[8]: {conv, stem, split_pack, pooling, LOW, 3 reserved}) receives the kernel family + 1 -- and the host
 * raises exactly as for an overflow (same recourse: "f32" packing).
 * Per-launch evidence needs a word per launch: between dlip_range_scope_begin and dlip_range_scope_end (thread-local, may
 * nest: the outermost pair counts) every producer launched by this thread takes the next 1024 words (32 cache lines: its waves
 * spread over them, so that thousands finishing together do not queue at one line) of `slots` (device int32[1024 n], zeroed once
 * by the caller; flags, not counters: plain stores, no read-modify-write); _end launches a one-block verdict kernel on `stream` -- which must be ordered behind every launch
 * of the scope (join side streams first) -- that reports and re-zeroes the words.  Recorded into a step plan the verdict is
 * part of every replay.  Outside a scope the low side is not guarded (the high side always is).  A scope with more producers than
 * slots ends with DLIP_ERANGE (the launches beyond n ran unguarded: never quietly).  Launches that split TWO tensors take two slots
 * (the stem + pool entry point: one for the clip its pre-pass splits, one for the pooled output). */
/* Span scope (measurement): what a replayed step plan cannot give the host -- no event recorded into a graph can be read back --
 * the kernel notes itself.  Between _begin and _end (thread-local, not nestable) every launch of an MFMA kernel on split-format
 * input (the LDS-DMA ring kernel behind dlip_conv_nhwc_f16x3 / dlip_conv2_nhwc_f16x3 / dlip_conv_pool_f16x3, the window kernel, the
 * rows kernel, the stem + pool kernel together with its pre-pass) takes the next RECORD of `pairs` (device uint64[16 n]: word 0 =
 * start, armed as ~0; words 8..15 = end, armed as 0, one per blockIdx.x % 8 so that a grid's workgroups do not queue at one word;
 * a record is one 128-byte line); its workgroups fold the constant 100 MHz clock (s_memrealtime) into it -- every 16th the minimum at
 * entry (a grid starts within a microsecond), EVERY one the maximum at exit.  _end launches a collect kernel on `stream` (order it
 * behind the scope's launches) that adds max(end) - start and 1 into acc[2 i], acc[2 i + 1] (device uint64[2 n], zeroed by the
 * caller) and re-arms the record -- recorded into a plan, every replay accumulates; *used = records taken.  Outside a scope the
 * kernels time nothing. */
int dlip_span_scope_begin(uint64_t* pairs, uint64_t* acc, int32_t n);
int dlip_span_scope_end(dlip_stream_t stream, DLIP_HOST int32_t* used);

#define DLIP_EVID_WORDS 1024                     /* int32 words of low-side evidence per launch: */
#define DLIP_EVID_LINES (DLIP_EVID_WORDS / 32)   /* 32 cache lines of 128 B */
int dlip_range_scope_begin(int32_t* slots, int32_t n);
int dlip_range_scope_end(dlip_stream_t stream);

/* Diagnostic overrides for tests and A/B runs (the launch path reads no environment variable):
 * key 0 tile of dlip_conv_nhwc_f32 / the register-staged f16x3 kernel, 1 tile of the LDS-DMA kernel,
 * 2 LDS-DMA kernel on/off (0 = off), 3 balanced split (0 never, 2 always), 4 window kernel on/off (0 = off),
 * 5 tile order of the LDS-DMA kernel (0 column block outer, 1 inner, 2 the column blocks as lanes of the balanced split: the blocks
 * of a row range on neighbouring workgroups at the same time -- built in for layer 3's two-block launches), 6 rows kernel (conv_rows_f16x3.hip: 0 = off, 1 = on for
 * every launch of its shape class whatever the size, 3 | 4 | 5 = on with that tile height in units of 32 rows),
 * 7 reserved (it forced the rows kernel's general mode, a retired experiment, EXPERIMENTS.md R8.2: DLIP_EINVAL for a value > 0, -1 / 0 are accepted);
 * key 3 also takes 3 (experiment: slabs of same-XCD tiles through
 * that XCD's L2) and 4 (the in-kernel finisher where the built-in choice is the reduce launch);
 * 8 the train-mode BatchNorm / column-sum entry points' launch sequence (0 = ABI 43's: statistics, finalize, apply [, lift] as separate
 * launches; otherwise the finalize steps run in the last workgroup of the pass before them and few-row tensors take one launch);
 * 9 the rows kernel's short last round (0 = off: every tile the full height);
 * 10 the LDS-DMA kernel's border groups (a padded convolution on the 256 x 128 tile run as its padding-free sub-convolutions in one
 * launch: 0 = never, 1 = whenever the construction applies; built in where a launch's share of padding taps is large enough);
 * 11 the segment boundary of the LDS-DMA kernel's 256 x 128 tile with split-format output (0 = the output tile staged in LDS, then
 * the next tile's set-up and ring fill; 1 = the epilogue straight from the accumulators; 2 = ... and the next tile's first slices
 * issued in front of it);
 * value -1 restores the built-in choice. */
enum { DLIP_DBG_CONV_TILE = 0, DLIP_DBG_DMA_TILE = 1, DLIP_DBG_DMA_ENABLE = 2, DLIP_DBG_STREAMK = 3, DLIP_DBG_WIN = 4, DLIP_DBG_NINNER = 5,
       DLIP_DBG_ROWS = 6, DLIP_DBG_ROWS2D = 7, DLIP_DBG_BN_FUSED = 8, DLIP_DBG_ROWS_TAIL = 9, DLIP_DBG_GROUPED = 10, DLIP_DBG_RING_HEAD = 11,
       DLIP_DBG_COUNT = 12 };
int dlip_debug_set(int32_t key, int32_t value);

/* ------------------------------------------------------------------------------------------
 * ShuffleNetV2 lip-clip trunk, eval mode, exact fp32 (Lipreading(backbone_type='shufflenet'); deeplip_amd/shufflenet.py).
 *
 * dlip_shuffle_stem24_f32: Conv3d(1->24, 5x7x7, stride (1,2,2), pad (2,3,3)) + folded BatchNorm3d + PReLU|ReLU (slope[k]: PReLU
 * weight or 0; NULL = identity), replacing models/video_models/model.py:81-83 for frontend_nout = 24 (model.py:76).  x [B,T,H,W],
 * w = [248][32] k-major (245 taps + 3 zero rows; channels 24..31 zero), y [(B*T),H/2,W/2,24].  H, W even, W <= 128.
 *
 * dlip_shuffle_dwpw_f32: one branch tail of an InvertedResidual unit (shufflenetv2.py:42-105):
 *   y = ReLU(W * A + bias), A = x (dw_w == NULL: plain 1x1) or A = dw3x3(x) + dw_b (pad 1, stride 1|2, groups = channels,
 *   no activation; computed on load and never stored), folded BatchNorms in both.  x [N,H,W,*] at pixel pitch ldx (Cin
 *   channels from the pointer on), dw_w [9][Cin] tap-major, dw_b [Cin], w [Cp][Kp] k-major (Cp = Cin rounded up to 32 with
 *   zero rows, Kp a multiple of 64 >= K), bias [K].  Output pixel m, channel j goes to y[m*ldy + j] (hp == 0) or, hp > 0, to
 *   the unit's shuffled position (channel_shuffle(cat(.,.), 2), shufflenetv2.py:27-40,96-105): logical channel L = 2j + par
 *   of the 2K-channel unit output, stored at L (L < K) or hp + L - K (L >= K), hp >= K the padded half, ldy >= 2hp; the launch with
 *   par == 1 also writes zeros to the padding channels [K, hp) and [hp + K, 2hp).  xp != NULL (stride 1, hp > 0): the
 *   passthrough half x1 (shufflenetv2.py:98-100) -- channel j < K of xp at pitch ldp goes to logical 2j + 1 - par.
 *   Cin, ldx multiples of 4; x, dw_w, dw_b 16-byte aligned.
 *
 * dlip_avgpool3_nhwc_f32: AvgPool2d(3) (stride 3, no padding; the `globalpool` of model.py:75 with input_size 96) of an
 * [N,H,W,C] map with 3 <= H, W <= 5 -- the one output pixel is the mean of the TOP-LEFT 3x3 window -- to y [N,C].
 * ------------------------------------------------------------------------------------------ */
int dlip_shuffle_stem24_f32(const float* x, const float* w_248x32, const float* bias, const float* slope, float* y,
                            int32_t B, int32_t T, int32_t H, int32_t W, dlip_stream_t stream);
int dlip_shuffle_dwpw_f32(const float* x, const float* dw_w, const float* dw_b, const float* w, const float* bias,
                          const float* xp, float* y, int32_t N, int32_t H, int32_t W, int32_t stride, int32_t Cin,
                          int32_t K, int32_t Kp, int32_t ldx, int32_t ldp, int32_t ldy, int32_t hp, int32_t par,
                          dlip_stream_t stream);
int dlip_avgpool3_nhwc_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 52) Depthwise dilated temporal convolution of the depthwise-separable TCN heads (tcn_dwpw): the grouped Conv1d
 * (groups = channels, bias=False) of models/video_models/tcn.py:33-34 (ConvBatchChompRelu, dwpw MS-TCN) and :158-159,169-170
 * (TemporalBlock), exact fp32.  Channels-last x [B,T,C] fp32, C % 4 == 0, 16-byte aligned tensors; weights tap-major [k][C].
 * One call serves 1 <= n <= 4 branches that read the same x (the kernel sizes of one dwpw MS-TCN stage); w, bias, slope, y, dz,
 * dw, k, pad, t_out are HOST arrays of n entries.  Branch r:
 *   z_r[b,t,c] = sum_j w_r[j,c] x[b, t - pad_r + j d, c] (zeros outside [0, T)),  t in [0, t_out_r).
 * Eval (deeplip_amd.video): pad = (k-1)d/2, t_out = T (the symmetric chomp folded into "same" padding), the BatchNorm folded into
 * w and bias, y = act(z + bias) with slope[c] the PReLU weight or 0 (ReLU); bias / slope NULL (or a NULL entry) = none.
 * Train: pad = (k-1)d, t_out = T + (k-1)d, raw z (tcn.py:35-38: the BatchNorm's batch statistics cover the padded length).
 *
 * dlip_tcn_dw_dgrad_f32: dx[b,s,c] = sum_r sum_j w_r[j,c] dz_r[b, s + pad_r - j d, c] (zeros outside [0, t_out_r)); every branch's
 *   gradient summed into one dx [B,T,C] in a fixed order.
 * dlip_tcn_dw_wgrad_f32: dw_r[j,c] = sum_{b,t} dz_r[b,t,c] x[b, t - pad_r + j d, c]: fp64 partial sums over chunks of rows, then a
 *   fixed-order fp64 sum of the chunks rounded once to fp32 -- two launches, no atomics, the same bits on every run.  workspace:
 *   sum_r dlip_tcn_dw_wgrad_chunks(B * t_out_r) * k_r * C doubles (workspace_len = its size in doubles).
 * ------------------------------------------------------------------------------------------ */
int dlip_tcn_dw_fwd_f32(const float* x, int32_t n, DLIP_HOST const float* const* w, DLIP_HOST const float* const* bias,
                        DLIP_HOST const float* const* slope, DLIP_HOST float* const* y, DLIP_HOST const int32_t* k,
                        DLIP_HOST const int32_t* pad, DLIP_HOST const int32_t* t_out, int32_t B, int32_t T, int32_t C, int32_t d,
                        dlip_stream_t stream);
int dlip_tcn_dw_dgrad_f32(DLIP_HOST const float* const* dz, int32_t n, DLIP_HOST const float* const* w, DLIP_HOST const int32_t* k,
                          DLIP_HOST const int32_t* pad, DLIP_HOST const int32_t* t_out, float* dx, int32_t B, int32_t T, int32_t C,
                          int32_t d, dlip_stream_t stream);
int dlip_tcn_dw_wgrad_chunks(int32_t rows);
int dlip_tcn_dw_wgrad_f32(const float* x, int32_t n, DLIP_HOST const float* const* dz, DLIP_HOST float* const* dw,
                          DLIP_HOST const int32_t* k, DLIP_HOST const int32_t* pad, DLIP_HOST const int32_t* t_out, int32_t B, int32_t T,
                          int32_t C, int32_t d, double* workspace, int64_t workspace_len, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 53) Online triplet loss with negative mining on the device: OnlineTriplet (models/audio_models/loss.py:18-31) and the
 * triplet selectors (models/audio_models/utils.py:18-142: FunctionNegativeTripletSelector.get_triplets copies the embeddings to
 * the host and runs one tensor index + one numpy call per anchor-positive pair; AllTripletSelector builds a Python list of every
 * triplet).  Exact fp32, x [B,E] row-major, 1 <= B <= 1024, E % 4 == 0, 16-byte aligned; labels device int32 [B].  Shapes depend on
 * B and E alone, nothing is read back, every sum has a fixed order (no float atomics): a replayed launch repeats the bits.
 * mode: 0 = all triplets, 1 = hardest negative, 2 = random hard negative, 3 = semi-hard negative.
 *
 * dlip_triplet_mine_f32 (replaces utils.py:89-113): g [B,B] = x x^T, the RAW dot products the reference mines on (utils.py:93),
 *   rownorm [B] = max(|x_i|, 1e-8) (F.cosine_similarity's clamp), and for mode != 0 the dense neg [B,B]: for an anchor-positive
 *   pair a < p of equal label, neg[a,p] = the chosen n of another label, by v_n = (g[a,n] + margin) - g[a,p]:
 *   hardest = argmax_n v_n (lowest index on ties) if that v > 0; random = candidate number floor(u[a,p] * count) in index order of
 *   {n : v_n > 0}; semi-hard = the same of {n : 0 < v_n < margin}; -1 where the set is empty and everywhere else.  u [B,B]: uniform
 *   draws in [0,1) (modes 2, 3; NULL otherwise).  mode 0 writes g and rownorm only (neg may be NULL).
 * dlip_triplet_loss_f32 (replaces loss.py:28-31): loss[0] = mean over the triplets of relu(cos(a,n) - cos(a,p) + margin), cos(i,j) =
 *   g[i,j] / (rownorm[i] rownorm[j]); n_triplets[0] = their number N.  N == 0: loss = 0 (the reference fails there, utils.py:114-118).
 *   Scratch the caller owns: rowsum [B] fp64, rowcnt [B]; wcount [B,B] = per anchor row the signed count of ACTIVE triplets
 *   (+1 per triplet in which column j is the negative, -1 per triplet in which it is the positive), kept for the backward pass.
 * dlip_triplet_loss_bwd_f32: dx [B,E] = gscale[0] * d loss / d x (gscale NULL = 1): with S = wcount + wcount^T (the transposed half is
 *   read, not scattered), M_ij = S_ij gscale / (N rownorm_i rownorm_j), M_ii = -sum_j M_ij g_ij / rownorm_i^2, dx = M x.  mw: scratch
 *   of B * (B rounded up to 16) floats, 16-byte aligned.  N == 0: dx = 0.
 * ------------------------------------------------------------------------------------------ */
int dlip_triplet_mine_f32(const float* x, const int32_t* labels, float margin, int32_t mode, const float* u, float* g,
                          float* rownorm, int32_t* neg, int32_t B, int32_t E, dlip_stream_t stream);
int dlip_triplet_loss_f32(const float* g, const float* rownorm, const int32_t* labels, const int32_t* neg, float margin,
                          int32_t mode, double* rowsum, int32_t* rowcnt, int32_t* wcount, float* loss, int32_t* n_triplets,
                          int32_t B, dlip_stream_t stream);
int dlip_triplet_loss_bwd_f32(const float* x, const float* g, const float* rownorm, const int32_t* wcount, const int32_t* n_triplets,
                              const float* gscale, float* mw, float* dx, int32_t B, int32_t E, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 54) Low-rank bilinear pooling, the product of deeplip_amd.fusion.BNBilinear (the head train_fusion.py:84 of the reference
 * names and LBP.py does not define; LBP.py:38-44 without the signed square root).  e1 [B,d1], e2 [B,d2], u [d1, k o], v [d2, k o],
 * all fp32 row-major and 16-byte aligned; d1 % 4 == 0, d2 % 4 == 0, any k >= 1, o >= 1, B >= 1.  Exact fp32 on the fp32 MFMA under
 * every arithmetic mode; every sum has a fixed order (no reduction split over workgroups, no float atomics): a replayed launch
 * repeats the bits.
 *
 * dlip_bilinear_pool_f32: z[b,j] = (1/k) sum_{i<k} P[b, j k + i] Q[b, j k + i] with P = e1 u, Q = e2 v, one launch.  p, q
 *   (both NULL, or both [B, k o]): P and Q are also written, for the backward pass.
 * dlip_bilinear_pool_bwd_w_f32: du [d1, k o] = e1^T dP, dv [d2, k o] = e2^T dQ, where dP[b,n] = dz[b, n / k] / k * q[b,n] and dQ
 *   likewise with p are formed on load.  One workgroup owns a 64-column stripe of both and reduces over B by itself.
 * dlip_bilinear_pool_bwd_x_f32: de1 [B,d1] = dP u^T, de2 [B,d2] = dQ v^T; either output may be NULL (not both).
 * dlip_bilinear_finish_f32: out[b,j] = z[b,j] / max(|z_b|_2, eps) * scale[j] + shift[j] on [B,o]: F.normalize followed by an
 *   eval-mode BatchNorm1d folded into scale and shift.
 * ------------------------------------------------------------------------------------------ */
int dlip_bilinear_pool_f32(const float* e1, const float* e2, const float* u, const float* v, float* z, float* p, float* q, int32_t B,
                           int32_t d1, int32_t d2, int32_t o, int32_t k, dlip_stream_t stream);
int dlip_bilinear_pool_bwd_w_f32(const float* e1, const float* e2, const float* p, const float* q, const float* dz, float* du, float* dv,
                                 int32_t B, int32_t d1, int32_t d2, int32_t o, int32_t k, dlip_stream_t stream);
int dlip_bilinear_pool_bwd_x_f32(const float* p, const float* q, const float* dz, const float* u, const float* v, float* de1, float* de2,
                                 int32_t B, int32_t d1, int32_t d2, int32_t o, int32_t k, dlip_stream_t stream);
int dlip_bilinear_finish_f32(const float* z, const float* scale, const float* shift, float* out, int32_t B, int32_t o, float eps,
                             dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 55) Compact bilinear pooling, `CompactBilinearPooling(embedding_dim, embedding_dim, 512)`: the fusion head train_fusion.py:31-32,83
 * of the reference imports and builds, and whose source upstream no longer ships (deeplip_amd.fusion.CompactBilinearPooling).  x1
 * [B,C1,P], x2 [B,C2,P]: contiguous NCHW with P = H W positions, read with stride P (no permuted copy).  A count sketch is given as
 * index lists, never as the dense [C,D] matrix: h[i] in [0,D) and s[i] = +-1 per input channel, and the same sorted by bin (CSR):
 * rowptr [D+1], idx [C] (ascending within a bin) and sgn [C] = s[idx].  1 <= D <= 4096.  Exact fp32 on the vector ALUs under every
 * arithmetic mode, every sum in a fixed order, no float atomics: a replayed launch repeats the bits.
 *
 * dlip_compact_bilinear_f32 (train_fusion.py:31-32,83): psi1[k] = sum_{h1[i] = k} s1[i] x1[i], psi2 likewise, and
 *   cbp[k] = D sum_m psi1[m] psi2[(k - m) mod D] per (sample, position), which is irfft(rfft(psi1) rfft(psi2)) D.  sum_pool != 0:
 *   out [B,D] is the sum over positions (ascending); else out [B,P,D].  psi1, psi2 (both NULL, or both [B,P,D]): the sketches are also
 *   written, for the backward pass.  One launch.
 * dlip_compact_bilinear_bwd_f32 (train_fusion.py:31-32,83; loss.backward(), :298): dpsi1[m] = D sum_k g[k] psi2[(k - m) mod D],
 *   dx1[i] = s1[i] dpsi1[h1[i]] written as [B,C1,P]; dx2 likewise with psi1.  g is [B,D] (sum_pool != 0: it serves every position)
 *   or [B,P,D].  Either output may be NULL; with both NULL nothing is launched.
 * ------------------------------------------------------------------------------------------ */
int dlip_compact_bilinear_f32(const float* x1, const float* x2, const int32_t* rowptr1, const int32_t* idx1, const float* sgn1,
                              const int32_t* rowptr2, const int32_t* idx2, const float* sgn2, float* out, float* psi1, float* psi2,
                              int32_t B, int32_t C1, int32_t C2, int32_t P, int32_t D, int32_t sum_pool, dlip_stream_t stream);
int dlip_compact_bilinear_bwd_f32(const float* g, const float* psi1, const float* psi2, const int32_t* h1, const float* s1,
                                  const int32_t* h2, const float* s2, float* dx1, float* dx2, int32_t B, int32_t C1, int32_t C2, int32_t P,
                                  int32_t D, int32_t sum_pool, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 56) Ragged batches through the ResNet speech encoder (`arch: resnet`, deeplip_amd/audio_resnet.py): a zero-padded batch of
 * utterances of differing length, every row computed as if run alone -- what replaces the one-utterance loop of train_audio.py:343-373
 * (batch 1, one launch sequence per utterance) for that encoder.  x is NHWC [N,H,W,C] with H = frequency and W = time; `lengths`
 * (device int32 [N]) holds the INPUT lengths in frames and `shift` the number of stride-2 stages in front of x, so utterance n is
 * valid for its first Lk = ((clamp(lengths[n], 1, W << shift) - 1) >> shift) + 1 frames of W (a stride-2 3x3 convolution with padding 1
 * maps L frames to (L - 1) / 2 + 1).  0 <= shift <= 16, C % 4 == 0, x 16-byte aligned.
 *
 * dlip_time_tail_zero_f32 (train_audio.py:343-373, arch resnet): in place, x[n, h, w >= Lk, :] = +0 -- the frames past an utterance's
 *   end, which a convolution's epilogue fills with its BatchNorm shift, neighbour spill and the residual, made the zeros the next
 *   zero-padded convolution reads when the utterance is run alone.  Store-only (x is never read: the traffic is the padding share of
 *   the tensor); all-zero bits, the zero of the fp32 container and of the split activation format alike.  The grid is N H whatever
 *   the lengths hold: a recorded plan replays with a new vector.
 * dlip_avgpool_time_ragged_f32 (train_audio.py:343-373, arch resnet: AdaptiveAvgPool2d(1) of each utterance at its own length):
 *   y[n, c] = sum_{h < H, w < Lk} x[n,h,w,c] / (H Lk), fp64 sums in a fixed order, no atomics.  x fp32 (not split), y [N,C]; N <= 65535.
 * ------------------------------------------------------------------------------------------ */
int dlip_time_tail_zero_f32(float* x, const int32_t* lengths, int32_t shift, int32_t N, int32_t H, int32_t W, int32_t C,
                            dlip_stream_t stream);
int dlip_avgpool_time_ragged_f32(const float* x, const int32_t* lengths, int32_t shift, float* y, int32_t N, int32_t H, int32_t W,
                                 int32_t C, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 57) RAGGED BATCHES through the audio front-end: a zero-padded batch of WAVEFORMS x [B,S] + one sample count per row, every row
 * computed as if it had been run alone -- what replaces calling the front-end once per utterance at batch 1 (the reference's loop,
 * train_fusion.py:334-349, train_audio.py:343-373) in front of the ragged encoders above.  sample_len (device int32 [B]) is clamped
 * to [1, S] by every kernel that reads it and never read on the host: a recorded plan replays with a new vector.  With
 * S_b = clamp(sample_len[b], 1, S) and NF_b = 1 if S_b <= frame_len else 1 + ceil((S_b - frame_len) / frame_step) (sigproc.framesig):
 *
 * dlip_wave_frame_lengths_i32: frame_lengths[b] = NF_b, on the device -- the length vector the ragged CMVN / delta kernels below and
 *   the encoders (dlip_conv_pool_f16x3's group_len, dlip_time_tail_zero_f32) read.
 * dlip_frame_preemph_ragged_f32 / dlip_powspec_wave_fft64_ragged_f32: the rectangular entry points with the row ending at S_b.  Frame
 *   f < NF_b is computed from samples < S_b exactly as the rectangular kernel computes it for an S_b-sample signal; samples >= S_b
 *   read as zero AFTER the pre-emphasis (sigproc.preemphasis runs on the S_b-sample signal, framesig zero-pads its result: position
 *   S_b holds 0, not -preemph * x[S_b - 1]) and are never loaded, so the caller's padding may hold anything.  Frames f >= NF_b: all
 *   zero (frames), resp. no FFT, a zero power-spectrum row and energy 0 -- finite input for the dense mel / log / DCT products.
 * dlip_cmvn_nct_ragged_f32: mean and population standard deviation over the row's own NF_b frames (summed in frame order by one
 *   thread in fp64: the order depends on NF_b alone, not on the neighbours or on NF; no atomics), (x - mean) / (std + 2e-12)
 *   (datasets.py:52-53); NF_b = 1 gives zeros as numpy does; columns t >= NF_b are written as exact zeros.
 * dlip_delta_nct_ragged_f32: python_speech_features.delta's edge padding repeats the row's own last valid frame NF_b - 1; columns
 *   t >= NF_b are zeros in all 1 + order blocks.
 * frame_lengths (device int32 [B]) is clamped to [1, NF].  Full lengths give the rectangular entry points' results bit for bit.
 * ------------------------------------------------------------------------------------------ */
int dlip_wave_frame_lengths_i32(const int32_t* sample_len, int32_t* frame_lengths, int32_t B, int64_t S, int32_t frame_len,
                                int32_t frame_step, dlip_stream_t stream);
int dlip_frame_preemph_ragged_f32(const float* x, const int32_t* sample_len, float* frames, int32_t B, int32_t S, int32_t NF,
                                  int32_t frame_len, int32_t frame_step, int32_t nfft, float preemph, dlip_stream_t stream);
int dlip_powspec_wave_fft64_ragged_f32(const float* x, const int32_t* sample_len, float* pw, float* energy, int64_t B, int64_t S,
                                       int32_t NF, int32_t frame_len, int32_t frame_step, int32_t nfft, double preemph, int32_t NB,
                                       int32_t NBp, dlip_stream_t stream);
int dlip_cmvn_nct_ragged_f32(const float* feat, const float* energy, const int32_t* frame_lengths, float* y, int32_t B, int32_t NF,
                             int32_t C, int32_t ldf, int32_t normalize, dlip_stream_t stream);
int dlip_delta_nct_ragged_f32(const float* x, const int32_t* frame_lengths, float* y, int32_t B, int32_t C, int32_t NF, int32_t order,
                              dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 59) STATISTICS AND ATTENTIVE POOLING of the ResNet speech encoder (`arch: resnet`, `pooling: statistic | attentive_statistic`;
 * conf/audio_config.yaml:102 names the key, no source ships upstream: deeplip_amd/audio_resnet.py and DESIGN.md 4b are the
 * definition).  x is the trunk's last map, NHWC [N,H,W,C] fp32 with H = frequency and W = time; the pooled feature index is
 * j = h C + c (the channels-last flatten), D = H C.  `lengths` / `shift` as in the ABI 56 block: utterance n is valid for its first
 * Wb = ((clamp(lengths[n], 1, W << shift) - 1) >> shift) + 1 frames; lengths == NULL: Wb = W.  The map is post-ReLU, so a feature
 * that is constant over time is ordinary: every standard deviation here carries eps > 0 UNDER the root, and the backward divides
 * by a std >= sqrt(eps).  C % 4 == 0, every tensor 16-byte aligned, no atomics, the same bits on every run.
 *
 * dlip_statpool_nhwc_f32 (pooling.py:24-26 on the map): y [N, 2D] = mean_j = sum_{w < Wb} x / Wb | std_j = sqrt(sum_{w < Wb}
 *   (x - mean)^2 / (Wb - 1) + eps), one pass over the map (no transposed or intermediate copy), fp64 sums in a fixed order.  The lengths
 *   are clamped on the device and never read on the host: a recorded plan replays with a new vector.  Frames w >= Wb are never
 *   loaded.  Wb == 1 gives std = sqrt(eps).  N, H <= 65535, 0 <= shift <= 16.
 * dlip_statpool_nhwc_bwd_f32: dx = dmean / W + dstd (x - mean) / ((W - 1) std) with mean and std read from y; every element of dx is
 *   written.  Rectangular batches only (a training batch is cropped to one length, datasets.py:112-115); W >= 2; eps > 0 is the
 *   forward's (the std in y holds it: the argument is checked, not used in the arithmetic).
 * dlip_swap_axes_nhwc_f32: y[n, b, a, :] = x[n, a, b, :] for x [N,A,B,C] -- the copy [N,H,W,C] -> [N,W,H C] that makes each frame's
 *   D-vector contiguous for the attentive pooling's hidden-layer GEMM; its backward is the same call with A and B exchanged.
 * dlip_time_valid_lengths_i32: valid[n] = Wb as above, on the device -- the frame counts the attentive pooling kernels take as `len`.
 * The attentive pooling itself (pooling.py:87-107 with std = sqrt(max(sum_t alpha x^2 - mean^2, 0) + eps)) is the dlip_mh_attn_* entry
 *   points below with n = 1 and this eps (ABI 67).
 * ------------------------------------------------------------------------------------------ */
int dlip_statpool_nhwc_f32(const float* x, const int32_t* lengths, int32_t shift, float eps, float* y, int32_t N, int32_t H, int32_t W,
                           int32_t C, dlip_stream_t stream);
int dlip_statpool_nhwc_bwd_f32(const float* x, const float* y, const float* dy, float eps, float* dx, int32_t N, int32_t H, int32_t W,
                               int32_t C, dlip_stream_t stream);
int dlip_swap_axes_nhwc_f32(const float* x, float* y, int32_t N, int32_t A, int32_t B, int32_t C, dlip_stream_t stream);
int dlip_time_valid_lengths_i32(const int32_t* lengths, int32_t shift, int32_t W, int32_t* valid, int32_t N, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 60) WAVEFORM AUGMENTATION in front of the audio front-end: what an x-vector recipe does to a training utterance before the
 * features are taken.  wave [B,S] fp32 + `lengths` (device int32 [B], nullable): row b holds n = clamp(lengths[b], 1, S) samples
 * (S when lengths == NULL) and is computed as if it were alone.  Every sum that decides a row's values (powers, mean, variance) is
 * taken in fp64 per tile of DLIP_FIR_TILE samples in a fixed order and the tiles are met front to back over the row's own
 * ceil(n / DLIP_FIR_TILE) tiles: no atomics, the same bits whatever B, S and the neighbours are.  Input samples t >= n are never
 * read; output samples t >= n are written as zeros.  Index and length vectors are clamped on the device and never read on the
 * host: a recorded plan replays with new vectors.  The three calls run in Kaldi's order (reverb, additive, normalise).
 *
 * dlip_wave_reverb_workspace_bytes: bytes of the caller-owned workspace the three calls below take (two doubles per row and tile;
 *   8-byte aligned; each call fills and reads it within its own launches, so one block serves them in turn); negative on bad sizes.
 * dlip_wave_reverb_f32 (train_audio.py:454: the 'reverb' kind of the training lists' augmentation, Kaldi's convolution with a room
 *   impulse response): rows with rir_idx[b] >= 0 (clamped to R - 1): h = rir[r, :len], len = clamp(rir_len[r], 1, Lmax), d =
 *   clamp(rir_peak[r], 0, len - 1) the tap of the direct path;  y[t] = sum_k h[k] x[t + d - k], 0 <= t < n, x zero outside [0, n) --
 *   as long as the input and aligned with it.  Exact fp32 (one fmaf per product, taps ascending) on the vector ALUs: a workgroup
 *   owns DLIP_FIR_TILE consecutive outputs of one row and walks the taps in chunks of DLIP_FIR_TAP_CHUNK, the tile's input window
 *   of each chunk staged in LDS.  keep_power != 0: y *= sqrt(Px / Py), P the mean square over [0, n), gain 1 when Py == 0 (a second
 *   launch).  Rows with rir_idx[b] < 0 pass through bit for bit.  rir [R, Lmax]; Lmax <= DLIP_FIR_MAX_TAPS, else DLIP_EINVAL;
 *   y must not be x; B <= 65535.
 * dlip_wave_add_noise_f32 (models/video_models/preprocess.py:150-179 AddNoise.__call__; train_audio.py:454 'music' / 'babble' /
 *   'noise'): rows with snr_db[b] < 9999: c = bank[st : st + n], st = clamp(noise_start[b], 0, bank_len - n) (an int64 vector: a
 *   noise corpus exceeds 2^31 samples);  z = y + c sqrt((Py / Pc) / 10^(snr_db[b] / 10)).  Rows at the sentinel 9999 pass through
 *   bit for bit, and so do rows whose slice has Pc == 0 (the reference divides by zero there).  Two launches.
 * dlip_wave_normalize_f32 (preprocess.py:141-147 NormalizeUtterance.__call__): (z - mean) / std with the population standard
 *   deviation of the row's n samples; std == 0 gives zeros (the reference divides by zero).  Two launches.
 * ------------------------------------------------------------------------------------------ */
#define DLIP_FIR_TILE 2048
#define DLIP_FIR_TAP_CHUNK 256
#define DLIP_FIR_MAX_TAPS 8192
int64_t dlip_wave_reverb_workspace_bytes(int64_t B, int64_t S);
int dlip_wave_reverb_f32(const float* x, const int32_t* lengths, const float* rir, const int32_t* rir_len, const int32_t* rir_peak,
                         const int32_t* rir_idx, float* y, void* workspace, int64_t workspace_bytes, int32_t B, int32_t S, int32_t R,
                         int32_t Lmax, int32_t keep_power, dlip_stream_t stream);
int dlip_wave_add_noise_f32(const float* y, const int32_t* lengths, const float* bank, int64_t bank_len, const int64_t* noise_start,
                            const float* snr_db, float* z, void* workspace, int64_t workspace_bytes, int32_t B, int32_t S,
                            dlip_stream_t stream);
int dlip_wave_normalize_f32(const float* z, const int32_t* lengths, float* out, void* workspace, int64_t workspace_bytes, int32_t B,
                            int32_t S, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 61) LOG-MAGNITUDE SPECTROGRAMS from the waveform: the loaders' fourth feature type, `stft` (models/audio_models/datasets.py:72-76:
 * librosa.stft(y, n_fft, hop_length, win_length) -> magphase -> log1p -> transpose; librosa's defaults center=True,
 * pad_mode="reflect", window="hann").  x [B,S] fp32; hop = int(rate * win_shift) and win = int(rate * win_len) TRUNCATE
 * (datasets.py:73), where the other three feature types round half up.  With lp = (n_fft - win) / 2 and the periodic Hann window
 * w[lp + k] = 0.5 - 0.5 cos(2 pi k / win), 0 <= k < win (zero elsewhere):
 *
 * dlip_stft_logmag_wave_f32 (models/audio_models/datasets.py:72-76): out[b NF + t, k] = log1p(|sum_j w[j] y[refl(t hop + j - n_fft / 2)]
 *   exp(-2 pi i j k / n_fft)|), k < F = n_fft / 2 + 1, NF = 1 + S / hop; refl reflects about 0 and about S - 1 without repeating the
 *   edge sample.  One launch, one workgroup per (row, frame), window, radix-2 FFT, modulus and log1p in fp64: the result is the
 *   reference's value but for the final rounding to fp32.  out [B NF, Fp], Fp >= F, pad columns zero.  DLIP_EINVAL unless n_fft is a
 *   power of two in 128 .. 1024, 1 <= win <= n_fft, hop >= 1, S >= n_fft / 2 + 1 (one reflection per side suffices),
 *   NF == 1 + S / hop, F == n_fft / 2 + 1, Fp >= F, B NF < 2^31.
 * dlip_stft_logmag_wave_ragged_f32 (models/audio_models/datasets.py:72-76, one utterance at a time: train_fusion.py:334-349): row b
 *   ends at S_b = clamp(sample_len[b], n_fft / 2 + 1, S) (device int32 [B], never read on the host), has NF_b = 1 + S_b / hop frames and
 *   is reflected about its own end; samples >= S_b are never read; frames t >= NF_b are zero rows.  Frame t < NF_b holds the bits the
 *   rectangular entry point gives for the S_b-sample signal alone.
 * dlip_stft_frame_lengths_i32 (models/audio_models/datasets.py:72-76: the frame count of librosa.stft): frame_lengths[b] = NF_b on the
 *   device, the counterpart of dlip_wave_frame_lengths_i32 -- the `frame_lengths` of dlip_cmvn_nct_ragged_f32 /
 *   dlip_delta_nct_ragged_f32 (datasets.py:52-63 behind the spectrogram, unchanged) and the encoders' `lengths`.
 * ------------------------------------------------------------------------------------------ */
int dlip_stft_logmag_wave_f32(const float* x, float* out, int64_t B, int64_t S, int32_t NF, int32_t win, int32_t hop, int32_t n_fft,
                              int32_t F, int32_t Fp, dlip_stream_t stream);
int dlip_stft_logmag_wave_ragged_f32(const float* x, const int32_t* sample_len, float* out, int64_t B, int64_t S, int32_t NF,
                                     int32_t win, int32_t hop, int32_t n_fft, int32_t F, int32_t Fp, dlip_stream_t stream);
int dlip_stft_frame_lengths_i32(const int32_t* sample_len, int32_t* frame_lengths, int32_t B, int64_t S, int32_t n_fft, int32_t hop,
                                dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 62) SLIDING-WINDOW CMN AND ENERGY-VAD FRAME SELECTION behind the front-end: the stage the reference's own speech pipeline
 * spells out (conf/audio_config.yaml:21 `plda_input` and :25 `nn_input`: `apply-cmvn-sliding --norm-vars=false --center=true
 * --cmn-window=300 ... | select-voiced-frames ... vad.scp`).  No source for these tools ships upstream: parity is UNPINNED, and this
 * block with DESIGN.md 4f is the definition, restated from Kaldi's published SlidingWindowCmn and ComputeVadEnergy.
 * x [B, C, NF] fp32, time contiguous (the front-end's output); `lengths` (device int32 [B], nullable): row b holds
 * n = clamp(lengths[b], 1, NF) frames (NF when NULL), clamped on the device and never read on the host -- a recorded plan replays
 * with a new vector -- and is computed as if it were alone: frames t >= n are never loaded (the padding may hold anything), full
 * lengths give the bits of lengths == NULL, no atomics, the same bits on every run.
 *
 * dlip_vad_energy_select_i32 (Kaldi compute-vad-energy + the index side of select-voiced-frames): e[t] = log_energy[b energy_stride + t]
 *   (a row of x is passed without a copy: log_energy = x + energy_row NF, energy_stride = C NF);
 *   thr = fp32(energy_threshold + energy_mean_scale (sum_{t<n} e[t]) / n), the sum in fp64 in an order n alone decides, rounded once
 *   (energy_mean_scale == 0: thr = fp32(energy_threshold), no sum);  for t < n: den = |[t - context, t + context] within [0, n)|,
 *   num = how many of those frames have e > thr, voiced[t] = (float)num >= (float)den * proportion_threshold (the product in fp32,
 *   Kaldi's BaseFloat).  `voiced` (uint8 [B, NF], nullable) is an external decision (`vad.scp`) taken instead; log_energy may then be
 *   NULL.  V = the row's voiced frames; V < min_keep: the row keeps all its n frames and fallback[b] = 1 (Kaldi drops an utterance
 *   without voiced frames; a batch cannot drop a row and the host never sees V), else 0.  out_len[b] = V, or n for a fallback row;
 *   pos [B, NF] = the destination column of frame t (kept frames packed to the front in order), -1 for a dropped frame and for
 *   t >= n.  One workgroup per row.  DLIP_EINVAL: context < 0, min_keep < 1, proportion_threshold outside [0, 1], B or NF < 1, NF > 2^30,
 *   neither log_energy nor voiced, energy_stride < NF.
 * dlip_cmn_sliding_select_f32 (Kaldi apply-cmvn-sliding, then the data side of select-voiced-frames): the window of frame t is
 *     center:  begin = t - window / 2 (integer division), end = begin + window;     else:  begin = t - window, end = t + 1
 *     if begin < 0: end -= begin, begin = 0;      if !center and end > t: end = max(t + 1, min_window)
 *     if end > n: begin -= end - n, end = n, if begin < 0: begin = 0
 *   v[t] = x[t] - mean(x[begin:end]); norm_vars != 0: v[t] *= max(sum x^2 / w - mean^2, 1e-10)^(-1/2), 0 where w = end - begin = 1.
 *   The window ALWAYS runs over the row's n frames of x, before the selection.  Sums in fp64 in an order (t, n, window, center,
 *   min_window) alone decide -- a workgroup owns the DLIP_CMN_TILE frames t belongs to, forms the fp64 prefix sums of the frames its
 *   windows reach over, less the first of them (thread by thread front to back, the threads' totals in thread order: mean and
 *   variance do not move with that pivot and the prefixes stay the size of the signal's variation) and takes a window's sum as
 *   the difference of two of them; a window of at most 16 frames is summed frame by frame -- and the result is rounded to fp32 once.  pos / out_len from the call above: y[b, c, pos[t]] = v[t] for pos[t] >= 0, columns >= out_len[b] exact
 *   zeros; both NULL: no selection (y[b, c, t] = v[t], zeros from n on).  window == 0: the selection alone, kept values copied
 *   bit for bit.  y must not be x.  DLIP_EINVAL: window outside [0, DLIP_CMN_MAX_WINDOW], min_window outside
 *   [1, DLIP_CMN_MAX_WINDOW], B, C or NF < 1, only one of pos / out_len given.
 * ------------------------------------------------------------------------------------------ */
#define DLIP_CMN_TILE 1024
#define DLIP_CMN_MAX_WINDOW 768
int dlip_vad_energy_select_i32(const float* log_energy, int64_t energy_stride, const uint8_t* voiced, const int32_t* lengths,
                               double energy_threshold, double energy_mean_scale, int32_t context, float proportion_threshold,
                               int32_t min_keep, int32_t* pos, int32_t* out_len, int32_t* fallback, int32_t B, int32_t NF,
                               dlip_stream_t stream);
int dlip_cmn_sliding_select_f32(const float* x, const int32_t* lengths, const int32_t* pos, const int32_t* out_len, float* y, int32_t B,
                                int32_t C, int32_t NF, int32_t window, int32_t center, int32_t min_window, int32_t norm_vars,
                                dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 63) WAVEFORM RESAMPLING in front of the audio front-end: the rate conversion of the reference's test loader
 * (models/audio_models/datasets.py:459-463: `librosa.resample(data, rate, self.rate)` for a file whose rate differs from the configured
 * one) and the speed perturbation of an x-vector recipe (sox `speed 0.9 / 1.0 / 1.1`, the third augmentation beside reverberation and
 * additive noise) are one operation, a rational polyphase FIR resampler.  For a row of n samples, a ratio up / down in lowest terms
 * and a prototype filter h[0 .. L) with centre c = (L - 1) / 2 (integer division):
 *
 *     n_out = ceil(n up / down),   y[m] = sum_i x[i] h[c + m down - i up],  0 <= m < n_out,  x = 0 outside [0, n),  h = 0 outside [0, L)
 *
 * -- scipy.signal.resample_poly(x, up, down) when h is scipy's default design (deeplip_amd/resample.py: design).  Parity with
 * librosa's own filter (resampy's `kaiser_best`) is UNPINNED: nothing upstream pins the result.  In polyphase form, with q = c + m down,
 * r = q mod up, i_hi = q div up and K = ceil(L / up):  y[m] = sum_{j < K} tab[r][j] x[i_hi - j],  tab[r][j] = h[r + j up].
 *
 * dlip_wave_resample_f32 (models/audio_models/datasets.py:459-463): wave [B, S] fp32 + `lengths` (device int32 [B], nullable): row b
 *   holds n = clamp(lengths[b], 1, S) samples (S when NULL); input samples t >= n are never read.  The bank of Q ratios lives on the
 *   device: `bank` int32 [Q, 4] = (up, down, c, K) per ratio and `tabs` fp32 [Q, tab_stride], ratio q's table at tabs + q tab_stride
 *   as [up][Kp] words, Kp = K | 1 (the phase stride is odd: lanes on different phases spread over the LDS banks; the pad word is
 *   never read).  `ratio_idx` int32 [B]: the row's ratio, clamped to Q - 1; < 0: the row passes through, min(n, S_out) samples copied
 *   bit for bit.  out [B, S_out]: row b gets n_out = min(ceil(n up / down), S_out) samples and exact zeros from n_out to S_out;
 *   out_lengths[b] = n_out (device int32 [B], never read on the host: a recorded plan replays with new lengths and indices).  Exact
 *   fp32 on the vector ALUs: one fmaf per product, j ascending from an accumulator of 0.f, the same for every output -- a row has
 *   the same bits whatever B, S, S_out, Q, `tile` and its neighbours are.  Every index product (m down, n up, q) is formed in 64
 *   bits.  A 256-lane workgroup owns tiles of `tile` consecutive outputs of one row (256, 512 or DLIP_RESAMPLE_TILE; consecutive
 *   lanes consecutive outputs) and stages the row's table (`tab_stride` words of LDS) and each tile's input span (`span_words`) in
 *   LDS.  A descriptor read on the device is not trusted: one with up or down outside [1, DLIP_RESAMPLE_MAX_FACTOR], c < 0, K < 1,
 *   up Kp > tab_stride or a tile span above span_words makes its rows pass through.  DLIP_EINVAL: tab_stride + span_words >
 *   DLIP_RESAMPLE_LDS_WORDS (a ratio that does not fit), another tile, B outside [1, 65535], S or S_out outside [1, 2^31 - 1 - tile],
 *   Q < 1, out == wave.
 * dlip_wave_resample_fits (host only, no launch): the longest tile (DLIP_RESAMPLE_TILE, 512 or 256) at which the ratio up / down
 *   with an L-tap prototype fits the kernel's LDS budget -- up Kp + span <= DLIP_RESAMPLE_LDS_WORDS -- or 0 where none does (or up
 *   or down lies outside [1, DLIP_RESAMPLE_MAX_FACTOR]).  A bank runs at the shortest tile of its ratios.
 * dlip_wave_resample_span_words (host only): ceil((tile - 1) down / up) + K, the input words a tile of one ratio reaches over;
 *   `span_words` of a launch is the largest over its bank.  Negative on bad arguments.
 * ------------------------------------------------------------------------------------------ */
#define DLIP_RESAMPLE_TILE 1024
#define DLIP_RESAMPLE_LDS_WORDS 15360
#define DLIP_RESAMPLE_MAX_FACTOR 4096
int32_t dlip_wave_resample_fits(int32_t up, int32_t down, int32_t L);
int64_t dlip_wave_resample_span_words(int32_t up, int32_t down, int32_t K, int32_t tile);
int dlip_wave_resample_f32(const float* wave, const int32_t* lengths, const float* tabs, const int32_t* bank, const int32_t* ratio_idx,
                           float* out, int32_t* out_lengths, int32_t B, int64_t S, int64_t S_out, int32_t Q, int32_t tab_stride,
                           int32_t span_words, int32_t tile, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 64) ATTENTIVE STATISTICS POOLING of both speech encoders, one head (`pooling: attentive_statistic`, pooling.py:73-107; on these
 * entry points since ABI 67) or several (`pooling: multi_head_attention`, conf/audio_config.yaml:71, conf/fusion_config.yaml:58;
 * upstream `MultiHeadAttention(input_size, head=4, hidden_size=[100,200,300,400])` is an empty TODO class,
 * models/audio_models/pooling.py:62-71: deeplip_amd/audio.py and DESIGN.md 4h are the definition).  n heads of widths Hd_h, S = sum Hd_h,
 * head_off = their prefix sums (DEVICE int32 [n + 1], head_off[0] = 0, head_off[n] = S; every value is clamped to [0, S] where it is
 * read, so a wrong array leaves no row; NULL is allowed for n == 1 and means the one head owns the columns [0, S)).  x [B,T,C] fp32
 * channels-last, hidden [B,T,S] = x W^T + b for ALL heads (one GEMM in front), v [S], k [n].  With L_b = clamp(len[b] + len_add, 0, T) valid frames (len / len_add as dlip_meanstd_pool_f32; NULL: T):
 *     e[b,h,t]     = relu(hidden[b,t,off_h:off_{h+1}]) . v[off_h:off_{h+1}] + k[h]
 *     alpha[b,h,:] = softmax over t < L_b of e[b,h,:]            (zeros for t >= L_b)
 *     m_h[c] = sum_t alpha x,   s_h[c] = sqrt(max(sum_t alpha x^2 - m_h^2, 0) + eps),   y[b] = cat_h [m_h | s_h]       [B, n 2C]
 * -- n attentive statistics poolings (pooling.py:87-107) from one read of hidden and one read of x.  eps == 0 (ABI 67) is the
 * reference's expression s_h[c] = sqrt(sum_t alpha x^2 - m_h^2) without floor: a feature that is constant over the valid frames gives
 * 0, or NaN where rounding takes the difference below zero, forward and a non-finite gradient (0 / 0) backward, as in the reference.
 * Exact fp32 data, fp64 wherever a sum runs over frames, channels or hidden units, no atomics, the same bits on every run; padding
 * frames of x and hidden are never loaded.  1 <= n <= 8, T <= 16000, B <= 65535.
 *
 * dlip_mh_attn_scores_f32: alpha [B,n,T] from hidden.  One wave per frame reads the row's S floats once (segmented dot products); the
 *   softmax runs on a (head, utterance) grid with its maximum and its sum reduced across the workgroup.  S >= n.
 * dlip_mh_attn_stat_pool_f32: y from x and alpha on a (C / 64, utterance) grid like dlip_meanstd_pool_f32's: alpha is staged in LDS 256
 *   frames at a time, each x element is loaded once and feeds the 2 n accumulators of all heads.  C % 4 == 0, x 16-byte aligned,
 *   eps >= 0, and the backward's LDS bound below (what could not be differentiated is refused here already).
 * dlip_mh_attn_stat_pool_bwd_f32: per head the chain through the root and the square on the centred value, with g_q,h = ds_h / (2 s_h)
 *   (s_h read from y, so the floor of eps > 0 is taken as the identity: the weighted variance is >= 0 in exact arithmetic):
 *     dalpha[b,h,t]   = sum_c x (dm_h + g_q,h (x - 2 m_h))                         pass 1 over x, all heads at once
 *     de [B,n,T]      = alpha (dalpha - sum_t' alpha dalpha)                       (zeros behind L_b);  dek [B,n] = sum_t de (its column
 *                                                                                    sums over B = dk)
 *     dx [B,T,C]      = sum_h alpha[b,h,t] (dm_h + 2 g_q,h (x - m_h))              pass 2 over x; summed over heads in fp64, written ONCE,
 *                                                                                    zeros in padding frames
 *     dhidden [B,T,S] = de[b,h(j),t] v_j [hidden > 0],   rde [B,T,S] = de[b,h(j),t] relu(hidden)       (column sums of rde = dv)
 *   Pass 1 runs on a (row range, utterance) grid with dm | g_q | m of every head in LDS: 3 n C floats <= 160 KiB (n = 4: C <= 3412, n = 8:
 *   C <= 1704; the E-TDNN's C = 1500 at n = 4 takes 70 KiB).  x, y, dy, dx 16-byte aligned, C % 4 == 0, S >= n, eps >= 0 (the forward's;
 *   checked, the std in y holds it).
 * DLIP_EINVAL before any launch: n outside [1, 8], T > 16000, B > 65535, the LDS bound, C % 4, alignment, eps < 0, a null pointer
 *   (head_off with n >= 2 included).
 * ------------------------------------------------------------------------------------------ */
int dlip_mh_attn_scores_f32(const float* hidden, const float* v, const float* k, const int32_t* head_off, const int32_t* len,
                            int32_t len_add, float* alpha, int32_t B, int32_t T, int32_t S, int32_t n, dlip_stream_t stream);
int dlip_mh_attn_stat_pool_f32(const float* x, const float* alpha, const int32_t* len, int32_t len_add, float eps, float* y, int32_t B,
                               int32_t T, int32_t C, int32_t n, dlip_stream_t stream);
int dlip_mh_attn_stat_pool_bwd_f32(const float* x, const float* hidden, const float* v, const int32_t* head_off, const float* alpha,
                                   const float* y, const float* dy, const int32_t* len, int32_t len_add, float eps, float* dx,
                                   float* dhidden, float* rde, float* de, float* dek, int32_t B, int32_t T, int32_t C, int32_t S, int32_t n,
                                   dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 65) REVERBERATION WITH LONG ROOM RESPONSES: the definition of dlip_wave_reverb_f32 (ABI 60) -- y[t] = sum_k h[k] x[t + d - k],
 * 0 <= t < n, x zero outside [0, n), d the tap of the direct path, optional keep_power, zero tail, pass-through rows bit for bit --
 * computed as a uniformly partitioned overlap-save convolution in fp32: P = DLIP_OLS_BLOCK new samples per step, transform length
 * 2P, partition boundaries anchored at sample 0 of the row and tap 0 of the response, so a row's bits depend on (x[:n], h, d) alone,
 * never on B, S, Lmax or the neighbours.  Responses up to DLIP_OLS_MAX_TAPS (4.1 s at 16 kHz); cost per output block proportional to
 * the response's own ceil(len / P) partitions.  The two routes agree to fp32 rounding, not bit for bit: the caller chooses one.
 *
 * dlip_wave_rir_spectra_bytes (train_audio.py:454; host only): bytes of the spectra block of a bank rir [R, Lmax] -- the twiddle table
 *   (P complex words) and P complex words per (response, partition of Lmax); negative on bad sizes (Lmax > DLIP_OLS_MAX_TAPS).
 * dlip_wave_rir_spectra_f32 (train_audio.py:454: the room responses of the 'reverb' kind, transformed once per bank): fills `spectra`
 *   (8-byte aligned, caller-owned) from rir [R, Lmax] and rir_len (clamped to [1, Lmax] on the device); partition p of response r =
 *   the half spectrum of h_r[pP : (p + 1)P) zero-padded to 2P, bins 0 and P sharing one word, scaled by 1 / P.  One launch.
 * dlip_wave_reverb_fft_workspace_bytes (train_audio.py:454; host only): bytes of the caller-owned workspace of the call below: the
 *   power partials of dlip_wave_reverb_workspace_bytes(B, S), then the input spectra, P complex words per (row, block of S);
 *   negative on bad sizes.
 * dlip_wave_reverb_fft_f32 (train_audio.py:454: the 'reverb' kind, as dlip_wave_reverb_f32): lengths, rir_idx, rir_len and rir_peak are
 *   clamped on the device exactly as there.  Launches: the input spectra of the reverberated rows (samples t >= n are never read);
 *   one workgroup per (row, output block) accumulates X[k - p] H[p] over the response's own partitions, p ascending, inverts in LDS
 *   and writes y[j - d] and the zero tail; keep_power != 0 adds the FIR route's own power sums (per DLIP_FIR_TILE tile, same order)
 *   and its gain launch: 2 launches, 4 with keep_power.  No atomics.  DLIP_EINVAL before any launch for Lmax > DLIP_OLS_MAX_TAPS,
 *   null pointers, y == x, a short or misaligned (8-byte) workspace or spectra block; B <= 65535.
 * ------------------------------------------------------------------------------------------ */
#define DLIP_OLS_BLOCK 2048
#define DLIP_OLS_MAX_TAPS 65536
int64_t dlip_wave_rir_spectra_bytes(int32_t R, int32_t Lmax);
int dlip_wave_rir_spectra_f32(const float* rir, const int32_t* rir_len, void* spectra, int64_t spectra_bytes, int32_t R, int32_t Lmax,
                              dlip_stream_t stream);
int64_t dlip_wave_reverb_fft_workspace_bytes(int64_t B, int64_t S, int32_t Lmax);
int dlip_wave_reverb_fft_f32(const float* x, const int32_t* lengths, const void* spectra, const int32_t* rir_len,
                             const int32_t* rir_peak, const int32_t* rir_idx, float* y, void* workspace, int64_t workspace_bytes, int32_t B,
                             int32_t S, int32_t R, int32_t Lmax, int32_t keep_power, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 66) THE A-SOFTMAX AND CONTRASTIVE CRITERIA: the last two names of `train.loss` (conf/audio_config.yaml:130: "CrossEntropy,
 * A-Softmax, LMCL(AM-Softmax), AAM-Softmax, Contrastive, Triplet") that were empty stubs -- `ASoftmax` (models/audio_models/loss.py:53-59)
 * and `Contrastive` (loss.py:69-75).  Upstream has no implementation: parity unpinned, the definitions are the build's own.
 *
 * dlip_asoftmax_logits_f32 (loss.py:53-59; SphereFace, Liu et al. 2017): c [B,K] cosine logits, r [B] = the rows' clamped norms
 *   (dlip_row_norm_f32), labels int64 [B], lambda = ONE float in device memory, read by the kernel (a recorded step follows the annealing
 *   schedule through the pointer), m = 1 .. 4.  backward == 0: out = z [B,K], z_bj = r_b c_bj off the target, z_by = r_b (lambda c +
 *   psi(c)) / (1 + lambda) on it, psi(c) = (-1)^k T_m(c) - 2k, k = #{ j in 1 .. m-1 : c <= cos(j pi / m) }, c clamped to [-1, 1], T_m the
 *   Chebyshev polynomial (dz, dr unused, may be NULL).  backward != 0: out = dc [B,K] (= r_b dz_bj, times (lambda + psi'(c)) / (1 + lambda)
 *   on the target) and dr [B] = sum_j dz_bj z_bj / r_b, summed in fp64 in a fixed order; 0 on a row with r_b <= r_floor (the clamp).
 * dlip_row_norm_f32 / dlip_row_norm_bwd_f32: r [U] = max(|x_u|, eps) with the sum, order and rounding of dlip_l2_normalize_f32 (the same
 *   bits as the norm it divides by); dx [U,D] = dr_u x_u / r_u, zeros on a row at the clamp (r_u <= eps).
 *
 * dlip_contrastive_loss_f32 (loss.py:69-75; the cosine form of adambielski/siamese-triplet's OnlineContrastiveLoss = torch.nn.
 *   CosineEmbeddingLoss on pairs selected on the device): x [B,E] and labels int32 [B] under the limits of dlip_triplet_mine_f32, whose Gram
 *   launch fills g [B,B] = x x^T and rownorm [B].  mode 0: every pair a < j; mode 1 (hard negative): every positive pair a < p and, per
 *   anchor row a with P_a later positives, the min(P_a, #negatives after a) negatives n > a of highest cosine, the lower index winning
 *   ties (exact, by rank counting).  A positive pair costs 1 - cos, a selected negative relu(cos - margin); loss[0] = the mean over all
 *   selected pairs, n_pairs[0] = their number N (N == 0: loss = 0).  Scratch the caller owns: rowsum [B] fp64, rowcnt [B].  w [B,B] int32,
 *   every element written: -1 positive pair, +1 selected negative with an active hinge, 0 otherwise -- the `wcount` that
 *   dlip_triplet_loss_bwd_f32 takes as it is (with n_triplets = n_pairs): that launch IS this loss's backward.  sel (nullable) [B,B] int32,
 *   every element written: 1 positive pair, 2 selected negative, 0 otherwise.  Launches: Gram, rows, finish.  No atomics.
 * ------------------------------------------------------------------------------------------ */
int dlip_asoftmax_logits_f32(const float* c, const float* r, const int64_t* labels, const float* lambda, const float* dz, float* out,
                             float* dr, int32_t B, int32_t K, int32_t m, float r_floor, int32_t backward, dlip_stream_t stream);
int dlip_row_norm_f32(const float* x, float* r, int32_t U, int32_t D, float eps, dlip_stream_t stream);
int dlip_row_norm_bwd_f32(const float* x, const float* r, const float* dr, float* dx, int32_t U, int32_t D, float eps,
                          dlip_stream_t stream);
int dlip_contrastive_loss_f32(const float* x, const int32_t* labels, float margin, int32_t mode, float* g, float* rownorm, double* rowsum,
                              int32_t* rowcnt, int32_t* w, int32_t* sel, float* loss, int32_t* n_pairs, int32_t B, int32_t E,
                              dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 67, added) SPECAUGMENT ON THE FEATURE BATCH (Park et al. 2019): a time warp, then frequency masks, then time masks -- the one
 * augmentation of a speaker-embedding recipe that acts on the features, and the only one the feature-fed training path can take
 * (`data.spec_augment` of conf/audio_config.yaml).  Nothing upstream defines the stage: this block and DESIGN.md 4j are the definition.
 *
 * dlip_spec_augment_f32: x, y fp32 [B, C, NF] -- the front-end's layout, features by frames, frames contiguous (the ResNet's
 *   [B, 1, F, T] is the same memory with C = F); y must not be x.  `lengths` (device int32 [B], nullable): row b holds
 *   n = clamp(lengths[b], 1, NF) frames (NF when NULL); frames t >= n of x are never loaded (the padding may hold NaN), frames t >= n of
 *   y are exact zeros.  `draws`: device int32 [B, DLIP_SPECAUG_DRAWS], DLIP_SPECAUG_DRAWS = 2 + 4 DLIP_SPECAUG_MAX_MASKS, each word a 31-bit
 *   uniform integer (negatives are taken as 0) that the DEVICE resolves against the row's length -- the host never sees n behind
 *   VoicedFrames or in a recorded plan, so it draws length-free integers:  pick(r, m) = (int64(r) m) >> 31, in [0, m).  Per row:
 *   [0] warp centre, [1] warp shift, then (width, start) of each of the MAX_MASKS frequency masks, then (width, start) of each of the
 *   MAX_MASKS time masks; slots past n_freq / n_time are ignored.
 *   Time warp (warp = W >= 0): We = min(W, (n - 3) / 2) (integer division; 0 for n < 3); We < 1: none.  Else c = We + 1 + pick(r0, n - 2 -
 *   2 We), d = pick(r1, 2 We + 1) - We, c' = c + d (1 <= c, c' <= n - 2).  Output frame t reads the source position s = (t c) / c' for
 *   t <= c', s = c + ((t - c')(n - 1 - c)) / (n - 1 - c') behind it (integer products in 64 bits, converted to fp64, ONE fp64 division):
 *   i = min(floor(s), n - 2), a = (float)(s - i), v[f, t] = fmaf(a, x[f, i + 1] - x[f, i], x[f, i]) with the difference in fp32; a == 0
 *   takes x[f, i] and a == 1 (only frame n - 1) takes x[f, i + 1] as they are, so frames 0, c' and n - 1 hold their sources' bits and
 *   frames 0 and n - 1 stay in place.  d == 0 leaves the row bit for bit.
 *   Frequency masks (i < n_freq): w = pick(r, min(freq_width, C) + 1), f0 = pick(r', C - w + 1): features [f0, f0 + w).
 *   Time masks (j < n_time): cap = min(time_width, (int)floor(time_ratio (double)n)) (the product in fp64), w = pick(r, cap + 1),
 *   t0 = pick(r', n - w + 1): frames [t0, t0 + w).  time_ratio = 1: no adaptive cap beyond the row itself.
 *   y[f, t] = the fill value where any mask covers (f, t), else v[f, t]: masks apply after the warp and may overlap.  fill = 0: exact
 *   zeros (the row's mean after CMVN).  fill = 1: the mean of the row's own INPUT over f < C, t < n -- a first launch of
 *   DLIP_SPECAUG_MEAN_PARTS fp64 partial sums per row into the workspace, in an order (C, n) alone decide, no atomics; rounded to fp32
 *   once, every masked entry of the row holds those bits.
 *   A row has the same bits whatever B, NF, its neighbours and the launch geometry are; full lengths give the bits of lengths == NULL.
 *   Lanes run along time (one 4-byte access per lane; one 16-byte access where NF % 4 == 0 and x, y are 16-byte aligned); a workgroup
 *   resolves its frames' (i, a, time-mask bit) once and walks a contiguous range of features with them.  Launches: 1, 2 with fill = 1.
 *   DLIP_EINVAL before any launch: B, C or NF < 1 (B <= 65535), a negative warp, freq_width or time_width, a mask count outside
 *   [0, DLIP_SPECAUG_MAX_MASKS], time_ratio outside [0, 1] or NaN, fill outside {0, 1}, y == x, a null pointer (lengths excepted), a
 *   workspace that is misaligned (8 bytes) or smaller than dlip_spec_augment_workspace_bytes says.
 * dlip_spec_augment_workspace_bytes (host only, no launch): bytes of the caller-owned workspace; negative on bad sizes.
 * ------------------------------------------------------------------------------------------ */
#define DLIP_SPECAUG_MAX_MASKS 8
#define DLIP_SPECAUG_DRAWS 34      /* 2 + 4 * DLIP_SPECAUG_MAX_MASKS */
#define DLIP_SPECAUG_MEAN_PARTS 8
int64_t dlip_spec_augment_workspace_bytes(int32_t B, int32_t C, int32_t NF);
int dlip_spec_augment_f32(const float* x, const int32_t* lengths, const int32_t* draws, float* y, void* workspace,
                          int64_t workspace_bytes, int32_t B, int32_t C, int32_t NF, int32_t warp, int32_t n_freq, int32_t freq_width,
                          int32_t n_time, int32_t time_width, double time_ratio, int32_t fill, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 67, added) THE FACTORIZED TDNN, `arch: ftdnn` (conf/audio_config.yaml:84-92 names the architecture; upstream ships no source
 * for it: this block and DESIGN.md 4k are the definition).  A factorized block is  factor: Conv1d(Cin -> Bn, k taps, dilated, no bias,
 * no BatchNorm, no activation) -> context_layer: Conv1d(Bn -> Cout, 1 tap, bias) -> BatchNorm / LeakyReLU(0.2) in the order bn_first
 * says -> (Cin == Cout and s != 0 only) the bypass y[b, :, t] += s x[b, :, t - context[0]], the input frame at context offset 0.  Both
 * convolutions are the TDNN's (dlip_conv_nhwc_*); what is new is below.
 *
 * dlip_semi_orth_step_f32 (conf/audio_config.yaml:84-92): the semi-orthogonal constraint of Povey et al. 2018 (Kaldi's
 *   ConstrainOrthonormalInternal with a floating scale) on EVERY factor matrix of a model in one launch pair.  `table`: device array of
 *   n_mats rows { float* M; int32 rows; int32 cols } (16 bytes each): M row-major [rows, cols] = the factor weight [Bn, Cin, k] seen as
 *   [Bn, Cin k], 1 <= rows <= max_rows <= DLIP_SEMI_ORTH_MAX_ROWS, rows <= cols <= max_cols (a row outside these is skipped by the
 *   device, never addressed).  `counter`: device int32[2]; counter[0] = optimizer steps so far.  With n = counter[0] + 1 the step is
 *   DUE iff every > 0 and n % every == 0; the pair always leaves counter[0] = n (counter[1] is its own scratch), so a recorded and
 *   replayed pair applies the step on the same iterations as an eager loop, without a host read.  When due, per matrix:
 *     P = M M^T,  tp = tr P,  tpp = |P|_F^2,  alpha2 = tpp / tp,  ratio = tpp rows / tp^2,
 *     nu = 1/8, halved if ratio > 1.02, halved again if ratio > 1.1,      M <- M - (4 nu / alpha2) (P - alpha2 I) M
 *   (tp = 0, an all-zero matrix: left alone).  Exact fp32 products (fma chains on the vector ALUs).  P is a split-K reduction over
 *   DLIP_SEMI_ORTH_SPLITS workgroups per matrix, the last one to arrive adds the partials in split order (ticket words in the
 *   workspace, self-resetting); the second launch holds P in LDS (64 KB at 128 rows), derives tp and tpp in fp64 in one fixed order --
 *   the same alpha2 and nu in every workgroup -- and rewrites a DLIP_SEMI_ORTH_PANEL-column panel of M in place.  No atomics on
 *   data: the result has the same bits on every run.  `workspace`: dlip_semi_orth_workspace_bytes(n_mats) bytes, 16-byte aligned,
 *   ZEROED ONCE by the caller before its first use and then left to the launches.  DLIP_EINVAL before any launch: a null pointer,
 *   n_mats outside [1, DLIP_SEMI_ORTH_MAX_MATS], every < 0, max_rows outside [1, DLIP_SEMI_ORTH_MAX_ROWS], max_cols < max_rows, a
 *   workspace too small or misaligned.  Launches: 2.
 * dlip_semi_orth_workspace_bytes (host only, no launch): bytes of that workspace; negative on a bad n_mats.
 * dlip_ftdnn_bypass_f32: out[b, t, :] = y[b, t, :] + scale x[b, t + shift, :] (one fma per element), y fp32 [B, Tp, C], x [B, T, C], out
 *   [B, Tp, C]; flags bit 0: x is in the split activation format, bit 1: out is written in it (C % 32 == 0 then; the range report of
 *   dlip_split_pack_f32).  C % 4 == 0, 0 <= shift, shift + Tp <= T, 16-byte aligned pointers; out may be y unless bit 1 is set, never x.
 *   Each element depends on its own (b, t, c) alone: a row has the same bits alone and in a ragged batch.
 * dlip_ftdnn_bypass_bwd_f32: dx[b, t + shift, :] += scale dy[b, t, :] IN PLACE on dx [B, T, C] (the factor convolution's data gradient),
 *   dy [B, Tp, C]: the block input's whole gradient after one pass, no zero-filled temporary.  Same conditions.
 * ------------------------------------------------------------------------------------------ */
#define DLIP_SEMI_ORTH_MAX_ROWS 128
#define DLIP_SEMI_ORTH_MAX_MATS 64
#define DLIP_SEMI_ORTH_SPLITS 16
#define DLIP_SEMI_ORTH_PANEL 64
int64_t dlip_semi_orth_workspace_bytes(int32_t n_mats);
int dlip_semi_orth_step_f32(const void* table, int32_t n_mats, int32_t max_rows, int32_t max_cols, int32_t* counter, int32_t every,
                            void* workspace, int64_t workspace_bytes, dlip_stream_t stream);
int dlip_ftdnn_bypass_f32(const float* y, const float* x, float* out, int32_t B, int32_t T, int32_t Tp, int32_t C, int32_t shift,
                          float scale, int32_t flags, dlip_stream_t stream);
int dlip_ftdnn_bypass_bwd_f32(const float* dy, float* dx, int32_t B, int32_t T, int32_t Tp, int32_t C, int32_t shift, float scale,
                              dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 67, added) THE SINC FILTER BANK, `arch: sincnet` (conf/audio_config.yaml names the architecture; upstream ships no source for it:
 * this block and DESIGN.md 4l are the definition): the SincNet layer (Ravanelli & Bengio 2018) in front of the TDNN stack -- F learnable
 * band-pass filters of L taps (odd, 3 .. DLIP_SINC_MAX_TAPS) on the raw waveform, squared, averaged per frame, logged.
 *
 * dlip_sinc_taps_f32: low_hz, band_hz [F] -> g [F, L].  With m = l - (L - 1) / 2:
 *     f1 = min_low_hz + |low_hz[f]|,   f2 = clamp(f1 + min_band_hz + |band_hz[f]|, min_low_hz, rate / 2)
 *     g[f, l] = w[l] (sin(2 pi f2 m / rate) - sin(2 pi f1 m / rate)) / ((pi m / rate) 2 (f2 - f1))  (m != 0),   g[f, (L - 1) / 2] = 1
 *     w[l] = 0.54 - 0.46 cos(2 pi l / (L - 1))
 *   formed in fp64 and rounded once; g is EVEN in m by construction (the half m >= 0 is computed and mirrored).  One workgroup.
 * dlip_sinc_taps_bwd_f32: dg [F, L] -> dlow, dband [F] by the chain rule through that formula (|.| has derivative sign(.), 0 at 0; a
 *   clamped f2 has derivative 0, as torch.clamp), summed over l in fp64 in one fixed order.  One workgroup.
 * dlip_sinc_features_f32: wave [B, S] (+ lengths int32 [B] or NULL: S; clamped to [1, S] on the device) and g -> y and frame_lengths
 *   int32 [B] (may be NULL).  x~ = the row on [0, len), zero outside -- never the neighbour row's bytes or the padding's:
 *     z[b, f, p] = sum_l g[f, l] x~[b, p + l - (L - 1) / 2]
 *     e[b, t, f] = (1 / frame_len) sum_{j < frame_len, t frame_step + j < len} z[b, f, t frame_step + j]^2,     y = log(e + eps)
 *   Frames per row: sigproc.framesig's count (1 for len <= frame_len, else 1 + ceil((len - frame_len) / frame_step)); NF is that count
 *   for S; frames at or past a row's count are zeros.  layout 0: y [B, F, NF] (Fp = F), the AudioFrontend contract; layout 1: y [B, NF, Fp]
 *   channels-last, F <= Fp <= F + 31, channels >= F written zero.  A workgroup owns (row, a tile of frames, 8 or 24 filters); the tile's
 *   samples + L - 1 halo sit in LDS (frame_len + L - 1 <= DLIP_SINC_LDS_SAMPLES); the pair sums x~[p - m] + x~[p + m] are formed once per
 *   position and shared by the filters ((L + 1) / 2 fma per filter and position: exact fp32 chains on the vector ALUs, m ascending);
 *   squares are added per frame on chip in fp64, positions ascending.  z is never stored.  Every row has the bits of the row run alone.
 * dlip_sinc_features_bwd_f32: y and dy (in `layout`) -> dg [F, L], the gradient on the even taps:
 *     dz[b, f, p] = z[b, f, p] (2 / frame_len) sum_{frames t of the row that hold p} dy[b, t, f] / (e[b, t, f] + eps)
 *     D[f, m] = sum_{b, p} dz[b, f, p] (x~[p - m] + x~[p + m])  (m > 0),  D[f, 0] = sum dz x~[p]
 *     dg[f, (L - 1) / 2 +- m] = D[f, m] / 2,   dg[f, (L - 1) / 2] = D[f, 0]
 *   (the two halves of an unconstrained tap gradient averaged: g[f, H - m] and g[f, H + m] are one quantity, and dlip_sinc_taps_bwd_f32
 *   yields the same parameter gradients from either).  z is recomputed, 1 / (e + eps) = exp(-y); rows of dy at or past a row's frame count
 *   are not read.  The waveform gets no gradient.  Workgroups walk (row, tile) items in a fixed stride and keep D in registers; one
 *   partial per workgroup goes to `workspace` (dlip_sinc_features_bwd_workspace_bytes, 16-byte aligned, needs no initialisation) and a
 *   second launch adds the partials in workgroup order in fp64: no atomics, two runs have the same bits.  Launches: 2.
 * DLIP_EINVAL before any launch: a null pointer (lengths and frame_lengths excepted), B outside [1, 65535], S < 1, F outside
 *   [1, DLIP_SINC_MAX_FILTERS], an even L or one outside [3, DLIP_SINC_MAX_TAPS], frame_len or frame_step < 1, frame_len + L - 1 >
 *   DLIP_SINC_LDS_SAMPLES, NF other than the frame count of S, a layout / Fp pair other than the two above, eps <= 0, rate <= 0, a
 *   negative min_low_hz / min_band_hz, min_low_hz > rate / 2, a workspace too small or misaligned.
 * ------------------------------------------------------------------------------------------ */
#define DLIP_SINC_MAX_TAPS 1023
#define DLIP_SINC_MAX_FILTERS 512
#define DLIP_SINC_LDS_SAMPLES 4096
int dlip_sinc_taps_f32(const float* low_hz, const float* band_hz, float* g, int32_t F, int32_t L, double rate, double min_low_hz,
                       double min_band_hz, dlip_stream_t stream);
int dlip_sinc_taps_bwd_f32(const float* low_hz, const float* band_hz, const float* dg, float* dlow, float* dband, int32_t F, int32_t L,
                           double rate, double min_low_hz, double min_band_hz, dlip_stream_t stream);
int dlip_sinc_features_f32(const float* wave, const int32_t* lengths, const float* g, float* y, int32_t* frame_lengths, int32_t B, int32_t S,
                           int32_t F, int32_t L, int32_t frame_len, int32_t frame_step, int32_t NF, int32_t layout, int32_t Fp, float eps,
                           dlip_stream_t stream);
int64_t dlip_sinc_features_bwd_workspace_bytes(int32_t B, int32_t S, int32_t F, int32_t L, int32_t frame_len, int32_t frame_step);
int dlip_sinc_features_bwd_f32(const float* wave, const int32_t* lengths, const float* g, const float* y, const float* dy, float* dg,
                               void* workspace, int64_t workspace_bytes, int32_t B, int32_t S, int32_t F, int32_t L, int32_t frame_len,
                               int32_t frame_step, int32_t NF, int32_t layout, int32_t Fp, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 67, added) LIP-CLIP AUGMENTATION ON THE DEVICE: time masks, cutout, mixup -- the training-time stage between the loader's frames
 * and the stem (train_video.py's --time-masks / --cutouts / --mixup-alpha; deeplip_amd.clip_augment.ClipAugment).  Nothing upstream
 * defines the stage: this block and DESIGN.md 4m are the definition, tests/clip_augment_ref.py restates it in numpy.
 *
 * Sources.  dlip_clip_augment_u8: uint8 frames [B, T, channels, Hs, Ws] (channels 1 gray | 3 RGB) with `crop`, `clip_params` (device
 *   int32 [B][4] = (oy, ox, flip, 0), clamped into the frame; NULL: the centre crop) and `lengths` exactly as dlip_crop_normalize_u8
 *   takes them; the base pixel is dlip_crop_normalize_u8's (BT.601 gray, (g / 255 - 0.421) / 0.165, contraction off), so an
 *   un-augmented pixel has its bits.  dlip_clip_augment_f32: float clips x [B, 1, T, H, W], already normalised, no crop and no flip
 *   (crop below = H, W).  Output y fp32 [B, 1, T, crop, crop] ([B, 1, T, H, W]); y must not be the source.
 * The augmented clip.  A_b = the cropped, flipped, normalised clip of row b, n_b = clamp(lengths[b], 1, T) (T when lengths is NULL);
 *   frames t >= n_b of the source are never loaded and frames t >= n_b of y are exact zeros.  `draws`: device int32
 *   [B, DLIP_CLIPAUG_DRAWS], DLIP_CLIPAUG_DRAWS = 6 DLIP_CLIPAUG_MAX_MASKS, each word a 31-bit uniform integer (negatives count as 0) the
 *   DEVICE resolves with pick(r, m) = (int64(r) m) >> 31, in [0, m): words [2 i], [2 i + 1] = (width, start) of time mask i, words
 *   [2 MAX + 4 j .. + 3] = (height, width, top, left) of cutout j; slots past n_time / n_cut are ignored.
 *   1. Fill value f_b: 0 for fill = 0; for fill = 1 the mean of A_b over its n_b crop crop pixels before any masking, accumulated in
 *      fp64 in one fixed order and rounded ONCE to fp32: a first launch writes one fp64 partial per (clip, chunk of
 *      DLIP_CLIPAUG_MEAN_FRAMES frames) into the workspace, the write pass adds the chunks below ceil(n_b / FRAMES) in index order.  No
 *      atomics: two runs and a replay have the same bits, and so has the row in any batch.
 *   2. Time mask i < n_time: cap = min(time_width, (int)floor(time_ratio (double)n_b)) (the product in fp64, as dlip_spec_augment_f32
 *      forms it), w = pick(r, cap + 1), t0 = pick(r', n_b - w + 1): frames [t0, t0 + w) become f_b.
 *   3. Cutout j < n_cut: h = min(pick(r, cut_size + 1), crop), w likewise, y0 = pick(r'', crop - h + 1), x0 = pick(r''', crop - w + 1):
 *      the rectangle [y0, y0 + h) x [x0, x0 + w) in OUTPUT coordinates (after the flip), the same in every frame t < n_b, becomes f_b.
 *   4. Mixup (perm and lam both non-NULL; both NULL: none): perm device int32 [B], lam device float [1].  p = perm[b]; p outside
 *      [0, B) or p == b: no partner, row b is A'_b (the result of 1-3) unblended.  Else for t < n_b
 *        y_b[t] = (lam A'_b[t]) + (mu A'_p[t]),   mu = 1 - lam in fp32,   A'_p[t] = 0 for t >= n_p,
 *      two fp32 products and one fp32 sum, contraction off (numpy float32 reproduces it bit for bit).  Frames t >= n_b stay zero.
 *   With mixup off every row has the bits of the row run alone with its own draws; with mixup on each operand has.
 * Launches: the mean pass (fill = 1 only; grid (chunk, clip)) and the write pass (grid (tile of 256 quads, frame, clip)): a lane
 *   forms four adjacent output pixels of both operands straight from the source bytes (one 4-byte word per colour plane, reversed
 *   under a flip, re-aligned for an odd ox) and stores one float4; no intermediate float clip exists; a lane whose quad is filled
 *   whole reads nothing of that clip.  crop (W) must be a multiple of 4.
 * DLIP_EINVAL before any launch: B or T outside [1, 65535], crop < 4 or crop % 4 != 0, channels not 1 or 3, Hs or Ws < crop, a mask
 *   count outside [0, DLIP_CLIPAUG_MAX_MASKS], a negative width or size (cut_size <= 2^30), time_ratio outside [0, 1] or NaN, fill
 *   outside {0, 1}, exactly one of perm / lam NULL, y == the source, y not 16-byte aligned, a null pointer (clip_params, lengths, perm,
 *   lam excepted), a workspace that is misaligned (8 bytes) or smaller than dlip_clip_augment_workspace_bytes says.
 * dlip_clip_augment_workspace_bytes (host only, no launch): bytes of the caller-owned workspace; negative on bad sizes.
 * ------------------------------------------------------------------------------------------ */
#define DLIP_CLIPAUG_MAX_MASKS 4
#define DLIP_CLIPAUG_DRAWS 24      /* 6 * DLIP_CLIPAUG_MAX_MASKS */
#define DLIP_CLIPAUG_MEAN_FRAMES 1
int64_t dlip_clip_augment_workspace_bytes(int32_t B, int32_t T);
int dlip_clip_augment_u8(const uint8_t* frames, const int32_t* clip_params, const int32_t* lengths, const int32_t* draws,
                         const int32_t* perm, const float* lam, float* y, void* workspace, int64_t workspace_bytes, int32_t B, int32_t T,
                         int32_t channels, int32_t Hs, int32_t Ws, int32_t crop, int32_t n_time, int32_t time_width, double time_ratio,
                         int32_t n_cut, int32_t cut_size, int32_t fill, dlip_stream_t stream);
int dlip_clip_augment_f32(const float* x, const int32_t* lengths, const int32_t* draws, const int32_t* perm, const float* lam, float* y,
                          void* workspace, int64_t workspace_bytes, int32_t B, int32_t T, int32_t H, int32_t W, int32_t n_time,
                          int32_t time_width, double time_ratio, int32_t n_cut, int32_t cut_size, int32_t fill, dlip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Step plans. The reference drives its encoders from a Python loop, one utterance and one torch.nn layer
 * at a time (train_fusion.py:338-358 extraction, :262-293 training step); here a step is ~45 short kernels
 * and the host must not sit between them.  A plan records every dlip_* launch made on `stream` between
 * dlip_plan_begin and dlip_plan_end (HIP stream capture, thread-local mode -> an instantiated hipGraph) and
 * dlip_plan_run replays them with ONE host call, asynchronously on the given stream.
 *   - `stream` of begin / end must be a created stream (the null stream cannot be captured);
 *   - between begin and end the caller makes launches only: no allocation, no synchronisation, no host copy
 *     (warm every kernel once on that stream first, so workspace registration and kernel attributes are set);
 *   - the plan addresses exactly the buffers of the recorded step: they stay caller-owned and must outlive it;
 *     new inputs are copied into the recorded input buffers;
 *   - a plan must not run concurrently with itself (replays on one stream are ordered).
 * dlip_plan_launches = kernel launches the plan holds.  dlip_plan_destroy(NULL) is a no-op.
 * ------------------------------------------------------------------------------------------ */
int dlip_plan_begin(dlip_stream_t stream);
int dlip_plan_end(dlip_stream_t stream, DLIP_HOST dlip_plan_t* plan);
int dlip_plan_run(dlip_plan_t plan, dlip_stream_t stream);
int dlip_plan_launches(dlip_plan_t plan);
int dlip_plan_destroy(dlip_plan_t plan);

#ifdef __cplusplus
}
#endif
#endif /* DEEPLIP_HIP_H */

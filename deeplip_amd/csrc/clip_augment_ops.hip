// Lip-clip augmentation on the device (added, the ABI version stays): time masks, cutout and mixup on the clips
// in front of the stem, straight from the loader's uint8 frames (crop + flip + BT.601 gray + normalisation, dlip_crop_normalize_u8's
// arithmetic through dlip_gray601 / dlip_pixel_norm) or from normalised float clips.  Nothing upstream defines the stage:
// include/deeplip_hip.h with DESIGN.md 4m is the definition, tests/clip_augment_ref.py restates it in numpy.  The host draws LENGTH-FREE
// 31-bit integers (`draws` [B, DLIP_CLIPAUG_DRAWS]); the device resolves them against the clip's own length n with
// pick(r, m) = (int64(r) m) >> 31, as dlip_spec_augment_f32 does.
//
// Write pass: a 256-lane workgroup owns (clip, frame, a tile of 256 quads); a lane forms FOUR adjacent output pixels and stores them as
// one float4.  Everything the clip alone decides -- its length, whether a time mask covers the frame, the cutout rectangles, the fill
// value, and the same for its mixup partner -- is computed from workgroup-uniform addresses, i.e. once per wave in scalar registers.  A
// lane then reads its four source pixels of each operand (one 4-byte word per colour plane, reversed under a flip, re-aligned where
// ox is odd), normalises, selects and blends: no intermediate float clip exists.  A lane whose quad is filled whole, and every lane
// of a frame past its clip's length, reads nothing of that clip.
// Mean pass (fill = 1 only): workgroup (clip, chunk of DLIP_CLIPAUG_MEAN_FRAMES frames) adds its frames' pixels in fp64 -- per lane
// quads ascending, lanes meeting in wave order -- into part[clip][chunk]; the write pass adds the chunks below ceil(n / FRAMES) in
// index order and rounds once.  (n, crop, the crop's origin and flip) alone decide the order: no atomics, the same bits on every run
// and in every batch.
#include "dlip_launch.h"
#include "dlip_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMasks = DLIP_CLIPAUG_MAX_MASKS;
constexpr int kMeanFrames = DLIP_CLIPAUG_MEAN_FRAMES;

// what both passes need to know about the launch (by value: kernel arguments, uniform)
struct ClipAug {
  const void* src;             // uint8 frames [B, T, CH, Hs, Ws] | float clips [B, 1, T, OH, OW]
  const int32_t* clip_params;  // [B, 4] = (oy, ox, flip, 0) | NULL: the centre crop (uint8 sources)
  const int32_t* lengths;      // [B] | NULL
  const int32_t* draws;        // [B, DLIP_CLIPAUG_DRAWS]
  const int32_t* perm;         // [B] | NULL
  const float* lam;            // [1] | NULL
  const double* part;          // [B, chunks] (fill = 1)
  float* y;                    // [B, 1, T, OH, OW]
  int B, T, Hs, Ws, OH, OW;    // OH = OW = crop for the uint8 sources
  int chunks;
  int n_time, time_width, n_cut, cut_size, fill;
  double time_ratio;
  int wide;                    // uint8: 4-byte words may be read at (address & ~3); float: float4 loads
};

__device__ __forceinline__ int row_len(const int32_t* lengths, int b, int T) {
  if (lengths == nullptr) return T;
  const int v = lengths[b];
  return v < 1 ? 1 : (v > T ? T : v);
}

// a 31-bit draw onto [0, m): negatives count as 0
__device__ __forceinline__ int pick(int r, int m) { return (int)(((long long)(r < 0 ? 0 : r) * m) >> 31); }

// the four bytes at p in memory order; `wide`: two aligned words, the second only where the first does not hold them all (so no byte
// past p + 3 rounded up to the next word is touched: the launch takes this path only for a word-aligned buffer of whole words)
__device__ __forceinline__ uint32_t load4_u8(const uint8_t* p, bool wide) {
  if (wide) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    const unsigned sh = (unsigned)(a & 3) * 8;
    const uint32_t lo = q[0];
    if (sh == 0) return lo;
    return (lo >> sh) | (q[1] << (32 - sh));
  }
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// where clip r's crop sits in its frames: (oy, ox) clamped into the frame as dlip_crop_normalize_u8 clamps them, and the flip
struct Geo {
  int oy, ox;
  bool flip;
};
__device__ __forceinline__ Geo clip_geo(const ClipAug& a, int r) {
  Geo g{(a.Hs - a.OH) / 2, (a.Ws - a.OW) / 2, false};
  if (a.clip_params != nullptr) {
    g.oy = min(max(a.clip_params[4 * r], 0), a.Hs - a.OH);
    g.ox = min(max(a.clip_params[4 * r + 1], 0), a.Ws - a.OW);
    g.flip = a.clip_params[4 * r + 2] != 0;
  }
  return g;
}

// KIND 0: float clips; 1: gray uint8 frames; 3: RGB uint8 frames.  The un-augmented pixels (cy, cx0 .. cx0 + 3) of frame t of clip r.
template <int KIND>
__device__ __forceinline__ void load_quad(const ClipAug& a, const Geo g, int r, int t, int cy, int cx0, float v[4]) {
  if constexpr (KIND == 0) {
    const float* p = static_cast<const float*>(a.src) + (((long long)r * a.T + t) * a.OH + cy) * a.OW + cx0;
    if (a.wide) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = p[k];
    }
  } else {
    const long long plane = (long long)a.Hs * a.Ws;
    const int sx = g.flip ? g.ox + a.OW - 4 - cx0 : g.ox + cx0;            // a flipped quad is the mirrored quad read backwards
    const uint8_t* p = static_cast<const uint8_t*>(a.src) + ((long long)r * a.T + t) * KIND * plane + (long long)(g.oy + cy) * a.Ws + sx;
    uint32_t w[KIND];
#pragma unroll
    for (int c = 0; c < KIND; ++c) w[c] = load4_u8(p + c * plane, a.wide != 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 8 * (g.flip ? 3 - k : k);
      float gray = (float)((w[0] >> e) & 255u);
      if constexpr (KIND == 3) gray = dlip_gray601(gray, (float)((w[1] >> e) & 255u), (float)((w[2] >> e) & 255u));
      v[k] = dlip_pixel_norm(gray);
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void clipaug_mean_kernel(const ClipAug a, double* __restrict__ part) {
  __shared__ double red[4];
  const int b = blockIdx.y, c = blockIdx.x;
  const int n = row_len(a.lengths, b, a.T);
  const int ta = c * kMeanFrames;
  if (ta >= n) {                                                  // (the whole workgroup: no barrier is skipped by some)
    if (threadIdx.x == 0) part[(long long)b * a.chunks + c] = 0.0;
    return;
  }
  const int nf = n - ta < kMeanFrames ? n - ta : kMeanFrames;
  const int quads = a.OH * a.OW / 4;
  const Geo g = clip_geo(a, b);
  double acc = 0.0;
  for (int i = threadIdx.x; i < nf * quads; i += kThreads) {
    const int t = ta + i / quads, q = i % quads;
    float v[4];
    load_quad<KIND>(a, g, b, t, (q * 4) / a.OW, (q * 4) % a.OW, v);
    acc += (((double)v[0] + (double)v[1]) + (double)v[2]) + (double)v[3];
  }
  const double tot = dlip_block_sum4(acc, red);
  if (threadIdx.x == 0) part[(long long)b * a.chunks + c] = tot;
}

// Frame t of A'_r (steps 1-3 of the definition) on the lane's quad.  r, n and t are workgroup-uniform, and so is everything up to the
// lane's own mask bits.
template <int KIND>
__device__ __forceinline__ void operand(const ClipAug& a, int r, int n, int t, int cy, int cx0, float v[4]) {
  const int32_t* dr = a.draws + (long long)r * DLIP_CLIPAUG_DRAWS;
  const int tr = (int)floor(a.time_ratio * (double)n);
  const int tcap = a.time_width < tr ? a.time_width : tr;
  bool tmask = false;
  unsigned m = 0;                                                 // bit k: pixel k of the quad is filled
#pragma unroll
  for (int j = 0; j < kMasks; ++j) {
    if (j < a.n_time) {
      const int w = pick(dr[2 * j], tcap + 1);
      const int t0 = pick(dr[2 * j + 1], n - w + 1);
      tmask = tmask || (t >= t0 && t < t0 + w);
    }
    if (j < a.n_cut) {
      const int32_t* dc = dr + 2 * kMasks + 4 * j;
      const int h0 = pick(dc[0], a.cut_size + 1), w0 = pick(dc[1], a.cut_size + 1);
      const int h = h0 < a.OH ? h0 : a.OH, w = w0 < a.OW ? w0 : a.OW;
      const int y0 = pick(dc[2], a.OH - h + 1), x0 = pick(dc[3], a.OW - w + 1);
      if (cy >= y0 && cy < y0 + h) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m |= (cx0 + k >= x0 && cx0 + k < x0 + w) ? 1u << k : 0u;
      }
    }
  }
  if (tmask) m = 15u;
  float fillv = 0.f;
  if (a.fill == 1) {
    const int used = (n + kMeanFrames - 1) / kMeanFrames;
    double tot = 0.0;
    for (int c = 0; c < used; ++c) tot += a.part[(long long)r * a.chunks + c];
    fillv = (float)(tot / ((double)n * (double)a.OH * (double)a.OW));
  }
  if (m == 15u) {                                                 // filled whole: nothing of the source is read
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fillv;
    return;
  }
  load_quad<KIND>(a, clip_geo(a, r), r, t, cy, cx0, v);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (m >> k) & 1u ? fillv : v[k];
}

template <int KIND>
__global__ __launch_bounds__(kThreads) void clipaug_write_kernel(const ClipAug a) {
  const int b = blockIdx.z, t = blockIdx.y;
  const int quads = a.OH * a.OW / 4;
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= quads) return;
  float4* yo = reinterpret_cast<float4*>(a.y) + ((long long)b * a.T + t) * quads + q;
  const int n = row_len(a.lengths, b, a.T);
  if (t >= n) {                                                   // the zero tail of the clip
    *yo = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int cy = (q * 4) / a.OW, cx0 = (q * 4) % a.OW;
  float v[4];
  operand<KIND>(a, b, n, t, cy, cx0, v);
  if (a.perm != nullptr && a.lam != nullptr) {
    const int p = a.perm[b];
    if (p >= 0 && p < a.B && p != b) {                            // anything else: no partner, the clip is stored unblended
      float u[4] = {0.f, 0.f, 0.f, 0.f};
      const int np = row_len(a.lengths, p, a.T);
      if (t < np) operand<KIND>(a, p, np, t, cy, cx0, u);
      const float lam = a.lam[0];
      {
#pragma clang fp contract(off)
        const float mu = 1.0f - lam;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (lam * v[k]) + (mu * u[k]);
      }
    }
  }
  *yo = make_float4(v[0], v[1], v[2], v[3]);
}

inline bool sizes_ok(long long B, long long T, long long OH, long long OW) {
  return B >= 1 && B <= 65535 && T >= 1 && T <= 65535 && OH >= 1 && OW >= 4 && OW % 4 == 0 && OH * OW <= (1ll << 30);
}

template <int KIND>
int launch(ClipAug a, void* workspace, hipStream_t st) {
  const int quads = a.OH * a.OW / 4;
  if (a.fill == 1) {
    hipLaunchKernelGGL(clipaug_mean_kernel<KIND>, dim3(a.chunks, a.B), dim3(kThreads), 0, st, a, static_cast<double*>(workspace));
  }
  hipLaunchKernelGGL(clipaug_write_kernel<KIND>, dim3((quads + kThreads - 1) / kThreads, a.T, a.B), dim3(kThreads), 0, st, a);
  return dlip_launch_status();
}

int check_common(const void* src, const int32_t* draws, const int32_t* perm, const float* lam, float* y, void* workspace,
                 int64_t workspace_bytes, int32_t B, int32_t T, int32_t n_time, int32_t time_width, double time_ratio, int32_t n_cut,
                 int32_t cut_size, int32_t fill) {
  DLIP_CHECK_ARG(src && draws && y && src != (const void*)y && dlip_aligned16(y));
  DLIP_CHECK_ARG((perm == nullptr) == (lam == nullptr));
  DLIP_CHECK_ARG(n_time >= 0 && n_time <= kMasks && n_cut >= 0 && n_cut <= kMasks && time_width >= 0 && cut_size >= 0 && cut_size <= (1 << 30));
  DLIP_CHECK_ARG(time_ratio >= 0.0 && time_ratio <= 1.0 && (fill == 0 || fill == 1));      // (a NaN ratio fails both comparisons)
  DLIP_CHECK_ARG(workspace && dlip_aligned<8>(workspace) && workspace_bytes >= dlip_clip_augment_workspace_bytes(B, T));
  return DLIP_OK;
}

}  // namespace

extern "C" int64_t dlip_clip_augment_workspace_bytes(int32_t B, int32_t T) {
  if (B < 1 || B > 65535 || T < 1 || T > 65535) return DLIP_EINVAL;
  return (int64_t)B * ((T + kMeanFrames - 1) / kMeanFrames) * (int64_t)sizeof(double);
}

extern "C" int dlip_clip_augment_u8(const uint8_t* frames, const int32_t* clip_params, const int32_t* lengths, const int32_t* draws,
                                    const int32_t* perm, const float* lam, float* y, void* workspace, int64_t workspace_bytes, int32_t B,
                                    int32_t T, int32_t channels, int32_t Hs, int32_t Ws, int32_t crop, int32_t n_time, int32_t time_width,
                                    double time_ratio, int32_t n_cut, int32_t cut_size, int32_t fill, dlip_stream_t stream) {
  DLIP_CHECK_ARG(sizes_ok(B, T, crop, crop) && (channels == 1 || channels == 3) && Hs >= crop && Ws >= crop);
  DLIP_CHECK_ARG((long long)Hs * Ws <= (1ll << 30));
  if (int rc = check_common(frames, draws, perm, lam, y, workspace, workspace_bytes, B, T, n_time, time_width, time_ratio, n_cut, cut_size,
                            fill))
    return rc;
  const long long bytes = (long long)B * T * channels * Hs * Ws;
  ClipAug a{frames, clip_params, lengths, draws, perm, lam, static_cast<const double*>(workspace), y, B, T, Hs, Ws, crop, crop,
            (T + kMeanFrames - 1) / kMeanFrames, n_time, time_width, n_cut, cut_size, fill, time_ratio,
            dlip_aligned<4>(frames) && bytes % 4 == 0};
  return channels == 3 ? launch<3>(a, workspace, dlip_hip_stream(stream)) : launch<1>(a, workspace, dlip_hip_stream(stream));
}

extern "C" int dlip_clip_augment_f32(const float* x, const int32_t* lengths, const int32_t* draws, const int32_t* perm, const float* lam,
                                     float* y, void* workspace, int64_t workspace_bytes, int32_t B, int32_t T, int32_t H, int32_t W,
                                     int32_t n_time, int32_t time_width, double time_ratio, int32_t n_cut, int32_t cut_size, int32_t fill,
                                     dlip_stream_t stream) {
  DLIP_CHECK_ARG(sizes_ok(B, T, H, W));
  if (int rc = check_common(x, draws, perm, lam, y, workspace, workspace_bytes, B, T, n_time, time_width, time_ratio, n_cut, cut_size, fill))
    return rc;
  ClipAug a{x, nullptr, lengths, draws, perm, lam, static_cast<const double*>(workspace), y, B, T, H, W, H, W,
            (T + kMeanFrames - 1) / kMeanFrames, n_time, time_width, n_cut, cut_size, fill, time_ratio, dlip_aligned16(x)};
  return launch<0>(a, workspace, dlip_hip_stream(stream));
}

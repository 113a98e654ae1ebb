// Split-fp16 convolution, ROWS variant: convolutions whose every tap is a plain row offset of the activation matrix --
// the 1-D "valid" convolutions of the speech encoder (models/audio_models/tdnn.py:23-43: Conv1d over time, no padding,
// dilation from the context list) and, with one tap, its k = 1 layers: plain [M x C] . [C x K] GEMMs over the B * T' frames.
//
// Why a third kernel.  On the ring kernel (conv_igemm_f16x3_dma.hip) the k = 1 layers -- 16 slices of 32 channels per
// tile -- ran at 0.21 of the split-fp16 ceiling for three rounds: a third of every 128 x 128 tile was set-up, first fills
// and epilogue around a 16-slice loop (in-kernel stamps: 7.8 k + 9.9 k of 52 k cycles), and 592 tiles on 512 slots made a
// second round that was 16 % full.  What such a layer needs is (1) more matrix work behind every barrier and every byte,
// (2) one round, (3) nothing between two tiles.  So:
//   * tile = (32 MI) x 256, MI = 5 | 4 | 3: eight waves (2 x 4), a wave owns 16 MI x 64 outputs = 4 MI accumulator quads
//     (80 registers at MI = 5).  Per 32-channel slice a workgroup moves (160 + 256) x 128 B = 52 KB for 60 MFMAs per
//     wave (the 256 x 128 ring tile: 48 KB for 48); the host picks MI so that rows x column blocks fill ONE round of the
//     chip's CUs where it can (B = 64, T' = 296: 119 x 2 = 238 tiles of 160 x 256 on 256 CUs).
//   * ONE persistent workgroup per CU walks its tiles with a CONTINUOUS slice stream: "two slices ahead" of a tile's last
//     slices are the next tile's first ones, the LDS ring never drains, and no barrier joins the waves between tiles.
//   * the epilogue goes from the accumulator registers straight to memory -- no LDS image, so the ring is not touched
//     (that is what let the stream run on; the ring kernel stages its output tile in the ring).  A split-format output
//     needs 16-B pieces: v_permlane16_swap_b32 exchanges the odd 16-lane rows of one accumulator with the even rows of
//     its neighbour in the channel direction, after which a lane holds 8 consecutive channels of its pixel = one 16-B
//     piece of hi halves and one of lo halves.  Each half of the waves runs a tile's epilogue at the head of its next LOAD
//     interval, i.e. beside its SIMD partner's matrix phase.
//   * main loop: the ring kernel's PING-PONG (its 256 x 128 instance): waves 0-3 and 4-7 -- one wave of every SIMD in each
//     half -- work on the same slice half a period apart, two barriers per slice; one half multiplies (60 MFMAs, nothing
//     else in its stream) while the other reads the 18 fragments of its next matrix phase, issues its LDS-DMA pieces
//     two slices ahead and waits for the pieces of the next slice.
// Arithmetic, slice order (channel slice outer, tap inner), product order per accumulator (lo*hi, hi*hi, hi*lo) and
// epilogue formula are the ring kernel's: a launch that the ring kernel runs as a plain (un-split) launch gives the
// same bits here (tests/test_kernels_gpu.py::test_conv_rows_*).
#include "conv_common.h"
#include "conv_dma_common.h"
#include "conv_dispatch.h"
#include "dlip_launch.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct RowsSched {
  int items;      // tiles of the launch: tiles_m * tiles_n, row block major (the column blocks of a row block are neighbours)
  int tiles_n;
  unsigned long long* span;   // NULL, or this launch's {first start, last end} in 100 MHz ticks (dlip_span_scope_*)
  // (round 5) the SHORT LAST ROUND: row tiles t_full.. (items item_short0..) are 32 * nmi_short rows high instead of 32 MI, so
  // that the rows left over after the launch's full rounds of tiles spread over ALL workgroups as one round of shorter tiles (B = 256:
  // 948 tiles of 160 rows on 256 CUs = 3 full rounds + a fourth that is 70 % full -> 3 rounds + one of 128-row tiles: 3.8 tile
  // times instead of 4).  A short tile keeps the LDS image of a full one: its wave row w holds rows w * 16 nmi_short .. of the tile
  // in LDS rows w * 16 MI ..; the rest of the image is not fetched (out-of-range offsets), not multiplied and not stored.
  // No short tiles: item_short0 = t_full = INT_MAX.
  int item_short0, t_full, nmi_short, row_short0;
#ifdef DLIP_LAB
  unsigned long long* stamps;
#endif
};

constexpr int ROWS_BN = 256;

// The kernel's RowsSched as the kernarg segment holds it (second explicit argument: at the next 8-byte boundary behind ConvArgs),
// behind an opaque asm: what is read through this pointer is (re)loaded where it is used -- scalar loads, once per tile -- instead
// of being kept in scalar registers for the whole kernel.
typedef const RowsSched __attribute__((address_space(4))) RowsKSched;
__device__ __forceinline__ RowsKSched* rows_ksched() {
  typedef const char __attribute__((address_space(4))) KChar;
  KChar* p = (KChar*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return (RowsKSched*)(p + ((sizeof(ConvArgs) + 7) & ~(size_t)7));
}

// EPI: 0 fp32 rows of y; 1 split-format rows of y (reports range); 2 no y: per HALF tile (the 16 MI rows of a wave row) and
// row-group segment the fp64 column sums of v and v^2 (a.pool, the ring kernel's pooled epilogue with tile rows = 16 MI)
// TAIL: the launch has a short last round (RowsSched); instances without it carry none of its code.
template <int MI, int EPI, bool TAIL = false>
__global__ __launch_bounds__(512, 2) void conv_rows_f16x3_kernel(const ConvArgs a, const RowsSched sc) {
  static_assert(!TAIL || EPI != 2, "short tiles: fp32 or split output");
  // (TAIL) the four schedule words are re-read from the kernel-argument segment (scalar loads) where a tile begins or ends: held in
  // scalar registers across the main loop they cost the split-output instances 40 SGPR spills and the B = 64 step 1 % (the
  // paired-lanes lesson again)
#define ROWS_SC(f) (rows_ksched()->f)
  constexpr int NW = 8, BN = ROWS_BN, BM = 32 * MI, NI = 4;
  constexpr int WM = BM / 2;                       // rows of a wave's tile (16 MI); WN = 64
  constexpr int A_PIECES = BM / 8, B_PER = 4;      // 1-KiB pieces of a slice's activation rows; weight pieces per wave
  constexpr int NA_A = (A_PIECES + 7) / 8, NA_B = A_PIECES / 8;   // activation pieces of a wave of half A (waves 0-3) / B (4-7)
  static_assert(A_PIECES % 8 == 0 || A_PIECES % 8 == 4, "waves 0-3 take one activation piece more than waves 4-7, or the same");
  constexpr int STAGE_B = (BM + BN) * ROWB, NSTAGE = 3;
  constexpr int LDK = 32;
  // output stores per lane and tile that the counted waits behind an epilogue may leave in flight: a LOWER bound of what the
  // epilogue issues (a larger number would let the wait return before the next slice's pieces have landed).  The pooled
  // epilogue's few stores are issued under lane masks: not counted, i.e. waited for.
  constexpr int NST = EPI == 1 ? MI * 4 : EPI == 0 ? MI * NI : 0;
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  const int g = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);   // neighbours in tile order share an XCD (L2)
  const int nk = a.nk;
  if (g >= sc.items) return;
  const int item0 = g;                                    // this workgroup's tiles: g, g + nwg, ...
  const int total = ((sc.items - g + nwg - 1) / nwg) * nk;   // slices of its stream

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const bool half_b = wave >= NW / 2;                     // (wave-uniform)
  const int wm = wave >> 2, wn = wave & 3;
  const int lrow = lane & 15, hq = lane >> 4;
  // DMA side: piece q = wave + 8 j covers tile rows 8 q .. 8 q + 7; lane -> (row lane >> 3, chunk position lane & 7); the XOR
  // swizzle of the LDS image (chunk p of row r at position p ^ ((r >> 1) & 7)) goes on the SOURCE chunk, and since
  // 4 q mod 8 is the same for every piece of a wave the key is a per-lane constant.
  const int prow = lane >> 3;
  const int key_st = (4 * (wave & 1) + (lane >> 4)) & 7;
  const int csrc = ((lane & 7) ^ key_st) << 2;            // first channel (dword) of the chunk this lane fetches
  const u32x4 xr = make_rsrc_words(a.x, a.x_bytes);
  const u32x4 wr = make_rsrc_words(a.w, a.w_bytes);
  // LEFT OVER from the retired general mode (EXPERIMENTS.md R8.2), with the dead branch of `issue`, the epilogue's local copies and
  // five unused variables of `run_half` below: nothing reads or runs them, but taking them out changes which variables the lambdas
  // capture, with that the order in which the optimiser creates the loop's phi nodes, and with that the schedule and the scalar
  // spills of all fifteen instances (fp32 output at MI = 5: 20 -> 48 spills).  They leave with the next change that is allowed to
  // move this kernel's machine code.
  constexpr bool DUAL = false;
  u32x4 x2r = xr;
  if constexpr (DUAL) x2r = make_rsrc_words(a.x2, a.x2_bytes);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const uint32_t piece0 = lds0 + wave * 1024;
  // fragment side (v_mfma_f32_16x16x32_f16; the weight fragment is the A operand: accumulators hold the transposed tile)
  const int a_frag = (wm * WM + lrow) * LDK;
  const int b_frag = BM * LDK + (wn * 64 + lrow) * LDK;
  const int key_rd = (lrow >> 1) & 7;
  const int khi = (hq ^ key_rd) << 2, klo = ((4 + hq) ^ key_rd) << 2;
  const int x_ds = a.dw * a.ldx * 4;                      // bytes between two taps of a row

  dlip_span_enter(sc.span, g);
#ifdef DLIP_LAB
#define ROWS_STAMP(i) do { if (sc.stamps && tid == 0) sc.stamps[(size_t)g * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define ROWS_SSTAMP(i) do { if (sc.stamps && tid == 0 && s == 8) sc.stamps[(size_t)g * 16 + 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
  if (sc.stamps && tid == 0) sc.stamps[(size_t)g * 16 + 7] = __builtin_amdgcn_s_memrealtime();
#else
#define ROWS_STAMP(i) do { } while (0)
#define ROWS_SSTAMP(i) do { } while (0)
#endif

  // ---- issue cursor: the slice the NEXT pieces belong to (two slices ahead of the one being multiplied) ----
  // (rows past M / weight rows past K carry the out-of-range offset itself: 2^31 plus any in-range tap offset is still beyond every
  // buffer, so a piece's address is ONE add -- the select per piece was two of every three vector instructions of a slice)
  uint32_t a_off[NA_A], b_off[B_PER];
  uint32_t a2_off[DUAL ? NA_A : 1];                       // (left over, see DUAL)
  int c_item = item0, c_k = 0, s_pos = 0, c0 = 0, x_tap = 0, w_tap = 0;
  auto set_item = [&](int item) __attribute__((always_inline)) {
    const int tile_m = item / sc.tiles_n, tile_n = item - tile_m * sc.tiles_n;
    [[maybe_unused]] int t_base = tile_m * BM, t_half = WM;   // the tile's first row, rows per wave row (RowsSched: short last round)
    if constexpr (TAIL) {
      if (item >= ROWS_SC(item_short0)) { t_half = 16 * ROWS_SC(nmi_short); t_base = ROWS_SC(row_short0) + (tile_m - ROWS_SC(t_full)) * 2 * t_half; }
    }
#pragma unroll
    for (int j = 0; j < NA_A; ++j) {
      const int lr = 8 * (wave + 8 * j) + prow;              // row of the LDS image; hr: within its wave row
      const int hr = lr >= WM ? lr - WM : lr;
      const int ms = t_base + (lr >= WM ? t_half : 0) + hr;
      const bool in = hr < t_half && ms < a.M;
      const int mc = in ? ms : 0;
      const int n = dlip_div(mc, a.div_howo);
      const int t = mc - n * a.HoWo;                         // H = 1: the row's first input pixel is n * W + t
      a_off[j] = in ? (uint32_t)(((n * a.W + t) * a.ldx + csrc) * 4) : DLIP_OOB_OFFSET;
    }
#pragma unroll
    for (int j = 0; j < B_PER; ++j) {
      const int n = tile_n * BN + 8 * (wave + 8 * j) + prow;
      b_off[j] = n < a.K ? (uint32_t)((n * a.rsc + csrc) * 4) : DLIP_OOB_OFFSET;
    }
  };
  auto advance = [&]() __attribute__((always_inline)) {   // channel slice outer, tap inner (the ring kernel's reduction order)
    if (++c_k == nk) {
      c_k = 0; s_pos = 0; c0 = 0;
      c_item += nwg;
      set_item(c_item);
    } else if (++s_pos == a.S) {
      s_pos = 0; c0 += BK;
    }
    x_tap = s_pos * x_ds + c0 * 4;
    w_tap = (s_pos * a.Cw + c0) * 4;
  };
  auto issue = [&](int stage, auto na) __attribute__((always_inline)) {
    const uint32_t base = piece0 + stage * STAGE_B;
    if (DUAL && c0 >= a.Cw) {                              // (left over, see DUAL: never taken)
#pragma unroll
      for (int j = 0; j < na(); ++j)
        dma_piece(x2r, a2_off[DUAL ? j : 0] + (uint32_t)x_tap, base + j * 8192);
    } else {
#pragma unroll
      for (int j = 0; j < na(); ++j) {
        dma_piece(xr, a_off[j] + (uint32_t)x_tap, base + j * 8192);
      }
    }
#pragma unroll
    for (int j = 0; j < B_PER; ++j)
      dma_piece(wr, b_off[j] + (uint32_t)w_tap, base + BM * ROWB + j * 8192);
  };

  f32x4 acc[MI][NI];
  f16x8 fal[MI], fah[MI], fbh[NI], fbl[NI];
#define DLIP_FENCE() __builtin_amdgcn_sched_barrier(0)
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[mi][ni][e] = 0.f;
  };
  auto read_all = [&](int stage) __attribute__((always_inline)) {
    const float* Aw = smem + stage * (STAGE_B / 4) + a_frag;
    const float* Bw = smem + stage * (STAGE_B / 4) + b_frag;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) fal[mi] = *reinterpret_cast<const f16x8*>(Aw + mi * 16 * LDK + klo);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) fbh[ni] = *reinterpret_cast<const f16x8*>(Bw + ni * 16 * LDK + khi);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) fah[mi] = *reinterpret_cast<const f16x8*>(Aw + mi * 16 * LDK + khi);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) fbl[ni] = *reinterpret_cast<const f16x8*>(Bw + ni * 16 * LDK + klo);
  };
  auto mfma_all = [&](int nmi) __attribute__((always_inline)) {   // nmi (wave-uniform): 16-row blocks of this wave's rows that exist
    __builtin_amdgcn_s_setprio(2);   // the matrix phase outranks its SIMD partner's load phase
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      // (TAIL) a tile of the short last round skips the blocks it does not have: one scalar compare-and-branch per block
      if (!TAIL || mi < nmi) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {   // accumulator-major: the three products of one accumulator back to back (ring kernel)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[ni], fal[mi], acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[ni], fah[mi], acc[mi][ni], 0, 0, 0);
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbl[ni], fah[mi], acc[mi][ni], 0, 0, 0);
        }
      }
      DLIP_FENCE();
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // ---- epilogue of one tile, from this wave's accumulators straight to memory:
  //      y = act(acc / wscale + bias) * post_scale + post_shift ----
  // (The descriptors are built once, here -- plain scalars, as the compiler keeps them best.  An aggregate carrying them into the
  // epilogue cost the speech-encoder layers 2 - 4 %: it lived in vector registers and came back through v_readfirstlane + hazard
  // s_nops, same-box A/B at B = 256.)
  const uint32_t kbytes0 = (uint32_t)a.K * 4u;
  const __amdgpu_buffer_rsrc_t yr0 = dlip_make_rsrc(a.y, a.y_bytes);
  const __amdgpu_buffer_rsrc_t scr0 = dlip_make_rsrc(a.wscale, kbytes0);
  const __amdgpu_buffer_rsrc_t bir0 = dlip_make_rsrc(a.bias, a.bias ? kbytes0 : 0u);
  const __amdgpu_buffer_rsrc_t slr0 = dlip_make_rsrc(a.slope, a.slope ? kbytes0 : 0u);
  const __amdgpu_buffer_rsrc_t psr0 = dlip_make_rsrc(a.pscale, a.pscale ? kbytes0 : 0u);
  const __amdgpu_buffer_rsrc_t ptr0 = dlip_make_rsrc(a.pshift, a.pshift ? kbytes0 : 0u);
  const bool has_slope0 = a.slope != nullptr;
  const bool has_post0 = a.pscale != nullptr;
  float amax = 0.f;
  // (round 5) fp32 / split output: the epilogue's per-channel parameters {1 / wscale, bias, slope} of this workgroup's column
  // block, 3 KB of LDS behind the ring, written once.  A workgroup's tiles g, g + G, ... share their column block whenever the column
  // blocks divide G (K = 512: two blocks on 256 workgroups), and the epilogue took them from memory per tile: two dependent L2 round
  // trips (~2.4 k cycles) at the head of the interval in which its SIMD partner multiplies for 1.1 k -- in-kernel stamps at B = 256:
  // 16 x 2 632 cycles of slices per k = 1 tile, but 60.6 k per tile, the difference being the two halves' epilogues each stalling the
  // other.  A tile of another column block (tab_n differs) takes the parameters from memory as before.
  constexpr bool TAB = EPI != 2;
  float* const ptab = smem + NSTAGE * (STAGE_B / 4);
  [[maybe_unused]] int tab_n = -1;
  if constexpr (TAB) {
    tab_n = __builtin_amdgcn_readfirstlane(item0 - (item0 / sc.tiles_n) * sc.tiles_n);
    if (tid < BN) {
      const int k = tab_n * BN + tid;
      float iv = 0.f, bv = 0.f, sv = 1.f;
      if (k < a.K) {
        iv = 1.f / a.wscale[k];                       // power of two: exact
        if (a.bias) bv = a.bias[k];
        if (a.slope) sv = a.slope[k];
      }
      ptab[tid] = iv; ptab[BN + tid] = bv; ptab[2 * BN + tid] = sv;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // landed before this wave reaches the first barrier of the loop
    }
  }
  auto epilogue_p = [&](int item, auto post_c) __attribute__((always_inline)) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    constexpr bool post = decltype(post_c)::value;   // (compile-time inside: the runtime flag selected and computed both forms per value)
    // (local copies: left over, see DUAL -- the general mode re-read these from the kernel arguments here)
    __amdgpu_buffer_rsrc_t yr = yr0, scr = scr0, bir = bir0, slr = slr0, psr = psr0, ptr_ = ptr0;
    bool has_slope = has_slope0;
    int eM = a.M, eK = a.K, eldy = a.ldy;
    const int tile_m = item / sc.tiles_n, tile_n = item - tile_m * sc.tiles_n;
    int row0 = tile_m * BM + wm * WM + lrow;
    [[maybe_unused]] int e_nmi = MI;                  // (TAIL) 16-row blocks of this wave's rows that exist (short last round)
    if constexpr (TAIL) {
      if (item >= ROWS_SC(item_short0)) { e_nmi = ROWS_SC(nmi_short); row0 = ROWS_SC(row_short0) + ((tile_m - ROWS_SC(t_full)) * 2 + wm) * 16 * e_nmi + lrow; }
    }
    const int col0 = tile_n * BN + wn * 64;
    if constexpr (EPI == 1) {
      // after the swap, 16-lane row hq of the pair (2 p, 2 p + 1) holds channels 32 p + {0, 16, 8, 24}[hq] + 0..7 of its pixel
      const int cs = ((hq & 1) << 4) | ((hq & 2) << 2);
#pragma unroll
      for (int p = 0; p < NI / 2; ++p) {
        const int kb = col0 + 32 * p;                    // first channel of the 32-channel block
        const int k0 = kb + cs;                          // first of this lane's 8 channels
        float inv[8], bi[8], sl[8], ps[8], pt[8];
        bool from_tab = false;
        if constexpr (TAB && !post) from_tab = tile_n == tab_n;      // (wave-uniform)
        if (from_tab) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const float* tp = ptab + wn * 64 + 32 * p + cs + 4 * q;
            const f32x4 i4 = *reinterpret_cast<const f32x4*>(tp), b4 = *reinterpret_cast<const f32x4*>(tp + BN);
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(tp + 2 * BN);
#pragma unroll
            for (int c = 0; c < 4; ++c) { inv[4 * q + c] = i4[c]; bi[4 * q + c] = b4[c]; sl[4 * q + c] = l4[c]; ps[4 * q + c] = 1.f; pt[4 * q + c] = 0.f; }
          }
        } else {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const f32x4 s4 = dlip_buffer_load_f4(scr, (uint32_t)(k0 + 4 * q) * 4u);
            const f32x4 b4 = dlip_buffer_load_f4(bir, (uint32_t)(k0 + 4 * q) * 4u);
            f32x4 l4 = {1.f, 1.f, 1.f, 1.f}, p4 = {1.f, 1.f, 1.f, 1.f}, t4 = {0.f, 0.f, 0.f, 0.f};
            if (has_slope) l4 = dlip_buffer_load_f4(slr, (uint32_t)(k0 + 4 * q) * 4u);
            if (post) { p4 = dlip_buffer_load_f4(psr, (uint32_t)(k0 + 4 * q) * 4u); t4 = dlip_buffer_load_f4(ptr_, (uint32_t)(k0 + 4 * q) * 4u); }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              inv[4 * q + c] = k0 + 4 * q + c < eK ? 1.f / s4[c] : 0.f;   // power of two: exact
              bi[4 * q + c] = b4[c]; sl[4 * q + c] = l4[c]; ps[4 * q + c] = p4[c]; pt[4 * q + c] = t4[c];
            }
          }
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          float v[8];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            // (__float_as_uint of a scalar copy: __builtin_bit_cast applied to the vector ELEMENT expression acc[..][c] makes this
            // clang read element 0 for every c -- tools/probes/permlane16_swap.hip)
            const float xc = acc[mi][2 * p][c], yc = acc[mi][2 * p + 1][c];
            const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(xc), __float_as_uint(yc), false, false);
            v[c] = __uint_as_float(r[0]);
            v[4 + c] = __uint_as_float(r[1]);
          }
          h8 hi, lo;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            float t = v[c] * inv[c] + bi[c];
            t = t >= 0.f ? t : t * sl[c];
            if (post) t = t * ps[c] + pt[c];
            hi[c] = (_Float16)t;
            lo[c] = (_Float16)(t - (float)hi[c]);
            amax = fmaxf(amax, fabsf(t));
          }
          const int m = row0 + mi * 16;
          const bool ok = m < eM && k0 < eK && (!TAIL || mi < e_nmi);   // K % 32 == 0 for a split output: a block is whole or absent
          const uint32_t off = ok ? (uint32_t)((m * eldy + kb) * 4 + cs * 2) : DLIP_OOB_OFFSET;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), yr, (int)off, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), yr, (int)(ok ? off + 64u : DLIP_OOB_OFFSET), 0, 0);
        }
        DLIP_FENCE();
      }
    } else if constexpr (EPI == 2) {
      // Pooled: nothing is written but, per wave ROW (its 16 MI rows are one "tile" of the partials: tile index 2 tile_m + wm) and
      // row-group segment, the column sums of v and v^2 -- fp64, fixed order: a lane adds its MI pixels, the 16 lanes of a
      // channel quad meet by butterfly, lane 0 of each quad stores.  Rows before the half tile's one possible group boundary
      // are segment 0, the rest segment 1 (pool_group >= 16 MI); dlip_pool_finish_f32 / znorm_cat_pooled add the tiles in row order.
      const int m0 = tile_m * BM + wm * WM;
      const int g0 = m0 / a.pool_group;
      const int rb = (g0 + 1) * a.pool_group - m0;
      int e0 = rb, e1 = WM;                           // ragged batches: tile-relative ends of the valid rows of the two segments
      if (a.pool_len.len != nullptr) {
        const int G = (eM + a.pool_group - 1) / a.pool_group;
        e0 = min(rb, g0 * a.pool_group + dlip_valid_rows(a.pool_len, g0, a.pool_group) - m0);
        e1 = g0 + 1 < G ? rb + dlip_valid_rows(a.pool_len, g0 + 1, a.pool_group) : rb;
      }
      const int Kp = (eK + 127) / 128 * 128;
      double* prow = a.pool + (size_t)(2 * tile_m + wm) * 4 * Kp;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int k0 = col0 + 16 * ni + 4 * hq;
        const f32x4 s4 = dlip_buffer_load_f4(scr, (uint32_t)k0 * 4u);
        const f32x4 b4 = dlip_buffer_load_f4(bir, (uint32_t)k0 * 4u);
        f32x4 l4 = {1.f, 1.f, 1.f, 1.f}, p4 = {1.f, 1.f, 1.f, 1.f}, t4 = {0.f, 0.f, 0.f, 0.f};
        if (has_slope) l4 = dlip_buffer_load_f4(slr, (uint32_t)k0 * 4u);
        if (post) { p4 = dlip_buffer_load_f4(psr, (uint32_t)k0 * 4u); t4 = dlip_buffer_load_f4(ptr_, (uint32_t)k0 * 4u); }
        f32x4 inv4;
#pragma unroll
        for (int c = 0; c < 4; ++c) inv4[c] = k0 + c < eK ? 1.f / s4[c] : 0.f;
        double st[4][4];   // [sum0, sumsq0, sum1, sumsq1][channel]
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int c = 0; c < 4; ++c) st[q][c] = 0.0;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const int r = mi * 16 + lrow;
          const bool seg1 = r >= rb, in = m0 + r < eM && r < (seg1 ? e1 : e0);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float t = acc[mi][ni][c] * inv4[c] + b4[c];
            t = t >= 0.f ? t : t * l4[c];
            if (post) t = t * p4[c] + t4[c];
            const double d = in ? (double)t : 0.0;
            st[0][c] += seg1 ? 0.0 : d; st[1][c] += seg1 ? 0.0 : d * d;
            st[2][c] += seg1 ? d : 0.0; st[3][c] += seg1 ? d * d : 0.0;
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) st[q][c] += __shfl_xor(st[q][c], o, 64);
        if (lrow == 0 && m0 < eM) {   // (a last tile's second half may lie wholly beyond M: it has no partial row set)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (k0 + c < Kp) prow[(size_t)q * Kp + k0 + c] = st[q][c];
        }
        DLIP_FENCE();
      }
    } else {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int k0 = col0 + 16 * ni + 4 * hq;
        f32x4 b4, inv4, l4 = {1.f, 1.f, 1.f, 1.f}, p4 = {1.f, 1.f, 1.f, 1.f}, t4 = {0.f, 0.f, 0.f, 0.f};
        bool from_tab = false;
        if constexpr (TAB && !post) from_tab = tile_n == tab_n;      // (wave-uniform: the parameter table in LDS, see ptab)
        if (from_tab) {
          const float* tp = ptab + wn * 64 + 16 * ni + 4 * hq;
          inv4 = *reinterpret_cast<const f32x4*>(tp); b4 = *reinterpret_cast<const f32x4*>(tp + BN); l4 = *reinterpret_cast<const f32x4*>(tp + 2 * BN);
        } else {
          const f32x4 s4 = dlip_buffer_load_f4(scr, (uint32_t)k0 * 4u);
          b4 = dlip_buffer_load_f4(bir, (uint32_t)k0 * 4u);
          if (has_slope) l4 = dlip_buffer_load_f4(slr, (uint32_t)k0 * 4u);
          if (post) { p4 = dlip_buffer_load_f4(psr, (uint32_t)k0 * 4u); t4 = dlip_buffer_load_f4(ptr_, (uint32_t)k0 * 4u); }
#pragma unroll
          for (int c = 0; c < 4; ++c) inv4[c] = k0 + c < eK ? 1.f / s4[c] : 0.f;
        }
        // (a.stats: launch-uniform) column sums of what this wave writes -- the batch statistics of the BatchNorm behind a
        // TDNN convolution under model.train() (tdnn.py:35-43) -- taken here instead of by a pass over y: a lane adds its MI pixels
        // (fp32: 5 values), the 16 lanes of a channel quad meet by four DPP row steps (fp32, a fixed tree: deterministic), lane 0 of
        // the quad converts to fp64 and stores {sum, sum of squares} of its 4 channels for chunk 2 tile_m + wm; the finalize kernel
        // adds the chunks in fp64 as it adds col_partial_kernel's.  80 values per fp32 sum: 5e-7 relative per chunk, random over
        // ~10^3 chunks.
        float st_s[4] = {0.f, 0.f, 0.f, 0.f}, st_q[4] = {0.f, 0.f, 0.f, 0.f};
        // (the pointer is re-read from the kernel arguments HERE: held in scalar registers across the main loop it cost the fp32
        // instances 30 extra SGPR spills -- the paired-lanes lesson of conv_igemm_f16x3_dma.hip)
        double* const stats_p = *reinterpret_cast<double* const volatile*>(&a.stats);
        const bool want_stats = stats_p != nullptr;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          f32x4 v;
          const int m = row0 + mi * 16;
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = acc[mi][ni][c] * inv4[c] + b4[c];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float t = v[c];
            t = t >= 0.f ? t : t * l4[c];
            if (post) t = t * p4[c] + t4[c];
            v[c] = t;
          }
          if (want_stats && m < eM && (!TAIL || mi < e_nmi)) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { st_s[c] += v[c]; st_q[c] += v[c] * v[c]; }
          }
          const uint32_t off = (m < eM && k0 < eK && (!TAIL || mi < e_nmi)) ? (uint32_t)((m * eldy + k0) * 4) : DLIP_OOB_OFFSET;   // K % 4 == 0
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yr, (int)off, 0, 0);
        }
        if (want_stats) {
          auto row_sum = [](float x) {   // the sum over the 16 lanes of a DPP row, in every lane: xor 1, xor 2, half mirror, mirror
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xf, 0xf, true));
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xf, 0xf, true));
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xf, 0xf, true));
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xf, 0xf, true));
            return x;
          };
#pragma unroll
          for (int c = 0; c < 4; ++c) { st_s[c] = row_sum(st_s[c]); st_q[c] = row_sum(st_q[c]); }
          if (lrow == 0 && k0 < eK) {
            double* dst = stats_p + ((size_t)(2 * tile_m + wm) * eK + k0) * 2;
#pragma unroll
            for (int c = 0; c < 4; ++c) { dst[2 * c] = (double)st_s[c]; dst[2 * c + 1] = (double)st_q[c]; }
          }
        }
        DLIP_FENCE();
      }
    }
  };
  auto epilogue = [&](int item) __attribute__((always_inline)) {
    bool has_post = has_post0;
    if (has_post) epilogue_p(item, std::true_type{}); else epilogue_p(item, std::false_type{});
  };

  // ---- prologue: the first two slices of the stream in flight ----
  constexpr std::integral_constant<int, NA_A> na_a{};
  constexpr std::integral_constant<int, NA_B> na_b{};
  set_item(c_item);
  ROWS_STAMP(0);
  if (!half_b) issue(0, na_a); else issue(0, na_b);
  if (total > 1) {
    advance();
    if (!half_b) issue(1, na_a); else issue(1, na_b);
  }
  zero_acc();

  // One half of the ping-pong loop; NL = this half's pieces per slice, FIRST = half A (reads a slice first).
  //   interval between barriers   b(2s-1) .. b(2s)      |  b(2s) .. b(2s+1)
  //   half A                      [EPI] LOAD(s)         |  MFMA(s), wait slice s+1
  //   half B                      MFMA(s-1)             |  [EPI] LOAD(s), wait slice s+1
  // LOAD(s): read every fragment of slice s (stage s % 3), issue this wave's pieces of slice s+2 into the stage of slice s-1
  // (whose last reader finished before b(2s-1)), lgkmcnt(0).  [EPI]: when the previous matrix phase finished a tile, its
  // epilogue runs first -- beside the partner's matrix phase -- and its NST stores are then the only vector-memory
  // operations younger than slice s+1's pieces besides slice s+2's: the counted wait leaves them in flight too.
  auto run_half = [&](auto na, auto first_c) __attribute__((always_inline)) {
    constexpr int NL = decltype(na)::value + B_PER;
    constexpr bool FIRST = decltype(first_c)::value;
    static_assert(NL + NST < 64, "vmcnt is a 6-bit counter");
    int st_iss = total > 1 ? 2 : 1;                        // stage the next issue goes to (the prologue issued slices 0, 1)
    // consumer side: the tile being multiplied
    int kleft = nk, e_item = item0, done_item = -1;
    [[maybe_unused]] int cur_nmi = MI;                     // (TAIL) the height of the tile being multiplied, in 16-row blocks per wave
    if constexpr (TAIL) { if (e_item >= ROWS_SC(item_short0)) cur_nmi = ROWS_SC(nmi_short); }
    [[maybe_unused]] int rem = 0;
    [[maybe_unused]] bool e_part = false, e_first = true, done_part = false, done_first = false;   // (left over, see DUAL)
    if (total > 1) wait_vmcnt<NL>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                          // slice 0 is complete
    ROWS_STAMP(1);
    if (!FIRST) __builtin_amdgcn_s_barrier();              // b(0): half A reads slice 0 first
    int st_cur = 0;
    for (int s = 0;; ++s) {
      bool did_epi = false;                                // (wave-uniform)
      ROWS_SSTAMP(0);
      if (done_item >= 0) {
        epilogue(done_item);
        did_epi = true;
        if (s == total) break;                             // the stream ends on a tile's last slice
        zero_acc(); done_item = -1;
      }
      const bool more2 = s + 2 < total;
      DLIP_FENCE();
      read_all(st_cur);                                    // the reads first: their latency passes under the piece issue below
      st_cur = st_cur + 1 == NSTAGE ? 0 : st_cur + 1;
      DLIP_FENCE();
      if (more2) {
        advance();
        issue(st_iss, na);
        st_iss = st_iss + 1 == NSTAGE ? 0 : st_iss + 1;
      }
      DLIP_FENCE();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the stage may be refilled behind the next barrier: the reads are done
      DLIP_FENCE();
      ROWS_SSTAMP(1);
      auto wait_next = [&]() __attribute__((always_inline)) {   // this wave's pieces of slice s + 1 have landed
        if (s + 1 >= total) return;
        if (more2) { if (did_epi) wait_vmcnt<NL + NST>(); else wait_vmcnt<NL>(); }
        else       { if (did_epi) wait_vmcnt<NST>(); else wait_vmcnt<0>(); }
      };
      if (!FIRST) wait_next();                             // half B waits in front of the barrier that opens its matrix phase
      ROWS_SSTAMP(2);
      __builtin_amdgcn_s_barrier();                        // A: b(2s)      B: b(2s+1)
      ROWS_SSTAMP(3);
      mfma_all(cur_nmi);
      ROWS_SSTAMP(4);
      if (--kleft == 0) {
        kleft = nk; done_item = e_item; e_item += nwg;
        if constexpr (TAIL) { if (e_item >= ROWS_SC(item_short0)) cur_nmi = ROWS_SC(nmi_short); }
      }
      if (FIRST) {
        __builtin_amdgcn_s_barrier();                      // b(2s+1)
        ROWS_SSTAMP(5);
        // half A is the FIRST reader of slice s + 1 (its next load phase): its own pieces must have landed before ITS reads
        wait_next();
        ROWS_SSTAMP(6);
      } else if (s + 1 < total) {
        __builtin_amdgcn_s_barrier();                      // b(2s+2)
        ROWS_SSTAMP(5);
      }
    }
    ROWS_STAMP(2);
  };
  if (!half_b) run_half(na_a, std::true_type{}); else run_half(na_b, std::false_type{});
#undef DLIP_FENCE
  if constexpr (EPI == 1) dlip_report_range(amax, a.status);
  ROWS_STAMP(3);
  dlip_span_exit(sc.span);
#ifdef DLIP_LAB
  if (sc.stamps && tid == 0) sc.stamps[(size_t)g * 16 + 6] = __builtin_amdgcn_s_memrealtime() - sc.stamps[(size_t)g * 16 + 7];
#endif
}

int rows_cus() {
  static int cus = 0;                                  // (one device kind per process: every MI355X has the same count)
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
  }
  return cus > 0 ? cus : 256;
}

// The short last round (RowsSched): M rows on tiles of 32 mi x 256, `slots` resident workgroups (one per CU).  full = row tiles of the
// full height (whole rounds of the chip), nmi = height of the rest in units of 32 rows (== mi: no short tiles), tiles_m = all row tiles.
struct RowsTail { long long tiles_m, full; int nmi; };
RowsTail rows_tail(long long M, int tiles_n, int mi, int slots) {
  const int bm = 32 * mi;
  RowsTail t{(M + bm - 1) / bm, 0, mi};
  if (dlip_dbg_value[DLIP_DBG_ROWS_TAIL] == 0 || slots <= 0 || tiles_n <= 0 || slots % tiles_n != 0) return t;
  const long long slots_m = slots / tiles_n, per_round = (long long)bm * slots_m;
  const long long rounds = M / per_round, rem = M - rounds * per_round;
  if (rounds == 0 || rem == 0) return t;              // (one round: rows_pick_mi has picked the height; whole rounds: nothing left over)
  const int nmi = (int)((rem + 32 * slots_m - 1) / (32 * slots_m));
  if (nmi >= mi) return t;
  t.full = rounds * slots_m;
  t.nmi = nmi;
  t.tiles_m = t.full + (rem + 32 * nmi - 1) / (32 * nmi);
  return t;
}

template <int MI, int EPI, bool TAIL = false>
int launch_rows(const ConvArgs& a, hipStream_t st, const ConvRoute& r) {
  constexpr int BM = 32 * MI;
  constexpr size_t lds = (size_t)3 * (BM + ROWS_BN) * ROWB + (EPI != 2 ? 3 * ROWS_BN * sizeof(float) : 0);   // ring + the epilogue's parameter table
  static_assert(lds <= 160 * 1024, "LDS ring exceeds a CU");
  ConvArgs b = a;
  b.tiles_n = (a.K + ROWS_BN - 1) / ROWS_BN;
  auto kern = conv_rows_f16x3_kernel<MI, EPI, TAIL>;
  static DlipKernelState ks;
  int e = ks.ensure_lds(reinterpret_cast<const void*>(kern), lds);
  if (e != DLIP_OK) return e;
  int slots = 0;
  e = ks.resident(reinterpret_cast<const void*>(kern), 512, lds, &slots);   // one workgroup per CU
  if (e != DLIP_OK) return e;
  RowsSched sc;
  sc.item_short0 = sc.t_full = 0x7FFFFFFF; sc.nmi_short = MI; sc.row_short0 = 0;
  if constexpr (TAIL) {
    // the route laid the short last round out for the CUs of the chip -- what dlip_conv_stats_chunks can know without a launch; `slots` is
    // that number whenever the kernel is resident once per CU (if it ever were not, the layout would still be correct, only less even)
    sc.t_full = r.tail_full; sc.item_short0 = r.tail_full * b.tiles_n; sc.nmi_short = r.tail_nmi; sc.row_short0 = r.tail_full * BM;
  }
  const long long items = r.tiles_m * b.tiles_n;
  if (items <= 0 || items > 0x3FFFFFFFll) return DLIP_EINVAL;
  sc.items = (int)items;
  sc.tiles_n = b.tiles_n;
  const long long grid = items < slots ? items : slots;
  sc.span = dlip_span_next();
#ifdef DLIP_LAB
  sc.stamps = nullptr;
  if (getenv("DLIP_STAMP_PRINT")) {
    static unsigned long long* dbuf = nullptr;
    if (!dbuf) (void)hipMalloc(reinterpret_cast<void**>(&dbuf), 4096 * 16 * 8);
    (void)hipMemsetAsync(dbuf, 0, 4096 * 16 * 8, st);
    sc.stamps = dbuf;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), lds, st, b, sc);
    (void)hipStreamSynchronize(st);
    std::vector<unsigned long long> h((size_t)grid * 16);
    (void)hipMemcpy(h.data(), dbuf, h.size() * 8, hipMemcpyDeviceToHost);
    auto med = [](std::vector<double>& v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    std::vector<double> d[3], sl[6], clk;
    for (long long i = 0; i < grid; ++i) {
      const unsigned long long* r = &h[(size_t)i * 16];
      if (!r[3]) continue;
      for (int j = 0; j < 3; ++j) d[j].push_back((double)(r[j + 1] - r[j]));
      if (r[6]) clk.push_back((double)(r[3] - r[0]) / (double)r[6] * 100.0);
      if (r[14]) for (int j = 0; j < 6; ++j) sl[j].push_back((double)(r[9 + j] - r[8 + j]));
    }
    fprintf(stderr, "[rows stamps %dx%d M=%d K=%d nk=%d grid=%lld] first fill %.0f  stream %.0f (%.0f / slice)  last epilogue %.0f  clock %.0f MHz\n",
            BM, ROWS_BN, b.M, b.K, b.nk, grid, med(d[0]), med(d[1]), med(d[1]) / (double)(((items + grid - 1) / grid) * b.nk), med(d[2]), med(clk));
    fprintf(stderr, "[rows slice 8, wave 0 (half A)] epi+reads+issue %.0f  (wait) %.0f  barrier %.0f  matrix phase %.0f  barrier %.0f  wait next %.0f\n",
            med(sl[0]), med(sl[1]), med(sl[2]), med(sl[3]), med(sl[4]), med(sl[5]));
    return dlip_launch_status();
  }
#endif
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), lds, st, b, sc);
  return dlip_launch_status();
}

// Tile height.  A launch takes ceil(items / CUs) rounds of one tile-time ~ MI (+ a fixed part per round: first fill and the
// exposed half of the last epilogue, about a slice and a half of a 16-slice tile); the fewest "row units" wins, the taller
// tile on a tie (fewer bytes per MFMA).
// (round 5) ... and a launch whose last round is SHORT (rows_tail) pays that round at its own height.
int rows_pick_mi(long long M, int K, int nk, int cus, bool tail) {   // tail = false: a pooled launch (tiles of one height)
  const int tiles_n = (K + ROWS_BN - 1) / ROWS_BN;
  int best = 5;
  double best_cost = 1e300;
  for (int mi = 5; mi >= 3; --mi) {
    const RowsTail t = tail ? rows_tail(M, tiles_n, mi, cus) : RowsTail{(M + 32 * mi - 1) / (32 * mi), 0, mi};
    const double eff = mi == 5 ? 1.0 : mi == 4 ? 1.04 : 1.10;
    double cost;
    if (t.nmi < mi) {
      const long long rounds = t.full * tiles_n / cus;
      cost = ((double)rounds * (mi * (double)nk + 1.5 * 5.0) + (t.nmi * (double)nk + 1.5 * 5.0)) * eff;
    } else {
      const long long items = t.tiles_m * tiles_n;
      const long long rounds = (items + cus - 1) / cus;
      cost = (double)rounds * (mi * (double)nk + 1.5 * 5.0) * eff;
    }
    if (cost < best_cost * 0.999) { best_cost = cost; best = mi; }
  }
  return best;
}

}  // namespace

// Which launches the rows kernel serves: every tap of every output row exists (a plain row offset), and there are enough
// rows and columns for its 256-column tiles to be the right shape (the fully connected layers on a batch of utterances stay on the ring kernel's split).
// The pooled epilogue on this kernel is correct and tested, and slower than the ring kernel's LDS-staged one (the fp64 column sums
// straight from the accumulators: tdnn.9 at B = 64 130 us against 96, tools/bench_rows.py): a pooled launch comes here only when FORCED.
static bool rows_shape_ok(const ConvArgs& a, const ConvAsk& q) {
  const int v = dlip_dbg_value[DLIP_DBG_ROWS];
  if (v == 0 || !dlip_conv_dma_enabled() || (q.epi == CONV_EPI_POOL && v < 0)) return false;
  if (q.residual || q.nk2 != 0 || a.Cw != a.C) return false;
  if (!(a.H == 1 && a.R == 1 && a.sw == 1 && a.sh == 1 && a.ph == 0 && a.pw == 0 && (a.C & 31) == 0 && a.S <= 32)) return false;
  if (v > 0) return true;                                  // forced (tests)
  return a.K >= 192 && a.M >= 4096;
}

// The tile height and the row tiles of the launch: the statistics epilogue writes two partial rows per row tile, the pooled one a
// partial band per WAVE ROW = half of its BM x 256 tile, columns rounded up to 128 like the ring kernel's (the same finishers).
extern "C" __attribute__((visibility("hidden"))) int dlip_conv_rows_route(const void* args, const ConvAsk* ask, ConvRoute* route) {
  const ConvArgs& a = *static_cast<const ConvArgs*>(args);
  if (!rows_shape_ok(a, *ask)) return 0;
  const bool pooled = ask->epi == CONV_EPI_POOL;           // (tiles of one height)
  const int cus = rows_cus();
  int mi = rows_pick_mi(a.M, a.K, a.nk, cus, !pooled);
  if (const int v = dlip_dbg_value[DLIP_DBG_ROWS]; v >= 3 && v <= 5) mi = v;   // dlip_debug_set: a forced tile height (tests, A/B)
  const RowsTail t = pooled ? RowsTail{((long long)a.M + 32 * mi - 1) / (32 * mi), 0, mi} : rows_tail(a.M, (a.K + ROWS_BN - 1) / ROWS_BN, mi, cus);
  // a launch with a short last round (rows_tail) runs the TAIL instance; everything else the instance without that code
  *route = ConvRoute{CONV_ROWS, 32 * mi, ROWS_BN, mi, 0, pooled ? 2 : ask->split_out, (int)t.full, t.nmi, t.tiles_m, 16 * mi, 128};
  return 1;
}

extern "C" __attribute__((visibility("hidden"))) int dlip_conv_f16x3_rows_launch(const void* args, void* stream, const ConvRoute* route) {
  const ConvArgs& a = *static_cast<const ConvArgs*>(args);
  hipStream_t st = dlip_hip_stream(stream);
  const ConvRoute& r = *route;
  const int mi = r.inst, epi = r.epi;
  // pooled: a half tile (16 mi rows) may contain at most one row-group boundary
  if (epi == 2 && (a.pool == nullptr || a.pool_group < 16 * mi)) return DLIP_EINVAL;
  if (epi == 2) return mi == 3 ? launch_rows<3, 2>(a, st, r) : mi == 4 ? launch_rows<4, 2>(a, st, r) : launch_rows<5, 2>(a, st, r);
  if (r.tail_nmi < mi) {
    switch (mi) {
      case 3: return epi ? launch_rows<3, 1, true>(a, st, r) : launch_rows<3, 0, true>(a, st, r);
      case 4: return epi ? launch_rows<4, 1, true>(a, st, r) : launch_rows<4, 0, true>(a, st, r);
      default: return epi ? launch_rows<5, 1, true>(a, st, r) : launch_rows<5, 0, true>(a, st, r);
    }
  }
  switch (mi) {
    case 3: return epi ? launch_rows<3, 1>(a, st, r) : launch_rows<3, 0>(a, st, r);
    case 4: return epi ? launch_rows<4, 1>(a, st, r) : launch_rows<4, 0>(a, st, r);
    default: return epi ? launch_rows<5, 1>(a, st, r) : launch_rows<5, 0>(a, st, r);
  }
}

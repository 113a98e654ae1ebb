// The convolution files' calls into each other: the ONE declaration of every function that one of them defines and another
// calls.  Included by the callers AND by the defining files, so a definition that drifts from its prototype is a compile error
// (the names are extern "C": nothing is mangled, a mismatch would link and read garbage).
// `args` is a const ConvArgs*, type-erased: ConvArgs lives in an unnamed namespace of conv_common.h, so it crosses a
// translation-unit boundary as an opaque pointer.
#pragma once
#include <stddef.h>
#include "deeplip_hip.h"

#define DLIP_INTERNAL extern "C" __attribute__((visibility("hidden")))

enum { CONV_EPI_Y = 0, CONV_EPI_POOL = 1, CONV_EPI_STATS = 2 };   // y | pooled partial sums, no y | y and its column sums
struct ConvAsk {                    // what a launch asks for beyond the geometry in ConvArgs
  int f16x3, split_in, split_out;   // 0: the fp32 kernel; x and the residual / y in the split activation format
  int epi, residual, nk2;           // CONV_EPI_*; a residual is added (a reporter: d->ldr != 0); slices of the second source
  int many_tap, aligned;            // more than 32 taps or slice-major operand images; y and the residual 16-byte aligned
};

enum { CONV_RING = 0, CONV_WIN = 1, CONV_ROWS = 2, CONV_STAGED = 3, CONV_F32 = 4 };
struct ConvRoute {     // the answer, which the launches execute and the reporters return: the kernel and the instance that runs
  int kind, bm, bn;    // CONV_*, workgroup tile
  int inst;            // ring: index of its tile menu; window: of its geometries (wave layout, workgroups per CU); register-staged, fp32: of kCfg; rows: bm / 32
  int many_tap, epi;   // ring: the tap-mask-free variant; the instance's epilogue: 0 fp32 y, 1 split y, 2 pooled partials
  int tail_full, tail_nmi;   // rows: row tiles of full height in front of a SHORT last round, its height / 32 (== inst: none, no TAIL instance)
  long long tiles_m;   // rows: row tiles, the short last round's included
  int pool_rows, pool_bn;   // pooled launches: rows of one partial band, column rounding of a band
};

// conv_igemm_f16x3.hip: the launch of `picked`, or of the route it picks itself (THE route: dlip_conv_route_pick there)
DLIP_INTERNAL int dlip_conv_dispatch(const void* args, const ConvAsk* ask, void* stream, const ConvRoute* picked);
// One pair per kernel file: 1 and the instance if the kernel serves the launch, else 0; the launch of the instance a route names
DLIP_INTERNAL int dlip_conv_win_route(const void* args, const ConvAsk* ask, ConvRoute* route);
DLIP_INTERNAL int dlip_conv_f16x3_win_launch(const void* args, void* stream, const ConvRoute* route);
DLIP_INTERNAL int dlip_conv_rows_route(const void* args, const ConvAsk* ask, ConvRoute* route);
DLIP_INTERNAL int dlip_conv_f16x3_rows_launch(const void* args, void* stream, const ConvRoute* route);
DLIP_INTERNAL int dlip_conv_ring_route(const void* args, const ConvAsk* ask, ConvRoute* route);
DLIP_INTERNAL int dlip_conv_f16x3_dma_launch(const void* args, void* stream, const ConvRoute* route);
DLIP_INTERNAL int dlip_conv_f32_launch(const void* args, void* stream, const ConvRoute* route);
// conv_igemm_f16x3_dma.hip: the per-stream workspace of the balanced split (slabs + ticket words); 0 = none / too small
DLIP_INTERNAL int dlip_conv_split_workspace(void* stream, size_t slab_floats, float** slabs, int** counters, int* counter_words);

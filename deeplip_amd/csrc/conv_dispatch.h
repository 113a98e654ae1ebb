// The convolution files' calls into each other: the ONE declaration of every function that one of them defines and another
// calls.  Included by the callers AND by the defining files, so a definition that drifts from its prototype is a compile error
// (the names are extern "C": nothing is mangled, a mismatch would link and read garbage).
// `args` is a const ConvArgs*, type-erased: ConvArgs lives in an unnamed namespace of conv_common.h, so it crosses a
// translation-unit boundary as an opaque pointer.
#pragma once
#include <stddef.h>
#include "deeplip_hip.h"

#define DLIP_INTERNAL extern "C" __attribute__((visibility("hidden")))

// conv_igemm_f16x3.hip: diagnostic switch (dlip_debug_set DLIP_DBG_DMA_ENABLE = 0 keeps split-format launches off the LDS-DMA kernels)
DLIP_INTERNAL int dlip_conv_dma_enabled(void);
// conv_igemm_f16x3_dma.hip: the ring kernel's tile for a launch, its launch (epi: 0 fp32 y, 1 split y, 2 pooled partials), and the
// per-stream workspace of the balanced split (slabs + ticket words); 0 = none / too small
DLIP_INTERNAL void dlip_conv_dma_tile(long long M, int K, int nk, int epi, int* bm, int* bn);
DLIP_INTERNAL int dlip_conv_f16x3_dma_launch(const void* args, void* stream, int epi);
DLIP_INTERNAL int dlip_conv_split_workspace(void* stream, size_t slab_floats, float** slabs, int** counters, int* counter_words);
// conv_win_f16x3.hip: the window kernel
DLIP_INTERNAL int dlip_conv_win_ok(const void* args);
DLIP_INTERNAL int dlip_conv_f16x3_win_launch(const void* args, void* stream, int out_split);
// conv_rows_f16x3.hip: the rows kernel
DLIP_INTERNAL int dlip_conv_rows_ok(const void* args);
DLIP_INTERNAL int dlip_conv_f16x3_rows_launch(const void* args, void* stream, int epi);
DLIP_INTERNAL int dlip_conv_rows_plan(const dlip_conv_desc* d, int* bm);
DLIP_INTERNAL long long dlip_conv_rows_tiles(const dlip_conv_desc* d);
DLIP_INTERNAL int dlip_conv_rows_pool_plan(const dlip_conv_desc* d, int* bm);

// Host-side interface of the bf16x3 split-MFMA convolution (conv_igemm_bf16x3.hip), shared with the conv launcher.
#pragma once
#include "ssp_common.h"

// Plan codes of the conv entry points: 6000000 + tile_rows * 100 + ksplit * 10 + 3 (tile_rows 64 | 128, ksplit 1..9).
#define SSP_BF16X3_PLAN 6000000
static inline int ssp_bf16x3_plan(int plan) { return plan >= SSP_BF16X3_PLAN && plan < SSP_BF16X3_PLAN + 1000000; }
static inline int ssp_bf16x3_plan_bm(int plan) { return (plan - SSP_BF16X3_PLAN) / 100; }
static inline int ssp_bf16x3_plan_ksplit(int plan) { return ((plan - SSP_BF16X3_PLAN) / 10) % 10; }

// Twin codes of the through-memory Winograd plans (conv_wino.h): base + 600000 + tile_rows * 100 + 13, base = 8000000
// (F(4x4)) | 9000000 (F(2x2)) - that plan with its batched GEMM on this kernel (tile_rows 64 | 128; 13 = the Winograd GEMM
// digit and the kernel's fixed 3-slot ring).  The fp32 twin of a code is the code minus 600000.
#define SSP_BF16X3_WINO_DIGIT 600000
static inline int ssp_bf16x3_wino_plan(int plan) {
  return plan >= 8000000 && plan < 10000000 && (plan / 100000) % 10 == 6;
}
static inline int ssp_bf16x3_wino_plan_bm(int plan) { return (plan / 100) % 1000; }

// 1 when a launch of that shape runs under that code, 0 otherwise (pure host function; the launcher switches on it)
int ssp_bf16x3_fits(int64_t M, int Cin, int Cout, int R, int plan);

struct ConvArgs;
// `a` is complete except for the tile counts; a.ksplit = the code's split depth (partials to a.ws when > 1).
// a.batch > 0: a batched launch (gridDim.y problems, ConvArgs::batch_*) - R = 1, un-split, plain stores only, else an error.
int ssp_bf16x3_launch(ConvArgs& a, int bm, int is_dgrad, hipStream_t stream);

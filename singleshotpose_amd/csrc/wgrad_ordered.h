// Ordered (bitwise-reproducible) filter gradients: what the four direct filter-gradient kernel families share.
//
// The atomic forms finish a (filter tile, pixel range) workgroup with fp32 atomic adds into dw, in whatever order the
// hardware retires them.  The ordered forms run the SAME main loops and finish with plain stores of the partial tile into
// slab `split` of a caller-owned workspace [nsplit][Cout][R*R][Cin]; wgrad_ordered_finish_kernel (conv_wgrad.hip) then adds
// the slabs of every element in the order 0, 1, ..., nsplit - 1 and performs the one dw += of the launch.  The split is a
// pure host function of the shape (ssp_wgrad_ordered_plan): no occupancy query, the same in every process.
#ifndef SSP_WGRAD_ORDERED_H
#define SSP_WGRAD_ORDERED_H
#include "ssp_common.h"

// Resolved launch geometry of an ordered filter gradient.  route: ssp_wgrad_route's code for stride 1, for stride 2
// 2'3'0'0'BMO'BNI in the same format (the register-staged family); 0 = refused.  ra: pixel rows per staged chunk.
struct SspWgradOrderedPlan {
  int route, ra, nsplit, chunk_m;
  int64_t M, slab_floats;
};
// split: 0 = the library's choice, else the number of pixel ranges asked for; more ranges than the pixel count allows
// (one staged chunk per range at least) are CLAMPED to that maximum, and a range count the rounding of the range length to
// whole chunks cannot produce gives the next smaller one that it can (7 ranges of 338 pixels in chunks of 16: 64-pixel
// ranges, 6 of them).  The result is what the launch runs and what the workspace query is built on.
SspWgradOrderedPlan ssp_wgrad_ordered_plan(int B, int H, int W, int Cin, int Cout, int lddy, int ldx, int R, int stride, int split);
// dw[e] += slab 0 [e] + slab 1 [e] + ... (float64 accumulation unless fp32_sum), e < n
int ssp_wgrad_ordered_finish_launch(const float* ws, float* dw, int64_t n, int nsplit, int fp32_sum, hipStream_t stream);
// launchers of the four families in their ordered form (ws = the slabs; plan from ssp_wgrad_ordered_plan)
int ssp_conv_wgrad_ordered_s1_launch(const float* dy, const float* x, float* ws, int B, int H, int W, int Cin, int Cout, int lddy,
                                     int ldx, int R, const SspWgradOrderedPlan& pl, hipStream_t stream);
int ssp_conv_wgrad_dma_ordered_launch(const float* dy, const float* x, float* ws, int B, int H, int W, int Cin, int Cout, int lddy,
                                      int ldx, int R, int route, int nsplit, int chunk_m, int64_t slab_floats, int batch,
                                      int64_t batch_dy, int64_t batch_x, int64_t batch_dw, hipStream_t stream);
int ssp_conv_s2_wgrad_ordered_launch(const float* dy, const float* x, float* ws, int B, int H, int W, int Cin, int Cout, int lddy,
                                     int ldx, int R, const SspWgradOrderedPlan& pl, hipStream_t stream);

#if defined(__HIPCC__)
// Epilogue of the register-staged kernels (conv_wgrad.hip, conv_strided.hip) in the ordered form: the WK k-groups of waves
// hold partial sums of one filter tile; groups 1 .. WK-1 hand theirs over through the LDS (free after the main loop's last
// barrier), group 0 adds them in that order and stores the tile plainly.  acc layout: the 32x32x2 MFMA's C/D map.
template <int BMO, int BNI, int WM, int WN, int WK, typename Acc>
__device__ __forceinline__ void ssp_wgrad_ordered_store(Acc& acc, float* smem, float* slab, int Cin, int Cout, int taps, int tap,
                                                        int co0, int ci0) {
  constexpr int WTM = BMO / WM, WTN = BNI / WN, TM = WTM / 32, TN = WTN / 32;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wk = wid / (WM * WN), wmn = wid % (WM * WN);
  const int wm = wmn / WN, wn = wmn % WN;
  const int li = lane & 31, lh = lane >> 5;
  if constexpr (WK > 1) {
    constexpr int PER = TM * TN * 16 * 64;      // floats of one wave's accumulators
    if (wk > 0) {
      float* dst = smem + ((wk - 1) * (WM * WN) + wmn) * PER + lane;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) dst[((i * TN + j) * 16 + r) * 64] = acc[i][j][r];
    }
    __syncthreads();
    if (wk > 0) return;
#pragma unroll
    for (int g = 1; g < WK; ++g) {
      const float* src = smem + ((g - 1) * (WM * WN) + wmn) * PER + lane;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += src[((i * TN + j) * 16 + r) * 64];
    }
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int ci = ci0 + wn * WTN + j * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (co < Cout && ci < Cin) slab[((int64_t)co * taps + tap) * Cin + ci] = acc[i][j][r];
      }
    }
}
#endif
#endif /* SSP_WGRAD_ORDERED_H */

// bf16x3 split-MFMA implicit-GEMM convolution (stride 1, "same" padding, R in {1,3}): the opt-in fast mode of the
// direct convolutions (plan codes 6000000 + tile_rows * 100 + ksplit * 10 + 3, conv_bf16x3.h) and, as a batched R = 1 launch,
// the GEMM of the through-memory Winograd plans (their twin codes 8 | 9 6xxx13, same header).
//
// Same contraction, same operands and same ConvArgs as conv_igemm_kernel (conv_igemm.hip): fp32 NHWC activations and
// the fp32 packed filter [Cout][R*R][Cin] of ssp_repack_fwd / ssp_repack_dgrad; nothing is pre-split in memory.
//
// The split.  Every fp32 operand element x is written as x = h + m + l with three bf16 terms,
//     h = bf16(x)    r = x - h (exact)    m = bf16(r)    l = r - m (exact, at most 8 significant bits, so a bf16)
// with ROUND-TO-NEAREST-EVEN conversions (v_cvt_pk_bf16_f32), so |m| <= 2^-9 |x| and |l| <= 2^-18 |x|.  (A truncating
// split is exact too, but its terms only shrink by 2^-8 each and the dropped products are about 8 times larger.)  The
// split happens where the register-staged loader stores a tile into LDS: once per element and workgroup, not once per
// reading wave.  LDS holds three bf16 planes per tile (6 B per element, 4 B in the fp32 kernel).
//
// The products.  x * w = sum of nine term products; the six of order <= 2 are evaluated on the bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16, fp32 accumulation), smallest first, into one accumulator per 32x32 tile that is folded
// into a running total every 6 K-steps (chunked accumulation, see the kernel):
//     l*h, h*l, m*m, m*h, h*m, h*h
// and m*l + l*m + l*l is dropped: at most 2^-24.3 of the product (measured on 2e6 random pairs; rms 2^-27), below the
// half-ulp of an fp32 product.  The C/D register layout of the 32x32 MFMA does not depend on the input type, so the
// shared epilogue (igemm_epilogue, conv_igemm_common.h) takes the accumulators unchanged: bias, eval-mode scale / slope,
// accumulate, per-tile BatchNorm statistics, split-K partials and the fused BatchNorm-backward sums all work as in the
// fp32 kernel, and splitk_reduce_kernel finishes a split launch.
//
// Non-finite inputs: an Inf operand gives NaN (Inf - Inf in the split), where the fp32 kernel gives Inf; a finite value
// within half a bf16 ulp of FLT_MAX rounds h to Inf and gives NaN as well.  NaN stays NaN.
//
// Operand map of v_mfma_f32_32x32x16_bf16: lane l holds A[row l&31][k = 8*(l>>5) + j] and B[k = 8*(l>>5) + j][col l&31],
// j = 0..7 (cdna_hip_programming.md section 3) - with both tiles k-contiguous in LDS, one ds_read_b128 per term and
// 32-row block.  A plane's rows are 32 B apart, so the 64 lanes of a fragment read cover 2 KiB contiguously.
#include "conv_igemm_common.h"
#include "conv_bf16x3.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// Pipeline: the register-staged loader of conv_igemm_kernel with BK = 16 - LDS ring of 3 slots, one barrier per K chunk;
// chunk it+2 goes from registers to its slot (split on the way) and chunk it+3 from memory to registers around the
// 6 * TM * TN MFMAs of chunk it.  Fragments are read at the top of their chunk (no fragment double buffer: its 48
// registers pay for the second accumulator; with two workgroups per CU the other wave's MFMAs cover the LDS latency).
// Loads are branch-free and clamped exactly as there.
// Batched launch (ConvArgs::batch > 0; the GEMM of the Winograd twin codes, conv_bf16x3.h): blockIdx.y picks the problem,
// the operand bases move by batch_in / batch_wt floats and the epilogue's output by batch_out; nothing else changes (the
// loader's rows and the filter rows stay clamped inside their own plane).  Resources with the batch offsets in (hipcc
// -Rpass-analysis=kernel-resource-usage, gfx950, no scratch): tile rows 128: 228 VGPRs (x 128 columns; 150 x 64) -> 2 waves
// per SIMD = 2 workgroups per CU, which 72 KiB (54 KiB) of LDS each allow too; tile rows 64: 141 VGPRs (x 128; 90 x 64) ->
// 3 (5) waves per SIMD by registers, 2 (4) workgroups per CU by their 54 KiB (36 KiB) of LDS.
// PASS (0 forward, 1 data gradient) only gives the two uses distinct kernel names for profiles.
template <int BM, int BN, int WM, int WN, int PASS = 0>
__global__ void __launch_bounds__(WM* WN * 64, 2) conv_igemm_bf16x3_kernel(ConvArgs p) {
  constexpr int NT = WM * WN * 64;
  constexpr int BK = 16;
  constexpr int TPR = BK / 4;       // loader threads per tile row (one float4 each)
  constexpr int RPP = NT / TPR;     // tile rows covered per loader pass
  constexpr int APASS = BM / RPP, BPASS = BN / RPP;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int PLANE = (BM + BN) * BK;   // bf16 elements per term plane: A rows then B rows, 16 k each
  constexpr int SLOT = 3 * PLANE;         // planes h, m, l
  static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the loader pass");
  static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile must be a multiple of the 32x32 MFMA");

  extern __shared__ __attribute__((aligned(16))) float smem[];   // 3 * SLOT bf16
  __bf16* const sm = reinterpret_cast<__bf16*>(smem);

  const int ntiles = p.ntile_m * p.ntile_n;
  const int nwg = ntiles * p.ksplit;
  const int lid0 = p.xcd_remap ? ssp_xcd_remap(blockIdx.x, nwg) : (int)blockIdx.x;
  const int split = lid0 / ntiles, lid = lid0 - split * ntiles;
  const int tile_n = lid % p.ntile_n, tile_m = lid / p.ntile_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int li = lane & 31, lh = lane >> 5;

  const int pad = p.R >> 1;
  const int K = p.R * p.R * p.Cin;
  const int cpt = p.Cin / BK;  // K chunks per filter tap
  const int it_begin = split * p.it_per_split;
  const int niter = min(p.R * p.R * cpt, it_begin + p.it_per_split) - it_begin;   // this workgroup's K chunks
  // batched launch (the P transform positions of a Winograd layer, conv_wino.hip): blockIdx.y = problem index (scalar);
  // batch = 0 is one problem at the operands themselves (gridDim.y = 1, every offset 0)
  const int64_t bz = (p.batch > 0) ? (int64_t)blockIdx.y : 0;
  const float* const in_b = p.in + bz * p.batch_in;
  const float* const wt_b = p.wt + bz * p.batch_wt;

  // ---- loader setup: rows are fixed for the whole K loop ----
  const int lrow = tid / TPR, lcol = (tid % TPR) * 4;
  const float* a_ptr[APASS];
  int a_y[APASS], a_x[APASS];
#pragma unroll
  for (int i = 0; i < APASS; ++i) {
    int m = m0 + lrow + i * RPP;
    if (m >= p.M) m = p.M - 1;   // clamped duplicate row: computed, never stored
    a_x[i] = m % p.W;
    a_y[i] = (m / p.W) % p.H;
    a_ptr[i] = in_b + (int64_t)m * p.ldin + lcol;
  }
  const float* b_ptr[BPASS];
#pragma unroll
  for (int i = 0; i < BPASS; ++i) {
    int n = n0 + lrow + i * RPP;
    if (n >= p.Cout) n = p.Cout - 1;
    b_ptr[i] = wt_b + (int64_t)n * K + lcol;
  }

  f32x4 a_reg[APASS], b_reg[BPASS];
  unsigned a_okmask = 0;   // bit i: pass i of the staged chunk is inside the image (applied at LDS-store time)
  const int tap0 = it_begin / cpt;
  int ld_c0 = (it_begin - tap0 * cpt) * BK, ld_dy = tap0 / p.R - pad, ld_dx = tap0 % p.R - pad;
  int64_t ld_koff = (int64_t)it_begin * BK;
  auto load_global = [&](f32x4 (&a_reg)[APASS], f32x4 (&b_reg)[BPASS], unsigned& a_okmask) {
    const int64_t shift = ((int64_t)ld_dy * p.W + ld_dx) * p.ldin + ld_c0;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      int yy = a_y[i] + ld_dy, xx = a_x[i] + ld_dx;
      bool ok = ((unsigned)yy < (unsigned)p.H) && ((unsigned)xx < (unsigned)p.W);
      a_reg[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + (ok ? shift : (int64_t)ld_c0));
      a_okmask = ok ? (a_okmask | (1u << i)) : (a_okmask & ~(1u << i));
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) b_reg[i] = *reinterpret_cast<const f32x4*>(b_ptr[i] + ld_koff);
    // advance; past the last chunk the walker re-reads the last filter columns / an in-image or clamped pixel
    // (harmless: those stagings land in a ring slot nobody reads), which keeps the K loop free of branches
    ld_koff = min(ld_koff + BK, (int64_t)(K - BK));
    ld_c0 += BK;
    const bool wrap = ld_c0 == p.Cin;
    ld_c0 = wrap ? 0 : ld_c0;
    ld_dx += wrap ? 1 : 0;
    const bool wrap2 = ld_dx > pad;
    ld_dx = wrap2 ? -pad : ld_dx;
    ld_dy += wrap2 ? 1 : 0;
  };
  // x = h + m + l (round to nearest even), four elements -> 8 bytes in each of the three planes
  auto split_store = [&](__bf16* dst, const f32x4& v) {
    bf16x4 h, m, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = v[e];
      h[e] = (__bf16)x;
      const float r = x - (float)h[e];
      m[e] = (__bf16)r;
      l[e] = (__bf16)(r - (float)m[e]);
    }
    *reinterpret_cast<bf16x4*>(dst) = h;
    *reinterpret_cast<bf16x4*>(dst + PLANE) = m;
    *reinterpret_cast<bf16x4*>(dst + 2 * PLANE) = l;
  };
  auto store_lds = [&](int slot, const f32x4 (&a_reg)[APASS], const f32x4 (&b_reg)[BPASS], unsigned a_okmask) {
    __bf16* As = sm + slot * SLOT;
    __bf16* Bs = As + BM * BK;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      const bool ok = (a_okmask >> i) & 1u;
      f32x4 v;
      v[0] = ok ? a_reg[i][0] : 0.f; v[1] = ok ? a_reg[i][1] : 0.f;
      v[2] = ok ? a_reg[i][2] : 0.f; v[3] = ok ? a_reg[i][3] : 0.f;
      split_store(As + (lrow + i * RPP) * BK + lcol, v);
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) split_store(Bs + (lrow + i * RPP) * BK + lcol, b_reg[i]);
  };
  // fragment read: lane (i,h) takes the 8 bf16 at k = 8h of its row, in each plane
  auto read_frag = [&](int slot, bf16x8 (&fa)[TM][3], bf16x8 (&fb)[TN][3]) {
    const __bf16* Ab = sm + slot * SLOT + (wm * WTM + li) * BK + lh * 8;
    const __bf16* Bb = sm + slot * SLOT + (BM + wn * WTN + li) * BK + lh * 8;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int t = 0; t < 3; ++t) fa[i][t] = *reinterpret_cast<const bf16x8*>(Ab + t * PLANE + i * 32 * BK);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int t = 0; t < 3; ++t) fb[j][t] = *reinterpret_cast<const bf16x8*>(Bb + t * PLANE + j * 32 * BK);
  };

  // Chunked accumulation, as in the fp32 kernel: `acc` takes the six products of GROUP K-steps
  // (K = 96), is folded into the running total `tot` with VALU adds (round to nearest) and cleared.  The matrix core's own
  // accumulate step is the dominant error of a long chain: at K = 2304 one accumulator for everything measured 5.5 x the
  // fp32 kernel's error against float64, the five low-order products in a second accumulator 2.0 x, this form 1.0 x
  //  - and it was no slower than either.
  constexpr int GROUP = 6;
  f32x16 acc[TM][TN], tot[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.f;

  // the six products of order <= 2, smallest first (term index 0 = h, 1 = m, 2 = l)
  auto mma = [&](bf16x8 (&fa)[TM][3], bf16x8 (&fb)[TN][3]) {
    constexpr int TA[6] = {2, 0, 1, 1, 0, 0};
    constexpr int TB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int s = 0; s < 6; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][TA[s]], fb[j][TB[s]], acc[i][j], 0, 0, 0);
  };

  // ---- prologue: chunks 0 and 1 into slots 0 and 1, chunk 2 into registers ----
  {
    f32x4 a0[APASS], b0[BPASS], a1[APASS], b1[BPASS];
    unsigned m0k = 0, m1k = 0;
    load_global(a0, b0, m0k);
    load_global(a1, b1, m1k);
    load_global(a_reg, b_reg, a_okmask);   // chunk 2 stays in registers until the first loop iteration stores it
    store_lds(0, a0, b0, m0k);
    store_lds(1, a1, b1, m1k);
  }
  __syncthreads();
  bf16x8 fa[TM][3], fb[TN][3];

  int slot = 0;   // it % 3
  int ingroup = 0;
  for (int it = 0; it < niter; ++it) {
    const int slot1 = (slot == 2) ? 0 : slot + 1;          // (it+1) % 3
    const int slot2 = (slot1 == 2) ? 0 : slot1 + 1;        // (it+2) % 3
    // in the last two chunks the staging of "chunk it+2" is a redundant re-read whose result is never consumed
    read_frag(slot, fa, fb);                               // written two chunks ago, published by the last barrier
    store_lds(slot2, a_reg, b_reg, a_okmask);              // slot (it-1) % 3: its readers passed the last barrier
    load_global(a_reg, b_reg, a_okmask);                   // chunk it+3 -> registers; a whole chunk of MFMAs to land
    mma(fa, fb);
    if (++ingroup == GROUP) {      // (workgroup-uniform)
      ingroup = 0;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          tot[i][j] += acc[i][j];
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
    }
    __syncthreads();
    slot = slot1;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] += tot[i][j];

  igemm_epilogue<BM, BN, WM, WN, NT>(p, acc, smem, m0, n0, tile_m, split, tid, p.ksplit > 1, bz * p.batch_out);
}

template <int BM, int BN, int PASS>
static int launch_bf16x3(ConvArgs a, hipStream_t stream) {
  a.ntile_m = ssp_cdiv(a.M, BM);
  a.ntile_n = ssp_cdiv(a.Cout, BN);
  const int niter_total = a.R * a.R * (a.Cin / 16);
  a.it_per_split = ssp_cdiv(niter_total, a.ksplit);
  a.ksplit = ssp_cdiv(niter_total, a.it_per_split);
  const int64_t nwg = (int64_t)a.ntile_m * a.ntile_n * a.ksplit;
  SSP_CHECK_ARG(nwg < (1ll << 31), "conv (bf16x3 plan): too many workgroups");
  if (a.batch > 0) {
    // a batched launch is the plain GEMM of a Winograd plan: everything else is the finishing pass's work
    SSP_CHECK_ARG(a.batch <= 65535 && a.R == 1 && a.ksplit == 1 && a.bias == nullptr && a.escale == nullptr &&
                      a.act_slope == 1.f && a.stats == nullptr && a.bn_partial == nullptr && a.accumulate == 0,
                  "conv (bf16x3 plan): a batched launch is R = 1, un-split, with no bias, scale, activation, statistics, "
                  "BatchNorm-backward sums or accumulate");
    SSP_CHECK_ARG(a.batch_in >= 0 && a.batch_wt >= 0 && a.batch_out >= 0, "conv (bf16x3 plan): negative batch strides");
  }
  const int lds_bytes = 3 * 3 * (BM + BN) * 16 * 2;
  auto kern = conv_igemm_bf16x3_kernel<BM, BN, 2, 2, PASS>;
  static SspKernelCache cache;   // per instantiation, per device
  if (int rc = ssp_kernel_prepare((const void*)kern, lds_bytes, 256, &cache, nullptr, "conv_igemm_bf16x3")) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg, a.batch > 0 ? a.batch : 1), dim3(256), lds_bytes, stream, a);
  SSP_CHECK_LAUNCH("conv_igemm_bf16x3");
  return SSP_OK;
}

int ssp_bf16x3_fits(int64_t M, int Cin, int Cout, int R, int plan) {
  if (ssp_bf16x3_wino_plan(plan)) {      // a through-memory Winograd plan with its batched GEMM on this kernel
    const int bm = ssp_bf16x3_wino_plan_bm(plan);
    if ((bm != 64 && bm != 128) || plan % 100 != 13) return 0;      // GEMM digit 1, the kernel's 3-slot ring
    if (R != 3 || Cin <= 0 || Cin % 16 != 0 || Cout < 64 || Cout % 4 != 0) return 0;
    return M > 0 && M < (1ll << 31);
  }
  if (!ssp_bf16x3_plan(plan)) return 0;
  const int bm = ssp_bf16x3_plan_bm(plan), ks = ssp_bf16x3_plan_ksplit(plan);
  if ((bm != 64 && bm != 128) || ks < 1 || plan % 10 != 3) return 0;
  if (R != 1 && R != 3) return 0;
  if (Cin <= 0 || Cin % 16 != 0 || Cout <= 32 || Cout % 4 != 0) return 0;
  if (M <= 0 || M >= (1ll << 31) || (int64_t)R * R * Cin >= (1ll << 31)) return 0;   // 32-bit pixel / k indices of the loader
  if (ks > 1 && (R * R * (Cin / 16)) / ks < 8) return 0;      // the fp32 plans' rule: >= 8 chunks per split
  return 1;
}

int ssp_bf16x3_launch(ConvArgs& a, int bm, int is_dgrad, hipStream_t stream) {
  if (a.Cout > 64) {
    if (bm == 64) return is_dgrad ? launch_bf16x3<64, 128, 1>(a, stream) : launch_bf16x3<64, 128, 0>(a, stream);
    return is_dgrad ? launch_bf16x3<128, 128, 1>(a, stream) : launch_bf16x3<128, 128, 0>(a, stream);
  }
  if (bm == 64) return is_dgrad ? launch_bf16x3<64, 64, 1>(a, stream) : launch_bf16x3<64, 64, 0>(a, stream);
  return is_dgrad ? launch_bf16x3<128, 64, 1>(a, stream) : launch_bf16x3<128, 64, 0>(a, stream);
}

// Stride-2 convolution (nn.Conv2d(..., stride=2, padding=(k-1)//2), k in {1,3}) on the CDNA4 fp32 matrix cores:
// forward, data gradient and filter gradient of a downsampling block (darknet.py:145-167 with stride = 2).
//
// Geometry (H x W input map, R = filter size, pad = R / 2):
//   Ho = (H + 2*pad - R) / 2 + 1, Wo likewise;  input row of output row yo and tap r = 2*yo + r - pad, zero outside.
//
// Forward: implicit GEMM over the OUTPUT pixels, M = B*Ho*Wo, N = Cout, K = R*R*Cin; the A gather uses the strided
// coordinates, the filter operand is ssp_repack_fwd's [Cout][R*R][Cin], the epilogue is igemm_epilogue
// (conv_igemm_common.h: bias, eval-mode affine + leaky, accumulate, per-tile BatchNorm statistics).
//
// Data gradient: decomposed by the parity of the destination pixel (yi, xi).  yi = 2*yo + r - pad, so at 3x3 pad 1
//   yi even: r = 1, yo = yi/2           yi odd: r = 0, yo = (yi+1)/2  and  r = 2, yo = (yi-1)/2
// (1, 2, 2 and 4 taps for the classes (even,even), (even,odd), (odd,even), (odd,odd)); at 1x1 only (even,even)
// receives anything.  Each class is a DENSE contraction over its own taps: rows = the class's pixels (yh, xh) with
// yi = 2*yh + py, source = dy at (yh + oy, xh + ox), oy in {0, 1}, zero when it falls on row Ho (odd yi = H-1 with
// r = 0).  All classes run in ONE launch (the class is a function of the workgroup's tile index, most taps first) over
// ssp_repack_dgrad's [Cin_dx][R*R][Cout_dy] operand (taps rotated by 180 degrees): 9/4 taps per pixel on average
// instead of the nine a masked gather would walk.  A launch too small to fill the chip gives every (class, tap) pair
// its own workgroups and sums the taps of a pixel with fp32 atomics (ssp_conv_s2_dgrad_launch).
//
// Filter gradient: conv_wgrad.hip's register-staged kernel with the strided gather on the x operand.
//
// The K loop is the register-staged pipeline of conv_igemm.hip (LDS ring of 3 slots, one barrier per chunk, branch-free
// loads: out-of-map taps read a clamped address and are zeroed when they are stored to the LDS).
#include "conv_igemm_common.h"
#include "wgrad_ordered.h"

struct S2Class {
  int py, px;          // data gradient: parity of the destination pixel (forward: 0, 0)
  int Hr, Wr, M;       // rows of the class: m = (b*Hr + y)*Wr + x, M = B*Hr*Wr
  int tile0;           // first M tile of the class in the launch's tile order
  int ntap;
  unsigned long long taps_lo;   // taps 0..7, one byte each: (oy + 1) | (ox + 1) << 2 | filter tap index << 4
  unsigned taps_hi;             // tap 8
  SspFastDiv divW, divH;
};

struct S2Args {
  ConvArgs c;          // in, wt, out, epilogue terms, Cin (channels per tap), Cout, ldin, ldout, ntile_n; M / ntile_m of class 0
  int Hs, Ws, ms;      // source map; source pixel of row (y, x) and tap = (ms*y + oy, ms*x + ox)
  int Hd, Wd, ds;      // destination map; destination pixel of row (y, x) = (ds*y + py, ds*x + px)
  int wld;             // floats per filter row (all taps)
  int ncls;
  S2Class cls[9];      // forward: one; data gradient: the four parity classes, or one per (class, tap) of a tap-split launch
};

// PASS 0: forward (epilogue of conv_igemm_common.h, destination row = m); 1: data gradient (scattered destination rows)
template <int BM, int BN, int WM, int WN, int BK, int PASS>
__global__ void __launch_bounds__(WM* WN * 64, 2) conv_s2_kernel(S2Args p) {
  constexpr int NT = WM * WN * 64;
  constexpr int LS = BK + 4;        // LDS row stride in floats (16-B aligned, conflict-free b128 reads)
  constexpr int TPR = BK / 4;       // loader threads per tile row (one float4 each)
  constexpr int RPP = NT / TPR;     // tile rows covered per loader pass
  constexpr int APASS = (BM + RPP - 1) / RPP;
  constexpr int BPASS = (BN + RPP - 1) / RPP;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int VEC = (BK >= 8) ? 4 : 2;
  constexpr int NQ = BK / (2 * VEC);
  constexpr int SLOT = (BM + BN) * LS;   // floats per ring slot: A rows then B rows
  static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile must be a multiple of the 32x32 MFMA");
  static_assert(NQ >= 1, "BK too small");

  extern __shared__ __attribute__((aligned(16))) float smem[];   // 3 * SLOT floats

  const int tile_n = (int)blockIdx.x % p.c.ntile_n, tile_g = (int)blockIdx.x / p.c.ntile_n;
  int ci = 0;
  for (int k = 1; k < p.ncls; ++k) ci = (tile_g >= p.cls[k].tile0) ? k : ci;
  const S2Class& cl = p.cls[ci];
  const int tile_m = tile_g - cl.tile0;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int M = cl.M;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int li = lane & 31, lh = lane >> 5;

  const int Cin = p.c.Cin;
  const int cpt = Cin / BK;           // K chunks per tap
  const int ntap = cl.ntap;
  const int niter = ntap * cpt;
  const unsigned long long taps_lo = cl.taps_lo;
  const unsigned taps_hi = cl.taps_hi;

  // ---- loader setup: rows are fixed for the whole K loop ----
  const int lrow = tid / TPR, lcol = (tid % TPR) * 4;
  const float* a_ptr[APASS];
  int a_y[APASS], a_x[APASS];
#pragma unroll
  for (int i = 0; i < APASS; ++i) {
    int m = m0 + lrow + i * RPP;
    if (m >= M) m = M - 1;   // clamped duplicate row: computed, never stored
    const unsigned t = ssp_div((unsigned)m, cl.divW);
    const int x = m - (int)t * cl.Wr;
    const unsigned b = ssp_div(t, cl.divH);
    const int y = (int)t - (int)b * cl.Hr;
    a_y[i] = p.ms * y;
    a_x[i] = p.ms * x;
    a_ptr[i] = p.c.in + (int64_t)b * p.Hs * p.Ws * p.c.ldin + lcol;    // pixel (b, 0, 0)
  }
  const float* b_ptr[BPASS];
#pragma unroll
  for (int i = 0; i < BPASS; ++i) {
    int n = n0 + lrow + i * RPP;
    if (n >= p.c.Cout) n = p.c.Cout - 1;
    b_ptr[i] = p.c.wt + (int64_t)n * p.wld + lcol;
  }

  f32x4 a_reg[APASS], b_reg[BPASS];
  unsigned a_okmask = 0;   // bit i: pass i of the staged chunk is inside the map (applied at LDS-store time)
  int ld_t = 0, ld_c0 = 0; // K-chunk walker of the loader: (tap, first channel); chunks are visited in order
  auto load_global = [&](f32x4 (&a_reg)[APASS], f32x4 (&b_reg)[BPASS], unsigned& a_okmask) {
    const unsigned code = (ld_t < 8) ? (unsigned)((taps_lo >> (8 * ld_t)) & 0xffull) : taps_hi;
    const int oy = (int)(code & 3u) - 1, ox = (int)((code >> 2) & 3u) - 1;
    const int woff = (int)(code >> 4) * Cin + ld_c0;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      const int yy = a_y[i] + oy, xx = a_x[i] + ox;
      const bool ok = ((unsigned)yy < (unsigned)p.Hs) && ((unsigned)xx < (unsigned)p.Ws);
      const int64_t off = ok ? ((int64_t)yy * p.Ws + xx) * p.c.ldin : (int64_t)0;
      a_reg[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + off + ld_c0);
      a_okmask = ok ? (a_okmask | (1u << i)) : (a_okmask & ~(1u << i));
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) b_reg[i] = *reinterpret_cast<const f32x4*>(b_ptr[i] + woff);
    // advance; past the last chunk the walker stays on it (re-reads in-bounds data into a ring slot nobody reads),
    // which keeps the K loop free of branches
    ld_c0 += BK;
    const bool wrap = ld_c0 == Cin;
    ld_c0 = wrap ? 0 : ld_c0;
    ld_t += wrap ? 1 : 0;
    const bool end = ld_t == ntap;
    ld_t = end ? ntap - 1 : ld_t;
    ld_c0 = end ? Cin - BK : ld_c0;
  };
  auto store_lds = [&](int slot, const f32x4 (&a_reg)[APASS], const f32x4 (&b_reg)[BPASS], unsigned a_okmask) {
    float* As = smem + slot * SLOT;
    float* Bs = As + BM * LS;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      int row = lrow + i * RPP;
      const bool ok = (a_okmask >> i) & 1u;
      f32x4 v;
      v[0] = ok ? a_reg[i][0] : 0.f; v[1] = ok ? a_reg[i][1] : 0.f;
      v[2] = ok ? a_reg[i][2] : 0.f; v[3] = ok ? a_reg[i][3] : 0.f;
      if (BM % RPP == 0 || row < BM) *reinterpret_cast<f32x4*>(As + row * LS + lcol) = v;
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
      int row = lrow + i * RPP;
      if (BN % RPP == 0 || row < BN) *reinterpret_cast<f32x4*>(Bs + row * LS + lcol) = b_reg[i];
    }
  };
  // fragment read: lane (i,h) takes VEC consecutive floats at column q*2*VEC + h*VEC of its row
  auto read_frag = [&](int slot, int q, float (&fa)[TM][VEC], float (&fb)[TN][VEC]) {
    const float* Ab = smem + slot * SLOT + (wm * WTM + li) * LS + lh * VEC + q * 2 * VEC;
    const float* Bb = smem + slot * SLOT + (BM + wn * WTN + li) * LS + lh * VEC + q * 2 * VEC;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if constexpr (VEC == 4) {
        f32x4 t = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LS);
        fa[i][0] = t[0]; fa[i][1] = t[1]; fa[i][2] = t[2]; fa[i][3] = t[3];
      } else {
        f32x2 t = *reinterpret_cast<const f32x2*>(Ab + i * 32 * LS);
        fa[i][0] = t[0]; fa[i][1] = t[1];
      }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if constexpr (VEC == 4) {
        f32x4 t = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LS);
        fb[j][0] = t[0]; fb[j][1] = t[1]; fb[j][2] = t[2]; fb[j][3] = t[3];
      } else {
        f32x2 t = *reinterpret_cast<const f32x2*>(Bb + j * 32 * LS);
        fb[j][0] = t[0]; fb[j][1] = t[1];
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto mma = [&](float (&fa)[TM][VEC], float (&fb)[TN][VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
  };

  // ---- prologue: chunks 0 and 1 into slots 0 and 1, chunk 2 into registers, first fragments into registers ----
  {
    f32x4 a0[APASS], b0[BPASS], a1[APASS], b1[BPASS];
    unsigned m0k = 0, m1k = 0;
    load_global(a0, b0, m0k);
    load_global(a1, b1, m1k);
    load_global(a_reg, b_reg, a_okmask);
    store_lds(0, a0, b0, m0k);
    store_lds(1, a1, b1, m1k);
  }
  __syncthreads();
  float fa[2][TM][VEC], fb[2][TN][VEC];   // fragment double buffer; set (q & 1) holds sub-step q
  read_frag(0, 0, fa[0], fb[0]);

  int slot = 0;   // it % 3
  for (int it = 0; it < niter; ++it) {
    const int slot1 = (slot == 2) ? 0 : slot + 1;          // (it+1) % 3
    const int slot2 = (slot1 == 2) ? 0 : slot1 + 1;        // (it+2) % 3
    // branch-free body: in the last two chunks the staging of "chunk it+2" and the fragment prefetch of "chunk it+1"
    // are redundant re-reads whose results are never consumed
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q + 1 < NQ) {
        read_frag(slot, q + 1, fa[(q + 1) & 1], fb[(q + 1) & 1]);
      } else {
        read_frag(slot1, 0, fa[NQ & 1], fb[NQ & 1]);
      }
      if (q == 0) {
        store_lds(slot2, a_reg, b_reg, a_okmask);   // chunk it+2, loaded during the previous chunk's MFMAs
        load_global(a_reg, b_reg, a_okmask);        // chunk it+3 -> registers
      }
      mma(fa[q & 1], fb[q & 1]);
    }
    __syncthreads();
    if constexpr ((NQ & 1) != 0) {   // odd NQ: the prefetched q=0 fragments sit in set 1, move them to set 0
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < VEC; ++e) fa[0][i][e] = fa[1][i][e];
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) fb[0][j][e] = fb[1][j][e];
    }
    slot = slot1;
  }

  if constexpr (PASS == 0) {
    igemm_epilogue<BM, BN, WM, WN, NT>(p.c, acc, smem, m0, n0, tile_m, 0, tid, false);
  } else {
    // destination rows are scattered (every second pixel of every second row): one predicated store per element
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < M) {
          const unsigned t = ssp_div((unsigned)m, cl.divW);
          const int x = m - (int)t * cl.Wr;
          const unsigned b = ssp_div(t, cl.divH);
          const int y = (int)t - (int)b * cl.Hr;
          float* o = p.c.out + (((int64_t)b * p.Hd + (p.ds * y + cl.py)) * p.Wd + (p.ds * x + cl.px)) * p.c.ldout;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WTN + j * 32 + li;
            if (n < p.c.Cout) {
              float v = acc[i][j][r];
              if (p.c.accumulate == 2) {        // tap-split launch: the taps of a pixel arrive from several workgroups
                atomicAdd(o + n, v);
              } else {
                if (p.c.accumulate) v += o[n];
                o[n] = v;
              }
            }
          }
        }
      }
  }
}

// Zero fill of dx's Cin_dx columns: odd_only = 1 - the three parity classes no output pixel reaches (1x1 data gradient,
// accumulate off); 0 - every pixel (in front of a tap-split launch, which adds into dx)
__global__ void __launch_bounds__(256) conv_s2_zero_kernel(float* dx, int lddx, int C, int H, int W, int64_t total, int odd_only) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const int64_t pix = e / C;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    if (!odd_only || ((x | y) & 1)) dx[pix * lddx + c] = 0.f;
  }
}

static inline int s2_out(int H, int R) { return (H + 2 * (R / 2) - R) / 2 + 1; }

// Tile choice, a pure function of the launch shape (the statistics query shares it): 128 x 128 tiles, 64 columns for thin
// layers, 64 rows when 128-row tiles would leave CUs of the 256 without a workgroup.
struct S2Tile { int bm, bn; };
static S2Tile s2_tile(const int64_t* Ms, int ncls, int Cout) {
  S2Tile t;
  t.bn = Cout > 64 ? 128 : 64;
  int64_t tiles = 0;
  for (int k = 0; k < ncls; ++k) tiles += (Ms[k] + 127) / 128;
  t.bm = tiles * ssp_cdiv(Cout, t.bn) < 256 ? 64 : 128;
  return t;
}
int ssp_conv_s2_tile_m(int B, int H, int W, int Cout, int R) {
  if ((R != 1 && R != 3) || B <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  const int64_t M = (int64_t)B * s2_out(H, R) * s2_out(W, R);
  return s2_tile(&M, 1, Cout).bm;
}

template <int BM, int BN, int BK, int PASS>
static int s2_launch_cfg(S2Args& a, hipStream_t stream) {
  int tiles = 0;
  for (int k = 0; k < a.ncls; ++k) {
    a.cls[k].tile0 = tiles;
    tiles += ssp_cdiv(a.cls[k].M, BM);
  }
  a.c.ntile_m = ssp_cdiv(a.cls[0].M, BM);     // forward: rows of the statistics buffer
  a.c.ntile_n = ssp_cdiv(a.c.Cout, BN);
  const int lds_bytes = 3 * (BM + BN) * (BK + 4) * 4;
  auto kern = conv_s2_kernel<BM, BN, 2, 2, BK, PASS>;
  static SspKernelCache cache;   // per instantiation, per device
  if (int rc = ssp_kernel_prepare((const void*)kern, lds_bytes, 256, &cache, nullptr, "conv_s2")) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * a.c.ntile_n)), dim3(256), lds_bytes, stream, a);
  SSP_CHECK_LAUNCH("conv_s2");
  return SSP_OK;
}

template <int PASS>
static int s2_launch(S2Args& a, hipStream_t stream) {
  int64_t Ms[9];
  for (int k = 0; k < a.ncls; ++k) Ms[k] = a.cls[k].M;
  const S2Tile t = s2_tile(Ms, a.ncls, a.c.Cout);
  const bool k16 = a.c.Cin % 16 == 0;
  if (t.bm == 128 && t.bn == 128) return k16 ? s2_launch_cfg<128, 128, 16, PASS>(a, stream) : s2_launch_cfg<128, 128, 4, PASS>(a, stream);
  if (t.bm == 64 && t.bn == 128) return k16 ? s2_launch_cfg<64, 128, 16, PASS>(a, stream) : s2_launch_cfg<64, 128, 4, PASS>(a, stream);
  if (t.bm == 128) return k16 ? s2_launch_cfg<128, 64, 16, PASS>(a, stream) : s2_launch_cfg<128, 64, 4, PASS>(a, stream);
  return k16 ? s2_launch_cfg<64, 64, 16, PASS>(a, stream) : s2_launch_cfg<64, 64, 4, PASS>(a, stream);
}

static void s2_args_init(S2Args& a) {
  memset(&a, 0, sizeof(a));
  a.c.act_slope = 1.f;
  a.c.ksplit = 1;
  a.c.bn_slope = 1.f;
  a.c.bn_nslot = 1;
}
static void s2_class_rows(S2Class& c, int B, int Hr, int Wr) {
  c.Hr = Hr; c.Wr = Wr; c.M = B * Hr * Wr;
  c.divW = ssp_fastdiv((unsigned)(Wr > 0 ? Wr : 1));
  c.divH = ssp_fastdiv((unsigned)(Hr > 0 ? Hr : 1));
}
static void s2_class_tap(S2Class& c, int oy, int ox, int widx) {
  const unsigned code = (unsigned)(oy + 1) | ((unsigned)(ox + 1) << 2) | ((unsigned)widx << 4);
  if (c.ntap < 8) c.taps_lo |= (unsigned long long)code << (8 * c.ntap);
  else c.taps_hi = code;
  ++c.ntap;
}

#define S2_CHECK_COMMON(name, B, H, W, R)                                                                         \
  SSP_CHECK_ARG(R == 1 || R == 3, name ": only 1x1 and 3x3 (pad 1) filters are supported (got %d)", R);        \
  SSP_CHECK_ARG(B > 0 && H > 0 && W > 0, name ": B, H, W must be positive");                                   \
  SSP_CHECK_ARG((int64_t)B * H * W < (1ll << 31), name ": too many pixels")

int ssp_conv_s2_fwd_launch(const float* in, const float* wt, float* out, const float* bias, float* stats, int B, int H, int W,
                           int Cin, int Cout, int ldin, int ldout, int R, int accumulate, const float* escale,
                           float act_slope, hipStream_t stream) {
  S2_CHECK_COMMON("conv_s2_fwd", B, H, W, R);
  SSP_CHECK_ARG(Cin % 4 == 0 && Cin > 0, "conv_s2_fwd: Cin must be a positive multiple of 4 (got %d)", Cin);
  SSP_CHECK_ARG(ldin % 4 == 0 && ldin >= Cin, "conv_s2_fwd: ldin must be a multiple of 4 and >= Cin");
  SSP_CHECK_ARG(Cout > 0 && ldout % 4 == 0 && ldout >= Cout, "conv_s2_fwd: ldout must be a multiple of 4 and >= Cout");
  SSP_CHECK_ARG(in != nullptr && wt != nullptr && out != nullptr, "conv_s2_fwd: in / wt / out must not be NULL");
  SSP_CHECK_ARG(((((uintptr_t)in) | ((uintptr_t)wt) | ((uintptr_t)out)) & 15) == 0, "conv_s2_fwd: in / wt / out must be 16-byte aligned");
  SSP_CHECK_ARG(!(accumulate && stats != nullptr), "conv_s2_fwd: statistics of an accumulating launch are not defined");
  const int Ho = s2_out(H, R), Wo = s2_out(W, R), pad = R / 2;
  S2Args a;
  s2_args_init(a);
  a.c.in = in; a.c.wt = wt; a.c.out = out; a.c.bias = bias; a.c.escale = escale; a.c.act_slope = act_slope; a.c.stats = stats;
  a.c.H = Ho; a.c.W = Wo; a.c.Cin = Cin; a.c.Cout = Cout; a.c.ldin = ldin; a.c.ldout = ldout; a.c.R = R;
  a.c.M = B * Ho * Wo; a.c.accumulate = accumulate;
  a.Hs = H; a.Ws = W; a.ms = 2; a.Hd = Ho; a.Wd = Wo; a.ds = 1; a.wld = R * R * Cin; a.ncls = 1;
  s2_class_rows(a.cls[0], B, Ho, Wo);
  for (int r = 0; r < R; ++r)
    for (int s = 0; s < R; ++s) s2_class_tap(a.cls[0], r - pad, s - pad, r * R + s);
  SspProfScope prof(SSP_PROF_CONV_FWD, stream, 2.0 * (double)a.c.M * Cout * (double)(R * R * Cin));
  return s2_launch<0>(a, stream);
}

int ssp_conv_s2_dgrad_launch(const float* dy, const float* wt, float* dx, int B, int H, int W, int Cout_dy, int Cin_dx,
                             int lddy, int lddx, int R, int accumulate, hipStream_t stream, int no_tap_split) {
  S2_CHECK_COMMON("conv_s2_dgrad", B, H, W, R);
  SSP_CHECK_ARG(Cout_dy % 4 == 0 && Cout_dy > 0, "conv_s2_dgrad: Cout_dy must be a positive multiple of 4 (got %d)", Cout_dy);
  SSP_CHECK_ARG(lddy % 4 == 0 && lddy >= Cout_dy, "conv_s2_dgrad: lddy must be a multiple of 4 and >= Cout_dy");
  SSP_CHECK_ARG(Cin_dx > 0 && lddx % 4 == 0 && lddx >= Cin_dx, "conv_s2_dgrad: lddx must be a multiple of 4 and >= Cin_dx > 0");
  SSP_CHECK_ARG(dy != nullptr && wt != nullptr && dx != nullptr, "conv_s2_dgrad: dy / wt / dx must not be NULL");
  SSP_CHECK_ARG(((((uintptr_t)dy) | ((uintptr_t)wt) | ((uintptr_t)dx)) & 15) == 0, "conv_s2_dgrad: dy / wt / dx must be 16-byte aligned");
  const int Ho = s2_out(H, R), Wo = s2_out(W, R), taps = R * R;
  S2Args a;
  s2_args_init(a);
  a.c.in = dy; a.c.wt = wt; a.c.out = dx;
  a.c.H = H; a.c.W = W; a.c.Cin = Cout_dy; a.c.Cout = Cin_dx; a.c.ldin = lddy; a.c.ldout = lddx; a.c.R = R;
  a.c.accumulate = accumulate;
  a.Hs = Ho; a.Ws = Wo; a.ms = 1; a.Hd = H; a.Wd = W; a.ds = 2; a.wld = taps * Cout_dy;
  // parity classes, most taps first; per dimension at 3x3: even -> tap 1 at offset 0; odd -> tap 0 at offset +1 and tap 2
  // at offset 0; at 1x1: even -> tap 0 at offset 0, odd -> nothing.  The operand stores tap t at index taps - 1 - t.
  double flops = 0.0;
  for (int cls = 3; cls >= 0; --cls) {
    const int py = cls >> 1, px = cls & 1;
    if (R == 1 && (py || px)) continue;
    const int Hr = (H - py + 1) / 2, Wr = (W - px + 1) / 2;
    if (Hr <= 0 || Wr <= 0) continue;
    S2Class& c = a.cls[a.ncls++];
    c.py = py; c.px = px;
    s2_class_rows(c, B, Hr, Wr);
    int ry[2], oy[2], ny = 0, rx[2], ox[2], nx = 0;
    if (R == 1) { ry[0] = 0; oy[0] = 0; ny = 1; rx[0] = 0; ox[0] = 0; nx = 1; }
    else {
      if (py) { ry[0] = 0; oy[0] = 1; ry[1] = 2; oy[1] = 0; ny = 2; } else { ry[0] = 1; oy[0] = 0; ny = 1; }
      if (px) { rx[0] = 0; ox[0] = 1; rx[1] = 2; ox[1] = 0; nx = 2; } else { rx[0] = 1; ox[0] = 0; nx = 1; }
    }
    for (int i = 0; i < ny; ++i)
      for (int j = 0; j < nx; ++j) s2_class_tap(c, oy[i], ox[j], taps - 1 - (ry[i] * R + rx[j]));
    flops += 2.0 * (double)c.M * Cin_dx * (double)c.ntap * Cout_dy;
  }
  a.c.M = a.cls[0].M;
  SspProfScope prof(SSP_PROF_CONV_DGRAD, stream, flops);
  // Small grids (3x3 only; a pure function of the shape): with fewer workgroups than the chip holds at once (2 per CU) the
  // launch lasts as long as its longest workgroup, a four-tap tile of the (odd, odd) class, while most CUs idle.  Those
  // launches give every (class, tap) pair workgroups of its own - equal K everywhere, 9/4 times the workgroups - and the
  // taps of a pixel meet in dx through fp32 atomic adds (dx zeroed first when not accumulating).
  bool split = false;
  if (R == 3) {
    int64_t Ms[4];
    for (int k = 0; k < a.ncls; ++k) Ms[k] = a.cls[k].M;
    const S2Tile t = s2_tile(Ms, a.ncls, Cin_dx);
    int64_t wgs = 0;
    for (int k = 0; k < a.ncls; ++k) wgs += (Ms[k] + t.bm - 1) / t.bm;
    split = wgs * ssp_cdiv(Cin_dx, t.bn) < 512 && !no_tap_split;      // (ordered form: one thread per pixel on every grid)
  }
  if (split) {
    S2Args b = a;
    b.ncls = 0;
    for (int k = 0; k < a.ncls; ++k)
      for (int tp = 0; tp < a.cls[k].ntap; ++tp) {
        S2Class& c = b.cls[b.ncls++];
        c = a.cls[k];
        c.ntap = 1;
        c.taps_lo = (a.cls[k].taps_lo >> (8 * tp)) & 0xffull;      // (a class has at most four taps)
        c.taps_hi = 0;
      }
    b.c.accumulate = 2;
    a = b;
  }
  if ((split || R == 1) && !accumulate && (split || H > 1 || W > 1)) {
    const int64_t total = (int64_t)B * H * W * Cin_dx;
    int64_t g = (total + 255) / 256;
    if (g > 65536) g = 65536;
    hipLaunchKernelGGL(conv_s2_zero_kernel, dim3((unsigned)g), dim3(256), 0, stream, dx, lddx, Cin_dx, H, W, total, split ? 0 : 1);
    SSP_CHECK_LAUNCH("conv_s2_zero");
  }
  return s2_launch<1>(a, stream);
}

// ---- filter gradient: dw[co][tap][ci] += sum_p dy[p][co] * x[2*yo + r - pad][2*xo + s - pad][ci] over the output pixels ----
struct S2WgradArgs {
  const float* dy;
  const float* x;
  float* dw;
  int H, W, Ho, Wo, Cin, Cout, lddy, ldx, R, M;
  int ntile_co, ntile_ci, nsplit, chunk_m;
  SspFastDiv divW, divH;
  int64_t slab_floats;      // ordered form (wgrad_ordered.h): > 0 = dw is the workspace [nsplit][slab_floats], plain stores
};

// conv_wgrad.hip's register-staged kernel (GEMM per tap: rows = cout, cols = cin, reduction = output pixels split across
// workgroups, partial tiles added to dw with fp32 atomics) with the strided gather on the x operand
template <int BMO, int BNI, int WM, int WN, int WK>
__global__ void __launch_bounds__(256, 2) conv_s2_wgrad_kernel(S2WgradArgs p) {
  static_assert(WM * WN * WK == 4, "256-thread workgroups");
  constexpr int NT = 256;
  constexpr int RA = 16 * WK;  // pixel rows staged per iteration (16 per k-group of waves)
  constexpr int WTM = BMO / WM, WTN = BNI / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int F4A = RA * BMO / 4, F4B = RA * BNI / 4;
  constexpr int APASS = (F4A + NT - 1) / NT, BPASS = (F4B + NT - 1) / NT;
  constexpr int SLOT = RA * (BMO + BNI);
  static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile must be a multiple of 32x32");

  extern __shared__ __attribute__((aligned(16))) float smem[];   // 3 * SLOT floats: per slot [RA][BMO] then [RA][BNI]

  const int taps = p.R * p.R;
  int bid = blockIdx.x;
  const int split = bid % p.nsplit; bid /= p.nsplit;
  const int tap = bid % taps; bid /= taps;
  const int tile_ci = bid % p.ntile_ci;
  const int tile_co = bid / p.ntile_ci;
  const int co0 = tile_co * BMO, ci0 = tile_ci * BNI;
  const int pad = p.R >> 1;
  const int dy = tap / p.R - pad, dx = tap % p.R - pad;

  const int m_begin = split * p.chunk_m;
  const int m_end = min(p.M, m_begin + p.chunk_m);
  const int niter = (m_end - m_begin + RA - 1) / RA;
  if (niter <= 0) return;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wk = wid / (WM * WN);
  const int wmn = wid % (WM * WN);
  const int wm = wmn / WN, wn = wmn % WN;
  const int li = lane & 31, lh = lane >> 5;

  // loader constants: (row, channel) of each pass; channels beyond the tensor read channel 0 and are zeroed
  int a_row[APASS], a_col[APASS], b_row[BPASS], b_col[BPASS];
  bool a_cok[APASS], b_cok[BPASS];
#pragma unroll
  for (int i = 0; i < APASS; ++i) {
    int idx = tid + i * NT;
    a_row[i] = idx / (BMO / 4);
    int co = co0 + (idx % (BMO / 4)) * 4;
    a_cok[i] = (idx < F4A) && (co < p.Cout);   // lddy % 4 == 0 and >= Cout: the float4 at co stays inside the row
    a_col[i] = a_cok[i] ? co : 0;
  }
#pragma unroll
  for (int i = 0; i < BPASS; ++i) {
    int idx = tid + i * NT;
    b_row[i] = idx / (BNI / 4);
    int ci = ci0 + (idx % (BNI / 4)) * 4;
    b_cok[i] = (idx < F4B) && (ci < p.Cin);
    b_col[i] = b_cok[i] ? ci : 0;
  }

  f32x4 a_reg[APASS], b_reg[BPASS];
  unsigned okmask = 0;   // bits [0,APASS): dy rows valid; bits [8,8+BPASS): x rows valid
  int ld_m = m_begin;
  auto load_global = [&](f32x4 (&ar)[APASS], f32x4 (&br)[BPASS], unsigned& okm) {
    okm = 0;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      int m = ld_m + a_row[i];
      bool ok = a_cok[i] && (m < m_end);
      int mc = ok ? m : m_begin;
      ar[i] = *reinterpret_cast<const f32x4*>(p.dy + (int64_t)mc * p.lddy + a_col[i]);
      okm |= ok ? (1u << i) : 0u;
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
      int m = ld_m + b_row[i];
      const bool inr = m < m_end;
      const int mc = inr ? m : m_begin;
      const unsigned t = ssp_div((unsigned)mc, p.divW);
      const int xo = mc - (int)t * p.Wo;
      const unsigned b = ssp_div(t, p.divH);
      const int yo = (int)t - (int)b * p.Ho;
      const int yy = 2 * yo + dy, xx = 2 * xo + dx;
      bool ok = b_cok[i] && inr && ((unsigned)yy < (unsigned)p.H) && ((unsigned)xx < (unsigned)p.W);
      int64_t off = ok ? ((((int64_t)b * p.H + yy) * p.W + xx) * p.ldx) : (int64_t)0;
      br[i] = *reinterpret_cast<const f32x4*>(p.x + off + b_col[i]);
      okm |= ok ? (1u << (8 + i)) : 0u;
    }
    ld_m += RA;   // past m_end every row is masked off, so running ahead is harmless
  };
  auto store_lds = [&](int slot, const f32x4 (&ar)[APASS], const f32x4 (&br)[BPASS], unsigned okm) {
    float* As = smem + slot * SLOT;
    float* Bs = As + RA * BMO;
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
      int idx = tid + i * NT;
      const bool ok = (okm >> i) & 1u;
      f32x4 v;
      v[0] = ok ? ar[i][0] : 0.f; v[1] = ok ? ar[i][1] : 0.f; v[2] = ok ? ar[i][2] : 0.f; v[3] = ok ? ar[i][3] : 0.f;
      if (F4A % NT == 0 || idx < F4A) *reinterpret_cast<f32x4*>(As + idx * 4) = v;
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
      int idx = tid + i * NT;
      const bool ok = (okm >> (8 + i)) & 1u;
      f32x4 v;
      v[0] = ok ? br[i][0] : 0.f; v[1] = ok ? br[i][1] : 0.f; v[2] = ok ? br[i][2] : 0.f; v[3] = ok ? br[i][3] : 0.f;
      if (F4B % NT == 0 || idx < F4B) *reinterpret_cast<f32x4*>(Bs + idx * 4) = v;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  {
    f32x4 a0[APASS], b0[BPASS], a1[APASS], b1[BPASS];
    unsigned k0 = 0, k1 = 0;
    load_global(a0, b0, k0);
    load_global(a1, b1, k1);
    load_global(a_reg, b_reg, okmask);
    store_lds(0, a0, b0, k0);
    store_lds(1, a1, b1, k1);
  }
  __syncthreads();

  // MFMA operands of k-step kk: A[i=cout][k=pixel row 2kk+lh], B[k][j=cin]: conflict-free ds_read_b32 rows
  auto read_frag = [&](int slot, int kk, float (&av)[TM], float (&bv)[TN]) {
    const float* Ab = smem + slot * SLOT + (wk * 16 + lh + kk * 2) * BMO + wm * WTM + li;
    const float* Bb = smem + slot * SLOT + RA * BMO + (wk * 16 + lh + kk * 2) * BNI + wn * WTN + li;
#pragma unroll
    for (int i = 0; i < TM; ++i) av[i] = Ab[i * 32];
#pragma unroll
    for (int j = 0; j < TN; ++j) bv[j] = Bb[j * 32];
  };
  float av[2][TM], bv[2][TN];
  read_frag(0, 0, av[0], bv[0]);

  int slot = 0;
  for (int it = 0; it < niter; ++it) {
    const int slot1 = (slot == 2) ? 0 : slot + 1;
    const int slot2 = (slot1 == 2) ? 0 : slot1 + 1;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      if (kk + 1 < 8) {
        read_frag(slot, kk + 1, av[(kk + 1) & 1], bv[(kk + 1) & 1]);
      } else {
        read_frag(slot1, 0, av[0], bv[0]);
      }
      if (kk == 0) {
        store_lds(slot2, a_reg, b_reg, okmask);
        load_global(a_reg, b_reg, okmask);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk & 1][i], bv[kk & 1][j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    slot = slot1;
  }

  if (p.slab_floats > 0) {      // ordered form: plain stores into this pixel range's slab
    ssp_wgrad_ordered_store<BMO, BNI, WM, WN, WK>(acc, smem, p.dw + (int64_t)split * p.slab_floats, p.Cin, p.Cout, taps, tap, co0, ci0);
    return;
  }
  // (WK > 1: the k-groups of waves hold partial sums of the same filter tile; every group adds its own)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      int ci = ci0 + wn * WTN + j * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int co = co0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (co < p.Cout && ci < p.Cin)
          atomicAdd(p.dw + ((int64_t)co * taps + tap) * p.Cin + ci, acc[i][j][r]);
      }
    }
}

template <int BMO, int BNI, int WM, int WN, int WK>
static int s2_launch_wgrad(S2WgradArgs a, hipStream_t stream) {
  constexpr int RA = 16 * WK;
  a.ntile_co = ssp_cdiv(a.Cout, BMO);
  a.ntile_ci = ssp_cdiv(a.Cin, BNI);
  const int64_t tiles = (int64_t)a.ntile_co * a.ntile_ci * a.R * a.R;
  const int lds_bytes = 3 * RA * (BMO + BNI) * 4;
  auto kern = conv_s2_wgrad_kernel<BMO, BNI, WM, WN, WK>;
  static SspKernelCache cache;   // per instantiation, per device
  int slots = 0;                 // workgroups resident on the whole chip (occupancy x CUs)
  if (int rc = ssp_kernel_prepare((const void*)kern, lds_bytes, 256, &cache, &slots, "conv_s2_wgrad")) return rc;
  if (a.slab_floats > 0) {       // ordered form: the pixel ranges were fixed on the host (ssp_wgrad_ordered_plan)
    SSP_CHECK_ARG(a.chunk_m % RA == 0 && a.nsplit >= 1 && tiles * a.nsplit < (1ll << 31), "conv_s2_wgrad (ordered): bad pixel ranges");
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * a.nsplit)), dim3(256), lds_bytes, stream, a);
    SSP_CHECK_LAUNCH("conv_s2_wgrad(ordered)");
    return SSP_OK;
  }
  // pixel split as conv_wgrad.hip: a grid of 2..5 whole resident waves of workgroups, >= 8 staged chunks per workgroup
  const int64_t max_split = (a.M + RA * 8 - 1) / (RA * 8);
  int64_t lo = (2 * (int64_t)slots + tiles - 1) / tiles, hi = (5 * (int64_t)slots) / tiles;
  if (lo < 1) lo = 1;
  if (hi < lo) hi = lo;
  if (lo > max_split) lo = max_split;
  if (hi > max_split) hi = max_split;
  int64_t nsplit = lo;
  double best = -1.0;
  for (int64_t sp = lo; sp <= hi; ++sp) {
    const double waves = (double)(tiles * sp) / slots;
    const double eff = waves / (double)((tiles * sp + slots - 1) / slots);
    if (eff > best + 1e-3) { best = eff; nsplit = sp; }
  }
  int64_t chunk = (a.M + nsplit - 1) / nsplit;
  chunk = (chunk + RA - 1) / RA * RA;
  nsplit = (a.M + chunk - 1) / chunk;
  a.nsplit = (int)nsplit;
  a.chunk_m = (int)chunk;
  SSP_CHECK_ARG(tiles * nsplit < (1ll << 31), "conv_s2_wgrad: grid too large");
  hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * nsplit)), dim3(256), lds_bytes, stream, a);
  SSP_CHECK_LAUNCH("conv_s2_wgrad");
  return SSP_OK;
}

static int s2_wgrad_launch_impl(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int lddy,
                                int ldx, int R, int nsplit, int chunk_m, int64_t slab_floats, hipStream_t stream) {
  S2_CHECK_COMMON("conv_s2_wgrad", B, H, W, R);
  SSP_CHECK_ARG(Cin % 4 == 0 && Cin > 0, "conv_s2_wgrad: Cin must be a positive multiple of 4 (got %d)", Cin);
  SSP_CHECK_ARG(ldx % 4 == 0 && ldx >= Cin, "conv_s2_wgrad: ldx must be a multiple of 4 and >= Cin");
  SSP_CHECK_ARG(Cout > 0 && lddy % 4 == 0 && lddy >= Cout, "conv_s2_wgrad: lddy must be a multiple of 4 and >= Cout");
  SSP_CHECK_ARG(dy != nullptr && x != nullptr && dw != nullptr, "conv_s2_wgrad: dy / x / dw must not be NULL");
  SSP_CHECK_ARG(((((uintptr_t)dy) | ((uintptr_t)x)) & 15) == 0, "conv_s2_wgrad: dy / x must be 16-byte aligned");
  S2WgradArgs a;
  a.dy = dy; a.x = x; a.dw = dw;
  a.H = H; a.W = W; a.Ho = s2_out(H, R); a.Wo = s2_out(W, R);
  a.Cin = Cin; a.Cout = Cout; a.lddy = lddy; a.ldx = ldx; a.R = R; a.M = B * a.Ho * a.Wo;
  a.divW = ssp_fastdiv((unsigned)a.Wo); a.divH = ssp_fastdiv((unsigned)a.Ho);
  a.ntile_co = a.ntile_ci = 0;
  a.nsplit = nsplit; a.chunk_m = chunk_m; a.slab_floats = slab_floats;
  const int bmo = Cout > 64 ? 128 : (Cout > 32 ? 64 : 32), bni = Cin > 64 ? 128 : (Cin > 32 ? 64 : 32);
  switch (bmo * 1000 + bni) {
    case 128128: return s2_launch_wgrad<128, 128, 2, 2, 1>(a, stream);
    case 128064: return s2_launch_wgrad<128, 64, 2, 2, 1>(a, stream);
    case 128032: return s2_launch_wgrad<128, 32, 4, 1, 1>(a, stream);
    case 64128: return s2_launch_wgrad<64, 128, 2, 2, 1>(a, stream);
    case 64064: return s2_launch_wgrad<64, 64, 2, 2, 1>(a, stream);
    case 64032: return s2_launch_wgrad<64, 32, 2, 1, 2>(a, stream);
    case 32128: return s2_launch_wgrad<32, 128, 1, 4, 1>(a, stream);
    case 32064: return s2_launch_wgrad<32, 64, 1, 2, 2>(a, stream);
    default: return s2_launch_wgrad<32, 32, 1, 1, 4>(a, stream);
  }
}

int ssp_conv_s2_wgrad_launch(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int lddy,
                             int ldx, int R, hipStream_t stream) {
  SspProfScope prof(SSP_PROF_CONV_WGRAD, stream, 2.0 * (double)B * s2_out(H, R) * s2_out(W, R) * Cout * (double)(R * R * Cin));
  return s2_wgrad_launch_impl(dy, x, dw, B, H, W, Cin, Cout, lddy, ldx, R, 0, 0, 0, stream);
}
int ssp_conv_s2_wgrad_ordered_launch(const float* dy, const float* x, float* ws, int B, int H, int W, int Cin, int Cout, int lddy,
                                     int ldx, int R, const SspWgradOrderedPlan& pl, hipStream_t stream) {
  return s2_wgrad_launch_impl(dy, x, ws, B, H, W, Cin, Cout, lddy, ldx, R, pl.nsplit, pl.chunk_m, pl.slab_floats, stream);
}

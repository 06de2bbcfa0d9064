// Depthwise 3x3 convolution (Darknet [convolutional] groups = channels = filters, pad = 1, stride 1 or 2): forward, data
// gradient and filter gradient on fp32 NHWC maps ([pixels][ld], channels fastest).  The contract is the header comment of
// this family in include/ssp_hip.h; this file adds how the work is cut.
//
// Every kernel is an HBM-bound pass without MFMA: a lane owns one channel QUAD (16-byte accesses) and the 36 filter
// floats of that quad, w[c*9 + tap], read from the parameter's own (C, 1, 3, 3) memory as nine 16-byte loads.
//
// Forward (and the stride-1 data gradient, which is the forward with the taps flipped): a work item is (strip, quad), a
// strip = DW_S = 4 consecutive output pixels of one output row.  The item walks the three input rows of its strip; of
// each it loads the (DW_S - 1) * stride + 3 pixels under the strip ONCE into registers and uses every value for all the
// (output pixel, tap) pairs it serves - 18 (stride 1) or 27 (stride 2) loads for 36 products per channel.  Items are
// numbered quads fastest, so the lanes of a wave read consecutive 16-byte pieces of a pixel row.  A workgroup owns one
// TILE of NS consecutive strips (NS = 1024 / quads, 1..64: ~1024 items) and all channels of it.
//   statistics: every item leaves (mean, M2) of its <= 4 values per channel in the LDS; then part p of channel c (256 / C
//   parts, one when C >= 256) Chan-combines the strips [p * ceil(NS / parts), ...) of the tile in ascending order, and one
//   thread per channel combines the parts in ascending order: fp32, a fixed order, no atomics.  The tile's pixel count
//   follows the pairs (the counted format of ssp_bn_fwd_finalize, tile_m = 0): tiles end in partial strips.
//
// Stride-2 data gradient: a work item is one channel quad of one 2 x 2 block of dx pixels (2a..2a+1, 2b..2b+1) - the four
// parity classes in one thread, so no lane diverges and the filter sits in registers under constant indices.  It loads
// the four dy pixels (a..a+1, b..b+1) once each and forms the 1 + 2 + 2 + 4 products of the block.
//
// Filter gradient: launch 1 - workgroup (range, group of <= 16 quads) sums dy * x over the strips of a fixed range: thread (quad,
// strip lane) takes strips lane, lane + SL, ... of the range in ascending order into 36 register sums, the lanes' sums go
// through the LDS and are added in ascending lane order into partial[range][C][9]; launch 2 - one thread per filter element
// adds the ranges in ascending order in float64, rounds once and stores (or adds the earlier content last).
#include "ssp_common.h"

#define DW_S 4
#define DW_ITEMS 1024
#define DW_NS_MAX 64
#define DW_RANGES_MAX 512

struct DwGeom {
  int Ho, Wo, SPR, G, NS, tiles;      // output map, strips per output row, quads, strips per forward tile, tiles
  int64_t strips;
  int QB, QG, SL, RS, ranges;         // filter gradient: quads per workgroup, quad groups, strip lanes, strips per range
};

static DwGeom dw_geom(int B, int H, int W, int C, int stride) {
  DwGeom g;
  g.Ho = (H - 1) / stride + 1;
  g.Wo = (W - 1) / stride + 1;
  g.SPR = (g.Wo + DW_S - 1) / DW_S;
  g.G = C / 4;
  g.strips = (int64_t)B * g.Ho * g.SPR;
  int ns = DW_ITEMS / (g.G > 0 ? g.G : 1);
  g.NS = ns < 1 ? 1 : (ns > DW_NS_MAX ? DW_NS_MAX : ns);
  g.tiles = (int)((g.strips + g.NS - 1) / g.NS);
  // 16 quads (256 contiguous bytes of a pixel row) per workgroup: deep layers get G / 16 quad groups per range, so the grid
  // fills the chip while the ranges - the length of the finishing pass's sequential chain - stay few
  int qb = 1;
  while (qb < g.G && qb < 16) qb *= 2;
  g.QB = qb;
  g.QG = (g.G + qb - 1) / qb;
  g.SL = 256 / qb;
  int64_t rs = (g.strips + DW_RANGES_MAX - 1) / DW_RANGES_MAX;
  if (rs < 2 * g.SL) rs = 2 * g.SL;
  rs = (rs + g.SL - 1) / g.SL * g.SL;
  g.RS = (int)rs;
  g.ranges = (int)((g.strips + rs - 1) / rs);
  return g;
}

__device__ __forceinline__ f32x4 dw_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void dw_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 dw_zero() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }

// the quad's 36 filter floats: element (channel k of the quad, tap t) is wq[(k * 9 + t) / 4][(k * 9 + t) % 4]
struct DwFilter {
  f32x4 wq[9];
  __device__ __forceinline__ void load(const float* w, int c) {
#pragma unroll
    for (int i = 0; i < 9; ++i) wq[i] = dw_ld4(w + (int64_t)c * 9 + i * 4);
  }
  __device__ __forceinline__ float at(int k, int t) const { return wq[(k * 9 + t) >> 2][(k * 9 + t) & 3]; }
};

__device__ __forceinline__ void dw_chan(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
  const float nt = n + nb;
  if (nb > 0.f) {
    const float d = mb - mean, f = nb / nt;
    mean += d * f;
    m2 += m2b + d * d * n * f;
    n = nt;
  }
}

// forward (FLIP = false) and stride-1 data gradient (FLIP = true, STRIDE = 1): out = epilogue(sum over the window)
template <int STRIDE, bool FLIP, bool STATS>
__global__ void __launch_bounds__(256) dw_fwd_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                     float* __restrict__ out, const float* __restrict__ scale,
                                                     const float* __restrict__ shift, float slope, int accumulate,
                                                     float* __restrict__ stats, int ntile, int H, int W, int C, int Ho, int Wo,
                                                     int SPR, int64_t strips, int NS, int ldin, int ldout) {
  constexpr int NCOL = (DW_S - 1) * STRIDE + 3;
  __shared__ __attribute__((aligned(16))) float item[STATS ? DW_ITEMS * 8 : 4];      // per item: mean[4] | M2[4]
  __shared__ float pn[STATS ? 256 : 1], pmean[STATS ? 256 : 1], pm2[STATS ? 256 : 1];
  const int G = C >> 2, tid = threadIdx.x;
  const int64_t s0 = (int64_t)blockIdx.x * NS;
  const int nitems = NS * G;
  for (int j = tid; j < nitems; j += 256) {
    const int sl = j / G, q = j - sl * G, c = q * 4;
    const int64_t s = s0 + sl;
    f32x4 mean = dw_zero(), m2 = dw_zero();
    int npx = 0;
    if (s < strips) {
      const int xs = (int)(s % SPR);
      const int64_t by = s / SPR;
      const int yo = (int)(by % Ho), b = (int)(by / Ho), xo0 = xs * DW_S;
      DwFilter f;
      f.load(w, c);
      f32x4 acc[DW_S];
#pragma unroll
      for (int jx = 0; jx < DW_S; ++jx) acc[jx] = dw_zero();
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int yi = yo * STRIDE + r - 1;
        if (yi < 0 || yi >= H) continue;
        const float* row = in + ((int64_t)b * H + yi) * W * ldin + c;
        f32x4 win[NCOL];
#pragma unroll
        for (int k = 0; k < NCOL; ++k) {
          const int xi = xo0 * STRIDE + k - 1;
          win[k] = (xi >= 0 && xi < W) ? dw_ld4(row + (int64_t)xi * ldin) : dw_zero();
        }
#pragma unroll
        for (int jx = 0; jx < DW_S; ++jx)
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            const int tap = FLIP ? (2 - r) * 3 + (2 - t) : r * 3 + t;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[jx][k] = fmaf(win[jx * STRIDE + t][k], f.at(k, tap), acc[jx][k]);
          }
      }
      f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = dw_zero();
      if (scale != nullptr) sc = dw_ld4(scale + c);
      if (shift != nullptr) sh = dw_ld4(shift + c);
      npx = min(DW_S, Wo - xo0);
      float* dst = out + (((int64_t)b * Ho + yo) * Wo + xo0) * ldout + c;
#pragma unroll
      for (int jx = 0; jx < DW_S; ++jx) {
        if (jx < npx) {
          f32x4 v = acc[jx];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float y = v[k];
            if (scale != nullptr) y = sc[k] * y;
            if (shift != nullptr) y = y + sh[k];
            v[k] = y > 0.f ? y : y * slope;
          }
          if (accumulate) {
            const f32x4 o = dw_ld4(dst + (int64_t)jx * ldout);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = o[k] + v[k];
          }
          dw_st4(dst + (int64_t)jx * ldout, v);
          acc[jx] = v;
        }
      }
      if (STATS) {
        const float inv = 1.f / (float)npx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float sum = 0.f;
#pragma unroll
          for (int jx = 0; jx < DW_S; ++jx) sum += jx < npx ? acc[jx][k] : 0.f;
          const float mu = sum * inv;
          float dd = 0.f;
#pragma unroll
          for (int jx = 0; jx < DW_S; ++jx) {
            const float d = acc[jx][k] - mu;
            dd += jx < npx ? d * d : 0.f;
          }
          mean[k] = mu;
          m2[k] = dd;
        }
      }
    }
    if (STATS) {
      if (NS == 1) {      // the item IS the tile (more than 512 quads): no LDS stage
        if (s < strips) {
          float* st = stats + ((int64_t)blockIdx.x * C + c) * 2;
          f32x4 a = {mean[0], m2[0], mean[1], m2[1]}, b2 = {mean[2], m2[2], mean[3], m2[3]};
          dw_st4(st, a);
          dw_st4(st + 4, b2);
          if (q == 0) stats[(int64_t)ntile * C * 2 + blockIdx.x] = (float)npx;
        }
      } else {
        dw_st4(&item[j * 8], mean);
        dw_st4(&item[j * 8 + 4], m2);
      }
    }
  }
  if (STATS && NS > 1) {
    __syncthreads();
    const int P = C >= 256 ? 1 : 256 / C;
    const int SPP = (NS + P - 1) / P;
    for (int e = tid; e < C * P; e += 256) {
      const int c = e % C, part = e / C;
      float n = 0.f, mu = 0.f, m2 = 0.f;
      const int hi = min(NS, (part + 1) * SPP);
      for (int sl = part * SPP; sl < hi; ++sl) {
        const int64_t s = s0 + sl;
        if (s >= strips) break;
        const float nb = (float)min(DW_S, Wo - (int)(s % SPR) * DW_S);
        const float* it = &item[(sl * G + (c >> 2)) * 8 + (c & 3)];
        dw_chan(n, mu, m2, nb, it[0], it[4]);
      }
      if (P == 1) {
        float* st = stats + ((int64_t)blockIdx.x * C + c) * 2;
        st[0] = mu;
        st[1] = m2;
        if (c == 0) stats[(int64_t)ntile * C * 2 + blockIdx.x] = n;
      } else {
        pn[e] = n; pmean[e] = mu; pm2[e] = m2;
      }
    }
    if (P > 1) {
      __syncthreads();
      if (tid < C) {
        float n = 0.f, mu = 0.f, m2 = 0.f;
        for (int part = 0; part < P; ++part) dw_chan(n, mu, m2, pn[part * C + tid], pmean[part * C + tid], pm2[part * C + tid]);
        float* st = stats + ((int64_t)blockIdx.x * C + tid) * 2;
        st[0] = mu;
        st[1] = m2;
        if (tid == 0) stats[(int64_t)ntile * C * 2 + blockIdx.x] = n;
      }
    }
  }
}

// stride-2 data gradient: H x W = dx's map, Ho x Wo = dy's; one item = a 2 x 2 block of dx pixels of one quad
__global__ void __launch_bounds__(256) dw_dgrad_s2_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                          float* __restrict__ dx, int B, int H, int W, int C, int Ho, int Wo,
                                                          int lddy, int lddx, int accumulate) {
  const int G = C >> 2;
  const int64_t total = (int64_t)B * Ho * Wo * G;      // (ceil(H / 2) = Ho blocks of rows, ceil(W / 2) = Wo of columns)
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % G) * 4;
    const int64_t p = idx / G;
    const int bb = (int)(p % Wo);
    const int64_t ba = p / Wo;
    const int a = (int)(ba % Ho), b = (int)(ba / Ho);
    DwFilter f;
    f.load(w, c);
    const float* q = dy + (((int64_t)b * Ho + a) * Wo + bb) * lddy + c;
    const bool right = bb + 1 < Wo, down = a + 1 < Ho;
    const f32x4 d00 = dw_ld4(q);
    const f32x4 d01 = right ? dw_ld4(q + lddy) : dw_zero();
    const f32x4 d10 = down ? dw_ld4(q + (int64_t)Wo * lddy) : dw_zero();
    const f32x4 d11 = (right && down) ? dw_ld4(q + ((int64_t)Wo + 1) * lddy) : dw_zero();
    f32x4 ee, eo, oe, oo;      // (row parity, column parity) of the dx pixel; products in ascending tap order
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ee[k] = d00[k] * f.at(k, 4);
      eo[k] = fmaf(d00[k], f.at(k, 5), d01[k] * f.at(k, 3));
      oe[k] = fmaf(d00[k], f.at(k, 7), d10[k] * f.at(k, 1));
      oo[k] = fmaf(d00[k], f.at(k, 8), fmaf(d01[k], f.at(k, 6), fmaf(d10[k], f.at(k, 2), d11[k] * f.at(k, 0))));
    }
    float* d = dx + (((int64_t)b * H + 2 * a) * W + 2 * bb) * lddx + c;
    const bool xodd = 2 * bb + 1 < W, yodd = 2 * a + 1 < H;
    if (accumulate) {
      const f32x4 o0 = dw_ld4(d);
      const f32x4 o1 = xodd ? dw_ld4(d + lddx) : dw_zero();
      const f32x4 o2 = yodd ? dw_ld4(d + (int64_t)W * lddx) : dw_zero();
      const f32x4 o3 = (xodd && yodd) ? dw_ld4(d + ((int64_t)W + 1) * lddx) : dw_zero();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ee[k] = o0[k] + ee[k]; eo[k] = o1[k] + eo[k]; oe[k] = o2[k] + oe[k]; oo[k] = o3[k] + oo[k];
      }
    }
    dw_st4(d, ee);
    if (xodd) dw_st4(d + lddx, eo);
    if (yodd) dw_st4(d + (int64_t)W * lddx, oe);
    if (xodd && yodd) dw_st4(d + ((int64_t)W + 1) * lddx, oo);
  }
}

// filter gradient, launch 1: partial[range][C][9]
template <int STRIDE>
__global__ void __launch_bounds__(256) dw_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                       float* __restrict__ partial, int H, int W, int C, int Ho, int Wo,
                                                       int SPR, int64_t strips, int RS, int QB, int lddy, int ldx) {
  constexpr int NCOL = (DW_S - 1) * STRIDE + 3;
  __shared__ __attribute__((aligned(16))) float red[256 * 36];
  const int G = C >> 2, tid = threadIdx.x;
  const int SL = 256 / QB;
  const int ql = tid % QB, lane = tid / QB;
  const int q = blockIdx.y * QB + ql, c = q * 4;
  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = dw_zero();
  if (q < G) {
    const int64_t lo = (int64_t)blockIdx.x * RS;
    const int64_t hi = lo + RS < strips ? lo + RS : strips;
    for (int64_t s = lo + lane; s < hi; s += SL) {
      const int xs = (int)(s % SPR);
      const int64_t by = s / SPR;
      const int yo = (int)(by % Ho), b = (int)(by / Ho), xo0 = xs * DW_S;
      const float* g = dy + (((int64_t)b * Ho + yo) * Wo + xo0) * lddy + c;
      f32x4 dv[DW_S];
#pragma unroll
      for (int jx = 0; jx < DW_S; ++jx) dv[jx] = xo0 + jx < Wo ? dw_ld4(g + (int64_t)jx * lddy) : dw_zero();
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int yi = yo * STRIDE + r - 1;
        if (yi < 0 || yi >= H) continue;
        const float* row = x + ((int64_t)b * H + yi) * W * ldx + c;
        f32x4 win[NCOL];
#pragma unroll
        for (int k = 0; k < NCOL; ++k) {
          const int xi = xo0 * STRIDE + k - 1;
          win[k] = (xi >= 0 && xi < W) ? dw_ld4(row + (int64_t)xi * ldx) : dw_zero();
        }
#pragma unroll
        for (int jx = 0; jx < DW_S; ++jx)
#pragma unroll
          for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[r * 3 + t][k] = fmaf(dv[jx][k], win[jx * STRIDE + t][k], acc[r * 3 + t][k]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) dw_st4(&red[tid * 36 + t * 4], acc[t]);      // [lane][ql][tap][k]
  __syncthreads();
  for (int e = tid; e < QB * 36; e += 256) {
    const int eq = e / 36, tk = e - eq * 36;
    float s = 0.f;
    for (int l = 0; l < SL; ++l) s += red[(l * QB + eq) * 36 + tk];
    const int qq = blockIdx.y * QB + eq;
    if (qq < G) partial[(int64_t)blockIdx.x * C * 9 + (int64_t)(qq * 4 + (tk & 3)) * 9 + (tk >> 2)] = s;
  }
}

// launch 2: dw[e] (=|+=) the ranges' partials in ascending order, float64, one rounding
__global__ void __launch_bounds__(256) dw_wgrad_finish_kernel(const float* __restrict__ partial, float* __restrict__ dw, int n,
                                                              int ranges, int accumulate) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
#pragma unroll 8
  for (int r = 0; r < ranges; ++r) s += (double)partial[(int64_t)r * n + e];      // (the loads are independent, the adds in order)
  const float v = (float)s;
  dw[e] = accumulate ? dw[e] + v : v;
}

// ---- host launchers (extern "C" wrappers in ssp_api.hip) ------------------------------------------------------
static bool dw_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

static int dw_check(const char* name, int B, int H, int W, int C, int lda, int ldb, int stride) {
  SSP_CHECK_ARG(C > 0 && C % 4 == 0, "%s: C = %d must be a positive multiple of 4", name, C);
  SSP_CHECK_ARG(lda % 4 == 0 && ldb % 4 == 0 && lda >= C && ldb >= C,
                "%s: leading dimensions %d, %d must be multiples of 4 and >= C = %d", name, lda, ldb, C);
  SSP_CHECK_ARG(stride == 1 || stride == 2, "%s: stride %d (1 or 2)", name, stride);
  SSP_CHECK_ARG(B > 0 && H > 0 && W > 0 && (int64_t)B * H * W < (1ll << 31), "%s: bad sizes (B * H * W must be below 2^31)", name);
  return SSP_OK;
}

int ssp_dwconv_stats_tile_m_q(int B, int H, int W, int C, int stride) { return 0; }
int ssp_dwconv_stats_tiles_q(int B, int H, int W, int C, int stride) {
  if (dw_check("dwconv_stats_tiles", B, H, W, C, C, C, stride) != SSP_OK) return 0;
  return dw_geom(B, H, W, C, stride).tiles;
}
int64_t ssp_dwconv_stats_floats_q(int B, int H, int W, int C, int stride) {
  if (dw_check("dwconv_stats_floats", B, H, W, C, C, C, stride) != SSP_OK) return 0;
  return (int64_t)dw_geom(B, H, W, C, stride).tiles * (C * 2 + 1);
}
int64_t ssp_dwconv_wgrad_workspace_floats_q(int B, int H, int W, int C, int stride) {
  if (dw_check("dwconv_wgrad_workspace_floats", B, H, W, C, C, C, stride) != SSP_OK) return 0;
  return (int64_t)dw_geom(B, H, W, C, stride).ranges * C * 9;
}

template <int STRIDE, bool FLIP>
static void dw_fwd_run(const DwGeom& g, const float* in, const float* w, float* out, const float* scale, const float* shift,
                       float slope, int accumulate, float* stats, int H, int W, int C, int ldin, int ldout, hipStream_t stream) {
  if (stats != nullptr)
    hipLaunchKernelGGL((dw_fwd_kernel<STRIDE, FLIP, true>), dim3(g.tiles), dim3(256), 0, stream, in, w, out, scale, shift, slope,
                       accumulate, stats, g.tiles, H, W, C, g.Ho, g.Wo, g.SPR, g.strips, g.NS, ldin, ldout);
  else
    hipLaunchKernelGGL((dw_fwd_kernel<STRIDE, FLIP, false>), dim3(g.tiles), dim3(256), 0, stream, in, w, out, scale, shift, slope,
                       accumulate, stats, g.tiles, H, W, C, g.Ho, g.Wo, g.SPR, g.strips, g.NS, ldin, ldout);
}

// forward: bias form (scale == nullptr, shift = bias, slope = 1) and affine form
int ssp_dwconv_fwd_launch(const char* name, const float* in, const float* w, float* out, const float* scale, const float* shift,
                          float slope, float* stats, int B, int H, int W, int C, int ldin, int ldout, int stride,
                          hipStream_t stream) {
  const int rc = dw_check(name, B, H, W, C, ldin, ldout, stride);
  if (rc != SSP_OK) return rc;
  SSP_CHECK_ARG(in != nullptr && w != nullptr && out != nullptr && dw_al16(in) && dw_al16(w) && dw_al16(out) && dw_al16(scale) &&
                    dw_al16(shift) && dw_al16(stats), "%s: null or unaligned operands", name);
  const DwGeom g = dw_geom(B, H, W, C, stride);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 4.0 * C * ((double)B * H * W + (double)B * g.Ho * g.Wo));
  if (stride == 1) dw_fwd_run<1, false>(g, in, w, out, scale, shift, slope, 0, stats, H, W, C, ldin, ldout, stream);
  else dw_fwd_run<2, false>(g, in, w, out, scale, shift, slope, 0, stats, H, W, C, ldin, ldout, stream);
  SSP_CHECK_LAUNCH(name);
  return SSP_OK;
}

int ssp_dwconv_dgrad_launch(const float* dy, const float* w, float* dx, int B, int H, int W, int C, int lddy, int lddx,
                            int stride, int accumulate, hipStream_t stream) {
  const int rc = dw_check("dwconv_dgrad", B, H, W, C, lddy, lddx, stride);
  if (rc != SSP_OK) return rc;
  SSP_CHECK_ARG(dy != nullptr && w != nullptr && dx != nullptr && dw_al16(dy) && dw_al16(w) && dw_al16(dx),
                "dwconv_dgrad: null or unaligned operands");
  const DwGeom g = dw_geom(B, H, W, C, stride);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 4.0 * C * ((double)B * H * W * (accumulate ? 2 : 1) + (double)B * g.Ho * g.Wo));
  if (stride == 1) {
    dw_fwd_run<1, true>(g, dy, w, dx, nullptr, nullptr, 1.f, accumulate ? 1 : 0, nullptr, H, W, C, lddy, lddx, stream);
  } else {
    const int64_t total = (int64_t)B * g.Ho * g.Wo * g.G;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(dw_dgrad_s2_kernel, dim3((int)blocks), dim3(256), 0, stream, dy, w, dx, B, H, W, C, g.Ho, g.Wo, lddy, lddx,
                       accumulate ? 1 : 0);
  }
  SSP_CHECK_LAUNCH("dwconv_dgrad");
  return SSP_OK;
}

int ssp_dwconv_wgrad_launch(const float* dy, const float* x, float* dw, int B, int H, int W, int C, int lddy, int ldx, int stride,
                            int accumulate, float* workspace, int64_t workspace_floats, hipStream_t stream) {
  const int rc = dw_check("dwconv_wgrad", B, H, W, C, lddy, ldx, stride);
  if (rc != SSP_OK) return rc;
  SSP_CHECK_ARG(dy != nullptr && x != nullptr && dw != nullptr && workspace != nullptr && dw_al16(dy) && dw_al16(x) && dw_al16(dw) &&
                    dw_al16(workspace), "dwconv_wgrad: null or unaligned operands");
  const DwGeom g = dw_geom(B, H, W, C, stride);
  SSP_CHECK_ARG(workspace_floats >= (int64_t)g.ranges * C * 9, "dwconv_wgrad: workspace of %lld floats, %lld needed",
                (long long)workspace_floats, (long long)g.ranges * C * 9);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 4.0 * C * ((double)B * H * W + (double)B * g.Ho * g.Wo));
  if (stride == 1)
    hipLaunchKernelGGL(dw_wgrad_kernel<1>, dim3(g.ranges, g.QG), dim3(256), 0, stream, dy, x, workspace, H, W, C, g.Ho, g.Wo, g.SPR,
                       g.strips, g.RS, g.QB, lddy, ldx);
  else
    hipLaunchKernelGGL(dw_wgrad_kernel<2>, dim3(g.ranges, g.QG), dim3(256), 0, stream, dy, x, workspace, H, W, C, g.Ho, g.Wo, g.SPR,
                       g.strips, g.RS, g.QB, lddy, ldx);
  SSP_CHECK_LAUNCH("dwconv_wgrad");
  hipLaunchKernelGGL(dw_wgrad_finish_kernel, dim3((C * 9 + 255) / 256), dim3(256), 0, stream, workspace, dw, C * 9, g.ranges,
                     accumulate ? 1 : 0);
  SSP_CHECK_LAUNCH("dwconv_wgrad_finish");
  return SSP_OK;
}

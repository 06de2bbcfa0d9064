// Darknet blocks outside the pose cfgs' hot path: stride-1 max-pool, shortcut, global average pool, softmax over
// channels.  All of them are HBM-bound passes over fp32 NHWC maps ([pixels][ld], ld % 4 == 0), loaded as float4 along
// channels with grid-stride loops; backward passes write or accumulate (accumulate = 1) into the input's gradient, so a
// map with several consumers gets the sum of their gradients (same convention as ssp_maxpool_bwd / ssp_copy_channels).
//
// Reference semantics:
//   MaxPoolStride1   /root/reference/darknet.py:8-14     max_pool2d(pad(x, (0,1,0,1), 'replicate'), 2, stride=1)
//   GlobalAvgPool2d  /root/reference/darknet.py:37-47    avg_pool2d(x, (H, W)).view(N, C)
//   softmax          /root/reference/darknet.py:181-184  nn.Softmax() (implicit dim = 1 for 2-D and 4-D input)
//   shortcut         /root/reference/darknet.py:107-118  act(x[from] + x[ind-1]), act in {linear, leaky 0.1, relu}
#include "ssp_common.h"

static int gb_grid(int64_t total, int threads) {
  int64_t blocks = (total + threads - 1) / threads;
  const int64_t cap = 256 * 16;
  return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// ---- stride-1 max-pool ----------------------------------------------------------------------------------------
// out[y][x] = max of the 2x2 window at (y, x) of the right / bottom replicate-padded map: rows y, min(y+1, H-1),
// columns x, min(x+1, W-1).  Output is H x W.
// A work item is one channel quad of one image COLUMN (b, x, quad), walked top to bottom: the window's lower row is the
// next step's upper row, so each step loads 2 pixels instead of 4, and the index arithmetic is paid once per column.
// (One item per output pixel re-read every input pixel 4 times - the x+1 neighbour sits in another workgroup, usually on
// another XCD, so those re-reads missed L2: 37 % of the HBM peak at B = 64, 13 x 13 x 1024.)
__global__ void __launch_bounds__(256) maxpool_s1_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out,
                                                             int ldo, int C, int B, int H, int W) {
  const int G = C >> 2;
  const int64_t total = (int64_t)B * W * G;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % G) * 4;
    const int64_t t = idx / G;
    const int xx = (int)(t % W);
    const int64_t img = (t / W) * H * W;                 // pixel (b, 0, 0)
    const int x1 = xx + 1 < W ? xx + 1 : xx;
    const float* col0 = x + (img + xx) * ldx + c;
    const float* col1 = x + (img + x1) * ldx + c;
    const int64_t row = (int64_t)W * ldx;
    float* o = out + (img + xx) * ldo + c;
    f32x4 v0 = ld4(col0), v1 = ld4(col1);
    for (int y = 0; y < H; ++y) {
      const int64_t yp = (y + 1 < H ? y + 1 : y) * row;
      const f32x4 v2 = ld4(col0 + yp), v3 = ld4(col1 + yp);
      f32x4 r;
#pragma unroll
      for (int k = 0; k < 4; ++k) {     // window scan order, first maximum kept (ATen's `val > maxval`)
        float m = v0[k];
        if (v1[k] > m) m = v1[k];
        if (v2[k] > m) m = v2[k];
        if (v3[k] > m) m = v3[k];
        r[k] = m;
      }
      st4(o + (int64_t)y * W * ldo, r);
      v0 = v2;
      v1 = v3;
    }
  }
}

// Gather form (the windows overlap, a scatter would race): input pixel (y, x) belongs to the windows of outputs
// (y-1, x-1), (y-1, x), (y, x-1), (y, x).  Each window's winner is recomputed from the 3 x 3 neighbourhood (first maximum
// in row-then-column order, as ATen) and mapped back through the replicate clamp: a winner on the pad folds onto the
// edge pixel it copies.  Gradients are summed in output scan order - the order ATen's max_pool2d backward adds them.
// Same column walk as the forward: the neighbourhood and the two gradient rows slide down with y, so a step loads one
// new row of 3 pixels and 2 gradients (not 9 + 4).
__global__ void __launch_bounds__(256) maxpool_s1_bwd_kernel(const float* __restrict__ x, int ldx,
                                                             const float* __restrict__ gr, int ldg, float* __restrict__ dx,
                                                             int lddx, int C, int B, int H, int W, int accumulate) {
  const int G = C >> 2;
  const int64_t total = (int64_t)B * W * G;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % G) * 4;
    const int64_t t = idx / G;
    const int xx = (int)(t % W);
    const int64_t img = (t / W) * H * W;                 // pixel (b, 0, 0)
    // neighbourhood columns x-1, x, x+1 (clamped into the map; column -1 is never used at the left edge)
    const int xc[3] = {xx > 0 ? xx - 1 : 0, xx, xx + 1 < W ? xx + 1 : xx};
    auto X = [&](int y, int q) { return ld4(x + (img + (int64_t)y * W + xc[q]) * ldx + c); };
    auto Gr = [&](int y, int q) { return ld4(gr + (img + (int64_t)y * W + xc[q]) * ldg + c); };
    // rows y-1 (rm, gm) and y (r0) of the sliding window; row -1 is never used at the top edge
    f32x4 r0[3] = {X(0, 0), X(0, 1), X(0, 2)};
    f32x4 rm[3] = {r0[0], r0[1], r0[2]};
    f32x4 gm[2] = {zero, zero};
    for (int y = 0; y < H; ++y) {
      const int yp = y + 1 < H ? y + 1 : y;
      const f32x4 rp[3] = {X(yp, 0), X(yp, 1), X(yp, 2)};
      const f32x4 g0[2] = {xx > 0 ? Gr(y, 0) : zero, Gr(y, 1)};
      const f32x4* nb[3] = {rm, r0, rp};
      f32x4 acc = zero;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int oy = y - 1 + (o >> 1), ox = xx - 1 + (o & 1);
        if (oy < 0 || ox < 0) continue;
        const f32x4 gv = (o >> 1) ? g0[o & 1] : gm[o & 1];
        // window position q (scan order) reads neighbourhood entry [dy + (q >> 1)][dx + (q & 1)] (loaded through the
        // clamp, so a pad position holds its edge pixel's value); it is THIS pixel when the clamped coordinates say so
        unsigned hit = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int sr = oy + (q >> 1), sc = ox + (q & 1);
          sr = sr > H - 1 ? H - 1 : sr;
          sc = sc > W - 1 ? W - 1 : sc;
          hit |= (sr == y && sc == xx) ? (1u << q) : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float m = nb[o >> 1][o & 1][k];
          int s = 0;
#pragma unroll
          for (int q = 1; q < 4; ++q) {
            const float v = nb[(o >> 1) + (q >> 1)][(o & 1) + (q & 1)][k];
            if (v > m) { m = v; s = q; }
          }
          if ((hit >> s) & 1u) acc[k] += gv[k];
        }
      }
      float* d = dx + (img + (int64_t)y * W + xx) * lddx + c;
      if (accumulate) {
        const f32x4 od = ld4(d);
        acc[0] += od[0]; acc[1] += od[1]; acc[2] += od[2]; acc[3] += od[3];
      }
      st4(d, acc);
#pragma unroll
      for (int q = 0; q < 3; ++q) { rm[q] = r0[q]; r0[q] = rp[q]; }
      gm[0] = g0[0];
      gm[1] = g0[1];
    }
  }
}

// ---- shortcut -------------------------------------------------------------------------------------------------
// slope: 1 = linear, 0.1 = leaky, 0 = relu
__device__ __forceinline__ float sc_act(float v, float slope) {
  return v > 0.f ? v : (slope == 0.f ? 0.f : v * slope);
}

__global__ void __launch_bounds__(256) shortcut_fwd_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b,
                                                           int ldb, float* __restrict__ out, int ldo, int C, int64_t M,
                                                           float slope) {
  const int G = C >> 2;
  const int64_t total = M * G;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % G) * 4;
    const int64_t m = idx / G;
    const f32x4 va = ld4(a + m * lda + c), vb = ld4(b + m * ldb + c);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = sc_act(va[k] + vb[k], slope);
    st4(out + m * ldo + c, r);
  }
}

// g' = g * act'(out), act' from out > 0 (in-place leaky_relu / relu backward); da (+)= g', db (+)= g'.  da == db (the
// `from = -1` shortcut, both summands are the same map): one pass adds 2 g'.
__global__ void __launch_bounds__(256) shortcut_bwd_kernel(const float* __restrict__ gr, int ldg, const float* __restrict__ out,
                                                           int ldo, float* da, int ldda, int acc_a, float* db, int lddb,
                                                           int acc_b, int C, int64_t M, float slope) {
  const int G = C >> 2;
  const int64_t total = M * G;
  const bool alias = da == db;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % G) * 4;
    const int64_t m = idx / G;
    f32x4 gv = ld4(gr + m * ldg + c);
    if (slope != 1.f) {
      const f32x4 ov = ld4(out + m * ldo + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) gv[k] = ov[k] > 0.f ? gv[k] : (slope == 0.f ? 0.f : gv[k] * slope);
    }
    if (alias) {
      f32x4 r = gv + gv;
      float* d = da + m * ldda + c;
      if (acc_a) r += ld4(d);
      st4(d, r);
    } else {
      float* pa = da + m * ldda + c;
      float* pb = db + m * lddb + c;
      f32x4 ra = gv, rb = gv;
      if (acc_a) ra += ld4(pa);
      if (acc_b) rb += ld4(pb);
      st4(pa, ra);
      st4(pb, rb);
    }
  }
}

// ---- global average pool --------------------------------------------------------------------------------------
// One workgroup item = (image, 16 channel quads): 16 pixel lanes x 16 quads.  Lane ty sums pixels ty, ty+16, ... in
// order, then lane 0 adds the 16 partial sums in order: a fixed summation order, the same result every run.
#define AVG_QUADS 16
#define AVG_LANES 16
__global__ void __launch_bounds__(256) avgpool_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out,
                                                          int ldo, int C, int B, int HW) {
  __shared__ f32x4 part[AVG_LANES][AVG_QUADS];
  const int G = C >> 2;
  const int nchunk = (G + AVG_QUADS - 1) / AVG_QUADS;
  const int tx = threadIdx.x % AVG_QUADS, ty = threadIdx.x / AVG_QUADS;
  const float n = (float)HW;
  for (int64_t item = blockIdx.x; item < (int64_t)B * nchunk; item += gridDim.x) {
    const int64_t b = item / nchunk;
    const int q = (int)(item % nchunk) * AVG_QUADS + tx;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (q < G) {
      const float* src = x + (b * HW) * ldx + q * 4;
      for (int p = ty; p < HW; p += AVG_LANES) s += ld4(src + (int64_t)p * ldx);
    }
    part[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && q < G) {
      f32x4 r = part[0][tx];
#pragma unroll
      for (int l = 1; l < AVG_LANES; ++l) r += part[l][tx];
      r[0] /= n; r[1] /= n; r[2] /= n; r[3] /= n;
      st4(out + b * ldo + q * 4, r);
    }
    __syncthreads();
  }
}

// dx[b][p][c] (+)= g[b][c] / (H * W)
__global__ void __launch_bounds__(256) avgpool_bwd_kernel(const float* __restrict__ gr, int ldg, float* __restrict__ dx,
                                                          int lddx, int C, int B, int HW, int accumulate) {
  const int G = C >> 2;
  const int64_t total = (int64_t)B * HW * G;
  const float n = (float)HW;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % G) * 4;
    const int64_t p = idx / G;
    const int64_t b = p / HW;
    f32x4 v = ld4(gr + b * ldg + c);
    v[0] /= n; v[1] /= n; v[2] /= n; v[3] /= n;
    float* d = dx + p * lddx + c;
    if (accumulate) v += ld4(d);
    st4(d, v);
  }
}

// ---- softmax over channels ------------------------------------------------------------------------------------
// One wave per row of C channels (a row = one 2-D sample or one NHWC pixel); lanes stride the row in float4 steps,
// channels >= C (the padding up to ld) are neither read into the sums nor written.  Butterfly reductions: deterministic.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) softmax_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y,
                                                          int ldy, int C, int64_t M) {
  const int lane = threadIdx.x & 63;
  const int G = (C + 3) >> 2;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t m = wave; m < M; m += nwave) {
    const float* xr = x + m * ldx;
    float mx = -INFINITY;
    for (int q = lane; q < G; q += 64) {
      const f32x4 v = ld4(xr + q * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q * 4 + k < C) mx = fmaxf(mx, v[k]);
    }
    mx = wave_max(mx);
    float s = 0.f;
    for (int q = lane; q < G; q += 64) {
      const f32x4 v = ld4(xr + q * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q * 4 + k < C) s += expf(v[k] - mx);
    }
    const float inv = 1.f / wave_sum(s);
    float* yr = y + m * ldy;
    for (int q = lane; q < G; q += 64) {
      const f32x4 v = ld4(xr + q * 4);
      if (q * 4 + 4 <= C) {
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = expf(v[k] - mx) * inv;
        st4(yr + q * 4, r);
      } else {
        for (int k = 0; q * 4 + k < C; ++k) yr[q * 4 + k] = expf(v[k] - mx) * inv;
      }
    }
  }
}

// dx (+)= y * (g - sum_c g * y)
__global__ void __launch_bounds__(256) softmax_bwd_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ gr,
                                                          int ldg, float* __restrict__ dx, int lddx, int C, int64_t M,
                                                          int accumulate) {
  const int lane = threadIdx.x & 63;
  const int G = (C + 3) >> 2;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t m = wave; m < M; m += nwave) {
    const float* yr = y + m * ldy;
    const float* gq = gr + m * ldg;
    float dot = 0.f;
    for (int q = lane; q < G; q += 64) {
      const f32x4 yv = ld4(yr + q * 4), gv = ld4(gq + q * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q * 4 + k < C) dot += gv[k] * yv[k];
    }
    dot = wave_sum(dot);
    float* d = dx + m * lddx;
    for (int q = lane; q < G; q += 64) {
      const f32x4 yv = ld4(yr + q * 4), gv = ld4(gq + q * 4);
      if (q * 4 + 4 <= C) {
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = yv[k] * (gv[k] - dot);
        if (accumulate) r += ld4(d + q * 4);
        st4(d + q * 4, r);
      } else {
        for (int k = 0; q * 4 + k < C; ++k) {
          const float r = yv[k] * (gv[k] - dot);
          d[q * 4 + k] = accumulate ? d[q * 4 + k] + r : r;
        }
      }
    }
  }
}

// ---- host launchers (extern "C" wrappers in ssp_api.hip) ------------------------------------------------------
static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

int ssp_maxpool_s1_fwd_launch(const float* x, int ldx, float* out, int ldo, int C, int B, int H, int W,
                              hipStream_t stream) {
  SSP_CHECK_ARG(C % 4 == 0 && C > 0 && ldx % 4 == 0 && ldo % 4 == 0 && ldx >= C && ldo >= C,
                "maxpool_s1_fwd: C and strides must be multiples of 4 (strides >= C)");
  SSP_CHECK_ARG(B > 0 && H > 0 && W > 0 && al16(x) && al16(out), "maxpool_s1_fwd: bad sizes or unaligned operands");
  const int64_t total = (int64_t)B * H * W * (C / 4);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 32.0 * total);
  hipLaunchKernelGGL(maxpool_s1_fwd_kernel, dim3(gb_grid(total / H, 256)), dim3(256), 0, stream, x, ldx, out, ldo, C, B, H, W);
  SSP_CHECK_LAUNCH("maxpool_s1_fwd");
  return SSP_OK;
}

int ssp_maxpool_s1_bwd_launch(const float* x, int ldx, const float* g, int ldg, float* dx, int lddx, int C, int B, int H,
                              int W, int accumulate, hipStream_t stream) {
  SSP_CHECK_ARG(C % 4 == 0 && C > 0 && ldx % 4 == 0 && ldg % 4 == 0 && lddx % 4 == 0 && ldx >= C && ldg >= C && lddx >= C,
                "maxpool_s1_bwd: C and strides must be multiples of 4 (strides >= C)");
  SSP_CHECK_ARG(B > 0 && H > 0 && W > 0 && al16(x) && al16(g) && al16(dx), "maxpool_s1_bwd: bad sizes or unaligned operands");
  const int64_t total = (int64_t)B * H * W * (C / 4);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, (accumulate ? 64.0 : 48.0) * total);
  hipLaunchKernelGGL(maxpool_s1_bwd_kernel, dim3(gb_grid(total / H, 256)), dim3(256), 0, stream, x, ldx, g, ldg, dx, lddx, C, B,
                     H, W, accumulate);
  SSP_CHECK_LAUNCH("maxpool_s1_bwd");
  return SSP_OK;
}

int ssp_shortcut_fwd_launch(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int C, int64_t M,
                            float slope, hipStream_t stream) {
  SSP_CHECK_ARG(C % 4 == 0 && C > 0 && lda % 4 == 0 && ldb % 4 == 0 && ldo % 4 == 0 && lda >= C && ldb >= C && ldo >= C,
                "shortcut_fwd: C and strides must be multiples of 4 (strides >= C)");
  SSP_CHECK_ARG(M > 0 && al16(a) && al16(b) && al16(out), "shortcut_fwd: bad sizes or unaligned operands");
  const int64_t total = M * (C / 4);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 48.0 * total);
  hipLaunchKernelGGL(shortcut_fwd_kernel, dim3(gb_grid(total, 256)), dim3(256), 0, stream, a, lda, b, ldb, out, ldo, C, M,
                     slope);
  SSP_CHECK_LAUNCH("shortcut_fwd");
  return SSP_OK;
}

int ssp_shortcut_bwd_launch(const float* g, int ldg, const float* out, int ldo, float* da, int ldda, int acc_a, float* db,
                            int lddb, int acc_b, int C, int64_t M, float slope, hipStream_t stream) {
  SSP_CHECK_ARG(C % 4 == 0 && C > 0 && ldg % 4 == 0 && ldo % 4 == 0 && ldda % 4 == 0 && lddb % 4 == 0 && ldg >= C &&
                ldo >= C && ldda >= C && lddb >= C, "shortcut_bwd: C and strides must be multiples of 4 (strides >= C)");
  SSP_CHECK_ARG(M > 0 && al16(g) && al16(out) && al16(da) && al16(db), "shortcut_bwd: bad sizes or unaligned operands");
  SSP_CHECK_ARG(da != db || (ldda == lddb && acc_a == acc_b), "shortcut_bwd: aliased gradients need equal strides and flags");
  const int64_t total = M * (C / 4);
  const double bytes = 16.0 * total * ((slope != 1.f ? 2 : 1) + (da == db ? 1 + acc_a : 2 + acc_a + acc_b));
  SspProfScope prof(SSP_PROF_LAYOUT, stream, bytes);
  hipLaunchKernelGGL(shortcut_bwd_kernel, dim3(gb_grid(total, 256)), dim3(256), 0, stream, g, ldg, out, ldo, da, ldda,
                     acc_a, db, lddb, acc_b, C, M, slope);
  SSP_CHECK_LAUNCH("shortcut_bwd");
  return SSP_OK;
}

int ssp_avgpool_fwd_launch(const float* x, int ldx, float* out, int ldo, int C, int B, int H, int W, hipStream_t stream) {
  SSP_CHECK_ARG(C % 4 == 0 && C > 0 && ldx % 4 == 0 && ldo % 4 == 0 && ldx >= C && ldo >= C,
                "avgpool_fwd: C and strides must be multiples of 4 (strides >= C)");
  SSP_CHECK_ARG(B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && al16(x) && al16(out),
                "avgpool_fwd: bad sizes or unaligned operands");
  const int64_t items = (int64_t)B * ((C / 4 + AVG_QUADS - 1) / AVG_QUADS);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 4.0 * B * C * ((double)H * W + 1));
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(gb_grid(items, 1)), dim3(AVG_QUADS * AVG_LANES), 0, stream, x, ldx, out, ldo,
                     C, B, H * W);
  SSP_CHECK_LAUNCH("avgpool_fwd");
  return SSP_OK;
}

int ssp_avgpool_bwd_launch(const float* g, int ldg, float* dx, int lddx, int C, int B, int H, int W, int accumulate,
                           hipStream_t stream) {
  SSP_CHECK_ARG(C % 4 == 0 && C > 0 && ldg % 4 == 0 && lddx % 4 == 0 && ldg >= C && lddx >= C,
                "avgpool_bwd: C and strides must be multiples of 4 (strides >= C)");
  SSP_CHECK_ARG(B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && al16(g) && al16(dx),
                "avgpool_bwd: bad sizes or unaligned operands");
  const int64_t total = (int64_t)B * H * W * (C / 4);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 16.0 * total * (1 + accumulate));
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(gb_grid(total, 256)), dim3(256), 0, stream, g, ldg, dx, lddx, C, B, H * W,
                     accumulate);
  SSP_CHECK_LAUNCH("avgpool_bwd");
  return SSP_OK;
}

int ssp_softmax_fwd_launch(const float* x, int ldx, float* y, int ldy, int C, int64_t M, hipStream_t stream) {
  SSP_CHECK_ARG(C > 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C,
                "softmax_fwd: strides must be multiples of 4 and >= C");
  SSP_CHECK_ARG(M > 0 && al16(x) && al16(y), "softmax_fwd: bad sizes or unaligned operands");
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 8.0 * M * C);
  hipLaunchKernelGGL(softmax_fwd_kernel, dim3(gb_grid(M, 4)), dim3(256), 0, stream, x, ldx, y, ldy, C, M);
  SSP_CHECK_LAUNCH("softmax_fwd");
  return SSP_OK;
}

int ssp_softmax_bwd_launch(const float* y, int ldy, const float* g, int ldg, float* dx, int lddx, int C, int64_t M,
                           int accumulate, hipStream_t stream) {
  SSP_CHECK_ARG(C > 0 && ldy % 4 == 0 && ldg % 4 == 0 && lddx % 4 == 0 && ldy >= C && ldg >= C && lddx >= C,
                "softmax_bwd: strides must be multiples of 4 and >= C");
  SSP_CHECK_ARG(M > 0 && al16(y) && al16(g) && al16(dx), "softmax_bwd: bad sizes or unaligned operands");
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 4.0 * M * C * (3 + accumulate));
  hipLaunchKernelGGL(softmax_bwd_kernel, dim3(gb_grid(M, 4)), dim3(256), 0, stream, y, ldy, g, ldg, dx, lddx, C, M,
                     accumulate);
  SSP_CHECK_LAUNCH("softmax_bwd");
  return SSP_OK;
}

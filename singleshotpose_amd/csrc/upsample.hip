// Darknet [upsample] block: nearest-neighbour replication by an integer stride N on fp32 NHWC maps ([pixels][ld],
// ld % 4 == 0), the top-down step of a YOLOv3-style feature path.
//
//   forward   dst[b, y, x, c] = src[b, y / N, x / N, c]                      (F.interpolate(scale_factor=N, mode='nearest'))
//   backward  dsrc[b, y, x, c] (=|+=) sum_{i, j < N} g[b, N y + i, N x + j, c]
//
// H x W is the SOURCE (coarse) map in both entry points.  Both are HBM-bound passes: a work item is one channel quad of
// one coarse pixel, quads fastest, so the 64 lanes of a wave read (forward) or write (backward) consecutive 16-byte
// pieces of a coarse row, and every fine-side access of a lane group covering one pixel is a contiguous run of 4 C bytes.
// Only columns [0, C) of a row are touched on either side, so a map may be a channel slice of a wider buffer (ld > C, the
// pointer offset by a multiple of 4 floats): that is how the plan writes an upsample straight into the concatenation
// buffer of the route behind it, and reads its gradient out of the route's gradient buffer in place.
//
// Backward sum order (fixed, part of the contract - the tests pin it bit for bit): the N x N window is taken row-major
// with sequential fp32 adds, s = g[0][0]; s += g[0][1]; ... s += g[N-1][N-1]; then dsrc = accumulate ? dsrc + s : s.
// One thread owns one output element: no atomics, the same bits every run (the reproducible training mode needs no
// second form of this kernel).
#include "ssp_common.h"

static int up_grid(int64_t items, int64_t sized_by) {
  // sized by the destination's quad count, capped (grid-stride loop), and never more workgroups than there are items
  int64_t blocks = (sized_by + 255) / 256;
  const int64_t need = (items + 255) / 256;
  const int64_t cap = 256 * 16;
  if (blocks > cap) blocks = cap;
  if (blocks > need) blocks = need;
  return (int)(blocks < 1 ? 1 : blocks);
}

__device__ __forceinline__ f32x4 up_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void up_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// one source read serves the N x N destination pixels
__global__ void __launch_bounds__(256) upsample_fwd_kernel(const float* __restrict__ src, int lds_, float* __restrict__ dst,
                                                           int ldd, int C, int B, int H, int W, int N) {
  const int G = C >> 2;
  const int64_t total = (int64_t)B * H * W * G;
  const int64_t Wd = (int64_t)W * N;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % G) * 4;
    const int64_t p = idx / G;                   // coarse pixel (b, y, x)
    const int x = (int)(p % W);
    const int64_t by = p / W;                    // b * H + y
    const f32x4 v = up_ld4(src + p * lds_ + c);
    float* d = dst + ((by * N) * Wd + (int64_t)x * N) * ldd + c;      // fine pixel (b, N y, N x)
    for (int i = 0; i < N; ++i) {
      for (int j = 0; j < N; ++j) up_st4(d + (int64_t)j * ldd, v);
      d += Wd * ldd;
    }
  }
}

__global__ void __launch_bounds__(256) upsample_bwd_kernel(const float* __restrict__ g, int ldg, float* __restrict__ dsrc,
                                                           int ldds, int C, int B, int H, int W, int N, int accumulate) {
  const int G = C >> 2;
  const int64_t total = (int64_t)B * H * W * G;
  const int64_t Wd = (int64_t)W * N;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % G) * 4;
    const int64_t p = idx / G;
    const int x = (int)(p % W);
    const int64_t by = p / W;
    const float* q = g + ((by * N) * Wd + (int64_t)x * N) * ldg + c;
    f32x4 s = up_ld4(q);                         // window row-major, sequential adds: the documented order
    for (int i = 0; i < N; ++i) {
      for (int j = (i == 0 ? 1 : 0); j < N; ++j) {
        const f32x4 t = up_ld4(q + (int64_t)j * ldg);
        s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[3] += t[3];
      }
      q += Wd * ldg;
    }
    float* d = dsrc + p * ldds + c;
    if (accumulate) {
      const f32x4 o = up_ld4(d);
      s[0] = o[0] + s[0]; s[1] = o[1] + s[1]; s[2] = o[2] + s[2]; s[3] = o[3] + s[3];
    }
    up_st4(d, s);
  }
}

// ---- host launchers (extern "C" wrappers in ssp_api.hip) ------------------------------------------------------
static bool up_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

static int up_check(const char* name, const void* coarse, int ldc, const void* fine, int ldf, int C, int B, int H, int W,
                    int stride) {
  SSP_CHECK_ARG(C % 4 == 0 && C > 0 && ldc % 4 == 0 && ldf % 4 == 0 && ldc >= C && ldf >= C,
                "%s: C and strides must be multiples of 4 (strides >= C)", name);
  SSP_CHECK_ARG(stride >= 1 && stride <= 8, "%s: stride %d is outside 1..8", name, stride);
  SSP_CHECK_ARG(B > 0 && H > 0 && W > 0 && (int64_t)B * H * W * stride * stride < (1ll << 31),
                "%s: bad sizes (B * H * W * stride^2 must be below 2^31)", name);
  SSP_CHECK_ARG(coarse != nullptr && fine != nullptr && up_al16(coarse) && up_al16(fine), "%s: null or unaligned operands", name);
  return SSP_OK;
}

int ssp_upsample_fwd_launch(const float* src, int lds_, float* dst, int ldd, int C, int B, int H, int W, int stride,
                            hipStream_t stream) {
  const int rc = up_check("upsample_fwd", src, lds_, dst, ldd, C, B, H, W, stride);
  if (rc != SSP_OK) return rc;
  const int64_t total = (int64_t)B * H * W * (C / 4);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 16.0 * total * (1 + stride * stride));
  hipLaunchKernelGGL(upsample_fwd_kernel, dim3(up_grid(total, total * stride * stride)), dim3(256), 0, stream, src, lds_, dst,
                     ldd, C, B, H, W, stride);
  SSP_CHECK_LAUNCH("upsample_fwd");
  return SSP_OK;
}

int ssp_upsample_bwd_launch(const float* g, int ldg, float* dsrc, int ldds, int C, int B, int H, int W, int stride,
                            int accumulate, hipStream_t stream) {
  const int rc = up_check("upsample_bwd", dsrc, ldds, g, ldg, C, B, H, W, stride);
  if (rc != SSP_OK) return rc;
  const int64_t total = (int64_t)B * H * W * (C / 4);
  SspProfScope prof(SSP_PROF_LAYOUT, stream, 16.0 * total * (1 + (accumulate ? 1 : 0) + stride * stride));
  hipLaunchKernelGGL(upsample_bwd_kernel, dim3(up_grid(total, total)), dim3(256), 0, stream, g, ldg, dsrc, ldds, C, B, H, W,
                     stride, accumulate);
  SSP_CHECK_LAUNCH("upsample_bwd");
  return SSP_OK;
}

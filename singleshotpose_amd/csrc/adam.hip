// Adam / AdamW (with optional AMSGrad) over flat fp32 buffers, and global-norm gradient clipping: the optimizer family
// next to sgd.hip.  The contract is the comment in include/ssp_hip.h (ssp_adam_step, ssp_adam_step_table,
// ssp_grad_sumsq_table, ssp_grad_scale_table); singleshotpose_amd/optim.py (Adam, AdamW, clip_grad_norm_) is the caller.
//
// Per element, in the order of torch.optim.Adam's single-tensor path (torch/optim/adam.py):
//   AdamW: p *= 1 - lr*wd                 Adam: g = fma(wd, p, g)                    (only when wd != 0)
//   m = m + (1-beta1) * (g - m)
//   v = beta2*v + ((1-beta2)*g)*g
//   amsgrad: vmax = max(vmax, v), the denominator uses vmax
//   denom = sqrt(v) / bc2_sqrt + eps
//   p = p + (-step_size * m) / denom          (addcdiv_ rounds the product, the quotient and the sum)
// The fused multiply-adds sit where torch's CPU kernels fuse (add(alpha), lerp_, addcmul_ onto beta2*v) and nowhere else,
// so on an FMA-capable host the kernel and torch.optim.Adam round in the same places.
// step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) come from the host, which owns the step count t.
// Every hyper-parameter arrives as a double and is rounded to fp32 ONCE, after the host-side double arithmetic
// (1 - beta2 formed in fp32 from fp32(0.999) would be off by 1.3e-5 relative; torch rounds the double too).
//
// This file is compiled with -ffp-contract=off (Makefile): every product and sum below is rounded where it is written,
// the fused multiply-adds are the explicit __fmaf_rn calls.  Square root and division are the IEEE correctly rounded
// ones: sqrtf and `/`, which hipcc compiles correctly rounded by default (-fhip-fp32-correctly-rounded-divide-sqrt);
// this toolchain's __fsqrt_rn is the NATIVE (1 ulp) square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined, so it is
// not used.
//
// HBM-bound: read p, g, m, v and write p, m, v = 28 B per parameter (36 B with amsgrad): 1.41 GB per step for
// yolo-pose.cfg's 50.5 M parameters.
#include <cmath>

#include "ssp_common.h"

#define ADAM_DECOUPLED 1      // p *= decay            (AdamW with weight_decay != 0)
#define ADAM_L2 2             // g = fma(wd, p, g)     (Adam with weight_decay != 0)
#define ADAM_AMSGRAD 4

// one update's hyper-parameters, already rounded to fp32: a whole launch's (adam_kernel) or one tuple of a segment
// table's (adam_table_kernel)
struct AdamHyper {
  float decay;      // 1 - lr*wd
  float wd;
  float w1;         // 1 - beta1
  float b2;         // beta2
  float w2;         // 1 - beta2
  float bc2;        // sqrt(1 - beta2^t)
  float eps;
  float nstep;      // -lr / (1 - beta1^t)
  int flags;
};

// THE arithmetic: the single-range kernel, the table kernel and both scalar tails go through this one function, so every
// path gives the same bits for the same element
__device__ __forceinline__ float adam_one(float p, float g, float& m, float& v, float& vmax, const AdamHyper& h) {
  if (h.flags & ADAM_DECOUPLED) p = __fmul_rn(p, h.decay);
  if (h.flags & ADAM_L2) g = __fmaf_rn(h.wd, p, g);
  m = __fmaf_rn(h.w1, __fsub_rn(g, m), m);
  v = __fmaf_rn(__fmul_rn(h.w2, g), g, __fmul_rn(h.b2, v));
  float d = v;
  if (h.flags & ADAM_AMSGRAD) {
    vmax = (v > vmax || v != v) ? v : vmax;      // torch.maximum: a NaN propagates
    d = vmax;
  }
  const float denom = __fadd_rn(sqrtf(d) / h.bc2, h.eps);
  return __fadd_rn(p, __fmul_rn(h.nstep, m) / denom);      // addcdiv_: (value * m) / denom, each rounded
}

// four consecutive elements at float offset 4 * i of 16-byte aligned buffers; all loads are issued before the first use
__device__ __forceinline__ void adam_quad(float* p, const float* g, float* m, float* v, float* vmax, int64_t i,
                                          const AdamHyper& h) {
  const bool ams = (h.flags & ADAM_AMSGRAD) != 0;
  float4 pv = reinterpret_cast<const float4*>(p)[i];
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 mv = reinterpret_cast<const float4*>(m)[i];
  float4 vv = reinterpret_cast<const float4*>(v)[i];
  float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ams) xv = reinterpret_cast<const float4*>(vmax)[i];
  pv.x = adam_one(pv.x, gv.x, mv.x, vv.x, xv.x, h);
  pv.y = adam_one(pv.y, gv.y, mv.y, vv.y, xv.y, h);
  pv.z = adam_one(pv.z, gv.z, mv.z, vv.z, xv.z, h);
  pv.w = adam_one(pv.w, gv.w, mv.w, vv.w, xv.w, h);
  reinterpret_cast<float4*>(p)[i] = pv;
  reinterpret_cast<float4*>(m)[i] = mv;
  reinterpret_cast<float4*>(v)[i] = vv;
  if (ams) reinterpret_cast<float4*>(vmax)[i] = xv;
}

__device__ __forceinline__ void adam_scalar(float* p, const float* g, float* m, float* v, float* vmax, int64_t i,
                                            const AdamHyper& h) {
  const bool ams = (h.flags & ADAM_AMSGRAD) != 0;
  float mv = m[i], vv = v[i];
  float xv = ams ? vmax[i] : 0.f;
  p[i] = adam_one(p[i], g[i], mv, vv, xv, h);
  m[i] = mv;
  v[i] = vv;
  if (ams) vmax[i] = xv;
}

struct AdamArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* vmax;
  int64_t n;
  AdamHyper h;
};

__global__ void __launch_bounds__(256) adam_kernel(AdamArgs a) {
  const int64_t n4 = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) adam_quad(a.p, a.g, a.m, a.v, a.vmax, i, a.h);
  // tail (n not a multiple of 4): the first workgroup finishes it
  if (blockIdx.x == 0) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    if (i < a.n) adam_scalar(a.p, a.g, a.m, a.v, a.vmax, i, a.h);
  }
}

// hyper = {lr, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt, decoupled, amsgrad}: checked, then rounded to fp32
static int adam_hyper(const char* who, int t, const double* d, bool have_vmax, AdamHyper* out) {
  const double lr = d[0], b1 = d[1], b2 = d[2], eps = d[3], wd = d[4], step_size = d[5], bc2 = d[6];
  const bool decoupled = d[7] != 0.0, amsgrad = d[8] != 0.0;
  SSP_CHECK_ARG(std::isfinite(lr) && lr >= 0.0, "%s: tuple %d: lr must be finite and >= 0", who, t);
  SSP_CHECK_ARG(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, "%s: tuple %d: beta1 and beta2 must lie in [0, 1)", who, t);
  SSP_CHECK_ARG(eps > 0.0 && std::isfinite(eps) && (float)eps > 0.f, "%s: tuple %d: eps must be > 0 (as fp32)", who, t);
  SSP_CHECK_ARG(std::isfinite(wd) && wd >= 0.0, "%s: tuple %d: weight_decay must be finite and >= 0", who, t);
  SSP_CHECK_ARG(std::isfinite(step_size) && std::isfinite((float)step_size), "%s: tuple %d: step_size is not finite", who, t);
  SSP_CHECK_ARG(std::isfinite(bc2) && bc2 > 0.0 && (float)bc2 > 0.f, "%s: tuple %d: bc2_sqrt must be finite and > 0", who, t);
  SSP_CHECK_ARG(!amsgrad || have_vmax, "%s: tuple %d: amsgrad needs the max_exp_avg_sq buffer", who, t);
  out->decay = (float)(1.0 - lr * wd);
  out->wd = (float)wd;
  out->w1 = (float)(1.0 - b1);
  out->b2 = (float)b2;
  out->w2 = (float)(1.0 - b2);
  out->bc2 = (float)bc2;
  out->eps = (float)eps;
  out->nstep = (float)(-step_size);
  out->flags = (wd != 0.0 ? (decoupled ? ADAM_DECOUPLED : ADAM_L2) : 0) | (amsgrad ? ADAM_AMSGRAD : 0);
  return SSP_OK;
}

#define ADAM_MAX_GRID (256 * 8)      // workgroups: 8 per CU, the same cap as sgd.hip

int ssp_adam_step_launch(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, double lr, double beta1,
                         double beta2, double eps, double weight_decay, double step_size, double bc2_sqrt, int decoupled,
                         int amsgrad, hipStream_t stream) {
  SSP_CHECK_ARG(p != nullptr && g != nullptr && m != nullptr && v != nullptr && n > 0, "adam_step: null buffer or empty range");
  SSP_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax) & 15) == 0,
                "adam_step: buffers must be 16-byte aligned");
  const double d[9] = {lr, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt, decoupled ? 1.0 : 0.0, amsgrad ? 1.0 : 0.0};
  AdamArgs a{p, g, m, v, vmax, n, {}};
  const int rc = adam_hyper("adam_step", 0, d, vmax != nullptr, &a.h);
  if (rc != SSP_OK) return rc;
  SspProfScope prof(SSP_PROF_OPTIM, stream, 0.0);
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > ADAM_MAX_GRID) blocks = ADAM_MAX_GRID;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  SSP_CHECK_LAUNCH("adam_step");
  return SSP_OK;
}

// ---- the same update over a table of segments (include/ssp_hip.h: ssp_adam_step_table) ------------------------------
// The walk of sgd_table_kernel: rows {parameter offset, gradient offset, state offset, length, tuple} in device memory,
// the tuples in the kernel arguments, work cut into chunks of 4096 floats dealt round-robin over the workgroups in table
// order.  m, v and vmax have one layout, so one state offset serves the three.
#define SSP_ADAM_MAX_TUPLES 16
#define ADAM_CHUNK 4096       // floats per chunk (= 1 << 12)
#define ADAM_MAX_SEGMENT ((int64_t)1 << 42)      // floats: chunk indices stay far inside 32 bits

struct AdamTableArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* vmax;
  const int64_t* table;      // [nseg][5]
  int nseg;
  AdamHyper h[SSP_ADAM_MAX_TUPLES];
};

__global__ void __launch_bounds__(256) adam_table_kernel(AdamTableArgs a) {
  const uint32_t grid = gridDim.x;
  uint32_t pos = 0;          // (chunks of the segments before this one) % grid
  for (int s = 0; s < a.nseg; ++s) {
    const int64_t* row = a.table + (int64_t)s * 5;
    const int64_t len = row[3];
    const uint32_t nch = (uint32_t)((len + ADAM_CHUNK - 1) >> 12);      // (the entry point bounds it: 32-bit walk)
    // chunk c of this segment belongs to workgroup (pos + c) % grid: this workgroup's first one
    uint32_t c = blockIdx.x >= pos ? blockIdx.x - pos : blockIdx.x + grid - pos;
    if (c < nch) {
      float* p = a.p + row[0];
      const float* g = a.g + row[1];
      float* m = a.m + row[2];
      float* v = a.v + row[2];
      float* vmax = a.vmax + row[2];      // (never dereferenced by a tuple without amsgrad)
      const AdamHyper h = a.h[row[4]];
      for (; c < nch; c += grid) {
        const int64_t lo = (int64_t)c * ADAM_CHUNK;
        const int64_t hi = lo + ADAM_CHUNK < len ? lo + ADAM_CHUNK : len;
        const int64_t q0 = lo >> 2, q1 = hi >> 2;      // whole quads of the chunk (lo is a multiple of 4)
        for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) adam_quad(p, g, m, v, vmax, q, h);
        const int64_t t = (q1 << 2) + threadIdx.x;     // scalar tail of the segment (its last chunk only)
        if (t < hi) adam_scalar(p, g, m, v, vmax, t, h);
      }
    }
    pos += nch % grid;
    if (pos >= grid) pos -= grid;
  }
}

int ssp_adam_step_table_launch(float* p, const float* g, float* m, float* v, float* vmax, int64_t p_floats,
                               int64_t g_floats, int64_t s_floats, const int64_t* table_dev, const int64_t* table_host,
                               int nseg, const double* hyper, int ntuple, hipStream_t stream) {
  SSP_CHECK_ARG(p != nullptr && g != nullptr && m != nullptr && v != nullptr && p_floats > 0 && g_floats > 0 && s_floats > 0,
                "adam_step_table: null buffer or empty buffer");
  SSP_CHECK_ARG(table_dev != nullptr && table_host != nullptr && nseg >= 1, "adam_step_table: no segment table");
  SSP_CHECK_ARG(hyper != nullptr && ntuple >= 1 && ntuple <= SSP_ADAM_MAX_TUPLES,
                "adam_step_table: between 1 and %d hyper-parameter tuples", SSP_ADAM_MAX_TUPLES);
  SSP_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax) & 15) == 0 &&
                    (((uintptr_t)table_dev) & 7) == 0,
                "adam_step_table: buffers must be 16-byte aligned");
  AdamTableArgs a;
  a.p = p; a.g = g; a.m = m; a.v = v; a.vmax = vmax; a.table = table_dev; a.nseg = nseg;
  for (int t = 0; t < SSP_ADAM_MAX_TUPLES; ++t) {
    const int rc = adam_hyper("adam_step_table", t < ntuple ? t : 0, hyper + 9 * (t < ntuple ? t : 0), vmax != nullptr, &a.h[t]);
    if (rc != SSP_OK) return rc;
  }
  // every row against the buffer lengths, BEFORE anything is launched: a bad table must never become a write outside
  // the buffers
  int64_t chunks = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t* row = table_host + (int64_t)s * 5;
    const int64_t po = row[0], go = row[1], so = row[2], len = row[3], t = row[4];
    SSP_CHECK_ARG(len >= 1 && len <= ADAM_MAX_SEGMENT, "adam_step_table: segment %d: length %lld", s, (long long)len);
    SSP_CHECK_ARG(t >= 0 && t < ntuple, "adam_step_table: segment %d: tuple index %lld of %d", s, (long long)t, ntuple);
    SSP_CHECK_ARG(po >= 0 && go >= 0 && so >= 0 && ((po | go | so) & 3) == 0,
                  "adam_step_table: segment %d: offsets must be non-negative multiples of 4 floats", s);
    SSP_CHECK_ARG(len <= p_floats && po <= p_floats - len, "adam_step_table: segment %d ends outside the parameter buffer", s);
    SSP_CHECK_ARG(len <= g_floats && go <= g_floats - len, "adam_step_table: segment %d ends outside the gradient buffer", s);
    SSP_CHECK_ARG(len <= s_floats && so <= s_floats - len, "adam_step_table: segment %d ends outside the state buffers", s);
    chunks += (len + ADAM_CHUNK - 1) / ADAM_CHUNK;
  }
  SspProfScope prof(SSP_PROF_OPTIM, stream, 0.0);
  const int64_t blocks = chunks < ADAM_MAX_GRID ? chunks : ADAM_MAX_GRID;
  hipLaunchKernelGGL(adam_table_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  SSP_CHECK_LAUNCH("adam_step_table");
  return SSP_OK;
}

// ---- global-norm gradient clipping (include/ssp_hip.h: ssp_grad_sumsq_table, ssp_grad_scale_table) -------------------
// Two launches on one stream, no host synchronisation and no atomics.  Both walk the gradient segments of a table (row
// fields 1 and 3: gradient offset and length; the gaps between segments are never read) with the chunk dealing above; a
// NULL table means the single range [0, grad_floats).
//   sumsq: every lane adds the squares of its elements in double (an fp32 square is exact in double) in walk order, the
//          256 lane sums are added in LDS by a fixed halving tree, one double partial per workgroup.
//   scale: every workgroup adds the partials in the same fixed order (lane t adds partials t, t + 256, ... in ascending
//          order, then the same tree), so all workgroups hold the same sum bit for bit; norm = sqrt(sum),
//          coef = min(1, max_norm / (norm + 1e-6)) in double, rounded once to fp32; g *= coef in place (skipped when the
//          rounded coef is exactly 1).  Workgroup 0 writes {norm, coef} as fp32.
#define CLIP_MAX_PARTIALS 65536      // partials one scale launch adds (a table launch writes at most ADAM_MAX_GRID)

struct ClipArgs {
  float* g;
  const int64_t* table;      // [nseg][5], or nullptr: the one range [0, n)
  int64_t n;
  int nseg;
  double* partial;
  int npartial;
  double max_norm;
  float* result;
};

__device__ __forceinline__ double clip_block_sum(double s, double* lds) {
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) lds[threadIdx.x] = lds[threadIdx.x] + lds[threadIdx.x + w];
    __syncthreads();
  }
  return lds[0];
}

template <bool SCALE>
__device__ __forceinline__ void clip_walk(const ClipArgs& a, float coef, double& acc) {
  const uint32_t grid = gridDim.x;
  uint32_t pos = 0;
  for (int s = 0; s < a.nseg; ++s) {
    const int64_t goff = a.table ? a.table[(int64_t)s * 5 + 1] : 0;
    const int64_t len = a.table ? a.table[(int64_t)s * 5 + 3] : a.n;
    const uint32_t nch = (uint32_t)((len + ADAM_CHUNK - 1) >> 12);
    uint32_t c = blockIdx.x >= pos ? blockIdx.x - pos : blockIdx.x + grid - pos;
    float* g = a.g + goff;
    for (; c < nch; c += grid) {
      const int64_t lo = (int64_t)c * ADAM_CHUNK;
      const int64_t hi = lo + ADAM_CHUNK < len ? lo + ADAM_CHUNK : len;
      const int64_t q0 = lo >> 2, q1 = hi >> 2;
      for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        float4 x = reinterpret_cast<const float4*>(g)[q];
        if (SCALE) {
          x.x = __fmul_rn(x.x, coef); x.y = __fmul_rn(x.y, coef); x.z = __fmul_rn(x.z, coef); x.w = __fmul_rn(x.w, coef);
          reinterpret_cast<float4*>(g)[q] = x;
        } else {
          acc += (double)x.x * (double)x.x;
          acc += (double)x.y * (double)x.y;
          acc += (double)x.z * (double)x.z;
          acc += (double)x.w * (double)x.w;
        }
      }
      const int64_t t = (q1 << 2) + threadIdx.x;
      if (t < hi) {
        if (SCALE) g[t] = __fmul_rn(g[t], coef);
        else acc += (double)g[t] * (double)g[t];
      }
    }
    pos += nch % grid;
    if (pos >= grid) pos -= grid;
  }
}

__global__ void __launch_bounds__(256) grad_sumsq_kernel(ClipArgs a) {
  __shared__ double lds[256];
  double acc = 0.0;
  clip_walk<false>(a, 0.f, acc);
  const double s = clip_block_sum(acc, lds);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) grad_scale_kernel(ClipArgs a) {
  __shared__ double lds[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < a.npartial; i += 256) acc += a.partial[i];
  const double norm = sqrt(clip_block_sum(acc, lds));
  const double c = a.max_norm / (norm + 1e-6);
  const float coef = (float)(c < 1.0 || c != c ? c : 1.0);      // clamp(max = 1); a NaN norm propagates, as in torch
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.result[0] = (float)norm;
    a.result[1] = coef;
  }
  if (coef == 1.f) return;      // (workgroup-uniform) x * 1 is x: nothing to write
  double unused = 0.0;
  clip_walk<true>(a, coef, unused);
}

// the rows of a clip launch against the gradient buffer; *chunks = the chunks of the walk
static int clip_check(const char* who, const float* g, int64_t g_floats, const int64_t* table_dev, const int64_t* table_host,
                      int nseg, int64_t* chunks) {
  SSP_CHECK_ARG(g != nullptr && g_floats > 0, "%s: null or empty gradient buffer", who);
  SSP_CHECK_ARG((((uintptr_t)g) & 15) == 0 && (((uintptr_t)table_dev) & 7) == 0, "%s: buffers must be 16-byte aligned", who);
  SSP_CHECK_ARG((table_dev == nullptr) == (table_host == nullptr), "%s: the table needs its device and its host copy", who);
  if (table_dev == nullptr) {
    SSP_CHECK_ARG(nseg == 1 && g_floats <= ADAM_MAX_SEGMENT, "%s: without a table nseg is 1 (the range [0, grad_floats))", who);
    *chunks = (g_floats + ADAM_CHUNK - 1) / ADAM_CHUNK;
    return SSP_OK;
  }
  SSP_CHECK_ARG(nseg >= 1, "%s: no segment table", who);
  int64_t n = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t go = table_host[(int64_t)s * 5 + 1], len = table_host[(int64_t)s * 5 + 3];
    SSP_CHECK_ARG(len >= 1 && len <= ADAM_MAX_SEGMENT, "%s: segment %d: length %lld", who, s, (long long)len);
    SSP_CHECK_ARG(go >= 0 && (go & 3) == 0, "%s: segment %d: offsets must be non-negative multiples of 4 floats", who, s);
    SSP_CHECK_ARG(len <= g_floats && go <= g_floats - len, "%s: segment %d ends outside the gradient buffer", who, s);
    n += (len + ADAM_CHUNK - 1) / ADAM_CHUNK;
  }
  *chunks = n;
  return SSP_OK;
}

int ssp_grad_sumsq_table_launch(const float* g, int64_t g_floats, const int64_t* table_dev, const int64_t* table_host,
                                int nseg, double* partial, int partial_capacity, int* npartial, hipStream_t stream) {
  int64_t chunks = 0;
  const int rc = clip_check("grad_sumsq_table", g, g_floats, table_dev, table_host, nseg, &chunks);
  if (rc != SSP_OK) return rc;
  SSP_CHECK_ARG(partial != nullptr && (((uintptr_t)partial) & 7) == 0 && partial_capacity >= 1 && npartial != nullptr,
                "grad_sumsq_table: no room for the partial sums");
  int64_t blocks = chunks < ADAM_MAX_GRID ? chunks : ADAM_MAX_GRID;
  if (blocks > partial_capacity) blocks = partial_capacity;
  ClipArgs a{const_cast<float*>(g), table_dev, g_floats, nseg, partial, (int)blocks, 0.0, nullptr};
  SspProfScope prof(SSP_PROF_OPTIM, stream, 0.0);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  SSP_CHECK_LAUNCH("grad_sumsq_table");
  *npartial = (int)blocks;
  return SSP_OK;
}

int ssp_grad_scale_table_launch(float* g, int64_t g_floats, const int64_t* table_dev, const int64_t* table_host, int nseg,
                                const double* partial, int npartial, double max_norm, float* result, hipStream_t stream) {
  int64_t chunks = 0;
  const int rc = clip_check("grad_scale_table", g, g_floats, table_dev, table_host, nseg, &chunks);
  if (rc != SSP_OK) return rc;
  SSP_CHECK_ARG(partial != nullptr && (((uintptr_t)partial) & 7) == 0 && npartial >= 1 && npartial <= CLIP_MAX_PARTIALS,
                "grad_scale_table: between 1 and %d partial sums", CLIP_MAX_PARTIALS);
  SSP_CHECK_ARG(result != nullptr && (((uintptr_t)result) & 3) == 0, "grad_scale_table: no result buffer");
  SSP_CHECK_ARG(max_norm == max_norm && max_norm >= 0.0, "grad_scale_table: max_norm must be >= 0");
  const int64_t blocks = chunks < ADAM_MAX_GRID ? chunks : ADAM_MAX_GRID;
  ClipArgs a{g, table_dev, g_floats, nseg, const_cast<double*>(partial), npartial, max_norm, result};
  SspProfScope prof(SSP_PROF_OPTIM, stream, 0.0);
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  SSP_CHECK_LAUNCH("grad_scale_table");
  return SSP_OK;
}

// SGD with momentum, dampening, L2 weight decay and Nesterov over one contiguous fp32 range: the update the reference
// runs through torch.optim.SGD (train.py:388 `optim.SGD(model.parameters(), lr=learning_rate/batch_size,
// momentum=momentum, dampening=0, weight_decay=decay*batch_size)`, train.py:106 `optimizer.step()`).
//
//   d = g + weight_decay * p
//   first step with momentum:  buf = d          later steps:  buf = momentum * buf + (1 - dampening) * d
//   d = nesterov ? d + momentum * buf : buf     (momentum == 0: d stays g + weight_decay * p)
//   p = p - lr * d
//
// HBM-bound: 3 reads + 2 writes of 4 B per parameter (202 MB each for yolo-pose.cfg => ~1 GB, ~0.13 ms at 8 TB/s).
// The host side (singleshotpose_amd/optim.py) keeps parameters, momentum and the backward's gradients in three flat
// buffers with one layout, so a whole step is ONE launch instead of torch's ~70 x 3 foreach segments.
#include "ssp_common.h"

// the hyper-parameters of one update: a whole launch's (sgd_kernel) or one tuple of a segment table's (sgd_table_kernel)
struct SgdHyper {
  float lr, momentum, dampening, wd;
  int nesterov, first;
};

struct SgdArgs {
  float* p;
  const float* g;
  float* m;
  int64_t n;
  SgdHyper h;
};

__device__ __forceinline__ float sgd_one(float p, float g, float& buf, const SgdHyper& a) {
  // one fused multiply-add per torch foreach pass (add(alpha) -> mul, add(alpha) -> add(alpha)): the same operation
  // order as torch.optim.SGD, each pass rounded once (torch's CPU build may round the product separately: <= 1 ulp)
  float d = (a.wd != 0.f) ? __fmaf_rn(a.wd, p, g) : g;
  if (a.momentum != 0.f) {
    if (a.first) buf = d;
    else buf = __fmaf_rn(1.f - a.dampening, d, __fmul_rn(a.momentum, buf));
    d = a.nesterov ? __fmaf_rn(a.momentum, buf, d) : buf;
  }
  return __fmaf_rn(-a.lr, d, p);
}

// four consecutive elements at float offset 4 * i of 16-byte aligned p / g / m
__device__ __forceinline__ void sgd_quad(float* p, const float* g, float* m, int64_t i, const SgdHyper& h) {
  const bool mom = h.momentum != 0.f;
  float4 pv = reinterpret_cast<const float4*>(p)[i];
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (mom && !h.first) b = reinterpret_cast<const float4*>(m)[i];
  pv.x = sgd_one(pv.x, gv.x, b.x, h);
  pv.y = sgd_one(pv.y, gv.y, b.y, h);
  pv.z = sgd_one(pv.z, gv.z, b.z, h);
  pv.w = sgd_one(pv.w, gv.w, b.w, h);
  reinterpret_cast<float4*>(p)[i] = pv;
  if (mom) reinterpret_cast<float4*>(m)[i] = b;
}

__device__ __forceinline__ void sgd_scalar(float* p, const float* g, float* m, int64_t i, const SgdHyper& h) {
  const bool mom = h.momentum != 0.f;
  float b = (mom && !h.first) ? m[i] : 0.f;
  p[i] = sgd_one(p[i], g[i], b, h);
  if (mom) m[i] = b;
}

__global__ void __launch_bounds__(256) sgd_kernel(SgdArgs a) {
  const int64_t n4 = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) sgd_quad(a.p, a.g, a.m, i, a.h);
  // tail (n not a multiple of 4): the first workgroup finishes it
  if (blockIdx.x == 0) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    if (i < a.n) sgd_scalar(a.p, a.g, a.m, i, a.h);
  }
}

int ssp_sgd_step_launch(float* p, const float* g, float* m, int64_t n, float lr, float momentum, float dampening,
                        float weight_decay, int nesterov, int first_step, hipStream_t stream) {
  SSP_CHECK_ARG(p != nullptr && g != nullptr && n > 0, "sgd_step: null buffer or empty range");
  SSP_CHECK_ARG(momentum == 0.f || m != nullptr, "sgd_step: momentum needs a momentum buffer");
  SSP_CHECK_ARG(!nesterov || (momentum > 0.f && dampening == 0.f), "sgd_step: nesterov needs momentum > 0 and dampening == 0");
  SSP_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0, "sgd_step: buffers must be 16-byte aligned");
  SspProfScope prof(SSP_PROF_OPTIM, stream, 0.0);
  SgdArgs a{p, g, m, n, {lr, momentum, dampening, weight_decay, nesterov, first_step}};
  int64_t blocks = ((n >> 2) + 255) / 256;
  const int64_t cap = 256 * 8;
  if (blocks < 1) blocks = 1;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  SSP_CHECK_LAUNCH("sgd_step");
  return SSP_OK;
}

// ---- the same update over a table of segments (include/ssp_hip.h: ssp_sgd_step_table) --------------------------------
// Parameter groups with different hyper-parameters (train.py:381-387: no weight decay on BatchNorm / bias parameters) and
// optimizers that hold part of a model (a fine-tuned head) are many short ranges, each with one of a few hyper-parameter
// tuples.  One launch walks them all: the table rows {param offset, grad offset, momentum offset, length, tuple} sit in
// device memory (they change only with the layout), the tuples travel in the kernel arguments (lr changes every batch).
// Work is cut into chunks of SGD_CHUNK floats, dealt round-robin over the workgroups in table order: every workgroup walks
// the (short, L2-resident) table once with uniform arithmetic and needs no prefix array.
#define SSP_SGD_MAX_TUPLES 16
#define SGD_CHUNK 4096       // floats per chunk: 256 lanes x 4 quads (= 1 << 12)
#define SGD_MAX_SEGMENT ((int64_t)1 << 42)      // floats: chunk indices stay far inside 32 bits

struct SgdTableArgs {
  float* p;
  const float* g;
  float* m;
  const int64_t* table;      // [nseg][5]
  int nseg;
  SgdHyper h[SSP_SGD_MAX_TUPLES];
};

__global__ void __launch_bounds__(256) sgd_table_kernel(SgdTableArgs a) {
  const uint32_t grid = gridDim.x;
  uint32_t pos = 0;          // (chunks of the segments before this one) % grid
  for (int s = 0; s < a.nseg; ++s) {
    const int64_t* row = a.table + (int64_t)s * 5;
    const int64_t len = row[3];
    const uint32_t nch = (uint32_t)((len + SGD_CHUNK - 1) >> 12);      // (the entry point bounds it: 32-bit walk)
    // chunk c of this segment belongs to workgroup (pos + c) % grid: this workgroup's first one
    uint32_t c = blockIdx.x >= pos ? blockIdx.x - pos : blockIdx.x + grid - pos;
    if (c < nch) {
      float* p = a.p + row[0];
      const float* g = a.g + row[1];
      float* m = a.m + row[2];        // (never dereferenced by a tuple without momentum)
      const SgdHyper h = a.h[row[4]];
      for (; c < nch; c += grid) {
        const int64_t lo = (int64_t)c * SGD_CHUNK;
        const int64_t hi = lo + SGD_CHUNK < len ? lo + SGD_CHUNK : len;
        const int64_t q0 = lo >> 2, q1 = hi >> 2;      // whole quads of the chunk (lo is a multiple of 4)
        for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) sgd_quad(p, g, m, q, h);
        const int64_t t = (q1 << 2) + threadIdx.x;     // scalar tail of the segment (its last chunk only)
        if (t < hi) sgd_scalar(p, g, m, t, h);
      }
    }
    pos += nch % grid;
    if (pos >= grid) pos -= grid;
  }
}

int ssp_sgd_step_table_launch(float* p, const float* g, float* m, int64_t p_floats, int64_t g_floats, int64_t m_floats,
                              const int64_t* table_dev, const int64_t* table_host, int nseg, const float* hyper, int ntuple,
                              hipStream_t stream) {
  SSP_CHECK_ARG(p != nullptr && g != nullptr && p_floats > 0 && g_floats > 0 && m_floats >= 0,
                "sgd_step_table: null buffer or empty buffer");
  SSP_CHECK_ARG(table_dev != nullptr && table_host != nullptr && nseg >= 1, "sgd_step_table: no segment table");
  SSP_CHECK_ARG(hyper != nullptr && ntuple >= 1 && ntuple <= SSP_SGD_MAX_TUPLES,
                "sgd_step_table: between 1 and %d hyper-parameter tuples", SSP_SGD_MAX_TUPLES);
  SSP_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0 && (((uintptr_t)table_dev) & 7) == 0,
                "sgd_step_table: buffers must be 16-byte aligned");
  SgdTableArgs a;
  a.p = p; a.g = g; a.m = m; a.table = table_dev; a.nseg = nseg;
  bool mom[SSP_SGD_MAX_TUPLES];
  for (int t = 0; t < SSP_SGD_MAX_TUPLES; ++t) {
    const float* h = hyper + 6 * (t < ntuple ? t : 0);
    a.h[t] = SgdHyper{h[0], h[1], h[2], h[3], h[4] != 0.f ? 1 : 0, h[5] != 0.f ? 1 : 0};
    mom[t] = a.h[t].momentum != 0.f;
    SSP_CHECK_ARG(!a.h[t].nesterov || (a.h[t].momentum > 0.f && a.h[t].dampening == 0.f),
                  "sgd_step_table: tuple %d: nesterov needs momentum > 0 and dampening == 0", t);
    SSP_CHECK_ARG(!mom[t] || m != nullptr, "sgd_step_table: tuple %d: momentum needs a momentum buffer", t);
  }
  // every row against the buffer lengths, BEFORE anything is launched: a bad table must never become a write outside
  // the buffers
  int64_t chunks = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t* row = table_host + (int64_t)s * 5;
    const int64_t po = row[0], go = row[1], mo = row[2], len = row[3], t = row[4];
    SSP_CHECK_ARG(len >= 1 && len <= SGD_MAX_SEGMENT, "sgd_step_table: segment %d: length %lld", s, (long long)len);
    SSP_CHECK_ARG(t >= 0 && t < ntuple, "sgd_step_table: segment %d: tuple index %lld of %d", s, (long long)t, ntuple);
    SSP_CHECK_ARG(po >= 0 && go >= 0 && mo >= 0 && ((po | go | mo) & 3) == 0,
                  "sgd_step_table: segment %d: offsets must be non-negative multiples of 4 floats", s);
    SSP_CHECK_ARG(len <= p_floats && po <= p_floats - len, "sgd_step_table: segment %d ends outside the parameter buffer", s);
    SSP_CHECK_ARG(len <= g_floats && go <= g_floats - len, "sgd_step_table: segment %d ends outside the gradient buffer", s);
    SSP_CHECK_ARG(!mom[t] || (len <= m_floats && mo <= m_floats - len),
                  "sgd_step_table: segment %d ends outside the momentum buffer", s);
    chunks += (len + SGD_CHUNK - 1) / SGD_CHUNK;
  }
  SspProfScope prof(SSP_PROF_OPTIM, stream, 0.0);
  const int64_t cap = 256 * 8;
  const int64_t blocks = chunks < cap ? chunks : cap;
  hipLaunchKernelGGL(sgd_table_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  SSP_CHECK_LAUNCH("sgd_step_table");
  return SSP_OK;
}

// Evaluation maths of valid.py:152-177 on the device, batched over poses.
//
// pose_errors: per pose pair (gt, predicted), over the N mesh vertices
//   pixel_dist  = mean_i || proj(K [R|t]_gt v_i) - proj(K [R|t]_pr v_i) ||    (utils.py:40-45 compute_projection: the
//                 projections are stored as float32, valid.py:163-164 takes the float32 norm)
//   vertex_dist = mean_i || [R|t]_gt v_i - [R|t]_pr v_i ||                     (utils.py:47-48, valid.py:168-172, float64)
//   trans_dist  = || t_gt - t_pr ||                                            (valid.py:148)
//   angle_dist  = deg(acos((trace(R_gt R_pr^T) - 1) / 2))                       (utils.py:31-35; NaN when rounding pushes
//                 the argument above 1 for identical rotations, as numpy's arccos does)
// pose_errors_models: the same with one mesh per pose (multi_obj_pose_estimation/valid_multi.py:47-50 loads a mesh per
//   object); the loop body is shared, so one mesh gives the single-mesh bits.
// pts_diameter: largest pairwise distance of the mesh (utils.py:50-58), O(N^2) pairs.
// adds: ADD-S, adi(pts_est, pts_gt) of utils.py:60-63 - mean over the ground-truth-posed vertices of the distance to the
//   nearest predicted-posed vertex; all N^2 pairs per pose in fp64 instead of the reference's KD-tree.
//
// One workgroup per pose; vertices stream from HBM/L2 (N*24 bytes, shared by every pose), the means are fp64 tree
// reductions in LDS.  Latency-bound sizes (N ~ 6 k for LINEMOD ape): reported as time per call, not a roofline.
#include "ssp_common.h"

__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// The four errors of pose b over the N vertices at `verts`: the body of both pose-error kernels (one mesh for the launch,
// or one mesh per pose), so that the two cannot drift apart.
__device__ __forceinline__ void pose_errors_body(const double* __restrict__ verts, int N, int b,
                                                 const double* __restrict__ Rt_gt, const double* __restrict__ Rt_pr,
                                                 const double* __restrict__ Kmat, int k_per_pose,
                                                 double* __restrict__ out, double* red) {
  const int tid = threadIdx.x;
  // Rt stored as R (9, row-major) | t (3): the layout ssp_pnp_batched writes
  double Rg[9], tg[3], Rp[9], tp[3], K[9], Pg[12], Pp[12];
#pragma unroll
  for (int i = 0; i < 9; ++i) { Rg[i] = Rt_gt[b * 12 + i]; Rp[i] = Rt_pr[b * 12 + i]; K[i] = Kmat[(k_per_pose ? b * 9 : 0) + i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { tg[i] = Rt_gt[b * 12 + 9 + i]; tp[i] = Rt_pr[b * 12 + 9 + i]; }
  // P = K [R|t]  (3x4), as internal_calibration.dot(transformation)
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double sg = 0.0, sp = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        sg += K[r * 3 + k] * (c < 3 ? Rg[k * 3 + c] : tg[k]);
        sp += K[r * 3 + k] * (c < 3 ? Rp[k * 3 + c] : tp[k]);
      }
      Pg[r * 4 + c] = sg;
      Pp[r * 4 + c] = sp;
    }
  double s2d = 0.0, s3d = 0.0;
  for (int i = tid; i < N; i += 256) {
    const double x = verts[i * 3], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
    double cg[3], cp[3], vg[3], vp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      cg[r] = Pg[r * 4] * x + Pg[r * 4 + 1] * y + Pg[r * 4 + 2] * z + Pg[r * 4 + 3];
      cp[r] = Pp[r * 4] * x + Pp[r * 4 + 1] * y + Pp[r * 4 + 2] * z + Pp[r * 4 + 3];
      vg[r] = Rg[r * 3] * x + Rg[r * 3 + 1] * y + Rg[r * 3 + 2] * z + tg[r];
      vp[r] = Rp[r * 3] * x + Rp[r * 3 + 1] * y + Rp[r * 3 + 2] * z + tp[r];
    }
    // float32 projections, float32 difference and norm (compute_projection's dtype='float32' array)
    const float dx = __fsub_rn((float)(cg[0] / cg[2]), (float)(cp[0] / cp[2]));
    const float dy = __fsub_rn((float)(cg[1] / cg[2]), (float)(cp[1] / cp[2]));
    s2d += (double)__fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
    const double ex = vg[0] - vp[0], ey = vg[1] - vp[1], ez = vg[2] - vp[2];
    s3d += sqrt(ex * ex + ey * ey + ez * ez);
  }
  s2d = block_sum(s2d, red);
  s3d = block_sum(s3d, red);
  if (tid == 0) {
    out[b * 4 + 0] = s2d / (double)N;
    out[b * 4 + 1] = s3d / (double)N;
    const double dx = tg[0] - tp[0], dy = tg[1] - tp[1], dz = tg[2] - tp[2];
    out[b * 4 + 2] = sqrt(dx * dx + dy * dy + dz * dz);
    double trace = 0.0;   // trace(R_gt R_pr^T) = sum_ij Rg[i][j] Rp[i][j]
#pragma unroll
    for (int i = 0; i < 3; ++i) trace += Rg[i * 3] * Rp[i * 3] + Rg[i * 3 + 1] * Rp[i * 3 + 1] + Rg[i * 3 + 2] * Rp[i * 3 + 2];
    out[b * 4 + 3] = acos((trace - 1.0) / 2.0) * (180.0 / 3.14159265358979323846);
  }
}

__global__ void __launch_bounds__(256) pose_errors_kernel(const double* __restrict__ verts, int N,
                                                          const double* __restrict__ Rt_gt,
                                                          const double* __restrict__ Rt_pr,
                                                          const double* __restrict__ Kmat, int k_per_pose,
                                                          double* __restrict__ out) {
  __shared__ double red[256];
  pose_errors_body(verts, N, blockIdx.x, Rt_gt, Rt_pr, Kmat, k_per_pose, out, red);
}

// One mesh per pose: pose b reads verts[model_off[m] .. model_off[m+1]) with m = pose_model[b].  The offsets and the
// model indices are the caller's to get right (include/ssp_hip.h); nothing here re-checks them.
__global__ void __launch_bounds__(256) pose_errors_models_kernel(const double* __restrict__ verts,
                                                                 const int* __restrict__ model_off,
                                                                 const int* __restrict__ pose_model,
                                                                 const double* __restrict__ Rt_gt,
                                                                 const double* __restrict__ Rt_pr,
                                                                 const double* __restrict__ Kmat, int k_per_pose,
                                                                 double* __restrict__ out) {
  __shared__ double red[256];
  const int m = pose_model[blockIdx.x];
  const int v0 = model_off[m];
  pose_errors_body(verts + (size_t)v0 * 3, model_off[m + 1] - v0, blockIdx.x, Rt_gt, Rt_pr, Kmat, k_per_pose, out, red);
}

// ADD-S (adi(pts_est, pts_gt), utils.py:60-63): for every ground-truth-posed vertex the distance to the NEAREST
// predicted-posed vertex of the same mesh, averaged.  Brute force, no tree: workgroup (chunk, pose) owns ADDS_CHUNK
// ground-truth-posed query vertices in registers (ADDS_Q per thread) and sweeps all predicted-posed vertices through an
// LDS tile; they are transformed as the tile is loaded, so no transformed copy of a mesh is ever written to HBM.  Every
// thread keeps the running minimum of the SQUARED distance, (dx*dx + dy*dy) + dz*dz with every operation rounded on its
// own (no contraction) - the arithmetic of the numpy restatement `((gt[:, None] - est[None]) ** 2).sum(axis=2).min(axis=1)`
// - and takes one square root per query after the sweep (the minimum commutes with the root).  The workgroup's sum goes to
// part[pose][chunk]; adds_finish_kernel adds a pose's chunks in index order: no atomics, the same bits every launch.
// Queries per thread, timed at N = 5841, n = 128: 1 -> 1.42 ms, 2 -> 1.39 ms, 4 -> 1.43 ms; the
// fp64 vector stream is the bound, not the LDS reads, and 4 leave too few workgroups when few poses are scored.
#ifndef SSP_ADDS_Q
#define SSP_ADDS_Q 2
#endif
constexpr int ADDS_Q = SSP_ADDS_Q;            // query vertices per thread: each LDS read of a tile vertex serves ADDS_Q pairs
constexpr int ADDS_TILE = 256;                // predicted-posed vertices per LDS tile (one per thread per load)
constexpr int ADDS_CHUNK = 256 * ADDS_Q;      // query vertices per workgroup

__global__ void __launch_bounds__(256) adds_partial_kernel(const double* __restrict__ verts,
                                                           const int* __restrict__ model_off,
                                                           const int* __restrict__ pose_model,
                                                           const double* __restrict__ Rt_gt,
                                                           const double* __restrict__ Rt_pr, int nchunks,
                                                           double* __restrict__ part) {
  __shared__ double tx[ADDS_TILE], ty[ADDS_TILE], tz[ADDS_TILE];
  __shared__ double red[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m = pose_model[b];
  const int v0 = model_off[m];
  const int N = model_off[m + 1] - v0;
  const int g0 = blockIdx.x * ADDS_CHUNK;
  if (g0 >= N) return;        // a chunk past this pose's mesh (the grid is sized for the largest one): whole workgroup
  const double* __restrict__ v = verts + (size_t)v0 * 3;
  double Rg[9], tg[3], Rp[9], tp[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) { Rg[i] = Rt_gt[b * 12 + i]; Rp[i] = Rt_pr[b * 12 + i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { tg[i] = Rt_gt[b * 12 + 9 + i]; tp[i] = Rt_pr[b * 12 + 9 + i]; }
  // query q of this thread: vertex g0 + q*256 + tid (coalesced loads); a query past N repeats vertex 0 and is not summed
  double qx[ADDS_Q], qy[ADDS_Q], qz[ADDS_Q], best[ADDS_Q];
#pragma unroll
  for (int q = 0; q < ADDS_Q; ++q) {
    const int g = g0 + q * 256 + tid;
    const int gi = g < N ? g : 0;
    const double x = v[gi * 3], y = v[gi * 3 + 1], z = v[gi * 3 + 2];
    qx[q] = Rg[0] * x + Rg[1] * y + Rg[2] * z + tg[0];
    qy[q] = Rg[3] * x + Rg[4] * y + Rg[5] * z + tg[1];
    qz[q] = Rg[6] * x + Rg[7] * y + Rg[8] * z + tg[2];
    best[q] = HUGE_VAL;
  }
  for (int e0 = 0; e0 < N; e0 += ADDS_TILE) {
    const int e = e0 + tid;
    if (e < N) {
      const double x = v[e * 3], y = v[e * 3 + 1], z = v[e * 3 + 2];
      tx[tid] = Rp[0] * x + Rp[1] * y + Rp[2] * z + tp[0];
      ty[tid] = Rp[3] * x + Rp[4] * y + Rp[5] * z + tp[1];
      tz[tid] = Rp[6] * x + Rp[7] * y + Rp[8] * z + tp[2];
    }
    __syncthreads();
    const int cnt = min(ADDS_TILE, N - e0);
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
      const double ex = tx[k], ey = ty[k], ez = tz[k];      // one address for the whole wave: an LDS broadcast
#pragma unroll
      for (int q = 0; q < ADDS_Q; ++q) {
        // every product and every sum rounded on its own.  Written with * and + under contract(off): __dmul_rn and
        // __dadd_rn are inline `x * y` / `x + y` in this compiler's headers, which the default contraction fuses into
        // FMAs all the same, and the pragma does not reach into them
#pragma clang fp contract(off)
        const double dx = qx[q] - ex, dy = qy[q] - ey, dz = qz[q] - ez;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        best[q] = fmin(d2, best[q]);
      }
    }
    __syncthreads();
  }
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < ADDS_Q; ++q)
    if (g0 + q * 256 + tid < N) s += sqrt(best[q]);
  s = block_sum(s, red);
  if (tid == 0) part[(size_t)b * nchunks + blockIdx.x] = s;
}

__global__ void __launch_bounds__(64) adds_finish_kernel(const double* __restrict__ part,
                                                         const int* __restrict__ model_off,
                                                         const int* __restrict__ pose_model, int nchunks, int n,
                                                         double* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n) return;
  const int m = pose_model[b];
  const int N = model_off[m + 1] - model_off[m];
  const int used = min(nchunks, (N + ADDS_CHUNK - 1) / ADDS_CHUNK);      // the chunks adds_partial_kernel wrote for this pose
  double s = 0.0;
  for (int c = 0; c < used; ++c) s += part[(size_t)b * nchunks + c];
  out[b] = s / (double)N;
}

// max_ij |p_i - p_j|^2, exact fp64 with the reference's summation order ((dx*dx + dy*dy) + dz*dz, no contraction):
// each thread owns one i, all threads sweep j through LDS tiles; the result is order-independent (a max), so the
// atomic on the bit pattern of the non-negative double is exact.
__global__ void __launch_bounds__(256) pts_diameter_kernel(const double* __restrict__ pts, int N,
                                                           unsigned long long* __restrict__ best_bits) {
  __shared__ double tile[256 * 3];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  double xi = 0.0, yi = 0.0, zi = 0.0;
  if (i < N) { xi = pts[i * 3]; yi = pts[i * 3 + 1]; zi = pts[i * 3 + 2]; }
  double best = 0.0;
  // pairs (i, j >= i) only, as the reference's triangular sweep: start at this workgroup's own tile
  for (int j0 = blockIdx.x * 256; j0 < N; j0 += 256) {
    const int j = j0 + tid;
    if (j < N) { tile[tid * 3] = pts[j * 3]; tile[tid * 3 + 1] = pts[j * 3 + 1]; tile[tid * 3 + 2] = pts[j * 3 + 2]; }
    __syncthreads();
    const int cnt = min(256, N - j0);
    if (i < N) {
      for (int k = 0; k < cnt; ++k) {
        const double dx = xi - tile[k * 3], dy = yi - tile[k * 3 + 1], dz = zi - tile[k * 3 + 2];
        const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        best = d2 > best ? d2 : best;
      }
    }
    __syncthreads();
  }
  // wave max, then one atomic per wave
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(best, off, 64);
    best = o > best ? o : best;
  }
  if ((tid & 63) == 0) atomicMax(best_bits, (unsigned long long)__double_as_longlong(best));
}

__global__ void diameter_finish_kernel(const unsigned long long* best_bits, double* out) {
  out[0] = sqrt(__longlong_as_double((long long)best_bits[0]));
}

int ssp_pose_errors_launch(const double* verts, int N, const double* Rt_gt, const double* Rt_pr, const double* K,
                           int k_per_pose, int n, double* out, hipStream_t stream) {
  SSP_CHECK_ARG(verts && Rt_gt && Rt_pr && K && out, "pose_errors: null buffer");
  SSP_CHECK_ARG(N > 0 && n > 0, "pose_errors: need N > 0 vertices and n > 0 poses");
  SspProfScope prof(SSP_PROF_REGION, stream, 0.0);
  hipLaunchKernelGGL(pose_errors_kernel, dim3(n), dim3(256), 0, stream, verts, N, Rt_gt, Rt_pr, K, k_per_pose, out);
  SSP_CHECK_LAUNCH("pose_errors");
  return SSP_OK;
}

int ssp_pts_diameter_launch(const double* pts, int N, double* out, double* scratch, hipStream_t stream) {
  SSP_CHECK_ARG(pts && out && scratch, "pts_diameter: null buffer");
  SSP_CHECK_ARG(N > 0, "pts_diameter: empty point set");
  SspProfScope prof(SSP_PROF_REGION, stream, 0.0);
  if (hipMemsetAsync(scratch, 0, 8, stream) != hipSuccess) {
    ssp_set_error("pts_diameter: hipMemsetAsync failed");
    return SSP_ERR_HIP;
  }
  hipLaunchKernelGGL(pts_diameter_kernel, dim3(ssp_cdiv(N, 256)), dim3(256), 0, stream, pts, N,
                     reinterpret_cast<unsigned long long*>(scratch));
  SSP_CHECK_LAUNCH("pts_diameter");
  hipLaunchKernelGGL(diameter_finish_kernel, dim3(1), dim3(1), 0, stream,
                     reinterpret_cast<const unsigned long long*>(scratch), out);
  SSP_CHECK_LAUNCH("pts_diameter_finish");
  return SSP_OK;
}

int ssp_pose_errors_models_launch(const double* verts, const int* model_off, const int* pose_model, int nM,
                                  const double* Rt_gt, const double* Rt_pr, const double* K, int k_per_pose, int n,
                                  double* out, hipStream_t stream) {
  SSP_CHECK_ARG(verts && model_off && pose_model && Rt_gt && Rt_pr && K && out, "pose_errors_models: null buffer");
  SSP_CHECK_ARG(nM > 0 && n > 0, "pose_errors_models: need nM > 0 models and n > 0 poses");
  SspProfScope prof(SSP_PROF_REGION, stream, 0.0);
  hipLaunchKernelGGL(pose_errors_models_kernel, dim3(n), dim3(256), 0, stream, verts, model_off, pose_model, Rt_gt, Rt_pr,
                     K, k_per_pose, out);
  SSP_CHECK_LAUNCH("pose_errors_models");
  return SSP_OK;
}

int64_t ssp_adds_workspace_doubles_impl(int n, int maxN) {
  if (n <= 0 || maxN <= 0) return 0;
  return (int64_t)n * ssp_cdiv(maxN, ADDS_CHUNK);
}

int ssp_adds_errors_launch(const double* verts, const int* model_off, const int* pose_model, int nM, int maxN,
                           const double* Rt_gt, const double* Rt_pr, int n, double* out, double* workspace,
                           int64_t workspace_doubles, hipStream_t stream) {
  SSP_CHECK_ARG(verts && model_off && pose_model && Rt_gt && Rt_pr && out && workspace, "adds_errors: null buffer");
  SSP_CHECK_ARG(nM > 0 && maxN > 0 && n > 0, "adds_errors: need nM > 0 models, maxN > 0 vertices and n > 0 poses");
  SSP_CHECK_ARG(n <= 65535, "adds_errors: at most 65535 poses per launch (got %d)", n);
  SSP_CHECK_ARG(workspace_doubles >= ssp_adds_workspace_doubles_impl(n, maxN),
                "adds_errors: workspace of %lld doubles, %lld needed (ssp_adds_workspace_doubles)",
                (long long)workspace_doubles, (long long)ssp_adds_workspace_doubles_impl(n, maxN));
  SspProfScope prof(SSP_PROF_REGION, stream, 0.0);
  const int nchunks = ssp_cdiv(maxN, ADDS_CHUNK);
  hipLaunchKernelGGL(adds_partial_kernel, dim3(nchunks, n), dim3(256), 0, stream, verts, model_off, pose_model, Rt_gt,
                     Rt_pr, nchunks, workspace);
  SSP_CHECK_LAUNCH("adds_partial");
  hipLaunchKernelGGL(adds_finish_kernel, dim3(ssp_cdiv(n, 64)), dim3(64), 0, stream, workspace, model_off, pose_model,
                     nchunks, n, out);
  SSP_CHECK_LAUNCH("adds_finish");
  return SSP_OK;
}

/* ssp_hip.h - C ABI of libssp_hip.so, the MI355X (gfx950) kernels behind the singleshotpose hot path.
 *
 * The reference (microsoft/singleshotpose) is pure Python on PyTorch; it has no native interface.  The device
 * work it performs happens inside ATen/cuDNN ops called from darknet.py / region_loss.py / utils.py.  Each entry
 * point below names the reference call site (file:line under /root/reference) whose device work it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (never throws); ssp_last_error() gives the thread-local text.
 *   - all pointers are DEVICE pointers owned by the caller (PyTorch); nothing is allocated or freed here, workspaces
 *     are passed in.  Launches are asynchronous on `stream` (a hipStream_t passed as void*); no hidden sync.
 *   - activations are fp32 NHWC: pixel p = (b*H + y)*W + x, channel c at base[p*ld + c]; `ld` (floats per pixel)
 *     may exceed the channel count so a call can read/write a channel slice of a wider buffer (route/concat).
 *   - packed filters are fp32 [rows][R*R][cols] with cols contiguous (see ssp_repack_*).
 */
#ifndef SSP_HIP_H
#define SSP_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* ssp_last_error(void);
int ssp_abi_version(void);
/* EXPERIMENT knobs (kernel variant / tile-order A-B switches used by bench.py --opt and tools/): process-wide, not
 * synchronised, never written by the product path (engine.Plan passes its per-launch choices as explicit `plan`
 * arguments below).  Unknown names are an error.  Never changes results beyond fp32 summation order. */
int ssp_set_option(const char* name, int value);

/* ---- convolution (stride 1, "same" padding, R = 1 or 3): nn.Conv2d at darknet.py:156,160 ------------------- */

/* out[p][co] (+)= sum_{tap,ci} in[p + tap][ci] * wt[co][tap][ci]  (+ bias[co]);  wt from ssp_repack_fwd.
 * stats (nullable): [ceil(B*H*W / ssp_conv_stats_tile_m(...))][Cout][2] per-tile (mean, M2) of the raw output,
 * input of ssp_bn_fwd_finalize (training-mode BatchNorm statistics, darknet.py:157).
 * workspace: ssp_conv_workspace_floats(...) floats (0 for most shapes; the 13x13 layers split their K loop over
 * several workgroups per tile and sum the partial tiles from it; so do thin layers - Cout <= 64 - whose single tile
 * column cannot fill the chip, e.g. the 1024 -> 20 head conv: those fall back to the un-split walk when no workspace
 * is passed).  The shape arguments of the two queries are those
 * of the launch (for ssp_conv_dgrad: Cin = channels of dy, Cout = channels of dx).
 * plan: tile / split choice of THIS launch, 0 = the library's shape heuristic, else
 *   tail*100000 + tile_rows*100 + ksplit*10 + ring_slots   (tile_rows 64|128, ksplit 1..9, ring_slots 3|4, or 8 =
 *   the latency form for grids of about one workgroup per CU: seven K chunks in flight, one workgroup per CU;
 *   tail 0 or 2..9 = hybrid launch: whole resident waves un-split, the last partial wave's tiles split `tail` ways);
 * a code that does not fit the shape falls back to the heuristic.  It is an argument, not state: two threads (or two
 * models) may run different plans concurrently.  The same code must be passed to the two queries.
 *   9000000 + tile_rows*100 + 10 + ring_slots (3|4|8) = Winograd F(2x2, 3x3) evaluation of a 3x3 layer (Cin % 16 == 0, Cout >= 64
 *   and % 4 == 0; conv_wino.hip): same result to ~1e-6 of its range with 16/36 of the multiplies;
 *   8000000 + the same = Winograd F(4x4, 3x3) (points 0, 1, -1, 1/2, -2): 36/144 of the multiplies, result within ~5e-6 of its
 *   range (about twice the direct fp32 kernel's own rounding error).  `wt` must then be the TRANSFORMED filter from
 *   ssp_wino_filter_transform_t with the plan's tile size (of the ssp_repack_fwd / ssp_repack_dgrad layout) and the
 *   workspace (ssp_conv_workspace_floats: (tile+2)^2 * tiles * (Cin + Cout) floats, tiles = ssp_conv_wino_tiles(B, H, W, tile))
 *   is mandatory; a Winograd code on a shape it does not fit is an error, not a fallback (the filter operand differs).
 *   7000001 = Winograd F(2x2, 3x3) with the transform domain kept ON THE CHIP (conv_wino_fused.hip; ABI 5): ONE persistent
 *   launch, no workspace (ssp_conv_workspace_floats = 0), `wt` = the same transformed filter as a 9xxxxxx plan
 *   (ssp_wino_filter_transform_t, tile 2; ssp_conv_plan_wino_tile returns 2); Cin % 32 == 0 and Cout % 32 == 0 (no
 *   lower bound of 64), 16-byte aligned in / out / bias / scale, ldin % 4 == 0, ldout % 4 == 0, every operand below
 *   2 GiB; statistics in the counted format with one group per block of four 8 x 16-pixel patches
 *   (ssp_conv_stats_tiles); accumulate, bias / affine and the fused BatchNorm-backward sums as for the other plans
 *   (bias / affine may be combined with accumulate, the BatchNorm-backward sums with neither).
 *   Valid for ssp_conv_fwd, ssp_conv_fwd_affine, ssp_conv_dgrad and ssp_conv_dgrad_bnbwd.
 *   6000000 + tile_rows*100 + ksplit*10 + 3 (tile_rows 64|128, ksplit 1..9 with >= 8 K-steps of 16 per split) = the
 *   bf16x3 fast mode of the direct kernel (conv_igemm_bf16x3.hip): same operands (`wt` from ssp_repack_fwd /
 *   ssp_repack_dgrad, fp32), same workspace, statistics format and epilogue as the direct plan of that tile and split, but
 *   every operand element is split on the chip into three bf16 terms (round to nearest even) and six of the nine term
 *   products run on the bf16 matrix cores; the three dropped ones are at most 2^-24.3 of a product.  Needs Cin % 16 == 0,
 *   Cout > 32 and % 4 == 0; a 6xxxxxx code on a launch it does not fit (ssp_conv_bf16x3_fits) is an error, never a run of
 *   the fp32 kernel.  Non-finite inputs: an Inf operand (or a finite one within half a bf16 ulp of FLT_MAX) gives NaN
 *   where the fp32 kernel gives Inf (Inf - Inf in the split).  Same four entry points; ssp_conv_plan_wino_tile returns
 *   0 and the adjoint entry points refuse the code.
 *   8000000 | 9000000 + 600000 + tile_rows*100 + 13 (tile_rows 64|128; e.g. 8612813, 9606413) = the Winograd plan
 *   8000000 | 9000000 + tile_rows*100 + 13 (its "fp32 twin") with its batched GEMM on the bf16x3 kernel: the input,
 *   output-gradient and filter transforms and both finishing passes are those of the fp32 twin, V, U and M (dM, dV) stay
 *   fp32 in the workspace, and `wt`, the workspace, the statistics format, ssp_conv_plan_wino_tile (4 | 2) and every query
 *   answer as for the fp32 twin.  Valid wherever a through-memory Winograd code is: ssp_conv_fwd, ssp_conv_fwd_affine,
 *   ssp_conv_dgrad, ssp_conv_dgrad_bnbwd, ssp_conv_dgrad_adj and ssp_conv_dgrad_adj_bnbwd (with the caller's dM or its
 *   own).  Needs R = 3, Cin % 16 == 0, Cout >= 64 and % 4 == 0 (ssp_conv_bf16x3_fits); the hundred-thousands digit of a
 *   Winograd code must be 0 or 6, the ring digit under 6 must be 3, and a 7xxxxxx code has no such form: everything else is
 *   an error and nothing is written.  Non-finite inputs as in the direct family: an Inf in V or U gives NaN.
 * stats of a Winograd plan are in the COUNTED format: ssp_conv_stats_tile_m returns 0, the buffer holds
 *   [ssp_conv_stats_tiles(...)][Cout][2] (mean, M2) pairs followed by [ssp_conv_stats_tiles(...)] pixel counts
 *   (ssp_conv_stats_floats floats in all) and ssp_bn_fwd_finalize takes tile_m = 0. */
int ssp_conv_fwd(const float* in, const float* wt, float* out, const float* bias, float* stats, int B, int H, int W,
                 int Cin, int Cout, int ldin, int ldout, int R, int accumulate, int plan, float* workspace,
                 int64_t workspace_floats, void* stream);
/* eval-mode block in one launch (darknet.py:154-167 with BatchNorm in inference mode):
 * out[p][co] = leaky(scale[co] * conv(in, wt)[p][co] + shift[co], slope); scale / shift from ssp_bn_eval_prepare
 * (either may be NULL = 1 / 0), slope = 1 for a linear block.  Same shapes, workspace and limits as ssp_conv_fwd. */
int ssp_conv_fwd_affine(const float* in, const float* wt, float* out, const float* scale, const float* shift,
                        float slope, int B, int H, int W, int Cin, int Cout, int ldin, int ldout, int R, int plan,
                        float* workspace, int64_t workspace_floats, void* stream);
int ssp_conv_stats_tile_m(int B, int H, int W, int Cin, int Cout, int R, int plan);
/* number of statistics tiles of the launch (= rows of its `stats` / of ssp_conv_dgrad_bnbwd's `partial`), and the size of
 * its `stats` buffer in floats */
int ssp_conv_stats_tiles(int B, int H, int W, int Cin, int Cout, int R, int plan);
int64_t ssp_conv_stats_floats(int B, int H, int W, int Cin, int Cout, int R, int plan);
/* tile size of a plan code: 2 or 4 for a Winograd plan, 0 otherwise */
int ssp_conv_plan_wino_tile(int plan);
/* tiles (rows of each of the (tile+2)^2 batched GEMMs) a Winograd launch of that tile size cuts B maps of H x W into:
 * B * ceil(H/tile) * ceil(W/tile), or - when that needs fewer - ceil(B/4) * ceil((2H+1)/tile) * ceil((2W+1)/tile): four
 * images tiled as one 2 x 2 mosaic with a zero row / column between them (13 x 13 at tile 4: 49 tiles per four images
 * instead of 64).  What the workspace and statistics queries are built on. */
int64_t ssp_conv_wino_tiles(int B, int H, int W, int tile);
/* U[xi][row][k] = (G g G^T)[xi], xi = 0..(tile+2)^2-1, of the 3x3 filters g[tap] = w9[row][tap][k] (rows x 9 x K floats,
 * K % 4 == 0): the filter operand of a Winograd plan of that tile size (2 or 4).  rows = Cout, K = Cin for the forward
 * layout; rows = Cin_dx, K = Cout_dy for the data-gradient layout.  U: (tile+2)^2 * rows * K floats.
 * ssp_wino_filter_transform = tile 2. */
int ssp_wino_filter_transform_t(const float* w9, float* U, int rows, int K, int tile, void* stream);
int ssp_wino_filter_transform(const float* w9, float* U, int rows, int K, void* stream);
int64_t ssp_conv_workspace_floats(int B, int H, int W, int Cin, int Cout, int R, int plan);
/* 1 when a launch of that shape runs under the bf16x3 code `plan` (6xxxxxx, or a Winograd twin 8 | 9 6xxxxx, above), 0
 * when the entry points would refuse it (bad code, Cin % 16, Cout <= 32 or % 4, R not 1 | 3, a split with fewer than 8
 * K-steps, 2^31 pixels or more; a twin: R not 3, Cin % 16, Cout < 64 or % 4, tile rows not 64 | 128, last digits not 13).  A pure host function: no GPU is touched.  Operand alignment and the workspace are checked by the launch. */
int ssp_conv_bf16x3_fits(int B, int H, int W, int Cin, int Cout, int R, int plan);

/* data gradient (autograd of nn.Conv2d, train.py:103): dx[p][ci] (+)= sum dy[p - tap][co] * w[co][ci][tap];
 * same contraction as ssp_conv_fwd with `wt` from ssp_repack_dgrad; Cout_dy = channels of dy (multiple of 4). */
int ssp_conv_dgrad(const float* dy, const float* wt, float* dx, int B, int H, int W, int Cout_dy, int Cin_dx, int lddy,
                   int lddx, int R, int accumulate, int plan, float* workspace, int64_t workspace_floats,
                   void* stream);

/* ssp_conv_dgrad (accumulate = 0) that ALSO performs the two BatchNorm-backward reductions of the block whose
 * activation gradient it writes (darknet.py:157,162 under autograd): dx is g = dL/d leaky(BN(raw)); with that block's
 * raw conv output and forward BN vectors the finishing pass of the launch leaves
 *   partial[tile][c] = (sum over the tile's pixels of dy, of dy * xhat),  dy = g * leaky'(scale*raw + shift),
 *   xhat = (raw - mean) * invstd;   tile = pixel / ssp_conv_stats_tile_m(B,H,W,Cout_dy,Cin_dx,R,plan) (Winograd plans: groups of 16 tiles),
 * i.e. what ssp_bn_act_bwd's reduce pass would re-read g and raw for; ssp_bn_act_bwd_partials finishes the block.
 * partial: partial_rows * Cin_dx * 2 floats.  A launch with ntile = ssp_conv_stats_tiles(...) <= partial_rows tiles stores row
 * `tile` plainly (deterministic); a launch with more tiles folds tile t into row t % partial_rows with fp32 atomic adds,
 * and the buffer must then be ZERO on entry (ssp_bn_act_bwd_partials with zero_after = 1 leaves it so).  Cin_dx % 4 == 0.
 * partial_rows < 0 refuses the folding for THIS call: the buffer has -partial_rows rows, and a launch with more tiles than
 * that is an error (nothing is launched, nothing written) instead of a run with atomics.  The same holds for
 * ssp_conv_dgrad_adj_bnbwd. */
int ssp_conv_dgrad_bnbwd(const float* dy, const float* wt, float* dx, int B, int H, int W, int Cout_dy, int Cin_dx,
                         int lddy, int lddx, int R, int plan, float* workspace, int64_t workspace_floats,
                         const float* raw, int ldraw, const float* scale, const float* shift, const float* mean,
                         const float* invstd, float slope, float* partial, int partial_rows, void* stream);

/* The data gradient of a 3x3 layer as the ADJOINT of the Winograd forward map (appended to ABI 5; csrc/conv_wino.hip
 * wino_dgrad_finish_kernel).  The adjoint of Y = A^T [U (.) (B^T d B)] A is, per tile,
 *   dd = B [ sum_co U_xi[co][ci] * (A dY A^T)_xi[co] ] B^T,     dX = overlap-add of the (tile+2) x (tile+2) windows dd,
 * so it contracts dM = A dY A^T - the planes the Winograd filter gradient of the same layer and tile size transforms dY
 * into anyway - with the FORWARD filter transform, channels transposed; no B^T dY B planes and no second transform of dY.
 * Same result as the data gradient entry points above with the same plan, to fp32 rounding (~5e-6 of the range at tile 4).
 *   ssp_wino_outgrad_transform_t: dM [(tile+2)^2][tiles][C] = A dY A^T of dy [B*H*W][lddy], tile 2 or 4, C % 4 == 0; timed
 *     with the Winograd data-gradient family.  Into the dM slot of a filter-gradient workspace (V | dM | dU: V
 *     [(tile+2)^2][tiles][Cin] at the head, dM [(tile+2)^2][tiles][Cout] at offset (tile+2)^2 * tiles * Cin floats, dU
 *     [(tile+2)^2][Cout][Cin] - the transform-domain filter gradient sum_t dM[t][co] * V[t][ci] that G^T dU G turns into dw,
 *     left there by the launch - at offset (tile+2)^2 * tiles * (Cin + Cout)) it feeds BOTH gradients: ssp_conv_wgrad_wino_t
 *     then takes dy == NULL (tiles 2 and 4 only; tile 12 keeps dM on the chip and refuses it).
 *   ssp_wino_filter_transform_adj_t: Ut[xi][row][k] = (G g G^T)[xi] of the UN-flipped filters out of the data-gradient
 *     layout w9d [rows = Cin_dx][tap][K = Cout_dy] (ssp_repack_dgrad, whose taps are rotated by 180 degrees): bit for bit
 *     the forward transform of the same filters packed [Cin_dx][tap][Cout_dy] without the rotation.
 *   ssp_conv_dgrad_adj / ssp_conv_dgrad_adj_bnbwd: the arguments, epilogues and limits of the two data gradient entry points
 *     above, with wt = Ut, plan = a through-memory Winograd code (8xxxxxx / 9xxxxxx: tile rows, ring slots; any other code
 *     is an error) and dM: the transformed output gradient [(tile+2)^2][tiles][Cout_dy] (dy is then not read), or NULL =
 *     transform dy here.  One batched GEMM launch dV_xi[tiles][Cin_dx] = dM_xi * Ut_xi^T and the finishing pass.
 *     workspace: ssp_conv_dgrad_adj_workspace_floats(..., own_dm = (dM == NULL)) floats, dV | (own dM); never more than
 *     ssp_conv_workspace_floats of the same plan. */
int ssp_wino_outgrad_transform_t(const float* dy, int lddy, float* dM, int B, int H, int W, int C, int tile, void* stream);
int ssp_wino_filter_transform_adj_t(const float* w9d, float* Ut, int rows, int K, int tile, void* stream);
int64_t ssp_conv_dgrad_adj_workspace_floats(int B, int H, int W, int Cout_dy, int Cin_dx, int plan, int own_dm);
int ssp_conv_dgrad_adj(const float* dy, const float* wt, float* dx, int B, int H, int W, int Cout_dy, int Cin_dx, int lddy,
                       int lddx, int R, int accumulate, int plan, float* workspace, int64_t workspace_floats,
                       const float* dM, void* stream);
int ssp_conv_dgrad_adj_bnbwd(const float* dy, const float* wt, float* dx, int B, int H, int W, int Cout_dy, int Cin_dx,
                             int lddy, int lddx, int R, int plan, float* workspace, int64_t workspace_floats,
                             const float* raw, int ldraw, const float* scale, const float* shift, const float* mean,
                             const float* invstd, float slope, float* partial, int partial_rows, const float* dM,
                             void* stream);

/* filter gradient: dw[co][tap][ci] += sum_p dy[p][co] * x[p + tap][ci]; dw is [Cout][R*R][Cin] packed and must be
 * zeroed by the caller (split reduction uses fp32 atomics). */
int ssp_conv_wgrad(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int lddy,
                   int ldx, int R, void* stream);
/* Which kernel instantiation ssp_conv_wgrad runs for these arguments under the current wgrad_variant option: a pure host
 * function of the shape (no GPU call; works on a machine without a GPU), the one the launch itself switches on.
 *   family*100000000 + ring_slots*10000000 + flags*1000000 + BMO*1000 + BNI
 *   family 1 = LDS-direct loader (csrc/conv_wgrad_dma.hip), 2 = register-staged loader, 3 = the first layer's 4-channel
 *   kernel (both csrc/conv_wgrad.hip); BMO x BNI = couts x cins of a workgroup's filter tile; ring_slots = staged pixel
 *   chunks in the LDS; flags bit 0 = fold (Cin 32: two filter taps share a 64-column tile), bit 1 = interleaved cin blocks
 *   (an experiment variant).  E.g. 130256128 = LDS-direct 256 x 128 on three slots, 141064064 = folded LDS-direct 64 x 64,
 *   230032128 = register-staged 32 x 128 (the 1024 -> 20 head), 320032004 = the 4-channel kernel.
 * 0: the launch refuses these arguments (R, Cin % 4, leading dimensions, pixel count; no pixel or no filter).  The pixel
 * split is not part of the code: it depends on the device's occupancy and is chosen inside the launch. */
int ssp_conv_wgrad_route(int B, int H, int W, int Cin, int Cout, int lddy, int ldx, int R);
/* The same filter gradient of a 3x3 layer (Cin, Cout >= 64 and % 16 == 0) evaluated in the Winograd F(tile x tile, 3x3)
 * domain, tile = 2 or 4 (csrc/conv_wino.hip): dw += the direct result to ~1e-6 (tile 2) / ~4e-6 (tile 4: the direct
 * kernel's own rounding level) of its range with 16/36 / 36/144 of the multiplies.  dw must be 16-byte
 * aligned, [Cout][3][3][Cin] floats (the ssp_repack_fwd layout), written by this launch alone while it runs;
 * workspace: ssp_conv_wgrad_wino_workspace_floats_t(...) floats.  x == NULL: the transformed input V is already at the head
 * of the workspace - left there by this layer's ssp_conv_fwd with a Winograd plan of the SAME tile size and the SAME
 * workspace buffer (both layouts start with V [(tile+2)^2][tiles][Cin]) - so the layer input is transformed once per
 * training step, not twice.  The un-suffixed names = tile 2.
 * tile = 12 (ABI 5): F(2x2) with BOTH transforms on the chip (conv_wino_wgrad_fused.hip) - each lane loads the 2 x 2
 * output-gradient pixels / the 4 x 4 input window of its (channel, tile) and transforms them in registers, waves own a
 * 32 x 32 channel block of all 16 planes over a chunk of tile rows, back-transform their own sums (G^T dU G is linear) and
 * add nine taps per channel pair into dw with fp32 atomics; Cin % 32 == 0 and Cout % 32 == 0 (from 32 channels up), x must
 * be given (no shared transformed input), NO workspace (the query returns 0; a workspace argument is ignored). */
int64_t ssp_conv_wgrad_wino_workspace_floats_t(int B, int H, int W, int Cin, int Cout, int tile);
/* The input transform alone: V[(tile+2)^2][tiles][C] = B^T d B of x [B*H*W][ldx] - for a layer whose FORWARD does not run in
 * the Winograd domain (or runs another tile size) while its filter gradient does: the engine queues it on the second stream
 * during the forward pass, into the head of that layer's filter-gradient workspace, and calls ssp_conv_wgrad_wino_t with
 * x == NULL (an HBM-bound pass under the MFMA-bound forward launches instead of inside the backward pass, where both
 * streams are busy). */
int ssp_wino_input_transform_t(const float* x, int ldx, float* V, int B, int H, int W, int C, int tile, void* stream);
int ssp_conv_wgrad_wino_t(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int lddy,
                          int ldx, int tile, float* workspace, int64_t workspace_floats, void* stream);
int64_t ssp_conv_wgrad_wino_workspace_floats(int B, int H, int W, int Cin, int Cout);
int ssp_conv_wgrad_wino(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int lddy,
                        int ldx, float* workspace, int64_t workspace_floats, void* stream);

/* ---- ordered filter gradients (appended to ABI 5; csrc/wgrad_ordered.h): the same sums, bitwise reproducible ------------
 * ssp_conv_wgrad, ssp_conv_s2_wgrad and a split ssp_conv_wgrad_wino_t launch add their per-pixel-range partial sums into
 * the gradient with fp32 atomics, in the order the hardware retires them: two runs on the same operands differ in the last
 * bits.  The entry points below run the SAME main loops (an epilogue argument of the same kernels) but every (filter tile,
 * pixel range) workgroup stores its partial tile plainly into slab `range` of a caller-owned workspace
 * [nsplit][Cout][R*R][Cin], and a finishing kernel adds the slabs of each element in the order 0 .. nsplit-1 (in float64,
 * rounded once; flags bit 0 = in fp32) and performs the one dw += of the launch.  dw need NOT be zero: the launch
 * accumulates onto it, exactly once per element.  Same operands, layouts and limits as the atomic entry points; stride =
 * 1 (every route family of ssp_conv_wgrad_route) or 2 (H, W = the INPUT map, as ssp_conv_s2_wgrad).
 *   split: the number of pixel ranges - an ARGUMENT, not process state (ssp_set_option is not consulted: the routes are
 *     those of wgrad_variant 0): 0 = the library's choice, a pure host function of the shape built on a fixed model of the
 *     chip (256 CUs, workgroups per CU from the kernel's LDS ring) instead of the occupancy the runtime reports, so it is
 *     the same in every process; > 0 = that many ranges, CLAMPED to one staged chunk (16 pixels; 32 or 64 for thin tiles,
 *     64 for the 4-channel kernel) per range, and - ranges are whole chunks - reduced to the count the rounded range
 *     length gives (7 ranges asked of 338 pixels in chunks of 16 = 6 ranges of 64).  ssp_conv_wgrad_ordered_split returns
 *     the count a launch with these arguments runs, ssp_conv_wgrad_ordered_workspace_floats = that count * Cout * R*R * Cin;
 *     both are pure host functions (no GPU is touched) and return 0 where ssp_conv_wgrad_route returns 0 (a refused shape).
 *   workspace: 16-byte aligned, at least the query's floats; every float of the first nsplit slabs is written, nothing
 *     past them.  Two launches must not share a workspace concurrently.
 * Results with different splits agree to fp32 rounding, not bit for bit: the split is part of what "the same launch" means. */
int ssp_conv_wgrad_ordered_split(int B, int H, int W, int Cin, int Cout, int lddy, int ldx, int R, int stride, int split);
int64_t ssp_conv_wgrad_ordered_workspace_floats(int B, int H, int W, int Cin, int Cout, int lddy, int ldx, int R, int stride,
                                                int split);
int ssp_conv_wgrad_ordered(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int lddy, int ldx,
                           int R, int stride, int split, int flags, float* workspace, int64_t workspace_floats, void* stream);
/* The Winograd filter gradient (tiles 2 and 4; tile 12 adds with atomics on the chip and is refused) in the ordered form:
 * the batched dU launch writes one transform-domain gradient [(tile+2)^2][Cout][Cin] per pixel (= tile row) range and
 * the finishing kernel sums them in order before the back-transform G^T dU G.  split as above (ranges of 16 tile rows);
 * workspace = ssp_conv_wgrad_wino_workspace_floats_t + (nsplit - 1) * (tile+2)^2 * Cout * Cin floats, laid out V | dM |
 * dU slab 0 | ... | slab nsplit-1, so x == NULL / dy == NULL share V and dM as with ssp_conv_wgrad_wino_t.  0 = refused. */
int ssp_conv_wgrad_wino_ordered_split(int B, int H, int W, int Cin, int Cout, int tile, int split);
int64_t ssp_conv_wgrad_wino_ordered_workspace_floats(int B, int H, int W, int Cin, int Cout, int tile, int split);
int ssp_conv_wgrad_wino_ordered(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int lddy,
                                int ldx, int tile, int split, float* workspace, int64_t workspace_floats, void* stream);
/* ssp_conv_s2_dgrad with the tap split of small grids refused for THIS call: one thread per pixel on every grid, no atomics,
 * the same bits from run to run (slower on grids under 512 workgroups: the longest workgroup contracts four taps). */
int ssp_conv_s2_dgrad_ordered(const float* dy, const float* wt, float* dx, int B, int H, int W, int Cout_dy, int Cin_dx, int lddy,
                              int lddx, int R, int accumulate, void* stream);

/* ---- stride-2 convolution (appended to ABI 5; csrc/conv_strided.hip): nn.Conv2d(Cin, Cout, R, stride 2, padding R/2) at
 * darknet.py:156,160 with stride = 2, R = 1 or 3, exact fp32 on the matrix cores, any position of a net but the first
 * block.  H, W are ALWAYS the sizes of the block's INPUT map; the output map is Ho x Wo, Ho = (H + 2*(R/2) - R)/2 + 1 (odd
 * and even H both), input row of output row yo and tap r = 2*yo + r - R/2, zero outside the map.  No plan codes, no
 * workspace.  Limits of all three: Cin % 4 == 0 (data gradient: Cout_dy % 4 == 0, the padded width of dy), leading dimensions
 * % 4 == 0 and >= the channel counts, 16-byte aligned operands, B*H*W < 2^31; anything else is SSP_ERR_ARG with a message
 * and nothing is launched.
 *   forward: out[po][co] (+)= sum_{tap,ci} in[gather(po, tap)][ci] * wt[co][tap][ci] (+ bias[co]) over the B*Ho*Wo output
 *     pixels; wt from ssp_repack_fwd.  stats (nullable, not with accumulate): per-tile (mean, M2) pairs of the raw output,
 *     [ssp_conv_s2_stats_tiles][Cout][2], tiles of ssp_conv_s2_stats_tile_m output pixels (64 or 128, the last tile
 *     partial): ssp_bn_fwd_finalize takes them with that tile_m and M = B*Ho*Wo.  The _affine form is the eval-mode block
 *     in one launch, out = leaky(scale[co] * conv + shift[co], slope), as ssp_conv_fwd_affine.
 *   data gradient: dx[pi][ci] (+)= sum over the (output pixel, tap) pairs that read input pixel pi of dy[po][co] *
 *     w[co][ci][tap]; wt from ssp_repack_dgrad (Coutp = Cout_dy).  One launch, decomposed by the parity of pi = (yi, xi):
 *     at R = 3 an even coordinate is reached by tap 1 only, an odd one by taps 0 and 2, so the four classes contract 1, 2,
 *     2 and 4 taps (9/4 per pixel on average, never nine masked ones); at R = 1 only (even, even) pixels receive anything,
 *     the others are written as zeros (accumulate = 0) or left untouched (accumulate = 1).  Every pixel of dx's Cin_dx
 *     columns is written by exactly one thread (deterministic) - except on grids of fewer than 512 workgroups (3x3), which
 *     hand every (class, tap) pair to workgroups of its own and sum a pixel's taps with fp32 atomic adds (dx zeroed first
 *     when accumulate = 0): the same sum in an order that may differ from run to run.  Columns >= Cin_dx of a wider lddx are
 *     not touched.
 *   filter gradient: dw[co][tap][ci] += sum_po dy[po][co] * in[gather(po, tap)][ci], [Cout][R*R][Cin] packed, zeroed by
 *     the caller (the pixel reduction is split over workgroups and summed with fp32 atomics), as ssp_conv_wgrad. */
int ssp_conv_s2_fwd(const float* in, const float* wt, float* out, const float* bias, float* stats, int B, int H, int W,
                    int Cin, int Cout, int ldin, int ldout, int R, int accumulate, void* stream);
int ssp_conv_s2_fwd_affine(const float* in, const float* wt, float* out, const float* scale, const float* shift, float slope,
                           int B, int H, int W, int Cin, int Cout, int ldin, int ldout, int R, void* stream);
int ssp_conv_s2_stats_tile_m(int B, int H, int W, int Cin, int Cout, int R);
int ssp_conv_s2_stats_tiles(int B, int H, int W, int Cin, int Cout, int R);
int ssp_conv_s2_dgrad(const float* dy, const float* wt, float* dx, int B, int H, int W, int Cout_dy, int Cin_dx, int lddy,
                      int lddx, int R, int accumulate, void* stream);
int ssp_conv_s2_wgrad(const float* dy, const float* x, float* dw, int B, int H, int W, int Cin, int Cout, int lddy, int ldx,
                      int R, void* stream);

/* ---- BatchNorm2d(eps) + LeakyReLU(slope) (+ 2x2/2 max-pool): darknet.py:157,162,172 ------------------------- */
/* stats: `ntile` per-tile (mean, M2) pairs per channel from a conv launch; tile_m = its ssp_conv_stats_tile_m (rows per
 * tile; the last tile holds M - (ntile-1)*tile_m), or 0 = counted format (the tiles' pixel counts follow the pairs) */
int ssp_bn_fwd_finalize(const float* stats, int ntile, int tile_m, int M, int C, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                        float* mean, float* invstd, float* scale, float* shift, void* stream);
int ssp_bn_eval_prepare(int C, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float* mean, float* invstd, float* scale, float* shift,
                        void* stream);
/* out = [maxpool2x2](leaky(scale*x + shift)); H, W are the un-pooled sizes */
int ssp_bn_act_fwd(const float* x, int ldx, float* out, int ldo, const float* scale, const float* shift, int C, int B,
                   int H, int W, int pool, float slope, void* stream);
/* g = gradient wrt the (pooled) activation; dx (may alias x) = gradient wrt the raw conv output;
 * partial: workspace of ssp_bn_bwd_blocks()*C*2 floats; c1, c2: C floats each (reduce -> fp64 finalize -> apply).
 * partial == NULL selects the single-pass form: dgamma / dbeta must be ZERO on entry and 16-byte aligned, the reduce
 * pass accumulates them with fp32 atomics and the apply pass reads them (no finalize launch; c1 / c2 unused). */
int ssp_bn_bwd_blocks(void);
int ssp_bn_act_bwd(const float* x, int ldx, const float* g, int ldg, float* dx, int lddx, const float* scale,
                   const float* shift, const float* mean, const float* invstd, int C, int B, int H, int W, int pool,
                   float slope, int training, float* partial, float* dgamma, float* dbeta, float* c1, float* c2,
                   void* stream);
/* un-pooled block whose reductions came out of ssp_conv_dgrad_bnbwd: fp64 sum of the `npartial` per-tile pairs ->
 * dgamma / dbeta (and c1 / c2), then dx (may alias x) = scale * (dy - c1 - xhat * c2) */
int ssp_bn_act_bwd_partials(const float* x, int ldx, const float* g, int ldg, float* dx, int lddx, const float* scale,
                            const float* shift, const float* mean, const float* invstd, int C, int B, int H, int W,
                            float slope, int training, float* partial, int npartial, int zero_after, float* dgamma,
                            float* dbeta, float* c1, float* c2, void* stream);
/* a BatchNorm block in inference mode whose gamma / beta want no gradient is the affine map leaky(scale*x + shift)
 * [+ max-pool]: its backward is the apply pass alone, dx (may alias x) = scale * leaky'(.) * pool-scatter(g); no
 * reduction, no finalize.  scale / shift / mean / invstd from ssp_bn_eval_prepare; shapes and limits as ssp_bn_act_bwd. */
int ssp_bn_act_bwd_affine(const float* x, int ldx, const float* g, int ldg, float* dx, int lddx, const float* scale,
                          const float* shift, const float* mean, const float* invstd, int C, int B, int H, int W, int pool,
                          float slope, void* stream);
/* just the fp64 finalize of `npartial` rows of (sum dy, sum dy * xhat) pairs -> dgamma, dbeta, c1 = mean(dy),
 * c2 = mean(dy * xhat) over npix pixels (c1 = c2 = 0 when training == 0) */
int ssp_bn_bwd_finalize(float* partial, int npartial, int C, int64_t npix, int training, int zero_after, float* dgamma,
                        float* dbeta, float* c1, float* c2, void* stream);
/* out[c] = sum_p g[p][c]  (bias gradient of the linear head conv) */
int ssp_colsum(const float* g, int ldg, int64_t M, int C, float* out, void* stream);

/* ---- first block: conv 3x3 (image, Cin padded to 4 -> 32) + BatchNorm + leaky + 2x2/2 max-pool, training mode, with
 * the convolution RECOMPUTED by every pass instead of stored (darknet.py:154-176 on the 416 x 416 input and its autograd
 * backward; SURVEY.md section 7: the 22 MB-per-image map is the largest tensor of the net, its conv has K = 27).
 * x: [B*H*W][4] (channel 3 zero), wt: ssp_repack_fwd(conv.weight, Cinp = 4) = [32][9][4]; H even, W % 16 == 0.
 *   fwd_stats : stats[ssp_first_groups(B,H,W)][32][2] = per-group (mean, M2) of the raw conv output; feed
 *               ssp_bn_fwd_finalize(stats, groups, ssp_first_tile_pixels(), B*H*W, 32, ...)
 *   fwd_apply : out[pooled pixel][0..32) = maxpool2x2(leaky(scale * conv + shift))
 *   bwd_reduce: partial[groups][32][2] = (sum dy, sum dy * xhat) from g = dL/d out (pool arg-max = first maximum in
 *               window scan order, as ATen); feed ssp_bn_bwd_finalize
 *   bwd_wgrad : dw[32][9][4] = filter gradient (dx formed in registers from g, the recomputed conv and c1 / c2; the padding
 *               channel written as zero).  Two launches: every workgroup leaves its partial gradient in `workspace`
 *               (ssp_first_wgrad_workspace_floats(B,H,W) floats), a second kernel sums the workgroups in float64 - the
 *               gradient is a sum of terms that cancel ~1e3 : 1, and deterministic this way (ABI 4; ABI 3 accumulated
 *               with fp32 atomics into a zeroed dw)  */
int ssp_first_tile_pixels(void);
int ssp_first_groups(int B, int H, int W);
int ssp_first_fwd_stats(const float* x, const float* wt, float* stats, int B, int H, int W, void* stream);
int ssp_first_fwd_apply(const float* x, const float* wt, const float* scale, const float* shift, float slope, float* out,
                        int ldo, int B, int H, int W, void* stream);
/* the raw conv output itself, [B*H*W][ldraw], by the same instruction sequence the four passes use (bit-identical
 * values): for checkers that need the pool / leaky decisions of the fused path - the training path never calls it */
int ssp_first_conv_raw(const float* x, const float* wt, float* raw, int ldraw, int B, int H, int W, void* stream);
int ssp_first_bwd_reduce(const float* x, const float* wt, const float* g, int ldg, const float* scale, const float* shift,
                         const float* mean, const float* invstd, float slope, float* partial, int B, int H, int W,
                         void* stream);
int ssp_first_bwd_wgrad(const float* x, const float* wt, const float* g, int ldg, const float* scale, const float* shift,
                        const float* mean, const float* invstd, const float* c1, const float* c2, float slope, float* dw,
                        float* workspace, int64_t workspace_floats, int B, int H, int W, void* stream);
int64_t ssp_first_wgrad_workspace_floats(int B, int H, int W);
/*   bwd_dgrad : dx[B*H*W][4] = dL/dx, the gradient of the block's input: conv_transpose3x3(dy_raw, w) with dy_raw the
 *               BatchNorm-backward of leaky'(pool-scatter(g)) (c1 / c2 from bwd_reduce + ssp_bn_bwd_finalize, as
 *               bwd_wgrad); the padding channel is written as zero.  The full-resolution map and its gradient are
 *               recomputed per tile (one-window border) and never stored; every element is written once by one thread,
 *               no atomics: two calls give bitwise-equal results.  dx 16-byte aligned. */
int ssp_first_bwd_dgrad(const float* x, const float* wt, const float* g, int ldg, const float* scale, const float* shift,
                        const float* mean, const float* invstd, const float* c1, const float* c2, float slope, float* dx,
                        int B, int H, int W, void* stream);

/* ---- optimizer ------------------------------------------------------------------ */
/* One torch.optim.SGD step (train.py:388,106) over a contiguous fp32 range of n values, in place:
 *   d = grad + weight_decay*param;  buf = first_step ? d : momentum*buf + (1-dampening)*d;
 *   param -= lr * (nesterov ? d + momentum*buf : buf)        (momentum == 0: param -= lr*d, momentum_buf may be NULL)
 * All three pointers 16-byte aligned. */
int ssp_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                 float dampening, float weight_decay, int nesterov, int first_step, void* stream);
#define SSP_SGD_MAX_TUPLES 16
/* The same update over a TABLE of segments in one launch (parameter groups with different hyper-parameters, an optimizer
 * that holds part of a model): segment s is table[s] = {param offset, grad offset, momentum offset, length, tuple index}
 * (five int64, offsets and lengths in floats; offsets multiples of 4, lengths arbitrary, nseg >= 1), tuple t is
 * hyper[t] = {lr, momentum, dampening, weight_decay, nesterov (0 / 1), first_step (0 / 1)} (six floats, at most
 * SSP_SGD_MAX_TUPLES = 16 of them: they travel by value with the launch, so a changed lr needs no upload).
 * Every element is updated exactly as by ssp_sgd_step on its segment (bit-identical).  table_dev is the device-resident
 * table the kernel reads, table_host the caller's host copy of the same nseg rows: before anything is launched every row
 * is checked against the three buffer lengths (param_floats, grad_floats, momentum_floats; momentum_buf may be NULL with
 * momentum_floats = 0 when no tuple has momentum) - an offset that is negative, misaligned or, with its length, past the
 * end of a buffer, a length < 1, a tuple index outside [0, ntuple) or a bad tuple is SSP_ERR_ARG and nothing runs.
 * Segments must not overlap in param / momentum_buf (not checked).  All pointers 16-byte aligned. */
int ssp_sgd_step_table(float* param, const float* grad, float* momentum_buf, int64_t param_floats, int64_t grad_floats,
                       int64_t momentum_floats, const int64_t* table_dev, const int64_t* table_host, int nseg,
                       const float* hyper, int ntuple, void* stream);

/* One torch.optim.Adam / AdamW step over a contiguous fp32 range of n values, in place.  param, grad, exp_avg (m),
 * exp_avg_sq (v) and max_exp_avg_sq (vmax; non-NULL iff amsgrad) are 16-byte aligned.  Per element, in the order of
 * torch/optim/adam.py's single-tensor path:
 *   decoupled (AdamW):  p = p * (1 - lr*weight_decay)        else (Adam):  g = fma(weight_decay, p, g)
 *                       (both only when weight_decay != 0)
 *   m = fma(1 - beta1, g - m, m)
 *   v = fma((1 - beta2)*g, g, beta2*v)
 *   amsgrad:  vmax = max(vmax, v) (a NaN propagates);  d = vmax          else:  d = v
 *   denom = sqrt(d) / bc2_sqrt + eps
 *   p = p + (-step_size * m) / denom          (= p - step_size * (m / denom); product, quotient and sum each rounded,
 *                                              as torch's addcdiv_ does)
 * Every operation written here is rounded once to fp32 (nothing else is contracted); sqrt and `/` are the IEEE correctly
 * rounded ones.  The hyper-parameters travel by value as doubles; 1 - lr*weight_decay, 1 - beta1, 1 - beta2 and
 * -step_size are formed in double and rounded to fp32 once, as are the others.  The caller owns the step count t and
 * passes step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t); the kernel never sees t.
 * SSP_ERR_ARG before any launch: a NULL param / grad / m / v or n < 1, a misaligned pointer, amsgrad without vmax,
 * beta1 or beta2 outside [0, 1), eps <= 0 (also when it rounds to 0 in fp32), lr or weight_decay negative or not
 * finite, a step_size that is not finite, a bc2_sqrt that is not finite or <= 0. */
int ssp_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                  double lr, double beta1, double beta2, double eps, double weight_decay, double step_size,
                  double bc2_sqrt, int decoupled, int amsgrad, void* stream);
#define SSP_ADAM_MAX_TUPLES 16
/* The same update over a TABLE of segments in one launch, as ssp_sgd_step_table: segment s is table[s] = {param offset,
 * grad offset, state offset, length, tuple index} (five int64, in floats; offsets multiples of 4, lengths arbitrary); the
 * state offset serves exp_avg, exp_avg_sq and max_exp_avg_sq, which share one layout of state_floats floats.  Tuple t is
 * hyper[t] = {lr, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt, decoupled (0 / 1), amsgrad (0 / 1)} (nine
 * doubles, at most SSP_ADAM_MAX_TUPLES = 16: they travel by value with the launch, so the per-batch lr rewrite and the
 * per-step bias corrections upload nothing).  Every element is updated exactly as by ssp_adam_step on its segment
 * (bit-identical).  Before anything is launched every tuple is checked as above and every row of table_host against the
 * buffer lengths: a negative or misaligned offset, a segment that ends outside a buffer, a length < 1 or a tuple index
 * outside [0, ntuple) is SSP_ERR_ARG and nothing runs.  Work is dealt in 4096-float chunks round-robin over at most 2048
 * workgroups.  Segments must not overlap in param / state (not checked). */
int ssp_adam_step_table(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                        int64_t param_floats, int64_t grad_floats, int64_t state_floats, const int64_t* table_dev,
                        const int64_t* table_host, int nseg, const double* hyper, int ntuple, void* stream);
/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) as two launches on one stream, with no
 * host synchronisation and no atomics: the same inputs give the same bits on every run.  Both walk the GRADIENT segments
 * of a table as above (fields 1 and 3 of a row: grad offset, length; the other fields are not read, and the floats
 * between segments are never read or written); table_dev = table_host = NULL with nseg = 1 means the one range
 * [0, grad_floats).
 * ssp_grad_sumsq_table: every lane adds the squares of its elements in double (an fp32 square is exact in double), the
 *   256 lane sums of a workgroup are added in LDS by a fixed halving tree, and workgroup b writes partial[b].
 *   *npartial = the workgroups launched = min(chunks, 2048, partial_capacity).
 * ssp_grad_scale_table: every workgroup adds partial[0 .. npartial) in one fixed order (lane t adds t, t + 256, ...
 *   ascending, then the same tree; npartial <= 65536, so several sumsq launches may fill one array), then
 *   norm = sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)) in double (a NaN propagates), coef rounded once to fp32,
 *   and multiplies its chunks of grad by coef in place (one rounding per element; nothing is written when the rounded
 *   coef is exactly 1).  Workgroup 0 writes result[0] = (float)norm, result[1] = coef.
 * SSP_ERR_ARG before any launch: NULL / misaligned buffers, a bad row (as above), no room for partials, npartial outside
 * [1, 65536], max_norm negative or NaN. */
int ssp_grad_sumsq_table(const float* grad, int64_t grad_floats, const int64_t* table_dev, const int64_t* table_host,
                         int nseg, double* partial, int partial_capacity, int* npartial, void* stream);
int ssp_grad_scale_table(float* grad, int64_t grad_floats, const int64_t* table_dev, const int64_t* table_host, int nseg,
                         const double* partial, int npartial, double max_norm, float* result, void* stream);

/* ---- layout / index kernels -------------------------------------------------------------------------------- */
int ssp_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, int Cpad, int ld, void* stream);
int ssp_nhwc_to_nchw(const float* src, float* dst, int B, int C, int H, int W, int ld, void* stream);
/* uint8 (B,H,W,C) image bytes -> fp32 [B*H*W][ld], value/255 as transforms.ToTensor (dataset.py:113-131); channels
 * [C,Cpad) = 0.  SURVEY.md section 8(f) row 3: the byte image is uploaded instead of the fp32 NCHW tensor. */
int ssp_u8hwc_to_nhwc(const unsigned char* src, float* dst, int B, int H, int W, int C, int Cpad, int ld, void* stream);
/* ---- training-time augmentation (second half): image.py:14-31,46-76,111-128 ----------
 * What the reference does per sample with Pillow on the host - bg.resize + mask composite, jitter crop (zero fill) +
 * resize to the network shape, HSV jitter through Image.point tables - as batched launches, byte-exact with Pillow.
 * A resize is two passes (horizontal over the rows the vertical pass needs, 8-bit intermediate, then vertical) of a
 * per-output-index FIR with Pillow's 22-bit fixed-point bicubic coefficients; the coefficient rows come from the caller
 * (singleshotpose_amd/image.py computes them in double, as ImagingResample's precompute_coeffs does).
 * One descriptor per sample, an array of them in DEVICE memory; u8 images are (rows, cols, 3) with a byte pitch. */
typedef struct SspResampleDesc {
  const void* src;     /* pass 0: source image (src_h x src_w); pass 1: the horizontal pass's output (src_h rows) */
  void* dst;           /* dst_h x dst_w */
  const void* bounds;  /* int32 [n_out][2] = (first input index, taps) of this pass's axis */
  const void* kk;      /* int32 [n_out][ksize] fixed-point coefficients */
  const void* img;     /* epilogue 1: foreground image, dst-sized */
  const void* mask;    /* epilogue 1: mask, dst-sized: channel value >= 128 keeps the foreground (image.py:121-125) */
  const void* lut;     /* epilogue 2: 768 bytes = H, S, V tables of image.py:14-31 */
  int src_w, src_h, src_pitch;
  int x0, y0;          /* pass 0: logical input pixel (Y, X) is source pixel (Y + y0, X + x0); outside the source = 0 (crop) */
  int row0;            /* first logical input row the vertical pass needs (pass 0 writes rows row0 ...; pass 1 reads them) */
  int dst_w, dst_h, dst_pitch;
  int ksize, img_pitch, reserved;
} SspResampleDesc;
/* pass 0 = horizontal (epilogue 0 or 3), 1 = vertical (epilogue 0, 1, 2 or 4); epilogue 0 = store, 1 = composite with
 * img / mask, 2 = distort_image (RGB -> HSV -> tables -> RGB), 3 = masked source: the taps read src * round(mask / 255)
 * per channel, `mask` laid out as `src` (mask_background of image_multi.py; mask == NULL reads src plainly),
 * 4 = moved destination: the result pixel (y, x) is stored at ((y + y0) % dst_h, (x + x0) % dst_w), mirrored in x
 * when `reserved` != 0 (ImageChops.offset then FLIP_LEFT_RIGHT; 0 <= x0 < dst_w, 0 <= y0 < dst_h).
 * max_dst_pixels = the largest dst_w * dst_h of the batch. */
int ssp_resample_u8(const SspResampleDesc* descs_dev, int count, int pass, int epilogue, int max_dst_pixels, void* stream);
/* The layer compositor of the multi-object augmentation (image_multi.py augment_objects + change_background): all layers
 * are dense uint8 arrays of `nbytes` bytes (network shape x 3), 16-byte aligned.  Per byte, pos(m) = m >= 128:
 *   total = pos(scene_mask) ? scene : 0, tmask = scene_mask;
 *   for k < nobj: tmask = min(255, obj_mask[k] + (pos(obj_mask[k]) ? 0 : tmask)), total = pos(obj_mask[k]) ? obj[k] : total;
 *   total = pos(scene_mask) ? scene : total;  out = pos(tmask) ? total : bg.
 * One descriptor per sample, an array of them in DEVICE memory. */
#define SSP_COMPOSITE_MAX_OBJS 8
typedef struct SspCompositeDesc {
  const void* scene;
  const void* scene_mask;
  const void* bg;
  void* out;
  const void* obj[SSP_COMPOSITE_MAX_OBJS];
  const void* obj_mask[SSP_COMPOSITE_MAX_OBJS];
  long long nbytes;
  int nobj, reserved;
} SspCompositeDesc;
int ssp_composite_u8(const SspCompositeDesc* descs_dev, int count, long long max_bytes, void* stream);
/* distort_image alone on npix packed RGB pixels (mode 0, lut = 768 bytes); modes 1 / 2 = RGB -> HSV / HSV -> RGB only
 * (Image.convert), which is how the tests pin both conversions over all 2^24 inputs. */
int ssp_distort_u8(const unsigned char* rgb, unsigned char* out, int64_t npix, const unsigned char* lut, int mode, void* stream);
/* conv.weight (Cout,Cin,R,R) (cfg.py:157,175) -> [Cout][R*R][Cinp] */
int ssp_repack_fwd(const float* w, float* out, int Cout, int Cin, int Cinp, int R, void* stream);
/* conv.weight -> [Cin][R*R][Coutp], taps flipped */
int ssp_repack_dgrad(const float* w, float* out, int Cout, int Cin, int Coutp, int R, void* stream);
/* same operand from filters stored channels-last, [Cout][R*R][Cin] (a torch.channels_last conv.weight): that layout IS
 * the forward operand and the layout ssp_conv_wgrad accumulates, so such parameters need no other repack */
int ssp_repack_dgrad_packed(const float* wp, float* out, int Cout, int Cin, int Coutp, int R, void* stream);
/* packed gradient [Cout][R*R][Cinp] -> (Cout,Cin,R,R) */
int ssp_unpack_grad(const float* dwp, float* grad, int Cout, int Cin, int Cinp, int R, void* stream);
/* Reorg(2) (darknet.py:16-35) on NHWC: dst[b,y/2,x/2,((y&1)*2+(x&1))*C+c] = src[b,y,x,c]; backward = inverse */
int ssp_reorg(const float* src, int lds, float* dst, int ldd, int C, int B, int H, int W, int backward,
              int accumulate, void* stream);
/* route (darknet.py:96-106): dst[p][0..C) (+)= src[p][0..C) */
int ssp_copy_channels(const float* src, int lds, float* dst, int ldd, int C, int64_t M, int accumulate, void* stream);
/* nn.MaxPool2d(2,2) (darknet.py:172) standalone */
int ssp_maxpool_fwd(const float* x, int ldx, float* out, int ldo, int C, int B, int H, int W, void* stream);
int ssp_maxpool_bwd(const float* x, int ldx, const float* g, int ldg, float* dx, int lddx, int C, int B, int H, int W,
                    int accumulate, void* stream);

/* ---- generic Darknet blocks (csrc/generic_blocks.hip): fp32 NHWC [pixels][ld] maps, ld % 4 == 0; backward passes write
 * (accumulate = 0) or add (accumulate = 1) into the input gradient ------------------------------------------------ */
/* MaxPoolStride1 (darknet.py:8-14, chosen at :168-176 when stride == 1): out = max_pool2d(pad(x, (0,1,0,1), 'replicate'),
 * 2, stride=1), H x W -> H x W (the cfg's size is ignored); C % 4 == 0.  Backward recomputes the winner from x (first
 * maximum in row-then-column order); a winner on the pad folds onto the edge pixel */
int ssp_maxpool_s1_fwd(const float* x, int ldx, float* out, int ldo, int C, int B, int H, int W, void* stream);
int ssp_maxpool_s1_bwd(const float* x, int ldx, const float* g, int ldg, float* dx, int lddx, int C, int B, int H, int W,
                       int accumulate, void* stream);
/* shortcut (darknet.py:107-118, :210-214): out = act(a + b) over M pixels, slope 1 = linear, 0.1 = leaky, 0 = relu; C % 4 == 0.
 * Backward: g' = g * act'(out) (from out > 0, as in-place leaky_relu / relu); da (+)= g', db (+)= g'.  da == db (from = -1:
 * both summands are one map) adds 2 g' and needs ldda == lddb, acc_a == acc_b */
int ssp_shortcut_fwd(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int C, int64_t M, float slope,
                     void* stream);
int ssp_shortcut_bwd(const float* g, int ldg, const float* out, int ldo, float* da, int ldda, int acc_a, float* db, int lddb,
                     int acc_b, int C, int64_t M, float slope, void* stream);
/* GlobalAvgPool2d (darknet.py:37-47, :177-180): (B,H,W,C) -> out[b][c] (B rows of ldo), fixed summation order
 * (deterministic); backward dx[b][p][c] (+)= g[b][c] / (H * W); C % 4 == 0 */
int ssp_avgpool_fwd(const float* x, int ldx, float* out, int ldo, int C, int B, int H, int W, void* stream);
int ssp_avgpool_bwd(const float* g, int ldg, float* dx, int lddx, int C, int B, int H, int W, int accumulate, void* stream);
/* nn.Softmax() (darknet.py:181-184; implicit dim = 1): softmax over the C channels of each of M rows (B samples of a 2-D
 * input or B*H*W pixels of an NHWC map), row maximum subtracted before exp; channels >= C are neither read nor written.
 * Backward: dx (+)= y * (g - sum_c g * y) */
int ssp_softmax_fwd(const float* x, int ldx, float* y, int ldy, int C, int64_t M, void* stream);
int ssp_softmax_bwd(const float* y, int ldy, const float* g, int ldg, float* dx, int lddx, int C, int64_t M, int accumulate,
                    void* stream);
/* [upsample] stride=N (csrc/upsample.hip; appended to ABI 5): nearest-neighbour replication, dst[b,y,x,c] =
 * src[b,y/N,x/N,c] - F.interpolate(scale_factor=N, mode='nearest').  H x W is the SOURCE (coarse) map in both calls;
 * C % 4 == 0 (the padded count of a padded map); every stride a multiple of 4 and >= C; pointers 16-byte aligned;
 * 1 <= stride <= 8; B * H * W * stride^2 < 2^31 - anything else is SSP_ERR_ARG and nothing is launched.  Only columns
 * [0, C) of a row are read or written, so either side may be a channel slice of a wider buffer.
 * Backward: dsrc[b,y,x,c] (=|+=) sum of the N x N window of g, taken row-major with sequential fp32 adds (s = g00;
 * s += g01; ...), then dsrc = accumulate ? dsrc + s : s; one thread per element, no atomics: the same bits every run */
int ssp_upsample_fwd(const float* src, int lds, float* dst, int ldd, int C, int B, int H, int W, int stride, void* stream);
int ssp_upsample_bwd(const float* g, int ldg, float* dsrc, int ldds, int C, int B, int H, int W, int stride,
                     int accumulate, void* stream);

/* ---- depthwise 3x3 convolution (appended to ABI 5; csrc/conv_depthwise.hip): nn.Conv2d(C, C, 3, stride, padding 1,
 * groups = C) at darknet.py:156,160 - a Darknet [convolutional] block with groups = channels = filters - stride 1 or 2, any
 * position of a net but the first block.  fp32 NHWC maps [pixels][ld], channels fastest; a lane owns one channel quad, every
 * access is 16 bytes; no matrix cores.  Only columns [0, C) of a row are read or written on either side, so a map may be a
 * channel slice of a wider buffer (ld > C, the pointer offset by a multiple of 4 floats).  H, W are ALWAYS the sizes of the
 * block's INPUT map (the data gradient's dx, the filter gradient's x); the output map is Ho x Wo, Ho = (H + 2 - 3)/stride + 1,
 * Wo likewise; input pixel of output pixel (yo, xo) and tap (r, t) = (stride*yo + r - 1, stride*xo + t - 1), tap = 3 r + t,
 * zero outside the map - a tap never reads a neighbouring row's or image's pixel.
 * The filter operand `w` is the parameter's own memory, (C, 1, 3, 3) contiguous: w[c*9 + tap]; the filter gradient `dw` has
 * the same layout (the parameter's range of the flat gradient buffer).  No repacked operand, no plan code, no state.
 * Limits of all entry points: C > 0 and C % 4 == 0; leading dimensions % 4 == 0 and >= C; operands (bias / scale / shift /
 * stats / workspace included, where given) 16-byte aligned; stride 1 or 2; B*H*W < 2^31; workspace_floats >= the query -
 * anything else is SSP_ERR_ARG with a message and nothing is launched (the queries return 0 on bad sizes).
 *   forward: out[po][c] = sum_tap in[gather(po, tap)][c] * w[c*9 + tap] (+ bias[c]): the nine products are added with fp32
 *     fused multiply-adds in ascending tap order from 0, the bias last.  Every input value is loaded once per thread and
 *     serves all taps of a strip of four output pixels of one row.  The _affine form is the eval-mode block in one launch,
 *     out = leaky(scale[c] * conv + shift[c], slope), scale / shift nullable (= 1 / 0), slope = 1 for a linear block.
 *     stats (nullable): per-tile (mean, M2) pairs of the stored output in the COUNTED format of ssp_bn_fwd_finalize -
 *     ssp_dwconv_stats_tile_m returns 0; the buffer holds [ssp_dwconv_stats_tiles][C][2] pairs followed by
 *     [ssp_dwconv_stats_tiles] pixel counts (ssp_dwconv_stats_floats floats in all) and the finalize takes tile_m = 0,
 *     M = B*Ho*Wo.  A tile = max(1, min(64, 1024 / (C/4))) consecutive strips (b, yo, four xo; a row's last strip partial) in
 *     row-major order.  Per channel: (mean, M2) of a strip's <= 4 values, strips Chan-combined in ascending order within
 *     max(1, 256 / C) equal parts of the tile, parts combined in ascending order - fp32, a fixed order, no atomics.
 *   data gradient: dx[pi][c] (=|+=) sum over the (po, tap) pairs that read pi of dy[po][c] * w[c*9 + tap].  Stride 1: the
 *     forward kernel with the taps flipped (products added in DESCENDING tap order).  Stride 2: a gather by the parity of
 *     pi = (yi, xi) - an even coordinate is reached by tap 1 only, an odd one by taps 0 and 2, so a pixel sums 1, 2, 2 or 4
 *     products (ascending tap order), never nine masked ones; one thread owns the four pixels of a 2 x 2 block of dx and
 *     loads its four dy pixels once.  Every element of dx's C columns is written by exactly one thread, no atomics: the same
 *     bits every run.  accumulate = 1 adds the earlier content last: dx = dx + s.
 *   filter gradient: dw[c*9 + tap] (=|+=) sum_po dy[po][c] * in[gather(po, tap)][c].  Two launches: workgroups sum fixed
 *     ranges of strips (ssp_dwconv_wgrad_workspace_floats = ranges * C * 9 floats; ranges <= 512 and a function of the shape
 *     alone) - a thread its strips in ascending order with fp32 fused multiply-adds, the threads of a range in ascending
 *     order - into the workspace; the finishing pass adds the ranges of an element in ascending order in float64, rounds
 *     once, and stores (accumulate = 1: dw = dw + s).  No atomics in either launch: the kernel is its own ordered form. */
int ssp_dwconv_fwd(const float* in, const float* w, float* out, const float* bias, float* stats, int B, int H, int W, int C,
                   int ldin, int ldout, int stride, void* stream);
int ssp_dwconv_fwd_affine(const float* in, const float* w, float* out, const float* scale, const float* shift, float slope,
                          int B, int H, int W, int C, int ldin, int ldout, int stride, void* stream);
int ssp_dwconv_stats_tile_m(int B, int H, int W, int C, int stride);   /* 0 = counted format */
int ssp_dwconv_stats_tiles(int B, int H, int W, int C, int stride);
int64_t ssp_dwconv_stats_floats(int B, int H, int W, int C, int stride);
int ssp_dwconv_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int C, int lddy, int lddx, int stride,
                     int accumulate, void* stream);
int64_t ssp_dwconv_wgrad_workspace_floats(int B, int H, int W, int C, int stride);
int ssp_dwconv_wgrad(const float* dy, const float* x, float* dw, int B, int H, int W, int C, int lddy, int ldx, int stride,
                     int accumulate, float* workspace, int64_t workspace_floats, void* stream);

/* ---- RegionLoss(region_loss.py:9-175, region_loss_multi.py:9-189, utils.py:138-187) ----------------------- */
/* out, grad: (nB, nA*(2K+1+nC), nH, nW) NCHW contiguous; target: (nB, 50*(2K+3)) float or double on the device;
 * partials: nB*8 floats; stats[8] = {loss_x, loss_y, loss_conf, loss_cls, total, nGT, nCorrect, nProposals}. */
int ssp_region_loss(const float* out, const void* target, int target_is_f64, float* grad, float* partials,
                    float* stats, int nB, int nA, int nC, int nH, int nW, int num_keypoints, float noobject_scale,
                    float object_scale, float coord_scale, float class_scale, float thresh, int conf_on, int multi,
                    const float* anchors, int anchor_step, void* stream);
/* get_region_boxes (utils.py:216-296): boxes[b][2K+4] = {2K coords, det_conf, cls_max_conf, cls_max_id, conf} */
int ssp_region_decode_argmax(const float* out, float* boxes, int nB, int nA, int nC, int nH, int nW,
                             int num_keypoints, int only_objectness, void* stream);

/* get_multi_region_boxes (multi_obj_pose_estimation/utils_multi.py:266-382): dense decode, scan order
 * key = (cy*nW + cx)*nA + anchor: rows[b][key][2K+3+nC] = {2K coords, det_conf, cls_max_conf, cls_max_id, softmax[nC]} */
int ssp_region_decode_all(const float* out, float* rows, int nB, int nA, int nC, int nH, int nW, int num_keypoints,
                          void* stream);

/* Multi-object validation matching (multi_obj_pose_estimation/valid_multi.py:110-123 on top of utils_multi.py:266-382),
 * every image on its own, one workgroup per image.  target: (nB, 50, 2K+3) floats on the device in the label layout
 * ssp_region_loss reads; the ground-truth count of an image is the index of its first row whose column 1 is 0 (50
 * when there is none).  For ground truth t of class c: among the cells with conf > conf_thresh (conf = det_conf *
 * cls_max_conf, or det_conf when only_objectness) whose arg-max class is c, the one with the largest det_conf, first
 * in scan order on a tie (source 1); when there is none, the reference's fallback box of class c - the last cell its
 * sequential `det_conf > max_conf and p_c > max_cls_conf` walk takes (source 2); source 0 when that walk takes no cell
 * (NaN head), when c is outside [0, nC) and for rows at or past the ground-truth count.
 *   rows[b][t][2K+4] = {2K coords as ssp_region_decode_all, det_conf, class confidence, class, match}
 *   meta[b][t][2]    = {source, scan-order key (cy*nW + cx)*nA + anchor, -1 when source is 0}
 * match = corner_confidence(gt corners, predicted corners) in fp32 with th = 80, sharpness = 2, the pixel scale
 * im_width x im_height and the exp(2) - 1 + 1e-5 normaliser.  num_keypoints == 9 only; at most 4096 cells
 * (nA * nH * nW) per image and 65535 classes, anything larger is refused. */
int ssp_region_match_multi(const float* out, const float* target, float* rows, int* meta, int nB, int nA, int nC, int nH,
                           int nW, int num_keypoints, float conf_thresh, int only_objectness, int im_width, int im_height,
                           void* stream);

/* Label-free multi-object detection: the same selection as ssp_region_match_multi, for a LIST OF CLASSES instead of an
 * image's label rows, one workgroup per image, every image on its own.  classes: nQ class ids (int32, on the device),
 * or NULL for every class in order (nQ must then equal nC, slot q is class q); an id may repeat, each slot gets its
 * class's row.  For image b and slot q of class c the result is the box get_multi_region_boxes(out[b:b+1], ...,
 * correspondingclass = c, only_objectness) followed by valid_multi.py:118-123 selects: source, key, tie rule and
 * fallback chain exactly as described above (the two kernels call the same device functions).
 *   rows[b][q][2K+3] = {2K coords as ssp_region_decode_all, det_conf, class confidence, class id}
 *   meta[b][q][2]    = {source, scan-order key (cy*nW + cx)*nA + anchor}
 * source 0 (an all-zero row, key -1): c outside [0, nC), or a head whose det_conf is NaN everywhere.  Every element of
 * rows and meta is written by every launch; nQ is not capped.  Refused before the launch: num_keypoints != 9, more
 * than 4096 cells (nA * nH * nW) per image, nQ < 1, nC outside 1..65535, a null out / rows / meta, classes == NULL
 * with nQ != nC. */
int ssp_region_detect_multi(const float* out, const int* classes, float* rows, int* meta, int nB, int nA, int nC, int nH,
                            int nW, int num_keypoints, int nQ, float conf_thresh, int only_objectness, void* stream);

/* ---- PnP (utils.py:86-100: cv2.solvePnP ITERATIVE + cv2.Rodrigues) ----------------------------------------- */
/* batched: pts3d [n][N][3], pts2d [n][N][2], K [n][9] (row-major) doubles on the device -> Rt [n][12] = R (9) | t (3) */
int ssp_pnp_batched(const double* pts3d, const double* pts2d, const double* K, double* Rt, int n, int N, int max_iter,
                    void* stream);

/* ---- evaluation metrics (valid.py:148-172, utils.py:31-58) ------------------------ */
/* n pose pairs over one mesh: vertices [N][3], Rt_gt / Rt_pr [n][12] = R (9, row-major) | t (3) (ssp_pnp_batched's
 * layout), K [9] (k_per_pose = 0) or [n][9], all doubles on the device ->
 * out [n][4] = {mean 2D reprojection distance (float32 projections, valid.py:160-165), mean 3D vertex distance
 * (valid.py:168-172), translation distance (valid.py:148), angular distance in degrees (utils.py:31-35)} */
int ssp_pose_errors(const double* vertices, int N, const double* Rt_gt, const double* Rt_pr, const double* K,
                    int k_per_pose, int n, double* out, void* stream);
/* calc_pts_diameter (utils.py:50-58): out[0] = largest pairwise distance of pts [N][3]; scratch: 8 bytes */
int ssp_pts_diameter(const double* pts, int N, double* out, double* scratch, void* stream);
/* The same four numbers with one mesh PER POSE (multi_obj_pose_estimation/valid_multi.py:47-50 loads a mesh per object;
 * valid.py:146-172 is the maths): verts [sumN][3] holds the nM meshes back to back, model_off [nM+1] int32 their vertex
 * offsets (model m is verts[model_off[m] .. model_off[m+1])), pose_model [n] int32 the mesh of each pose.  Pose i
 * averages over the vertices of its own mesh and divides by that mesh's count; with one mesh the result has the bits
 * of the single-mesh entry point above (one loop body serves both kernels).  THE CALLER GUARANTEES: model_off
 * non-decreasing with every model non-empty, pose_model values in [0, nM) - the kernel does not re-check them (the
 * Python layer validates them before the launch).  nM <= 0 is refused. */
int ssp_pose_errors_models(const double* verts, const int* model_off, const int* pose_model, int nM, const double* Rt_gt,
                           const double* Rt_pr, const double* K, int k_per_pose, int n, double* out, void* stream);
/* ADD-S, the metric of symmetric objects: adi(pts_est, pts_gt) of utils.py:60-63 /
 * multi_obj_pose_estimation/utils_multi.py:66-69, where the KD-tree is built on the ESTIMATED points and queried with
 * the GROUND-TRUTH points:
 *   out[i] = mean over g of  min over e of  || (R_gt v_g + t_gt) - (R_pr v_e + t_pr) ||,   g, e over the mesh of pose i
 * (the other direction is another number).  Brute force over all pairs in fp64: every squared distance is
 * (dx*dx + dy*dy) + dz*dz, each product and sum rounded on its own, one square root per query after the sweep; the
 * partial sums of a pose are added in a fixed order (no floating-point atomics), so two launches give the same bits.
 * verts / model_off / pose_model / Rt_* as for the per-mesh pose errors, with the same guarantees by the caller;
 * maxN >= the vertex count of every mesh a pose refers to (it sizes the grid; vertices past it would be left out, never
 * read out of range).  workspace: at least workspace_doubles(n, maxN) doubles on the device, refused when
 * `workspace_doubles` says it is smaller. */
int64_t ssp_adds_workspace_doubles(int n, int maxN);
int ssp_adds_errors(const double* verts, const int* model_off, const int* pose_model, int nM, int maxN,
                    const double* Rt_gt, const double* Rt_pr, int n, double* out, double* workspace,
                    int64_t workspace_doubles, void* stream);

/* ---- timed-launch bookkeeping (bench.py roofline): HIP events around every launch of a kernel family -------- */
/* mask: bit k = kernel family k (0 conv fwd, 1 conv dgrad, 2 conv wgrad, 3 BN/activation, 4 layout, 5 region/pnp/eval,
 * 6 optimizer, 7 first block forward passes, 8 first block backward passes); -1 = all, 0 = off.  Every timed launch costs two event packets on its stream. */
int ssp_prof_enable(int mask);
/* ms[k], work[k] (FLOPs or bytes), count[k] for k in 0..ssp_prof_nkinds()-1; synchronises on the recorded events */
int ssp_prof_nkinds(void);
int ssp_prof_collect(double* ms, double* work, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* SSP_HIP_H */

"""Exact-arithmetic test data of the through-memory Winograd pipeline, F(2x2) and F(4x4): operands, a geometry model,
float64 references and the case tables shared by tests/test_exact_wino_cpu.py (properties of the data, the model and the
bounds, no GPU) and tests/test_gpu_wino_exact.py (the kernels on them).

Method.  Of the three F(4x4) matrices (points 0, 1, -1, 1/2, -2) only G holds thirds and fifteenths: 2 B^T and 8 A^T are
integer matrices.  Every conv entry point takes the TRANSFORMED filter as its operand, so a test can hand in a U of small
integers that is the transform of no real filter.  With x, dy in {-1, 0, 1} everything downstream of U then lives on a
dyadic grid - V = B^T d B on 1/4, dM = A dY A^T on 1/64, Y = A^T [sum U V] A, dX = overlap-add of B [sum Ut dM] B^T and
dU = sum_t dM V on 1/256 - and, as long as the sum of the |terms| of every stage stays below 2^24 grid steps (bound_*()
below, asserted per case by the CPU test), every partial sum in ANY order is exactly representable in fp32: the input and
output-gradient transforms, the batched GEMM, both finishing passes with their neighbour gathers, and the transform-domain
filter-gradient contraction must reproduce the float64 reference bit for bit.  What stays inexact is the two per-filter
kernels that apply G (no geometry in them); they get an elementwise a-priori rounding bound (gamma()).

Because such a U is not the transform of a filter, the result is NOT a convolution and depends on the tile phase: the
references work on the tiled canvas.  The geometry is written from the description in include/ssp_hip.h, not from the
kernels: plain tiling (tile t = (b * th + ty) * tw + tx covers outputs (n ty .., n tx ..) of image b, windows one pixel
further out), or - when ssp_conv_wino_tiles says it needs fewer tiles - four consecutive images as one 2 x 2 mosaic with a
zero row / column between them, tiled as ONE map of (2H + 1) x (2W + 1): a mosaic is a plain tiling of a bigger canvas.
Planes are [(n+2)^2][T][C], plane xi = i * (n+2) + j.
"""
import collections

import numpy as np
import torch

import exact_data as X
from exact_data import rng
from oracle.wino_ref import matrices

TWO24 = 2 ** 24
U32 = 2.0 ** -24                     # unit roundoff of fp32
PREFILL, BIAS = 5, 3
F8 = np.float64


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ geometry
Geom = collections.namedtuple('Geom', 'B H W tile mosaic nb Hc Wc th tw T')


def geom(B, H, W, tile, mosaic=None):
    """Tiling of B maps of H x W (include/ssp_hip.h, ssp_conv_wino_tiles): the mosaic when it needs fewer tiles."""
    plain = B * cdiv(H, tile) * cdiv(W, tile)
    mos = cdiv(B, 4) * cdiv(2 * H + 1, tile) * cdiv(2 * W + 1, tile)
    if mosaic is None:
        mosaic = mos < plain
    nb, Hc, Wc = (cdiv(B, 4), 2 * H + 1, 2 * W + 1) if mosaic else (B, H, W)
    th, tw = cdiv(Hc, tile), cdiv(Wc, tile)
    return Geom(B, H, W, tile, bool(mosaic), nb, Hc, Wc, th, tw, nb * th * tw)


def to_canvas(img, g, gap=0.0, shift=(0, 0)):
    """[B,H,W,C] -> canvases [nb][Hc][Wc][C]: image 4 mb + 2 iy + ix of a mosaic at (iy (H+1), ix (W+1)), one row / column
    of `gap` between the images, phantom images zero.  `shift` moves the SECOND image of every mosaic (a wrong model)."""
    img = np.asarray(img, dtype=F8)
    if not g.mosaic:
        return img.copy()
    C = img.shape[-1]
    cv = np.zeros((g.nb, g.Hc, g.Wc, C), dtype=F8)
    cv[:, g.H, :, :] = gap
    cv[:, :, g.W, :] = gap
    for b in range(g.B):
        mb, iy, ix = b // 4, (b % 4) // 2, b % 2
        sy, sx = shift if b % 4 == 1 else (0, 0)
        y0, x0 = iy * (g.H + 1) + sy, ix * (g.W + 1) + sx
        cv[mb, y0:y0 + g.H, x0:min(x0 + g.W, g.Wc), :] = img[b][:, :min(g.W, g.Wc - x0)]
    return cv


def from_canvas(cv, g):
    """canvases -> [B,H,W,C]: gap rows / columns and phantom images dropped."""
    if not g.mosaic:
        return cv.copy()
    out = np.empty((g.B, g.H, g.W, cv.shape[-1]), dtype=cv.dtype)
    for b in range(g.B):
        mb, iy, ix = b // 4, (b % 4) // 2, b % 2
        out[b] = cv[mb, iy * (g.H + 1):iy * (g.H + 1) + g.H, ix * (g.W + 1):ix * (g.W + 1) + g.W]
    return out


def _to_planes(per_tile):
    """[nb,th,tw,a,a,C] -> [a*a][T][C]"""
    nb, th, tw, a, _, C = per_tile.shape
    return np.ascontiguousarray(per_tile.transpose(3, 4, 0, 1, 2, 5)).reshape(a * a, nb * th * tw, C)


def _from_planes(planes, g):
    """[a*a][T][C] -> [nb,th,tw,a,a,C]"""
    a = g.tile + 2
    return planes.reshape(a, a, g.nb, g.th, g.tw, planes.shape[-1]).transpose(2, 3, 4, 0, 1, 5)


def mats(tile, absolute=False):
    BT, G, AT = matrices(tile)
    return (np.abs(BT), np.abs(G), np.abs(AT)) if absolute else (BT, G, AT)


# ------------------------------------------------------------------------------------------------ references (float64)
def ref_V(x, g, m=None, gap=0.0, shift=(0, 0)):
    """V = B^T d B of the (n+2)^2 input windows at (n ty - 1, n tx - 1) of the canvas: planes [P][T][C]."""
    BT = (m or mats(g.tile))[0]
    n, a = g.tile, g.tile + 2
    cv = to_canvas(x, g, gap, shift)
    pad = np.zeros((g.nb, n * g.th + 2, n * g.tw + 2, cv.shape[-1]), dtype=F8)
    pad[:, 1:g.Hc + 1, 1:g.Wc + 1] = cv
    d = np.empty((g.nb, g.th, g.tw, a, a, cv.shape[-1]), dtype=F8)
    for ty in range(g.th):
        for tx in range(g.tw):
            d[:, ty, tx] = pad[:, n * ty:n * ty + a, n * tx:n * tx + a]
    return _to_planes(np.einsum('ik,nyxklc,jl->nyxijc', BT, d, BT))


def ref_dM(dy, g, m=None):
    """dM = A dY A^T of the n x n output-gradient tiles (zero past the canvas): planes [P][T][C]."""
    AT = (m or mats(g.tile))[2]
    n = g.tile
    cv = to_canvas(dy, g)
    pad = np.zeros((g.nb, n * g.th, n * g.tw, cv.shape[-1]), dtype=F8)
    pad[:, :g.Hc, :g.Wc] = cv
    d = pad.reshape(g.nb, g.th, n, g.tw, n, -1).transpose(0, 1, 3, 2, 4, 5)
    return _to_planes(np.einsum('pi,nyxpqc,qj->nyxijc', AT, d, AT))


def contract(planes, U):
    """[P][T][K] x [P][rows][K] -> [P][T][rows]: the batched GEMM."""
    return np.einsum('ptk,prk->ptr', planes, U)


def ref_fwd(V, U, g, m=None, last_row=True):
    """Y = A^T [sum_k U_xi[row][k] V_xi[t][k]] A scattered to the tiles' n x n outputs: [B,H,W,rows] (the forward form, and
    the data gradient by the older form with V = B^T dY B).  last_row=False drops the last tile row (a wrong model)."""
    AT = (m or mats(g.tile))[2]
    n = g.tile
    M = _from_planes(contract(V, U), g)
    Y = np.einsum('pi,nyxijc,qj->nyxpqc', AT, M, AT)
    if not last_row:
        Y[:, g.th - 1] = 0
    cv = Y.transpose(0, 1, 3, 2, 4, 5).reshape(g.nb, n * g.th, n * g.tw, -1)[:, :g.Hc, :g.Wc]
    return from_canvas(cv, g)


NEIGHBOURS = [(sy, sx) for sy in (-1, 0, 1) for sx in (-1, 0, 1) if (sy, sx) != (0, 0)]


def _span(s, n):
    """Rows of a tile's (n+2)-window that fall into the output tile s tile rows away FROM it: the tile at +1 gives its row 0."""
    return {1: [0], 0: list(range(1, n + 1)), -1: [n + 1]}[s]


def ref_adj(dM, Ut, g, m=None, skip=None, corner_swap=False):
    """dX = overlap-add of the windows B [sum_co Ut_xi[ci][co] dM_xi[t][co]] B^T: [B,H,W,Cin].
    skip = (sy, sx): every tile loses the contribution of its neighbour at (ty + sy, tx + sx); corner_swap: the coefficients
    of the (0, n+1) / (n+1, 0) corners and of the (n+1, n+1) corner exchanged - both wrong models."""
    BT = (m or mats(g.tile))[0]
    n, a = g.tile, g.tile + 2
    dV = _from_planes(contract(dM, Ut), g)
    dd = np.einsum('ik,nyxijc,jl->nyxklc', BT, dV, BT)
    if skip is not None:
        for r in _span(skip[0], n):
            for c in _span(skip[1], n):
                dd[:, :, :, r, c] = 0
    if corner_swap:
        c0, cl = BT[0][0], BT[a - 1][a - 1]
        dd[:, :, :, 0, a - 1] *= (cl * cl) / (c0 * cl)
        dd[:, :, :, a - 1, 0] *= (cl * cl) / (c0 * cl)
        dd[:, :, :, a - 1, a - 1] *= (c0 * cl) / (cl * cl)
    pad = np.zeros((g.nb, n * g.th + 2, n * g.tw + 2, dd.shape[-1]), dtype=F8)
    for ty in range(g.th):
        for tx in range(g.tw):
            pad[:, n * ty:n * ty + a, n * tx:n * tx + a] += dd[:, ty, tx]
    return from_canvas(pad[:, 1:g.Hc + 1, 1:g.Wc + 1], g)


def ref_dU(dM, V):
    """dU_xi[co][ci] = sum_t dM_xi[t][co] V_xi[t][ci]: [P][Cout][Cin]."""
    return np.einsum('ptc,ptk->pck', dM, V)


def back_filter(dU, tile, m=None):
    """G^T dU G: [P][Cout][Cin] -> [Cout][9][Cin] (the ssp_repack_fwd layout)."""
    G = (m or mats(tile))[1]
    a = tile + 2
    d = dU.reshape(a, a, dU.shape[1], dU.shape[2])
    return np.ascontiguousarray(np.einsum('ia,ijck,jb->cabk', G, d, G)).reshape(dU.shape[1], 9, dU.shape[2])


def filter_transform(w9, tile, m=None):
    """U[xi][row][k] = (G g G^T)[xi] of g[tap] = w9[row][tap][k]."""
    G = (m or mats(tile))[1]
    a = tile + 2
    g = np.asarray(w9, dtype=F8).reshape(w9.shape[0], 3, 3, w9.shape[2])
    return np.ascontiguousarray(np.einsum('ia,rabk,jb->ijrk', G, g, G)).reshape(a * a, w9.shape[0], w9.shape[2])


def gamma(n):
    """Bound of the relative error of n accumulated fp32 roundings (Higham): n u / (1 - n u)."""
    return n * U32 / (1 - n * U32)


# rounding counts of the two kernels that apply G at F(4x4), from csrc/conv_wino.hip (see tests/test_gpu_wino_exact.py)
N_FILTER, N_WGRAD_FINISH = 8, 13

# grid (1 / steps per unit) of each stage for x, dy, U integer
GRID = {4: dict(V=4, dM=64, Y=256, dX=256, dU=256), 2: dict(V=1, dM=1, Y=1, dX=1, dU=1)}


# ------------------------------------------------------------------------------------------------ operands
def int_map(key, B, H, W, C, p_zero=0.0, border=False, patch=False):
    """[B,H,W,C] in {-1, 0, 1}; optionally a zero border of odd width at the top / left and one all-non-zero patch."""
    rs = rng(*key)
    v = (rs.randint(0, 2, (B, H, W, C)) * 2 - 1) * (rs.uniform(0, 1, (B, H, W, C)) >= p_zero) if p_zero else \
        rs.randint(-1, 2, (B, H, W, C))
    v = v.astype(F8)
    if border:
        v[:, :X.odd_border(H)] = 0
        v[:, :, :X.odd_border(W)] = 0
    if patch:
        y0, x0 = min(X.odd_border(H) + 1, H - 1), min(X.odd_border(W) + 1, W - 1)
        blk = v[:, y0:y0 + 3, x0:x0 + 5]
        blk[...] = np.where(blk == 0, 1.0, blk)
    return v


def hand_U(key, tile, rows, K, density):
    """[P][rows][K] in {-1, 0, 1}, non-zero with probability `density`; every (plane, row) keeps at least one non-zero."""
    rs = rng(*key, 31)
    P = (tile + 2) ** 2
    U = ((rs.randint(0, 2, (P, rows, K)) * 2 - 1) * (rs.uniform(0, 1, (P, rows, K)) < density)).astype(F8)
    fix = rs.randint(0, K, (P, rows))
    pp, rr = np.nonzero((U != 0).sum(-1) == 0)
    U[pp, rr, fix[pp, rr]] = 1.0
    return U


def prefill(key, shape):
    return rng(*key, 77).randint(-PREFILL, PREFILL + 1, tuple(shape)).astype(F8)


def bias(key, C):
    return rng(*key, 78).randint(-BIAS, BIAS + 1, C).astype(F8)


def bn_vectors(key, C):
    """scale from exact_data.SCALES (zero, negative and positive in every group of four), integer shift (one zero per four)
    and mean, invstd a power of two; the raw map (raw_map) holds integers in [-1, 1]."""
    rs = rng(*key, 79)
    sc = X.scale(rs, C).numpy()
    sh = np.round(X.shift(rs, C, kmax=8).numpy())          # the grid k/4, |k| <= 8, rounded: integers in [-2, 2]
    mu = rs.randint(-1, 2, C).astype(F8)
    istd = np.asarray((1.0, 2.0))[rs.randint(0, 2, C)]
    return sc, sh, mu, istd


def raw_map(key, B, H, W, C):
    return rng(*key, 80).randint(-1, 2, (B, H, W, C)).astype(F8)


def leaky(y, slope):
    return np.where(y > 0, y, y * slope)


def bn_sums(g, raw, sc, sh, mu, istd, slope):
    """(sum dy', sum dy' xhat, sum |dy'|, sum |dy' xhat|) per channel over all pixels; dy' = g * leaky'(scale raw + shift)
    with the leaky sign taken from y > 0 as the kernels do (y == 0 counts as negative)."""
    y = raw * sc + sh
    dyq = np.where(y > 0, g, g * slope)
    xhat = (raw - mu) * istd
    ax = (0, 1, 2)
    return dyq.sum(ax), (dyq * xhat).sum(ax), np.abs(dyq).sum(ax), np.abs(dyq * xhat).sum(ax)


def nhwc(v, ld=None, off=0, fill=float('nan')):
    """float64 [B,H,W,C] -> fp32 torch [B*H*W][ld]: the values at [off, off + C), `fill` in every other column."""
    C = v.shape[-1]
    ld = ld or C
    assert off % 4 == 0 and ld % 4 == 0 and off + C <= ld
    buf = torch.full((v.size // C, ld), fill, dtype=torch.float32)
    buf[:, off:off + C] = torch.from_numpy(np.ascontiguousarray(v).reshape(-1, C)).float()
    return buf


def f32(a):
    """float64 array -> fp32 torch tensor, asserted to lose nothing."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    assert torch.equal(t.float().double(), t), "reference value not representable in fp32"
    return t.float()


# ------------------------------------------------------------------------------------------------ cases
# B, H, W: what it reaches (at tile 4 unless said)
TILINGS = [
    (1, 4, 4),         # one tile per row and column at tile 4: every neighbour absent
    (2, 8, 12),        # exact tiling, all neighbours present in the interior
    (3, 10, 7),        # ragged plain tiling
    (4, 13, 13),       # one full mosaic
    (7, 13, 13),       # two mosaics, one phantom image
    (4, 13, 9),        # non-square mosaic
    (2, 13, 13),       # 13 x 13 plain at tile 4 (too few images for a mosaic)
]

W4, W4_128, W4_RING8, W4_A128, W2 = 8006413, 8012814, 8006418, 8012813, 9006413

Case = collections.namedtuple('Case', 'id shape K N plan density p_zero wide')


def _case(kind, shape, K, N, plan, density, p_zero=0.0, wide=False):
    return Case('%s-%dx%dx%d-%dto%d-p%d%s' % ((kind,) + shape + (K, N, plan, '-wide' if wide else '')), shape, K, N, plan,
                density, p_zero, wide)


# forward (ssp_conv_fwd: K = Cin, N = Cout) and data gradient by the older form (ssp_conv_dgrad: K = Cout_dy, N = Cin_dx):
# every tiling once, the three F(4x4) plan codes, a partial 64-channel slab (144, 80), 64 -> 128, and a 256-wide output that also
# runs under wino_variant 4
CONV_CASES = [
    _case('conv', (1, 4, 4), 64, 64, W4, 1.0),
    _case('conv', (2, 8, 12), 64, 144, W4, 0.5),
    _case('conv', (3, 10, 7), 80, 64, W4_128, 0.5),
    _case('conv', (4, 13, 13), 64, 128, W4, 0.5),
    _case('conv', (7, 13, 13), 64, 64, W4_RING8, 0.5),
    _case('conv', (4, 13, 9), 64, 128, W4_128, 0.5),
    _case('conv', (2, 13, 13), 64, 256, W4, 0.5, wide=True),
    _case('conv', (2, 13, 13), 64, 256, W2, 0.5, wide=True),          # the F(2x2) finishing pass on 256-channel slabs
]

# adjoint data gradient (ssp_conv_dgrad_adj: K = Cout_dy, N = Cin_dx): all tilings x the three plan codes; the shapes of
# tests/test_gpu_wino_adjoint.py plus the full mosaic and a 256-wide dx (wino_variant 4)
_ADJ_SHAPES = [((1, 4, 4), 64, 64, 0.5), ((2, 8, 12), 144, 64, 0.125), ((3, 10, 7), 64, 80, 0.25), ((4, 13, 13), 64, 64, 0.25),
               ((7, 13, 13), 64, 128, 0.25), ((4, 13, 9), 128, 64, 0.125), ((2, 13, 13), 64, 256, 0.25)]
ADJ_CASES = [_case('adj', s, K, N, plan, d, 0.5, wide=(N >= 256)) for s, K, N, d in _ADJ_SHAPES for plan in (W4, W4_A128, W2)]

# fused epilogues at F(4x4): a ragged plain tiling and a mosaic, each with more than one group of 16 tiles (so that fewer
# `partial` rows than groups exist).  Sparse operands: the BatchNorm-backward sums run over ALL pixels of a channel on the
# grid 1/2048 (slope 0.125), which leaves 8192 units for the sum of |dy' xhat|
EPI_CASES = [
    _case('epi', (3, 10, 7), 64, 64, W4, 1.0 / 32, 0.97),
    _case('epi', (8, 5, 5), 64, 80, W4_128, 1.0 / 32, 0.97),
]
SLOPES = (1.0, 0.0, 0.125, 0.1)

# filter gradient at tile 4 (T >= 16, Cin, Cout >= 64 and % 16 == 0): a mosaic and a ragged plain tiling
WGRAD_CASES = [((4, 13, 13), 64, 128), ((3, 10, 7), 80, 64)]

# the F(2x2) adjoint with real filters (multiples of 4), against exact_conv.ref_dgrad: shapes of exact_conv.CONV_CASES
ADJ_F2_REAL_SHAPES = [(2, 13, 13, 64, 128, 3), (3, 10, 14, 128, 96, 3), (5, 7, 9, 128, 128, 3)]

TRANSFORM_C = 20                      # channels of the transform-only cases: five quads, ten pairs - no power of two


def case_operands(c, tile=None):
    """(x-like map [B,H,W,K], hand-built U [P][N][K]) of a case; every second case gets the zero border and the patch."""
    tile = tile or (4 if c.plan < 9000000 else 2)
    B, H, W = c.shape
    odd = (B + H + c.K) % 2 == 1 and c.p_zero < 0.9          # (the sparse epilogue cases stay sparse)
    v = int_map((B, H, W, c.K, c.N, c.plan), B, H, W, c.K, c.p_zero, border=odd, patch=odd)
    return v, hand_U((B, H, W, c.K, c.N, c.plan), tile, c.N, c.K, c.density)


def wgrad_operands(shape, Cin, Cout):
    """(x with the zero border and the patch, dy) of a filter-gradient case."""
    return (int_map(shape + (Cin, 1), *shape, Cin, border=True, patch=True), int_map(shape + (Cout, 2), *shape, Cout))


def epilogue_refs(c):
    """What the three fused-epilogue launches of a case must give (float64): shared with the GPU test."""
    g = geom(*c.shape, 4)
    v, U = case_operands(c)
    key = c.shape + (c.K, c.N)
    conv = ref_fwd(ref_V(v, g), U, g)                       # forward form: ssp_conv_fwd_affine, ssp_conv_dgrad_bnbwd
    adj = ref_adj(ref_dM(v, g), U, g)                       # adjoint form: ssp_conv_dgrad_adj_bnbwd
    sc, sh, mu, istd = bn_vectors(key, c.N)
    raw = raw_map(key, *c.shape, c.N)
    return dict(g=g, v=v, U=U, conv=conv, adj=adj, sc=sc, sh=sh, mu=mu, istd=istd, raw=raw)


# ------------------------------------------------------------------------------------------------ bounds
def steps(tile, stage, value):
    return float(value) * GRID[tile][stage]


def bound_fwd(v, U, g):
    """{stage: grid steps} of the forward form on these operands: sums of |terms| through |B^T|, |U|, |A^T|."""
    ma = mats(g.tile, absolute=True)
    Va = ref_V(np.abs(v), g, ma)
    out = dict(V=steps(g.tile, 'V', Va.max()))
    out['M'] = steps(g.tile, 'V', contract(Va, np.abs(U)).max())
    out['Y'] = steps(g.tile, 'Y', ref_fwd(Va, np.abs(U), g, ma).max())
    return out


def bound_adj(dy, Ut, g):
    """{stage: grid steps} of the adjoint form: |A| |dY| |A^T|, its contraction with |Ut|, and |B| . |B^T| summed over the
    overlapping windows (the overlap-add counted as a sum of absolute values)."""
    ma = mats(g.tile, absolute=True)
    dMa = ref_dM(np.abs(dy), g, ma)
    out = dict(dM=steps(g.tile, 'dM', dMa.max()))
    out['dV'] = steps(g.tile, 'dM', contract(dMa, np.abs(Ut)).max())
    out['dX'] = steps(g.tile, 'dX', ref_adj(dMa, np.abs(Ut), g, ma).max())
    return out


def bound_wgrad(x, dy, g):
    ma = mats(g.tile, absolute=True)
    return dict(dU=steps(g.tile, 'dU', ref_dU(ref_dM(np.abs(dy), g, ma), ref_V(np.abs(x), g, ma)).max()))

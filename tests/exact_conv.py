"""Exact-integer test data of the convolution family: operands, buffers, int64 references and the case tables shared by
tests/test_exact_conv_cpu.py (properties of the data, the references and the route coverage, no GPU) and
tests/test_gpu_conv_exact.py (the kernels on them).

Method.  x and dy are integers in [-3, 3], filters integers in [-2, 2] (multiples of 4 in [-8, 8] where a Winograd F(2x2)
plan transforms them: G has entries 0, +-1, +-1/2, so G g G^T is then an integer too).  Every product and every partial
sum of a forward, data-gradient or filter-gradient contraction is then an integer far below 2^24, exactly representable
in fp32 WHATEVER the summation order: split-K partials, hybrid tails, atomics arriving in any order and the Winograd
F(2x2) transforms (matrices of 0, +-1, +-1/2) must all reproduce the int64 reference bit for bit.  A dropped or doubled
pixel row, a tap leaking across an image border, a stale workspace row or a leaking pad column changes an integer and
fails torch.equal; none of them hides below a 1e-4 tolerance.  F(4x4) uses the point 1/2 and thirds in G: not exact, it
stays on its tolerance (test_exact_conv_cpu.py pins that split).

Layout.  Activations are NHWC [B*H*W][ld]; channel counts are padded to a multiple of 4 with ZERO pad columns (as the
engine allocates them), every other column of a wider buffer is NaN (gpu_util.to_nhwc).  Filters: [Cout][R*R][Cinp]
(forward / filter gradient) and [Cin][R*R][Coutp] with flipped taps (data gradient), built here on the host.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from exact_data import rng

XMAX, WMAX, WMAX_WINO, PREFILL = 3, 2, 8, 5
TWO24 = 2 ** 24


def pad4(c):
    return (c + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ route codes
# include/ssp_hip.h, ssp_conv_wgrad_route: family*1e8 + ring_slots*1e7 + flags*1e6 + BMO*1000 + BNI
LDS, REG, C4 = 1, 2, 3


def route_code(family, nslot, bmo, bni, fold=False, bvec=False):
    return family * 100000000 + nslot * 10000000 + (int(fold) + 2 * int(bvec)) * 1000000 + bmo * 1000 + bni


def route_fields(code):
    return dict(family=code // 100000000, nslot=code // 10000000 % 10, fold=bool(code // 1000000 % 10 & 1),
                bvec=bool(code // 1000000 % 10 & 2), bmo=code // 1000 % 1000, bni=code % 1000)


# ------------------------------------------------------------------------------------------------ operands and buffers
def operands(key, B, H, W, Cin, Cout, R, wino=False):
    """(x [B,H,W,Cin], dy [B,H,W,Cout], w [Cout,R,R,Cin]) as int64 tensors, seeded by `key`."""
    rs = rng(*key)
    x = torch.from_numpy(rs.randint(-XMAX, XMAX + 1, (B, H, W, Cin)).astype(np.int64))
    dy = torch.from_numpy(rs.randint(-XMAX, XMAX + 1, (B, H, W, Cout)).astype(np.int64))
    w = torch.from_numpy(rs.randint(-WMAX, WMAX + 1, (Cout, R, R, Cin)).astype(np.int64))
    return x, dy, (w * 4 if wino else w)


def prefill(key, shape):
    """Integers in [-PREFILL, PREFILL]: what an accumulating launch finds in its output."""
    return torch.from_numpy(rng(*key, 77).randint(-PREFILL, PREFILL + 1, tuple(shape)).astype(np.int64))


def nhwc_buffer(v, ld=None, off=0, fill=float('nan')):
    """int64 [B,H,W,C] -> fp32 [B*H*W][ld]: the values at [off, off + C), zeros up to off + pad4(C), `fill` elsewhere."""
    C = v.shape[-1]
    cp = pad4(C)
    ld = ld or cp
    assert off % 4 == 0 and ld % 4 == 0 and off + cp <= ld
    buf = torch.full((v.numel() // C, ld), fill, dtype=torch.float32)
    buf[:, off:off + cp] = 0.0
    buf[:, off:off + C] = v.reshape(-1, C).float()
    return buf


def pack_fwd(w):
    """[Cout,R,R,Cin] -> int64 [Cout][R*R][Cinp] (ssp_repack_fwd's layout, zero pad)."""
    Cout, R, _, Cin = w.shape
    out = torch.zeros(Cout, R * R, pad4(Cin), dtype=torch.int64)
    out[:, :, :Cin] = w.reshape(Cout, R * R, Cin)
    return out


def pack_dgrad(w):
    """[Cout,R,R,Cin] -> int64 [Cin][R*R][Coutp], taps flipped (ssp_repack_dgrad's layout, zero pad)."""
    Cout, R, _, Cin = w.shape
    out = torch.zeros(Cin, R * R, pad4(Cout), dtype=torch.int64)
    out[:, :, :Cout] = torch.flip(w.reshape(Cout, R * R, Cin), dims=[1]).permute(2, 1, 0)
    return out


# ------------------------------------------------------------------------------------------------ int64 references
def _pad_hw(t, p):
    return F.pad(t, (0, 0, p, p, p, p)) if p else t


def ref_fwd(x, w):
    """out[b,y,x,co] = sum_{ky,kx,ci} x[b, y+ky-p, x+kx-p, ci] * w[co,ky,kx,ci], zero outside the image; int64 NHWC."""
    B, H, W, Cin = x.shape
    Cout, R = w.shape[0], w.shape[1]
    xp = _pad_hw(x, R // 2)
    out = torch.zeros(B * H * W, Cout, dtype=torch.int64)
    for ky in range(R):
        for kx in range(R):
            out += xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Cin) @ w[:, ky, kx, :].t()
    return out.view(B, H, W, Cout)


def ref_dgrad(dy, w):
    """dx[b,y,x,ci] = sum_{ky,kx,co} dy[b, y-ky+p, x-kx+p, co] * w[co,ky,kx,ci]; int64 NHWC."""
    B, H, W, Cout = dy.shape
    R, Cin = w.shape[1], w.shape[3]
    p = R // 2
    dyp = _pad_hw(dy, p)
    dx = torch.zeros(B * H * W, Cin, dtype=torch.int64)
    for ky in range(R):
        for kx in range(R):
            dx += dyp[:, 2 * p - ky:2 * p - ky + H, 2 * p - kx:2 * p - kx + W, :].reshape(-1, Cout) @ w[:, ky, kx, :]
    return dx.view(B, H, W, Cin)


def ref_wgrad(dy, x, R):
    """dw[co][ky*R+kx][ci] = sum_{b,y,x} dy[b,y,x,co] * x[b, y+ky-p, x+kx-p, ci]; int64, packed [Cout][R*R][Cinp]."""
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    xp = _pad_hw(x, R // 2)
    dyt = dy.reshape(-1, Cout).t().contiguous()
    dw = torch.zeros(Cout, R * R, pad4(Cin), dtype=torch.int64)
    for ky in range(R):
        for kx in range(R):
            dw[:, ky * R + kx, :Cin] = dyt @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Cin)
    return dw


def macs(B, H, W, Cin, Cout, R):
    return B * H * W * R * R * Cin * Cout


def first_diffs(got, want, names, n=5):
    """'count differ; first (names) = got / want ...' of two equally shaped tensors (NaN counts as different)."""
    bad = (got != want).nonzero()
    rows = ['%s: %r != %r' % (tuple(int(i) for i in ix), float(got[tuple(ix)]), float(want[tuple(ix)])) for ix in bad[:n]]
    return '%d of %d differ; first (%s): %s' % (bad.shape[0], got.numel(), ', '.join(names), '; '.join(rows))


# ------------------------------------------------------------------------------------------------ bounds
def bound_wgrad(B, H, W, prefilled=True):
    """Largest |partial sum| of a direct filter gradient: one product <= 9 per pixel (+ the prefill)."""
    return B * H * W * XMAX * XMAX + (PREFILL if prefilled else 0)


def bound_conv(K, R, wmax=WMAX, prefilled=True):
    """Largest |partial sum| of a forward / data-gradient output over K channels and R*R taps."""
    return R * R * K * XMAX * wmax + (PREFILL if prefilled else 0)


def bound_wino2_conv(K):
    """F(2x2) forward / data gradient, filters multiples of 4 up to 8: |B^T d B| <= 4 * 3 (two +-1 per row, twice),
    |G g G^T| <= 1.5^2 * 8 (row sums of |G| <= 1.5), transform-domain sums over K channels, then A^T . A with three
    +-1 per row: 9 of them.  The bound of the largest intermediate."""
    return 9 * (4 * XMAX) * int(2.25 * WMAX_WINO) * K


def bound_wino2_wgrad(T):
    """F(2x2) filter gradient over T tiles: |A dY A^T| <= 4 * 3 and |B^T d B| <= 4 * 3 (two +-1 per row, twice), their
    products summed over the tiles, then G^T . G (row sums of |G^T| <= 2, entries on the 1/2 grid): the back-transformed
    values are multiples of 1/4, so FOUR times their bound has to stay below 2^24 grid steps."""
    du = (4 * XMAX) * (4 * XMAX) * T
    return du, 4 * (2 * 2 * du)


def wino_tiles(B, H, W, tile):
    """ssp_conv_wino_tiles: plain tiling, or the 2 x 2 image mosaic when that needs fewer tiles."""
    c = lambda a, b: (a + b - 1) // b
    return min(B * c(H, tile) * c(W, tile), c(B, 4) * c(2 * H + 1, tile) * c(2 * W + 1, tile))


# ------------------------------------------------------------------------------------------------ filter-gradient cases
WgradCase = collections.namedtuple('WgradCase', 'id shape route ldx xoff lddy dyoff prefill opts')


def _wg(name, shape, route, sliced=False, pre=False, opts=(), slice_x=True):
    B, H, W, Cin, Cout, R = shape
    cinp, coutp = pad4(Cin), pad4(Cout)
    ldx, xoff = (cinp + 16, 8) if (sliced and slice_x) else (cinp, 0)
    lddy, dyoff = (coutp + 12, 4) if sliced else (coutp, 0)
    tag = '%s-%dx%dx%d-%dto%d-r%d%s%s%s' % (name, B, H, W, Cin, Cout, R, '-sliced' if sliced else '', '-acc' if pre else '',
                                          ''.join('-%s%d' % (k.replace('wgrad_', ''), v) for k, v in opts))
    return WgradCase(tag, shape, route, ldx, xoff, lddy, dyoff, pre, tuple(opts))


# pixel ranges: M < 16 (fewer chunks than the ring prologue issues), W = 8 (two row wraps per 16-pixel chunk) with M no
# multiple of 16, an odd W < 16 with B >= 2 (the row walker crosses image borders), H = 1
_PIX_WIDE = [(1, 1, 9), (3, 3, 8), (2, 5, 11), (2, 1, 19)]
# the same for the routes reached through W < 8 (a wider map would move to the LDS-direct family)
_PIX_NARROW = [(1, 1, 5), (3, 5, 7), (2, 1, 7), (2, 6, 3)]

# name, route, base (B, H, W, Cin, Cout, R) - the issue's table -, ragged (Cin, Cout) or None, pixel ranges
WGRAD_ROUTES = [
    ('lds256x128', route_code(LDS, 3, 256, 128), (2, 13, 13, 128, 256, 3), (144, 272), _PIX_WIDE),
    ('lds128x128', route_code(LDS, 3, 128, 128), (2, 13, 13, 128, 128, 3), (160, 200), _PIX_WIDE),
    ('lds128x64', route_code(LDS, 4, 128, 64), (2, 13, 13, 64, 128, 3), (80, 136), _PIX_WIDE),
    ('lds64x128', route_code(LDS, 4, 64, 128), (3, 9, 11, 128, 64, 3), (132, 70), _PIX_WIDE),       # Cout % 4 == 2
    ('lds64x64', route_code(LDS, 4, 64, 64), (2, 10, 12, 96, 64, 1), (80, 72), _PIX_WIDE),
    ('fold128x64', route_code(LDS, 4, 128, 64, fold=True), (1, 9, 11, 32, 128, 3), (32, 136), _PIX_WIDE),
    ('fold64x64', route_code(LDS, 4, 64, 64, fold=True), (2, 16, 20, 32, 64, 3), (32, 72), _PIX_WIDE),
    ('reg128x128', route_code(REG, 3, 128, 128), (4, 5, 5, 128, 128, 3), (132, 136), _PIX_NARROW),
    ('reg128x64', route_code(REG, 3, 128, 64), (4, 5, 5, 64, 128, 3), (80, 136), _PIX_NARROW),
    ('reg64x128', route_code(REG, 3, 64, 128), (4, 5, 5, 128, 64, 3), (132, 72), _PIX_NARROW),
    ('reg64x64', route_code(REG, 3, 64, 64), (4, 3, 3, 64, 64, 3), (80, 72), _PIX_NARROW),
    ('reg128x32', route_code(REG, 3, 128, 32), (2, 9, 11, 32, 128, 1), (20, 136), _PIX_WIDE),
    ('reg64x32', route_code(REG, 3, 64, 32), (2, 9, 11, 32, 64, 1), (20, 72), _PIX_WIDE),
    ('reg32x128', route_code(REG, 3, 32, 128), (2, 7, 9, 1024, 20, 1), (132, 18), _PIX_WIDE),       # the real head, 1024 -> 20
    ('reg32x64', route_code(REG, 3, 32, 64), (2, 7, 9, 64, 20, 1), (80, 22), _PIX_WIDE),
    ('reg32x32', route_code(REG, 3, 32, 32), (3, 7, 9, 32, 20, 1), (20, 6), _PIX_WIDE),
    ('c4', route_code(C4, 2, 32, 4), (1, 20, 24, 3, 32, 3), None, _PIX_WIDE),                       # first layer, RGB + zero pad
]


def _route_cases():
    out = []
    for name, route, base, ragged, pix in WGRAD_ROUTES:
        sx = name != 'c4'                      # the 4-channel kernel takes ldx == 4 only: its dy alone is sliced
        R = base[5]
        out.append(_wg(name, base, route))
        if ragged is not None:                 # ragged cout and cin tiles, as slices of wider buffers, accumulating
            out.append(_wg(name, base[:3] + ragged + (R,), route, sliced=True, pre=True, slice_x=sx))
        else:
            out.append(_wg(name, base, route, sliced=True, pre=True, slice_x=sx))
        for i, bhw in enumerate(pix):
            out.append(_wg(name, bhw + base[3:], route, sliced=bool(i & 1), pre=not (i & 1), slice_x=sx))
    # a first layer that misses the 4-channel kernel: 8 filters (tests/golden/tiny-pose.cfg), and ldx = 8
    out.append(_wg('first8', (1, 20, 24, 3, 8, 3), route_code(REG, 3, 32, 32)))
    c = _wg('firstld8', (1, 20, 24, 3, 32, 3), route_code(REG, 3, 32, 32))
    out.append(c._replace(ldx=8, xoff=4, id=c.id + '-ldx8'))
    return out


_S = (2, 13, 13, 128, 128, 3)          # M = 338: at most 3 pixel ranges of >= 8 chunks
_X = (12, 13, 13, 128, 128, 3)         # M = 2028 >= 1921, 9 tiles: the XCD-ordered grid, its split a multiple of 8 (<= 16)
_T = (2, 13, 13, 128, 256, 3)


def _split_cases():
    r128, r256 = route_code(LDS, 3, 128, 128), route_code(LDS, 3, 256, 128)
    out = [_wg('split', _S, r128, opts=(('wgrad_split', s),)) for s in (1, 3)]
    out += [_wg('xcd', _X, r128, pre=True)]
    out += [_wg('xcd', _X, r128, sliced=True, opts=(('wgrad_split', s),)) for s in (8, 16)]
    # the A/B variants documented as "same results"
    out += [_wg('var', _S, route_code(REG, 3, 128, 128), opts=(('wgrad_variant', 2),)),       # register-staged kernels only
            _wg('var', _S, route_code(LDS, 4, 128, 128), opts=(('wgrad_variant', 3),)),       # 4-slot ring
            _wg('var', _S, route_code(LDS, 3, 128, 128, bvec=True), opts=(('wgrad_variant', 6),)),   # interleaved cin blocks
            _wg('var', _T, r128, opts=(('wgrad_variant', 8),)),                               # no 256-cout tiles
            _wg('var', _X, r128, opts=(('wgrad_variant', 10),)),                              # plain workgroup order
            _wg('var', _T, r256, pre=True, opts=(('wgrad_variant', 11),)),                    # generic epilogue
            _wg('var', (12, 13, 13, 256, 1024, 3), r256, opts=(('wgrad_variant', 20),))]      # (range, cout tile) units per XCD
    return out


WGRAD_CASES = _route_cases() + _split_cases()

# Winograd filter gradient: (tile, (B, H, W, Cin, Cout)); tile 2 / 12 exact, tile 4 on the same data at 1e-4.  An odd
# map, a mosaic-tiled batch, and 32-channel operands (tile 12 alone goes below 64 channels)
WINO_WGRAD_CASES = [(t, s) for s in ((2, 13, 13, 64, 128), (7, 13, 13, 64, 128), (3, 10, 14, 128, 64)) for t in (2, 12, 4)] + \
                   [(12, (2, 9, 11, 32, 32)), (12, (1, 5, 3, 32, 64))]

# ------------------------------------------------------------------------------------------------ forward / data gradient
WINO2, WINO2_128, WINOF, WINO4, WINO4_128 = 9006413, 9012814, 7000001, 8006413, 8012814
# (direction, (B, H, W, Cin, Cout, R), plan): every case runs on channel slices of wider buffers, once into a NaN-filled
# output and once accumulating into an integer-prefilled one
CONV_CASES = [
    ('fwd', (2, 13, 13, 64, 128, 3), 0),
    ('fwd', (2, 10, 12, 128, 64, 1), 0),
    ('fwd', (3, 7, 9, 32, 20, 1), 0),
    ('fwd', (2, 13, 13, 48, 160, 3), 0),
    ('fwd', (1, 12, 12, 3, 32, 3), 0),            # first layer: 4-channel K chunks
    ('fwd', (2, 7, 9, 1024, 20, 1), 0),           # the head: thin split-K
    ('dgrad', (2, 13, 13, 64, 128, 3), 0),
    ('dgrad', (2, 10, 12, 128, 64, 1), 0),
    ('dgrad', (3, 7, 9, 32, 20, 1), 0),
    ('dgrad', (2, 13, 13, 1024, 20, 1), 0),       # the head's data gradient: 20 -> 1024, register-staged kernel
    ('dgrad', (4, 13, 13, 256, 256, 3), 12834),   # forced split-K x3
]
for _s in ((2, 13, 13, 64, 128, 3), (3, 10, 14, 128, 96, 3), (5, 7, 9, 128, 128, 3), (2, 1, 5, 64, 128, 3)):
    for _p in (WINO2, WINO2_128, WINOF, WINO4, WINO4_128):
        if _p in (WINO2_128, WINO4_128) and _s[0] != 3:
            continue
        CONV_CASES += [('fwd', _s, _p), ('dgrad', _s, _p)]


def conv_case_id(c):
    return '%s-%dx%dx%d-%dto%d-r%d-p%d' % ((c[0],) + c[1] + (c[2],))


def wino_exact(plan):
    """Winograd F(2x2) plans (9xxxxxx, 7000001) are exact on these operands; F(4x4) (8xxxxxx) is not."""
    return not (8000000 <= plan < 9000000)


def is_wino(plan):
    return plan >= 7000000


# ------------------------------------------------------------------------------------------------ plan sweep
# every direct code the tuner hands out, forward and data gradient: more than one resident wave at both tile heights
# (hybrid codes get a main part and a tail), and a grid smaller than one wave
SWEEP_SHAPES = [(16, 52, 52, 128, 256, 3), (2, 13, 13, 128, 256, 3)]


def sweep_ref_images(B):
    """Images the int64 reference covers: everything on the small shape, the first and the last two of the large one."""
    return list(range(B)) if B <= 4 else [0, B - 2, B - 1]


def decode_plan(code):
    """(tail, rows, ksplit, slots) of a direct plan code (include/ssp_hip.h)."""
    return code // 100000, code // 100 % 1000, code // 10 % 10, code % 10

"""Test data of the bf16x3 twin codes of the through-memory Winograd plans (base + 600000 + tile_rows * 100 + 13: the plan's
batched GEMM on the bf16 matrix cores, csrc/conv_igemm_bf16x3.hip): the method of tests/exact_bf16x3.py carried to the
transform domain - shared by tests/test_wino_bf16x3_cpu.py (properties of the data, no GPU) and tests/test_gpu_wino_bf16x3.py.

The GEMM contracts V [P][T][K] (planes of the input transform; dM for the adjoint form) with the transformed filter U
[P][N][K], which every entry point takes directly.  Both are split h + m + l on their way into LDS and the six products
h*h, h*m, m*h, m*m, h*l, l*h are evaluated.  Three classes of operand pairs, built from the integers of exact_bf16x3.py:

  v3u1   V multi-term (x sprinkled with +-262657), U one-term ({-1, 0, 1})     needs h*h, m*h, l*h
  v1u3   V one-term (x in {-1, 0, 1}, sparse), U sprinkled with +-262657       needs h*h, h*m, h*l
  v2u2   V two-term (x sprinkled with +-257 / 385 / 513), U the same           needs h*h, h*m, m*h, m*m

V is whatever B^T d B makes of x, so the CPU test ASSERTS per case and class, on the float64 transform model of
tests/exact_wino.py: V is exactly an fp32, the three dropped products vanish identically, each pinned product is needed, and
sum_k |U| |V| stays below 2^24 (every value is an integer: at F(4x4), whose B^T holds halves, x is scaled by 4).  The x maps
are sparse for that reason: a window must not collect more than a few of the large values.
For the adjoint form with the caller's dM both GEMM operands are handed in (planes(), no transform in front).  The adjoint
form that transforms dY itself runs the classes at F(2x2) (A holds 0 and +-1); at F(4x4) A spans 1/8 .. 8 per axis, twelve
binary orders in a plane, which leaves no room for multi-term values in one exact fp32 sum: that path runs on the {-1, 0, 1}
operands of tests/exact_wino.py (class 'ones').
"""
import collections

import numpy as np
import torch

import exact_bf16x3 as X3
import exact_wino as XW
from exact_data import rng

CLASSES = ('v3u1', 'v1u3', 'v2u2')
PRODUCTS, DROPPED = X3.PRODUCTS, X3.DROPPED
PINNED = {'v3u1': X3.PINNED['x3w1'], 'v1u3': X3.PINNED['x1w3'], 'v2u2': X3.PINNED['x2w2']}
X3_WINO = 600000
BMS = (64, 128)


def twin(tile, bm):
    return (8000000 if tile == 4 else 9000000) + X3_WINO + bm * 100 + 13


def fp32_twin(code):
    """The fp32 Winograd code with the same tiling of the GEMM (hundred-thousands digit removed, ring digit 3)."""
    return code - X3_WINO


Case = collections.namedtuple('Case', 'id shape tile K N')


def _case(shape, tile, K, N):
    return Case('%dx%dx%d-f%d-%dto%d' % (shape + (tile, K, N)), shape, tile, K, N)


# plain tiling with one partial row tile (T = 24 / 8); T = 80 at F(4x4): two 64-row tiles, the last partial; T = 392 at
# F(2x2): four 128-row tiles, the last partial; a full mosaic from the exact_wino table.  K = 16 / 48 / 112: 1, 3 and 7
# K-steps (7 crosses the 6-step fold and leaves a remainder); N = 64: the 64-column tile, 68: one partial 128-column tile,
# 132: two column tiles, the second partial.
CASES = [
    _case((2, 5, 7), 2, 16, 64), _case((2, 5, 7), 2, 48, 132),
    _case((2, 5, 7), 4, 112, 68), _case((2, 5, 7), 4, 16, 132),
    _case((5, 13, 13), 4, 48, 64), _case((5, 13, 13), 4, 112, 132),
    _case((8, 13, 13), 2, 112, 64), _case((8, 13, 13), 2, 16, 68),
    _case((4, 13, 13), 4, 48, 68),
]
assert XW.geom(5, 13, 13, 4).T == 80 and XW.geom(8, 13, 13, 2).T == 392 and XW.geom(4, 13, 13, 4).mosaic


def geom(c):
    return XW.geom(*c.shape, c.tile)


def scale(c):
    return 4 if c.tile == 4 else 1


def _sparse_ones(rs, shape, density):
    return ((rs.randint(0, 2, shape) * 2 - 1) * (rs.uniform(0, 1, shape) < density)).astype(np.int64)


def _place(rs, a, values, count):
    """`count` entries of a (flat positions drawn without replacement) set to +- one of `values`."""
    flat = a.reshape(-1)
    pos = rs.choice(flat.size, size=min(count, flat.size), replace=False)
    flat[pos] = rs.choice(np.asarray(values, dtype=np.int64), size=pos.size) * (rs.randint(0, 2, pos.size) * 2 - 1)
    return a


def x_map(cls, c):
    """[B,H,W,K] float64: the launch's input map (forward: x, data gradient: dy), integers times scale(c)."""
    B, H, W = c.shape
    g = geom(c)
    rs = rng(CLASSES.index(cls), 41, *c.shape, c.tile, c.K, c.N)
    x = _sparse_ones(rs, (B, H, W, c.K), 0.02 if cls == 'v1u3' else 0.05)      # (v1u3: |V| * 262657 must stay below 2^24)
    if cls == 'v3u1':
        x = _place(rs, x, (X3.THREE_TERM,), max(4, g.T // 4))
    elif cls == 'v2u2':
        x = _place(rs, x, X3.TWO_TERM, max(8, g.T))
    return (x * scale(c)).astype(np.float64)


def planes(cls, c):
    """[P][T][K] float64, hand-built: the dM operand of the adjoint form when the caller gives it."""
    g = geom(c)
    P = (c.tile + 2) ** 2
    rs = rng(CLASSES.index(cls), 43, *c.shape, c.tile, c.K, c.N)
    v = _sparse_ones(rs, (P, g.T, c.K), 0.25)
    if cls == 'v3u1':
        v = _place(rs, v, (X3.THREE_TERM,), max(8, P * g.T // 8))
    elif cls == 'v2u2':
        v = _place(rs, v, X3.TWO_TERM, max(16, P * g.T))
    return v.astype(np.float64)


def u_op(cls, c):
    """[P][N][K] float64: the transformed-filter operand (U, or Ut of the adjoint form), hand-built integers."""
    P = (c.tile + 2) ** 2
    rs = rng(CLASSES.index(cls), 47, *c.shape, c.tile, c.K, c.N)
    u = _sparse_ones(rs, (P, c.N, c.K), 0.25)
    if cls == 'v1u3':
        u = _place(rs, u, (X3.THREE_TERM,), P * c.N // 8)
    elif cls == 'v2u2':
        u = _place(rs, u, X3.TWO_TERM, P * c.N * c.K // 8)
    return u.astype(np.float64)


def terms(a):
    """float64 array of fp32 values -> its (h, m, l) as float64 arrays (exact_bf16x3.split3: the kernel's split)."""
    t = XW.f32(a)
    return tuple(p.double().numpy() for p in X3.split3(t))


def model(V, U, products=PRODUCTS):
    """Sum of the listed term products of the batched GEMM, float64 [P][T][N] (exact: every value an integer below 2^53)."""
    tv, tu = terms(V), terms(U)
    out = 0.0
    for a, b in products:
        out = out + XW.contract(tv[a], tu[b])
    return out


def abs_bound(V, U):
    return float(XW.contract(np.abs(V), np.abs(U)).max())


def gemm_operands(cls, c, entry):
    """(V-like planes float64 [P][T][K], U float64 [P][N][K], the pixel map they came from or None) of an entry point:
    'fwd' / 'dgrad' (V = B^T x B), 'adj-dm' (hand-built dM), 'adj-own' (dM = A dY A^T; class 'ones' at F(4x4))."""
    g = geom(c)
    if entry == 'adj-dm':
        return planes(cls, c), u_op(cls, c), None
    if entry == 'adj-own':
        if c.tile == 4:
            xc = XW.Case(c.id, c.shape, c.K, c.N, twin(4, 64), 0.25, 0.5, False)
            dy, Ut = XW.case_operands(xc, 4)
            return XW.ref_dM(dy, g), Ut, dy
        dy = x_map(cls, c)
        return XW.ref_dM(dy, g), u_op(cls, c), dy
    x = x_map(cls, c)
    return XW.ref_V(x, g), u_op(cls, c), x


ENTRIES = ('fwd', 'dgrad', 'adj-dm', 'adj-own')

# ------------------------------------------------------------------------------------------------ host queries
# (B, H, W, Cin, Cout, R, plan, fits)
FITS_TABLE = [
    (2, 5, 7, 16, 64, 3, twin(4, 128), 1),
    (2, 5, 7, 16, 64, 3, twin(4, 64), 1),
    (2, 5, 7, 48, 68, 3, twin(2, 128), 1),
    (8, 13, 13, 112, 132, 3, twin(2, 64), 1),
    (64, 13, 13, 1024, 1024, 3, 8612813, 1),
    (64, 26, 26, 512, 256, 3, 9606413, 1),
    (2, 5, 7, 24, 64, 3, twin(4, 128), 0),                # Cin % 16
    (2, 5, 7, 16, 32, 3, twin(4, 128), 0),                # Cout < 64
    (2, 5, 7, 16, 66, 3, twin(2, 64), 0),                 # Cout % 4
    (2, 5, 7, 16, 64, 1, twin(4, 128), 0),                # R
    (2, 5, 7, 16, 64, 3, 8600000 + 3213, 0),              # tile rows 32
    (2, 5, 7, 16, 64, 3, 9600000 + 25613, 0),             # tile rows 256
    (2, 5, 7, 16, 64, 3, 8512813, 0),                     # hundred-thousands digit 5
    (2, 5, 7, 16, 64, 3, 9706413, 0),                     # ... and 7
    (2, 5, 7, 16, 64, 3, 8612814, 0),                     # ring digit 4
    (2, 5, 7, 64, 64, 3, 7612813, 0),                     # an on-chip code with the digit
]
MISFITS = [r[:7] for r in FITS_TABLE if not r[7]]

"""Test data of the bf16x3 convolution (csrc/conv_igemm_bf16x3.hip): a host model of the three-term split, and exact-integer
operands on which EACH of the six evaluated products is needed - shared by tests/test_bf16x3_cpu.py (properties of the
data, no GPU) and tests/test_gpu_bf16x3.py (the kernel on them).

The kernel writes every fp32 operand as h + m + l (three bf16 terms, round to nearest even) and evaluates
h*h + h*m + m*h + m*m + h*l + l*h; it drops m*l + l*m + l*l.  The method of tests/exact_conv.py (integer operands, every
partial sum an exact fp32 whatever the order, torch.equal against int64) is extended with integers that NEED the lower
terms, chosen so that round-to-nearest-even and truncation split them the same way (remainders below half an ulp, or - 257 and
385 - a tie whose even neighbour is the truncated value):

  one-term    integers in [-3, 3]
  two-term    +-257, +-385, +-513             = (256, 1), (384, 1), (512, 1)
  three-term  +-262657 = 2^18 + 2^9 + 1       = (262144, 512, 1)

Three classes of operand pairs (x = the launch's input map, w = its filter):

  x3w1   x three-term (sparse), w one-term     needs h*h, m*h, l*h
  x1w3   x one-term, w three-term (sparse)     needs h*h, h*m, h*l
  x2w2   both two-term (sparse)                needs h*h, h*m, m*h, m*m

and in each the three dropped products are identically zero, so the six-product sum IS the product.  Sparsity keeps
sum |x| |w| below 2^24 at every output (asserted by the CPU test, never assumed).
"""
import numpy as np
import torch

import exact_conv as E
from exact_data import rng

TWO_TERM = (257, 385, 513)
THREE_TERM = 262657
CLASSES = ('x3w1', 'x1w3', 'x2w2')
# (term of x, term of w) of the six evaluated products, in the kernel's order (smallest first); 0 = h, 1 = m, 2 = l
PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
DROPPED = ((1, 2), (2, 1), (2, 2))
# the products each class is there to pin
PINNED = {'x3w1': ((0, 0), (1, 0), (2, 0)), 'x1w3': ((0, 0), (0, 1), (0, 2)), 'x2w2': ((0, 0), (0, 1), (1, 0), (1, 1))}
DENSITY = {'x3w1': (0.02, None), 'x1w3': (None, 0.02), 'x2w2': (0.15, 0.5)}      # share of multi-term values in (x, w)

BF16X3 = 6000000


def plan_code(bm, ksplit=1):
    return BF16X3 + bm * 100 + ksplit * 10 + 3


# ------------------------------------------------------------------------------------------------ host model of the split
def bf16_rne(x):
    """fp32 -> nearest bf16 (ties to even), back in fp32."""
    return x.to(torch.bfloat16).to(torch.float32)


def bf16_trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def is_bf16(x):
    return bool(((x.contiguous().view(torch.int32) & 0xFFFF) == 0).all())


def split3(x, cvt=bf16_rne):
    """x = h + m + l as the kernel forms it: h = bf16(x), r = x - h, m = bf16(r), l = r - m (fp32 tensors)."""
    x = x.to(torch.float32)
    h = cvt(x)
    r = x - h
    m = cvt(r)
    return h, m, r - m


# ------------------------------------------------------------------------------------------------ operands
def _sprinkle(rs, base, values, density):
    if density is None:
        return base
    pick = rs.random_sample(base.shape) < density
    v = rs.choice(np.asarray(values, dtype=np.int64), size=base.shape) * rs.choice(np.asarray([-1, 1], dtype=np.int64), size=base.shape)
    return np.where(pick, v, base)


def operands(cls, key, B, H, W, K, N, R):
    """(inp [B,H,W,K], w [N][R*R][K]) int64: the input map of a launch with K input and N output channels and its filter
    in the packed layout the kernel reads (forward: ssp_repack_fwd's; data gradient: ssp_repack_dgrad's - the contraction
    is the same, so the same operands serve both entry points)."""
    rs = rng(CLASSES.index(cls), *key)
    x = rs.randint(-E.XMAX, E.XMAX + 1, (B, H, W, K)).astype(np.int64)
    w = rs.randint(-E.WMAX, E.WMAX + 1, (N, R * R, K)).astype(np.int64)
    dx_, dw_ = DENSITY[cls]
    vals = {'x3w1': (THREE_TERM,), 'x1w3': (THREE_TERM,), 'x2w2': TWO_TERM}[cls]
    x = _sprinkle(rs, x, vals, dx_)
    w = _sprinkle(rs, w, vals, dw_)
    return torch.from_numpy(x), torch.from_numpy(w)


def conv(inp, w, R):
    """int64 reference of the launch: out[b,y,x,n] = sum_{tap,k} inp[b, y+ty-p, x+tx-p, k] * w[n][tap][k]."""
    N, _, K = w.shape
    return E.ref_fwd(inp, w.reshape(N, R, R, K))


def terms(v):
    """int64 tensor -> its (h, m, l) as int64 tensors (the split of the fp32 value; exact for these integers)."""
    return tuple(t.to(torch.int64) for t in split3(v.to(torch.float32)))


def model(inp, w, R, products=PRODUCTS):
    """Sum of the listed term products, int64: what a kernel evaluating exactly those products computes."""
    ti, tw = terms(inp), terms(w)
    out = None
    for a, b in products:
        c = conv(ti[a], tw[b], R)
        out = c if out is None else out + c
    return out


def abs_bound(inp, w, R):
    """max over the outputs of sum |inp| |w|: every partial sum of every product, in any order, stays below it."""
    return int(conv(inp.abs(), w.abs(), R).max())


# ------------------------------------------------------------------------------------------------ cases
# pixels: one partial tile with odd sizes and every border; three row tiles at 128 rows / five at 64 with image borders
# inside the tiles.  K = 16 / 48: one and three K-steps per tap.  N = 64: the 64-column tile; 68: a partial second
# column tile; 132: two column tiles, the second partial.
PIXELS = ((2, 5, 7), (3, 9, 11))
KS = (16, 48)
NS = (64, 68, 132)
CASES = [(b, h, w_, k, n, r) for (b, h, w_) in PIXELS for k in KS for n in NS for r in (1, 3)]


def case_id(c):
    return '%dx%dx%d-%dto%d-r%d' % c


# launches the fits query must refuse / accept: (B, H, W, Cin, Cout, R, plan, fits)
FITS_TABLE = [
    (2, 5, 7, 16, 64, 3, plan_code(128), 1),
    (2, 5, 7, 16, 64, 1, plan_code(64), 1),
    (3, 9, 11, 48, 68, 3, plan_code(64, 3), 1),           # 27 K-steps, 9 per split
    (3, 9, 11, 48, 132, 3, plan_code(128, 2), 1),
    (64, 104, 104, 32, 64, 3, plan_code(128), 1),         # layer 2 of yolo-pose
    (64, 13, 13, 1024, 64, 1, plan_code(128, 8), 1),
    (2, 5, 7, 24, 64, 3, plan_code(128), 0),              # Cin % 16
    (2, 5, 7, 4, 64, 3, plan_code(128), 0),               # the first block's Cin
    (2, 5, 7, 16, 32, 3, plan_code(128), 0),              # Cout <= 32
    (2, 5, 7, 16, 20, 1, plan_code(128), 0),
    (2, 5, 7, 16, 66, 3, plan_code(128), 0),              # Cout % 4
    (2, 5, 7, 16, 64, 5, plan_code(128), 0),              # R
    (2, 5, 7, 16, 64, 3, plan_code(256), 0),              # tile rows
    (2, 5, 7, 16, 64, 3, plan_code(32), 0),
    (2, 5, 7, 16, 64, 3, plan_code(128, 0), 0),           # split 0
    (2, 5, 7, 16, 64, 3, plan_code(128) + 1, 0),          # last digit
    (2, 5, 7, 16, 64, 3, plan_code(128, 2), 0),           # 9 K-steps: fewer than 8 per split
    (3, 9, 11, 48, 68, 3, plan_code(64, 4), 0),           # 27 K-steps / 4 < 8
    (2, 5, 7, 16, 64, 3, 12813, 0),                       # a direct code
    (2, 5, 7, 64, 64, 3, 9006413, 0),                     # a Winograd code
    (2, 5, 7, 16, 64, 3, 0, 0),
    (1 << 10, 1 << 11, 1 << 10, 16, 64, 3, plan_code(128), 0),   # 2^31 pixels
]
# the rows a LAUNCH can be asked for (finite buffers): every misfit above but the last
MISFIT_LAUNCHES = [r[:7] for r in FITS_TABLE if not r[7] and r[0] * r[1] * r[2] < (1 << 20) and r[6] >= BF16X3 and r[6] < 7000000]

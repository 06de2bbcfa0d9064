"""Exact-arithmetic test data: inputs on coarse dyadic grids, so that every intermediate of the operation under test is
exactly representable in fp32.  fp32 and float64 then agree on every per-element decision (leaky sign, pool winner),
ties and zeros are frequent instead of measure-zero, the float64 reference may take its OWN decisions, and most outputs
can be compared bit for bit (tests/test_gpu_decisions.py; the properties are pinned by tests/test_exact_data_cpu.py).

Everything is returned as float64 torch tensors (NCHW for maps); the caller casts to fp32 for the launch."""
import numpy as np
import torch

SCALES = (-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0)
INVSTD = (0.5, 1.0, 2.0)


def rng(*key):
    return np.random.RandomState(np.random.SeedSequence([int(k) for k in key]).generate_state(4))


def odd_border(n):
    """An odd border width of about n / 8: window boundaries (even) and the constant region never align."""
    return (n // 8) | 1


def image(rs, B, H, W, C=3, border=True, patch=True):
    """(B, C, H, W) on the grid k/4 in [0, 1]; a zero-filled border of odd width at the top and at the left (what a jitter
    crop leaves) and a saturated (all-ones) patch around the centre, 11 x 21 pixels from an odd corner: it crosses the
    16-pixel block seams of the first-block kernels on every map wider than 32."""
    x = rs.randint(0, 5, (B, C, H, W)).astype(np.float64) / 4
    if border:
        x[:, :, :odd_border(H), :] = 0
        x[:, :, :, :odd_border(W)] = 0
    if patch:
        y0, x0 = max((H // 2 - 5) | 1, odd_border(H) + 2), max((W // 2 - 10) | 1, odd_border(W) + 2)
        x[:, :, y0:y0 + 11, x0:x0 + 21] = 1
    return torch.from_numpy(x)


def filters(rs, cout, cin, R, denom=8, kmax=8):
    """(cout, cin, R, R) on the grid k / denom, |k| <= kmax."""
    return torch.from_numpy(rs.randint(-kmax, kmax + 1, (cout, cin, R, R)).astype(np.float64) / denom)


def int_map(rs, shape, lo, hi):
    """Small integers in [lo, hi]: raw conv outputs / upstream gradients."""
    return torch.from_numpy(rs.randint(lo, hi + 1, tuple(shape)).astype(np.float64))


def sparse_map(rs, shape, p_zero=0.5):
    """Values in {-1, 0, 1} with P(0) = p_zero."""
    v = rs.randint(0, 2, tuple(shape)) * 2 - 1
    return torch.from_numpy((v * (rs.uniform(0, 1, tuple(shape)) >= p_zero)).astype(np.float64))


def scale(rs, C):
    """Per-channel BatchNorm scale from SCALES; every group of four channels (what one lane / one float4 holds) has at
    least one zero, one negative and one positive value, at shuffled positions."""
    out = np.empty(C)
    neg, pos = [s for s in SCALES if s < 0], [s for s in SCALES if s > 0]
    for c0 in range(0, C, 4):
        grp = [0.0, neg[rs.randint(len(neg))], pos[rs.randint(len(pos))], SCALES[rs.randint(len(SCALES))]]
        rs.shuffle(grp)
        out[c0:c0 + 4] = grp[:min(4, C - c0)]
    return torch.from_numpy(out)


def shift(rs, C, kmax=8):
    """Per-channel shift on the grid k/4, |k| <= kmax, with one exact zero per group of four channels (a zero raw value -
    the zero-filled border - then gives y == 0 exactly)."""
    out = rs.randint(-kmax, kmax + 1, C).astype(np.float64) / 4
    for c0 in range(0, C, 4):
        out[c0 + rs.randint(min(4, C - c0))] = 0.0
    return torch.from_numpy(out)


def mean(rs, C, kmax=8):
    return torch.from_numpy(rs.randint(-kmax, kmax + 1, C).astype(np.float64) / 4)


def invstd(rs, C):
    return torch.from_numpy(np.asarray(INVSTD)[rs.randint(0, len(INVSTD), C)])


def per_channel(v):
    return v.view(1, -1, 1, 1)


def assert_exact(t64, grid, bound=None):
    """Construction check, run on the float64 reference BEFORE any launch.  Every value of t64 is a multiple of `grid` (a
    power of two) and survives a round trip through fp32; `bound` >= the largest sum of |terms| any output of the
    operation is made of (default: max |t64|) stays below 2^24 grid steps.  Then every partial sum, in any order and with
    or without fused multiply-adds, is an integer number of grid steps below 2^24: exactly representable in fp32."""
    t = t64.detach()
    assert t.dtype == torch.float64
    assert float(np.log2(grid)) == int(np.log2(grid)), "grid must be a power of two"
    assert torch.equal(t.float().double(), t), "not representable in fp32"
    assert torch.equal(torch.round(t / grid) * grid, t), "off the grid %g" % grid
    b = float(t.abs().max()) if bound is None else float(bound)
    assert b >= float(t.abs().max())
    assert b / grid < 2 ** 24, "sum of |terms| %g needs more than 24 bits on the grid %g" % (b, grid)


def conv_exact(x64, w64, gx, gw, transpose=False):
    """float64 'same' convolution (or its transpose: the data gradient) of two on-grid operands, asserted exact."""
    import torch.nn.functional as F
    pad = w64.shape[-1] // 2
    op = F.conv_transpose2d if transpose else F.conv2d
    out = op(x64, w64, None, padding=pad)
    assert_exact(out, gx * gw, op(x64.abs(), w64.abs(), None, padding=pad).max())
    return out


def leaky(y, slope):
    return torch.where(y > 0, y, y * slope)


def block_ref(raw64, sc, sh, slope, pool):
    """Reference of the BatchNorm-affine + leaky (+ 2x2 max-pool) block with its own decisions: returns (y, out) with y a
    leaf that requires grad, so out.backward(g) leaves dL/dy (leaky sign and ATen's first-maximum pool winner) in y.grad."""
    import torch.nn.functional as F
    y = (raw64 * per_channel(sc) + per_channel(sh)).detach().requires_grad_(True)
    a = F.leaky_relu(y, slope)
    return y, (F.max_pool2d(a, 2, 2) if pool else a)


def tied_window_fraction(a):
    """Fraction of 2x2 windows of the activation map whose maximum is attained more than once."""
    B, C, H, W = a.shape
    w = a.detach().view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    return float(((w == w.max(dim=-1, keepdim=True)[0]).sum(-1) > 1).double().mean())


def ulp_diff(got32, ref64):
    """Largest distance of the fp32 result from the float64 reference, in units of the fp32 spacing at the reference."""
    ref32 = ref64.float().numpy()
    ulp = np.spacing(np.maximum(np.abs(ref32), np.float32(2.0 ** -100))).astype(np.float64)
    return float((np.abs(got32.double().numpy() - ref64.numpy()) / ulp).max())


# ------------------------------------------------------------------------------------------------ the cases, shared by
# tests/test_exact_data_cpu.py (properties of the data alone) and tests/test_gpu_decisions.py (the kernels on them)
BN_SHAPES = [(32, 2, 8, 12), (1024, 1, 4, 6), (20, 3, 6, 6), (64, 5, 26, 26)]          # (C, B, H, W)
FIRST_SHAPES = [(2, 8, 32), (3, 16, 96), (2, 64, 128), (1, 100, 112), (1, 416, 416)]   # (B, H, W)


def bn_case(C, B, H, W, pool):
    """Inputs of ssp_bn_act_fwd / _bwd: integer raw map in [-4, 4], integer upstream gradient in [-3, 3], vectors."""
    rs = rng(C, B, H, W, pool)
    d = dict(raw=int_map(rs, (B, C, H, W), -4, 4), scale=scale(rs, C), shift=shift(rs, C), mean=mean(rs, C),
             invstd=invstd(rs, C))
    d['g'] = int_map(rs, (B, C, H // 2, W // 2) if pool else (B, C, H, W), -3, 3)
    for k in ('raw', 'g'):
        assert_exact(d[k], 1.0)
    assert_exact(d['raw'] * per_channel(d['scale']) + per_channel(d['shift']), 0.25, 4 * 2 + 2)
    return d


def first_case(B, H, W):
    """Inputs of the fused first block (3 -> 32 channels, 3 x 3): image, filters, vectors, pooled upstream gradient."""
    rs = rng(B, H, W)
    d = dict(x=image(rs, B, H, W), w=filters(rs, 32, 3, 3), scale=scale(rs, 32), shift=shift(rs, 32), mean=mean(rs, 32),
             invstd=invstd(rs, 32), g=int_map(rs, (B, 32, H // 2, W // 2), -2, 2),
             c1=mean(rs, 32, 4) / 4, c2=mean(rs, 32, 4) / 4)
    assert_exact(d['x'], 0.25)
    assert_exact(d['w'], 0.125)
    return d

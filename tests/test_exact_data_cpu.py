"""The exact-arithmetic data of tests/exact_data.py, on the float64 reference alone (no kernel, no GPU): the conditions
that make tests/test_gpu_decisions.py able to fail.  Every intermediate is exactly representable in fp32 (so fp32 and
float64 agree on every decision and the results can be compared bit for bit), pooled windows tie often, y == 0 occurs,
and a kernel that pooled the raw map before the affine (legal only for scale > 0) would give a different result."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_data as X


def _check_block(raw, d, zeros_min=0.01):
    sc, sh = d['scale'], d['shift']
    y = raw * X.per_channel(sc) + X.per_channel(sh)
    X.assert_exact(y, 1.0 / 64)
    # fp32 arithmetic takes the same decisions: the affine is exact in fp32, fused or not
    y32 = raw.float() * X.per_channel(sc).float() + X.per_channel(sh).float()
    assert torch.equal(y32.double(), y)
    assert float((y == 0).double().mean()) >= zeros_min
    a = X.leaky(y, 0.125)                    # the dyadic slope with the fewest ties (0 ties every negative value)
    X.assert_exact(a, 1.0 / 512)
    assert X.tied_window_fraction(a) >= 0.20
    # first and last maximum differ wherever the maximum is tied: a >= for a > in a winner loop moves gradient
    B, C, H, W = a.shape
    w = a.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    first = w.argmax(-1)
    last = 3 - w.flip(-1).argmax(-1)
    tied = (w == w.max(-1, keepdim=True)[0]).sum(-1) > 1
    assert bool(((first != last) == tied).all())
    # pool-before-affine (max of the raw window, then scale / shift / leaky) is wrong in every group of four channels
    # that holds a negative scale - and every group does
    true = F.max_pool2d(a, 2, 2)
    early = X.leaky(F.max_pool2d(raw, 2, 2) * X.per_channel(sc) + X.per_channel(sh), 0.125)
    differs = (true != early).flatten(2).any(-1).any(0)
    for c0 in range(0, C, 4):
        grp = sc[c0:c0 + 4]
        assert bool((grp == 0).any()) and bool((grp < 0).any()) and bool((grp > 0).any())
        assert bool(differs[c0:c0 + 4][grp < 0].any())
    assert set(sc.tolist()) <= set(X.SCALES) and set(d['invstd'].tolist()) <= set(X.INVSTD)
    assert torch.equal(sh * 4, torch.round(sh * 4)) and torch.equal(d['mean'] * 4, torch.round(d['mean'] * 4))


@pytest.mark.parametrize("C,B,H,W", X.BN_SHAPES + [(24, 2, 6, 10)])
def test_bn_case_data(C, B, H, W):
    d = X.bn_case(C, B, H, W, 1)
    _check_block(d['raw'], d)
    assert d['g'].shape == (B, C, H // 2, W // 2) and float(d['g'].abs().max()) <= 3
    assert X.bn_case(C, B, H, W, 0)['g'].shape == (B, C, H, W)


@pytest.mark.parametrize("B,H,W", X.FIRST_SHAPES)
def test_first_case_data(B, H, W):
    d = X.first_case(B, H, W)
    x, w = d['x'], d['w']
    assert float(x.min()) == 0 and float(x.max()) == 1
    bh, bw = X.odd_border(H), X.odd_border(W)
    assert bh % 2 == 1 and bw % 2 == 1 and float(x[:, :, :bh].abs().max()) == 0 and float(x[:, :, :, :bw].abs().max()) == 0
    raw = X.conv_exact(x, w, 0.25, 0.125)
    # fp32 convolution == float64 convolution, whatever the summation order (here: ATen's, and the taps reversed)
    raw32 = F.conv2d(x.float(), w.float(), None, padding=1)
    assert torch.equal(raw32.double(), raw)
    flipped = F.conv2d(x.float().flip(-1, -2), w.float().flip(-1, -2), None, padding=1).flip(-1, -2)
    assert torch.equal(flipped.double(), raw)
    _check_block(raw, d)
    # the data gradient of the block with c1 = c2 = 0 is exact too (integer upstream gradient, dyadic slope)
    y, out = X.block_ref(raw, d['scale'], d['shift'], 0.125, 1)
    out.backward(d['g'])
    dx = X.conv_exact(X.per_channel(d['scale']) * y.grad, w, 1.0 / 16, 0.125, transpose=True)
    assert torch.equal(F.conv_transpose2d((X.per_channel(d['scale']) * y.grad).float(), w.float(), None, padding=1).double(), dx)


def test_assert_exact_rejects_bad_constructions():
    X.assert_exact(torch.tensor([0.25, -3.0], dtype=torch.float64), 0.25)
    with pytest.raises(AssertionError):
        X.assert_exact(torch.tensor([0.1], dtype=torch.float64), 0.25)                 # not a dyadic value
    with pytest.raises(AssertionError):
        X.assert_exact(torch.tensor([0.125], dtype=torch.float64), 0.25)               # off the grid
    with pytest.raises(AssertionError):
        X.assert_exact(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), 2.0 ** -30)   # dyadic, but 31 bits
    with pytest.raises(AssertionError):
        X.assert_exact(torch.tensor([1.0], dtype=torch.float64), 0.25, bound=2.0 ** 23)     # the sum of |terms| overflows
    assert X.ulp_diff(torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([1.0], dtype=torch.float64)) == 1.0


def test_sparse_and_filter_generators():
    rs = X.rng(1)
    s = X.sparse_map(rs, (2, 8, 5, 5))
    assert set(s.flatten().tolist()) == {-1.0, 0.0, 1.0}
    w = X.filters(rs, 8, 4, 3, denom=4, kmax=2)
    X.assert_exact(w, 0.25)
    assert float(w.abs().max()) <= 0.5

"""Properties of tests/exact_conv.py that tests/test_gpu_conv_exact.py relies on, checked without a GPU: the int64
references against PyTorch's float64 convolution and its autograd, the 2^24 bounds that make every summation order
exact, the exact / tolerance split between Winograd F(2x2) and F(4x4), and the coverage of the filter-gradient routes
(ssp_conv_wgrad_route is a host function: the library is loaded, no GPU call is made)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_conv as E

SMALL_MACS = 3e8      # cases below this many multiply-adds are cross-checked against float64 here


def _nchw(t):
    return t.permute(0, 3, 1, 2).double().contiguous()


def _float64_triplet(x, dy, w):
    """(forward, data gradient, filter gradient) of F.conv2d in float64, as int64 NHWC / [Cout][R*R][Cinp]."""
    R = w.shape[1]
    xd = _nchw(x).requires_grad_(True)
    wd = w.permute(0, 3, 1, 2).double().contiguous().requires_grad_(True)
    out = F.conv2d(xd, wd, None, padding=R // 2)
    out.backward(_nchw(dy))
    Cout, Cin = w.shape[0], w.shape[3]
    dw = torch.zeros(Cout, R * R, E.pad4(Cin), dtype=torch.int64)
    dw[:, :, :Cin] = wd.grad.reshape(Cout, Cin, R * R).permute(0, 2, 1).round().long()
    assert torch.equal(wd.grad, wd.grad.round()) and torch.equal(out, out.round())
    return out.detach().permute(0, 2, 3, 1).long(), xd.grad.permute(0, 2, 3, 1).round().long(), dw


def _small_shapes():
    shapes = {c.shape for c in E.WGRAD_CASES} | {c[1] for c in E.CONV_CASES} | {s + (3,) for _, s in E.WINO_WGRAD_CASES}
    shapes.add((1, 5, 6, 8, 12, 3))
    return sorted(s for s in shapes if E.macs(*s) <= SMALL_MACS)


@pytest.mark.parametrize("shape", _small_shapes(), ids=lambda s: 'x'.join(map(str, s)))
def test_int64_references_equal_float64_conv2d_and_autograd(shape):
    x, dy, w = E.operands(shape, *shape)
    out, dx, dw = _float64_triplet(x, dy, w)
    assert torch.equal(E.ref_fwd(x, w), out)
    assert torch.equal(E.ref_dgrad(dy, w), dx)
    assert torch.equal(E.ref_wgrad(dy, x, shape[5]), dw)


def test_operand_ranges_buffers_and_packed_layouts():
    x, dy, w = E.operands((1, 2, 3), 2, 3, 5, 6, 10, 3)
    assert int(x.min()) == -3 and int(x.max()) == 3 and int(dy.min()) == -3 and int(dy.max()) == 3
    assert int(w.min()) == -2 and int(w.max()) == 2
    _, _, w4 = E.operands((1, 2, 3), 2, 3, 5, 6, 10, 3, wino=True)
    assert torch.equal(w4, 4 * w) and int(w4.abs().max()) == 8
    buf = E.nhwc_buffer(x, ld=24, off=8)
    assert buf.shape == (30, 24) and torch.isnan(buf[:, :8]).all() and torch.isnan(buf[:, 16:]).all()
    assert torch.equal(buf[:, 8:14].long(), x.reshape(-1, 6)) and (buf[:, 14:16] == 0).all()      # zero pad to a multiple of 4
    pf, pd = E.pack_fwd(w), E.pack_dgrad(w)
    assert pf.shape == (10, 9, 8) and (pf[:, :, 6:] == 0).all() and int(pf[3, 5, 2]) == int(w[3, 1, 2, 2])
    assert pd.shape == (6, 9, 12) and (pd[:, :, 10:] == 0).all() and int(pd[2, 8 - 5, 3]) == int(w[3, 1, 2, 2])
    # the packed data-gradient operand is ssp_repack_dgrad's: flipped taps, channels swapped
    ref = torch.flip(w.permute(0, 3, 1, 2).reshape(10, 6, 9), dims=[2]).permute(1, 2, 0)
    assert torch.equal(pd[:, :, :10], ref)


def test_every_partial_sum_stays_below_two_to_the_24():
    for c in E.WGRAD_CASES:
        B, H, W = c.shape[:3]
        assert E.bound_wgrad(B, H, W) < E.TWO24, c.id
    for d, s, plan in E.CONV_CASES:
        K = s[3] if d == 'fwd' else s[4]
        if not E.is_wino(plan):
            assert E.bound_conv(K, s[5]) < E.TWO24
        elif E.wino_exact(plan):
            assert E.bound_wino2_conv(K) + E.PREFILL < E.TWO24
    for s in E.SWEEP_SHAPES:
        assert E.bound_conv(max(s[3], s[4]), s[5]) < E.TWO24
    for tile, s in E.WINO_WGRAD_CASES:
        du, back4 = E.bound_wino2_wgrad(E.wino_tiles(s[0], s[1], s[2], 2))
        assert du < E.TWO24 and back4 + 4 * E.PREFILL < E.TWO24
    # the bounds are bounds: the largest value of a reference stays below them
    shape = (2, 13, 13, 64, 128, 3)
    x, dy, w = E.operands(shape, *shape)
    assert int(E.ref_wgrad(dy, x, 3).abs().max()) <= E.bound_wgrad(2, 13, 13, False)
    assert int(E.ref_fwd(x, w).abs().max()) <= E.bound_conv(64, 3, prefilled=False)
    assert int(E.ref_dgrad(dy, w).abs().max()) <= E.bound_conv(128, 3, prefilled=False)


def test_fp32_winograd_f2_is_exact_on_these_operands_and_f4_is_not():
    """The transforms in fp32 with the kernels' matrices (oracle/wino_ref.py): F(2x2) reproduces the int64 result, F(4x4)
    (thirds in G) does not - why the 8xxxxxx plans and the tile-4 filter gradient stay on a tolerance."""
    from oracle import wino_ref
    shape = (2, 7, 9, 16, 24, 3)
    x, dy, w = E.operands(shape, *shape, wino=True)
    xn = x.permute(0, 3, 1, 2).numpy().astype(np.float32)
    dyn = dy.permute(0, 3, 1, 2).numpy().astype(np.float32)
    wn = w.permute(0, 3, 1, 2).numpy().astype(np.float32)
    out = E.ref_fwd(x, w).permute(0, 3, 1, 2).numpy()
    dw = E.ref_wgrad(dy, x, 3).reshape(24, 3, 3, 16).permute(0, 3, 1, 2).numpy()
    y2, g2 = wino_ref.conv3x3(xn, wn, 2), wino_ref.conv3x3_wgrad(xn, dyn, 2)
    assert y2.dtype == np.float32 and g2.dtype == np.float32
    assert np.array_equal(y2.astype(np.float64), out.astype(np.float64))
    assert np.array_equal(g2.astype(np.float64), dw.astype(np.float64))
    # the transformed F(2x2) filters are integers (multiples of 4 through two factors of 1/2)
    U = wino_ref.filter_transform(wn, 2)
    assert np.array_equal(U, np.round(U))
    y4, g4 = wino_ref.conv3x3(xn, wn, 4), wino_ref.conv3x3_wgrad(xn, dyn, 4)
    assert not np.array_equal(y4.astype(np.float64), out.astype(np.float64))
    assert not np.array_equal(g4.astype(np.float64), dw.astype(np.float64))
    assert np.abs(y4 - out).max() <= 1e-4 * np.abs(out).max() and np.abs(g4 - dw).max() <= 1e-4 * np.abs(dw).max()


# ------------------------------------------------------------------------------------------------ route coverage
def _route(lib, c):
    B, H, W, Cin, Cout, R = c.shape
    return lib.query('ssp_conv_wgrad_route', B, H, W, E.pad4(Cin), Cout, c.lddy, c.ldx, R)


def _reachable_default_routes(lib):
    """Every code the route function returns under default options, by enumeration over a grid of launch shapes."""
    chans = (4, 8, 20, 32, 36, 60, 64, 68, 96, 124, 128, 132, 252, 256, 260, 512, 1024)
    found = set()
    for Cin, Cout, W, R in itertools.product(chans, chans + (18, 70), (3, 7, 8, 13, 52), (1, 3)):
        for ldx in {Cin, Cin + 4}:
            found.add(lib.query('ssp_conv_wgrad_route', 2, 5, W, Cin, Cout, E.pad4(Cout), ldx, R))
    found.discard(0)
    return found


def test_route_query_covers_every_reachable_instantiation():
    from singleshotpose_amd import _lib
    reachable = _reachable_default_routes(_lib)
    assert len(reachable) == 7 + 9 + 1, sorted(reachable)         # LDS-direct, register-staged, the 4-channel kernel
    default_cases = [c for c in E.WGRAD_CASES if not any(k == 'wgrad_variant' for k, _ in c.opts)]
    for c in default_cases:
        assert _route(_lib, c) == c.route, (c.id, _route(_lib, c), c.route)
    covered = {c.route for c in default_cases}
    assert covered == reachable, (sorted(reachable - covered), sorted(covered - reachable))
    # each route: a plain, a ragged / sliced / accumulating and the pixel-range variants
    for name, route, base, ragged, pix in E.WGRAD_ROUTES:
        mine = [c for c in default_cases if c.route == route and c.id.startswith(name + '-')]
        assert len(mine) >= 2 + len(pix) and any(c.prefill for c in mine)
        assert any(c.lddy > E.pad4(c.shape[4]) and c.dyoff > 0 for c in mine)
        if name != 'c4':
            assert any(c.ldx > E.pad4(c.shape[3]) and c.xoff > 0 for c in mine)
            co, ci = route_tile = (E.route_fields(route)['bmo'], E.route_fields(route)['bni'])
            assert any(c.shape[4] % co and (c.shape[3] % ci or E.route_fields(route)['fold']) for c in mine), route_tile
        assert any(c.shape[0] * c.shape[1] * c.shape[2] < 16 for c in mine)
        assert any((c.shape[0] * c.shape[1] * c.shape[2]) % 16 for c in mine)
        assert any(c.shape[1] == 1 for c in mine) and any(c.shape[0] >= 2 for c in mine)
    assert any(c.shape[4] % 4 == 2 for c in default_cases)
    codes = {c.route for c in E.WGRAD_CASES}
    assert all(E.route_code(**{k: v for k, v in E.route_fields(r).items()}) == r for r in codes)


def test_route_query_follows_the_variant_option():
    from singleshotpose_amd import _lib
    cases = [c for c in E.WGRAD_CASES if any(k == 'wgrad_variant' for k, _ in c.opts)]
    assert sorted(dict(c.opts)['wgrad_variant'] for c in cases) == [2, 3, 6, 8, 10, 11, 20]
    try:
        for c in cases:
            _lib.call('ssp_set_option', b'wgrad_variant', dict(c.opts)['wgrad_variant'])
            assert _route(_lib, c) == c.route, c.id
        _lib.call('ssp_set_option', b'wgrad_variant', 1)       # no 4-channel kernel: the first layer runs 32 x 32 tiles
        assert _lib.query('ssp_conv_wgrad_route', 1, 20, 24, 4, 32, 32, 4, 3) == E.route_code(E.REG, 3, 32, 32)
    finally:
        _lib.call('ssp_set_option', b'wgrad_variant', 0)
    assert _lib.query('ssp_conv_wgrad_route', 1, 20, 24, 4, 32, 32, 4, 3) == E.route_code(E.C4, 2, 32, 4)


def test_route_query_returns_zero_for_arguments_the_launch_rejects():
    from singleshotpose_amd import _lib
    q = lambda *a: _lib.query('ssp_conv_wgrad_route', *a)
    assert q(2, 13, 13, 128, 128, 128, 128, 3) != 0
    assert q(2, 13, 13, 128, 128, 128, 128, 5) == 0 and q(2, 13, 13, 128, 128, 128, 128, 2) == 0      # R
    assert q(2, 13, 13, 126, 128, 128, 128, 3) == 0 and q(2, 13, 13, 0, 128, 128, 128, 3) == 0        # Cin % 4, Cin > 0
    assert q(2, 13, 13, 128, 128, 128, 124, 3) == 0 and q(2, 13, 13, 128, 128, 128, 130, 3) == 0      # ldx
    assert q(2, 13, 13, 128, 128, 124, 128, 3) == 0 and q(2, 13, 13, 128, 128, 130, 128, 3) == 0      # lddy
    assert q(2, 13, 13, 128, 18, 20, 128, 3) != 0 and q(2, 13, 13, 128, 18, 16, 128, 3) == 0          # lddy >= Cout
    assert q(1 << 15, 1 << 8, 1 << 8, 128, 128, 128, 128, 3) == 0                                     # 2^31 pixels
    assert q((1 << 15) - 1, 1 << 8, 1 << 8, 128, 128, 128, 128, 3) != 0
    assert q(0, 13, 13, 128, 128, 128, 128, 3) == 0 and q(2, 13, 13, 128, 0, 128, 128, 3) == 0        # nothing to do


# ------------------------------------------------------------------------------------------------ plan codes
def test_tuner_candidates_decode_to_documented_plans():
    from singleshotpose_amd import engine
    assert engine.IGEMM_CANDS and engine.IGEMM_LATENCY_CANDS and engine.WINO_GEMM_CANDS
    for code in engine.IGEMM_CANDS + engine.IGEMM_LATENCY_CANDS + engine.WINO_GEMM_CANDS:
        tail, rows, ks, slots = E.decode_plan(code)
        # include/ssp_hip.h: tile_rows 64|128, ksplit 1..9, ring_slots 3|4 or 8, tail 0 or 2..9 (hybrid: un-split main part)
        assert rows in (64, 128) and 1 <= ks <= 9 and slots in (3, 4, 8) and (tail == 0 or (2 <= tail <= 9 and ks == 1)), code
        assert tail * 100000 + rows * 100 + ks * 10 + slots == code
    assert all(E.decode_plan(c)[3] == 8 for c in engine.IGEMM_LATENCY_CANDS)
    assert all(E.decode_plan(c)[2] == 1 and E.decode_plan(c)[0] == 0 for c in engine.WINO_GEMM_CANDS)      # 9xxxxxx + rows*100 + 10 + slots
    for want in (12823, 6423, 6424, 206414, 212813, 406413, 406414, 412813):
        assert want in engine.IGEMM_CANDS
    assert 6428 in engine.IGEMM_LATENCY_CANDS and 12828 in engine.IGEMM_LATENCY_CANDS
    assert len(set(engine.IGEMM_CANDS + engine.IGEMM_LATENCY_CANDS)) == len(engine.IGEMM_CANDS) + len(engine.IGEMM_LATENCY_CANDS)

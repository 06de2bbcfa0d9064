"""The convolution family on exact-integer operands (tests/exact_conv.py): every filter-gradient instantiation the route
query can name, the operand forms the engine passes (channel slices of wider buffers, in-place accumulation, ragged
channel tiles, short and odd pixel ranges), the forced splits and A/B variants of the LDS-direct kernel, the Winograd
filter gradient, forward / data-gradient launches on slices with accumulation, and every plan code the tuner hands out.

All operands are small integers, so every partial sum is an exactly representable integer whatever the order it is formed
in (test_exact_conv_cpu.py pins the bounds): each comparison is torch.equal against an int64 reference - except the
Winograd F(4x4) forms, whose G matrix holds thirds; they run on the same data at the 1e-4 bar of the other kernel tests."""
import contextlib
import functools

import pytest
import torch

import exact_conv as E
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAN = float('nan')


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


@contextlib.contextmanager
def _options(_lib, opts):
    """Experiment knobs of the library for the launches inside; every one back to 0 afterwards."""
    try:
        for k, v in opts:
            _lib.call('ssp_set_option', k.encode(), v)
        yield
    finally:
        for k in ('wgrad_variant', 'wgrad_split'):
            _lib.call('ssp_set_option', k.encode(), 0)


def _assert_equal(got, want, names):
    assert torch.equal(got, want), E.first_diffs(got, want, names)


# ------------------------------------------------------------------------------------------------ direct filter gradient
@pytest.mark.parametrize("c", E.WGRAD_CASES, ids=lambda c: c.id)
def test_wgrad_every_route_exact(c):
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    cinp = E.pad4(Cin)
    x, dy, _ = E.operands(c.shape, *c.shape)
    ref = E.ref_wgrad(dy, x, R)                                      # [Cout][R*R][cinp]
    pre = E.prefill(c.shape, ref.shape) if c.prefill else torch.zeros_like(ref)
    xd = E.nhwc_buffer(x, c.ldx, c.xoff).to(G.dev())
    dyd = E.nhwc_buffer(dy, c.lddy, c.dyoff).to(G.dev())
    dw = pre.float().to(G.dev())
    with _options(_lib, c.opts):
        route = _lib.query('ssp_conv_wgrad_route', B, H, W, cinp, Cout, c.lddy, c.ldx, R)
        assert route == c.route, (route, c.route)                    # the kernel this case is about is the one that runs
        _lib.call('ssp_conv_wgrad', G.p(dyd, c.dyoff), G.p(xd, c.xoff), dw.data_ptr(), B, H, W, cinp, Cout, c.lddy, c.ldx, R,
                  G.stream())
        torch.cuda.synchronize()
    _assert_equal(dw.cpu(), (ref + pre).float(), ('co', 'tap', 'ci'))


# ------------------------------------------------------------------------------------------------ Winograd filter gradient
@pytest.mark.parametrize("tile,shape", E.WINO_WGRAD_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_wino_wgrad_sliced_accumulating(tile, shape):
    """ssp_conv_wgrad_wino_t on channel slices (ldx > Cin, lddy > Cout) into a non-zero dw with a NaN-poisoned workspace:
    tile 2 (transforms through HBM) and 12 (on the chip) bit for bit, tile 4 on the same inputs at 1e-4."""
    G, _lib = _imports()
    B, H, W, Cin, Cout = shape
    s6 = shape + (3,)
    x, dy, _ = E.operands(s6, *s6)
    ref = E.ref_wgrad(dy, x, 3)
    pre = E.prefill(s6, ref.shape)
    ldx, xoff, lddy, dyoff = Cin + 16, 8, Cout + 12, 4
    xd = E.nhwc_buffer(x, ldx, xoff).to(G.dev())
    dyd = E.nhwc_buffer(dy, lddy, dyoff).to(G.dev())
    dw = pre.float().to(G.dev())
    wsn = _lib.query('ssp_conv_wgrad_wino_workspace_floats_t', B, H, W, Cin, Cout, tile)
    ws = torch.full((max(1, wsn),), NAN, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_conv_wgrad_wino_t', G.p(dyd, dyoff), G.p(xd, xoff), dw.data_ptr(), B, H, W, Cin, Cout, lddy, ldx, tile,
              ws.data_ptr(), wsn, G.stream())
    torch.cuda.synchronize()
    got, want = dw.cpu(), (ref + pre).float()
    if tile == 4:
        err = rel_err(got.numpy(), want.numpy())
        print('F(4x4) filter gradient vs int64: %.2e' % err)
        assert err < TOL
    else:
        _assert_equal(got, want, ('co', 'tap', 'ci'))


# ------------------------------------------------------------------------------------------------ forward / data gradient
def _conv_call(_lib, G, direction, inp, inoff, wt, out, outoff, B, H, W, K, N, ldin, ldout, R, accumulate, plan, ws, wsn):
    if direction == 'fwd':
        _lib.call('ssp_conv_fwd', G.p(inp, inoff), wt.data_ptr(), G.p(out, outoff), None, None, B, H, W, K, N, ldin, ldout, R,
                  accumulate, plan, ws.data_ptr(), wsn, G.stream())
    else:
        _lib.call('ssp_conv_dgrad', G.p(inp, inoff), wt.data_ptr(), G.p(out, outoff), B, H, W, K, N, ldin, ldout, R, accumulate,
                  plan, ws.data_ptr(), wsn, G.stream())


def _conv_operands(direction, shape, wino):
    """(input map, packed filter [N][R*R][Kp], reference [B,H,W,N]) of a forward or data-gradient launch, int64."""
    x, dy, w = E.operands(shape, *shape, wino=wino)
    if direction == 'fwd':
        return x, E.pack_fwd(w), E.ref_fwd(x, w)
    return dy, E.pack_dgrad(w), E.ref_dgrad(dy, w)


@pytest.mark.parametrize("case", E.CONV_CASES, ids=E.conv_case_id)
def test_conv_fwd_dgrad_sliced_accumulating(case):
    """Direct and Winograd plans with ldin > Cin and a sliced output: a plain launch into a NaN-filled buffer (nothing outside
    the slice is touched), then accumulate = 1 into an integer-prefilled one.  Workspaces NaN-poisoned."""
    G, _lib = _imports()
    direction, shape, plan = case
    B, H, W, Cin, Cout, R = shape
    wino, exact = E.is_wino(plan), E.wino_exact(plan)
    inp, wp, ref = _conv_operands(direction, shape, wino)
    N, Kp = wp.shape[0], wp.shape[2]
    M = B * H * W
    ref = ref.reshape(M, N)
    ldin, inoff, ldout, outoff = Kp + 16, 8, N + 12, 4
    ind = E.nhwc_buffer(inp, ldin, inoff).to(G.dev())
    wt = wp.float().to(G.dev())
    if wino:
        tile = _lib.query('ssp_conv_plan_wino_tile', plan)
        U = torch.empty((tile + 2) ** 2 * N * Kp, dtype=torch.float32, device=G.dev())
        _lib.call('ssp_wino_filter_transform_t', wt.data_ptr(), U.data_ptr(), N, Kp, tile, G.stream())
        wt = U
    wsn = max(1, _lib.query('ssp_conv_workspace_floats', B, H, W, Kp, N, R, plan))
    pre = E.prefill(shape + (plan,), ref.shape)
    for accumulate, want in ((0, ref), (1, ref + pre)):
        out = torch.full((M, ldout), NAN, dtype=torch.float32)
        if accumulate:
            out[:, outoff:outoff + N] = pre.float()
        out = out.to(G.dev())
        ws = torch.full((wsn,), NAN, dtype=torch.float32, device=G.dev())
        _conv_call(_lib, G, direction, ind, inoff, wt, out, outoff, B, H, W, Kp, N, ldin, ldout, R, accumulate, plan, ws, wsn)
        torch.cuda.synchronize()
        o = out.cpu()
        assert torch.isnan(o[:, :outoff]).all() and torch.isnan(o[:, outoff + N:]).all(), "wrote outside its channel slice"
        got = o[:, outoff:outoff + N].contiguous()
        if exact:
            _assert_equal(got, want.float(), ('pixel', 'channel'))
        else:
            err = rel_err(got.numpy(), want.float().numpy())
            print('F(4x4) %s (accumulate %d) vs int64: %.2e' % (direction, accumulate, err))
            assert err < TOL


# ------------------------------------------------------------------------------------------------ plan sweep
@functools.lru_cache(maxsize=2)
def _sweep_operands(shape):
    return E.operands(shape, *shape)


@pytest.mark.parametrize("direction", ['fwd', 'dgrad'])
@pytest.mark.parametrize("shape", E.SWEEP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_tuner_plan_code_exact(shape, direction):
    """Every direct plan code Plan._autotune hands out (tile rows x split-K x ring depth, hybrid tails, the latency ring),
    forward and data gradient: NaN-filled output, NaN-poisoned workspace, torch.equal against the plan-0 output of the same
    launch - a code select_plan declines falls back to the heuristic and must be equal too - and plan 0 against int64."""
    G, _lib = _imports()
    from singleshotpose_amd import engine
    B, H, W, Cin, Cout, R = shape
    M, HW = B * H * W, H * W
    x, dy, w = _sweep_operands(shape)
    inp, wp = (x, E.pack_fwd(w)) if direction == 'fwd' else (dy, E.pack_dgrad(w))
    N, Kp = wp.shape[0], wp.shape[2]
    ind = E.nhwc_buffer(inp).to(G.dev())
    wt = wp.float().to(G.dev())
    base, bad = None, []
    for code in (0,) + engine.IGEMM_CANDS + engine.IGEMM_LATENCY_CANDS:
        wsn = max(1, _lib.query('ssp_conv_workspace_floats', B, H, W, Kp, N, R, code))
        ws = torch.full((wsn,), NAN, dtype=torch.float32, device=G.dev())
        out = torch.full((M, N), NAN, dtype=torch.float32, device=G.dev())
        _conv_call(_lib, G, direction, ind, 0, wt, out, 0, B, H, W, Kp, N, Kp, N, R, 0, code, ws, wsn)
        torch.cuda.synchronize()
        if code == 0:
            base = out
        elif not torch.equal(out, base):
            bad.append((code, E.first_diffs(out.cpu(), base.cpu(), ('pixel', 'channel'))))
        del ws
    assert not bad, bad
    got = base.cpu()
    for img in E.sweep_ref_images(B):
        ref = (E.ref_fwd(x[img:img + 1], w) if direction == 'fwd' else E.ref_dgrad(dy[img:img + 1], w)).reshape(HW, N)
        assert torch.equal(got[img * HW:(img + 1) * HW], ref.float()), \
            'image %d: %s' % (img, E.first_diffs(got[img * HW:(img + 1) * HW], ref.float(), ('pixel', 'channel')))

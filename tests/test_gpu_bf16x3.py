"""The bf16x3 split-MFMA convolution (csrc/conv_igemm_bf16x3.hip, plan codes 6xxxxxx) on the GPU.

Bit for bit against int64 on the exact-integer operands of tests/exact_bf16x3.py - three classes that together need each
of the six evaluated products (tests/test_bf16x3_cpu.py pins that), so a kernel with a product missing, a term misplaced
or a plane misread cannot pass - over the smallest shapes that reach every path of the kernel and of the shared epilogue;
misfits are errors; accuracy on random operands against float64 and against the fp32 kernel; and the mode through the
engine (Darknet.conv_math)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_bf16x3 as X
import exact_conv as E
from helpers import rel_err

pytestmark = pytest.mark.gpu
NAN = float('nan')
BMS = (64, 128)


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


def _assert_equal(got, want, what):
    assert torch.equal(got, want), '%s: %s' % (what, E.first_diffs(got, want, ('pixel', 'channel')))


@functools.lru_cache(maxsize=None)
def _case(cls, case):
    """(input map int64 [B,H,W,K], packed filter int64 [N][R*R][K], int64 reference [M][N]) - computed once per case."""
    B, H, W, K, N, R = case
    inp, w = X.operands(cls, case, *case)
    return inp, w, X.conv(inp, w, R).reshape(B * H * W, N)


def _launch(_lib, G, direction, ind, inoff, wt, out, outoff, shape, ldin, ldout, accumulate, plan, ws, bias=None):
    B, H, W, K, N, R = shape
    wsp, wsn = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    if direction == 'fwd':
        _lib.call('ssp_conv_fwd', G.p(ind, inoff), wt.data_ptr(), G.p(out, outoff), bias, None, B, H, W, K, N, ldin, ldout, R,
                  accumulate, plan, wsp, wsn, G.stream())
    else:
        _lib.call('ssp_conv_dgrad', G.p(ind, inoff), wt.data_ptr(), G.p(out, outoff), B, H, W, K, N, ldin, ldout, R, accumulate,
                  plan, wsp, wsn, G.stream())


def _workspace(_lib, G, shape, plan):
    n = _lib.query('ssp_conv_workspace_floats', *(shape + (plan,)))
    return torch.full((n,), NAN, dtype=torch.float32, device=G.dev()) if n else None


# ------------------------------------------------------------------------------------------------ exact, every path
@pytest.mark.parametrize("direction", ['fwd', 'dgrad'])
@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_exact_on_every_class(case, direction):
    """Forward and data-gradient entry points, both tile heights, the three operand classes: channel slices of wider,
    NaN-poisoned buffers (ldin > K, ldout > N), a plain launch into NaN and an accumulating one onto an integer prefill."""
    G, _lib = _imports()
    B, H, W, K, N, R = case
    M = B * H * W
    ldin, inoff, ldout, outoff = K + 16, 8, N + 12, 4
    for cls in X.CLASSES:
        inp, w, ref = _case(cls, case)
        ind = E.nhwc_buffer(inp, ldin, inoff).to(G.dev())
        wt = w.float().to(G.dev())
        pre = E.prefill(case + (X.CLASSES.index(cls),), ref.shape)
        for bm in BMS:
            plan = X.plan_code(bm)
            assert _lib.query('ssp_conv_bf16x3_fits', *(case + (plan,))) == 1
            for accumulate, want in ((0, ref), (1, ref + pre)):
                out = torch.full((M, ldout), NAN, dtype=torch.float32)
                if accumulate:
                    out[:, outoff:outoff + N] = pre.float()
                out = out.to(G.dev())
                _launch(_lib, G, direction, ind, inoff, wt, out, outoff, case, ldin, ldout, accumulate, plan, None)
                torch.cuda.synchronize()
                o = out.cpu()
                assert torch.isnan(o[:, :outoff]).all() and torch.isnan(o[:, outoff + N:]).all(), "wrote outside its slice"
                _assert_equal(o[:, outoff:outoff + N].contiguous(), want.float(), '%s bm %d acc %d' % (cls, bm, accumulate))


SPLIT_CASES = [(3, 9, 11, 48, n, 3) for n in X.NS]       # 27 K-steps: splits of 2 (14 + 13) and 3 (9 each)


@pytest.mark.parametrize("direction", ['fwd', 'dgrad'])
@pytest.mark.parametrize("case", SPLIT_CASES, ids=X.case_id)
def test_exact_split_k(case, direction):
    """Split-K 2 and 3: partial tiles through a NaN-poisoned workspace, finished by the reduce pass - plain, and with a
    bias on an accumulating launch (forward)."""
    G, _lib = _imports()
    B, H, W, K, N, R = case
    M = B * H * W
    bias_i = torch.from_numpy(X.rng(7, N).randint(-4, 5, (N,)).astype(np.int64))
    bias = bias_i.float().to(G.dev())
    for cls in X.CLASSES:
        inp, w, ref = _case(cls, case)
        ind = E.nhwc_buffer(inp).to(G.dev())
        wt = w.float().to(G.dev())
        pre = E.prefill(case + (5,), ref.shape)
        for bm in BMS:
            for ks in (2, 3):
                plan = X.plan_code(bm, ks)
                assert _lib.query('ssp_conv_workspace_floats', *(case + (plan,))) == ks * M * N
                out = torch.full((M, N), NAN, dtype=torch.float32, device=G.dev())
                _launch(_lib, G, direction, ind, 0, wt, out, 0, case, K, N, 0, plan, _workspace(_lib, G, case, plan))
                torch.cuda.synchronize()
                _assert_equal(out.cpu(), ref.float(), '%s bm %d split %d' % (cls, bm, ks))
                if direction == 'fwd':
                    out = pre.float().to(G.dev())
                    _launch(_lib, G, direction, ind, 0, wt, out, 0, case, K, N, 1, plan, _workspace(_lib, G, case, plan),
                            bias.data_ptr())
                    torch.cuda.synchronize()
                    _assert_equal(out.cpu(), (ref + bias_i[None, :] + pre).float(), '%s bm %d split %d bias+acc' % (cls, bm, ks))
                with pytest.raises(_lib.SspError):           # a split launch without its workspace is an error
                    _launch(_lib, G, direction, ind, 0, wt, out, 0, case, K, N, 0, plan, None)


AFFINE_CASES = [(2, 5, 7, 16, 68, 3), (3, 9, 11, 48, 132, 1), (3, 9, 11, 16, 64, 3)]


@pytest.mark.parametrize("case", AFFINE_CASES, ids=X.case_id)
def test_exact_bias_and_affine(case):
    """ssp_conv_fwd with a bias, and the eval block ssp_conv_fwd_affine: per-channel scale +-1 / +-2, integer shift, slope 1
    and 1/2 - every result a half-integer below 2^23, so still exact."""
    G, _lib = _imports()
    B, H, W, K, N, R = case
    M = B * H * W
    rs = X.rng(11, N)
    scale_i = torch.from_numpy(rs.choice(np.asarray([-2, -1, 1, 2], dtype=np.int64), N))
    shift_i = torch.from_numpy(rs.randint(-4, 5, (N,)).astype(np.int64))
    scale, shift = scale_i.float().to(G.dev()), shift_i.float().to(G.dev())
    for cls in X.CLASSES:
        inp, w, ref = _case(cls, case)
        assert 2 * X.abs_bound(inp, w, R) + 4 < E.TWO24
        ind = E.nhwc_buffer(inp).to(G.dev())
        wt = w.float().to(G.dev())
        for bm in BMS:
            plan = X.plan_code(bm)
            out = torch.full((M, N), NAN, dtype=torch.float32, device=G.dev())
            _launch(_lib, G, 'fwd', ind, 0, wt, out, 0, case, K, N, 0, plan, None, shift.data_ptr())
            torch.cuda.synchronize()
            _assert_equal(out.cpu(), (ref + shift_i[None, :]).float(), '%s bm %d bias' % (cls, bm))
            for slope in (1.0, 0.5):
                out = torch.full((M, N), NAN, dtype=torch.float32, device=G.dev())
                _lib.call('ssp_conv_fwd_affine', ind.data_ptr(), wt.data_ptr(), out.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                          slope, B, H, W, K, N, K, N, R, plan, None, 0, G.stream())
                torch.cuda.synchronize()
                v = (ref * scale_i[None, :] + shift_i[None, :]).double()
                want = torch.where(v > 0, v, v * slope).float()
                _assert_equal(out.cpu(), want, '%s bm %d affine slope %g' % (cls, bm, slope))


# ------------------------------------------------------------------------------------------------ statistics, fused sums
@pytest.mark.parametrize("case", [(3, 9, 11, 48, 132, 3), (3, 9, 11, 48, 64, 3), (2, 5, 7, 16, 68, 1)], ids=X.case_id)
def test_bn_statistics_match_plan0(case):
    """Per-tile (mean, M2) partials of a bf16x3 launch (tile epilogue, and the reduce pass of a split launch), finalized by
    ssp_bn_fwd_finalize, against plan 0's on the same integer operands (the raw maps are equal bit for bit; the tilings
    differ) - at the tolerance of the existing statistics tests (rtol 1e-4, atol 1e-5)."""
    G, _lib = _imports()
    B, H, W, K, N, R = case
    M = B * H * W
    inp, w, ref = _case('x2w2', case)
    ind = E.nhwc_buffer(inp).to(G.dev())
    wt = w.float().to(G.dev())

    def finalized(plan):
        tile_m = _lib.query('ssp_conv_stats_tile_m', *(case + (plan,)))
        ntile = _lib.query('ssp_conv_stats_tiles', *(case + (plan,)))
        stats = torch.full((_lib.query('ssp_conv_stats_floats', *(case + (plan,))),), NAN, dtype=torch.float32, device=G.dev())
        out = torch.full((M, N), NAN, dtype=torch.float32, device=G.dev())
        ws = _workspace(_lib, G, case, plan)
        _lib.call('ssp_conv_fwd', ind.data_ptr(), wt.data_ptr(), out.data_ptr(), None, stats.data_ptr(), B, H, W, K, N, K, N, R,
                  0, plan, ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, G.stream())
        vec = torch.zeros(4, N, device=G.dev())
        ones, zeros = torch.ones(N, device=G.dev()), torch.zeros(N, device=G.dev())
        rm, rv = torch.zeros(N, device=G.dev()), torch.ones(N, device=G.dev())
        _lib.call('ssp_bn_fwd_finalize', stats.data_ptr(), ntile, tile_m, M, N, ones.data_ptr(), zeros.data_ptr(), rm.data_ptr(),
                  rv.data_ptr(), 1.0, 0.0, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), G.stream())
        torch.cuda.synchronize()
        return out.cpu(), vec[0].cpu().numpy(), vec[1].cpu().numpy(), rv.cpu().numpy()

    base = finalized(0)
    _assert_equal(base[0], ref.float(), 'plan 0')
    m64 = ref.double().numpy()
    np.testing.assert_allclose(base[1], m64.mean(axis=0), rtol=1e-4, atol=1e-5)
    splits = (1, 3) if R * R * K // 16 >= 24 else (1,)
    for bm in BMS:
        for ks in splits:
            got = finalized(X.plan_code(bm, ks))
            _assert_equal(got[0], ref.float(), 'bm %d split %d' % (bm, ks))
            for a, b in zip(got[1:], base[1:]):
                np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("case", [(3, 9, 11, 48, 132, 3), (3, 9, 11, 48, 64, 3), (2, 5, 7, 16, 68, 1)], ids=X.case_id)
def test_fused_bn_backward_sums_match_plan0(case):
    """ssp_conv_dgrad_bnbwd under a bf16x3 code: the gradient bit for bit, and the (sum dy', sum dy' * xhat) rows, summed
    over the tiles, equal to plan 0's.  One-term operands and BatchNorm vectors on dyadic grids keep every sum an exact
    fp32 (|g| <= 432 * 6 on a grid of 1/2, |xhat| <= 8, 297 pixels), so the comparison is torch.equal."""
    G, _lib = _imports()
    B, H, W, K, N, R = case
    M = B * H * W
    rs = X.rng(13, *case)
    inp = torch.from_numpy(rs.randint(-E.XMAX, E.XMAX + 1, (B, H, W, K)).astype(np.int64))
    w = torch.from_numpy(rs.randint(-E.WMAX, E.WMAX + 1, (N, R * R, K)).astype(np.int64))
    ref = X.conv(inp, w, R).reshape(M, N)
    raw = torch.from_numpy(rs.randint(-3, 4, (M, N)).astype(np.float32))
    mean = torch.from_numpy(rs.choice([-1.0, 0.0, 1.0], N).astype(np.float32))
    istd = torch.from_numpy(rs.choice([1.0, 2.0], N).astype(np.float32))
    scale = torch.from_numpy(rs.choice([-1.0, 1.0, 2.0], N).astype(np.float32))
    shift = torch.from_numpy(rs.choice([-0.5, 0.25, 1.0], N).astype(np.float32))
    SLOPE = 0.5                                                    # dy' on a grid of 1/2, xhat an integer, |xhat| <= 8
    assert R * R * K * E.XMAX * E.WMAX * 8 * M * 2 < E.TWO24
    dev = lambda t: t.to(G.dev())
    ind, wt, rawd = dev(E.nhwc_buffer(inp)), dev(w.float()), dev(raw)
    vec = [dev(t) for t in (scale, shift, mean, istd)]

    def run(plan):
        tm = _lib.query('ssp_conv_stats_tile_m', *(case + (plan,)))
        ntile = _lib.query('ssp_conv_stats_tiles', *(case + (plan,)))
        assert ntile == (M + tm - 1) // tm
        partial = torch.zeros(ntile * N * 2, device=G.dev())
        gx = torch.full((M, N), NAN, dtype=torch.float32, device=G.dev())
        ws = _workspace(_lib, G, case, plan)
        _lib.call('ssp_conv_dgrad_bnbwd', ind.data_ptr(), wt.data_ptr(), gx.data_ptr(), B, H, W, K, N, K, N, R, plan,
                  ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, rawd.data_ptr(), N,
                  vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), SLOPE, partial.data_ptr(), ntile,
                  G.stream())
        torch.cuda.synchronize()
        return gx.cpu(), partial.cpu().double().view(ntile, N, 2).sum(0)

    g0, s0 = run(0)
    _assert_equal(g0, ref.float(), 'plan 0')
    y = raw.double() * scale.double() + shift.double()
    dy = torch.where(y > 0, ref.double(), ref.double() * SLOPE)
    want = torch.stack([dy.sum(0), (dy * ((raw.double() - mean.double()) * istd.double())).sum(0)], dim=1)
    assert torch.equal(s0, want)
    splits = (1, 3) if R * R * K // 16 >= 24 else (1,)
    for bm in BMS:
        for ks in splits:
            g, s = run(X.plan_code(bm, ks))
            _assert_equal(g, ref.float(), 'bm %d split %d' % (bm, ks))
            assert torch.equal(s, s0), (bm, ks, float((s - s0).abs().max()))


# ------------------------------------------------------------------------------------------------ misfits
def test_a_code_that_does_not_fit_is_an_error_and_writes_nothing():
    """Every misfit row of the table, on both entry points, and an unaligned operand: SSP_ERR_ARG with a message, the
    NaN-filled output untouched - never a quiet run of the fp32 kernel under a bf16x3 code."""
    G, _lib = _imports()
    rows = list(X.MISFIT_LAUNCHES)
    assert len(rows) >= 10
    for B, H, W, K, N, R, plan in rows:
        assert _lib.query('ssp_conv_bf16x3_fits', B, H, W, K, N, R, plan) == 0
        M = B * H * W
        RR = R * R
        ind = torch.ones((M, K), dtype=torch.float32, device=G.dev())
        wt = torch.ones((N, RR, K), dtype=torch.float32, device=G.dev())
        ws = torch.full((9 * M * N,), NAN, dtype=torch.float32, device=G.dev())
        for direction in ('fwd', 'dgrad'):
            out = torch.full((M, N), NAN, dtype=torch.float32, device=G.dev())
            with pytest.raises(_lib.SspError) as e:
                _launch(_lib, G, direction, ind, 0, wt, out, 0, (B, H, W, K, N, R), K, N, 0, plan, ws)
            assert str(e.value)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()), (B, H, W, K, N, R, plan, direction)
    # operands off the 16-byte grid
    case, plan = (2, 5, 7, 16, 64, 3), X.plan_code(128)
    M = 70
    ind = torch.ones((M * 16 + 4,), dtype=torch.float32, device=G.dev())
    wt = torch.ones((64 * 9 * 16 + 4,), dtype=torch.float32, device=G.dev())
    out = torch.full((M, 64), NAN, dtype=torch.float32, device=G.dev())
    for inoff, woff in ((1, 0), (0, 1)):
        with pytest.raises(_lib.SspError):
            _lib.call('ssp_conv_fwd', G.p(ind, inoff), G.p(wt, woff), out.data_ptr(), None, None, 2, 5, 7, 16, 64, 16, 64, 3, 0, plan,
                      None, 0, G.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the adjoint entry points know no bf16x3 plan
    with pytest.raises(_lib.SspError):
        _lib.call('ssp_conv_dgrad_adj', ind.data_ptr(), wt.data_ptr(), out.data_ptr(), 2, 5, 7, 16, 64, 16, 64, 3, 0, plan, None, 0,
                  None, G.stream())


# ------------------------------------------------------------------------------------------------ accuracy
# rho: e3 <= RHO * e0.  Twice the largest e3 / e0 measured on the MI355X over the three cases below (1.038 at 256 -> 128,
# K = 2304; DESIGN.md section 3c, accuracy table): the margin is for operand seeds.
RHO = 2.0 * 1.038
ACCURACY_CASES = [(256, 128, 3), (1024, 64, 1), (32, 64, 3)]


@pytest.mark.parametrize("Cin,Cout,R", ACCURACY_CASES)
def test_accuracy_against_float64_and_the_fp32_kernel(Cin, Cout, R):
    """Uniform(-1, 1) operands, B = 1, 8 x 8, float64 reference on the CPU: e = max|out - f64| / max|f64| for the bf16x3
    kernel (e3, the worse of its two tile heights) and for plan 0 (e0) on the same operands."""
    G, _lib = _imports()
    B, H, W = 1, 8, 8
    rs = X.rng(17, Cin, Cout, R)
    x = torch.from_numpy(rs.uniform(-1, 1, (B, Cin, H, W)).astype(np.float32))
    w = torch.from_numpy(rs.uniform(-1, 1, (Cout, Cin, R, R)).astype(np.float32))
    ref = F.conv2d(x.double(), w.double(), None, padding=R // 2).numpy()
    xd, wd = G.to_nhwc(x), G.pack_fwd(w)
    shape = (B, H, W, Cin, Cout, R)

    def err(plan):
        out = torch.full((B * H * W, Cout), NAN, dtype=torch.float32, device=G.dev())
        _launch(_lib, G, 'fwd', xd, 0, wd, out, 0, shape, Cin, Cout, 0, plan, _workspace(_lib, G, shape, plan))
        torch.cuda.synchronize()
        return rel_err(G.from_nhwc(out, B, Cout, H, W).numpy(), ref)

    e0 = err(0)
    e3s = [err(X.plan_code(bm)) for bm in BMS]
    e3 = max(e3s)
    print('ACCURACY %4d -> %4d r%d  K %5d  e0 %.3e  e3 %.3e (bm 64 %.3e, bm 128 %.3e)  e3/e0 %.3f'
          % (Cin, Cout, R, Cin * R * R, e0, e3, e3s[0], e3s[1], e3 / e0))
    assert e3 <= 1e-5
    assert e3 <= RHO * e0


# ------------------------------------------------------------------------------------------------ through the engine
_CFG = """[net]
batch=4
height=32
width=32
channels=3
num_keypoints=9

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2
""" + ''.join("""
[convolutional]
batch_normalize=1
filters=%d
size=%d
stride=1
pad=1
activation=leaky
""" % fk for fk in ((64, 3), (128, 3), (64, 1), (128, 3))) + """
[convolutional]
filters=20
size=1
stride=1
pad=1
activation=linear

[region]
anchors =
classes=1
coords=18
num=1
object_scale=5
noobject_scale=0.1
class_scale=1
coord_scale=1
thresh = .6
"""
X3_LAYERS = (2, 3, 4, 5)           # 32->64, 64->128, 128->64 (1x1), 64->128; layer 0 is the first block, 6 the 128->20 head
HEAD_BAR, GRAD_BAR = 3.5e-5, 7e-5


def _range_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _engine_model(tmp_path):
    from oracle.darknet_ref import seeded_state
    from helpers import load_state_into
    from singleshotpose_amd.darknet import Darknet
    cfg = tmp_path / 'bf16x3.cfg'
    cfg.write_text(_CFG)
    model = Darknet(str(cfg))
    load_state_into(model, model.blocks, seeded_state(model.blocks, 5))
    return model.cuda()


def _step(model, x, gout):
    """One training-mode forward / backward from the same state: (head, {name: grad}, x.grad, plan)."""
    model.train()
    for p in model.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    y = model(xin)
    y.backward(gout)
    torch.cuda.synchronize()
    plan = list(model._plans.values())[-1]
    return y.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, xin.grad.detach().clone(), plan


def _bn_state(model):
    return {n: b.detach().clone() for n, b in model.named_buffers()}


def _restore(model, state):
    with torch.no_grad():
        for n, b in model.named_buffers():
            b.copy_(state[n])


def _engine_compare(model, tune):
    from singleshotpose_amd import _lib, engine
    rs = X.rng(19)
    x = torch.from_numpy(rs.uniform(0, 1, (4, 3, 32, 32)).astype(np.float32)).cuda()
    gout = torch.from_numpy(rs.standard_normal((4, 20, 16, 16)).astype(np.float32)).cuda()
    bn0 = _bn_state(model)
    model.conv_math = 'fp32'
    y0, g0, dx0, plan0 = _step(model, x, gout)
    assert plan0.conv_math == dict(mode='fp32', layers={}, head_deviation=0.0, taken_back=[])
    assert all(engine.conv_math_of(c) == 'fp32' for cs in plan0.convs.values() for c in (cs.plan_fwd, cs.plan_dgrad))
    _restore(model, bn0)
    model.conv_math = 'bf16x3'
    assert not model._plans
    y3, g3, dx3, plan3 = _step(model, x, gout)
    rec = plan3.conv_math
    assert rec['mode'] == 'bf16x3'
    e_head = _range_err(y3, y0)
    e_grads = {n: _range_err(g3[n], g0[n]) for n in g0}
    e_dx = _range_err(dx3, dx0)
    print('ENGINE tune=%d head %.3e  worst grad %.3e  dx %.3e  record %r' % (tune, e_head, max(e_grads.values()), e_dx, rec))
    assert e_head <= HEAD_BAR
    assert max(e_grads.values()) <= GRAD_BAR, e_grads
    assert e_dx <= GRAD_BAR
    return x, gout, bn0, y0, y3, plan3, rec


def test_engine_mode_substitutes_exactly_the_launches_that_fit(tmp_path, monkeypatch):
    from singleshotpose_amd import _lib, engine
    monkeypatch.setenv('SSP_AUTOTUNE', '0')
    monkeypatch.delenv('SSP_CONV_MATH', raising=False)
    model = _engine_model(tmp_path)
    x, gout, bn0, y0, y3, plan, rec = _engine_compare(model, 0)
    assert sorted(plan.convs) == [0, 2, 3, 4, 5, 6]
    fits = lambda cs, K, N: bool(_lib.query('ssp_conv_bf16x3_fits', 4, cs.H, cs.W, K, N, cs.k, X.plan_code(128)))
    for ind, cs in sorted(plan.convs.items()):
        # forward: the four launches that fit; data gradient: those of them whose OWN launch (channels swapped) fits - the
        # 32 -> 64 block's gradient has 32 output channels, which the kernel does not serve
        want_f = ind in X3_LAYERS
        want_d = ind in X3_LAYERS and cs.cin > 32
        assert want_f == (not cs.first and fits(cs, cs.cinp, cs.cout)) and want_d == (not cs.first and fits(cs, cs.coutp, cs.cin))
        assert (engine.conv_math_of(cs.plan_fwd) == 'bf16x3') == want_f, (ind, cs.plan_fwd)
        assert (engine.conv_math_of(cs.plan_dgrad) == 'bf16x3') == want_d, (ind, cs.plan_dgrad)
        if want_f:
            assert _lib.query('ssp_conv_bf16x3_fits', 4, cs.H, cs.W, cs.cinp, cs.cout, cs.k, cs.plan_fwd) == 1
    assert rec['taken_back'] == [] and sorted(rec['layers']) == list(X3_LAYERS)
    assert rec['layers'] == {i: (plan.convs[i].plan_fwd, plan.convs[i].plan_dgrad) for i in X3_LAYERS}
    assert 0.0 < rec['head_deviation'] <= HEAD_BAR
    # eval: eager, and replayed from a captured graph
    _restore(model, bn0)
    model.eval()
    with torch.no_grad():
        ye = model(x).clone()
        model.graph_inference = True
        yg = model(x).clone()
        yg2 = model(x).clone()
        model.graph_inference = False
        plan_e = list(model._plans.values())[-1]
        assert [engine.conv_math_of(plan_e.convs[i].plan_fwd) for i in sorted(plan_e.convs)] == \
            ['fp32', 'bf16x3', 'bf16x3', 'bf16x3', 'bf16x3', 'fp32']
        assert torch.equal(ye, yg) and torch.equal(yg, yg2)
        model.conv_math = 'fp32'
        ye0 = model(x).clone()
    assert 0.0 < _range_err(ye, ye0) <= HEAD_BAR
    # back to fp32: the training head bit for bit
    _restore(model, bn0)
    y0b, _, _, plan0b = _step(model, x, gout)
    assert torch.equal(y0b, y0)
    assert plan0b.conv_math['layers'] == {}


def test_engine_mode_with_the_tuner(tmp_path, monkeypatch):
    """The same comparison with the tuner on: the bf16x3 codes are timed against the fp32 codes and verified after tuning;
    whichever wins, nothing may be refused and the bars hold."""
    from singleshotpose_amd import engine
    monkeypatch.setenv('SSP_AUTOTUNE', '1')
    monkeypatch.delenv('SSP_CONV_MATH', raising=False)
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    n_rej = len(engine.TUNE_REJECTED)
    model = _engine_model(tmp_path)
    x, gout, bn0, y0, y3, plan, rec = _engine_compare(model, 1)
    assert engine.TUNE_REJECTED[n_rej:] == []
    for ind, cs in plan.convs.items():
        if ind not in X3_LAYERS:
            assert engine.conv_math_of(cs.plan_fwd) == 'fp32' and engine.conv_math_of(cs.plan_dgrad) == 'fp32'
    assert any(k[0] == 'fwd-bf16x3' for k in engine._TUNE_CACHE) and any(k[0] == 'dgrad-bf16x3' for k in engine._TUNE_CACHE)
    assert not any(engine.conv_math_of(v) == 'bf16x3' for k, v in engine._TUNE_CACHE.items() if k[0] in ('fwd', 'dgrad'))

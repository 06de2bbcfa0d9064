"""The data gradient as the adjoint of the Winograd forward map (ssp_conv_dgrad_adj; csrc/conv_wino.hip
wino_dgrad_finish_kernel) through the C ABI: against autograd of F.conv2d on the CPU (the 1e-4 bar of tests/test_gpu_wino.py)
and against the existing data gradient of the same plan; with the transformed output gradient dM handed in
(ssp_wino_outgrad_transform_t - what the filter gradient of the layer contracts too) and transformed by the launch
itself (dM = NULL); out-of-bounds canaries around every transform-domain buffer; the filter gradient fed from the same dM;
the transposed filter operand; and the engine's rule end to end (tests/test_wino_adjoint_cpu.py pins the algebra).

Run as a script (`python tests/test_gpu_wino_adjoint.py`) it is the child process of the engine test with the rule
switched off: one checked training step, its errors printed as one JSON line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, 'tests')):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from helpers import load_state_into, make_targets, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
# against ssp_conv_dgrad of the same plan: about 4x the largest float32 deviation of either form from float64 in the CPU
# simulation of both (3.2e-6 ... 5.0e-6 of the range at F(4x4))
TOL_FORMS = 2e-5
PLANS = [8006413, 8012813, 9006413]
SHAPES = [
    # B, H, W, Cin_dx, Cout_dy
    (3, 10, 7, 80, 64),       # ragged plain tiling, a partial 64-channel slab, 18 tiles at F(4x4)
    (2, 8, 12, 64, 144),      # exact tiling
    (7, 13, 13, 128, 64),     # F(4x4): 2 x 2 image mosaics, the second with one phantom image
    (4, 13, 9, 64, 128),      # F(4x4): non-square mosaic
    (1, 4, 4, 64, 64),        # F(4x4): one tile per row and column - every neighbour is absent
]
GUARD = 1 << 16               # NaN floats in front of and behind every carved buffer (many tile rows of any shape here)


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


def _tile(_lib, plan):
    return _lib.query('ssp_conv_plan_wino_tile', plan)


def _carve(G, n):
    """n floats out of the middle of a NaN-filled buffer: (whole buffer, view of the middle)."""
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=G.dev())
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_adjoint_dgrad(B, H, W, Cin, Cout, plan):
    """Plain, accumulating and with the fused BatchNorm-backward sums (the sums check of test_wino_conv_dgrad), each with dM
    from ssp_wino_outgrad_transform_t and with dM = NULL; dV / dM carved out of NaN-filled buffers and dx NaN-filled: a stray
    neighbour read poisons the result, a stray write breaks a guard."""
    G, _lib = _imports()
    tile = _tile(_lib, plan)
    P = (tile + 2) ** 2
    T = _lib.query('ssp_conv_wino_tiles', B, H, W, tile)
    rs = np.random.RandomState(Cin + Cout + H + tile)
    x = torch.from_numpy(rs.standard_normal((B, Cin, H, W)).astype(np.float32)).requires_grad_(True)
    w = torch.from_numpy((rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32))
    dy = torch.from_numpy(rs.standard_normal((B, Cout, H, W)).astype(np.float32))
    F.conv2d(x, w, None, padding=1).backward(dy)
    want = x.grad.numpy()
    dyd = G.to_nhwc(dy)
    wd = G.pack_dgrad(w, Cout)                                   # [Cin][tap, rotated][Cout]
    M = B * H * W
    Ut = torch.empty(P * Cin * Cout, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_wino_filter_transform_adj_t', wd.data_ptr(), Ut.data_ptr(), Cin, Cout, tile, G.stream())
    # the existing form of the same plan
    Ud = torch.empty(P * Cin * Cout, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_wino_filter_transform_t', wd.data_ptr(), Ud.data_ptr(), Cin, Cout, tile, G.stream())
    wsn0 = _lib.query('ssp_conv_workspace_floats', B, H, W, Cout, Cin, 3, plan)
    ws0 = torch.empty(wsn0, dtype=torch.float32, device=G.dev())
    dx0 = torch.empty(M, Cin, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_conv_dgrad', dyd.data_ptr(), Ud.data_ptr(), dx0.data_ptr(), B, H, W, Cout, Cin, Cout, Cin, 3, 0, plan,
              ws0.data_ptr(), wsn0, G.stream())
    torch.cuda.synchronize()
    old = G.from_nhwc(dx0, B, Cin, H, W).numpy()
    # BatchNorm-backward operands of the block that produced this conv's input
    raw = torch.from_numpy(rs.standard_normal((B, Cin, H, W)).astype(np.float32))
    scale = torch.from_numpy(rs.uniform(0.5, 1.5, Cin).astype(np.float32))
    shift = torch.from_numpy(rs.standard_normal(Cin).astype(np.float32) * 0.3)
    mean = torch.from_numpy(rs.standard_normal(Cin).astype(np.float32) * 0.1)
    invstd = torch.from_numpy(rs.uniform(0.5, 2.0, Cin).astype(np.float32))
    rows = _lib.query('ssp_conv_stats_tiles', B, H, W, Cout, Cin, 3, plan)
    rawd = G.to_nhwc(raw)
    dv = [t.to(G.dev()) for t in (scale, shift, mean, invstd)]
    g64 = x.grad.double()
    yv = raw.double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    dyp = torch.where(yv > 0, g64, g64 * 0.1)
    xhat = (raw.double() - mean.double()[None, :, None, None]) * invstd.double()[None, :, None, None]
    s1, s2 = dyp.sum(dim=(0, 2, 3)).numpy(), (dyp * xhat).sum(dim=(0, 2, 3)).numpy()

    for shared in (True, False):
        wsn = _lib.query('ssp_conv_dgrad_adj_workspace_floats', B, H, W, Cout, Cin, plan, 0 if shared else 1)
        assert wsn == P * T * (Cin + (0 if shared else Cout)) and wsn <= wsn0
        wbuf, ws = _carve(G, wsn)
        mbuf, dM = _carve(G, P * T * Cout)
        dm_ptr = None
        if shared:
            _lib.call('ssp_wino_outgrad_transform_t', dyd.data_ptr(), Cout, dM.data_ptr(), B, H, W, Cout, tile, G.stream())
            dm_ptr = dM.data_ptr()
        dx = torch.full((M, Cin), float('nan'), dtype=torch.float32, device=G.dev())
        _lib.call('ssp_conv_dgrad_adj', dyd.data_ptr(), Ut.data_ptr(), dx.data_ptr(), B, H, W, Cout, Cin, Cout, Cin, 3, 0, plan,
                  ws.data_ptr(), wsn, dm_ptr, G.stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dx).all()), "a read outside the transform-domain planes reached the result"
        assert bool(torch.isfinite(ws[:P * T * Cin]).all())
        assert _guards_intact(wbuf) and _guards_intact(mbuf)
        if shared:
            assert bool(torch.isfinite(dM).all())
        else:
            assert bool(torch.isnan(dM).all())       # not given: not touched
        got = G.from_nhwc(dx, B, Cin, H, W).numpy()
        e_ref, e_old = rel_err(got, want), rel_err(got, old)
        print('adjoint (%s dM) vs autograd %.2e (existing form %.2e), vs the existing form %.2e' % (
            'shared' if shared else 'own', e_ref, rel_err(old, want), e_old))
        assert e_ref < TOL
        assert e_old <= TOL_FORMS
        # accumulating
        _lib.call('ssp_conv_dgrad_adj', dyd.data_ptr(), Ut.data_ptr(), dx.data_ptr(), B, H, W, Cout, Cin, Cout, Cin, 3, 1, plan,
                  ws.data_ptr(), wsn, dm_ptr, G.stream())
        torch.cuda.synchronize()
        assert rel_err(G.from_nhwc(dx, B, Cin, H, W).numpy(), 2 * want) < TOL
        # fused BatchNorm-backward reductions
        part = torch.zeros(rows * Cin * 2, dtype=torch.float32, device=G.dev())
        dx2 = torch.full((M, Cin), float('nan'), dtype=torch.float32, device=G.dev())
        _lib.call('ssp_conv_dgrad_adj_bnbwd', dyd.data_ptr(), Ut.data_ptr(), dx2.data_ptr(), B, H, W, Cout, Cin, Cout, Cin, 3,
                  plan, ws.data_ptr(), wsn, rawd.data_ptr(), Cin, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(),
                  dv[3].data_ptr(), 0.1, part.data_ptr(), rows, dm_ptr, G.stream())
        torch.cuda.synchronize()
        assert rel_err(G.from_nhwc(dx2, B, Cin, H, W).numpy(), want) < TOL
        sums = part.view(rows, Cin, 2).double().sum(dim=0).cpu().numpy()
        assert rel_err(sums[:, 0], s1) < TOL and rel_err(sums[:, 1], s2) < TOL
        assert _guards_intact(wbuf) and _guards_intact(mbuf)


def test_adjoint_dgrad_refuses_other_plans():
    """Tile 12 / 7xxxxxx (the transform domain never reaches memory) and direct codes are an error, not a fallback."""
    G, _lib = _imports()
    B, H, W, Cin, Cout = 2, 8, 8, 64, 64
    z = torch.zeros(1 << 20, device=G.dev())
    for plan in (7000001, 0, 6413):
        assert _lib.query('ssp_conv_dgrad_adj_workspace_floats', B, H, W, Cout, Cin, plan, 1) == 0
        with pytest.raises(_lib.SspError):
            _lib.call('ssp_conv_dgrad_adj', z.data_ptr(), z.data_ptr(), z.data_ptr(), B, H, W, Cout, Cin, Cout, Cin, 3, 0, plan,
                      z.data_ptr(), z.numel(), None, G.stream())
    with pytest.raises(_lib.SspError):      # workspace too small for the launch's own dM
        n = _lib.query('ssp_conv_dgrad_adj_workspace_floats', B, H, W, Cout, Cin, 8006413, 0)
        _lib.call('ssp_conv_dgrad_adj', z.data_ptr(), z.data_ptr(), z.data_ptr(), B, H, W, Cout, Cin, Cout, Cin, 3, 0, 8006413,
                  z.data_ptr(), n, None, G.stream())


@pytest.mark.parametrize("tile", [2, 4])
def test_filter_gradient_from_the_shared_dm(tile):
    """ssp_wino_outgrad_transform_t into the dM slot of the filter-gradient workspace + ssp_conv_wgrad_wino_t(dy = NULL): the
    gradient of the launch that transforms dy itself, to the 1e-6 of test_wino_input_transform_alone_feeds_the_filter_gradient
    (the same fp32 atomics).  A mosaic-tiled 13 x 13 map."""
    G, _lib = _imports()
    B, H, W, Cin, Cout = 8, 13, 13, 64, 128
    rs = np.random.RandomState(6)
    xd = G.to_nhwc(torch.from_numpy(rs.standard_normal((B, Cin, H, W)).astype(np.float32)))
    dyd = G.to_nhwc(torch.from_numpy(rs.standard_normal((B, Cout, H, W)).astype(np.float32)))
    wsn = _lib.query('ssp_conv_wgrad_wino_workspace_floats_t', B, H, W, Cin, Cout, tile)
    T = _lib.query('ssp_conv_wino_tiles', B, H, W, tile)
    res = []
    for shared in (False, True):
        ws = torch.full((wsn,), float('nan'), dtype=torch.float32, device=G.dev())
        dw = torch.zeros(Cout * 9 * Cin, dtype=torch.float32, device=G.dev())
        if shared:
            _lib.call('ssp_wino_outgrad_transform_t', dyd.data_ptr(), Cout, G.p(ws, (tile + 2) ** 2 * T * Cin), B, H, W, Cout, tile,
                      G.stream())
        _lib.call('ssp_conv_wgrad_wino_t', None if shared else dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), B, H, W, Cin, Cout,
                  Cout, Cin, tile, ws.data_ptr(), wsn, G.stream())
        torch.cuda.synchronize()
        res.append(dw.cpu())
    assert torch.isfinite(res[0]).all() and float(res[0].abs().max()) > 0
    assert rel_err(res[1].numpy(), res[0].numpy()) < 1e-6


def test_filter_gradient_on_the_chip_refuses_a_missing_dy():
    G, _lib = _imports()
    B, H, W, Cin, Cout = 8, 13, 13, 64, 128
    xd = torch.zeros(B * H * W, Cin, device=G.dev())
    dw = torch.zeros(Cout * 9 * Cin, device=G.dev())
    wsn = max(1, _lib.query('ssp_conv_wgrad_wino_workspace_floats_t', B, H, W, Cin, Cout, 12))
    ws = torch.zeros(wsn, device=G.dev())
    with pytest.raises(_lib.SspError):
        _lib.call('ssp_conv_wgrad_wino_t', None, xd.data_ptr(), dw.data_ptr(), B, H, W, Cin, Cout, Cout, Cin, 12, ws.data_ptr(),
                  wsn, G.stream())


@pytest.mark.parametrize("tile", [2, 4])
def test_transposed_filter_operand_is_the_forward_transform(tile):
    """ssp_wino_filter_transform_adj_t of the ssp_repack_dgrad operand == ssp_wino_filter_transform_t of the same filters packed
    [Cin][tap][Cout] WITHOUT the rotation, bit for bit."""
    G, _lib = _imports()
    Cout, Cin = 96, 80
    rs = np.random.RandomState(tile)
    w = torch.from_numpy(rs.standard_normal((Cout, Cin, 3, 3)).astype(np.float32))
    wd = G.pack_dgrad(w, Cout)
    plain = w.permute(1, 2, 3, 0).reshape(Cin, 9, Cout).contiguous().to(G.dev())
    # (the layout's taps ARE rotated: the two operands differ)
    torch.cuda.synchronize()
    assert torch.equal(wd.view(Cin, 9, Cout).cpu(), plain.cpu().flip(1))
    n = (tile + 2) ** 2 * Cin * Cout
    a = torch.full((n,), float('nan'), dtype=torch.float32, device=G.dev())
    b = torch.full((n,), float('nan'), dtype=torch.float32, device=G.dev())
    _lib.call('ssp_wino_filter_transform_adj_t', wd.data_ptr(), a.data_ptr(), Cin, Cout, tile, G.stream())
    _lib.call('ssp_wino_filter_transform_t', plain.data_ptr(), b.data_ptr(), Cin, Cout, tile, G.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all()) and torch.equal(a.cpu(), b.cpu())


# ---------------------------------------------------------------------------------------------------- the engine's rule
def _checked_step():
    """One training step of cfg/yolo-pose.cfg at B = 8, 416 x 416 against the oracle (tests/test_gpu_fullsize.py's step)."""
    from oracle.darknet_ref import seeded_state
    from oracle.step_check import check_train_step
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.region_loss import RegionLoss
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    load_state_into(model, model.blocks, seeded_state(model.blocks, 11))
    model = model.cuda()
    rs = np.random.RandomState(8)
    x = torch.from_numpy(rs.uniform(0, 1, (8, 3, 416, 416)).astype(np.float32))
    tgt = torch.from_numpy(make_targets(rs, 8, [1, 2, 1, 3, 1, 1, 2, 1]))
    # first step: the plan tunes itself.  Which tile size wins a 13 x 13 layer's data gradient at this batch is a matter of
    # microseconds (one run measured F(2x2) on layers 18 - 22 next to an F(4x4) filter gradient: no shared dM there), so
    # the benchmark's choice - F(4x4) for both gradients of every 13 x 13 layer - is set by hand, as
    # test_backward_winograd_choices_stay_under_the_gradient_bar_when_forced does for layers 4 and 6; the rest stays tuned
    from singleshotpose_amd import _lib, engine
    crit = RegionLoss()
    crit.verbose = False
    model.train()
    crit(model(x.cuda()), tgt, 20).backward()
    plan = next(iter(model._plans.values()))
    for cs in plan.convs.values():
        if cs.k == 3 and cs.H == 13:
            cs.plan_dgrad = engine.WINO4 + 6413
            cs.wgrad_wino = 4
            cs.wino_ws_floats = _lib.query('ssp_conv_wgrad_wino_workspace_floats_t', plan.B, cs.H, cs.W, cs.cinp, cs.cout, 4)
            cs.wino_ws = None
            cs.ws_dgrad = _lib.query('ssp_conv_workspace_floats', plan.B, cs.H, cs.W, cs.coutp, cs.cin, cs.k, cs.plan_dgrad)
    plan._plan_bn_fusion()
    plan._fit_workspace()
    res = check_train_step(model, crit, x, tgt, 20)
    return model, plan, x, res


def _layers(plan):
    """{layer: (H, data-gradient plan, filter-gradient tile, adjoint form)} of the 3x3 layers behind the first."""
    return {ind: (cs.H, cs.plan_dgrad, cs.wgrad_wino, bool(cs.dgrad_adj)) for ind, cs in sorted(plan.convs.items())
            if cs.k == 3 and not cs.first}


def _slim(res):
    return {k: res[k] for k in ('head', 'loss', 'loss_gpu', 'loss_ref', 'running', 'conv', 'conv_by_layer', 'grad_out',
                                'grad_by_param')}


def _assert_step(res):
    from test_gpu_fullsize import GRAD_TOL, GRAD_TOL_FIRST_FILTER, HEAD_TOL
    assert res['head'] < HEAD_TOL, res['head']
    assert res['loss'] < TOL, (res['loss_gpu'], res['loss_ref'])
    assert res['running'] < TOL, res['running']
    assert res['conv'] < TOL, res['conv_by_layer']
    assert res['grad_out'] < TOL, res['grad_out']
    for name, err in res['grad_by_param'].items():
        assert err < (GRAD_TOL_FIRST_FILTER if name == '0.weight' else GRAD_TOL), \
            sorted(res['grad_by_param'].items(), key=lambda kv: -kv[1])[:5]


@pytest.fixture(scope='module')
def stepped():
    assert os.environ.get('SSP_WINO_SHARE_DM', '1') != '0'
    return _checked_step()


def test_engine_step_with_the_rule_on(stepped):
    from singleshotpose_amd import engine
    model, plan, x, res = stepped
    lay = _layers(plan)
    print('3x3 layers (H, dgrad plan, wgrad tile, adjoint): %s' % lay)
    print('worst grads %s' % sorted(res['grad_by_param'].items(), key=lambda kv: -kv[1])[:3])
    _assert_step(res)
    for ind, (H, code, wt, adj) in lay.items():      # the rule, restated
        t = engine.wino_tile(code)
        cs = plan.convs[ind]
        assert adj == bool(t and not engine.wino_fused(code) and wt == t and cs.coutp == cs.cout), (ind, lay[ind])
    deep = [ind for ind, v in lay.items() if v[0] == 13]
    assert deep and all(lay[ind][3] for ind in deep), lay


def test_engine_step_with_the_rule_off_in_a_child_process():
    env = dict(os.environ, SSP_WINO_SHARE_DM='0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"adjoint"')][-1])
    assert out['adjoint'] == []
    _assert_step(out['res'])


def test_engine_frozen_trunk_transforms_dy_in_the_launch(stepped, monkeypatch):
    """Head only trainable, input gradient wanted: the trunk's filter gradients do not run, so the adjoint-form layers get
    dM = NULL.  The step's dL/dx against the all-trainable step's (which shares dM with the filter gradients): the same
    arithmetic up to the order of the BatchNorm-backward sums - 1e-5 of the range, the bar verify-after-tune uses for
    results that differ in fp32 summation order only."""
    from singleshotpose_amd import _lib
    model, plan, x, _ = stepped
    model.train()
    adj = [ind for ind, v in _layers(plan).items() if v[3]]
    assert adj
    log = []
    orig = _lib.call

    def rec(name, *args):
        log.append((name, args))
        return orig(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)

    def step():
        del log[:]
        model.zero_grad(set_to_none=True)
        xi = x.cuda().requires_grad_(True)
        y = model(xi)
        g = torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(y.shape)).astype(np.float32)).cuda()
        (y * g).sum().backward()
        torch.cuda.synchronize()
        calls = [(n, a) for n, a in log if n in ('ssp_conv_dgrad_adj', 'ssp_conv_dgrad_adj_bnbwd')]
        return xi.grad.detach().cpu().numpy(), calls, sum(n == 'ssp_wino_outgrad_transform_t' for n, _ in log)

    dx_all, calls, ntr = step()
    assert len(calls) == len(adj) == ntr and all(a[-2] is not None for _, a in calls)
    last = max(plan.convs)
    for ind in plan.convs:
        if ind != last:
            for p in model.models[ind].parameters():
                p.requires_grad_(False)
    try:
        dx_frozen, calls, ntr = step()
    finally:
        for p in model.parameters():
            p.requires_grad_(True)
    n_own = sum(a[-2] is None for _, a in calls)
    print('frozen trunk: %d adjoint launches, %d with their own dM; dL/dx vs the all-trainable step %.2e' % (
        len(calls), n_own, rel_err(dx_frozen, dx_all)))
    assert len(calls) == len(adj) and ntr <= 1 and n_own >= len(adj) - 1      # (the head is the one trainable layer)
    assert np.isfinite(dx_frozen).all() and rel_err(dx_frozen, dx_all) <= 1e-5


if __name__ == '__main__':
    _, plan_, _, res_ = _checked_step()
    print(json.dumps({'adjoint': [i for i, v in _layers(plan_).items() if v[3]], 'res': _slim(res_)}, default=float))

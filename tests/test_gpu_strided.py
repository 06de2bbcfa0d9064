"""Stride-2 convolutions on the MI355X: the three entry points of csrc/conv_strided.hip on exact-integer operands
(tests/strided_cases.py: torch.equal against int64 references, BatchNorm statistics included), their argument checks,
and a small residual network with three downsampling blocks through engine.Plan against oracle/darknet_ref.py."""
import functools
import os

import numpy as np
import pytest
import torch

import exact_conv as E
import strided_cases as S
from helpers import rel_err

pytestmark = pytest.mark.gpu
NAN = float('nan')
EPS32 = float(np.finfo(np.float32).eps)


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


@functools.lru_cache(maxsize=None)
def _data(c):
    """Operands and int64 references of a case, computed once and shared (never modified) by the tests below."""
    B, H, W, Cin, Cout, R = c.shape
    x, dy, w = S.operands(c.shape)
    if c is S.DGRAD_UNSPLIT or isinstance(c, S.DgradPad):
        return dict(dy=dy, w=w, dgrad=S.ref_dgrad(dy, w, H, W))
    return dict(x=x, dy=dy, w=w, fwd=S.ref_fwd(x, w), dgrad=S.ref_dgrad(dy, w, H, W), wgrad=S.ref_wgrad(dy, x, R))


def _assert_equal(got, want, names):
    assert torch.equal(got, want), E.first_diffs(got, want, names)


def _untouched(buf, before, lo, hi):
    """Columns outside [lo, hi) of a [rows][ld] buffer hold the bits they held before the launch (NaN included)."""
    a, b = buf.cpu().view(torch.int32), before.cpu().view(torch.int32)
    return torch.equal(a[:, :lo], b[:, :lo]) and torch.equal(a[:, hi:], b[:, hi:])


# ------------------------------------------------------------------------------------------------ forward + statistics
@pytest.mark.parametrize('c', S.CASES, ids=S.case_id)
def test_forward_exact_with_statistics(c):
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    Ho, Wo = S.out_hw(H, W, R)
    d = _data(c)
    ldx, ldy, off = S.buffers(c)
    xd = E.nhwc_buffer(d['x'], ldx, off).to(G.dev())
    wd = E.pack_fwd(d['w']).float().to(G.dev())
    M = B * Ho * Wo
    out = torch.full((M, ldy), NAN, dtype=torch.float32, device=G.dev())
    before = out.clone()
    cinp = E.pad4(Cin)
    tile_m = _lib.query('ssp_conv_s2_stats_tile_m', B, H, W, cinp, Cout, R)
    ntile = _lib.query('ssp_conv_s2_stats_tiles', B, H, W, cinp, Cout, R)
    assert tile_m in (64, 128) and ntile == (M + tile_m - 1) // tile_m
    stats = torch.full((ntile * Cout * 2,), NAN, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_conv_s2_fwd', G.p(xd, off), wd.data_ptr(), G.p(out, off), None, stats.data_ptr(), B, H, W, cinp, Cout,
              ldx, ldy, R, 0, G.stream())
    torch.cuda.synchronize()
    want = d['fwd'].reshape(M, Cout).float()
    _assert_equal(out.cpu()[:, off:off + Cout], want, ('pixel', 'co'))
    assert _untouched(out, before, off, off + Cout)
    # accumulate + bias on top of an integer prefill
    pre = E.prefill(c.shape, (M, Cout))
    bias = torch.arange(Cout, dtype=torch.float32) - 3
    out2 = torch.full((M, ldy), NAN, dtype=torch.float32)
    out2[:, off:off + Cout] = pre.float()
    out2 = out2.to(G.dev())
    bd = bias.to(G.dev())
    _lib.call('ssp_conv_s2_fwd', G.p(xd, off), wd.data_ptr(), G.p(out2, off), bd.data_ptr(), None, B, H, W, cinp, Cout, ldx,
              ldy, R, 1, G.stream())
    torch.cuda.synchronize()
    _assert_equal(out2.cpu()[:, off:off + Cout], want + bias + pre.float(), ('pixel', 'co'))
    # BatchNorm statistics through the finalize, against the exact mean and (biased) variance.  eps = 1 keeps
    # var = 1 / invstd^2 - 1 well conditioned down to var = 0 (the single-pixel case).
    vec = torch.zeros(4, Cout, dtype=torch.float32, device=G.dev())
    gamma, beta = torch.ones(Cout, device=G.dev()), torch.zeros(Cout, device=G.dev())
    rm, rv = torch.zeros(Cout, device=G.dev()), torch.ones(Cout, device=G.dev())
    _lib.call('ssp_bn_fwd_finalize', stats.data_ptr(), ntile, tile_m, M, Cout, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
              rv.data_ptr(), 0.1, 1.0, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), G.stream())
    torch.cuda.synchronize()
    r64 = d['fwd'].reshape(M, Cout).double()
    mean, var = r64.mean(0), r64.var(0, unbiased=False)
    A = float(r64.abs().max())
    got_mean = vec[0].cpu().double()
    got_var = 1.0 / vec[1].cpu().double() ** 2 - 1.0
    # fp32 rounding of the two quantities: a lane sums <= 32 squared deviations, the Chan combines add <= ~30 levels
    # (lane halves, waves, tiles), each step rounds once relative to a quantity bounded by A (mean) or A^2 (variance);
    # reading the variance back out of invstd adds ~4 roundings relative to var + 1
    err_mean, err_var = float((got_mean - mean).abs().max()), float((got_var - var).abs().max())
    tol_mean, tol_var = 16 * EPS32 * max(A, 1.0), 64 * EPS32 * max(A * A, 1.0) + 4 * EPS32 * float(var.max() + 1.0)
    print('statistics: mean err %.3g (bar %.3g), var err %.3g (bar %.3g)' % (err_mean, tol_mean, err_var, tol_var))
    assert err_mean <= tol_mean and err_var <= tol_var


def test_forward_affine_epilogue():
    """The eval-mode epilogue leaky(scale * conv + shift): dyadic scale / shift keep every value exact."""
    G, _lib = _imports()
    c = S.CASES[2]
    B, H, W, Cin, Cout, R = c.shape
    Ho, Wo = S.out_hw(H, W, R)
    d = _data(c)
    M = B * Ho * Wo
    xd = E.nhwc_buffer(d['x']).to(G.dev())
    wd = E.pack_fwd(d['w']).float().to(G.dev())
    scale = torch.tensor([(-2.0, 0.5, 1.0, 0.0)[i % 4] for i in range(Cout)])
    shift = torch.tensor([float(i % 5 - 2) for i in range(Cout)])
    out = torch.full((M, E.pad4(Cout)), NAN, dtype=torch.float32, device=G.dev())
    sd, hd = scale.to(G.dev()), shift.to(G.dev())
    _lib.call('ssp_conv_s2_fwd_affine', xd.data_ptr(), wd.data_ptr(), out.data_ptr(), sd.data_ptr(), hd.data_ptr(), 0.5,
              B, H, W, E.pad4(Cin), Cout, E.pad4(Cin), E.pad4(Cout), R, G.stream())
    torch.cuda.synchronize()
    v = d['fwd'].reshape(M, Cout).float() * scale + shift
    _assert_equal(out.cpu()[:, :Cout], torch.where(v > 0, v, v * 0.5), ('pixel', 'co'))


# ------------------------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize('accumulate', [0, 1], ids=['plain', 'acc'])
@pytest.mark.parametrize('c', S.CASES + [S.DGRAD_UNSPLIT], ids=S.case_id)
def test_data_gradient_exact(c, accumulate):
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    d = _data(c)
    ldx, ldy, off = S.buffers(c)
    dyd = E.nhwc_buffer(d['dy'], ldy, off).to(G.dev())
    wd = E.pack_dgrad(d['w']).float().to(G.dev())
    M = B * H * W
    pre = E.prefill(c.shape, (M, Cin))
    dx = torch.full((M, ldx), NAN, dtype=torch.float32)
    if accumulate:
        dx[:, off:off + Cin] = pre.float()
    dx = dx.to(G.dev())
    before = dx.clone()
    _lib.call('ssp_conv_s2_dgrad', G.p(dyd, off), wd.data_ptr(), G.p(dx, off), B, H, W, E.pad4(Cout), Cin, ldy, ldx, R,
              accumulate, G.stream())
    torch.cuda.synchronize()
    want = d['dgrad'].reshape(M, Cin).float() + (pre.float() if accumulate else 0)
    _assert_equal(dx.cpu()[:, off:off + Cin], want, ('pixel', 'ci'))
    assert _untouched(dx, before, off, off + Cin)          # a destination wider than Cin_dx keeps its other columns


# ------------------------------------------------------------------------------------------------ filter gradient
@pytest.mark.parametrize('c', S.CASES, ids=S.case_id)
def test_filter_gradient_exact(c):
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    d = _data(c)
    ldx, ldy, off = S.buffers(c)
    xd = E.nhwc_buffer(d['x'], ldx, off).to(G.dev())
    dyd = E.nhwc_buffer(d['dy'], ldy, off).to(G.dev())
    dw = torch.zeros(d['wgrad'].shape, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_conv_s2_wgrad', G.p(dyd, off), G.p(xd, off), dw.data_ptr(), B, H, W, E.pad4(Cin), Cout, ldy, ldx, R,
              G.stream())
    torch.cuda.synchronize()
    _assert_equal(dw.cpu(), d['wgrad'].float(), ('co', 'tap', 'ci'))


# ------------------------------------------------------------------------------------------------ C % 4 == 2
def _sentinel_kept(buf, lo, hi):
    """Every column outside [lo, hi) still holds S.SENTINEL."""
    b = buf.cpu()
    rest = torch.cat([b[:, :lo], b[:, hi:]], 1)
    return rest.numel() > 0 and bool((rest == S.SENTINEL).all())


@pytest.mark.parametrize('c', S.PAD_OUT, ids=S.case_id)
def test_forward_and_filter_gradient_with_padded_cout(c):
    """Cout of 18 and 6 into ldout = lddy = pad4(Cout): the forward writes Cout columns and leaves the two behind them
    alone (plain, and accumulating with a bias); the filter gradient reads dy rows of pad4(Cout) floats."""
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    Ho, Wo = S.out_hw(H, W, R)
    d = _data(c)
    ldx, ldy, off = S.buffers(c)
    assert Cout % 4 == 2 and ldy == Cout + 2 and off == 0
    M = B * Ho * Wo
    xd = E.nhwc_buffer(d['x'], ldx).to(G.dev())
    wd = E.pack_fwd(d['w']).float().to(G.dev())
    want = d['fwd'].reshape(M, Cout).float()
    cinp = E.pad4(Cin)
    ntile = _lib.query('ssp_conv_s2_stats_tiles', B, H, W, cinp, Cout, R)
    stats = torch.full((ntile * Cout * 2,), NAN, dtype=torch.float32, device=G.dev())
    out = torch.full((M, ldy), S.SENTINEL, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_conv_s2_fwd', xd.data_ptr(), wd.data_ptr(), out.data_ptr(), None, stats.data_ptr(), B, H, W, cinp, Cout,
              ldx, ldy, R, 0, G.stream())
    torch.cuda.synchronize()
    _assert_equal(out.cpu()[:, :Cout], want, ('pixel', 'co'))
    assert _sentinel_kept(out, 0, Cout)
    assert bool(torch.isfinite(stats).all())
    pre = E.prefill(c.shape, (M, Cout))
    bias = torch.arange(Cout, dtype=torch.float32) - 3
    out2 = torch.full((M, ldy), S.SENTINEL, dtype=torch.float32)
    out2[:, :Cout] = pre.float()
    out2 = out2.to(G.dev())
    bd = bias.to(G.dev())
    _lib.call('ssp_conv_s2_fwd', xd.data_ptr(), wd.data_ptr(), out2.data_ptr(), bd.data_ptr(), None, B, H, W, cinp, Cout, ldx,
              ldy, R, 1, G.stream())
    torch.cuda.synchronize()
    _assert_equal(out2.cpu()[:, :Cout], want + bias + pre.float(), ('pixel', 'co'))
    assert _sentinel_kept(out2, 0, Cout)
    # filter gradient: dy as the plan holds it, zero pad columns
    dyd = E.nhwc_buffer(d['dy'], ldy).to(G.dev())
    dw = torch.zeros(d['wgrad'].shape, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_conv_s2_wgrad', dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), B, H, W, cinp, Cout, ldy, ldx, R, G.stream())
    torch.cuda.synchronize()
    _assert_equal(dw.cpu(), d['wgrad'].float(), ('co', 'tap', 'ci'))
    # ... and as the source of a data gradient: Cout_dy = the padded count
    dx = torch.full((B * H * W, ldx), S.SENTINEL, dtype=torch.float32, device=G.dev())
    wdg = E.pack_dgrad(d['w']).float().to(G.dev())
    _lib.call('ssp_conv_s2_dgrad', dyd.data_ptr(), wdg.data_ptr(), dx.data_ptr(), B, H, W, ldy, Cin, ldy, ldx, R, 0, G.stream())
    torch.cuda.synchronize()
    _assert_equal(dx.cpu()[:, :Cin], d['dgrad'].reshape(-1, Cin).float(), ('pixel', 'ci'))


@pytest.mark.parametrize('accumulate', [0, 1], ids=['plain', 'acc'])
@pytest.mark.parametrize('c', S.PAD_DGRAD, ids=S.case_id)
def test_data_gradient_with_padded_cin(c, accumulate):
    """Cin_dx of 18 and 6 (the unpadded count, as the plan passes it) into lddx = pad4(Cin_dx) or a slice of a wider buffer:
    the scatter epilogue, the zero fill in front of a tap-split or 1x1 launch and the atomic adds write Cin_dx columns;
    every other column keeps its sentinel."""
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    d = _data(c)
    assert Cin % 4 == 2 and c.off + E.pad4(Cin) <= c.lddx
    dyd = E.nhwc_buffer(d['dy']).to(G.dev())
    wd = E.pack_dgrad(d['w']).float().to(G.dev())
    M = B * H * W
    pre = E.prefill(c.shape, (M, Cin))
    dx = torch.full((M, c.lddx), S.SENTINEL, dtype=torch.float32)
    dx[:, c.off:c.off + Cin] = pre.float() if accumulate else NAN
    dx = dx.to(G.dev())
    _lib.call('ssp_conv_s2_dgrad', dyd.data_ptr(), wd.data_ptr(), G.p(dx, c.off), B, H, W, E.pad4(Cout), Cin, E.pad4(Cout),
              c.lddx, R, accumulate, G.stream())
    torch.cuda.synchronize()
    want = d['dgrad'].reshape(M, Cin).float() + (pre.float() if accumulate else 0)
    _assert_equal(dx.cpu()[:, c.off:c.off + Cin], want, ('pixel', 'ci'))
    assert _sentinel_kept(dx, c.off, c.off + Cin)


# ------------------------------------------------------------------------------------------------ argument checks
def test_out_of_range_arguments_are_refused():
    G, _lib = _imports()
    buf = torch.zeros(4096, dtype=torch.float32, device=G.dev())
    p, st = buf.data_ptr(), G.stream()
    fwd = lambda **k: _lib.call('ssp_conv_s2_fwd', k.get('inp', p), p, p, None, None, 1, 4, 4, k.get('Cin', 8), 8,
                                k.get('ldin', 8), k.get('ldout', 8), k.get('R', 3), 0, st)
    dgr = lambda **k: _lib.call('ssp_conv_s2_dgrad', p, p, k.get('dx', p), 1, 4, 4, k.get('Cout', 8), 8, k.get('lddy', 8),
                                k.get('lddx', 8), k.get('R', 3), 0, st)
    wgr = lambda **k: _lib.call('ssp_conv_s2_wgrad', p, k.get('x', p), p, 1, 4, 4, k.get('Cin', 8), 8, k.get('lddy', 8),
                                k.get('ldx', 8), k.get('R', 3), st)
    for fn, kw, msg in [(fwd, dict(R=5), '1x1 and 3x3'), (fwd, dict(Cin=6), 'multiple of 4'), (fwd, dict(ldin=4), 'ldin'),
                        (fwd, dict(ldout=6), 'ldout'), (fwd, dict(inp=p + 4), 'aligned'),
                        (dgr, dict(R=2), '1x1 and 3x3'), (dgr, dict(Cout=6), 'multiple of 4'), (dgr, dict(lddy=4), 'lddy'),
                        (dgr, dict(lddx=6), 'lddx'), (dgr, dict(dx=p + 8), 'aligned'),
                        (wgr, dict(R=7), '1x1 and 3x3'), (wgr, dict(Cin=10), 'multiple of 4'), (wgr, dict(ldx=4), 'ldx'),
                        (wgr, dict(lddy=6), 'lddy'), (wgr, dict(x=p + 4), 'aligned')]:
        with pytest.raises(_lib.SspError, match=msg):
            fn(**kw)
    with pytest.raises(_lib.SspError, match='too many pixels'):
        _lib.call('ssp_conv_s2_fwd', p, p, p, None, None, 1 << 11, 1 << 10, 1 << 10, 8, 8, 8, 8, 3, 0, st)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ a residual network
# tests/strided_cases.py NET_CFG on a 2 x 3 x 26 x 38 input: conv s1 -> 3x3 s2 BN leaky -> 1x1 -> 3x3 -> shortcut -> 3x3 s2 ->
# a 1x1 s2 projection of layer 1 through route + shortcut -> linear 1x1 head with 20 channels.  The reference is
# oracle.darknet_ref.forward_ref on the same network with each shortcut restated as route + [I | I] convolution
# (strided_cases.ORACLE_CFG: forward_ref has no shortcut block).  Bars: the forward 1e-4 of tests/test_gpu_generic_blocks.py,
# gradients its 3e-4 floor (element and norm error of every parameter gradient; x.grad as tests/test_gpu_input_grad.py),
# with the decisions frozen as tests/test_gpu_input_grad.py freezes them.
TOL_FWD, TOL_GRAD = 1e-4, 3e-4


def _net(tmp_path, seed=3):
    from helpers import load_state_into
    from oracle.darknet_ref import seeded_state
    from singleshotpose_amd.cfg import parse_cfg
    from singleshotpose_amd.darknet import Darknet
    model = Darknet(S.write_cfg(tmp_path))
    state = seeded_state(model.blocks, seed)
    load_state_into(model, model.blocks, state)
    oblocks = parse_cfg(S.write_cfg(tmp_path, S.ORACLE_CFG, 'oracle.cfg'))
    return model.cuda(), state, oblocks


def _x(seed=1):
    return torch.from_numpy(np.random.RandomState(seed).uniform(0, 1, S.NET_INPUT).astype(np.float32))


def _probe(y, seed=5):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(tuple(y.shape)).astype(np.float32))


def _model_state(model):
    """The module tree's current parameters and buffers as a seeded_state-shaped list (CPU, fp32)."""
    out = []
    for ind, b in enumerate(model.blocks[1:]):
        if b['type'] != 'convolutional':
            out.append(None)
            continue
        seq = model.models[ind]
        e = {'weight': seq[0].weight.detach().cpu().contiguous().clone()}
        if int(b['batch_normalize']):
            e.update(bn_weight=seq[1].weight.detach().cpu().clone(), bn_bias=seq[1].bias.detach().cpu().clone(),
                     running_mean=seq[1].running_mean.cpu().clone(), running_var=seq[1].running_var.cpu().clone())
        else:
            e['bias'] = seq[0].bias.detach().cpu().clone()
        out.append(e)
    return out


def _frozen_decisions(model):
    """tests/test_gpu_input_grad.py _decisions on the product's layers, re-indexed to the oracle's; the sign of the leaky
    shortcut's output is frozen the same way (forward_ref's act_override on the restated sum)."""
    from test_gpu_input_grad import _decisions
    B, _, H, W = S.NET_INPUT
    d = _decisions(model, B, H, W)
    assert not d['pool_override']
    plan = model._plans[(B, H, W, 0)]
    out = dict(raw_override={S.ORACLE_INDEX[k]: v for k, v in d['raw_override'].items()},
               act_override={S.ORACLE_INDEX[k]: v for k, v in d['act_override'].items()})
    a = plan.acts[8]
    out['act_override'][S.ORACLE_INDEX[8]] = a.t.view(-1, a.ld)[:, :a.C].reshape(B, a.H, a.W, a.C).permute(0, 3, 1, 2).cpu()
    return out


def test_network_forward_train_and_eval(tmp_path):
    from oracle.darknet_ref import forward_ref
    model, state, oblocks = _net(tmp_path)
    x = _x()
    model.eval()
    with torch.no_grad():
        y = model(x.cuda())
    ref = forward_ref(oblocks, S.oracle_state(state), x.double(), training=False)
    assert tuple(y.shape) == tuple(ref.shape) == (2, 20, 7, 10)
    assert rel_err(y.cpu().numpy(), ref.numpy()) < TOL_FWD
    model.train()
    y = model(x.cuda())
    ost = S.oracle_state(state)
    ref = forward_ref(oblocks, ost, x.double(), training=True)
    assert rel_err(y.detach().cpu().numpy(), ref.numpy()) < TOL_FWD
    for ind in S.NET_STRIDED:          # running statistics of the strided BatchNorm blocks followed the batch
        bn = model.models[ind][1]
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), ost[S.ORACLE_INDEX[ind]]['running_mean'].numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), ost[S.ORACLE_INDEX[ind]]['running_var'].numpy(), rtol=1e-4, atol=1e-5)


def test_network_gradients_and_sgd_step(tmp_path):
    from oracle.darknet_ref import forward_ref
    from singleshotpose_amd.optim import SGD
    model, state, oblocks = _net(tmp_path)
    model.train()
    kw = dict(lr=1e-2, momentum=0.9, dampening=0, weight_decay=5e-4)
    opt = SGD(model.parameters(), **kw)
    opt.zero_grad()
    x = _x()
    xg = x.cuda().requires_grad_(True)
    y = model(xg)
    frozen = _frozen_decisions(model)
    probe = _probe(y)
    (y * probe.cuda()).sum().backward()
    torch.cuda.synchronize()
    ost = S.oracle_state(state, requires_grad=True)
    xr = x.double().requires_grad_(True)
    yr = forward_ref(oblocks, ost, xr, training=True, **frozen)
    assert rel_err(y.detach().cpu().numpy(), yr.detach().numpy()) < TOL_FWD
    yr.backward(probe.double())
    err_x = rel_err(xg.grad.cpu().numpy(), xr.grad.numpy())
    print('x.grad: %.3g' % err_x)
    worst = []
    for ind, b in enumerate(model.blocks[1:]):
        if b['type'] != 'convolutional':
            continue
        seq, e = model.models[ind], ost[S.ORACLE_INDEX[ind]]
        pairs = [('weight', seq[0].weight)]
        pairs += [('bn_weight', seq[1].weight), ('bn_bias', seq[1].bias)] if 'bn_weight' in e else [('bias', seq[0].bias)]
        for name, prm in pairs:
            got, want = prm.grad.detach().cpu().double().numpy(), e[name].grad.numpy()
            de = rel_err(got, want)
            dn = abs(float(np.sqrt((got ** 2).sum())) / float(np.sqrt((want ** 2).sum())) - 1)
            print('layer %d %s: element %.3g norm %.3g' % (ind, name, de, dn))
            worst.append((max(de, dn), ind, name))
    assert err_x < TOL_GRAD
    assert max(worst)[0] <= TOL_GRAD, max(worst)
    # one fused SGD step (ssp_sgd_step over the flat gradient layout), then a second forward on the moved weights
    shadow = [torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters()]
    sopt = torch.optim.SGD(shadow, **kw)
    for p, q in zip(model.parameters(), shadow):
        q.grad = p.grad.detach().cpu().clone()
    opt.step()
    sopt.step()
    assert opt.fused_steps == 1
    for (n, p), q in zip(model.named_parameters(), shadow):
        assert rel_err(p.detach().cpu().numpy(), q.detach().numpy()) < 1e-6, n
    model.eval()
    with torch.no_grad():
        y2 = model(x.cuda())
    ref2 = forward_ref(oblocks, S.oracle_state(_model_state(model)), x.double(), training=False)
    assert rel_err(y2.cpu().numpy(), ref2.numpy()) < TOL_FWD
    assert not torch.equal(y2.cpu(), y.detach().cpu())


def _record(monkeypatch):
    from singleshotpose_amd import _lib
    log = []
    orig = _lib.call

    def rec(name, *args):
        log.append(name)
        return orig(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)
    return log


def test_frozen_trunk_launches_no_strided_gradient_it_does_not_need(tmp_path, monkeypatch):
    """Layers 0-5 frozen (parameters and BatchNorm modes), the projection (layer 7) and the head trainable: the backward
    runs layer 7's filter gradient and no strided data gradient at all; with x.requires_grad every strided block's data
    gradient runs and still only layer 7's filter gradient; the gradients that remain are those of the full backward."""
    model, state, _ = _net(tmp_path)
    model.train()
    x = _x().cuda()

    def step(want_x=False):
        model.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(want_x)
        y = model(xi)
        (y * _probe(y).cuda()).sum().backward()
        torch.cuda.synchronize()
        return xi.grad

    step()
    full = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    for ind in range(6):
        m = model.models[ind]
        if isinstance(m, torch.nn.Sequential):
            for p in m.parameters():
                p.requires_grad_(False)
            if len(m) > 1 and isinstance(m[1], torch.nn.BatchNorm2d):
                m[1].eval()
    step()                                   # new schedule: bookkeeping of its first step
    log = _record(monkeypatch)
    step()
    assert log.count('ssp_conv_s2_wgrad') == 1 and log.count('ssp_conv_s2_dgrad') == 0, log
    assert log.count('ssp_conv_s2_fwd') + log.count('ssp_conv_s2_fwd_affine') == 3
    for n, p in model.named_parameters():
        assert (p.grad is not None) == p.requires_grad, n
    del log[:]
    gx = step(True)
    assert log.count('ssp_conv_s2_wgrad') == 1 and log.count('ssp_conv_s2_dgrad') == 3, log
    assert gx is not None and torch.isfinite(gx).all() and float(gx.abs().max()) > 0
    # layers 0-5 in eval() change the forward (running statistics instead of the batch's), so only the head-side structure is
    # compared with the full step: the same parameters get gradients of the same shape
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad.shape == full[n].shape and torch.isfinite(p.grad).all(), n


def test_graph_replay_equals_eager(tmp_path):
    model, _, _ = _net(tmp_path)
    model.eval()
    xs = [_x(s).cuda() for s in (1, 2)]
    with torch.no_grad():
        model.graph_inference = False
        eager = [model(x).clone() for x in xs]
        model.graph_inference = True
        got = [model(x).clone() for x in xs]
        plan = list(model._plans.values())[0]
        assert plan._graph is not None and not plan._graph_failed
        for a, b in zip(eager, got):
            assert torch.equal(a, b)
    model.graph_inference = False


def test_fused_pool_behind_a_strided_block_on_the_gpu(tmp_path):
    """conv -> 3x3 s2 BN leaky -> 2x2/2 max-pool (fused into the strided block) -> head, against forward_ref; gradients of
    every parameter at the bars above (decisions frozen, the pool's winners included)."""
    from helpers import load_state_into
    from oracle.darknet_ref import forward_ref, seeded_state
    from singleshotpose_amd.darknet import Darknet
    from test_gpu_input_grad import _decisions
    net = '[net]\nheight=24\nwidth=28\nchannels=3\n\n'
    conv = '[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=3\nstride=%d\npad=1\nactivation=leaky\n\n'
    head = '[convolutional]\nfilters=8\nsize=1\nstride=1\npad=1\nactivation=linear\n\n'
    model = Darknet(S.write_cfg(tmp_path, net + conv % (8, 1) + conv % (16, 2) + '[maxpool]\nsize=2\nstride=2\n\n' + head, 'p.cfg'))
    state = seeded_state(model.blocks, 4)
    load_state_into(model, model.blocks, state)
    model = model.cuda().train()
    x = torch.from_numpy(np.random.RandomState(2).uniform(0, 1, (2, 3, 24, 28)).astype(np.float32))
    y = model(x.cuda())
    plan = model._plans[(2, 24, 28, 0)]
    assert plan.convs[1].stride == 2 and plan.convs[1].pool and plan.fused_pool == {2}
    frozen = _decisions(model, 2, 24, 28)
    probe = _probe(y)
    (y * probe.cuda()).sum().backward()
    st = [None if e is None else {k: v.double().requires_grad_(not k.startswith('running')) for k, v in e.items()} for e in state]
    yr = forward_ref(model.blocks, st, x.double(), training=True, **frozen)
    assert tuple(y.shape) == (2, 8, 6, 7) and rel_err(y.detach().cpu().numpy(), yr.detach().numpy()) < TOL_FWD
    yr.backward(probe.double())
    for ind in (0, 1, 3):
        seq, e = model.models[ind], st[ind]
        pairs = [('weight', seq[0].weight)] + ([('bn_weight', seq[1].weight), ('bn_bias', seq[1].bias)] if 'bn_weight' in e
                                               else [('bias', seq[0].bias)])
        for name, prm in pairs:
            assert rel_err(prm.grad.cpu().numpy(), e[name].grad.numpy()) < TOL_GRAD, (ind, name)

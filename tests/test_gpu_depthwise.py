"""Depthwise 3x3 convolutions on the MI355X: the entry points of csrc/conv_depthwise.hip through the C ABI against the host
statements of tests/depthwise_cases.py on exact-integer operands (torch.equal: every partial sum stays below 2^24), their
BatchNorm statistics through ssp_bn_fwd_finalize, their argument checks, and every net of that module through Darknet +
engine.Plan against its float64 CPU reference - eval and training forward, running statistics, dL/dx and every parameter
gradient at the bars of tests/test_gpu_topology.py: max(floor, 3 x the float32 CPU reference's own distance to float64),
floors 1e-4 (outputs, dL/dx) and 3e-4 (parameter gradients); the exact-integer net bit for bit.  Then the plan's other routes
through the block: the input-only backward, graph replay, a second step on changed weights, batch 1, a frozen depthwise
filter, run-to-run reproducibility, and the shipped cfg.  Every figure is printed before it is asserted."""
import functools
import os

import numpy as np
import pytest
import torch

import depthwise_cases as D
from exact_conv import first_diffs
from helpers import make_targets, rel_err

pytestmark = pytest.mark.gpu
FLOOR_Y, FLOOR_G = 1e-4, 3e-4
EPS32 = float(np.finfo(np.float32).eps)
ids = lambda cases: [c.id for c in cases]
NAN = float('nan')


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()          # (a copy: the shared case data is read-only)


def _st():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _refs(k):
    """float64 references of a kernel case, computed once and shared (never modified) by the tests below."""
    x, dy, w, pre_out, pre_in, pre_w = D.kernel_data(k)
    return dict(fwd=D.dw_fwd_ref(x, w, k.stride), dgrad=D.dw_dgrad_ref(dy, w, k.H, k.W, k.stride), wgrad=D.dw_wgrad_ref(dy, x, k.stride))


def _same(got, want, what):
    """got == want as torch.equal compares (a zero of either sign is zero; a NaN equals nothing) - values and every sentinel
    column."""
    if not np.array_equal(got, want):
        bad = np.argwhere(~(got == want))
        raise AssertionError('%s: %d elements differ, first %s: got %r, want %r' % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------------- kernels, C ABI
@pytest.mark.parametrize('k', D.KERNEL_CASES, ids=D.kcase_id)
def test_forward_exact_with_bias_and_statistics(k):
    from singleshotpose_amd import _lib
    (ldi, offi), (ldo, offo) = D.sides(k)
    x, dy, w, pre_out, pre_in, pre_w = D.kernel_data(k)
    Ho, Wo = D.out_hw(k.H, k.W, k.stride)
    M = k.B * Ho * Wo
    xd, wd = _dev(D.embed(x, ldi, offi)), _dev(w)
    out = _dev(D.embed(pre_out, ldo, offo, fill=NAN))
    assert _lib.query('ssp_dwconv_stats_tile_m', k.B, k.H, k.W, k.C, k.stride) == 0
    ntile = _lib.query('ssp_dwconv_stats_tiles', k.B, k.H, k.W, k.C, k.stride)
    nfl = _lib.query('ssp_dwconv_stats_floats', k.B, k.H, k.W, k.C, k.stride)
    assert ntile >= 1 and nfl == ntile * (2 * k.C + 1)
    stats = torch.full((nfl + 8,), NAN, dtype=torch.float32, device='cuda')
    _lib.call('ssp_dwconv_fwd', xd.data_ptr() + 4 * offi, wd.data_ptr(), out.data_ptr() + 4 * offo, None, stats.data_ptr(),
              k.B, k.H, k.W, k.C, ldi, ldo, k.stride, _st())
    torch.cuda.synchronize()
    want = _refs(k)['fwd']
    _same(out.cpu().numpy(), D.embed(want.astype(np.float32), ldo, offo), 'forward')
    _same(xd.cpu().numpy(), D.embed(x, ldi, offi), 'forward input')
    s = stats.cpu().numpy()
    assert np.isfinite(s[:nfl]).all() and np.isnan(s[nfl:]).all()          # every float of the buffer written, nothing past it
    counts = s[ntile * 2 * k.C:nfl]
    assert counts.sum() == M and counts.min() >= 1
    # with a bias, no statistics
    bias = (np.arange(k.C) % 7 - 3).astype(np.float32)
    out2, bd = _dev(D.embed(pre_out, ldo, offo, fill=NAN)), _dev(bias)
    _lib.call('ssp_dwconv_fwd', xd.data_ptr() + 4 * offi, wd.data_ptr(), out2.data_ptr() + 4 * offo, bd.data_ptr(), None,
              k.B, k.H, k.W, k.C, ldi, ldo, k.stride, _st())
    torch.cuda.synchronize()
    _same(out2.cpu().numpy(), D.embed((want + bias).astype(np.float32), ldo, offo), 'forward + bias')
    # BatchNorm statistics through the finalize (counted format, tile_m = 0), against the exact mean and (biased) variance.
    # eps = 1 keeps var = 1 / invstd^2 - 1 well conditioned down to var = 0 (the single-pixel case).
    vec = torch.zeros(4, k.C, dtype=torch.float32, device='cuda')
    gamma, beta = torch.ones(k.C, device='cuda'), torch.zeros(k.C, device='cuda')
    rm, rv = torch.zeros(k.C, device='cuda'), torch.ones(k.C, device='cuda')
    _lib.call('ssp_bn_fwd_finalize', stats.data_ptr(), ntile, 0, M, k.C, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
              rv.data_ptr(), 0.1, 1.0, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), _st())
    torch.cuda.synchronize()
    r64 = want.reshape(M, k.C)
    mean, var = r64.mean(0), r64.var(0)
    A = float(np.abs(r64).max())
    got_mean = vec[0].cpu().double().numpy()
    got_var = 1.0 / vec[1].cpu().double().numpy() ** 2 - 1.0
    # fp32 rounding of the two quantities, derived as tests/test_gpu_strided.py derives its bars, from the depth of THIS
    # kernel's combine (D.stats_depth, from the header comment): a strip's mean and M2 are <= 4 terms; a pair is then the end
    # of a chain of at most `depth` Chan combines (strips of a part, then the parts), each of which rounds ~8 times
    # (d, f, d f, mean +; d d, n f, their product, M2 +) relative to a quantity bounded by 2 A (mean) or by 4 A^2 times the
    # pixels combined so far - A^2 after the division by the count (variance); the tiles are combined in float64; reading
    # the variance back out of invstd adds ~4 roundings relative to var + 1
    depth = D.stats_depth(k.C)
    err_mean, err_var = float(np.abs(got_mean - mean).max()), float(np.abs(got_var - var).max())
    tol_mean = 8 * depth * EPS32 * 2 * max(A, 1.0)
    tol_var = 8 * depth * EPS32 * 4 * max(A * A, 1.0) + 4 * EPS32 * float(var.max() + 1.0)
    print('DWK %s statistics: depth %d, mean err %.3g (bar %.3g), var err %.3g (bar %.3g)' % (
        D.kcase_id(k), depth, err_mean, tol_mean, err_var, tol_var))
    assert err_mean <= tol_mean and err_var <= tol_var


@pytest.mark.parametrize('k', D.KERNEL_CASES, ids=D.kcase_id)
def test_forward_affine_epilogue(k):
    """The eval-mode epilogue leaky(scale * conv + shift, slope): dyadic scale / shift / slope keep every value exact."""
    from singleshotpose_amd import _lib
    (ldi, offi), (ldo, offo) = D.sides(k)
    x, dy, w, pre_out, pre_in, pre_w = D.kernel_data(k)
    xd, wd = _dev(D.embed(x, ldi, offi)), _dev(w)
    scale = np.array([(-2.0, 0.5, 1.0, 0.0)[i % 4] for i in range(k.C)], np.float32)
    shift = np.array([float(i % 5 - 2) for i in range(k.C)], np.float32)
    conv = _refs(k)['fwd']
    for sc, sh, slope in ((scale, shift, 0.5), (None, shift, 1.0), (scale, None, 0.0), (None, None, 0.5)):
        out = _dev(D.embed(pre_out, ldo, offo, fill=NAN))
        scd, shd = (None if sc is None else _dev(sc)), (None if sh is None else _dev(sh))      # (held until the launch is done)
        _lib.call('ssp_dwconv_fwd_affine', xd.data_ptr() + 4 * offi, wd.data_ptr(), out.data_ptr() + 4 * offo,
                  None if scd is None else scd.data_ptr(), None if shd is None else shd.data_ptr(), slope,
                  k.B, k.H, k.W, k.C, ldi, ldo, k.stride, _st())
        torch.cuda.synchronize()
        v = conv * (1.0 if sc is None else sc) + (0.0 if sh is None else sh)
        want = np.where(v > 0, v, v * slope) + 0.0          # (+ 0.0: the kernel's y * slope of y = -0.0 ... compare values)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, offo:offo + k.C].reshape(want.shape), want.astype(np.float32)), (slope, sc is None, sh is None)
        rest = np.delete(got, np.s_[offo:offo + k.C], 1)
        assert (rest == D.SENTINEL).all()


@pytest.mark.parametrize('accumulate', [0, 1], ids=['plain', 'acc'])
@pytest.mark.parametrize('k', D.KERNEL_CASES, ids=D.kcase_id)
def test_data_gradient_exact(k, accumulate):
    from singleshotpose_amd import _lib
    (ldi, offi), (ldo, offo) = D.sides(k)
    x, dy, w, pre_out, pre_in, pre_w = D.kernel_data(k)
    dyd, wd = _dev(D.embed(dy, ldo, offo)), _dev(w)
    dx = _dev(D.embed(pre_in, ldi, offi, fill=None if accumulate else NAN))
    _lib.call('ssp_dwconv_dgrad', dyd.data_ptr() + 4 * offo, wd.data_ptr(), dx.data_ptr() + 4 * offi, k.B, k.H, k.W, k.C, ldo, ldi,
              k.stride, accumulate, _st())
    torch.cuda.synchronize()
    want = _refs(k)['dgrad'] + (pre_in if accumulate else 0)
    _same(dx.cpu().numpy(), D.embed(want.astype(np.float32), ldi, offi), 'data gradient')
    _same(dyd.cpu().numpy(), D.embed(dy, ldo, offo), 'dy')


@pytest.mark.parametrize('accumulate', [0, 1], ids=['plain', 'acc'])
@pytest.mark.parametrize('k', D.KERNEL_CASES, ids=D.kcase_id)
def test_filter_gradient_exact(k, accumulate):
    from singleshotpose_amd import _lib
    (ldi, offi), (ldo, offo) = D.sides(k)
    x, dy, w, pre_out, pre_in, pre_w = D.kernel_data(k)
    xd, dyd = _dev(D.embed(x, ldi, offi)), _dev(D.embed(dy, ldo, offo))
    need = _lib.query('ssp_dwconv_wgrad_workspace_floats', k.B, k.H, k.W, k.C, k.stride)
    assert need > 0 and need % (9 * k.C) == 0 and need // (9 * k.C) <= 512
    ws = torch.full((need + 8,), NAN, dtype=torch.float32, device='cuda')
    dw = _dev(pre_w.copy()) if accumulate else torch.full((k.C, 9), NAN, dtype=torch.float32, device='cuda')
    _lib.call('ssp_dwconv_wgrad', dyd.data_ptr() + 4 * offo, xd.data_ptr() + 4 * offi, dw.data_ptr(), k.B, k.H, k.W, k.C, ldo, ldi,
              k.stride, accumulate, ws.data_ptr(), need, _st())
    torch.cuda.synchronize()
    want = _refs(k)['wgrad'] + (pre_w if accumulate else 0)
    _same(dw.cpu().numpy(), want.astype(np.float32), 'filter gradient')
    wsn = ws.cpu().numpy()
    assert np.isfinite(wsn[:need]).all() and np.isnan(wsn[need:]).all()          # the partial sums stay inside the workspace
    # the ranges' partial sums ARE the gradient (integers: exact in any order)
    assert np.array_equal(wsn[:need].reshape(-1, k.C, 9).astype(np.float64).sum(0), _refs(k)['wgrad'])


BAD = [   # (what, C, ldin, ldout, B, H, W, stride, input pointer offset in bytes, output pointer offset in bytes)
    ('C not a multiple of 4', 6, 8, 8, 1, 4, 4, 1, 0, 0),
    ('C zero', 0, 8, 8, 1, 4, 4, 1, 0, 0),
    ('input stride not a multiple of 4', 4, 6, 8, 1, 4, 4, 1, 0, 0),
    ('output stride below C', 8, 8, 4, 1, 4, 4, 1, 0, 0),
    ('stride 0', 4, 4, 4, 1, 4, 4, 0, 0, 0),
    ('stride 3', 4, 4, 4, 1, 4, 4, 3, 0, 0),
    ('empty batch', 4, 4, 4, 0, 4, 4, 1, 0, 0),
    ('2^31 pixels', 4, 4, 4, 1 << 15, 1 << 8, 1 << 8, 1, 0, 0),
    ('unaligned input', 4, 8, 8, 1, 4, 4, 1, 4, 0),
    ('unaligned output', 4, 8, 8, 1, 4, 4, 2, 0, 8),
    ('null input', 4, 4, 4, 1, 4, 4, 1, None, 0),
]


@pytest.mark.parametrize('bad', BAD, ids=[b[0].replace(' ', '_') for b in BAD])
def test_out_of_range_arguments_are_refused(bad):
    from singleshotpose_amd import _lib
    what, C, ldi, ldo, B, H, W, s, io, oo = bad
    a, b, w, ws = (torch.full((4096,), D.SENTINEL, dtype=torch.float32, device='cuda') for _ in range(4))
    ap = None if io is None else a.data_ptr() + io
    bp = b.data_ptr() + oo
    calls = [('ssp_dwconv_fwd', (ap, w.data_ptr(), bp, None, None, B, H, W, C, ldi, ldo, s, _st())),
             ('ssp_dwconv_fwd_affine', (ap, w.data_ptr(), bp, None, None, 0.1, B, H, W, C, ldi, ldo, s, _st())),
             ('ssp_dwconv_dgrad', (bp, w.data_ptr(), ap, B, H, W, C, ldo, ldi, s, 0, _st())),
             ('ssp_dwconv_wgrad', (bp, ap, w.data_ptr(), B, H, W, C, ldo, ldi, s, 0, ws.data_ptr(), 4096, _st()))]
    for name, args in calls:
        with pytest.raises(_lib.SspError, match=r'dwconv_\w+: '):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert all(bool((t == D.SENTINEL).all()) for t in (a, b, w, ws))


def test_short_workspace_and_unaligned_vectors_are_refused():
    from singleshotpose_amd import _lib
    a, b, w, ws = (torch.full((4096,), D.SENTINEL, dtype=torch.float32, device='cuda') for _ in range(4))
    need = _lib.query('ssp_dwconv_wgrad_workspace_floats', 2, 4, 4, 8, 1)
    with pytest.raises(_lib.SspError, match='dwconv_wgrad: workspace'):
        _lib.call('ssp_dwconv_wgrad', b.data_ptr(), a.data_ptr(), w.data_ptr(), 2, 4, 4, 8, 8, 8, 1, 0, ws.data_ptr(), need - 1, _st())
    with pytest.raises(_lib.SspError, match='dwconv_wgrad: null or unaligned'):
        _lib.call('ssp_dwconv_wgrad', b.data_ptr(), a.data_ptr(), w.data_ptr(), 2, 4, 4, 8, 8, 8, 1, 0, None, need, _st())
    with pytest.raises(_lib.SspError, match='dwconv_fwd: null or unaligned'):
        _lib.call('ssp_dwconv_fwd', a.data_ptr(), w.data_ptr(), b.data_ptr(), ws.data_ptr() + 4, None, 2, 4, 4, 8, 8, 8, 1, _st())
    with pytest.raises(_lib.SspError, match='dwconv_fwd_affine: null or unaligned'):
        _lib.call('ssp_dwconv_fwd_affine', a.data_ptr(), w.data_ptr(), b.data_ptr(), None, ws.data_ptr() + 8, 0.1, 2, 4, 4, 8, 8, 8, 1,
                  _st())
    torch.cuda.synchronize()
    assert all(bool((t == D.SENTINEL).all()) for t in (a, b, w, ws))


# ---------------------------------------------------------------------------------------------------- nets
def _poison():
    """NaNs in the caching allocator's free blocks: what a plan allocates with torch.empty and never writes reads as NaN."""
    t = torch.full((16 << 20,), NAN, dtype=torch.float32, device='cuda')
    del t


def _model(case, monkeypatch):
    monkeypatch.setenv('SSP_AUTOTUNE', '0')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    return D.make_model(case).cuda()


def _plan_of(model, case):
    return model._plans[(case.B, case.H, case.W, 0)]


def _check(case, what, got, want64, want32, floor):
    err, own = rel_err(got, want64.numpy()), rel_err(want32.numpy(), want64.numpy())
    bar = max(floor, 3.0 * own)
    print('DW %s %s err %.3e ref32 %.3e bar %.3e' % (case.id, what, err, own, bar))
    assert tuple(got.shape) == tuple(want64.shape), (case.id, what, got.shape, want64.shape)
    assert err <= bar, (case.id, what, err, bar)      # (a NaN fails: not <=)


def _eval(model, case, ref):
    r64, r32 = ref
    model.eval()
    _poison()
    with torch.no_grad():
        y = model(D.make_input(case, D.seed_of(case)).cuda())
    _check(case, 'y_eval', y.cpu().numpy(), r64.y_eval, r32.y_eval, FLOOR_Y)
    return y.cpu()


def _train_step(model, case, ref, x=None, probe=None, stats=True, params=True):
    """One training forward + backward of (y * probe).sum() against the reference; returns (y, dL/dx)."""
    r64, r32 = ref
    seed = D.seed_of(case)
    model.train()
    model.zero_grad(set_to_none=True)
    xg = (D.make_input(case, seed) if x is None else x).cuda().requires_grad_(True)
    _poison()
    y = model(xg)
    _check(case, 'y_train', y.detach().cpu().numpy(), r64.y_train, r32.y_train, FLOOR_Y)
    if stats:
        for n, b in model.named_buffers():
            if 'running' in n and n.startswith('models.'):
                print('DW %s stat:%s maxabs %.3e' % (case.id, n, float((b.cpu().double() - r64.stats[n]).abs().max())))
                np.testing.assert_allclose(b.cpu().numpy(), r64.stats[n].numpy(), rtol=1e-4, atol=1e-5, err_msg=n)
    _poison()
    (y * (D.make_probe(case, seed, y.shape) if probe is None else probe).cuda()).sum().backward()
    torch.cuda.synchronize()
    _check(case, 'dx', xg.grad.cpu().numpy(), r64.dx, r32.dx, FLOOR_Y)
    for n, p in model.models.named_parameters():
        n = 'models.' + n
        if not params:
            assert p.grad is None, n
        else:
            assert p.grad is not None, (case.id, n)
            _check(case, 'grad:' + n, p.grad.cpu().numpy(), r64.grads[n], r32.grads[n], FLOOR_G)
    return y.detach().cpu(), xg.grad.detach().cpu()


@pytest.mark.parametrize('case', D.FLOAT, ids=ids(D.FLOAT))
def test_float_net(case, monkeypatch):
    model = _model(case, monkeypatch)
    ref = D.reference(case, D.seed_of(case))
    _eval(model, case, ref)
    _train_step(model, case, ref)
    plan = _plan_of(model, case)
    want = D.PLANS[case.id]
    assert plan.depthwise == want['depthwise'] and plan.fused_pool == want['fused_pool']
    assert {i: cs.bn_fuse_src.ind for i, cs in plan.convs.items() if cs.bn_fuse_src is not None} == want['bn_pairs']


def test_exact_net_equals_float64(monkeypatch):
    """Integer data below the 2^24 budget: fp32 is exact in any summation order, so the product's numbers ARE float64's."""
    case = D.DW_EXACT
    model = _model(case, monkeypatch)
    r64, _ = D.reference(case, 0)
    x = D.make_input(case, 0).cuda()
    model.eval()
    _poison()
    with torch.no_grad():
        y_eval = model(x).cpu()
    model.train()
    xg = x.clone().requires_grad_(True)
    _poison()
    y = model(xg)
    _poison()
    (y * D.make_probe(case, 0, y.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert _plan_of(model, case).depthwise == [2, 4]
    for what, got, want in [('y_eval', y_eval, r64.y_eval), ('y_train', y.detach().cpu(), r64.y_train),
                            ('dx', xg.grad.cpu(), r64.dx)]:
        assert torch.equal(got, want.float()), (what, first_diffs(got, want.float(), ('b', 'c', 'y', 'x')))
    for n, p in model.models.named_parameters():
        got, want = p.grad.cpu().contiguous(), r64.grads['models.' + n].float()
        assert torch.equal(got, want), (n, first_diffs(got, want, ('co', 'ci', 'ky', 'kx')[:got.dim()]))


def _record(monkeypatch):
    from singleshotpose_amd import _lib
    log = []
    orig = _lib.call

    def rec(name, *args):
        log.append(name)
        return orig(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)
    return log


def test_launches_of_the_separable_net(monkeypatch):
    """Training: one ssp_dwconv_fwd / _dgrad / _wgrad per depthwise block and no repack or dense kernel for it; eval: the
    one-launch affine form."""
    case = D.DW_SEP
    model = _model(case, monkeypatch)
    log = _record(monkeypatch)
    _eval(model, case, D.reference(case, 0))          # (first: the training step below moves the running statistics)
    assert log.count('ssp_dwconv_fwd_affine') == 2 and log.count('ssp_dwconv_fwd') == 0
    del log[:]
    _train_step(model, case, D.reference(case, 0))
    assert log.count('ssp_dwconv_fwd') == 2 and log.count('ssp_dwconv_dgrad') == 2 and log.count('ssp_dwconv_wgrad') == 2
    assert log.count('ssp_dwconv_fwd_affine') == 0 and log.count('ssp_conv_s2_fwd') == 0 and log.count('ssp_conv_s2_dgrad') == 0
    assert not any('wino' in n for n in log)


def test_input_only_backward_gives_the_same_dx(monkeypatch):
    case = D.DW_SEP
    model = _model(case, monkeypatch)
    ref = D.reference(case, 0)
    _, full = _train_step(model, case, ref, stats=False)
    for p in model.parameters():
        p.requires_grad_(False)
    log = _record(monkeypatch)
    _, only = _train_step(model, case, ref, stats=False, params=False)
    assert log.count('ssp_dwconv_dgrad') == 2 and log.count('ssp_dwconv_wgrad') == 0
    err = rel_err(only.numpy(), full.numpy())
    print('DW %s dx_only_vs_full err %.3e' % (case.id, err))
    assert err <= FLOOR_Y


@pytest.mark.parametrize('case', [D.DW_SEP, D.DW_LAST], ids=ids([D.DW_SEP, D.DW_LAST]))
def test_graph_replay_equals_eager_eval(case, monkeypatch):
    model = _model(case, monkeypatch).eval()
    x = D.make_input(case, D.seed_of(case)).cuda()
    with torch.no_grad():
        model.graph_inference = False
        eager = model(x).cpu()
        model.graph_inference = True
        first = model(x).cpu()          # captures
        again = model(x).cpu()          # replays
    plan = _plan_of(model, case)
    assert plan._graph is not None and not plan._graph_failed
    assert torch.equal(first, eager) and torch.equal(again, eager)
    model.graph_inference = False


def test_second_step_on_changed_weights(monkeypatch):
    """The parameter is the operand: after an in-place update (no repack exists that could be stale) the next step is the
    reference's on the new weights, in training and in eval mode."""
    case, then = D.DW_SEP, D.DW_SEP_STEP2
    model = _model(case, monkeypatch)
    _train_step(model, case, D.reference(case, 0))
    fresh = D.make_model(then)          # (its data seed keeps the decision margins under these weights: test_depthwise_cpu.py)
    with torch.no_grad():
        for (_, p), (_, q) in zip(model.named_parameters(), fresh.named_parameters()):
            p.copy_(q)
        for (_, t), (_, s) in zip(model.named_buffers(), fresh.named_buffers()):
            t.copy_(s)
    ref = D.reference(then, D.seed_of(then))
    _eval(model, then, ref)
    _train_step(model, then, ref)
    assert len(model._plans) == 1          # the same plan ran every pass


def test_frozen_depthwise_filter_schedules_no_filter_gradient(monkeypatch):
    case = D.DW_SEP
    model = _model(case, monkeypatch)
    model.deterministic = True          # (the two runs are compared bit for bit)
    model.train()
    x = D.make_input(case, 0).cuda()

    def step():
        model.zero_grad(set_to_none=True)
        y = model(x)
        (y * D.make_probe(case, 0, y.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().cpu().clone() for n, p in model.models.named_parameters() if p.grad is not None}

    log = _record(monkeypatch)
    full = step()
    assert log.count('ssp_dwconv_wgrad') == 2 and len(full) == len(list(model.models.parameters()))
    model.models[2][0].weight.requires_grad_(False)
    # (the running statistics moved, the batch statistics the training forward normalises with did not)
    del log[:]
    rest = step()
    assert log.count('ssp_dwconv_wgrad') == 1 and log.count('ssp_dwconv_dgrad') == 2 and log.count('ssp_dwconv_fwd') == 2, log
    assert sorted(rest) == sorted(n for n in full if n != '2.conv2.weight')
    for n in rest:
        assert torch.equal(rest[n], full[n]), (n, first_diffs(rest[n], full[n], ('co', 'ci', 'ky', 'kx')[:rest[n].dim()]))


@pytest.mark.parametrize('det', [True, False], ids=['deterministic', 'default'])
def test_two_runs_give_identical_bits(det, monkeypatch):
    """deterministic mode: every gradient of the separable net, twice in one process.  Default mode: the depthwise launches
    are ordered by construction - the depthwise filters' gradients and dL/dx of a net whose other layers are 1x1 (no 3x3 dense
    filter gradient with its atomic sums upstream of either)."""
    case = D.DW_SEP if det else D.DW_ONLY
    runs = []
    for _ in range(2):
        model = _model(case, monkeypatch)
        model.deterministic = det
        model.train()
        xg = D.make_input(case, 0).cuda().requires_grad_(True)
        _poison()
        y = model(xg)
        (y * D.make_probe(case, 0, y.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
        plan = _plan_of(model, case)
        assert plan.deterministic['mode'] == det and plan.depthwise == D.PLANS[case.id]['depthwise']
        runs.append((y.detach().cpu(), xg.grad.cpu(), {n: p.grad.detach().cpu().clone() for n, p in model.models.named_parameters()}))
    a, b = runs
    for n in a[2]:
        print('DW %s %s: %d elements differ between two runs' % ('deterministic' if det else 'default', n, int((a[2][n] != b[2][n]).sum())))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    names = list(a[2]) if det else ['%d.conv%d.weight' % (i, j) for i, j in ((1, 2), (3, 4))]
    for n in names:
        assert tuple(a[2][n].shape)[1:] == (1, 3, 3) or det
        assert torch.equal(a[2][n], b[2][n]), n


def test_shipped_cfg_trains(monkeypatch):
    """cfg/yolo-pose-dw.cfg at batch 2, 416 x 416: one training step with its RegionLoss; shapes and finiteness only."""
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.region_loss import RegionLoss
    from singleshotpose_amd.utils import get_region_boxes
    monkeypatch.setenv('SSP_AUTOTUNE', '0')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    model = Darknet(os.path.join(root, 'cfg', 'yolo-pose-dw.cfg')).cuda().train()
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, (2, 3, 416, 416)).astype(np.float32)).cuda()
    out = model(x)
    assert tuple(out.shape) == (2, 20, 13, 13)
    loss = RegionLoss()(out, torch.from_numpy(make_targets(rs, 2, [1, 1])), 20)
    loss.backward()
    torch.cuda.synchronize()
    plan = model._plans[(2, 416, 416, 0)]
    assert plan.depthwise == [2, 5, 8, 11, 14, 17, 20, 23, 26, 29, 32, 34, 36, 42]
    print('DW yolo-pose-dw loss %.6f' % float(loss.detach()))
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(out).all())
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    box = get_region_boxes(out.detach(), 1, 9)
    assert len(box) == 21 and all(np.isfinite(float(v)) for v in box)

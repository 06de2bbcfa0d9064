"""Darknet + engine.Plan on the MI355X against the float64 CPU reference of tests/topology_cases.py, over the table of
hand-written and seeded random topologies: eval and training forward, running statistics, dL/dx and every parameter
gradient of every supported case; bit-for-bit on the exact family; and the same numbers by the plan's other routes
(input-only backward, graph replay, a second step, both BatchNorm-backward forms, a second batch size and resolution, tuned
plans).  Bars per tensor: max(floor, 3 x the float32 CPU reference's own distance to float64), floors 1e-4 for y and dL/dx
(SURVEY.md 8(d)), 3e-4 for parameter gradients and rtol 1e-4 / atol 1e-5 for running statistics
(tests/test_gpu_generic_blocks.py::test_network_matches_reference).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import topology_cases as T
from exact_conv import first_diffs
from helpers import rel_err

pytestmark = pytest.mark.gpu
FLOOR_Y, FLOOR_G = 1e-4, 3e-4
ids = lambda cases: [c.id for c in cases]


def _poison():
    """Leave NaNs in the caching allocator's free blocks: what a plan allocates with torch.empty and never writes (padding
    channels, gradient buffers) then reads as NaN instead of as whatever an earlier test left there."""
    t = torch.full((16 << 20,), float('nan'), dtype=torch.float32, device='cuda')
    del t


def _model(case, monkeypatch, autotune='0'):
    monkeypatch.setenv('SSP_AUTOTUNE', autotune)
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    return T.make_model(case).cuda()


def _check(case, what, got, want64, want32, floor):
    err, own = rel_err(got, want64.numpy()), rel_err(want32.numpy(), want64.numpy())
    bar = max(floor, 3.0 * own)
    print('TOPO %s %s err %.3e ref32 %.3e bar %.3e' % (case.id, what, err, own, bar))
    assert tuple(got.shape) == tuple(want64.shape), (case.id, what, got.shape, want64.shape)
    assert err <= bar, (case.id, what, err, bar)      # (a NaN fails: not <=)


def _padding_is_zero(model, case):
    """The padding channels [C, ld) of every activation the plan allocated with torch.zeros (C % 4 != 0: block outputs,
    pooled / softmax / shortcut maps; not the raw conv outputs kept for the backward, which nothing reads as an input) are
    still exactly zero: their consumers read them as Cin padding.  A launch
    that wrote ld instead of C columns shows here - in y or dL/dx it may not (a strided block behind an 18-filter block
    reads 20 columns forward, and its data gradient writes 18 of the 20 its destination has)."""
    plan = model._plans[(case.B, case.H, case.W, 0)]
    maps = [(('act', ind), a.t, a.C, a.ld) for ind, a in enumerate(plan.acts) if a is not None and a.off == 0]
    n = 0
    for name, t, C, ld in maps:
        if C % 4 and ld == T._pad4(C) and t.numel() % ld == 0:
            pad = t.view(-1, ld)[:, C:]
            assert not bool(pad.ne(0).any()), (case.id, name, 'padding channels written')      # (NaN != 0 as well)
            n += 1
    return n


def _eval(model, case, seed):
    r64, r32 = T.reference(case, seed)
    model.eval()
    _poison()
    with torch.no_grad():
        y = model(T.make_input(case, seed).cuda())
    _check(case, 'y_eval', y.cpu().numpy(), r64.y_eval, r32.y_eval, FLOOR_Y)


def _train_step(model, case, seed, stats=True, params=True):
    """One training forward + backward of (y * probe).sum() against the reference; returns dL/dx."""
    r64, r32 = T.reference(case, seed)
    model.train()
    model.zero_grad(set_to_none=True)
    xg = T.make_input(case, seed).cuda().requires_grad_(True)
    _poison()
    y = model(xg)
    _check(case, 'y_train', y.detach().cpu().numpy(), r64.y_train, r32.y_train, FLOOR_Y)
    if stats:
        for n, b in model.named_buffers():
            if 'running' in n:
                d = float((b.cpu().double() - r64.stats[n]).abs().max())
                print('TOPO %s stat:%s maxabs %.3e' % (case.id, n, d))
                np.testing.assert_allclose(b.cpu().numpy(), r64.stats[n].numpy(), rtol=1e-4, atol=1e-5, err_msg=n)
    _poison()
    (y * T.make_probe(case, seed, y.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    _check(case, 'dx', xg.grad.cpu().numpy(), r64.dx, r32.dx, FLOOR_Y)
    for n, p in model.named_parameters():
        if not params:
            assert p.grad is None, n
        elif r64.grads[n] is None:
            assert p.grad is None, (case.id, n)          # a dead branch: no gradient, as in the reference
        else:
            assert p.grad is not None, (case.id, n)
            _check(case, 'grad:' + n, p.grad.cpu().numpy(), r64.grads[n], r32.grads[n], FLOOR_G)
    npad = _padding_is_zero(model, case)
    assert npad or 'pad_before_conv' not in T.features(T.blocks_of(case), case.B, case.H, case.W), case.id
    return xg.grad.detach().cpu()


# ---------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize('case', T.FLOAT, ids=ids(T.FLOAT))
def test_float_case(case, monkeypatch):
    model = _model(case, monkeypatch)
    seed = T.seed_of(case)
    _eval(model, case, seed)
    _train_step(model, case, seed)


@pytest.mark.parametrize('case', T.EXACT + T.XS2, ids=ids(T.EXACT + T.XS2))
def test_exact_case(case, monkeypatch):
    """Integer data below the 2^24 budget: fp32 is exact in any summation order, so the product's numbers ARE the float64
    reference's."""
    from singleshotpose_amd.engine import wino_tile
    model = _model(case, monkeypatch)
    r64, _ = T.reference(case, 0)
    x = T.make_input(case, 0).cuda()
    model.eval()
    _poison()
    with torch.no_grad():
        y_eval = model(x).cpu()
    model.train()
    xg = x.clone().requires_grad_(True)
    _poison()
    y = model(xg)
    _poison()
    (y * T.make_probe(case, 0, y.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    plan = model._plans[(case.B, case.H, case.W, 0)]
    for cs in plan.convs.values():       # F(4x4) Winograd is the one code family that is not exact on integers
        assert wino_tile(cs.plan_fwd) != 4 and wino_tile(cs.plan_dgrad) != 4 and cs.wgrad_wino != 4, cs.ind
    names = ('b', 'c', 'y', 'x') if y.dim() == 4 else ('b', 'c')
    for what, got, want in [('y_eval', y_eval, r64.y_eval), ('y_train', y.detach().cpu(), r64.y_train)]:
        assert torch.equal(got, want.float()), (case.id, what, first_diffs(got, want.float(), names))
    assert torch.equal(xg.grad.cpu(), r64.dx.float()), (case.id, 'dx', first_diffs(xg.grad.cpu(), r64.dx.float(),
                                                                                 ('b', 'c', 'y', 'x')))
    for n, p in model.named_parameters():
        if r64.grads[n] is None:
            assert p.grad is None, (case.id, n)
            continue
        assert p.grad is not None, (case.id, n)
        got, want = p.grad.cpu().contiguous(), r64.grads[n].float()
        assert torch.equal(got, want), (case.id, n, first_diffs(got, want, ('co', 'ci', 'ky', 'kx')[:got.dim()]))
    _padding_is_zero(model, case)


PADDED = [c for c in T.FLOAT if 's2_after_pad' in T.features(T.blocks_of(c), c.B, c.H, c.W)]


@pytest.mark.parametrize('case', PADDED, ids=ids(PADDED))
def test_strided_block_behind_a_padded_map_on_later_steps(case, monkeypatch):
    """A strided data gradient writes Cin_dx of the pad4(Cin_dx) columns of its producer's gradient buffer; what the other
    columns hold (here: NaN) must not travel through the producer's in-place backward into its next forward.  Three
    training steps and an eval forward of ONE plan, every one at the bars of the first."""
    model = _model(case, monkeypatch)
    seed = T.seed_of(case)
    for step in range(3):
        _train_step(model, case, seed, stats=step == 0)
    _reset_stats(model, case)
    _eval(model, case, seed)


# ---------------------------------------------------------------------------------------------------- other routes
def _reset_stats(model, case):
    """The running statistics back at the case's seeded values (a training forward moved them), in place."""
    fresh = T.make_model(case)
    with torch.no_grad():
        for (_, t), (_, s) in zip(model.named_buffers(), fresh.named_buffers()):
            t.copy_(s)


MULTI = [T.CASES[i] for i in T.ROUTES]


@pytest.mark.parametrize('case', MULTI, ids=ids(MULTI))
def test_input_only_backward_gives_the_same_dx(case, monkeypatch):
    model = _model(case, monkeypatch)
    seed = T.seed_of(case)
    full = _train_step(model, case, seed, stats=False)
    for p in model.parameters():
        p.requires_grad_(False)
    # (the running statistics moved, the batch statistics the training forward normalises with did not)
    only = _train_step(model, case, seed, stats=False, params=False)
    err = rel_err(only.numpy(), full.numpy())
    print('TOPO %s dx_only_vs_full err %.3e' % (case.id, err))
    assert err <= FLOOR_Y


@pytest.mark.parametrize('case', MULTI, ids=ids(MULTI))
def test_graph_replay_equals_eager_eval(case, monkeypatch):
    model = _model(case, monkeypatch).eval()
    seed = T.seed_of(case)
    x = T.make_input(case, seed).cuda()
    with torch.no_grad():
        eager = model(x).cpu()
        plan = model._plans[(case.B, case.H, case.W, 0)]
        first = plan.forward_graph(x).cpu()         # captures
        again = plan.forward_graph(x).cpu()         # replays
    assert plan._graph is not None and not plan._graph_failed
    assert torch.equal(first, eager) and torch.equal(again, eager)
    r64, r32 = T.reference(case, seed)
    _check(case, 'y_graph', again.numpy(), r64.y_eval, r32.y_eval, FLOOR_Y)


@pytest.mark.parametrize('case', MULTI, ids=ids(MULTI))
def test_second_step_after_in_place_weight_change(case, monkeypatch):
    model = _model(case, monkeypatch)
    _train_step(model, case, T.seed_of(case))
    nplans = len(model._plans)
    step2 = T.variant(case, 'step2')
    fresh = T.make_model(step2)
    with torch.no_grad():
        for (n, t), (_, s) in zip(list(model.named_parameters()) + list(model.named_buffers()),
                                  list(fresh.named_parameters()) + list(fresh.named_buffers())):
            t.copy_(s)
    _train_step(model, step2, T.seed_of(step2))
    assert len(model._plans) == nplans         # the same plan ran both steps
    _reset_stats(model, step2)
    _eval(model, step2, T.seed_of(step2))


@pytest.mark.parametrize('case', MULTI, ids=ids(MULTI))
def test_both_batchnorm_backward_forms(case, monkeypatch):
    blocks = T.blocks_of(case)
    want = T.expected_bn_fuse(blocks, case.B, case.H, case.W)
    dxs = []
    for on in ('0', '1'):
        monkeypatch.setenv('SSP_BN_FUSE', on)
        model = _model(case, monkeypatch)
        dxs.append(_train_step(model, case, T.seed_of(case)))
        plan = model._plans[(case.B, case.H, case.W, 0)]
        fused = {cs.ind: cs.bn_fuse_src.ind for cs in plan.convs.values() if cs.bn_fuse_src is not None}
        assert fused == (want if on == '1' else {})
    err = rel_err(dxs[0].numpy(), dxs[1].numpy())
    print('TOPO %s dx_fuse0_vs_fuse1 err %.3e' % (case.id, err))
    assert err <= FLOOR_Y


@pytest.mark.parametrize('case', MULTI, ids=ids(MULTI))
def test_second_batch_size_and_resolution(case, monkeypatch):
    model = _model(case, monkeypatch)
    _train_step(model, case, T.seed_of(case))
    for what in ('b1', 'res2'):
        v = T.variant(case, what)
        _reset_stats(model, v)
        _eval(model, v, T.seed_of(v))
        _train_step(model, v, T.seed_of(v))
    shapes = set(k[:3] for k in model._plans)
    assert shapes == {(case.B, case.H, case.W), (1, case.H, case.W), (case.B, case.H + 8, case.W + 8)}


# ---------------------------------------------------------------------------------------------------- tuned plans
WIDE = [T.CASES[i] for i in T.TUNED]


@pytest.mark.parametrize('case', WIDE, ids=ids(WIDE))
def test_tuned_plan(case, monkeypatch):
    """The same numbers with the tuner on (timed forward / data-gradient / filter-gradient choices, the head-error budget):
    64-channel 3x3 layers are where it has Winograd and split-K candidates to pick from."""
    model = _model(case, monkeypatch, autotune='1')
    seed = T.seed_of(case)
    _eval(model, case, seed)
    _train_step(model, case, seed)
    plan = model._plans[(case.B, case.H, case.W, 0)]
    assert plan._tune
    print('TOPO %s codes %s' % (case.id, [(cs.ind, cs.plan_fwd, cs.plan_dgrad, cs.wgrad_wino) for cs in plan.convs.values()]))
    if case.id == 'wide-4':
        # layer 3 (stride 2) and layer 4 (stride 1) launch data gradients of one shape key: the tuner skips the strided block,
        # not its neighbour, and not the stride-1 layer that reads the map the strided block reads
        # (a 64 -> 64 layer of these small maps may well keep code 0 after being timed - wide-0's do - so "was tuned" is
        # read off the tune cache: both stride-1 layers have their data- and filter-gradient entries there, and run them)
        from singleshotpose_amd import engine
        wide = {cs.ind: cs for cs in plan.convs.values() if cs.k == 3 and cs.cin == 64 and cs.cout == 64}
        assert sorted((i, cs.stride) for i, cs in wide.items()) == [(3, 2), (4, 1), (6, 1)]
        assert plan._dgrad_key(wide[3]) == plan._dgrad_key(wide[4])
        assert (wide[3].plan_fwd, wide[3].plan_dgrad, wide[3].wgrad_wino) == (0, 0, 0)
        for i in (4, 6):
            cs = wide[i]
            for key, code in ((plan._dgrad_key(cs), cs.plan_dgrad), (plan._wgrad_key(cs), cs.wgrad_wino)):
                assert key in engine._TUNE_CACHE, (i, key)
                assert code in (engine._TUNE_CACHE[key], 0), (i, key, code, engine._TUNE_CACHE[key])

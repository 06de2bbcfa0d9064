"""Fine-tuning with frozen layers and eval-mode BatchNorm on stride-2, depthwise and upsample blocks, on the MI355X: every
(net, pattern) of tests/finetune_block_cases.py through Darknet + engine.Plan against its float64 CPU reference, which takes
each BatchNorm's mode from the pattern.  One training step of (y * probe).sum() with the modes and requires_grad flags set
before the first forward, in the product's default mode, SSP_AUTOTUNE=0, the caching allocator poisoned with NaN before every
forward and backward (a gradient buffer that is read without having been written shows).

Bars of tests/test_gpu_depthwise.py: max(floor, 3 x the float32 CPU reference's own distance to float64), floors 1e-4 (output,
dL/dx) and 3e-4 (parameter gradients); the exact twins bit for bit.  A frozen parameter has no gradient and its range of the
flat gradient buffer is exactly zero; an eval-mode BatchNorm's running statistics are bit-unchanged, a training-mode one's
match the reference.  Launch counts come from the schedule restated in finetune_block_cases, never from the plan.  Every
figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import finetune_block_cases as C
from exact_conv import first_diffs
from helpers import rel_err
from test_gpu_depthwise import FLOOR_G, FLOOR_Y, _poison

pytestmark = pytest.mark.gpu
DIMS = ('co', 'ci', 'ky', 'kx')


def _model(case, pat, monkeypatch, det=None):
    monkeypatch.setenv('SSP_AUTOTUNE', '0')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    model = C.make_model(case).cuda()
    if det is not None:
        model.deterministic = det
    return C.apply_pattern(model, pat)


def _plan_of(model, case):
    assert len(model._plans) == 1
    return model._plans[(case.B, case.H, case.W, 0)]


def _step(model, case, pat, seed):
    """One training step under the pattern: (y, dL/dx or None, {name: gradient or None}), all on the CPU."""
    model.zero_grad(set_to_none=True)
    x = C.make_input(case, seed).cuda().requires_grad_(pat.want_input)
    _poison()
    y = model(x)
    _poison()
    (y * C.make_probe(case, seed, y.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {'models.' + n: (None if p.grad is None else p.grad.detach().cpu().contiguous()) for n, p in model.models.named_parameters()}
    return y.detach().cpu(), (x.grad.detach().cpu() if pat.want_input else None), grads


def _frozen_ranges_are_zero(model, case, pat):
    if not any(any(o) for o in pat.own.values()):
        return          # an input-only backward has no flat gradient buffer
    plan = _plan_of(model, case)
    flat = plan.last_flat_grad
    for n, p in model.models.named_parameters():
        if not C.trainable(pat, n):
            off, numel, _ = plan.grad_layout[id(p)]
            assert float(flat[off:off + numel].abs().max()) == 0.0, (case.id, pat.id, n)       # (a NaN fails: not ==)


def _check(case, pat, what, got, want64, want32, floor):
    err, own = rel_err(got.numpy(), want64.numpy()), rel_err(want32.numpy(), want64.numpy())
    bar = max(floor, 3.0 * own)
    print('FT %s %s %s err %.3e ref32 %.3e bar %.3e' % (case.id, pat.id, what, err, own, bar))
    assert tuple(got.shape) == tuple(want64.shape), (case.id, pat.id, what, got.shape, want64.shape)
    assert err <= bar, (case.id, pat.id, what, err, bar)      # (a NaN fails: not <=)


def _float_step(case, pat, monkeypatch, det=None):
    model = _model(case, pat, monkeypatch, det)
    r64, r32 = C.reference(case, pat)
    before = {n: b.detach().cpu().clone() for n, b in model.models.named_buffers() if 'running' in n}
    y, dx, grads = _step(model, case, pat, C.seed_of(case, pat))
    _check(case, pat, 'y', y, r64.y, r32.y, FLOOR_Y)
    if pat.want_input:
        _check(case, pat, 'dx', dx, r64.dx, r32.dx, FLOOR_Y)
    n_train = 0
    for n, g in grads.items():
        if C.trainable(pat, n[len('models.'):]):
            assert g is not None, (case.id, pat.id, n)
            _check(case, pat, 'grad:' + n, g, r64.grads[n], r32.grads[n], FLOOR_G)
            n_train += 1
        else:
            assert g is None, (case.id, pat.id, n)
    assert n_train >= 1 and n_train == sum(sum(o) for o in pat.own.values())
    _frozen_ranges_are_zero(model, case, pat)
    n_eval = 0
    for n, b in model.models.named_buffers():
        if 'running' not in n:
            continue
        if pat.bn_train[int(n.split('.')[0])]:
            assert not torch.equal(b.cpu(), before[n]), n
            np.testing.assert_allclose(b.cpu().numpy(), r64.stats['models.' + n].numpy(), rtol=1e-4, atol=1e-5, err_msg=n)
        else:
            assert torch.equal(b.cpu(), before[n]), (case.id, pat.id, n)       # an eval() module's statistics are bit-unchanged
            n_eval += 1
    assert n_eval == 2 * sum(1 for i, bn in C.conv_layers(case).items() if bn and not pat.bn_train[i])
    plan = _plan_of(model, case)
    want = C.PLANS[case.id]
    assert plan.depthwise == want['depthwise'] and plan.upsample == want['upsample'] and plan.fused_pool == want['fused_pool']
    assert {i: cs.bn_fuse_src.ind for i, cs in plan.convs.items() if cs.bn_fuse_src is not None} == want['bn_pairs']
    return y, dx, grads


# ---------------------------------------------------------------------------------------------------- float patterns
@pytest.mark.parametrize('cp', C.FLOAT_PATTERNS, ids=C.pid)
def test_float_pattern(cp, monkeypatch):
    _float_step(cp[0], cp[1], monkeypatch)


# ---------------------------------------------------------------------------------------------------- exact patterns
def _exact_check(case, pat, got, r64):
    y, dx, grads = got
    assert torch.equal(y, r64.y.float()), (case.id, pat.id, 'y', first_diffs(y, r64.y.float(), ('b', 'c', 'y', 'x')))
    if pat.want_input:
        assert torch.equal(dx, r64.dx.float()), (case.id, pat.id, 'dx', first_diffs(dx, r64.dx.float(), ('b', 'c', 'y', 'x')))
    for n, g in grads.items():
        if C.trainable(pat, n[len('models.'):]):
            want = r64.grads[n].float()
            assert g is not None, (case.id, pat.id, n)
            assert torch.equal(g, want), (case.id, pat.id, n, first_diffs(g, want, DIMS[:g.dim()]))
        else:
            assert g is None, (case.id, pat.id, n)


@pytest.mark.parametrize('cp', C.EXACT_PATTERNS, ids=C.pid)
def test_exact_pattern_equals_float64(cp, monkeypatch):
    """Integer data below the 2^24 budget: fp32 is exact in any summation order, so the product's numbers ARE float64's."""
    case, pat = cp
    model = _model(case, pat, monkeypatch)
    r64, _ = C.reference(case, pat)
    _exact_check(case, pat, _step(model, case, pat, C.XSEED), r64)
    _frozen_ranges_are_zero(model, case, pat)
    plan = _plan_of(model, case)
    assert plan.depthwise == C.PLANS[case.id]['depthwise'] and plan.upsample == C.PLANS[case.id]['upsample']


def test_one_plan_under_changing_schedules(monkeypatch):
    """One model, one plan, six schedules in a row: a gradient-buffer alias (the upsample's gradient IS columns of its
    route's) or an accumulate flag that survived from an earlier schedule would change the integers of a later one."""
    case = C.FTX_MIX
    seq = [C.everything(case, True), C.prefix_eval(case, 8), C.sandwich(case, 4), C.everything(case, True), C.prefix_eval(case, 3),
           C.input_only(case)]
    model = _model(case, seq[0], monkeypatch)
    r64, _ = C.reference(case, seq[0])
    for n, pat in enumerate(seq):
        C.apply_pattern(model, pat)
        got = _step(model, case, pat, C.XSEED)
        print('FT %s pass %d %s: %d gradients' % (case.id, n, pat.id, sum(g is not None for g in got[2].values())))
        _exact_check(case, pat, got, r64)
        _frozen_ranges_are_zero(model, case, pat)
        assert len(model._plans) == 1, (n, pat.id)


# ---------------------------------------------------------------------------------------------------- launch logs
def _record(monkeypatch):
    from singleshotpose_amd import _lib
    log = []
    orig = _lib.call

    def rec(name, *args):
        log.append(name)
        return orig(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)
    return log


@pytest.mark.parametrize('cp', C.FLOAT_PATTERNS + C.EXACT_PATTERNS, ids=C.pid)
def test_launch_log_follows_the_restated_schedule(cp, monkeypatch):
    case, pat = cp
    model = _model(case, pat, monkeypatch)
    seed = C.seed_of(case, pat)
    _step(model, case, pat, seed)          # plan construction, first-batch bookkeeping
    log = _record(monkeypatch)
    _step(model, case, pat, seed)
    got, want = C.counted(log), C.expected_launches(case, pat)
    print('FT %s %s launches %s' % (case.id, pat.id, ' '.join('%s=%d' % (k, got[k]) for k in C.COUNTED if got[k] or want[k])))
    assert {k: got[k] for k in C.COUNTED} == {k: want[k] for k in C.COUNTED}
    assert 'ssp_conv_s2_dgrad_ordered' not in log and 'ssp_conv_wgrad_ordered' not in log          # the default mode
    key = (case.id, pat.id)
    if key in (('ft_mix', 'prefix-eval-3'), ('ft_mix', 'prefix-eval-5')):
        # the frozen trunk takes the one-launch affine forward
        assert log.count('ssp_conv_s2_fwd_affine') == 1 and log.count('ssp_dwconv_fwd_affine') == (1 if pat.id.endswith('3') else 2)
    if key == ('ft_dw_pool', 'prefix-eval-5'):
        # pooled blocks cannot: the conv without statistics, then ssp_bn_act_fwd on the running-statistics affine
        assert log.count('ssp_dwconv_fwd_affine') == 0 and log.count('ssp_dwconv_fwd') == 2
        assert log.count('ssp_bn_fwd_finalize') == 1 and log.count('ssp_bn_act_fwd') == 3
    if key == ('ft_two_branch', 'branch-1-7-8'):
        assert log.count('ssp_upsample_bwd') == 0 and log.count('ssp_upsample_fwd') == 1


# ---------------------------------------------------------------------------------------------------- deterministic mode
@pytest.mark.parametrize('cp', [(C.FT_MIX, C.pattern(C.FT_MIX, 'prefix-eval-3')), (C.FT_S2_ODD, C.pattern(C.FT_S2_ODD, 'sandwich-3'))],
                         ids=C.pid)
def test_deterministic_mode_same_bars_and_identical_bits(cp, monkeypatch):
    case, pat = cp
    runs = []
    for _ in range(2):
        runs.append(_float_step(case, pat, monkeypatch, det=True))
    (ya, dxa, ga), (yb, dxb, gb) = runs
    assert torch.equal(ya, yb)
    for n in ga:
        if ga[n] is not None:
            print('FT %s %s deterministic %s: %d elements differ between two runs' % (case.id, pat.id, n, int((ga[n] != gb[n]).sum())))
            assert torch.equal(ga[n], gb[n]), n

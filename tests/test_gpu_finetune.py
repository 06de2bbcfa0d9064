"""Fine-tuning with frozen layers on the GPU: every BatchNorm block in its own module's mode, a backward that runs only
what the trainable parameters need, and the one-launch SGD over a segment table (parameter groups, subset optimizers).

The reference is torch autograd in float64 on a deep copy of the module tree that KEEPS each module's `training` and each
parameter's `requires_grad` flag.  Bars: forward 1e-4, gradients TOL = 3e-4 (tests/test_gpu_input_grad.py); between two
runs of the product itself, 4x the distance between two identical all-trainable steps, floor 1e-6 (the generic
filter-gradient kernels sum with fp32 atomics).

Forwards are compared with the reference as it is.  Gradients are compared in the project's decision-frozen mode
(oracle/darknet_ref.py forward_ref, tests/test_gpu_input_grad.py::_decisions): the reference takes every leaky branch and
every fused max-pool winner the product took, and the value of each raw conv output from the product (its gradient still
flows into the reference's own convolution).  Two independent forwards flip a branch wherever a pre-activation is within
rounding of a decision, and on the 3 x 3 maps of tiny-pose.cfg one flipped pool winner moves a filter gradient by 10 % -
measured here on the all-trainable step as much as on a frozen one; both branches are valid fp32 results."""
import copy
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

import topology_cases as T
from helpers import GOLD, ROOT, load_state_into, rel_err
from sequence_cases import _ref_forward
from test_finetune_cpu import _expected, _own

pytestmark = pytest.mark.gpu
TOL = 3e-4
YOLO = os.path.join(ROOT, 'cfg', 'yolo-pose.cfg')
TINY = os.path.join(GOLD, 'tiny-pose.cfg')
SHAPES = {TINY: (2, 96, 96), YOLO: (2, 64, 64)}
TINY_CONVS = (0, 2, 4, 5, 6, 8, 10, 12, 13, 15, 18, 19)


# ---------------------------------------------------------------------------------------------------- helpers
def _model(cfg, seed=3):
    from oracle.darknet_ref import seeded_state
    from singleshotpose_amd.darknet import Darknet
    model = Darknet(cfg)
    load_state_into(model, model.blocks, seeded_state(model.blocks, seed))
    return model.cuda().train()


def _convs(model):
    return [i for i, b in enumerate(model.blocks[1:]) if b['type'] == 'convolutional']


def _bn_of(model, ind):
    seq = model.models[ind]
    return seq[1] if len(seq) > 1 and isinstance(seq[1], torch.nn.BatchNorm2d) else None


def _freeze_before(model, k, params=True, bn_eval=False):
    for ind in _convs(model):
        if ind < k:
            if params:
                for p in model.models[ind].parameters():
                    p.requires_grad_(False)
            if bn_eval and _bn_of(model, ind) is not None:
                _bn_of(model, ind).eval()


def _input(cfg, seed=1):
    B, H, W = SHAPES[cfg]
    return torch.from_numpy(np.random.RandomState(seed).uniform(0, 1, (B, 3, H, W)).astype(np.float32))


def _probe(y, seed=5):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(tuple(y.shape)).astype(np.float32))


def _reference(model, x, probe=None, frozen=None):
    """(y, modules) of the float64 reference; with a probe, (y * probe).sum() is back-propagated into the copy."""
    mods = copy.deepcopy(model.models).cpu().double()
    for (_, a), (_, b) in zip(model.models.named_modules(), mods.named_modules()):
        assert a.training == b.training
    for a, b in zip(model.models.parameters(), mods.parameters()):
        assert a.requires_grad == b.requires_grad
    y = _ref_forward(model.blocks, mods, x.double(), frozen)
    if probe is not None:
        (y * probe.double()).sum().backward()
    return y.detach(), mods


def _kept_step(model, cfg, x):
    """One step with every block kept for backward: (y, gradients, the product's decisions of that forward)."""
    from test_gpu_input_grad import _decisions
    model.zero_grad(set_to_none=True)
    y = model(x)
    frozen = _decisions(model, *SHAPES[cfg])       # before backward: it rewrites the raw conv outputs in place
    (y * _probe(y).cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), [p.grad.detach().clone() for p in model.parameters()], frozen


def _step(model, x, want_x=False):
    model.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(want_x)
    y = model(xi)
    (y * _probe(y).cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]


def _record(monkeypatch):
    from singleshotpose_amd import _lib
    log = []
    orig = _lib.call

    def rec(name, *args):
        log.append(name)
        return orig(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)
    return log


def _spread_ok(b, a, c):
    """b against a under the spread of two identical runs a, c."""
    tol = max(4 * rel_err(c.cpu().numpy(), a.cpu().numpy()), 1e-6)
    return rel_err(b.cpu().numpy(), a.cpu().numpy()) <= tol


# ---------------------------------------------------------------------------------------------------- 1. BN mode
@pytest.mark.parametrize('cfg,k', [(TINY, 2), (TINY, 10), (YOLO, 2), (YOLO, 12)])
def test_batchnorm_mode_is_honoured_per_module(cfg, k):
    """model.train() with the BatchNorm modules of the blocks before conv k in eval() (k = 2: the first block alone - on
    yolo-pose.cfg the fused first block)."""
    model = _model(cfg)
    _freeze_before(model, k, params=False, bn_eval=True)
    before = {n: b.detach().clone() for n, b in model.models.named_buffers()}
    x = _input(cfg)
    yr, mods = _reference(model, x)
    y, grads, frozen = _kept_step(model, cfg, x.cuda())
    e = rel_err(y.cpu().numpy(), yr.numpy())
    print('forward rel err %.2e' % e)
    assert e < 1e-4
    ref = dict(mods.named_buffers())
    n_eval = n_train = 0
    for n, b in model.models.named_buffers():
        if 'running' not in n:
            continue
        if int(n.split('.')[0]) < k:
            assert torch.equal(b, before[n]), n           # an eval() module's statistics are bit-unchanged
            n_eval += 1
        else:
            assert not torch.equal(b, before[n]), n
            np.testing.assert_allclose(b.cpu().numpy(), ref[n].numpy(), rtol=1e-4, atol=1e-5, err_msg=n)
            n_train += 1
    assert n_eval >= 2 and n_train >= 2
    # the gradients through the eval-mode blocks are those of an affine map: everything trainable, same bars
    # (training-mode blocks normalise by batch statistics, eval-mode ones kept theirs: the updated buffers change nothing)
    _, mods = _reference(model, x, _probe(y), frozen)
    errs = [(rel_err(g.cpu().numpy(), r.grad.numpy()), n)
            for (n, _), g, r in zip(model.models.named_parameters(), grads, mods.parameters())]
    print('worst gradient rel err %.2e (%s)' % max(errs))
    assert max(errs)[0] < TOL, max(errs)


def test_train_mode_module_under_model_eval_uses_batch_statistics():
    model = _model(TINY).eval()
    _bn_of(model, 8).train()
    before = {n: b.detach().clone() for n, b in model.models.named_buffers() if 'running' in n}
    x = _input(TINY)
    yr, mods = _reference(model, x)
    with torch.no_grad():
        y = model(x.cuda())
    assert rel_err(y.cpu().numpy(), yr.numpy()) < 1e-4
    for n, b in model.models.named_buffers():
        if 'running' in n:
            assert torch.equal(b, before[n]) == (not n.startswith('8.')), n


# ---------------------------------------------------------------------------------------------------- 2. frozen prefix
def _frozen_case(model, cfg, freeze):
    """Two all-trainable steps (the spread), then freeze() and one more step: against the reference and the first step."""
    x = _input(cfg).cuda()
    _step(model, x)                       # plan construction, tuning, first-batch bookkeeping
    _, g0, frozen = _kept_step(model, cfg, x)
    _, g2 = _step(model, x)
    freeze()
    y, g1 = _step(model, x)
    yr, _ = _reference(model, x.cpu())
    assert rel_err(y.cpu().numpy(), yr.numpy()) < 1e-4
    _, mods = _reference(model, x.cpu(), _probe(y), frozen)       # (the same function: the all-trainable step's decisions)
    errs, spread = [], []
    for (n, p), a, b, c, r in zip(model.models.named_parameters(), g0, g1, g2, mods.parameters()):
        if not p.requires_grad:
            assert b is None and p.grad is None, n
            continue
        errs.append((rel_err(b.cpu().numpy(), r.grad.numpy()), n))
        spread.append((rel_err(b.cpu().numpy(), a.cpu().numpy()), rel_err(c.cpu().numpy(), a.cpu().numpy()), n))
    print('trainable %d, worst gradient rel err %.2e (%s), worst distance to the all-trainable step %.2e (two of those: '
          '%.2e)' % ((len(errs),) + max(errs) + max(spread)[:2]))
    assert len(errs) >= 1
    assert max(errs)[0] < TOL, max(errs)
    for d, s_, n in spread:
        assert d <= max(4 * s_, 1e-6), n
    # the frozen ranges of the flat gradient buffer stay zero
    plan = next(iter(model._plans.values()))
    flat = plan.last_flat_grad
    for p in model.models.parameters():
        if not p.requires_grad:
            off, n, _ = plan.grad_layout[id(p)]
            assert float(flat[off:off + n].abs().max()) == 0.0


@pytest.mark.parametrize('k', TINY_CONVS)
def test_frozen_prefix_gradients(k):
    """Parameters of the blocks before conv k frozen; BatchNorm of those blocks left in training mode for every other k and
    put in eval() for the rest (the modes are set BEFORE the all-trainable steps: they define the function)."""
    model = _model(TINY)
    bn_eval = TINY_CONVS.index(k) % 2 == 0
    _freeze_before(model, k, params=False, bn_eval=bn_eval)
    _frozen_case(model, TINY, lambda: _freeze_before(model, k))


def test_frozen_prefix_with_the_fused_first_block():
    model = _model(YOLO)
    _freeze_before(model, 2, params=False, bn_eval=True)
    _frozen_case(model, YOLO, lambda: _freeze_before(model, 2))


def test_frozen_sandwich_and_bn_only():
    # a frozen middle block: the gradient must pass through it to the trainable blocks in front of it
    model = _model(TINY)
    _bn_of(model, 8).eval()

    def freeze():
        for p in model.models[8].parameters():
            p.requires_grad_(False)
    _frozen_case(model, TINY, freeze)
    assert all(p.grad is not None for p in model.models[6].parameters())
    # only the BatchNorm parameters trainable
    model = _model(TINY)

    def freeze_convs():
        for n, p in model.models.named_parameters():
            p.requires_grad_('.bn' in n)
    _frozen_case(model, TINY, freeze_convs)


def _one_sided_shortcut():
    """(case, k): a topology case and a conv index such that, with the parameters of the convs before k frozen, a shortcut
    passes a gradient to only ONE of its two sources (the other derives from frozen blocks alone)."""
    from singleshotpose_amd import engine
    for case in T.FLOAT:
        if 'shortcut' not in T.features(T.blocks_of(case), case.B, case.H, case.W):
            continue
        model = T.make_model(case, init=False)
        plan = engine.Plan(model, case.B, case.H, case.W, torch.device('cpu'))
        for k in sorted(plan.convs)[1:]:
            ids = [id(p) for i, cs in plan.convs.items() if i >= k for p in model.models[i].parameters()]
            if any(s.kind == 'shortcut' and s.visited and sorted(s.dgrad) == [False, True]
                   for s in plan.backward_schedule(ids, False, True)):
                return case, k
    raise AssertionError("no topology case with a one-sided shortcut")


def test_frozen_prefix_through_a_shortcut():
    case, k = _one_sided_shortcut()
    model = T.make_model(case).cuda().train()
    dseed = T.SEEDS[case.id]
    x = T.make_input(case, dseed).cuda()
    probe = None

    def step():
        model.zero_grad(set_to_none=True)
        y = model(x)
        (y * T.make_probe(case, dseed, y.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]
    step()
    _, g0 = step()
    _, g2 = step()
    for i in _convs(model):
        if i < k:
            for p in model.models[i].parameters():
                p.requires_grad_(False)
    y, g1 = step()
    yr, mods, _ = T.ref_run(model, x.cpu(), True)      # (every module of these cases is in training mode)
    assert rel_err(y.cpu().numpy(), yr.detach().numpy()) < 1e-4
    (yr * T.make_probe(case, dseed, yr.shape).double()).sum().backward()
    n_train = 0
    for (n, p), a, b, c, r in zip(model.models.named_parameters(), g0, g1, g2, mods.parameters()):
        if not p.requires_grad:
            assert b is None and r.grad is None, n
        elif a is not None:            # (None: a dead branch)
            n_train += 1
            assert rel_err(b.cpu().numpy(), r.grad.numpy()) < TOL, n
            assert _spread_ok(b, a, c), n
    assert n_train >= 1


# ---------------------------------------------------------------------------------------------------- 3. launch log
def _count(log, *prefixes):
    return sum(1 for n in log if n.startswith(prefixes))


def _logged_step(model, cfg, monkeypatch):
    x = _input(cfg).cuda()
    _step(model, x)
    log = _record(monkeypatch)
    _step(model, x)
    return list(log)


@pytest.mark.parametrize('cfg,k', [(TINY, 0), (TINY, 5), (TINY, 10), (TINY, 15), (TINY, 18), (TINY, 19), (YOLO, 0),
                                   (YOLO, 2), (YOLO, 24)])
def test_launch_log_of_a_frozen_prefix(monkeypatch, cfg, k):
    from singleshotpose_amd import engine
    from singleshotpose_amd.cfg import parse_cfg
    model = _model(cfg)
    _freeze_before(model, k, bn_eval=True)
    log = _logged_step(model, cfg, monkeypatch)
    B, H, W = SHAPES[cfg]
    plan = next(iter(model._plans.values()))
    own, _ = _own(plan, lambda i, kind: i >= k)
    bn_train = {i: bool(cs.bn) and i >= k for i, cs in plan.convs.items()}
    exp = _expected(parse_cfg(cfg), B, H, W, own, False, bn_train)
    convs = _convs(model)
    visited = [i for i in convs if exp[i]['visited']]
    assert visited == [i for i in convs if i >= k]
    n_w = sum(1 for i in convs if i >= k)
    assert _count(log, 'ssp_conv_wgrad', 'ssp_first_bwd_wgrad') == n_w
    n_d = sum(1 for i in visited if exp[i]['dgrad'][0])
    assert _count(log, 'ssp_conv_dgrad') == n_d
    # nothing for a block that is not visited: the BatchNorm / activation backward, the bias column sum, the data-gradient
    # operand repack and its Winograd transform exist once per visited block that needs them
    n_act = sum(1 for i in visited if plan.convs[i].needs_act and not plan.convs[i].first_live)
    assert _count(log, 'ssp_bn_act_bwd') == n_act
    assert _count(log, 'ssp_first_bwd_reduce') == sum(1 for i in visited if plan.convs[i].first_live)
    assert _count(log, 'ssp_colsum') == sum(1 for i in visited if plan.convs[i].conv.bias is not None)
    assert _count(log, 'ssp_repack_dgrad') == n_d
    n_wino = sum(1 for cs in plan.convs.values() if engine.wino_tile(cs.plan_fwd)) + \
        sum(1 for i in visited if exp[i]['dgrad'][0] and engine.wino_tile(plan.convs[i].plan_dgrad))
    assert _count(log, 'ssp_wino_filter_transform_t') == n_wino
    if k == 0:
        assert n_d == len(convs) - 1      # nothing frozen: one data gradient per conv block but the first - today's step
        assert 'ssp_bn_act_bwd_affine' not in log and 'ssp_conv_fwd_affine' not in log
    else:
        # the frozen eval-BatchNorm prefix runs the inference chain: no statistics for it
        n_bn_train = sum(1 for i in convs if i >= k and plan.convs[i].bn)
        assert _count(log, 'ssp_bn_fwd_finalize') == n_bn_train
    if k == convs[-1]:
        # head only: one filter gradient, one column sum, no data gradient
        assert (n_w, n_d, _count(log, 'ssp_colsum')) == (1, 0, 1)
        assert _count(log, 'ssp_bn_act_bwd', 'ssp_first_bwd', 'ssp_repack_dgrad', 'ssp_unpack_grad') == 0


# ---------------------------------------------------------------------------------------------------- 4. the table kernel
LENS = (1, 2, 3, 4, 5, 7, 8, 1023, 1025, 4099)
TUPLES = ((0.1, 0.0, 0.0, 0.0, 0), (0.05, 0.9, 0.1, 0.0, 0), (0.02, 0.8, 0.0, 0.01, 1))      # plain; momentum + dampening; Nesterov + decay


def _table_fixture():
    g = torch.Generator().manual_seed(7)
    rows, po, go = [], 0, 16
    for i, n in enumerate(LENS):
        rows.append([po, 0, po, n, i % 3])
        po += (n + 3) // 4 * 4
    for r in reversed(rows):              # gradients in another order, with gaps
        r[1] = go
        go += (r[3] + 3) // 4 * 4 + 8
    p = torch.randn(po, generator=g).cuda()
    m = torch.randn(po, generator=g).cuda()
    gr = [torch.randn(go, generator=g).cuda() for _ in range(2)]
    return rows, p, m, gr


def _call_table(rows, tuples, p, g, m, st):
    from singleshotpose_amd import _lib
    host = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
    dev = torch.from_numpy(host).cuda()
    hyper = (ctypes.c_float * (6 * len(tuples)))(*[float(v) for t in tuples for v in t])
    _lib.call('ssp_sgd_step_table', p.data_ptr(), g.data_ptr(), m.data_ptr(), p.numel(), g.numel(), m.numel(),
              dev.data_ptr(), host.ctypes.data, len(rows), ctypes.cast(hyper, ctypes.c_void_p), len(tuples), st)
    torch.cuda.synchronize()


def test_sgd_table_is_bit_identical_to_per_segment_launches():
    from singleshotpose_amd import _lib
    rows, p, m, grads = _table_fixture()
    st = torch.cuda.current_stream().cuda_stream
    p2, m2 = p.clone(), m.clone()
    untouched = torch.ones(p.numel(), dtype=torch.bool)
    for r in rows:
        untouched[r[0]:r[0] + r[3]] = False
    for step, g in enumerate(grads):
        first = 1 if step == 0 else 0
        _call_table(rows, [t + (first,) for t in TUPLES], p, g, m, st)
        for po, go, mo, n, t in rows:
            lr, mom, damp, wd, nest = TUPLES[t]
            _lib.call('ssp_sgd_step', p2.data_ptr() + 4 * po, g.data_ptr() + 4 * go, m2.data_ptr() + 4 * mo, n, lr, mom, damp,
                      wd, nest, first, st)
        torch.cuda.synchronize()
        assert torch.equal(p, p2) and torch.equal(m, m2), step
    # the padding between segments was never written, segments without momentum left the momentum buffer alone
    _, p0, m0, _ = _table_fixture()
    assert torch.equal(p.cpu()[untouched], p0.cpu()[untouched]) and torch.equal(m.cpu()[untouched], m0.cpu()[untouched])
    for po, go, mo, n, t in rows:
        assert not torch.equal(p[po:po + n], p0[po:po + n])
        assert torch.equal(m[mo:mo + n], m0[mo:mo + n]) == (TUPLES[t][1] == 0)


@pytest.mark.parametrize('bad,why', [([0, 0, 0, 1 << 20, 0], 'outside'), ([1 << 30, 0, 0, 8, 0], 'outside'),
                                     ([0, 1 << 30, 0, 8, 0], 'outside'), ([0, 0, 1 << 30, 8, 1], 'outside'),
                                     ([2, 0, 0, 8, 0], 'multiples of 4'), ([0, 0, 0, 8, 3], 'tuple index')])
def test_sgd_table_refuses_a_bad_segment(bad, why):
    from singleshotpose_amd import _lib
    rows, p, m, grads = _table_fixture()
    keep = [t.clone() for t in (p, m, grads[0])]
    with pytest.raises(_lib.SspError, match=why):
        _call_table(rows[:3] + [bad] + rows[3:], [t + (0,) for t in TUPLES], p, grads[0], m,
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (p, m, grads[0])))


# ---------------------------------------------------------------------------------------------------- 5. grouped optimizer
def _groups(named):
    """The parameter-group list of train.py:381-387: no weight decay on BatchNorm and bias parameters."""
    out = []
    for key, value in named:
        bn_or_bias = key.find('.bn') >= 0 or key.find('.bias') >= 0
        out.append({'params': [value], 'weight_decay': 0.0 if bn_or_bias else 0.002})
    return out


def test_grouped_optimizer_is_one_table_launch(monkeypatch):
    from singleshotpose_amd.optim import SGD
    a, b = _model(TINY, 5), _model(TINY, 5)
    kw = dict(lr=2e-4, momentum=0.9)
    oa, ob = SGD(_groups(a.named_parameters()), **kw), SGD(_groups(b.named_parameters()), **kw)
    sh = [torch.nn.Parameter(p.detach().cpu().clone()) for p in a.parameters()]
    osh = torch.optim.SGD(_groups(zip([n for n, _ in a.named_parameters()], sh)), **kw)
    assert len(oa.param_groups) == len(sh) and len(set(g['weight_decay'] for g in oa.param_groups)) == 2
    log = _record(monkeypatch)
    for step in range(3):
        x = _input(TINY, 20 + step).cuda()
        if step == 2:
            for grp in oa.param_groups + ob.param_groups + osh.param_groups:
                grp['lr'] = grp['lr'] * 0.5          # train.py:44-45 rewrites lr: the tuples change, the table does not
        oa.zero_grad()
        y = a(x)
        (y * _probe(y).cuda()).sum().backward()
        for p, q, r in zip(a.parameters(), b.parameters(), sh):
            q.grad = p.grad.detach().clone()        # copies: no flat views - the twin takes the per-parameter launches
            r.grad = p.grad.detach().cpu().clone()
        table_before = None if oa._tab is None else oa._tab['dev'].data_ptr()
        del log[:]
        oa.step()
        assert log.count('ssp_sgd_step_table') == 1 and log.count('ssp_sgd_step') == 0, step
        if step:
            assert oa._tab['dev'].data_ptr() == table_before      # no per-step table upload
        del log[:]
        ob.step()
        assert log.count('ssp_sgd_step') == len(sh) and log.count('ssp_sgd_step_table') == 0
        osh.step()
        torch.cuda.synchronize()
        for (n, p), q, r in zip(a.named_parameters(), b.parameters(), sh):
            assert torch.equal(p.detach(), q.detach()), (step, n)
            assert torch.equal(oa.state[p]['momentum_buffer'], ob.state[q]['momentum_buffer']), (step, n)
            assert rel_err(p.detach().cpu().numpy(), r.detach().numpy()) < 1e-6, (step, n)
            assert rel_err(oa.state[p]['momentum_buffer'].cpu().numpy(), osh.state[r]['momentum_buffer'].numpy()) < 1e-6
    assert oa.table_steps == 3 and oa.fused_steps == 0 and ob.table_steps == 0
    assert oa.flat_numel == sum((p.numel() + 3) // 4 * 4 for p in a.parameters())


# ---------------------------------------------------------------------------------------------------- 6. subset optimizer
def test_subset_optimizer_touches_only_what_it_holds(monkeypatch):
    from singleshotpose_amd.optim import SGD
    model = _model(TINY, 5)
    head = list(model.models[19].parameters())
    _freeze_before(model, 19, bn_eval=True)
    frozen = {n: t.detach().clone() for n, t in list(model.models.named_parameters()) + list(model.models.named_buffers())
              if not n.startswith('19.')}
    kw = dict(lr=1e-3, momentum=0.9, weight_decay=0.01)
    opt = SGD(head, **kw)
    sh = [torch.nn.Parameter(p.detach().cpu().clone()) for p in head]
    start = [p.detach().cpu().clone() for p in head]
    osh = torch.optim.SGD(sh, **kw)
    log = _record(monkeypatch)
    for step in range(3):
        x = _input(TINY, 30 + step).cuda()
        opt.zero_grad()
        y = model(x)
        (y * _probe(y).cuda()).sum().backward()
        for p, r in zip(head, sh):
            r.grad = p.grad.detach().cpu().clone()
        opt.step()
        osh.step()
    torch.cuda.synchronize()
    assert opt.table_steps == 3 and log.count('ssp_sgd_step_table') == 3 and log.count('ssp_sgd_step') == 0
    assert 0 < opt.flat_numel <= sum((p.numel() + 3) // 4 * 4 for p in head)
    now = dict(list(model.models.named_parameters()) + list(model.models.named_buffers()))
    for n, t in frozen.items():
        assert torch.equal(now[n].detach(), t), n      # a frozen weight does not decay, an eval() BatchNorm keeps its statistics
    for p, r in zip(head, sh):
        assert rel_err(p.detach().cpu().numpy(), r.detach().numpy()) < 1e-6
    assert all(not torch.equal(p.detach().cpu(), q) for p, q in zip(head, start))


# ---------------------------------------------------------------------------------------------------- 7. reducer
def test_frozen_prefix_step_with_a_reducer():
    import torch.distributed as dist
    from singleshotpose_amd.dist import GradReducer, init_distributed
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1')
    init_distributed('nccl')
    try:
        x = _input(TINY).cuda()

        def run(with_reducer):
            model = _model(TINY, 41)
            _freeze_before(model, 10, bn_eval=True)
            red = GradReducer(model, 1, bucket_bytes=16 << 10, force=True) if with_reducer else None
            out = []
            for _ in range(3 if not with_reducer else 1):
                _, g = _step(model, x)
                if red is not None:
                    red.all_reduce()
                    plan = next(iter(model._plans.values()))
                    # every bucket was launched: together they cover the whole flat buffer, in order
                    assert red.launched[0][0] == 0 and red.launched[-1][1] == plan.grad_total and len(red.launched) >= 2
                    assert all(a[1] == b[0] for a, b in zip(red.launched[:-1], red.launched[1:]))
                torch.cuda.synchronize()
                out.append([None if t is None else t.clone() for t in g])
            return out
        plain, reduced = run(False), run(True)
        for a, c, b in zip(plain[1], plain[2], reduced[0]):
            assert (a is None) == (b is None)
            if a is not None:
                assert _spread_ok(b, a, c)
    finally:
        dist.destroy_process_group()

"""Fused Adam / AdamW (ssp_adam_step, ssp_adam_step_table, singleshotpose_amd.optim.Adam / AdamW) on the GPU.

Kernel level, through the C ABI: against the float64 statement of adam_cases.py under the bar max(2 * e_torch, 2^-23)
(e_torch = what torch.optim.Adam in fp32 on the CPU loses against the same statement on the same inputs, computed here),
bitwise identity of the single-range, table and per-segment paths with NaN-poisoned gaps, every refusal.  Optimizer level:
the tiny net trained on the HIP path, shadowed by torch.optim.Adam / AdamW on the CPU fed the GPU run's own gradients
(test_gpu_optim.py's method and bar, rel_err < 1e-6).  Nothing is compared with the code under test."""
import ctypes
import os

import numpy as np
import pytest
import torch

import adam_cases as A
from helpers import GOLD, load_state_into, make_targets, rel_err

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -23      # one fp32 ulp of the largest element: the final store alone can cost it
STEPS = 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _args(h, step, lr=None):
    lr = h.lr if lr is None else lr
    step_size, bc2_sqrt = A.bias_corrections(h._replace(lr=lr), step)
    return (lr, h.beta1, h.beta2, h.eps, h.weight_decay, step_size, bc2_sqrt, 1 if h.decoupled else 0, 1 if h.amsgrad else 0)


def _single(p, g, m, v, x, n, h, step, lr=None, off=(0, 0, 0)):
    from singleshotpose_amd import _lib
    po, go, so = off
    _lib.call('ssp_adam_step', p.data_ptr() + 4 * po, g.data_ptr() + 4 * go, m.data_ptr() + 4 * so, v.data_ptr() + 4 * so,
              x.data_ptr() + 4 * so if h.amsgrad else None, n, *(_args(h, step, lr) + (_stream(),)))


def _table(p, g, m, v, x, rows, tuples, ams=None):
    """rows [[po, go, so, len, tuple]], tuples [(Hyper, step, lr)] or the nine raw figures of a tuple"""
    from singleshotpose_amd import _lib
    host = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
    dev = torch.from_numpy(host).cuda()
    raw = [t if len(t) == 9 else _args(*t) for t in tuples]
    flat = [float(a) for t in raw for a in t]
    hyper = (ctypes.c_double * len(flat))(*flat)
    ams = any(t[8] for t in raw) if ams is None else ams
    _lib.call('ssp_adam_step_table', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), x.data_ptr() if ams else None,
              p.numel(), g.numel(), m.numel(), dev.data_ptr(), host.ctypes.data, len(rows),
              ctypes.cast(hyper, ctypes.c_void_p), len(tuples), _stream())
    torch.cuda.synchronize()      # (dev and hyper stay alive until the launch is done)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _torch_opt(h, params):
    cls = torch.optim.AdamW if h.decoupled else torch.optim.Adam
    return cls(params, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=h.weight_decay, amsgrad=h.amsgrad)


# ------------------------------------------------------------------------------------------------ kernel against the statement
@pytest.mark.parametrize('n,h', A.KERNEL_CASES, ids=lambda v: v.name if isinstance(v, A.Hyper) else str(v))
def test_kernel_against_the_float64_statement(n, h):
    """Three steps (the state and both bias corrections move, lr is rewritten before the last) through ssp_adam_step and,
    from the same start, through a one-row ssp_adam_step_table: the two give the same bits, and p, m, v (vmax) stay
    within max(2 * e_torch, 2^-23) of the float64 statement."""
    p0, grads = A.inputs(n, A.SEED + n, STEPS)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = _torch_opt(h, [q])
    ref = [p0.astype(np.float64), np.zeros(n), np.zeros(n), np.zeros(n)]
    dev = [torch.from_numpy(p0.copy()).cuda()] + [torch.zeros(n, device='cuda') for _ in range(3)]
    tab = [t.clone() for t in dev]
    for step, g in enumerate(grads):
        lr = h.lr * (0.5 if step == STEPS - 1 else 1.0)
        for grp in opt.param_groups:
            grp['lr'] = lr
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        ref = list(A.adam_statement(ref[0], g, ref[1], ref[2], ref[3], h, step + 1, lr=lr))
        gd = torch.from_numpy(g).cuda()
        _single(dev[0], gd, dev[1], dev[2], dev[3], n, h, step + 1, lr)
        _table(tab[0], gd, tab[1], tab[2], tab[3], [[0, 0, 0, n, 0]], [(h, step + 1, lr)])
    torch.cuda.synchronize()
    st = opt.state[q]
    theirs = [q.detach().numpy(), st['exp_avg'].numpy(), st['exp_avg_sq'].numpy()] + ([st['max_exp_avg_sq'].numpy()] if h.amsgrad else [])
    for name, ours, table, torch_cpu, want in zip(('p', 'm', 'v', 'vmax'), dev, tab, theirs, ref):
        assert np.array_equal(_bits(ours), _bits(table)), name
        e_torch, e_kernel = rel_err(torch_cpu, want), rel_err(ours.cpu().numpy(), want)
        print('ADAM n=%d %s %s: e_kernel %.3e e_torch %.3e' % (n, h.name, name, e_kernel, e_torch))
        assert e_kernel <= max(2 * e_torch, FLOOR), (name, e_kernel, e_torch)
    if not h.amsgrad:
        assert not dev[3].any()      # without amsgrad the fifth buffer is never touched


# ------------------------------------------------------------------------------------------------ three paths, bit for bit
@pytest.mark.parametrize('ams', [False, True], ids=['plain', 'amsgrad'])
def test_single_range_table_and_per_segment_launches_agree_bit_for_bit(ams):
    """~300 segments of lengths 1 ... 40 and one of 2049 * 4096 + 3 floats (more chunks than workgroups: the walk wraps),
    three hyper-parameter tuples, at different offsets in the parameter, gradient and state buffers.  The floats between
    segments carry a NaN bit pattern: in p / m / v / vmax they come back bit-identical, in g they reach no result."""
    rows4, np_, ng, ns = A.segment_layout(A.LENGTHS[-1])
    base = A.HYPERS[6] if ams else A.HYPERS[4]
    tuples = [(base, 2, None), (base._replace(weight_decay=0.0, decoupled=False), 5, 3e-4), (base._replace(eps=1e-3, beta2=0.99), 2, None)]
    rows = [r + [i % 3] for i, r in enumerate(rows4)]
    rs = np.random.RandomState(A.SEED + 7)
    host = {k: A.poisoned(n) for k, n in (('p', np_), ('g', ng), ('m', ns), ('v', ns), ('x', ns))}
    for po, go, so, n, t in rows:
        host['p'][po:po + n] = rs.standard_normal(n)
        host['g'][go:go + n] = rs.standard_normal(n) * 0.1
        host['m'][so:so + n] = rs.standard_normal(n) * 0.05
        host['v'][so:so + n] = rs.uniform(0, 1e-2, n)
        host['x'][so:so + n] = rs.uniform(0, 1e-2, n)
    make = lambda: {k: torch.from_numpy(a.copy()).cuda() for k, a in host.items()}
    # (a) one table launch
    a = make()
    _table(a['p'], a['g'], a['m'], a['v'], a['x'], rows, tuples, ams)
    # (b) one ssp_adam_step per segment, at the segment's own offsets
    b = make()
    for po, go, so, n, t in rows:
        h, step, lr = tuples[t]
        _single(b['p'], b['g'], b['m'], b['v'], b['x'], n, h, step, lr, off=(po, go, so))
    torch.cuda.synchronize()
    out = {k: _bits(a[k]) for k in 'pmvx'}
    for k in 'pmvx':
        assert np.array_equal(out[k], _bits(b[k])), k
    assert np.array_equal(_bits(a['g']), host['g'].view(np.uint32))      # the gradient is read-only
    # (c) per tuple, the segments' elements packed into ONE contiguous range (quads straddle the old segment borders)
    for t, (h, step, lr) in enumerate(tuples):
        mine = [r for r in rows if r[4] == t]
        pack = lambda k, col: torch.from_numpy(np.concatenate([host[k][r[col]:r[col] + r[3]] for r in mine])).cuda()
        c = {'p': pack('p', 0), 'g': pack('g', 1), 'm': pack('m', 2), 'v': pack('v', 2), 'x': pack('x', 2)}
        _single(c['p'], c['g'], c['m'], c['v'], c['x'], c['p'].numel(), h, step, lr)
        torch.cuda.synchronize()
        for k, col in (('p', 0), ('m', 2), ('v', 2)) + ((('x', 2),) if ams else ()):
            got = np.concatenate([out[k][r[col]:r[col] + r[3]] for r in mine])
            assert np.array_equal(got, _bits(c[k])), (t, k)
    # the gaps: untouched, bit for bit; the segments: all finite (no poisoned gradient float reached them) and changed
    for k, col in (('p', 0), ('m', 2), ('v', 2), ('x', 2)):
        gap = np.ones(host[k].size, dtype=bool)
        for r in rows:
            gap[r[col]:r[col] + r[3]] = False
        was = host[k].view(np.uint32)
        assert gap.any() and np.array_equal(out[k][gap], was[gap]), k
        if k == 'x' and not ams:
            assert np.array_equal(out[k], was)
            continue
        assert np.isfinite(out[k].view(np.float32)[~gap]).all(), k
        assert not np.array_equal(out[k][~gap], was[~gap]), k


# ------------------------------------------------------------------------------------------------ refusals
def _sentinels(n=64):
    return [torch.full((n,), float(i + 2), device='cuda') for i in range(5)]


OKH = A.HYPERS[6]
BAD_SINGLE = [
    ('null param', dict(null=0), 'null buffer'),
    ('null grad', dict(null=1), 'null buffer'),
    ('null exp_avg', dict(null=2), 'null buffer'),
    ('null exp_avg_sq', dict(null=3), 'null buffer'),
    ('empty', dict(n=0), 'empty range'),
    ('misaligned param', dict(shift=0), 'aligned'),
    ('misaligned state', dict(shift=3), 'aligned'),
    ('amsgrad without vmax', dict(null=4), 'amsgrad'),
    ('beta1 = 1', dict(args={1: 1.0}), 'beta'),
    ('beta2 < 0', dict(args={2: -0.1}), 'beta'),
    ('beta2 NaN', dict(args={2: float('nan')}), 'beta'),
    ('eps = 0', dict(args={3: 0.0}), 'eps'),
    ('eps < 0', dict(args={3: -1e-8}), 'eps'),
    ('step_size inf', dict(args={5: float('inf')}), 'step_size'),
    ('step_size NaN', dict(args={5: float('nan')}), 'step_size'),
    ('bc2_sqrt NaN', dict(args={6: float('nan')}), 'bc2_sqrt'),
    ('bc2_sqrt inf', dict(args={6: float('inf')}), 'bc2_sqrt'),
    ('bc2_sqrt 0', dict(args={6: 0.0}), 'bc2_sqrt'),
]


@pytest.mark.parametrize('what,spec,why', BAD_SINGLE, ids=[b[0].replace(' ', '-') for b in BAD_SINGLE])
def test_single_range_refusals_launch_nothing(what, spec, why):
    from singleshotpose_amd import _lib
    bufs = _sentinels()
    keep = [t.clone() for t in bufs]
    ptrs = [t.data_ptr() for t in bufs]
    if 'null' in spec:
        ptrs[spec['null']] = None
    if 'shift' in spec:
        ptrs[spec['shift']] += 4
    args = list(_args(OKH, 3))
    for i, val in spec.get('args', {}).items():
        args[i] = val
    with pytest.raises(_lib.SspError, match=why):
        _lib.call('ssp_adam_step', *(ptrs + [spec.get('n', 32)] + args + [_stream()]))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, bufs))


BAD_ROWS = [([0, 0, 0, 1 << 20, 0], 'outside the parameter'), ([1 << 30, 0, 0, 8, 0], 'outside the parameter'),
            ([0, 1 << 30, 0, 8, 0], 'outside the gradient'), ([0, 0, 1 << 30, 8, 0], 'outside the state'),
            ([0, 0, 60, 8, 0], 'outside the state'), ([2, 0, 0, 8, 0], 'multiples of 4'), ([0, -4, 0, 8, 0], 'multiples of 4'),
            ([0, 0, 0, 0, 0], 'length'), ([0, 0, 0, 8, 2], 'tuple index'), ([0, 0, 0, 8, -1], 'tuple index')]


@pytest.mark.parametrize('bad,why', BAD_ROWS, ids=[str(b[0]).replace(' ', '') for b in BAD_ROWS])
def test_table_refuses_a_bad_row_and_launches_nothing(bad, why):
    from singleshotpose_amd import _lib
    bufs = _sentinels()
    keep = [t.clone() for t in bufs]
    rows = [[0, 0, 0, 5, 0], [8, 8, 8, 8, 1], bad, [16, 16, 16, 3, 0]]
    with pytest.raises(_lib.SspError, match=why):
        _table(*bufs, rows, [(OKH, 1, None), (OKH, 2, None)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, bufs))


def test_table_refuses_bad_tuples_and_launches_nothing():
    from singleshotpose_amd import _lib
    bufs = _sentinels()
    keep = [t.clone() for t in bufs]
    rows = [[0, 0, 0, 5, 0], [8, 8, 8, 8, 1]]
    ok = _args(OKH, 1)
    bad = lambda i, val: ok[:i] + (val,) + ok[i + 1:]
    for tuples, why in (([ok] * 17, 'between 1 and 16'), ([ok, bad(3, 0.0)], 'eps'), ([ok, bad(1, 1.0)], 'beta'),
                        ([ok, bad(0, float('inf'))], 'lr'), ([ok, bad(4, -0.1)], 'weight_decay'),
                        ([ok, bad(5, float('nan'))], 'step_size'), ([ok, bad(6, 0.0)], 'bc2_sqrt')):
        with pytest.raises(_lib.SspError, match=why):
            _table(*bufs, rows, tuples)
    with pytest.raises(_lib.SspError, match='amsgrad'):
        _table(*bufs, rows, [(OKH, 1, None), (OKH, 2, None)], ams=False)       # an amsgrad tuple, no vmax buffer
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, bufs))


# ------------------------------------------------------------------------------------------------ optimizer level
def _tiny():
    from oracle.darknet_ref import seeded_state
    from singleshotpose_amd.darknet import Darknet
    model = Darknet(os.path.join(GOLD, 'tiny-pose.cfg'))
    load_state_into(model, model.blocks, seeded_state(model.blocks, 5))
    return model


def _crit():
    from singleshotpose_amd.region_loss import RegionLoss
    crit = RegionLoss()
    crit.verbose = False
    return crit


def _backward(model, crit, g, seed, accumulate=1):
    for i in range(accumulate):
        x = torch.rand(4, 3, 96, 96, generator=g).cuda()
        crit(model(x), torch.from_numpy(make_targets(np.random.RandomState(10 * seed + i), 4, [1] * 4)), 20).backward()


def _shadow_step(params, sh_params, sh_opt):
    for p, q in zip(params, sh_params):
        q.grad = None if p.grad is None else p.grad.detach().cpu().clone()
    sh_opt.step()


STATE_KEYS = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


def _assert_shadowed(tag, named, opt, sh, osh):
    for (n, p), q in zip(named, sh):
        assert rel_err(p.detach().cpu().numpy(), q.detach().numpy()) < 1e-6, (tag, n)
        for k in STATE_KEYS:
            if k in osh.state[q]:
                assert rel_err(opt.state[p][k].cpu().numpy(), osh.state[q][k].numpy()) < 1e-6, (tag, n, k)
        assert set(opt.state[p]) == set(osh.state[q])
        s = opt.state[p]['step']
        assert s.device.type == 'cpu' and s.dtype == torch.float32 and float(s) == float(osh.state[q]['step'])


@pytest.mark.parametrize('cls,kw', [('Adam', dict(lr=1e-3, weight_decay=0.002)), ('AdamW', dict(lr=1e-3, amsgrad=True))],
                         ids=['adam-l2', 'adamw-amsgrad'])
def test_fused_adam_matches_torch_over_training_steps(cls, kw):
    """The tiny net trained 4 steps with uniform hyper-parameters: one ssp_adam_step launch per step, shadowed by torch's
    class on the CPU; a state_dict hand-over to torch's class and back in the middle; eval right after a step sees the
    new weights."""
    from singleshotpose_amd import optim
    b = _tiny().cuda().train()
    ob = getattr(optim, cls)(b.parameters(), **kw)
    sh = [torch.nn.Parameter(p.detach().cpu().clone()) for p in b.parameters()]
    osh = getattr(torch.optim, cls)(sh, **kw)
    crit = _crit()
    g = torch.Generator().manual_seed(3)
    for step in range(4):
        if step == 2:
            for grp in osh.param_groups + ob.param_groups:
                grp['lr'] = grp['lr'] * 0.1
            # hand the state to torch's class on the CPU and take it back from there: the run continues as before
            mid = getattr(torch.optim, cls)([torch.nn.Parameter(p.detach().cpu().clone()) for p in b.parameters()], **kw)
            mid.load_state_dict(ob.state_dict())
            assert all(t.device.type == 'cpu' for s in mid.state.values() for t in s.values())
            ob.load_state_dict(mid.state_dict())
        ob.zero_grad()
        _backward(b, crit, g, step)
        _shadow_step(list(b.parameters()), sh, osh)
        ob.step()
        _assert_shadowed(step, list(b.named_parameters()), ob, sh, osh)
    assert ob.fused_steps == 4 and ob.table_steps == 0
    base = ob._lay['p'].data_ptr()
    assert all(base <= p.data_ptr() < base + 4 * ob.flat_numel for p in b.parameters())
    # eval right after a fused step uses the updated filters (cached operands refreshed)
    b.eval()
    x = torch.rand(2, 3, 96, 96, generator=g).cuda()
    with torch.no_grad():
        y0 = b(x)
    ob.zero_grad()
    b.train()
    _backward(b, crit, g, 9)
    ob.step()
    b.eval()
    with torch.no_grad():
        y1 = b(x)
    fresh = _tiny().cuda().eval()
    fresh.load_state_dict(b.state_dict())
    with torch.no_grad():
        y2 = fresh(x)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, y2)


def _groups(named):
    """The parameter-group list of train.py:381-387: no weight decay on BatchNorm and bias parameters."""
    out = []
    for key, value in named:
        wd = 0.0 if (key.find('.bn') >= 0 or key.find('.bias') >= 0) else 0.002
        out.append({'params': [value], 'weight_decay': wd})
    return out


def test_grouped_adam_with_accumulated_gradients_is_one_table_launch(monkeypatch):
    """The group list of train.py:381-387 (two distinct tuples) and gradients accumulated over two backwards (autograd adds
    in place: the .grads stay views of one flat buffer): one ssp_adam_step_table launch per step."""
    from singleshotpose_amd import _lib, optim
    b = _tiny().cuda().train()
    names = [n for n, _ in b.named_parameters()]
    ob = optim.AdamW(_groups(b.named_parameters()), lr=2e-4)
    sh = [torch.nn.Parameter(p.detach().cpu().clone()) for p in b.parameters()]
    osh = torch.optim.AdamW(_groups(zip(names, sh)), lr=2e-4)
    log = []
    orig = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (log.append(name), orig(name, *a))[1])
    crit = _crit()
    g = torch.Generator().manual_seed(11)
    for step in range(3):
        ob.zero_grad()
        _backward(b, crit, g, step, accumulate=2)
        _shadow_step(list(b.parameters()), sh, osh)
        table_before = None if ob._lay is None else ob._lay['dev'].data_ptr()
        del log[:]
        ob.step()
        assert log.count('ssp_adam_step_table') == 1 and log.count('ssp_adam_step') == 0, step
        if step:
            assert ob._lay['dev'].data_ptr() == table_before      # no per-step table upload
        _assert_shadowed(step, list(b.named_parameters()), ob, sh, osh)
    assert ob.fused_steps == 0 and ob.table_steps == 3
    assert ob.flat_numel == sum((p.numel() + 3) // 4 * 4 for p in b.parameters())


def test_head_only_adam_under_a_frozen_trunk_is_one_table_launch(monkeypatch):
    """An optimizer that holds the head alone, the trunk frozen with its BatchNorm in eval(): one table launch per step,
    trunk parameters and buffers bit-identical afterwards.  In the last step one head parameter has no gradient: its step
    count falls behind, the others' tuples differ from its own from then on - still one launch."""
    from singleshotpose_amd import _lib, optim
    model = _tiny().cuda().train()
    head = list(model.models[19].parameters())
    for ind, blk in enumerate(model.blocks[1:]):
        if blk['type'] == 'convolutional' and ind < 19:
            for p in model.models[ind].parameters():
                p.requires_grad_(False)
            for mod in model.models[ind]:
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.eval()
    frozen = {n: t.detach().clone() for n, t in list(model.models.named_parameters()) + list(model.models.named_buffers())
              if not n.startswith('19.')}
    kw = dict(lr=1e-3, weight_decay=0.01, amsgrad=True)
    opt = optim.Adam(head, **kw)
    sh = [torch.nn.Parameter(p.detach().cpu().clone()) for p in head]
    osh = torch.optim.Adam(sh, **kw)
    log = []
    orig = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (log.append(name), orig(name, *a))[1])
    crit = _crit()
    g = torch.Generator().manual_seed(13)
    for step in range(4):
        opt.zero_grad()
        _backward(model, crit, g, step)
        if step == 2 and len(head) > 1:
            head[-1].grad = None
        _shadow_step(head, sh, osh)
        opt.step()
        _assert_shadowed(step, [(str(i), p) for i, p in enumerate(head)], opt, sh, osh)
    torch.cuda.synchronize()
    assert opt.table_steps == 4 and opt.fused_steps == 0
    assert log.count('ssp_adam_step_table') == 4 and log.count('ssp_adam_step') == 0
    if len(head) > 1:
        assert float(opt.state[head[-1]]['step']) == 3.0 and float(opt.state[head[0]]['step']) == 4.0
    assert 0 < opt.flat_numel <= sum((p.numel() + 3) // 4 * 4 for p in head)
    now = dict(list(model.models.named_parameters()) + list(model.models.named_buffers()))
    for n, t in frozen.items():
        assert torch.equal(now[n].detach(), t), n


def test_gradients_that_are_no_flat_views_take_per_parameter_launches():
    from singleshotpose_amd import optim
    rs = np.random.RandomState(A.SEED + 9)
    shapes = [(7,), (3, 5), (4, 2, 3, 3)]
    ps = [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(s).astype(np.float32)).cuda()) for s in shapes]
    sh = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    kw = dict(lr=1e-2, weight_decay=0.1)
    opt, osh = optim.AdamW(ps, **kw), torch.optim.AdamW(sh, **kw)
    for step in range(3):
        for p in ps:
            p.grad = torch.from_numpy(rs.standard_normal(tuple(p.shape)).astype(np.float32)).cuda()
        _shadow_step(ps, sh, osh)
        opt.step()
        _assert_shadowed(step, [(str(i), p) for i, p in enumerate(ps)], opt, sh, osh)
    assert opt.fused_steps == 0 and opt.table_steps == 0

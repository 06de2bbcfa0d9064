"""Adam / AdamW / clip_grad_norm_ without a GPU: the float64 statement of the update (adam_cases.py) pinned to
torch.optim.Adam / AdamW, the segment-table builder as a pure function, the constructor refusals, state_dict round trips
with torch's classes, and the new entry points in the header and the binding."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import adam_cases as A
from helpers import ROOT, rel_err

NEW = {'ssp_adam_step': 16, 'ssp_adam_step_table': 14, 'ssp_grad_sumsq_table': 9, 'ssp_grad_scale_table': 10}


def _torch_opt(h, params, lr=None):
    cls = torch.optim.AdamW if h.decoupled else torch.optim.Adam
    return cls(params, lr=h.lr if lr is None else lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=h.weight_decay,
               amsgrad=h.amsgrad)


# ------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize('h', A.HYPERS, ids=lambda h: h.name)
def test_statement_is_torch_adam_in_float64(h):
    """Eight steps, gradient magnitudes 1e-4 ... 1, lr rewritten after the third step.  torch runs in fp32, the
    statement in float64 from the same fp32 inputs; a step costs torch at most one rounding of the largest element
    beyond the (lr-scaled) error of the update itself, so eight steps stay within 8 * 2^-23."""
    from singleshotpose_amd.optim import _bias_corrections
    n = 4099
    p0, grads = A.inputs(n, A.SEED + 1, 8)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = _torch_opt(h, [q])
    p, m, v, vmax = p0.astype(np.float64), np.zeros(n), np.zeros(n), np.zeros(n)
    for step, g in enumerate(grads):
        lr = h.lr * (0.1 if step >= 3 else 1.0)
        for grp in opt.param_groups:
            grp['lr'] = lr
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v, vmax = A.adam_statement(p, g, m, v, vmax, h, step + 1, lr=lr)
        # the host side of the product computes the two bias-correction figures exactly as the statement does
        assert _bias_corrections(lr, h.beta1, h.beta2, float(step + 1)) == A.bias_corrections(h._replace(lr=lr), step + 1)
    st = opt.state[q]
    errs = {'p': rel_err(q.detach().numpy(), p), 'm': rel_err(st['exp_avg'].numpy(), m),
            'v': rel_err(st['exp_avg_sq'].numpy(), v)}
    if h.amsgrad:
        errs['vmax'] = rel_err(st['max_exp_avg_sq'].numpy(), vmax)
    print('e_torch after 8 steps (%s): %s' % (h.name, ', '.join('%s %.2e' % kv for kv in errs.items())))
    assert all(e < 8 * 2.0 ** -23 for e in errs.values()), errs


def test_clip_statement_is_torch_clip_grad_norm():
    import inspect
    from singleshotpose_amd.optim import clip_grad_norm_
    ours = inspect.signature(clip_grad_norm_).parameters
    theirs = inspect.signature(torch.nn.utils.clip_grad_norm_).parameters
    for name in ('parameters', 'max_norm', 'norm_type', 'error_if_nonfinite'):
        assert ours[name].default == theirs[name].default, name
    rs = np.random.RandomState(A.SEED + 2)
    segs = [rs.standard_normal(n) for n in (1, 5, 4099, 300)]      # float64 tensors: torch computes in float64 too
    for max_norm in (0.5, 10.0, 1e3):
        ps = [torch.nn.Parameter(torch.zeros(len(s), dtype=torch.float64)) for s in segs]
        for q, s in zip(ps, segs):
            q.grad = torch.from_numpy(s.copy())
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        ref_norm, coef, scaled = A.clip_statement(segs, max_norm)
        assert abs(float(norm) - ref_norm) <= 1e-14 * ref_norm
        assert (coef == 1.0) == (max_norm > ref_norm)
        for q, s in zip(ps, scaled):
            assert rel_err(q.grad.numpy(), s) < 1e-14


# ------------------------------------------------------------------------------------------------ the table builder
def _key(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=False, amsgrad=False, step=1.0):
    return (lr, b1, b2, eps, wd, decoupled, amsgrad, step)


def test_table_builder_is_a_pure_function_of_what_is_held():
    from singleshotpose_amd.optim import build_adam_segment_table as build
    a, b, c = _key(), _key(wd=0.01), _key(step=2.0)
    entries = [(5, 40, a), (8, 0, b), (1, 48, a), (4097, 8000, c), (3, 56, b)]
    rows, keys, numel = build(entries)
    # parameter and state offsets pack the held parameters in order, each rounded up to 4 floats; gradient offsets are kept
    assert rows == [[0, 40, 0, 5, 0], [8, 0, 8, 8, 1], [16, 48, 16, 1, 0], [20, 8000, 20, 4097, 2], [4120, 56, 4120, 3, 1]]
    assert numel == 4124 and all(r[0] % 4 == 0 and r[2] % 4 == 0 for r in rows)
    assert keys == [a, b, c]                                  # tuples in order of first use
    assert build(entries) == (rows, keys, numel)              # nothing remembered between calls
    # the step count is part of the key: the same hyper-parameters at another count are another tuple
    assert len(build([(4, 0, _key(step=3.0)), (4, 4, _key(step=4.0))])[1]) == 2
    assert len(build([(4, 0, _key(step=3.0)), (4, 4, _key(step=3.0))])[1]) == 1
    # so are the two flags
    assert len(build([(4, 0, _key()), (4, 4, _key(amsgrad=True)), (4, 8, _key(decoupled=True))])[1]) == 3


def test_table_builder_falls_back():
    from singleshotpose_amd.optim import build_adam_segment_table as build
    assert build([]) is None
    assert build([(4, None, _key())]) is None                 # a gradient that is no flat view
    assert build([(4, 2, _key())]) is None                    # ... or a misaligned one
    assert build([(0, 0, _key())]) is None
    many = [(4, 4 * i, _key(lr=1e-3 * (i + 1))) for i in range(17)]
    assert build(many) is None                                # more than 16 distinct tuples: per-parameter launches
    assert len(build(many[:16])[1]) == 16
    assert len(build(many, max_tuples=17)[1]) == 17
    # 17 parameters at 17 different step counts are 17 tuples as well
    assert build([(4, 4 * i, _key(step=float(i + 1))) for i in range(17)]) is None


def test_sgd_table_builder_is_what_it_was():
    from singleshotpose_amd.optim import MAX_TUPLES, build_segment_table
    rows, tuples, numel = build_segment_table([(5, 8, (0.1, 0.9, 0.0, 0.01, False), False), (3, 0, (0.1, 0.0, 0.0, 0.0, False), False)])
    assert MAX_TUPLES == 16 and rows == [[0, 8, 0, 5, 0], [8, 0, 8, 3, 1]] and numel == 12
    assert tuples == [(0.1, 0.9, 0.0, 0.01, 0.0, 1.0), (0.1, 0.0, 0.0, 0.0, 0.0, 0.0)]
    from singleshotpose_amd import optim
    assert hasattr(optim, 'Adam')


# ------------------------------------------------------------------------------------------------ the constructors
@pytest.mark.parametrize('cls', ['Adam', 'AdamW'])
def test_constructor_defaults_and_refusals(cls):
    from singleshotpose_amd import optim
    C = getattr(optim, cls)
    mk = lambda **kw: C([torch.nn.Parameter(torch.zeros(4))], **kw)
    g = mk().param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['amsgrad']) == (1e-3, (0.9, 0.999), 1e-8, False)
    assert g['weight_decay'] == (1e-2 if cls == 'AdamW' else 0) and g['decoupled_weight_decay'] == (cls == 'AdamW')
    for name, value in (('maximize', True), ('capturable', True), ('differentiable', True), ('foreach', True), ('fused', True)):
        with pytest.raises(ValueError, match=name):
            mk(**{name: value})
    with pytest.raises(ValueError, match='tensor lr'):
        mk(lr=torch.tensor(1e-3))
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError, match='Invalid'):
            mk(**kw)
    o = mk(foreach=False, fused=None, amsgrad=True)
    assert o.fused_steps == 0 and o.table_steps == 0 and o.flat_numel == 0
    o.param_groups[0]['params'][0].grad = torch.ones(4)
    with pytest.raises(RuntimeError, match='HIP kernel only'):
        o.step()


def test_clip_grad_norm_refusals():
    from singleshotpose_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    for bad in (1, 1.0, float('inf'), 3):
        with pytest.raises(ValueError, match='norm_type'):
            clip_grad_norm_([p], 1.0, norm_type=bad)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        clip_grad_norm_([p], 1.0)
    assert torch.equal(p.grad, torch.ones(4))


# ------------------------------------------------------------------------------------------------ state_dict round trips
@pytest.mark.parametrize('h', [A.HYPERS[0], A.HYPERS[6], A.HYPERS[3]], ids=lambda h: h.name)
def test_state_dict_moves_between_torch_and_these_classes(h):
    """torch -> ours -> torch on CPU state: the second torch optimizer continues bit for bit like the first."""
    from singleshotpose_amd import optim
    shapes = [(7,), (3, 5), (4, 2, 3, 3)]
    rs = np.random.RandomState(A.SEED + 3)
    start = [rs.standard_normal(s).astype(np.float32) for s in shapes]
    grads = [[rs.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(4)]
    mk = lambda: [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in start]

    def run(opt, ps, gs):
        for step in gs:
            for q, g in zip(ps, step):
                q.grad = torch.from_numpy(g.copy())
            opt.step()
    pa = mk()
    oa = _torch_opt(h, [{'params': pa[:2]}, {'params': pa[2:], 'lr': 5e-4}])
    run(oa, pa, grads[:2])
    ours_params = mk()
    ours = (optim.AdamW if h.decoupled else optim.Adam)([{'params': ours_params[:2]}, {'params': ours_params[2:]}])
    ours.load_state_dict(copy.deepcopy(oa.state_dict()))      # (torch's load keeps same-device tensors: no aliasing here)
    assert [g['lr'] for g in ours.param_groups] == [h.lr, 5e-4] and ours.param_groups[0]['amsgrad'] == h.amsgrad
    keys = {'step', 'exp_avg', 'exp_avg_sq'} | ({'max_exp_avg_sq'} if h.amsgrad else set())
    for q, r in zip(pa, ours_params):
        st = ours.state[r]
        assert set(st) == keys
        assert st['step'].device.type == 'cpu' and st['step'].dtype == torch.float32 and st['step'].dim() == 0
        assert float(st['step']) == 2.0
        assert all(torch.equal(st[k], oa.state[q][k]) for k in keys)
    pb = mk()
    for q, r in zip(pa, pb):
        r.data.copy_(q.data)
    ob = _torch_opt(h._replace(lr=123.0, eps=0.5), [{'params': pb[:2]}, {'params': pb[2:]}])      # (overwritten by the load)
    ob.load_state_dict(copy.deepcopy(ours.state_dict()))
    run(oa, pa, grads[2:])
    run(ob, pb, grads[2:])
    for q, r in zip(pa, pb):
        assert torch.equal(q.detach(), r.detach())
        assert all(torch.equal(oa.state[q][k], ob.state[r][k]) for k in keys)


def test_a_loaded_group_that_asks_for_an_unsupported_mode_is_refused():
    from singleshotpose_amd import optim
    q = torch.nn.Parameter(torch.zeros(4))
    ot = torch.optim.Adam([q], maximize=True)
    ours = optim.Adam([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match='maximize'):
        ours.load_state_dict(ot.state_dict())


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_and_exports_with_matching_argument_counts():
    from singleshotpose_amd import _lib as lib
    with open(os.path.join(ROOT, 'include', 'ssp_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, name + ' is not declared in include/ssp_hip.h'
        assert len(m.group(1).split(',')) == nargs, name
        assert name in lib.exported_symbols() and len(lib._SIGS[name]) == nargs, name
        assert hasattr(lib.load(), name), name + ' is not exported by the library'
    assert 'SSP_ADAM_MAX_TUPLES 16' in header
    assert lib.query('ssp_abi_version') == 5
    with open(os.path.join(ROOT, 'singleshotpose_amd', 'csrc', 'Makefile')) as f:
        assert ' adam.hip ' in f.read()

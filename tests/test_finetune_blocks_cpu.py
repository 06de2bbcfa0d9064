"""Fine-tuning on stride-2, depthwise and upsample blocks, without a GPU: the data of tests/finetune_block_cases.py is what it
claims to be (decision margins under each pattern's own BatchNorm modes, the exact twins' 2^24 budget, the reference tied to
the references the suite already trusts), and Plan.backward_schedule - on plans built on the CPU device, where scheduling
launches nothing - agrees with the rules restated from the cfg on every net, over every prefix in both modes and over the
table's own patterns."""
import pytest
import torch

import depthwise_cases as D
import finetune_block_cases as C
import topology_cases as T
import upsample_cases as U
from test_finetune_cpu import _no_launch, _own, _patterns

ids = lambda cases: [c.id for c in cases]


# ---------------------------------------------------------------------------------------------------- the data
def test_the_table_is_the_one_the_tests_run():
    want = {'ft_mix': 9, 'ft_s2_odd': 6, 'ft_dw_pool': 5, 'ft_two_branch': 4, 'ftx_mix': 7, 'ftx_two_branch': 4}
    assert {k: len(v) for k, v in C.TABLE.items()} == want
    assert sorted(C.SEEDS) == sorted((c.id, p.id) for c, p in C.FLOAT_PATTERNS)
    for c, p in C.FLOAT_PATTERNS + C.EXACT_PATTERNS:
        assert sorted(p.own) == sorted(p.bn_train) == C.PLANS[c.id]['convs'] == sorted(C.conv_layers(c))
    # what the pattern names mean, on one net
    mix = {p.id: p for p in C.TABLE['ft_mix']}
    p = mix['prefix-eval-3']
    assert [i for i in p.own if any(p.own[i])] == [3, 4, 5, 8, 9] and [i for i in p.bn_train if p.bn_train[i]] == [3, 4, 5, 8]
    p = mix['bn-eval-5+input']
    assert all(any(o) for o in p.own.values()) and [i for i in p.bn_train if p.bn_train[i]] == [5, 8] and p.want_input
    p = mix['sandwich-4']
    assert [i for i in p.own if not any(p.own[i])] == [4] and [i for i in (0, 1, 2, 3, 4, 5, 8) if not p.bn_train[i]] == [4]
    p = mix['bn-only']
    assert all(o == (False, False, True, True) for i, o in p.own.items() if i != 9) and p.own[9] == (False, False, False, False)
    assert all(p.bn_train[i] for i in (0, 1, 2, 3, 4, 5, 8))
    p = C.pattern(C.FT_TWO_BRANCH, 'branch-1-7-8')
    assert [i for i in p.own if any(p.own[i])] == [1, 7, 8] and [i for i in p.bn_train if p.bn_train[i]] == [1, 7]


@pytest.mark.parametrize('cp', C.FLOAT_PATTERNS, ids=C.pid)
def test_seed_keeps_the_decision_margins_under_its_pattern(cp):
    case, pat = cp
    seed = C.SEEDS[case.id, pat.id]
    m, d = C.margins(case, pat.bn_train, seed)
    print('FT %s %s seed %d: margin %.3e, float32 forward difference %.3e' % (case.id, pat.id, seed, m, d))
    assert m >= 4.0 * d
    assert seed == C.find_seed(case, pat.bn_train)          # the first such seed in 0..7


@pytest.mark.parametrize('case', C.EXACT, ids=ids(C.EXACT))
def test_exact_twins_fit_fp32_and_are_not_trivial(case):
    budget = C.exact_budget(case, C.XSEED)
    r64, r32 = C.reference(case, C.TABLE[case.id][0])
    nz = lambda t: float((t != 0).double().mean())
    print('FT %s budget %.3g (2^24 = %.3g), non-zero: y %.2f dx %.2f gradients >= %.2f' % (
        case.id, budget, 2.0 ** 24, nz(r64.y), nz(r64.dx), min(nz(g) for g in r64.grads.values())))
    assert budget < 2 ** 24
    assert nz(r64.y) >= 1 / 3 and nz(r64.dx) >= 0.1
    assert all(nz(g) > 0 for g in r64.grads.values())
    # integers below the budget: the float32 reference IS the float64 one
    assert torch.equal(r32.y.double(), r64.y) and torch.equal(r32.dx.double(), r64.dx)
    assert all(torch.equal(r32.grads[n].double(), r64.grads[n]) for n in r64.grads)
    assert not any(int(b.get('batch_normalize', 0)) for b in T.blocks_of(case)[1:])


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert tuple(a.shape) == tuple(b.shape) and err <= 1e-12 * max(1.0, float(b.abs().max())), (what, err)


@pytest.mark.parametrize('mod,case', [(D, D.DW_SEP), (U, U.UP_NET)], ids=['dw_sep', 'up_net'])
def test_reference_equals_the_trusted_ones_with_every_mode_in_training(mod, case):
    seed = mod.seed_of(case)
    want = mod.reference(case, seed)[0]
    model = mod.make_model(case)
    x = mod.make_input(case, seed)
    got = C.run_ref(model, x, mod.make_probe(case, seed, want.y_train.shape), torch.float64, True)
    _close(got.y, want.y_train, 'y')
    _close(got.dx, want.dx, 'dx')
    assert sorted(got.grads) == sorted(want.grads) and sorted(got.stats) == sorted(want.stats)
    for n in want.grads:
        _close(got.grads[n], want.grads[n], n)
    for n in want.stats:
        _close(got.stats[n], want.stats[n], n)
    # ... and with every mode in eval it is their eval forward, which leaves the statistics alone
    ev = C.run_ref(model, x, None, torch.float64, False)
    _close(ev.y, want.y_eval, 'y_eval')
    assert all(torch.equal(ev.stats['models.' + n], b.double()) for n, b in model.models.named_buffers() if 'running' in n)


# ---------------------------------------------------------------------------------------------------- the schedule
def _plan(case, monkeypatch):
    from singleshotpose_amd import engine
    monkeypatch.delenv('SSP_BN_FUSE', raising=False)
    monkeypatch.delenv('SSP_UPSAMPLE_FUSE', raising=False)
    _no_launch(monkeypatch)
    model = T.make_model(case, init=False)
    plan = engine.Plan(model, case.B, case.H, case.W, torch.device('cpu'))
    plan._plan_bn_fusion()
    return plan


def _compare(plan, case, pat, ids_):
    """plan.backward_schedule under the pattern against C.expected, op by op; returns the number of ops compared."""
    sched = plan.backward_schedule(ids_, pat.want_input, pat.bn_train)
    exp = C.expected(case, pat)
    assert len(sched) == len(plan.ops) and [s.ind for s in sched] == [op.ind for op in plan.ops]
    last = plan.last
    n = 0
    for op, s in zip(plan.ops, sched):
        e = exp[op.ind]
        where = (case.id, pat.id, op.ind, op.kind)
        if op.kind == 'alias':
            # a one-layer route passes its source's map on: the gradient goes straight to the source's producer
            assert s.visited == (e['visited'] and op.ind == last), where
            continue
        assert s.visited == e['visited'], where
        assert s.dgrad == e['dgrad'], where
        if op.kind == 'conv':
            got = dict(wgrad=s.wgrad, bias=s.bias, dgamma=s.dgamma, dbeta=s.dbeta, bn_reduce=s.bn_reduce, fold_bn=s.fold_bn)
            assert got == {k: e[k] for k in got}, where
            if op.pool:
                assert exp[op.ind + 1]['visited'] == e['visited'], where
        else:
            assert not (s.wgrad or s.bias or s.dgamma or s.dbeta or s.bn_reduce or s.fold_bn), where
        if not s.visited:
            assert not any(s.dgrad) and not (s.wgrad or s.bias or s.dgamma or s.dbeta or s.bn_reduce or s.fold_bn), where
        n += 1
    return n


@pytest.mark.parametrize('case', C.NETS, ids=ids(C.NETS))
def test_plan_records(case, monkeypatch):
    plan = _plan(case, monkeypatch)
    want = C.PLANS[case.id]
    assert sorted(plan.convs) == want['convs']
    assert plan.depthwise == want['depthwise'] and plan.upsample == want['upsample'] and plan.fused_pool == want['fused_pool']
    assert {i: cs.bn_fuse_src.ind for i, cs in plan.convs.items() if cs.bn_fuse_src is not None} == want['bn_pairs']
    # the block families the nets are there for
    strided = [i for i, cs in plan.convs.items() if cs.stride == 2 and not cs.depthwise]
    assert strided == {'ft_mix': [1], 'ftx_mix': [1], 'ft_s2_odd': [1, 3, 5]}.get(case.id, [])
    if case.id == 'ft_s2_odd':
        assert [(cs.H, cs.W) for cs in plan.convs.values()] == [(26, 22), (13, 11), (13, 11), (7, 6), (7, 6), (4, 3), (4, 3)]
        assert (plan.convs[5].cin, plan.convs[5].cinp) == (18, 20)
    concat = [op for op in plan.ops if op.kind == 'concat']
    assert [op.inplace for op in concat] == [True] * len(want['upsample'])


@pytest.mark.parametrize('case', C.NETS, ids=ids(C.NETS))
def test_schedule_follows_the_rules_on_every_prefix_in_both_modes(case, monkeypatch):
    plan = _plan(case, monkeypatch)
    n = 0
    for name, pick, want_input in _patterns(plan):
        own, ids_ = _own(plan, pick)
        for mode in (True, False):
            bn_train = {i: bool(cs.bn) and mode for i, cs in plan.convs.items()}
            n += _compare(plan, case, C.Pattern('%s/%s' % (name, mode), own, bn_train, want_input), ids_)
    assert n > 100


@pytest.mark.parametrize('cp', C.FLOAT_PATTERNS + C.EXACT_PATTERNS, ids=C.pid)
def test_schedule_follows_the_rules_on_the_table(cp, monkeypatch):
    case, pat = cp
    plan = _plan(case, monkeypatch)
    own, ids_ = _own(plan, lambda i, kind: pat.own[i][C.KINDS.index(kind)])
    assert own == pat.own                               # the pattern asks only about parameters that exist
    assert {i: bool(cs.bn) for i, cs in plan.convs.items()} == C.conv_layers(case)
    assert _compare(plan, case, pat, ids_) >= len(plan.convs)
    # the module tree in the pattern's state gives the same schedule when the plan reads the modules itself
    model = C.apply_pattern(plan.net, pat)
    ids_m = [id(p) for p in model.models.parameters() if p.requires_grad]
    assert sorted(ids_m) == sorted(ids_)
    assert plan.backward_schedule(ids_m, pat.want_input) == plan.backward_schedule(ids_, pat.want_input, pat.bn_train)


def test_the_concat_is_one_sided_in_either_direction():
    """ft_two_branch: layer 1, the route's second source, is no ancestor of the upsample (5 <- 4 <- pool 3 <- route 2 <- 0)."""
    case = C.FT_TWO_BRANCH
    e = C.expected(case, C.pattern(case, 'branch-1-7-8'))
    assert e[6]['visited'] and e[6]['dgrad'] == (False, True) and not e[5]['visited'] and not e[4]['visited'] and e[1]['visited']
    e = C.expected(case, C.pattern(case, 'branch-4-7-8'))
    assert e[6]['visited'] and e[6]['dgrad'] == (True, False) and e[5]['visited'] and e[4]['visited'] and not e[1]['visited']
    assert not e[0]['visited'] and e[4]['dgrad'] == (False,)
    for name in ('branch-1-7-8', 'branch-4-7-8'):
        e = C.expected(C.FTX_TWO_BRANCH, C.pattern(C.FTX_TWO_BRANCH, name))
        assert sorted(e[6]['dgrad']) == [False, True]


def test_restated_launch_counts_of_the_frozen_prefixes():
    """What the GPU test's launch logs are held to, spelled out for the four cases the frozen forward is there for."""
    n = C.expected_launches(C.FT_MIX, C.pattern(C.FT_MIX, 'prefix-eval-3'))
    assert (n['ssp_conv_s2_fwd_affine'], n['ssp_dwconv_fwd_affine'], n['ssp_dwconv_fwd'], n['ssp_conv_s2_fwd']) == (1, 1, 1, 0)
    assert (n['ssp_dwconv_wgrad'], n['ssp_dwconv_dgrad'], n['ssp_conv_s2_wgrad'], n['ssp_conv_s2_dgrad']) == (1, 1, 0, 0)
    assert n['ssp_upsample_bwd'] == 1 and n['ssp_bn_fwd_finalize'] == 4 and n['ssp_bn_act_bwd_affine'] == 0
    n = C.expected_launches(C.FT_MIX, C.pattern(C.FT_MIX, 'prefix-eval-5'))
    assert (n['ssp_conv_s2_fwd_affine'], n['ssp_dwconv_fwd_affine'], n['ssp_dwconv_fwd']) == (1, 2, 0)
    assert (n['ssp_dwconv_wgrad'], n['ssp_dwconv_dgrad'], n['ssp_upsample_bwd'], n['ssp_bn_fwd_finalize']) == (0, 0, 1, 2)
    n = C.expected_launches(C.FT_DW_POOL, C.pattern(C.FT_DW_POOL, 'prefix-eval-5'))
    assert (n['ssp_dwconv_fwd_affine'], n['ssp_conv_fwd_affine'], n['ssp_dwconv_fwd'], n['ssp_bn_fwd_finalize']) == (0, 1, 2, 1)
    n = C.expected_launches(C.FT_TWO_BRANCH, C.pattern(C.FT_TWO_BRANCH, 'branch-1-7-8'))
    assert n['ssp_upsample_bwd'] == 0 and n['ssp_bn_fwd_finalize'] == 2 and n['ssp_conv_fwd_affine'] == 2
    # an eval-mode block that IS visited runs the affine backward only with gamma and beta frozen
    n = C.expected_launches(C.FT_MIX, C.pattern(C.FT_MIX, 'sandwich-4'))
    assert (n['ssp_bn_act_bwd_affine'], n['ssp_bn_act_bwd(+_partials)'], n['ssp_dwconv_wgrad'], n['ssp_dwconv_dgrad']) == (1, 6, 1, 2)
    n = C.expected_launches(C.FT_MIX, C.pattern(C.FT_MIX, 'bn-eval-5+input'))
    assert (n['ssp_bn_act_bwd_affine'], n['ssp_bn_act_bwd(+_partials)'], n['ssp_bn_fwd_finalize']) == (0, 7, 2)

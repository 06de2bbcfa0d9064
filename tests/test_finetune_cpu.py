"""Fine-tuning with frozen layers, without a GPU: Plan.backward_schedule against an independent restatement of its rules
(written here from topology_cases.layer_info / consumers_of, on plans built on the CPU device - scheduling launches
nothing), the segment-table builder of optim.SGD (a pure function), and ssp_sgd_step_table's refusal of a table that
points outside its buffers (the check runs before any launch, so it needs no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import topology_cases as T
from helpers import GOLD

CFGS = {'tiny-pose': (os.path.join(GOLD, 'tiny-pose.cfg'), 2, 96, 96),
        'generic-pose': (os.path.join(GOLD, 'generic-pose.cfg'), 2, 80, 80)}
_WANTED = ('route2', 'route1_rel', 'route1_abs', 'shortcut', 'dead_branch')
TOPO = [c for c in T.FLOAT if set(_WANTED) & T.features(T.blocks_of(c), c.B, c.H, c.W)][:24]


def test_the_topology_selection_has_routes_shortcuts_and_a_dead_branch():
    feats = [T.features(T.blocks_of(c), c.B, c.H, c.W) for c in TOPO]
    assert len(TOPO) >= 12
    for f in ('route2', 'shortcut', 'dead_branch'):
        assert sum(f in fs for fs in feats) >= 2, f
    assert any('route1_rel' in fs or 'route1_abs' in fs for fs in feats)


# ---------------------------------------------------------------------------------------------------- the rules, restated
def _expected(blocks, B, H, W, own, want_input, bn_train, fuse=None):
    """Per layer of the cfg: visited, data gradient per source, and for conv blocks (wgrad, bias, dgamma, dbeta, bn_reduce,
    fold_bn).  own: {conv layer: (weight, bias, gamma, beta) trainable}; bn_train: {conv layer: BatchNorm in training mode};
    fuse: the {consumer: source} BatchNorm pairs, for cfgs with blocks T.expected_bn_fuse does not know (groups=)."""
    info = T.layer_info(blocks, H, W)
    live = T.live_layers(info)
    rel = {-1: bool(want_input)}
    for i, l in enumerate(info):
        rel[i] = any(own.get(i, ())) or any(rel[s] for s in l.srcs)
    if fuse is None:
        fuse = T.expected_bn_fuse(blocks, B, H, W)
    out = {}
    for i, l in enumerate(info):
        visited = i in live and rel[i]
        rec = dict(visited=visited, dgrad=tuple(visited and rel[s] for s in l.srcs))
        if l.type in ('convolutional', 'connected'):
            w, b, g, be = own[i]
            reduce_ = lambda j: T._is_bn(info[j]) and (bn_train[j] or own[j][2] or own[j][3])
            rec.update(wgrad=visited and w, bias=visited and b, dgamma=visited and g, dbeta=visited and be,
                       bn_reduce=bool(visited and reduce_(i)),
                       fold_bn=bool(visited and rec['dgrad'][0] and i in fuse and reduce_(fuse[i])))
        out[i] = rec
    return out


def _own(plan, pick):
    """{conv layer: (weight, bias, gamma, beta) trainable} and the matching id set, from pick(layer, kind) -> bool."""
    own, ids = {}, set()
    for ind, cs in plan.convs.items():
        ps = (('weight', cs.conv.weight), ('bias', cs.conv.bias), ('gamma', cs.bnm.weight if cs.bn else None),
              ('beta', cs.bnm.bias if cs.bn else None))
        own[ind] = tuple(p is not None and bool(pick(ind, k)) for k, p in ps)
        ids |= set(id(p) for (k, p), o in zip(ps, own[ind]) if o)
    return own, ids


def _patterns(plan):
    convs = sorted(plan.convs)
    pats = [('all', lambda i, k: True, False), ('all+input', lambda i, k: True, True),
            ('none+input', lambda i, k: False, True),
            ('bn_only', lambda i, k: k in ('gamma', 'beta'), False), ('bias_only', lambda i, k: k == 'bias', False),
            ('middle', lambda i, k, m=convs[len(convs) // 2]: i == m, False)]
    for k_ in convs:
        pats.append(('prefix%d' % k_, lambda i, k, k_=k_: i >= k_, False))
    return pats


def _check(plan, blocks, B, H, W):
    info = T.layer_info(blocks, H, W)
    live = T.live_layers(info)
    last = max(i for i, l in enumerate(info) if l.type not in ('region', 'cost'))
    n = 0
    for name, pick, want_input in _patterns(plan):
        own, ids = _own(plan, pick)
        for mode in (True, False):
            bn_train = {i: bool(cs.bn) and mode for i, cs in plan.convs.items()}
            sched = plan.backward_schedule(ids, want_input, bn_train)
            exp = _expected(blocks, B, H, W, own, want_input, bn_train)
            assert len(sched) == len(plan.ops) and [s.ind for s in sched] == [op.ind for op in plan.ops]
            for op, s in zip(plan.ops, sched):
                e = exp[op.ind]
                where = (name, mode, op.ind, op.kind)
                if op.kind == 'alias':
                    # a one-layer route passes its source's map on: the gradient goes straight to the source's producer,
                    # the route itself runs only as the network's last layer
                    assert s.visited == (e['visited'] and op.ind == last), where
                    continue
                assert s.visited == e['visited'], where
                assert s.dgrad == e['dgrad'], where
                if op.kind == 'conv':
                    got = dict(wgrad=s.wgrad, bias=s.bias, dgamma=s.dgamma, dbeta=s.dbeta, bn_reduce=s.bn_reduce,
                               fold_bn=s.fold_bn)
                    assert got == {k: e[k] for k in got}, where
                    if op.pool:
                        assert exp[op.ind + 1]['visited'] == e['visited']
                else:
                    assert not (s.wgrad or s.bias or s.dgamma or s.dbeta or s.bn_reduce or s.fold_bn), where
                if not s.visited:
                    assert not any(s.dgrad) and not (s.wgrad or s.bias or s.dgamma or s.dbeta or s.bn_reduce or s.fold_bn)
                n += 1
            if name in ('all', 'all+input'):
                # nothing frozen: every block that reaches the output runs everything it has - today's backward
                for op, s in zip(plan.ops, sched):
                    if op.kind == 'alias':
                        continue
                    assert s.visited == (op.ind in live), (name, op.ind)
                    if s.visited and op.kind == 'conv':
                        assert s.wgrad and s.bias == (op.conv.bias is not None) and s.dgamma == s.dbeta == bool(op.bn)
                        assert s.bn_reduce == bool(op.bn) and s.fold_bn == (op.bn_fuse_src is not None)
                        assert s.dgrad == ((want_input,) if op.first else (True,))
    return n


def _no_launch(monkeypatch):
    from singleshotpose_amd import _lib

    def call(name, *args):
        raise AssertionError("scheduling launched %s" % name)
    monkeypatch.setattr(_lib, 'call', call)


@pytest.mark.parametrize('name', sorted(CFGS))
def test_schedule_follows_the_rules_on_the_shipped_cfgs(name, monkeypatch):
    from singleshotpose_amd import engine
    from singleshotpose_amd.cfg import parse_cfg
    from singleshotpose_amd.darknet import Darknet
    monkeypatch.delenv('SSP_BN_FUSE', raising=False)
    _no_launch(monkeypatch)
    cfg, B, H, W = CFGS[name]
    model = Darknet(cfg)
    plan = engine.Plan(model, B, H, W, torch.device('cpu'))
    plan._plan_bn_fusion()
    assert _check(plan, parse_cfg(cfg), B, H, W) > 100


@pytest.mark.parametrize('case', TOPO, ids=[c.id for c in TOPO])
def test_schedule_follows_the_rules_on_topologies(case, monkeypatch):
    from singleshotpose_amd import engine
    monkeypatch.delenv('SSP_BN_FUSE', raising=False)
    _no_launch(monkeypatch)
    model = T.make_model(case, init=False)
    plan = engine.Plan(model, case.B, case.H, case.W, torch.device('cpu'))
    plan._plan_bn_fusion()
    assert _check(plan, T.blocks_of(case), case.B, case.H, case.W) > 0


def test_schedule_reads_each_modules_own_mode_and_head_only_is_one_block(monkeypatch):
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    _no_launch(monkeypatch)
    cfg, B, H, W = CFGS['tiny-pose']
    model = Darknet(cfg).train()
    plan = engine.Plan(model, B, H, W, torch.device('cpu'))
    plan._plan_bn_fusion()
    convs = sorted(plan.convs)
    head = plan.convs[convs[-1]]
    sched = plan.backward_schedule([id(head.conv.weight), id(head.conv.bias)], False)
    on = [s for s in sched if s.visited]
    assert [s.ind for s in on] == [head.ind] and on[0].wgrad and on[0].bias and on[0].dgrad == (False,)
    # bn_training=None reads the modules: a frozen BatchNorm in eval() needs no reductions, one in train() does
    k = convs[len(convs) // 2]
    ids = [id(p) for i in convs if i >= k for p in plan.convs[i].conv.parameters()]      # conv parameters only
    for cs in plan.convs.values():
        if cs.bn:
            cs.bnm.train(cs.ind % 2 == 0)
    for s in plan.backward_schedule(ids, False):
        if s.kind == 'conv' and s.visited and plan.convs[s.ind].bn:
            assert s.bn_reduce == (s.ind % 2 == 0)


# ---------------------------------------------------------------------------------------------------- the table builder
PLAIN = (0.1, 0.0, 0.0, 0.0, False)
MOM = (0.1, 0.9, 0.1, 0.0, False)
NEST = (0.05, 0.9, 0.0, 0.01, True)


def test_table_builder_deduplicates_tuples_and_packs_segments():
    from singleshotpose_amd.optim import build_segment_table
    entries = [(5, 100, MOM, False), (8, 8, PLAIN, False), (1, 0, MOM, False), (1023, 2000, NEST, True), (3, 4, PLAIN, True)]
    rows, tuples, numel = build_segment_table(entries)
    assert [r[3] for r in rows] == [5, 8, 1, 1023, 3] and [r[1] for r in rows] == [100, 8, 0, 2000, 4]
    assert [r[0] for r in rows] == [0, 8, 16, 20, 1044] and all(r[0] == r[2] and r[0] % 4 == 0 for r in rows)
    assert numel == 1048
    assert [r[4] for r in rows] == [0, 1, 0, 2, 1] and len(tuples) == 3
    assert tuples[0] == (0.1, 0.9, 0.1, 0.0, 0.0, 1.0)        # momentum, no state yet: a first step
    assert tuples[1] == (0.1, 0.0, 0.0, 0.0, 0.0, 0.0)        # no momentum: never a first step, state ignored
    assert tuples[2] == (0.05, 0.9, 0.0, 0.01, 1.0, 0.0)      # momentum state present
    # 66 groups, two distinct tuples (the train.py:381-387 list): two tuples
    many = [(7 + i, 16 * i, MOM if i % 3 else NEST, True) for i in range(66)]
    rows, tuples, _ = build_segment_table(many)
    assert len(rows) == 66 and len(tuples) == 2
    # a changed lr changes the tuples only
    rows2, tuples2, _ = build_segment_table([(n, g, (h[0] * 0.5,) + h[1:], s) for n, g, h, s in many])
    assert rows2 == rows and tuples2 != tuples


def test_table_builder_fallback_conditions():
    from singleshotpose_amd.optim import MAX_TUPLES, build_segment_table
    ok = [(4, 4 * i, (0.1 * (i + 1), 0.0, 0.0, 0.0, False), False) for i in range(MAX_TUPLES)]
    assert build_segment_table(ok) is not None and len(build_segment_table(ok)[1]) == MAX_TUPLES
    assert build_segment_table(ok + [(4, 400, (9.0, 0.0, 0.0, 0.0, False), False)]) is None      # 17 tuples
    assert build_segment_table([(4, 0, MOM, True), (4, 4, MOM, False)]) is None                  # mixed momentum state
    assert build_segment_table([(4, 0, PLAIN, True), (4, 4, PLAIN, False)]) is not None          # (irrelevant without momentum)
    assert build_segment_table([(4, 0, MOM, True), (4, None, MOM, True)]) is None                # a non-flat gradient
    assert build_segment_table([(4, 0, MOM, True), (4, 6, MOM, True)]) is None                   # ... or a misaligned one
    assert build_segment_table([]) is None


def test_subset_table_names_only_its_own_segments():
    from singleshotpose_amd.optim import build_segment_table
    # a head of 20 x 64 filters + 20 biases somewhere inside a 50 M float gradient layout
    rows, tuples, numel = build_segment_table([(1280, 40000000, MOM, False), (20, 40001280, MOM, False)])
    assert numel == 1300 and len(rows) == 2 and len(tuples) == 1
    assert max(r[0] + r[3] for r in rows) <= numel and [r[1] for r in rows] == [40000000, 40001280]


# ---------------------------------------------------------------------------------------------------- the entry point's check
def _table_call(rows, tuples, p_floats, g_floats, m_floats, with_m=True):
    """ssp_sgd_step_table on HOST arrays: only for tables the entry point must refuse before it launches anything."""
    from singleshotpose_amd import _lib
    bufs = [np.zeros(max(n, 4) + 8, dtype=np.float32) for n in (p_floats, g_floats, m_floats)]
    ptr = [(b.ctypes.data + 15) // 16 * 16 for b in bufs]
    keep = [b.copy() for b in bufs]
    host = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 5))
    hyper = (ctypes.c_float * (6 * len(tuples)))(*[v for t in tuples for v in t])
    try:
        _lib.call('ssp_sgd_step_table', ptr[0], ptr[1], ptr[2] if with_m else None, p_floats, g_floats, m_floats,
                  host.ctypes.data, host.ctypes.data, len(host), ctypes.cast(hyper, ctypes.c_void_p), len(tuples), None)
    finally:
        assert all(np.array_equal(a, b) for a, b in zip(bufs, keep))


@pytest.mark.parametrize('rows,why', [
    ([[0, 0, 0, 65, 0]], 'parameter buffer'),
    ([[0, 64, 0, 8, 0]], 'gradient buffer'),
    ([[0, 0, 60, 8, 0]], 'momentum buffer'),
    ([[0, 0, 0, 8, 0], [8, 8, 8, 2 ** 40, 0]], 'parameter buffer'),
    ([[0, 0, 0, 8, 0], [8, 8, 8, 2 ** 62, 0]], 'length'),
    ([[2, 0, 0, 8, 0]], 'multiples of 4'),
    ([[0, 6, 0, 8, 0]], 'multiples of 4'),
    ([[0, 0, -4, 8, 0]], 'multiples of 4'),
    ([[0, 0, 0, 0, 0]], 'length'),
    ([[0, 0, 0, 8, 1]], 'tuple index'),
    ([[0, 0, 0, 8, -1]], 'tuple index')])
def test_entry_point_refuses_a_bad_table_before_launching(rows, why):
    from singleshotpose_amd import _lib
    with pytest.raises(_lib.SspError, match=why):
        _table_call(rows, [(0.1, 0.9, 0.0, 0.0, 0.0, 0.0)], 64, 64, 64)


def test_entry_point_refuses_bad_tuples():
    from singleshotpose_amd import _lib
    good = [[0, 0, 0, 8, 0]]
    with pytest.raises(_lib.SspError, match='tuples'):
        _table_call(good, [(0.1, 0.0, 0.0, 0.0, 0.0, 0.0)] * 17, 64, 64, 64)
    with pytest.raises(_lib.SspError, match='nesterov'):
        _table_call(good, [(0.1, 0.9, 0.5, 0.0, 1.0, 0.0)], 64, 64, 64)
    with pytest.raises(_lib.SspError, match='momentum buffer'):
        _table_call(good, [(0.1, 0.9, 0.0, 0.0, 0.0, 0.0)], 64, 64, 0, with_m=False)

"""Conditions on the operation sequences of tests/sequence_cases.py, checked on the float64 reference alone (no GPU): they keep
tests/test_gpu_sequences.py from passing vacuously.  A mutation whose effect on its first observer is below every tolerance of
the GPU test would let a stale operand through; a reference that blows up would make every bar meaningless; a vocabulary that
the sequences do not cover pins nothing."""
import collections

import pytest
import torch

import sequence_cases as S
import topology_cases as T
from helpers import rel_err

NET = S.TINY_NET
VISIBLE = 1e-2       # 100 x the project's forward bar of 1e-4
ids = lambda seqs: [s.id for s in seqs]


def _runs(seq, net=NET, cache={}):
    if (net.name, seq.id) not in cache:
        cache[net.name, seq.id] = S.run_reference(net, seq.ops)
    return cache[net.name, seq.id]


def visibility(ops, net=NET):
    """[(position, mutation kind, observer position, observer kind, rel_err of the observer's head with / without)]."""
    seen, _ = S.run_reference(net, ops)
    with_ = {pos: got['y'] for pos, _, got in seen}
    out = []
    for i, o in enumerate(ops):
        if o.kind not in S.MUTATIONS:
            continue
        j = S.first_observer(ops, i)
        if j is None:
            out.append((i, o.kind, None, None, 0.0))
            continue
        without, _ = S.run_reference(net, ops, skip=i, stop=j + 1)
        y0 = without[-1][2]['y']
        out.append((i, o.kind, j, ops[j].kind, rel_err(with_[j].numpy(), y0.numpy())))
    return out


def tame(seen):
    """Finite heads, and max|y| within 10 x the first value of the same mode (an eval-mode head of this net is 8 - 10 x a
    training-mode one before anything is changed: 28.6 and 36.4 against 3.3 on the seeded state, so the first value is taken
    per mode)."""
    first = {}
    worst = 0.0
    for _, o, got in seen:
        y = got['y']
        if not bool(torch.isfinite(y).all()):
            return False, float('inf')
        fam = o.kind in S.EVAL_KINDS
        m = float(y.abs().max())
        first.setdefault(fam, m)
        worst = max(worst, m / first[fam])
    return worst <= 10.0, worst


@pytest.mark.parametrize('seq', S.ALL, ids=ids(S.ALL))
def test_every_mutation_is_visible_to_its_first_observer(seq):
    rows = visibility(seq.ops)
    for i, kind, j, okind, e in rows:
        print('SEQ %s op %d %s -> op %s %s: %.3e' % (seq.id, i, kind, j, okind, e))
    assert rows or not any(o.kind in S.MUTATIONS for o in seq.ops)
    for i, kind, j, okind, e in rows:
        assert j is not None, (seq.id, i, kind, 'no observer: a generator bug')
        assert e >= VISIBLE, (seq.id, i, kind, j, okind, e)


@pytest.mark.parametrize('seq', S.ALL, ids=ids(S.ALL))
def test_the_reference_stays_tame(seq):
    seen, _ = _runs(seq)
    ok, worst = tame(seen)
    print('SEQ %s %d observations, max|y| / first of its mode: %.2f' % (seq.id, len(seen), worst))
    assert seen and ok, (seq.id, worst)


STRIDED = S.strided_sequences()


@pytest.mark.parametrize('seq', STRIDED, ids=ids(STRIDED))
def test_the_strided_net_sees_every_mutation_and_stays_tame(seq):
    """The same two conditions for the sequences tests/test_gpu_sequences.py runs on S.STRIDED_NET; and they do write the
    strided block's filter, running statistics and frozen prefix."""
    net = S.STRIDED_NET
    info = T.layer_info(T.blocks_of(net.case), net.case.H, net.case.W)
    convs = [l for l in info if l.type == 'convolutional']
    assert net.case.channels == 3 and T._is_s2(convs[net.mid]) and T._is_bn(convs[net.mid]) and net.mid < net.kfreeze
    rows = visibility(seq.ops, net)
    for i, kind, j, okind, e in rows:
        print('SEQ strided %s op %d %s -> op %s %s: %.3e' % (seq.id, i, kind, j, okind, e))
        assert j is not None and e >= VISIBLE, (seq.id, i, kind, j, okind, e)
    assert rows
    seen, _ = _runs(seq, net)
    ok, worst = tame(seen)
    assert seen and ok, (seq.id, worst)


def test_the_strided_sequences_reach_the_strided_block():
    net = S.STRIDED_NET
    assert len(STRIDED) == 6 and len(set(s.id for s in STRIDED)) == 6
    ops = [o for s in STRIDED for o in s.ops]
    for kind in ('perturb_w', 'perturb_w_data', 'relayout', 'perturb_running'):
        assert any(o.kind == kind and o.args == (net.mid,) for o in ops), kind
    assert any(o.kind == 'freeze_prefix' and o.args[0] > net.mid for o in ops)
    for kind in ('load_weights', 'eval_graph', 'fused_step', 'group_step', 'torch_step', 'train_step'):
        assert any(o.kind == kind for o in ops), kind


def test_generated_sequences_keep_their_form():
    assert len(S.GEN_SEEDS) == 24 and len(set(S.GEN_SEEDS)) == 24
    for seq in S.GEN:
        kinds = [o.kind for o in seq.ops]
        assert 10 <= len(kinds) <= 14, seq.id
        assert sum(k in S.OBS_KINDS for k in kinds) >= 5, seq.id
        assert not any(k in S.GUARDS for k in kinds), seq.id
        assert set(o.args[0] for o in seq.ops if o.kind in S.OBS_KINDS) == {'A', 'B'}, seq.id
        assert seq.ops[-2:] == (S.op('eval', 'A'), S.op('eval', 'B')), seq.id
        for i, k in enumerate(kinds):
            if k in S.STEP_KINDS:
                assert i and kinds[i - 1] == 'train_step', (seq.id, i)
    known = S.OBS_KINDS + S.MUTATIONS + S.PRESERVING + S.MODE_CHANGES + S.GUARDS
    assert all(o.kind in known for s in S.ALL for o in s.ops)
    assert len(set(s.id for s in S.ALL)) == len(S.ALL)


def test_coverage_of_the_vocabulary():
    pairs, adj, trans, hist = (collections.Counter() for _ in range(4))
    for seq in S.ALL:
        for item in S.coverage_items(seq.ops):
            if item[0] in ('stay', 'resume'):
                hist[(item, 'generated' if seq in S.GEN else 'hand-written')] += 1
            else:
                {'pair': pairs, 'adj': adj, 'layout': trans}[item[0]][item[1:]] += 1
    print('mutation -> first observer (rows: mutation; columns: %s)' % ' '.join(S.OBS_KINDS))
    for m in S.MUTATIONS:
        print('  %-16s %s' % (m, ' '.join('%3d' % pairs[(m, o)] for o in S.OBS_KINDS)))
    print('adjacent observations (rows: first; columns: second)')
    for a in S.OBS_KINDS:
        print('  %-16s %s' % (a, ' '.join('%3d' % adj[(a, b)] for b in S.OBS_KINDS)))
    print('optimizer layout transitions: %s' % dict(trans))
    print('step histories: %s' % dict(hist))
    for h in S.HISTORY:
        assert hist[(h, 'generated')] >= 1, ('step history in a generated sequence', h)
    for p in S.PAIRS:
        assert pairs[p] >= 2, ('mutation -> observer', p, pairs[p])
    for a in S.OBS_KINDS:
        for b in S.OBS_KINDS:
            assert adj[(a, b)] >= 1, ('adjacent observations', a, b)
    for a in S.LAYOUTS:
        for b in S.LAYOUTS:
            assert a == b or trans[(a, b)] >= 1, ('layout transition', a, b)
    assert not S.coverage_needs(S.ALL)
    # every mode change is followed by an eval kind and by a train kind; every vocabulary entry is used
    used = collections.Counter(o.kind for s in S.ALL for o in s.ops)
    print('ops used: %s' % dict(used))
    for kind in S.OBS_KINDS + S.MUTATIONS + S.PRESERVING + S.MODE_CHANGES + S.GUARDS:
        assert used[kind] >= 1, kind
    for seq in S.ALL:
        for i, o in enumerate(seq.ops):
            if o.kind in S.MODE_CHANGES:
                later = [p.kind for p in seq.ops[i + 1:]]
                assert any(k in S.EVAL_KINDS for k in later) and any(k in S.TRAIN_KINDS for k in later), (seq.id, i, o.kind)


def test_the_layout_prediction_is_the_segment_table_rule():
    """expected_layout against singleshotpose_amd.optim.build_segment_table on the same momentum states: one tuple or two, with
    none, all or part of the parameters holding state."""
    from singleshotpose_amd.optim import build_segment_table
    side = S.RefSide(NET)
    side.opt = side._new_opt()
    named = side.named()
    flags = [b for _, b in S.group_list(named)]
    for kind in ('fused_step', 'group_step'):
        for frozen_k in (0, 3):
            for with_state in ('none', 'all', 'filters', 'tail'):
                side.opt.state.clear()
                side.apply(S.op('unfreeze'), 0)
                side.apply(S.op('freeze_prefix', frozen_k), 0)
                entries = []
                for idx, ((n, p), bn_or_bias) in enumerate(zip(named, flags)):
                    has = {'none': False, 'all': True, 'filters': not bn_or_bias, 'tail': idx >= len(named) // 2}[with_state]
                    if has:
                        side.opt.state[p]['momentum_buffer'] = torch.zeros_like(p)
                    p.grad = torch.zeros_like(p) if p.requires_grad else None
                    if p.requires_grad:
                        wd = 0.0 if (bn_or_bias and kind == 'group_step') else S.DECAY
                        entries.append((p.numel(), 4 * idx * 4096, (S.LR, S.MOMENTUM, 0.0, wd, False), has))
                want = 'table' if build_segment_table(entries) is not None else 'per_param'
                if kind == 'fused_step' and frozen_k == 0:
                    want = 'whole'
                assert side.expected_layout(kind) == want, (kind, frozen_k, with_state)


def test_determinism():
    for s in S.GEN_SEEDS[:6]:
        assert S.random_sequence(s) == S.random_sequence(s)
        assert S.random_sequence(s) == dict((q.id, q.ops) for q in S.GEN)['gen%03d' % s]
    seq = S.GEN[0]
    a, ra = S.run_reference(NET, seq.ops)
    b, rb = S.run_reference(NET, seq.ops)
    assert len(a) == len(b) >= 5
    for (_, _, x), (_, _, y) in zip(a, b):
        assert torch.equal(x['y'], y['y'])
        for k in x.get('stats', {}):
            assert torch.equal(x['stats'][k], y['stats'][k])
        for g, h in zip(x.get('grads', []), y.get('grads', [])):
            assert (g is None and h is None) or torch.equal(g, h)
    for (_, p), (_, q) in zip(ra.named(), rb.named()):
        assert torch.equal(p, q)

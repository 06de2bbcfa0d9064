"""The topology table (tests/topology_cases.py) and the plans it gets, without a GPU: the generator and its coverage, the
float64 reference against the real reference's goldens, the recorded data seeds and exact budgets, the plan of every
supported case (built on the CPU device: planning launches nothing) and the refusal of every other at construction."""
import collections
import os
import re
import zlib

import numpy as np
import pytest
import torch

import topology_cases as T
from helpers import GOLD, gold, rel_err
from test_generic_blocks_cpu import _grad_layout_covers

SUPPORTED = T.HAND + T.GEN + T.GS2 + T.EXACT + T.XS2
VARIANTS = [T.variant(T.CASES[i], v) for i in T.ROUTES for v in T.VARIANTS]
ids = lambda cases: [c.id for c in cases]


# ---------------------------------------------------------------------------------------------------- the table
def _is_new(case):
    """The cases the table gained with the stride-2 block; every other one is pinned by test_the_old_table_did_not_move."""
    return case.id.startswith(('s2_', 'gs2', 'xs2', 'wide-4', 'refused-first_s2', 'refused-odd-s2'))


def test_the_old_table_did_not_move():
    """crc32 of the cfg texts and of the recorded seeds of every case the table held before it learnt the stride-2 block,
    computed on that revision: teaching conv() / layer_info() / random_case() the block changed none of them."""
    old = [c for c in T.HAND + T.GEN + T.EXACT + T.REFUSED if not _is_new(c)]
    assert len(old) == 40 + 30 + 16 + 14
    assert zlib.crc32(''.join(T.cfg_text(c) for c in old).encode()) == 4245394828
    seeds = sorted((k, v) for k, v in T.SEEDS.items() if not _is_new(T.Case(k, *[None] * 7)))
    assert len(seeds) == 94 and zlib.crc32(repr(seeds).encode()) == 3221372156


def test_generator_is_deterministic():
    for seed in T.GEN_SEEDS[:5] + T.EXACT_SEEDS[:3]:
        assert T.random_cfg(seed) == T.random_cfg(seed) and T.random_cfg(seed, True) == T.random_cfg(seed, True)
        assert T.random_cfg(seed, False, True) == T.random_cfg(seed, False, True)
        assert T.random_cfg(seed, True, True) == T.random_cfg(seed, True, True)
    assert [T.random_case(s) for s in T.GEN_SEEDS] == T.GEN and [T.random_case(s, True) for s in T.EXACT_SEEDS] == T.EXACT
    assert [T.random_case(s, False, True) for s in T.GS2_SEEDS] == T.GS2
    assert not any(T.rank_one_first_block(c) for c in T.GS2) and T.rank_one_first_block(T.random_case(23, False, True))
    assert [T.random_case(s, True, True) for s in T.XS2_SEEDS] == T.XS2
    assert len(set(c.body for c in T.GEN + T.GS2)) == len(T.GEN + T.GS2)
    for c in T.GEN + T.EXACT + T.GS2 + T.XS2:
        strided = c in T.GS2 + T.XS2
        n = len(T.blocks_of(c)) - 1
        assert 4 <= n <= 9, (c.id, n)
        assert c.B in (1, 2, 3) and (13 if strided else 16) <= c.H <= 32 and (13 if strided else 16) <= c.W <= 32
        assert c.channels in (1, 3)
        info = T.layer_info(T.blocks_of(c), c.H, c.W)
        assert any(T._is_s2(l) for l in info) == strided, c.id
        for l in info:
            if l.type == 'convolutional':
                assert 4 <= l.C <= 64
                assert l.H >= 2 and l.W >= 2          # strided blocks stop shrinking at 2 x 2
                assert not T._is_bn(l) or c.B * l.H * l.W >= 32      # BatchNorm only over at least 32 samples (of the OUTPUT map)


def test_strided_generator_reads_the_batchnorm_rule_off_the_output_map():
    """Over the first 300 seeds of both strided streams (cfg text only): BatchNorm only where the map the block WRITES has
    B * Ho * Wo >= 32, strided blocks never as block 0 and never below 2 x 2 - and the rule bites: blocks whose INPUT map has
    32 samples and whose output map has not exist among them (none of those may carry BatchNorm)."""
    bites = 0
    for seed in range(300):
        for exact in (False, True):
            c = T.random_case(seed, exact, True)
            blocks = T.blocks_of(c)
            info = T.layer_info(blocks, c.H, c.W)
            for ind, l in enumerate(info):
                if l.type != 'convolutional':
                    continue
                assert not T._is_bn(l) or c.B * l.H * l.W >= 32, (c.id, ind)
                if T._is_s2(l):
                    _, hi, wi, _ = T._in_shape(info, ind, blocks, c.H, c.W)
                    assert ind > 0 and l.H >= 2 and l.W >= 2 and (l.H, l.W) == ((hi + 1) // 2, (wi + 1) // 2), (c.id, ind)
                    bites += (not exact) and c.B * hi * wi >= 32 > c.B * l.H * l.W
    assert bites >= 3, bites


def test_table_sizes_and_coverage():
    assert len(T.HAND) >= 10 and len(T.GEN) >= 30 and len(T.EXACT) >= 12 and len(T.GS2) >= 12 and len(T.XS2) >= 8
    assert len([c for c in T.HAND if c.id.startswith('s2_') and c.id.rsplit('-', 1)[0] in T.HAND_PROPS]) >= 30
    assert len(T.CASES) == len(SUPPORTED) + len(T.REFUSED)       # ids are unique
    count = collections.Counter()
    for c in SUPPORTED:
        assert T.supported(T.blocks_of(c), c.B, c.H, c.W) == [], c.id
        count.update(T.features(T.blocks_of(c), c.B, c.H, c.W))
    for f in T.GRAMMAR + T.HAND_PROPS:
        assert count[f] >= 3, (f, count[f])
    for c in T.HAND:
        prop = c.id.rsplit('-', 1)[0]
        if prop in T.HAND_PROPS:
            assert prop in T.features(T.blocks_of(c), c.B, c.H, c.W), c.id
    # the exact family: no BatchNorm, linear | relu, no softmax, avgpool over a power-of-two pixel count
    for c in T.EXACT + T.XS2:
        info = T.layer_info(T.blocks_of(c), c.H, c.W)
        for i, l in enumerate(info):
            assert l.type != 'softmax' and not T._is_bn(l)
            assert l.block.get('activation', 'linear') in ('linear', 'relu')
            if l.type == 'avgpool':
                px = info[i - 1].H * info[i - 1].W
                assert px & (px - 1) == 0
    # every block type among the cases that are run by more than one route; wide 3x3 layers among the tuned ones
    types = set(l.type for i in T.ROUTES for l in T.layer_info(T.blocks_of(T.CASES[i]), T.CASES[i].H, T.CASES[i].W))
    assert len(T.ROUTES) >= 10 and types == {'convolutional', 'maxpool', 'reorg', 'route', 'shortcut', 'avgpool', 'connected',
                                            'softmax'}
    strides = set(l.block['stride'] for i in T.ROUTES for l in T.layer_info(T.blocks_of(T.CASES[i]), 16, 16)
                  if l.type == 'maxpool')
    nroute = set(len(l.srcs) for i in T.ROUTES for l in T.layer_info(T.blocks_of(T.CASES[i]), 16, 16) if l.type == 'route')
    assert strides == {'1', '2'} and nroute == {1, 2}
    # ... and stride-2 blocks, one of them with BatchNorm in a generated case, one map read by two of them through aliases
    routed = [T.CASES[i] for i in T.ROUTES]
    assert any(c in T.GS2 and 's2_bn' in T.features(T.blocks_of(c), c.B, c.H, c.W) for c in routed)
    assert any('s2_alias_two_s2_consumers' in T.features(T.blocks_of(c), c.B, c.H, c.W) for c in routed)
    assert len(T.TUNED) >= 5
    # a tuned case where a stride-2 and a stride-1 3x3 layer launch data gradients of one shape (B, H, W of the map they
    # write, channels): the tuner must skip the strided one without skipping its neighbour
    c = T.CASES['wide-4']
    info = T.layer_info(T.blocks_of(c), c.H, c.W)
    wide = lambda k, l: l.type == 'convolutional' and l.block['size'] == '3' and l.C == 64 and info[k - 1].C == 64
    shapes = collections.Counter((T._is_s2(l), l.H, l.W) for k, l in enumerate(info) if k and wide(k, l))
    assert shapes[(True, 4, 4)] == 1 and shapes[(False, 4, 4)] == 1 and shapes[(False, 8, 8)] == 1
    for i in T.TUNED:
        c = T.CASES[i]
        info = T.layer_info(T.blocks_of(c), c.H, c.W)
        assert any(l.type == 'convolutional' and l.block['size'] == '3' and l.C >= 64 and info[k - 1].C >= 64
                   for k, l in enumerate(info) if k)
    for c in VARIANTS:
        assert T.supported(T.blocks_of(c), c.B, c.H, c.W) == [], c.id
        assert all(not T._is_bn(l) or c.B * l.H * l.W >= 32 for l in T.layer_info(T.blocks_of(c), c.H, c.W)), c.id


def test_refused_table():
    classes = collections.Counter()
    for c in T.REFUSED:
        bad = T.supported(T.blocks_of(c), c.B, c.H, c.W)
        assert bad, c.id
        classes.update(set(k for k, _ in bad))
    for k in ('route3', 'route_first', 'concat4', 'odd', 'last4', 'narrow', 'first_s2'):
        assert classes[k] >= 2, (k, classes[k])
    assert len([c for c in T.REFUSED if _is_new(c)]) == 4
    # an odd map that a strided block made, not the network input
    made = [c for c in T.REFUSED if c.H % 2 == 0 and c.W % 2 == 0 and
            any(k == 'odd' and T.layer_info(T.blocks_of(c), c.H, c.W)[i - 1].type == 'convolutional' and
                T._is_s2(T.layer_info(T.blocks_of(c), c.H, c.W)[i - 1]) for k, i in T.supported(T.blocks_of(c), c.B, c.H, c.W))]
    assert len(made) >= 2


# ---------------------------------------------------------------------------------------------------- the reference
GOLDEN = {'pose': ('generic-pose.cfg', 2, 80, 80), 'cls': ('generic-cls.cfg', 4, 64, 64),
          'strided': ('generic-strided.cfg', 2, 40, 44)}


@pytest.mark.parametrize('tag', sorted(GOLDEN))
def test_reference_reproduces_the_goldens(tag, tmp_path):
    """The float64 forward of topology_cases on the reference Darknet's own numbers (tools/gen_generic_blocks_golden.py), at
    the bars tests/test_gpu_generic_blocks.py::test_network_matches_reference holds the product to."""
    from singleshotpose_amd.darknet import Darknet
    g = gold('generic_%s.npz' % tag)
    p = str(tmp_path / 'w.weights')
    with open(p, 'wb') as f:
        f.write(g['weights'].tobytes())
    model = Darknet(os.path.join(GOLD, GOLDEN[tag][0]))
    model.load_weights(p)
    x = torch.from_numpy(g['x'])
    with torch.no_grad():
        y = T.ref_generic(model, x, False)
    assert tuple(y.shape) == tuple(g['y_eval'].shape) and rel_err(y.numpy(), g['y_eval']) < 1e-4
    y, mods, _ = T.ref_run(model, x, True)
    assert tuple(y.shape) == tuple(g['y_train'].shape) and rel_err(y.detach().numpy(), g['y_train']) < 1e-4
    for n, b in mods.named_buffers():
        if 'running' in n:
            np.testing.assert_allclose(b.numpy(), g['buf/models.' + n], rtol=1e-4, atol=1e-5)
    (y * torch.from_numpy(g['probe']).double()).sum().backward()
    de_mine, de_ref, dn_mine, dn_ref = [], [], [], []
    for n, prm in mods.named_parameters():
        n = 'models.' + n
        gr = prm.grad.numpy()
        if 'g64/' + n in g.files:
            ref64, ref32, mine = g['g64/' + n], g['grad/' + n], gr
        else:
            ref64, ref32 = g['g64slice/' + n], g['gslice/' + n]
            mine = gr.reshape(-1)[:: max(1, gr.size // len(ref64))][:len(ref64)]
        de_mine.append(rel_err(mine, ref64))
        de_ref.append(rel_err(ref32, ref64))
        dn_mine.append(abs(float(np.sqrt((gr ** 2).sum())) / float(g['g64norm/' + n][0]) - 1))
        dn_ref.append(abs(float(g['gnorm/' + n][0]) / float(g['g64norm/' + n][0]) - 1))
    assert max(de_mine) <= max(3.0 * max(de_ref), 3e-4) and max(dn_mine) <= max(3.0 * max(dn_ref), 3e-4)
    # float64 against float64: the same numbers, not merely within the fp32 envelope
    assert max(de_mine) < 1e-9 and max(dn_mine) < 1e-9, (max(de_mine), max(dn_mine))


def test_reference_does_not_read_the_engine():
    src = open(T.__file__.replace('.pyc', '.py')).read()
    assert not re.search(r'^\s*(from|import)\s+\S*engine', src, re.M)
    assert 'engine' not in ''.join(T.ref_run.__code__.co_names + T.supported.__code__.co_names)


# ---------------------------------------------------------------------------------------------------- seeds, budgets
@pytest.mark.parametrize('case', T.FLOAT + VARIANTS, ids=ids(T.FLOAT + VARIANTS))
def test_recorded_seed_has_every_decision_margin(case):
    seed = T.SEEDS[case.id]
    assert 0 <= seed <= 7
    margin, diff = T.margins(case, seed)
    assert diff < 1e-5              # the two CPU runs agree to fp32 rounding
    assert margin >= 4.0 * diff, (margin, diff)


def test_recorded_seeds_are_the_first():
    for case in T.FLOAT[::7]:
        assert T.find_seed(case) == T.SEEDS[case.id], case.id


@pytest.mark.parametrize('case', T.EXACT + T.XS2, ids=ids(T.EXACT + T.XS2))
def test_exact_case_is_exact_and_within_budget(case):
    assert T.exact_budget(case) < 2 ** 24
    r64, r32 = T.reference(case, 0)
    for a, b, what in [(r64.y_eval, r32.y_eval, 'y_eval'), (r64.y_train, r32.y_train, 'y_train'), (r64.dx, r32.dx, 'dx')] + \
            [(r64.grads[n], r32.grads[n], n) for n in r64.grads]:
        assert (a is None) == (b is None), what
        if a is not None:
            assert torch.equal(a.float(), b) and torch.equal(a, b.double()), what
    assert torch.equal(r64.y_eval, r64.y_train)          # no BatchNorm: one forward
    # integer data must not be trivial data: the output and the input gradient are mostly non-zero, relu zeros exist
    assert float((r64.y_train != 0).double().mean()) > 0.33 and float((r64.dx != 0).double().mean()) > 0.1


# ---------------------------------------------------------------------------------------------------- plans
def _no_launch(monkeypatch):
    from singleshotpose_amd import _lib

    def call(name, *args):
        raise AssertionError("planning launched %s" % name)
    monkeypatch.setattr(_lib, 'call', call)


@pytest.mark.parametrize('case', SUPPORTED + VARIANTS, ids=ids(SUPPORTED + VARIANTS))
def test_supported_case_plans(case, monkeypatch):
    from singleshotpose_amd import engine
    monkeypatch.delenv('SSP_BN_FUSE', raising=False)
    _no_launch(monkeypatch)
    model = T.make_model(case, init=False)
    plan = engine.Plan(model, case.B, case.H, case.W, torch.device('cpu'))
    plan._plan_bn_fusion()
    blocks = T.blocks_of(case)
    info = T.layer_info(blocks, case.H, case.W)
    assert plan.consumers == T.consumers_of(info)
    assert plan.fused_pool == T.expected_fused_pool(blocks, case.B, case.H, case.W)
    fused = {cs.ind: cs.bn_fuse_src.ind for cs in plan.convs.values() if cs.bn_fuse_src is not None}
    assert fused == T.expected_bn_fuse(blocks, case.B, case.H, case.W)
    _grad_layout_covers(plan, model)
    assert sorted(plan.convs) == [i for i, l in enumerate(info) if l.type in ('convolutional', 'connected')]
    for ind, cs in plan.convs.items():
        assert cs.conv.weight.shape[1] == cs.cin and cs.conv.weight.shape[0] == cs.cout == info[ind].C
        assert cs.inp.ld >= cs.cinp and (cs.inp.C, cs.inp.H, cs.inp.W) == T._in_shape(info, ind, blocks, case.H, case.W)[:3]
        # the map the block reads and the map its convolution writes (they differ behind a stride of 2, and a fused pool
        # halves the stored activation once more, not the convolution's output)
        assert cs.stride == int(info[ind].block.get('stride', 1)), ind
        assert (cs.Hi, cs.Wi) == T._in_shape(info, ind, blocks, case.H, case.W)[1:3], ind
        assert (cs.H, cs.W) == (info[ind].H, info[ind].W) and cs.M == case.B * cs.H * cs.W, ind
        assert cs.stride == 1 or cs.bn_fuse_src is None, ind
    for ind, l in enumerate(info):
        a = plan.acts[ind]
        if ind + 1 in plan.fused_pool:
            assert a is None          # the un-pooled map of a block with a fused pool never exists
            continue
        assert (a.C, a.H, a.W, a.ld) == (l.C, l.H, l.W, l.ld), ind
    o = plan.out_act
    assert o.ld == o.C and plan.last == len(info) - 1


@pytest.mark.parametrize('case', T.REFUSED, ids=ids(T.REFUSED))
def test_refused_case_is_refused_at_construction(case, monkeypatch):
    """Darknet(cfg) or Plan(...) raises NotImplementedError naming the block, on the CPU device, before any launch."""
    from singleshotpose_amd import engine
    _no_launch(monkeypatch)
    blocks = [i for _, i in T.supported(T.blocks_of(case), case.B, case.H, case.W)]
    with pytest.raises(NotImplementedError) as e:
        model = T.make_model(case, init=False)
        engine.Plan(model, case.B, case.H, case.W, torch.device('cpu'))
    m = re.match(r'block (\d+) \((\w+)\)', str(e.value))
    assert m, str(e.value)
    assert int(m.group(1)) in blocks and m.group(2) == T.blocks_of(case)[int(m.group(1)) + 1]['type'], str(e.value)

"""Darknet blocks outside the yolo-pose cfgs (shortcut, stride-1 max-pool, avgpool, softmax, connected), host side:
module tree and .weights I/O against the reference's (tests/golden/generic_*.npz, tools/gen_generic_blocks_golden.py), and
the execution plan those cfgs get (built on the CPU device: planning launches nothing)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLD, gold

CFGS = {'pose': ('generic-pose.cfg', 2, 80, 80), 'cls': ('generic-cls.cfg', 4, 64, 64)}


def _model(tag):
    from singleshotpose_amd.darknet import Darknet
    return Darknet(os.path.join(GOLD, CFGS[tag][0]))


def _plan(model, tag):
    from singleshotpose_amd import engine
    _, B, H, W = CFGS[tag]
    return engine.Plan(model, B, H, W, torch.device('cpu'))


def _write(tmp_path, data, name='w.weights'):
    p = str(tmp_path / name)
    with open(p, 'wb') as f:
        f.write(data)
    return p


@pytest.mark.parametrize('tag', sorted(CFGS))
def test_module_tree_matches_reference(tag):
    g = gold('generic_%s.npz' % tag)
    sd = _model(tag).state_dict()
    assert list(sd.keys()) == [str(k) for k in g['keys']]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g['shapes']))


@pytest.mark.parametrize('tag', sorted(CFGS))
def test_weights_round_trip_byte_for_byte(tag, tmp_path):
    g = gold('generic_%s.npz' % tag)
    stream = g['weights'].tobytes()
    m = _model(tag)
    m.load_weights(_write(tmp_path, stream))
    out = str(tmp_path / 'out.weights')
    m.save_weights(out)
    assert open(out, 'rb').read() == stream


def test_connected_modules_and_parameters():
    from singleshotpose_amd.darknet import Darknet
    m = _model('cls')
    fc1, fc2 = m.models[7], m.models[8]
    # leaky -> Sequential(Linear, LeakyReLU(0.1)); linear -> bare Linear (darknet.py:215-229)
    assert isinstance(fc1, torch.nn.Sequential) and isinstance(fc1[0], torch.nn.Linear)
    assert isinstance(fc1[1], torch.nn.LeakyReLU) and fc1[1].negative_slope == 0.1
    assert isinstance(fc2, torch.nn.Linear)
    ids = set(id(p) for p in Darknet._params(m))
    assert ids == set(id(p) for p in m.parameters())
    assert id(fc2.weight) in ids and id(fc2.bias) in ids


def test_plan_ops_pose_cfg():
    m = _model('pose')
    plan = _plan(m, 'pose')
    kinds = [op.kind for op in plan.ops]
    assert kinds.count('shortcut') == 3 and kinds.count('maxpool_s1') == 1
    sc = {op.ind: op for op in plan.ops if op.kind == 'shortcut'}
    assert sorted(sc) == [6, 9, 15]
    assert [sc[i].slope for i in (6, 9, 15)] == [1.0, 0.1, 0.0]     # linear, leaky, relu
    assert sc[15].srcs[0] is sc[15].srcs[1]                          # from = -1: both summands are one map
    # the layers whose gradient buffers receive each map's gradient, resolved at plan construction
    assert [a.producer for a in sc[6].srcs] == [3, 5]
    assert [a.producer for a in sc[15].srcs] == [14, 14]
    assert plan.convs[0].out.producer == 1                           # a fused pool's output belongs to the pool
    assert plan.convs[4].inp.producer == 3
    # layer 3 (pool output) feeds conv 4 and shortcut 6; layer 6 feeds conv 7 and shortcut 9
    assert sorted(plan.consumers[3]) == [4, 6] and sorted(plan.consumers[6]) == [7, 9]
    assert plan.consumers[14] == [15, 15]
    # the 2x2/2 pools after BN blocks stay fused into them (first block included: the conv's only consumer is its pool,
    # whatever reads the pool's output); pool 10 follows a shortcut and runs standalone
    assert plan.fused_pool == {1, 3, 12} and 'maxpool' in kinds and plan.convs[0].pool
    assert 14 not in plan.fused_pool and plan.acts[14].H == 5 and plan.acts[14].W == 5
    # non-BN relu / leaky convolutions on the bias path
    for ind, slope in ((7, 0.0), (8, 0.1)):
        cs = plan.convs[ind]
        assert not cs.bn and cs.conv.bias is not None and cs.slope == slope and cs.needs_act
    assert not plan.out_flat and (plan.out_act.C, plan.out_act.H, plan.out_act.W) == (20, 5, 5)
    _grad_layout_covers(plan, m)


def test_plan_pose_cfg_bn_fusion_skips_shortcut_sources():
    """A block whose output is also read by a shortcut has two consumers: its BatchNorm-backward sums are not folded into
    the consumer conv's data-gradient launch (engine.Plan._plan_bn_fusion)."""
    m = _model('pose')
    plan = _plan(m, 'pose')
    plan._plan_bn_fusion()
    fused = {cs.ind: cs.bn_fuse_src.ind for cs in plan.convs.values() if cs.bn_fuse_src is not None}
    assert fused == {5: 4}          # conv 4 -> conv 5 is the only single-consumer BN conv -> conv pair


def test_plan_ops_classifier_cfg():
    m = _model('cls')
    plan = _plan(m, 'cls')
    kinds = [op.kind for op in plan.ops]
    assert kinds == ['conv', 'conv', 'conv', 'conv', 'avgpool', 'conv', 'conv', 'softmax']
    assert sorted(plan.convs) == [0, 2, 4, 5, 7, 8]
    fc1, fc2 = plan.convs[7], plan.convs[8]
    assert (fc1.k, fc1.H, fc1.W, fc1.M, fc1.cin, fc1.cout, fc1.slope) == (1, 1, 1, 4, 64, 32, 0.1)
    assert (fc2.k, fc2.M, fc2.cin, fc2.cout, fc2.slope) == (1, 4, 32, 16, 1.0)
    assert fc1.conv is m.models[7][0] and fc2.conv is m.models[8]
    from singleshotpose_amd.engine import _is_packed
    assert _is_packed(fc1.conv.weight, fc1.cinp) and _is_packed(fc2.conv.weight, fc2.cinp)
    assert plan.last == 9 and plan.out_flat and (plan.out_act.C, plan.out_act.H, plan.out_act.W) == (16, 1, 1)
    _grad_layout_covers(plan, m)


def _grad_layout_covers(plan, model):
    lay = plan.grad_layout
    assert set(lay) == set(id(p) for p in model.parameters())
    for p in model.parameters():
        off, n, shape = lay[id(p)]
        assert n == p.numel() and shape == tuple(p.shape) and off % 4 == 0 and off + n <= plan.grad_total
    spans = sorted((lay[id(p)][0], lay[id(p)][0] + lay[id(p)][1]) for p in model.parameters())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))       # disjoint


NET = '[net]\nheight=%d\nwidth=%d\nchannels=3\n\n'
CONV = '[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n'
POOL = '[maxpool]\nsize=2\nstride=2\n\n'
HEAD = '[convolutional]\nfilters=%d\nsize=1\nstride=1\npad=1\nactivation=linear\n\n'


@pytest.mark.parametrize('body,msg', [
    (CONV % 8 + '[maxpool]\nsize=3\nstride=2\n\n', 'maxpool'),
    (CONV % 8 + '[reorg]\nstride=3\n\n', 'reorg'),
    (CONV % 8 + '[connected]\noutput=16\nactivation=leaky\n\n', 'connected'),
    (CONV % 8 + CONV % 16 + '[shortcut]\nfrom=-2\nactivation=linear\n\n', 'same shape'),
    (CONV % 8 + '[convolutional]\nfilters=8\nsize=5\nstride=1\npad=1\nactivation=leaky\n\n', 'conv'),
    # what a launch would decline, or worse, is declined when the plan is built (the bodies of tests/topology_cases.py)
    (CONV % 8 + CONV % 8 + CONV % 8 + '[route]\nlayers=-1,-3,-1\n\n' + HEAD % 20, r'block 3 \(route\): 3 layers'),
    (CONV % 8 + CONV % 8 + '[route]\nlayers=-2,-1\n\n' + HEAD % 8, r'block 2 \(route\): the first of two'),
    (CONV % 18 + CONV % 6 + '[route]\nlayers=-1,-2\n\n' + HEAD % 8, r'block 2 \(route\): concatenates layer 1 with 6'),
    ((CONV % 8 + POOL) * 3 + CONV % 8 + POOL + HEAD % 8, r'block 7 \(maxpool\): a standalone 2x2/2 max-pool of a 3 x 3'),
    ((CONV % 8 + POOL) * 3 + CONV % 8 + '[reorg]\nstride=2\n\n' + HEAD % 8, r'block 7 \(reorg\): reorg of a 3 x 3'),
    (CONV % 8 + HEAD % 18, r'block 1 \(convolutional\): the network output has 18'),
])
def test_still_refused(tmp_path, body, msg):
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.engine import Plan
    cfg = tmp_path / 'bad.cfg'
    cfg.write_text(NET % (24, 24) + body)
    with pytest.raises(NotImplementedError, match=msg):
        m = Darknet(str(cfg))
        Plan(m, 1, 24, 24, torch.device('cpu'))


def test_parameter_width_is_checked_against_the_map(tmp_path):
    """A conv whose parameter was built for another input width than the map the plan hands it (a module tree edited after
    construction) is refused when the plan is built, not read out of bounds by its first launch."""
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.engine import Plan
    cfg = tmp_path / 'w.cfg'
    cfg.write_text(NET % (24, 24) + CONV % 8 + CONV % 16 + HEAD % 8)
    m = Darknet(str(cfg))
    m.models[1][0] = torch.nn.Conv2d(4, 16, 3, 1, 1, bias=False)
    with pytest.raises(NotImplementedError, match=r'block 1 \(convolutional\): its parameter takes 4 input channels'):
        Plan(m, 1, 24, 24, torch.device('cpu'))

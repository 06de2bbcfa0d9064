"""The product's state between launches against models that have none: every observation of every sequence of
tests/sequence_cases.py is compared with

1. a stateless twin - a fresh Darknet built at that moment from the model's state_dict, modes and requires_grad flags, fed the
   float form of the input, used once and dropped: eval-kind heads bit for bit (the suite asserts that equality for a fresh model,
   for uint8 input and for graph replay), everything that passes through the atomically summed filter gradients or the batch
   statistics under the spread of two twins (tests/test_gpu_finetune.py::_spread_ok: 4 x their distance, floor 1e-6);
2. the float64 reference interpreter: heads at 1e-4, running statistics at rtol 1e-4 / atol 1e-5 (the project's bars).  Its
   optimizer steps take the GPU run's gradients - the update is linear in them, while two independent backwards differ by
   whole pool-winner flips on the 3 x 3 maps (tests/test_gpu_finetune.py) - so gradients are compared with the twins only;
3. an optimizer shadow: torch.optim.SGD on CPU copies fed the GPU run's gradients (tests/test_gpu_optim.py::_shadow_step),
   parameters and momentum at 1e-6 after every step and after an optimizer state round trip.

Every figure is printed before it is asserted (lines starting with SEQ)."""
import numpy as np
import pytest
import torch

import sequence_cases as S
import topology_cases as T
from helpers import rel_err

pytestmark = pytest.mark.gpu
FWD, SGD_BAR = 1e-4, 1e-6
ids = lambda seqs: [s.id for s in seqs]


def _dist(a, b):
    return rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())


class _Figures(object):
    def __init__(self, name):
        self.name, self.fwd, self.spread, self.twin = name, {}, 0.0, 0.0

    def report(self):
        print('SEQ %s worst forward error against float64 per kind: %s' % (
            self.name, ' '.join('%s %.2e' % kv for kv in sorted(self.fwd.items()))))
        print('SEQ %s worst distance to a twin %.2e, worst distance between two twins %.2e' % (self.name, self.twin, self.spread))


def _snapshot(side):
    return dict(sd={k: v.detach().clone() for k, v in side.model.models.state_dict().items()},
                rg=[p.requires_grad for p in side.model.parameters()], bnk=side.bn_eval_k)


def _copy_codes(src, dst):
    """The twin's plan runs the kernels the model's plan runs (the tuned variant): forward codes as _apply_head_budget moves a
    layer, data- / filter-gradient choices as _sync_codes adopts them."""
    for ind, cs in src.convs.items():
        dst.set_code(dst.convs[ind], 'fwd', cs.plan_fwd)
    dst._settle()
    dst._head_budget_done = True
    if src._dgrad_tuned:
        dst._prepare_backward()
        for ind, cs in src.convs.items():
            dst.set_code(dst.convs[ind], 'dgrad', cs.plan_dgrad)
            dst.set_code(dst.convs[ind], 'wgrad', cs.wgrad_wino)
        dst._settle()


def _twin_run(side, snap, o, pos, monkeypatch, tuned):
    """One observation on a fresh model in the snapshot's state: no cache to be stale."""
    kind = o.kind if o.kind in ('eval_autograd', 'backward_across_shapes') + S.TRAIN_KINDS else 'eval'
    if tuned:
        monkeypatch.setenv('SSP_AUTOTUNE', '0')       # the twin takes the model's codes, it times nothing itself
    try:
        twin = S.build_model(side.net, init=False).cuda()
        twin.models.load_state_dict(snap['sd'])      # (the module tree: a cfg without a region layer lists its last block twice)
        for p, r in zip(twin.parameters(), snap['rg']):
            p.requires_grad_(r)
        twin.graph_inference = False
        ts = S.ProductSide(side.net, twin)
        ts.bn_eval_k = snap['bnk']
        if tuned:
            dev = next(twin.parameters()).device
            for key, plan in side.model._plans.items():
                _copy_codes(plan, twin._plan(key[:3], dev))
        got = ts.observe(S.Op(kind, o.args), pos)
    finally:
        if tuned:
            monkeypatch.setenv('SSP_AUTOTUNE', '1')
    for a, b in zip(side.model.modules(), twin.modules()):
        assert a.training == b.training
    assert len(twin._plans) <= 2
    return got


def _tensors(got):
    """(name, tensor) of everything an observation produced but the eval head."""
    out = [('y', got['y'])] + ([('y2', got['y2'])] if 'y2' in got else [])
    out += [('grad%d' % i, g) for i, g in enumerate(got.get('grads', []))]
    out += [('stat:' + n, t) for n, t in sorted(got.get('stats', {}).items())]
    return out


def _check_observation(name, pos, o, got, twins, want, fig):
    tag = '%s op %d %s%s' % (name, pos, o.kind, o.args)
    t0 = twins[0]
    if o.kind in S.EVAL_KINDS:
        same = torch.equal(got['y'], t0['y'])
        print('SEQ %s head equals the twin: %s (distance %.2e)' % (tag, same, _dist(got['y'], t0['y'])))
        assert same, tag
        rest = _tensors(got)[1:]
    else:
        rest = _tensors(got)
    if rest:
        t1 = twins[1]
        for (n, a), (_, b), (_, c) in zip(rest, _tensors(t0)[-len(rest):], _tensors(t1)[-len(rest):]):
            if a is None or b is None:
                assert a is None and b is None and c is None, (tag, n)      # frozen: no gradient on either side
                continue
            d, s = _dist(a, b), _dist(c, b)
            fig.twin, fig.spread = max(fig.twin, d), max(fig.spread, s)
            if d > max(4 * s, 1e-6) * 0.25:
                print('SEQ %s %s distance to the twin %.2e, between two twins %.2e' % (tag, n, d, s))
            assert d <= max(4 * s, 1e-6), (tag, n, d, s)
    for key in ('y', 'y2'):
        if key in got:
            e = _dist(got[key], want[key])
            fig.fwd[o.kind] = max(fig.fwd.get(o.kind, 0.0), e)
            print('SEQ %s %s against float64: %.2e' % (tag, key, e))
            assert e < FWD, (tag, key, e)
    for n, b in got.get('stats', {}).items():
        np.testing.assert_allclose(b.cpu().numpy(), want['stats'][n].numpy(), rtol=1e-4, atol=1e-5, err_msg='%s %s' % (tag, n))


class _Shadow(object):
    """torch.optim.SGD on CPU copies, fed the GPU run's own gradients: one optimizer for the product's, one for torch_step's."""

    def __init__(self, side):
        self.side = side
        self.params = [torch.nn.Parameter(p.detach().cpu().clone()) for _, p in side.named()]
        self.names = [n for n, _ in side.named()]
        self.opt = self.topt = None

    def _groups(self, plain):
        return [dict(g, params=[q], weight_decay=0.0 if (b and not plain) else S.DECAY)
                for q, (g, b) in zip(self.params, S.group_list(zip(self.names, self.params)))]

    def before(self, kind):
        for (_, p), q in zip(self.side.named(), self.params):
            q.data.copy_(p.detach().cpu())
            q.grad = None if p.grad is None else p.grad.detach().cpu().clone()
        if kind == 'torch_step':
            if self.topt is None:
                self.topt = torch.optim.SGD(self.params, lr=S.LR, momentum=S.MOMENTUM, weight_decay=S.DECAY)
            self.topt.step()
            return
        if self.opt is None:
            self.opt = torch.optim.SGD(self._groups(True), lr=S.LR, momentum=S.MOMENTUM)
        for g, want in zip(self.opt.param_groups, self._groups(kind == 'fused_step')):
            g['weight_decay'] = want['weight_decay']
        self.opt.step()

    def check(self, tag, kind, params=True):
        mine, theirs = (self.topt, self.side.topt) if kind == 'torch_step' else (self.opt, self.side.opt)
        worst = 0.0
        for n, (_, p), q in zip(self.names, self.side.named(), self.params):
            if params:
                e = _dist(p, q)
                worst = max(worst, e)
                assert e < SGD_BAR, (tag, n, e)
            m = None if mine is None else mine.state.get(q, {}).get('momentum_buffer')
            t = theirs.state.get(p, {}).get('momentum_buffer')
            assert (m is None) == (t is None), (tag, n, 'momentum state')
            if m is not None:
                e = _dist(t, m)
                worst = max(worst, e)
                assert e < SGD_BAR, (tag, n, 'momentum', e)
        print('SEQ %s parameters and momentum against the shadow: %.2e' % (tag, worst))


def run_sequence(seq, net, model, monkeypatch, tmp_path, tuned=False):
    side = S.ProductSide(net, model, tmp_path)
    ref = S.RefSide(net, model)
    shadow = _Shadow(side)
    fig = _Figures(seq.id)
    for pos, o in enumerate(seq.ops):
        tag = '%s op %d %s%s' % (seq.id, pos, o.kind, o.args)
        if o.kind == 'stale_backward':
            side.observe(o, pos)         # raises unless the product refuses the backward
            ref.observe(o, pos)
        elif o.kind in S.OBS_KINDS or o.kind in S.GUARDS:
            snap = _snapshot(side)
            got = side.observe(o, pos)
            want = ref.observe(o, pos)
            n_twins = 1 if (o.kind in S.EVAL_KINDS and o.kind != 'eval_autograd') else 2
            twins = [_twin_run(side, snap, o, pos, monkeypatch, tuned) for _ in range(n_twins)]
            _check_observation(seq.id, pos, o, got, twins, want, fig)
            if o.kind == 'eval_graph':
                plan = model._plans[net.shapes[o.args[0]] + (torch.cuda.current_device(),)]
                assert plan._graph is not None and not plan._graph_failed, tag
        elif o.kind in S.STEP_KINDS:
            shadow.before(o.kind)
            grads = side.grads()
            count = lambda: (0, 0) if side.opt is None else (side.opt.fused_steps, side.opt.table_steps)
            before = count() if o.kind != 'torch_step' and side.opt is not None else (0, 0)
            side.apply(o, pos)
            torch.cuda.synchronize()
            ref.apply(o, pos, grads=grads)
            assert side.layouts[-1] == ref.layouts[-1], tag
            moved = tuple(a - b for a, b in zip(count(), before)) if o.kind != 'torch_step' else (0, 0)
            print('SEQ %s layout %s, fused_steps / table_steps moved by %s' % (tag, side.layouts[-1], moved))
            assert moved == {'whole': (1, 0), 'table': (0, 1), 'per_param': (0, 0)}[side.layouts[-1]], tag
            shadow.check(tag, o.kind)
        else:
            side.apply(o, pos)
            ref.apply(o, pos)
            if o.kind == 'opt_state_roundtrip':
                shadow.check(tag, o.kind, params=False)
    fig.report()
    shapes = set(net.shapes[s] for s in side.shapes_seen)
    assert set(k[:3] for k in model._plans) == shapes and len(model._plans) == len(shapes)
    return side


@pytest.mark.parametrize('seq', S.ALL, ids=ids(S.ALL))
def test_sequence(seq, monkeypatch, tmp_path):
    monkeypatch.setenv('SSP_AUTOTUNE', '0')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    model = S.build_model(S.TINY_NET).cuda()
    run_sequence(seq, S.TINY_NET, model, monkeypatch, tmp_path)


# ---------------------------------------------------------------------------------------------------- a strided block
STRIDED_SEQS = S.strided_sequences()


@pytest.mark.parametrize('seq', STRIDED_SEQS, ids=ids(STRIDED_SEQS))
def test_sequence_on_a_net_with_a_strided_block(seq, monkeypatch, tmp_path):
    """S.STRIDED_NET: the packed forward filter and the data-gradient operand of a stride-2 BatchNorm block (conv ordinal 1)
    across in-place writes, a relayout, frozen prefixes, optimizer steps in every layout, load_weights and graph replay."""
    monkeypatch.setenv('SSP_AUTOTUNE', '0')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    net = S.STRIDED_NET
    model = S.build_model(net).cuda()
    run_sequence(seq, net, model, monkeypatch, tmp_path)
    plan = model._plans[net.shapes['A'] + (torch.cuda.current_device(),)]
    cs = plan.convs[sorted(plan.convs)[net.mid]]
    assert cs.stride == 2 and cs.bn


# ---------------------------------------------------------------------------------------------------- tuned plans
TUNED_CASE = T.CASES[T.TUNED[0]]
TUNED_NET = S.case_net(TUNED_CASE, 2, 2)       # conv ordinals 2 and 3 are the 64 -> 64 3x3 layers; the first two blocks freeze
TUNED_SEQS = [s for s in S.hand_sequences(TUNED_NET) if s.id in S.TUNED_HAND] + \
    [S.Seq('gen%03d' % s, S.random_sequence(s, TUNED_NET)) for s in S.TUNED_GEN_SEEDS]


@pytest.mark.parametrize('seq', TUNED_SEQS, ids=ids(TUNED_SEQS))
def test_sequence_on_tuned_plans(seq, monkeypatch, tmp_path):
    """With the tuner on, so that the Winograd-transformed filters (`wino_version`) and the Winograd data-gradient operand are
    in play.  Conv ordinal 2 of shape A's plan - the layer the sequences write to - must run a Winograd forward code: the
    tuner's own where it chose one, else exact_conv.WINO2, set the way _apply_head_budget moves a layer (printed).  The codes
    then stay: the head-error budget, which would move them on the first training batch, is marked done."""
    from exact_conv import WINO2
    from singleshotpose_amd import engine
    monkeypatch.setenv('SSP_AUTOTUNE', '1')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    model = S.build_model(TUNED_NET).cuda()
    plan = model._plan(TUNED_NET.shapes['A'], torch.device('cuda', torch.cuda.current_device()))
    assert plan._tune
    chosen = [cs.ind for cs in plan.convs.values() if engine.wino_tile(cs.plan_fwd)]
    cs = plan.convs[sorted(plan.convs)[TUNED_NET.mid]]
    forced = not engine.wino_tile(cs.plan_fwd)
    if forced:
        assert cs.k == 3 and cs.cin % 16 == 0 and cs.cout % 16 == 0 and cs.cinp == cs.cin and not cs.first
        plan.set_code(cs, 'fwd', WINO2)
        plan._settle()
    plan._head_budget_done = True
    print('SEQ %s Winograd forward layers chosen by the tuner: %s; layer %d: %s' % (
        seq.id, chosen, cs.ind, 'WINO2 set by the test' if forced else 'the tuner\'s code %d' % cs.plan_fwd))
    run_sequence(seq, TUNED_NET, model, monkeypatch, tmp_path, tuned=True)
    print('SEQ %s codes %s' % (seq.id, [(c.ind, c.plan_fwd, c.plan_dgrad, c.wgrad_wino) for c in plan.convs.values()]))
    assert engine.wino_tile(cs.plan_fwd)
    assert cs.ind in plan.wino_version or any(o.kind == 'eval_graph' for o in seq.ops), "no Winograd-transformed filter was cached"


def test_a_moved_forward_code_recaptures_the_inference_graph(monkeypatch):
    """A captured inference chain holds the plan codes and the transformed-filter pointers of its moment: after conv ordinal
    2 moves from F(4x4) to F(2x2) and the F(4x4) filters are released - what the end of _apply_head_budget does - the next
    graph forward captures again and equals the eager forward bit for bit."""
    from exact_conv import WINO2, WINO4
    monkeypatch.setenv('SSP_AUTOTUNE', '1')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    model = S.build_model(TUNED_NET).cuda().eval()
    plan = model._plan(TUNED_NET.shapes['A'], torch.device('cuda', torch.cuda.current_device()))
    cs = plan.convs[sorted(plan.convs)[TUNED_NET.mid]]
    assert cs.k == 3 and cs.cin == cs.cout == 64 and cs.stride == 1 and not cs.first
    plan.set_code(cs, 'fwd', WINO4)
    plan._settle()
    x = T.make_input(TUNED_CASE, 0).cuda()
    with torch.no_grad():
        model.graph_inference = True
        model(x)
        graph0 = plan._graph
        model(x)
        assert graph0 is not None and plan._graph is graph0 and not plan._graph_failed
        u4 = id(cs.wino_u[4])
        plan.set_code(cs, 'fwd', WINO2)
        plan._settle()
        plan._release_filters('fwd', [cs])
        assert 4 not in cs.wino_u
        y = model(x)
        assert plan._graph is not graph0 and plan._graph is not None
        model.graph_inference = False
        want = model(x)
    print('SEQ recapture: F(4x4) filters %#x released, F(2x2) filters %#x, distance to the eager forward %.2e' % (
        u4, id(cs.wino_u[2]), _dist(y, want)))
    assert torch.equal(y, want)

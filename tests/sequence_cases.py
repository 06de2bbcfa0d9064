"""Seeded operation sequences against one model: the cases of tests/test_sequences_cpu.py and tests/test_gpu_sequences.py.

What the kernel tests cannot see is the host-side state the product keeps BETWEEN launches (packed and Winograd-transformed
filters, inference BatchNorm constants, the captured graph, one plan per input shape, the optimizer's flat layouts - the table
in DESIGN.md, "State kept between launches").  A stale entry is silent: every kernel is right and is fed an old operand.  So a
sequence of operations runs against ONE product model, and every observation is compared with models that have no such
state: a stateless twin built at that moment, the float64 reference interpreter below, and an optimizer shadow.

An op is a record (kind, args).  Layers are named by conv ORDINAL (0 = the first conv block of the cfg); shapes by 'A' / 'B'.

  observations   eval(S) eval_u8(S) eval_graph(S) eval_autograd(S)     model.eval(); the last one with grad mode on + backward
                 train_step(S) train_forward(S)                        model.train(); forward + backward / forward under no_grad
  mutations      perturb_w(j) perturb_gamma(j) perturb_beta(j)         no_grad in-place add of seeded noise
                 perturb_running(j)                                     running_mean += 0.25 sqrt(running_var) noise; var *= 2
                 perturb_w_data(j)                                      the same write through .data + engine.weights_changed()
                 load_weights(seed)                                     a .weights file of another seeded state
                 fused_step group_step torch_step                       an optimizer step on the gradients of the observation before
  value-preserving  relayout(j) model_state_roundtrip opt_state_roundtrip   the numbers stay, the tensors / storage / layout move
  mode changes   freeze_prefix(k) unfreeze bn_eval_prefix(k) bn_train_all
  guards (hand-written only)  stale_backward(S) backward_across_shapes

Modes: an observation calls model.eval() / model.train() itself; `bn_eval_prefix(k)` is a standing order - under model.train()
the BatchNorm modules of the conv blocks before ordinal k are put back in eval() before every train-kind forward.

Optimizers: ONE product optimizer lives through a sequence (singleshotpose_amd.optim.SGD on the GPU side, torch.optim.SGD in the
reference), built over the per-parameter group list of train.py:381-387.  `fused_step` gives every group the same weight decay
(uniform hyper-parameters: the whole-range launch when every parameter has a gradient, the segment table when a prefix is
frozen), `group_step` takes the decay off the BatchNorm / bias groups (two tuples: the segment table; per-parameter launches
when a tuple's parameters only partly have momentum state) - train.py rewrites group hyper-parameters between steps the same
way.  So momentum is carried across the layouts, which is the state under test.  `torch_step` is a second, stock
torch.optim.SGD over the same parameter tensors with its own momentum.  Layouts, for the coverage count: 'whole', 'table',
'per_param' (the update runs tensor by tensor on what the module tree holds: torch_step, or the product's own per-parameter
launches).  `expected_layout` predicts the one a step takes from the momentum state and the frozen set alone.

No GPU import at module level."""
import collections
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

import topology_cases as T
from helpers import GOLD, load_state_into

TINY = os.path.join(GOLD, 'tiny-pose.cfg')
LR, MOMENTUM, DECAY = 1e-4, 0.9, 5e-4

Op = collections.namedtuple('Op', 'kind args')
Seq = collections.namedtuple('Seq', 'id ops')
Net = collections.namedtuple('Net', 'name cfg case shapes mid kfreeze')

EVAL_KINDS = ('eval', 'eval_u8', 'eval_graph', 'eval_autograd')
TRAIN_KINDS = ('train_step', 'train_forward')
OBS_KINDS = EVAL_KINDS + TRAIN_KINDS
GRAD_KINDS = ('train_step', 'eval_autograd')                 # leave gradients behind: an optimizer step may follow
STEP_KINDS = ('fused_step', 'group_step', 'torch_step')
PARAM_MUTATIONS = ('perturb_w', 'perturb_gamma', 'perturb_beta', 'perturb_w_data', 'load_weights') + STEP_KINDS
MUTATIONS = PARAM_MUTATIONS + ('perturb_running',)           # every one of them must be visible to its first observer
PRESERVING = ('relayout', 'model_state_roundtrip', 'opt_state_roundtrip')
MODE_CHANGES = ('freeze_prefix', 'unfreeze', 'bn_eval_prefix', 'bn_train_all')
GUARDS = ('stale_backward', 'backward_across_shapes')
LAYOUTS = ('whole', 'table', 'per_param')

# (mutation kind, kind of its first observer): every pair that can see each other.  A changed parameter is seen by every
# observation, frozen or not; running statistics only by a block whose BatchNorm is in eval mode - every eval kind, and a train
# kind under a standing bn_eval_prefix that covers the layer (so those two pairs stay in).
PAIRS = tuple((m, o) for m in MUTATIONS for o in OBS_KINDS)


def op(kind, *args):
    return Op(kind, tuple(args))


# the net of the sequences: tiny-pose.cfg (12 conv blocks; first layer cin = 3 - always the packed-filter cache), seeded state 3,
# shapes A and B as the suite uses them on this cfg; mid = a 3x3 layer stored channels-last, kfreeze = the prefix hand-written
# sequences freeze
TINY_NET = Net('tiny', TINY, None, {'A': (2, 96, 96), 'B': (1, 128, 128)}, 5, 6)


def case_net(case, mid, kfreeze):
    """The same sequences on a topology case (the tuned variant): A = the case's shape, B = one image, 8 pixels larger."""
    return Net(case.id, None, case, {'A': (case.B, case.H, case.W), 'B': (1, case.H + 8, case.W + 8)}, mid, kfreeze)


def build_model(net, init=True):
    """The product's module tree on the CPU with the net's seeded parameters, in training mode."""
    if net.case is not None:
        return T.make_model(net.case, init=init).train()
    from oracle.darknet_ref import seeded_state
    from singleshotpose_amd.darknet import Darknet
    model = Darknet(net.cfg)
    if init:
        load_state_into(model, model.blocks, seeded_state(model.blocks, 3))
    return model.train()


def input_bytes(net, S, pos):
    """(B, H, W, 3) uint8 of observation `pos`: every input exists as bytes and as bytes.permute(0, 3, 1, 2).float().div(255)."""
    B, H, W = net.shapes[S]
    return torch.from_numpy(np.random.RandomState([B, H, W, pos]).randint(0, 256, (B, H, W, 3)).astype(np.uint8))


def as_float(xb):
    return xb.permute(0, 3, 1, 2).float().div(255)


def probe_of(y, seed=5):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(tuple(y.shape)).astype(np.float32))


def noise_of(pos, shape):
    return torch.from_numpy(np.random.RandomState([977, pos]).standard_normal(tuple(shape)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ reference forward
def _ref_forward(blocks, mods, x, frozen=None):
    """The reference's block semantics (darknet.py:82-130) on `mods` as they are - no .train() / .eval() call.  frozen: the
    product's decisions (_decisions), applied as oracle.darknet_ref.forward_ref applies them."""
    raw, act, pool = ((frozen or {}).get(k) or {} for k in ('raw_override', 'act_override', 'pool_override'))
    outputs = {}
    for ind, b in enumerate(blocks[1:]):
        t = b['type']
        if t == 'convolutional':
            for m in mods[ind]:
                if isinstance(m, torch.nn.LeakyReLU) and ind in act:
                    x = torch.where(act[ind] > 0, x, x * 0.1)
                    continue
                x = m(x)
                if isinstance(m, torch.nn.Conv2d) and ind in raw:
                    x = raw[ind].to(x.dtype) + (x - x.detach())
        elif t == 'maxpool' and ind in pool:
            x = x.flatten(2).gather(2, pool[ind].flatten(2)).view(pool[ind].shape)
        elif t == 'maxpool':
            x = F.max_pool2d(x, int(b['size']), int(b['stride']))
        elif t == 'reorg':
            x = T.reorg2(x)
        elif t == 'route':
            ls = T._resolve(b['layers'], ind)
            x = outputs[ls[0]] if len(ls) == 1 else torch.cat([outputs[l] for l in ls], 1)
        elif t == 'shortcut':
            x = outputs[T._resolve(b['from'], ind)[0]] + outputs[ind - 1]
            if b['activation'] in ('leaky', 'relu'):
                x = F.leaky_relu(x, 0.1) if b['activation'] == 'leaky' else F.relu(x)
        elif t in ('region', 'cost'):
            continue
        else:
            raise NotImplementedError(t)
        outputs[ind] = x
    return x


# ------------------------------------------------------------------------------------------------ the two interpreters
def group_list(named):
    """One group per parameter, as train.py:381-387 builds them; True = a BatchNorm or bias parameter."""
    return [({'params': [p]}, n.find('.bn') >= 0 or n.find('.bias') >= 0) for n, p in named]


class Side(object):
    """What both interpreters share: one module tree (`models`, indexed as the cfg's blocks), its modes and its optimizers.
    Subclasses say how a forward runs, how a .weights file arrives and which optimizer class takes the steps."""

    def __init__(self, net, blocks, models):
        self.net, self.blocks, self.models = net, blocks, models
        self.convs = [i for i, b in enumerate(blocks[1:]) if b['type'] == 'convolutional']
        self.bn_eval_k = 0
        self.opt = self.topt = None
        self.layouts = []            # the layout every step took, as expected_layout predicted it
        self.step_log = []           # ... and (kind, layout, first product step of an optimizer that loaded momentum)
        self._resumed = False
        self.shapes_seen = set()

    # ---- access
    def conv(self, j):
        return self.models[self.convs[j]][0]

    def bn(self, j):
        seq = self.models[self.convs[j]]
        return seq[1] if len(seq) > 1 and isinstance(seq[1], torch.nn.BatchNorm2d) else None

    def named(self):
        return list(self.models.named_parameters())

    def _like(self, t, ref):
        return t.to(device=ref.device, dtype=ref.dtype)

    def set_modes(self, train):
        self.root().train(train)
        if train:
            for j in range(self.bn_eval_k):
                if self.bn(j) is not None:
                    self.bn(j).eval()

    def zero_grad(self):
        for _, p in self.named():
            p.grad = None

    # ---- optimizers
    def _groups(self, plain):
        out = []
        for g, bn_or_bias in group_list(self.named()):
            g = dict(g)
            g['weight_decay'] = 0.0 if (bn_or_bias and not plain) else DECAY
            out.append(g)
        return out

    def _new_opt(self):
        return self.make_opt(self._groups(True), lr=LR, momentum=MOMENTUM)

    def expected_layout(self, kind):
        """The launch form a step takes: a pure function of the step kind, which parameters have a gradient and which have
        momentum state (singleshotpose_amd.optim.SGD.step / build_segment_table)."""
        if kind == 'torch_step':
            return 'per_param'
        held = [(p, bn_or_bias) for (n, p), (_, bn_or_bias) in zip(self.named(), group_list(self.named())) if p.grad is not None]
        if kind == 'fused_step' and len(held) == len(self.named()):
            return 'whole'
        tuples = {}
        for p, bn_or_bias in held:
            has = self.opt.state.get(p, {}).get('momentum_buffer') is not None
            tuples.setdefault(bn_or_bias and kind == 'group_step', set()).add(has)
        return 'table' if all(len(v) == 1 for v in tuples.values()) else 'per_param'

    def step(self, kind, grads=None):
        """grads: gradients to step on instead of this side's own (the float64 reference next to a GPU run takes the GPU run's:
        the optimizer is linear in them, while two independent backwards differ by whole pool-winner flips)."""
        if grads is not None:
            for (_, p), g in zip(self.named(), grads):
                p.grad = None if g is None else self._like(g.detach().cpu(), p).clone()
        assert any(p.grad is not None for _, p in self.named()), "an optimizer step without gradients"
        if kind == 'torch_step':
            if self.topt is None:
                self.topt = torch.optim.SGD([p for _, p in self.named()], lr=LR, momentum=MOMENTUM, weight_decay=DECAY)
            self.layouts.append('per_param')
            self.step_log.append((kind, 'per_param', False))
            self.topt.step()
            return
        if self.opt is None:
            self.opt = self._new_opt()
        for g, want in zip(self.opt.param_groups, self._groups(kind == 'fused_step')):
            g['weight_decay'] = want['weight_decay']
        self.layouts.append(self.expected_layout(kind))
        self.step_log.append((kind, self.layouts[-1], self._resumed))
        self._resumed = False
        self.opt.step()

    # ---- everything but observations
    def apply(self, o, pos, grads=None):
        kind, args = o
        if kind in ('perturb_w', 'perturb_w_data'):
            p = self.conv(args[0]).weight
            d = self._like(noise_of(pos, p.shape), p) * (0.25 * float(p.detach().std()))
            if kind == 'perturb_w':
                with torch.no_grad():
                    p.add_(d)
            else:
                p.data.add_(d)
                self.weights_changed()
        elif kind in ('perturb_gamma', 'perturb_beta'):
            p = self.bn(args[0]).weight if kind == 'perturb_gamma' else self.bn(args[0]).bias
            with torch.no_grad():
                p.add_(self._like(noise_of(pos, p.shape), p) * 0.25)
        elif kind == 'perturb_running':
            bn = self.bn(args[0])
            with torch.no_grad():
                d = self._like(noise_of(pos, bn.running_mean.shape), bn.running_mean)
                bn.running_mean.add_(0.25 * bn.running_var.sqrt() * d)
                bn.running_var.mul_(2)
        elif kind == 'relayout':
            p = self.conv(args[0]).weight
            p.data = p.data.contiguous()
        elif kind == 'load_weights':
            from oracle.darknet_ref import seeded_state
            self.load_weights(seeded_state(self.blocks, args[0]), pos)
        elif kind == 'model_state_roundtrip':
            m = self.root()
            m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
        elif kind in STEP_KINDS:
            self.step(kind, grads)
        elif kind == 'opt_state_roundtrip':
            old = self.opt if self.opt is not None else self._new_opt()
            self.opt = self._new_opt()
            self.opt.load_state_dict(old.state_dict())
            self._resumed = any('momentum_buffer' in st for st in self.opt.state.values())
            self.step_log.append((kind, None, False))
        elif kind == 'freeze_prefix':
            for j in range(args[0]):
                for p in self.models[self.convs[j]].parameters():
                    p.requires_grad_(False)
        elif kind == 'unfreeze':
            for _, p in self.named():
                p.requires_grad_(True)
        elif kind == 'bn_eval_prefix':
            self.bn_eval_k = args[0]
        elif kind == 'bn_train_all':
            self.bn_eval_k = 0
        else:
            raise ValueError(kind)

    def weights_changed(self):
        pass

    def stats(self):
        return {n: b.detach().clone() for n, b in self.models.named_buffers() if 'running' in n}

    def grads(self):
        return [None if p.grad is None else p.grad.detach().clone() for _, p in self.named()]

    # ---- observations and guards: {'y': head, 'grads': [per parameter or None], 'stats': {name: tensor}}
    def observe(self, o, pos):
        kind, args = o
        if kind == 'backward_across_shapes':
            self.shapes_seen.update('AB')
            self.set_modes(True)
            self.zero_grad()
            ya = self.forward('train_step', input_bytes(self.net, 'A', pos))
            yb = self.forward('train_step', input_bytes(self.net, 'B', pos))
            self.backward(ya)            # shape B's forward left shape A's saved activations alone
            return dict(y=ya.detach(), y2=yb.detach(), grads=self.grads(), stats=self.stats())
        S = args[0]
        self.shapes_seen.add(S)
        xb = input_bytes(self.net, S, pos)
        if kind == 'stale_backward':
            self.set_modes(True)
            self.zero_grad()
            self.stale_backward(xb, input_bytes(self.net, S, pos + 1000))
            return None
        train = kind in TRAIN_KINDS
        self.set_modes(train)
        self.zero_grad()
        out = {}
        if kind in GRAD_KINDS:
            y = self.forward(kind, xb)
            self.backward(y)
            out['grads'] = self.grads()
        else:
            with torch.no_grad():
                y = self.forward(kind, xb)
        out['y'] = y.detach()
        if train:
            out['stats'] = self.stats()
        return out


class RefSide(Side):
    """The float64 reference interpreter: a deep copy of the module tree on the CPU (it keeps every module's `training` flag and
    every parameter's `requires_grad`), run by _ref_forward; no cache of any kind."""

    def __init__(self, net, model=None):
        model = build_model(net) if model is None else model
        super(RefSide, self).__init__(net, model.blocks, copy.deepcopy(model.models).cpu().double())

    def root(self):
        return self.models

    def make_opt(self, groups, **kw):
        return torch.optim.SGD(groups, **kw)

    def load_weights(self, state, pos):
        load_state_into(self, self.blocks, state)

    def forward(self, kind, xb):
        return _ref_forward(self.blocks, self.models, as_float(xb).double())

    def backward(self, y):
        (y * probe_of(y).double()).sum().backward()

    def stale_backward(self, x1, x2):
        with torch.no_grad():            # two training-mode forwards moved the running statistics; the backward was refused
            self.forward('train_step', x1)
            self.forward('train_step', x2)


class ProductSide(Side):
    """The product: singleshotpose_amd.darknet.Darknet on the GPU, with every cache it keeps."""

    def __init__(self, net, model, tmpdir=None):
        super(ProductSide, self).__init__(net, model.blocks, model.models)
        self.model, self.tmpdir = model, tmpdir
        self.n_graph = 0

    def root(self):
        return self.model

    def make_opt(self, groups, **kw):
        from singleshotpose_amd.optim import SGD
        return SGD(groups, **kw)

    def weights_changed(self):
        from singleshotpose_amd.engine import weights_changed
        weights_changed()

    def load_weights(self, state, pos):
        from oracle.darknet_ref import write_weights
        path = os.path.join(str(self.tmpdir), 'seq_%d.weights' % pos)
        write_weights(path, self.blocks, state)
        self.model.load_weights(path)

    def forward(self, kind, xb):
        x = xb.cuda() if kind == 'eval_u8' else as_float(xb).cuda()
        if kind != 'eval_graph':
            return self.model(x)
        self.model.graph_inference = True
        try:
            self.n_graph += 1
            return self.model(x)
        finally:
            self.model.graph_inference = False

    def backward(self, y):
        (y * probe_of(y).cuda()).sum().backward()
        torch.cuda.synchronize()

    def stale_backward(self, x1, x2):
        import pytest
        y1 = self.model(as_float(x1).cuda())
        self.model(as_float(x2).cuda())
        with pytest.raises(RuntimeError, match='newer forward'):
            self.backward(y1)
        torch.cuda.synchronize()


def run_reference(net, ops, skip=None, stop=None):
    """The reference interpreter over ops[:stop] with op `skip` left out: [(position, op, observation)] of the observations."""
    ref = RefSide(net)
    seen = []
    for pos, o in enumerate(ops[:stop]):
        if pos == skip:
            continue
        if o.kind in OBS_KINDS or o.kind in GUARDS:
            got = ref.observe(o, pos)
            if got is not None:
                seen.append((pos, o, got))
        else:
            ref.apply(o, pos)
    return seen, ref


# ------------------------------------------------------------------------------------------------ who sees a mutation
def first_observer(ops, i):
    """Position of the first observation after mutation ops[i] that can depend on it, or None (a generator bug)."""
    kind, args = ops[i]
    k = 0
    for pos, o in enumerate(ops):
        if o.kind == 'bn_eval_prefix':
            k = o.args[0]
        elif o.kind == 'bn_train_all':
            k = 0
        if pos <= i or o.kind not in OBS_KINDS:
            continue
        if kind != 'perturb_running' or o.kind in EVAL_KINDS or args[0] < k:
            return pos
    return None


def layout_transitions(layouts):
    return [(a, b) for a, b in zip(layouts[:-1], layouts[1:]) if a != b]


# ------------------------------------------------------------------------------------------------ hand-written sequences
def hand_sequences(net=TINY_NET):
    m, k = net.mid, net.kfreeze
    ev, u8, gr, ag = (lambda S, kind=kind: op(kind, S) for kind in EVAL_KINDS)
    ts, tf = (lambda S, kind=kind: op(kind, S) for kind in TRAIN_KINDS)
    H = collections.OrderedDict()
    # the existing regressions, restated
    H['eval_step_eval'] = [ev('A'), ts('A'), op('fused_step'), ev('A')]
    H['eval_load_eval'] = [ev('A'), op('load_weights', 7), ev('A'), u8('A'), op('load_weights', 8), gr('A')]
    H['train_forward_between_evals_two_shapes'] = [ev('A'), ev('B'), ts('A'), ev('A'), ev('B'), tf('B'), ev('B'), ev('A')]
    H['graph_replay_after_in_place_update'] = [gr('A'), op('perturb_w', 0), ev('A'), gr('A'), op('perturb_running', 1), gr('A'),
                                               ev('A'), op('perturb_w_data', m), gr('A'), u8('A')]
    H['resume_momentum'] = [ts('A'), op('fused_step'), op('opt_state_roundtrip'), ts('A'), op('fused_step'),
                            op('model_state_roundtrip'), op('opt_state_roundtrip'), ts('A'), op('fused_step'), ev('A')]
    H['data_write_contract'] = [ev('A'), op('perturb_w_data', 0), ev('A'), u8('A'), op('relayout', m), ev('A'),
                                op('perturb_w_data', m), ev('A'), ev('B'), op('perturb_w_data', 0), ev('B')]
    # the crossings
    H['two_shapes_step_u8'] = [ev('A'), ev('B'), ts('A'), op('fused_step'), u8('B'), ev('A')]
    H['bn_eval_block_uses_new_running_statistics'] = [op('bn_eval_prefix', k), ts('A'), op('perturb_running', 1), ts('A'),
                                                      tf('B'), op('perturb_running', 0), tf('B'), op('bn_train_all'), ts('A'),
                                                      ev('A')]
    H['relayout_then_in_place_update'] = [op('relayout', m), ev('A'), op('perturb_w', m), ev('A'), ts('A'), op('fused_step'),
                                          ev('A')]
    H['table_to_whole_to_resumed'] = [op('freeze_prefix', k), ts('A'), op('group_step'), op('unfreeze'), ts('A'),
                                      op('fused_step'), op('opt_state_roundtrip'), ts('A'), op('fused_step'), ev('A'), ev('B')]
    H['eval_autograd_around_a_step'] = [ag('A'), op('fused_step'), ag('A'), ev('A')]
    H['state_roundtrip_after_adoption'] = [ts('A'), op('fused_step'), op('model_state_roundtrip'), ts('A'), op('fused_step'),
                                           ev('A')]
    # every optimizer layout entered from the other two; a mixed momentum state takes the per-parameter launches
    H['layouts_all_ways'] = [op('freeze_prefix', k), ts('A'), op('group_step'), op('unfreeze'), ts('A'), op('group_step'),
                             ts('B'), op('group_step'), ts('A'), op('torch_step'), ts('A'), op('fused_step'), ts('B'),
                             op('torch_step'), ts('A'), op('group_step'), ts('A'), op('fused_step'), ts('B'), op('group_step'),
                             ev('A'), ev('B')]
    H['frozen_eval_autograd_and_u8'] = [op('freeze_prefix', k), ag('A'), op('group_step'), u8('A'), ag('B'), tf('A'),
                                        op('unfreeze'), ag('A'), ts('A'), op('torch_step'), ag('A')]
    H['graph_sees_steps_and_in_place_writes'] = [gr('A'), op('perturb_w', 3), gr('A'), ts('A'), op('fused_step'), gr('A'), ts('B'),
                                                 op('fused_step'), gr('B'), op('perturb_w_data', 2), u8('A'), ev('B')]
    H['bn_eval_prefix_on_both_shapes'] = [op('bn_eval_prefix', k), ts('A'), ts('B'), op('perturb_running', 2), ts('B'),
                                          op('perturb_running', 0), tf('A'), u8('A'), op('bn_train_all'), tf('B'), ev('B')]
    # stock torch.optim.SGD writing through the views the product optimizer handed to the modules
    H['torch_step_on_adopted_views'] = [ts('A'), op('fused_step'), ts('A'), op('torch_step'), ev('A'), op('perturb_w_data', m),
                                        tf('B'), ts('B'), op('torch_step'), ev('B'), ts('A'), op('fused_step'), ev('A')]
    # the guards
    H['guard_stale_backward'] = [ev('A'), op('stale_backward', 'A'), ev('A'), ts('A'), op('fused_step'), ev('A')]
    H['guard_backward_across_shapes'] = [op('backward_across_shapes'), op('fused_step'), ev('A'), ev('B')]
    return [Seq(name, tuple(ops)) for name, ops in H.items()]


HAND = hand_sequences()
TUNED_HAND = ('graph_replay_after_in_place_update', 'relayout_then_in_place_update', 'table_to_whole_to_resumed')
# ... and two generated ones on that net: the first two seeds without a load_weights (it sends the plans back to their head-error
# budget) whose sequence writes the filter of conv ordinal 2 - the layer that runs a Winograd code there - in place between two
# eager forwards of shape A's plan
TUNED_GEN_SEEDS = (60, 378)


# ------------------------------------------------------------------------------------------------ generated sequences
def _layers(net):
    """(ordinals with BatchNorm, ordinals whose 3x3 filter is stored channels-last, conv count) of the net's cfg."""
    from singleshotpose_amd.cfg import parse_cfg
    blocks = T.blocks_of(net.case) if net.case is not None else parse_cfg(net.cfg)
    bn, cl, n, cin = [], [], 0, int(blocks[0].get('channels', 3))
    model = build_model(net, init=False)
    for m in model.models:
        if isinstance(m, torch.nn.Sequential) and isinstance(m[0], torch.nn.Conv2d):
            if len(m) > 1 and isinstance(m[1], torch.nn.BatchNorm2d):
                bn.append(n)
            if m[0].kernel_size[0] == 3 and m[0].in_channels % 4 == 0:
                cl.append(n)
            n += 1
    return bn, cl, n


_LAYERS = {}


def _valid(ops):
    kinds = [o.kind for o in ops]
    if not 10 <= len(ops) <= 14 or sum(k in OBS_KINDS for k in kinds) < 5:
        return False
    if set(o.args[0] for o in ops if o.kind in OBS_KINDS) != {'A', 'B'}:
        return False
    if tuple(ops[-2:]) != (op('eval', 'A'), op('eval', 'B')):
        return False
    for i, o in enumerate(ops):
        if o.kind in STEP_KINDS and (i == 0 or ops[i - 1].kind != 'train_step'):
            return False
        if o.kind in MUTATIONS and first_observer(ops, i) is None:
            return False
        if o.kind in MODE_CHANGES:
            later = [p.kind for p in ops[i + 1:]]
            if not (any(k in EVAL_KINDS for k in later) and any(k in TRAIN_KINDS for k in later)):
                return False
    return True


def random_sequence(seed, net=TINY_NET):
    """10 to 14 ops, a pure function of the seed: runs of observations, (mutation, observer) pairs drawn uniformly from PAIRS - a
    step is given the train_step it needs in front and is, three times in ten, two training iterations -, mode changes and
    value-preserving moves (an optimizer state round trip is followed by a step); at least 5 observations, both
    shapes, every mode change followed by an eval and a train kind, `eval(A), eval(B)` last.  Drawn again from the same stream
    until all of that holds."""
    if net.name not in _LAYERS:
        _LAYERS[net.name] = _layers(net)
    bn, cl, nconv = _LAYERS[net.name]
    rs = np.random.RandomState([4099, seed])
    pick = lambda xs: xs[int(rs.randint(len(xs)))]
    while True:
        n = int(rs.randint(10, 15)) - 2
        ops, frozen, bnk, stepped = [], 0, 0, False
        while len(ops) < n:
            room = n - len(ops)
            r = rs.rand()
            if r < 0.25:
                ops.append(op(pick(OBS_KINDS), pick('AB')))
            elif r < 0.72 and room >= 2:
                mk, ok = pick(PAIRS)
                S = pick('AB')
                if mk in STEP_KINDS:
                    if not (ops and ops[-1].kind == 'train_step'):
                        if room < 3:
                            continue
                        ops.append(op('train_step', pick('AB')))
                    ops.append(op(mk))
                    if rs.rand() < 0.3 and n - len(ops) >= 3:      # two training iterations in a row
                        ops += [op('train_step', pick('AB')), op(mk)]
                    stepped = stepped or mk != 'torch_step'
                elif mk == 'load_weights':
                    ops.append(op(mk, int(rs.randint(10, 100))))
                elif mk == 'perturb_running':
                    j = pick(bn)
                    if ok in TRAIN_KINDS and not j < bnk:
                        if bnk == 0:
                            ok = pick(EVAL_KINDS)
                        else:
                            j = pick([b for b in bn if b < bnk])
                    ops.append(op(mk, j))
                elif mk in ('perturb_gamma', 'perturb_beta'):
                    ops.append(op(mk, pick(bn)))
                else:
                    ops.append(op(mk, int(rs.randint(nconv))))
                ops.append(op(ok, S))
            elif r < 0.87:
                choices = ['freeze_prefix', 'bn_eval_prefix'] + (['unfreeze'] if frozen else []) + (['bn_train_all'] if bnk else [])
                mk = pick(choices)
                if mk == 'freeze_prefix':
                    frozen = int(rs.randint(1, nconv))          # (the head stays trainable)
                    ops.append(op(mk, frozen))
                elif mk == 'bn_eval_prefix':
                    bnk = int(rs.randint(1, nconv))
                    ops.append(op(mk, bnk))
                else:
                    frozen, bnk = (0, bnk) if mk == 'unfreeze' else (frozen, 0)
                    ops.append(op(mk))
            else:
                mk = pick(PRESERVING if stepped else PRESERVING[:2])
                ops.append(op(mk, pick(cl)) if mk == 'relayout' else op(mk))
                if mk == 'opt_state_roundtrip' and n - len(ops) >= 3:      # a resumed optimizer goes on stepping
                    ops += [op('train_step', pick('AB')), op(pick(STEP_KINDS[:2])), op(pick(OBS_KINDS), pick('AB'))]
        ops = tuple(ops) + (op('eval', 'A'), op('eval', 'B'))
        if _valid(ops):
            return ops


# How GEN_SEEDS was chosen: greedily from seeds 0..999.  Each round takes the seed whose sequence removes the most of what
# tests/test_sequences_cpu.py still counts as missing after the hand-written sequences and the seeds taken so far (a PAIRS entry
# seen fewer than twice, an ordered pair of observation kinds not yet adjacent, a layout transition not yet made, a HISTORY
# entry no generated sequence has), lowest seed
# first among equals; a seed whose sequence fails the visibility (>= 1e-2) or tameness condition on the reference is passed
# over (none of the 24 taken needed that).  The 24th seed closed the last gap.  (tests/sequence_cases.py::choose_seeds redoes
# the choice.)
GEN_SEEDS = (296, 50, 129, 197, 297, 60, 168, 434, 547, 12, 57, 248, 378, 566, 760, 777, 864, 21, 110, 16, 216, 581, 650, 0)


# what a step's history adds to the coverage count - over the GENERATED sequences alone, the hand-written ones were written with
# these in mind: a step that stays in the layout the optimizer has adopted (the validity checks pass: nothing moves, only the
# weights epoch tells the plans), first seen by an eval kind; and the first step of an optimizer that loaded momentum
HISTORY = (('stay', 'whole', 'eval'), ('stay', 'table', 'eval'), ('resume', 'whole'), ('resume', 'table'))


def coverage_needs(seqs):
    """What the coverage conditions still miss over `seqs`: {('pair', m, o): count short of 2, ('adj', a, b): 1,
    ('layout', a, b): 1, a HISTORY entry: 1}."""
    need = {}
    for p in PAIRS:
        need[('pair',) + p] = 2
    for a in OBS_KINDS:
        for b in OBS_KINDS:
            need[('adj', a, b)] = 1
    for a in LAYOUTS:
        for b in LAYOUTS:
            if a != b:
                need[('layout', a, b)] = 1
    for h in HISTORY:
        need[h] = 1
    for s in seqs:
        for item in coverage_items(s.ops):
            if need.get(item, 0) > 0 and (item not in HISTORY or s.id.startswith('gen')):
                need[item] -= 1
    return {k: v for k, v in need.items() if v > 0}


def step_layouts(net, ops):
    """[(kind, layout, resumed)] of every step and optimizer round trip of the sequence (no forward runs: the prediction needs
    the frozen set and the momentum state only - zero gradients stand in for the real ones)."""
    side = RefSide(net)
    for pos, o in enumerate(ops):
        if o.kind in OBS_KINDS or o.kind in GUARDS:
            side.zero_grad()
            if o.kind in GRAD_KINDS or o.kind == 'backward_across_shapes':
                for _, p in side.named():
                    if p.requires_grad:
                        p.grad = torch.zeros_like(p)
        elif o.kind in STEP_KINDS or o.kind in ('freeze_prefix', 'unfreeze', 'opt_state_roundtrip'):
            side.apply(o, pos)
    return side.step_log


_ITEMS = {}


def coverage_items(ops, net=TINY_NET):
    if (net.name, ops) in _ITEMS:
        return _ITEMS[(net.name, ops)]
    items = []
    for i, o in enumerate(ops):
        if o.kind in MUTATIONS:
            j = first_observer(ops, i)
            if j is not None:
                items.append(('pair', o.kind, ops[j].kind))
        if i and o.kind in OBS_KINDS and ops[i - 1].kind in OBS_KINDS:
            items.append(('adj', ops[i - 1].kind, o.kind))
    if any(o.kind in STEP_KINDS for o in ops):
        log = step_layouts(net, ops)
        items += [('layout', a, b) for a, b in layout_transitions([l for _, l, _ in log if l is not None])]
        where = [i for i, o in enumerate(ops) if o.kind in STEP_KINDS or o.kind == 'opt_state_roundtrip']
        last = None          # layout of the product optimizer's previous step, None after a round trip
        for i, (kind, layout, resumed) in zip(where, log):
            if kind == 'opt_state_roundtrip':
                last = None
            elif kind != 'torch_step':
                j = first_observer(ops, i)
                if layout == last and layout != 'per_param' and j is not None:
                    items.append(('stay', layout, 'eval' if ops[j].kind in EVAL_KINDS else 'train'))
                if resumed and layout != 'per_param':
                    items.append(('resume', layout))
                last = layout
    _ITEMS[(net.name, ops)] = items
    return items


def choose_seeds(ok, n=24, pool=1000):
    """ok(ops) -> bool: the reference conditions (visibility, tameness) of one sequence."""
    chosen, seqs = [], list(HAND)
    cands = {s: random_sequence(s) for s in range(pool)}
    items = {s: coverage_items(cands[s]) for s in range(pool)}
    bad = set()
    while len(chosen) < n:
        need = coverage_needs(seqs)
        best, gain = None, -1
        for s in range(pool):
            if s in chosen or s in bad:
                continue
            left = dict(need)
            g = 0
            for item in items[s]:
                if left.get(item, 0) > 0:
                    left[item] -= 1
                    g += 1
            if g > gain:
                best, gain = s, g
            if not need:
                break
        if not ok(cands[best]):
            bad.add(best)
            continue
        chosen.append(best)
        seqs.append(Seq('gen%03d' % best, cands[best]))
    return tuple(chosen), coverage_needs(seqs)


GEN = [Seq('gen%03d' % s, random_sequence(s)) for s in GEN_SEEDS]
ALL = HAND + GEN


# ------------------------------------------------------------------------------------------------ a net with a strided block
# topology case s2_bn_pair_producer-0: conv 8 -> 3x3 stride-2 BatchNorm conv 16 (ordinal 1 = mid) -> conv 16 -> head, shapes
# 2 x 16 x 16 and 1 x 24 x 24.  The strided block's packed forward filter and its data-gradient operand sit behind the same
# version keys as every other block's; the hand-written sequences write its filter in place, relayout it and freeze it
# (kfreeze = 2), and three generated ones: the first seed whose sequence on this net writes the filter of ordinal 1 in place
# (perturb_w / perturb_w_data), the first with a load_weights between two training steps (the data-gradient operand is
# packed again from the loaded filter), and the first that writes that filter after a relayout(1) and then takes two
# fused steps in front of an eval (a relayouted filter is not the forward operand: it is packed, behind the version key),
# all passing the visibility and tameness conditions of tests/test_sequences_cpu.py
STRIDED_NET = case_net(T.CASES['s2_bn_pair_producer-0'], 1, 2)
STRIDED_GEN_SEEDS = (12, 8, 212)


def strided_sequences():
    return [s for s in hand_sequences(STRIDED_NET) if s.id in TUNED_HAND] + \
        [Seq('gen%03d' % s, random_sequence(s, STRIDED_NET)) for s in STRIDED_GEN_SEEDS]

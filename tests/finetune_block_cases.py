"""Shared data of the fine-tuning tests on stride-2, depthwise and upsample blocks (tests/test_finetune_blocks_cpu.py,
tests/test_gpu_finetune_blocks.py): four small float nets and two exact-integer twins as cfg text, the fine-tuning patterns
each of them runs (which parameters are trainable, which BatchNorm modules are in eval(), whether the input wants a
gradient), a float64 / float32 torch reference that is a plain function of the parameters and takes the BatchNorm mode PER
LAYER, the data seeds, and the backward schedule and launch counts restated from the cfg alone.  Nothing here touches a GPU
or imports anything from oracle/.

A pattern is (own, bn_train, want_input): own = {conv layer: (weight, bias, gamma, beta) trainable}, bn_train = {conv layer:
its BatchNorm normalises with batch statistics}.  An eval-mode BatchNorm changes the function, so the reference and the data
seed belong to (net, BatchNorm modes); which parameters are frozen changes only which gradients are asked for.

Float patterns carry a data seed (SEEDS, found here on the CPU with find_seed) under which every leaky / relu sign and every
max-pool winner of the float64 reference keeps the margin tests/topology_cases.py demands (4x the float32-against-float64
forward difference), evaluated on the training forward under the pattern's own modes.  The exact twins have no BatchNorm,
integer data and parameters in {-1, 0, 1} with every partial sum below 2^24 (exact_budget): fp32 in any order is exact.
"""
import collections
import functools

import torch
import torch.nn.functional as F

import depthwise_cases as D
import topology_cases as T
import upsample_cases as U

conv, pool, route, head, dw, up = T.conv, T.pool, T.route, T.head, D.dw, U.up


def s2(f, k=3, bn=1, act='leaky'):
    return T.conv(f, k, bn, act, 2)


# ------------------------------------------------------------------------------------------------ nets
# 0 conv 8, 32x24 | 1 conv 16 / 2, 16x12 | 2 dw 16 | 3 1x1 16 | 4 dw 16 / 2, 8x6 | 5 1x1 16 | 6 upsample, 16x12 (writes into 7) |
# 7 route 6, 3 | 8 conv 16 | 9 head
FT_MIX = T.Case('ft_mix', 'ft', conv(8) + s2(16) + dw(16) + conv(16, 1) + dw(16, stride=2) + conv(16, 1) + up() + route(-1, 3) +
                conv(16) + head(8), 2, 32, 24, 3, 41)
# 0 conv 8 | 1 conv 8 | 2 route 0 | 3 pool, 8x8 | 4 conv 8 | 5 upsample, 16x16 (writes into 6) | 6 route 5, 1 | 7 conv 8 | 8 head.
# Layer 1, the route's second source, is no ancestor of the upsample: the concat can be one-sided in either direction.
FT_TWO_BRANCH = T.Case('ft_two_branch', 'ft', conv(8) + conv(8) + route(-2) + pool() + conv(8) + up() + route(-1, 1) + conv(8) +
                       head(8), 2, 16, 16, 3, 42)
# 26x22 -> 13x11 -> 7x6 -> 4x3: odd maps; block 5 reads a padded 18-channel map and has 3 * 4 * 3 = 36 pixels for BatchNorm
FT_S2_ODD = T.Case('ft_s2_odd', 'ft', conv(8) + s2(16) + conv(16, 1) + s2(16, 1) + conv(18, 3) + s2(16, 3, 1, 'relu') + head(8),
                   3, 26, 22, 3, 43)
# both depthwise blocks are pooled (2, 4 fused): neither can take the one-launch affine form
FT_DW_POOL = T.Case('ft_dw_pool', 'ft', conv(8) + dw(8) + pool() + dw(8, stride=2) + pool() + conv(16, 1) + head(8), 2, 32, 32, 3, 44)
# the exact twins: no BatchNorm, relu / linear, topology_cases.init_params' exact family, integer data
FTX_MIX = T.Case('ftx_mix', 'exact', conv(8, 3, 0, 'relu') + s2(16, 3, 0, 'linear') + dw(16, 0, 'relu') + conv(16, 1, 0, 'linear') +
                 dw(16, 0, 'linear', stride=2) + conv(16, 1, 0, 'relu') + up() + route(-1, 3) + conv(16, 3, 0, 'linear') + head(8),
                 2, 32, 24, 3, 51)
FTX_TWO_BRANCH = T.Case('ftx_two_branch', 'exact', conv(8, 3, 0, 'relu') + conv(8, 3, 0, 'linear') + route(-2) + pool() +
                        conv(8, 3, 0, 'linear') + up() + route(-1, 1) + conv(8, 3, 0, 'relu') + head(8), 2, 16, 16, 3, 52)

FLOAT = [FT_MIX, FT_S2_ODD, FT_DW_POOL, FT_TWO_BRANCH]
EXACT = [FTX_MIX, FTX_TWO_BRANCH]
NETS = FLOAT + EXACT
CASES = {c.id: c for c in NETS}

# what a plan records for each net, written out by hand: the conv layers, Plan.depthwise, Plan.upsample, Plan.fused_pool and
# the (consumer <- source) pairs of _plan_bn_fusion.  A depthwise or a stride-2 block is never the consumer of a pair; either
# may be its source.
PLANS = {
    'ft_mix': dict(convs=[0, 1, 2, 3, 4, 5, 8, 9], depthwise=[2, 4], upsample={6: 'route'}, fused_pool=set(),
                   bn_pairs={3: 2, 5: 4, 9: 8}),
    'ft_two_branch': dict(convs=[0, 1, 4, 7, 8], depthwise=[], upsample={5: 'route'}, fused_pool=set(), bn_pairs={8: 7}),
    'ft_s2_odd': dict(convs=[0, 1, 2, 3, 4, 5, 6], depthwise=[], upsample={}, fused_pool=set(), bn_pairs={2: 1, 4: 3, 6: 5}),
    'ft_dw_pool': dict(convs=[0, 1, 3, 5, 6], depthwise=[1, 3], upsample={}, fused_pool={2, 4}, bn_pairs={6: 5}),
    'ftx_mix': dict(convs=[0, 1, 2, 3, 4, 5, 8, 9], depthwise=[2, 4], upsample={6: 'route'}, fused_pool=set(), bn_pairs={}),
    'ftx_two_branch': dict(convs=[0, 1, 4, 7, 8], depthwise=[], upsample={5: 'route'}, fused_pool=set(), bn_pairs={}),
}


# ------------------------------------------------------------------------------------------------ patterns
Pattern = collections.namedtuple('Pattern', 'id own bn_train want_input')
KINDS = ('weight', 'bias', 'gamma', 'beta')


def conv_layers(case):
    """{conv layer: it has a BatchNorm} from the cfg (a BatchNorm block has no bias, any other block has one)."""
    return {i: bool(int(b['batch_normalize'])) for i, b in enumerate(T.blocks_of(case)[1:]) if b['type'] == 'convolutional'}


def _pattern(case, name, trainable, bn_training, want_input=False):
    """trainable(layer, kind) -> bool, bn_training(layer) -> bool, asked only about what exists."""
    own, modes = {}, {}
    for i, bn in conv_layers(case).items():
        exists = (True, not bn, bn, bn)
        own[i] = tuple(bool(e and trainable(i, k)) for e, k in zip(exists, KINDS))
        modes[i] = bool(bn and bn_training(i))
    return Pattern(name + ('+input' if want_input else ''), own, modes, bool(want_input))


def prefix_eval(case, k, want_input=False):
    """The convs before k frozen, their BatchNorm in eval().  (On an exact net: the convs before k frozen.)"""
    return _pattern(case, ('prefix-%d' if T.is_exact(case) else 'prefix-eval-%d') % k, lambda i, kind: i >= k, lambda i: i >= k,
                    want_input)


def bn_eval(case, k, want_input=False):
    """The BatchNorm of the convs before k in eval(), everything trainable."""
    return _pattern(case, 'bn-eval-%d' % k, lambda i, kind: True, lambda i: i >= k, want_input)


def sandwich(case, k):
    """Conv k alone frozen, with its BatchNorm in eval()."""
    return _pattern(case, 'sandwich-%d' % k, lambda i, kind: i != k, lambda i: i != k)


def bn_only(case):
    """Only gammas and betas trainable, every module in training mode."""
    return _pattern(case, 'bn-only', lambda i, kind: kind in ('gamma', 'beta'), lambda i: True)


def branch(case, layers):
    """Exactly the convs in `layers` trainable, every other BatchNorm in eval()."""
    return _pattern(case, 'branch-' + '-'.join(str(l) for l in sorted(layers)), lambda i, kind: i in layers, lambda i: i in layers)


def everything(case, want_input=False):
    return _pattern(case, 'all', lambda i, kind: True, lambda i: True, want_input)


def input_only(case):
    return _pattern(case, 'none', lambda i, kind: False, lambda i: True, True)


TABLE = {
    'ft_mix': [prefix_eval(FT_MIX, k) for k in (2, 3, 5, 8)] + [bn_eval(FT_MIX, 5, True)] +
              [sandwich(FT_MIX, k) for k in (1, 2, 4)] + [bn_only(FT_MIX)],
    'ft_s2_odd': [prefix_eval(FT_S2_ODD, k) for k in (2, 4)] + [bn_eval(FT_S2_ODD, 6, True)] +
                 [sandwich(FT_S2_ODD, k) for k in (3, 5)] + [bn_only(FT_S2_ODD)],
    'ft_dw_pool': [prefix_eval(FT_DW_POOL, k) for k in (3, 5)] + [bn_eval(FT_DW_POOL, 5, True)] +
                  [sandwich(FT_DW_POOL, k) for k in (1, 3)],
    'ft_two_branch': [branch(FT_TWO_BRANCH, {1, 7, 8}), branch(FT_TWO_BRANCH, {4, 7, 8}), prefix_eval(FT_TWO_BRANCH, 4),
                      bn_eval(FT_TWO_BRANCH, 7)],
    'ftx_mix': [prefix_eval(FTX_MIX, k) for k in (2, 3, 5, 8)] + [sandwich(FTX_MIX, k) for k in (2, 4)] + [everything(FTX_MIX, True)],
    'ftx_two_branch': [branch(FTX_TWO_BRANCH, {1, 7, 8}), branch(FTX_TWO_BRANCH, {4, 7, 8}), prefix_eval(FTX_TWO_BRANCH, 4),
                       everything(FTX_TWO_BRANCH, True)],
}
FLOAT_PATTERNS = [(c, p) for c in FLOAT for p in TABLE[c.id]]
EXACT_PATTERNS = [(c, p) for c in EXACT for p in TABLE[c.id]]


def pattern(case, pid):
    return next(p for p in TABLE[case.id] if p.id == pid)


def pid(cp):
    return '%s-%s' % (cp[0].id, cp[1].id)


# data seeds: find_seed(case, pattern.bn_train) on the CPU (test_finetune_blocks_cpu.py re-checks the margins under them).
# The exact twins run at data seed 0, where exact_budget is stated.
SEEDS = {
    ('ft_mix', 'prefix-eval-2'): 0, ('ft_mix', 'prefix-eval-3'): 0, ('ft_mix', 'prefix-eval-5'): 2,
    ('ft_mix', 'prefix-eval-8'): 1, ('ft_mix', 'bn-eval-5+input'): 2, ('ft_mix', 'sandwich-1'): 1,
    ('ft_mix', 'sandwich-2'): 0, ('ft_mix', 'sandwich-4'): 0, ('ft_mix', 'bn-only'): 0,
    ('ft_s2_odd', 'prefix-eval-2'): 1, ('ft_s2_odd', 'prefix-eval-4'): 0, ('ft_s2_odd', 'bn-eval-6+input'): 0,
    ('ft_s2_odd', 'sandwich-3'): 0, ('ft_s2_odd', 'sandwich-5'): 0, ('ft_s2_odd', 'bn-only'): 0,
    ('ft_dw_pool', 'prefix-eval-3'): 4, ('ft_dw_pool', 'prefix-eval-5'): 4, ('ft_dw_pool', 'bn-eval-5+input'): 4,
    ('ft_dw_pool', 'sandwich-1'): 4, ('ft_dw_pool', 'sandwich-3'): 2,
    ('ft_two_branch', 'branch-1-7-8'): 0, ('ft_two_branch', 'branch-4-7-8'): 0, ('ft_two_branch', 'prefix-eval-4'): 0,
    ('ft_two_branch', 'bn-eval-7'): 0,
}
XSEED = 0


def seed_of(case, pat):
    return XSEED if T.is_exact(case) else SEEDS[case.id, pat.id]


make_model, make_input, make_probe = T.make_model, T.make_input, T.make_probe


def param_key(name):
    """'<layer>.<child>.<weight|bias>' of model.models.named_parameters() -> (conv layer, index into KINDS)."""
    layer, child, what = name.split('.')
    return int(layer), (2 if what == 'weight' else 3) if child.startswith('bn') else (0 if what == 'weight' else 1)


def trainable(pat, name):
    layer, kind = param_key(name)
    return pat.own[layer][kind]


def apply_pattern(model, pat):
    """model.train(), then each BatchNorm module in the pattern's mode and each parameter's requires_grad."""
    model.train()
    for ind, seq in enumerate(model.models):
        for m in seq.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.train(pat.bn_train[ind])
    for n, p in model.models.named_parameters():
        p.requires_grad_(trainable(pat, n))
    return model


# ------------------------------------------------------------------------------------------------ float64 / float32 reference
def _tap(taps, kind, ind, x):
    if taps is not None:
        taps.setdefault(kind, {})[ind] = x.detach().clone()


def ref_forward(blocks, names, params, bufs, x, bn_train, taps=None, absnet=False):
    """The net as a function of its parameters.  blocks: the parsed cfg; names[ind]: the child names of block ind's
    nn.Sequential ('conv3', 'bn3', ...); params / bufs: {state_dict key without 'models.': tensor} (the running statistics of
    a training-mode BatchNorm are updated in place); bn_train: {conv layer: batch statistics} or one bool for all.  Stride,
    pad and groups come from the cfg; an [upsample] replicates each pixel stride x stride times.  Returns (y, {layer: output}).
    absnet: the magnitude network of exact_budget (the caller passes |parameters| and |x|; identity activations, a max-pool
    whose backward hands the gradient to the whole window)."""
    outs = {}
    for ind, b in enumerate(blocks[1:]):
        t = b['type']
        if t == 'convolutional':
            cn = names[ind][0]
            k, s, groups = int(b['size']), int(b['stride']), int(b.get('groups', 1))
            w, bias = params['%d.%s.weight' % (ind, cn)], params.get('%d.%s.bias' % (ind, cn))
            assert tuple(w.shape[1:]) == (x.shape[1] // groups, k, k), (ind, tuple(w.shape))
            if k == 1 and s > 1:
                # the same convolution on the pixels it reads (topology_cases.ref_run: torch's float32 CPU backward of a strided
                # 1x1 convolution is not to be trusted on some shapes)
                x, s = x[:, :, ::s, ::s], 1
            x = F.conv2d(x, w, bias, stride=s, padding=(k - 1) // 2 if int(b['pad']) else 0, groups=groups)
            if int(b['batch_normalize']):
                bn = '%d.%s.' % (ind, names[ind][1])
                mode = bn_train[ind] if isinstance(bn_train, dict) else bool(bn_train)
                x = F.batch_norm(x, bufs[bn + 'running_mean'], bufs[bn + 'running_var'], params[bn + 'weight'],
                                 params[bn + 'bias'], mode, 0.1, 1e-4)
            if b['activation'] in ('leaky', 'relu'):
                _tap(taps, 'pre', ind, x)
                if not absnet:
                    x = F.leaky_relu(x, 0.1) if b['activation'] == 'leaky' else F.relu(x)
            else:
                assert b['activation'] == 'linear'
        elif t == 'maxpool':
            assert int(b['size']) == 2 and int(b['stride']) == 2
            _tap(taps, 'pool', ind, x)
            y = F.max_pool2d(x, 2, 2)
            if absnet:
                sm = F.avg_pool2d(x, 2, 2) * 4
                y = y.detach() + (sm - sm.detach())
            x = y
        elif t == 'upsample':
            n = int(b.get('stride', 2))
            x = x.repeat_interleave(n, 2).repeat_interleave(n, 3)
        elif t == 'route':
            ls = T._resolve(b['layers'], ind)
            x = outs[ls[0]] if len(ls) == 1 else torch.cat([outs[l] for l in ls], 1)
        elif t == 'shortcut':
            assert b['activation'] == 'linear'
            x = outs[T._resolve(b['from'], ind)[0]] + outs[ind - 1]
        elif t == 'region':
            continue
        else:
            raise AssertionError(t)
        outs[ind] = x
    return x, outs


def model_state(model, dtype):
    """(names, params, bufs) of ref_forward from a Darknet module tree: detached copies in dtype, parameters wanting gradients."""
    names = {ind: [n for n, _ in m.named_children()] for ind, m in enumerate(model.models)}
    params = {n: p.detach().cpu().to(dtype).clone().requires_grad_(True) for n, p in model.models.named_parameters()}
    bufs = {n: b.detach().cpu().to(dtype).clone() for n, b in model.models.named_buffers() if 'running' in n}
    return names, params, bufs


Ref = collections.namedtuple('Ref', 'y dx grads stats')


def run_ref(model, x, probe, dtype, bn_train, taps=None):
    """Training output, dL/dx, the gradient of EVERY parameter of (y * probe).sum() and the running statistics after that
    forward, for `model` (any Darknet tree on the CPU; its own modes and requires_grad flags are not read) on input x with
    the BatchNorm modes bn_train.  probe None: the forward alone (dx and grads are None)."""
    names, params, bufs = model_state(model, dtype)
    xr = x.to(dtype).requires_grad_(True)
    y, _ = ref_forward(model.blocks, names, params, bufs, xr, bn_train, taps)
    stats = {'models.' + n: b for n, b in bufs.items()}
    if probe is None:
        return Ref(y.detach(), None, None, stats)
    (y * probe.to(dtype)).sum().backward()
    grads = {'models.' + n: (None if p.grad is None else p.grad.detach()) for n, p in params.items()}
    return Ref(y.detach(), xr.grad.detach(), grads, stats)


def _modes_key(bn_train):
    return tuple(sorted(bn_train.items()))


def _one_ref(model, case, dseed, dtype, bn_train, taps=None):
    x = make_input(case, dseed)
    shape = run_ref(model, x, None, dtype, bn_train).y.shape
    return run_ref(model, x, make_probe(case, dseed, shape), dtype, bn_train, taps)


@functools.lru_cache(maxsize=None)
def _reference(case, modes, dseed):
    model = make_model(case)
    return _one_ref(model, case, dseed, torch.float64, dict(modes)), _one_ref(model, case, dseed, torch.float32, dict(modes))


def reference(case, pat, dseed=None):
    """(float64 run, float32 run) of a net under a pattern's BatchNorm modes, at the pattern's data seed.  Computed once per
    (net, modes, seed), shared, never written."""
    return _reference(case, _modes_key(pat.bn_train), seed_of(case, pat) if dseed is None else dseed)


def margins(case, bn_train, dseed):
    """topology_cases.margins on this module's reference, on the training forward under bn_train: (smallest decision
    margin, largest float32-against-float64 forward difference), relative to their layer's largest magnitude."""
    model = make_model(case)
    t64, t32 = {}, {}
    _one_ref(model, case, dseed, torch.float64, bn_train, t64)
    _one_ref(model, case, dseed, torch.float32, bn_train, t32)
    margin, diff = float('inf'), 0.0
    for kind in t64:
        for ind, a in t64[kind].items():
            top = max(float(a.abs().max()), 1e-300)
            diff = max(diff, float((a - t32[kind][ind].double()).abs().max()) / top)
            if kind == 'pre':
                z = a[(a != 0) | (t32[kind][ind] != 0)]
                if z.numel():
                    margin = min(margin, float(z.abs().min()) / top)
            else:
                v = T._windows(a, 2).sort(dim=-1, descending=True)[0]
                gap = v[..., :1] - v[..., 1:]
                gap = gap[gap > 0]
                if gap.numel():
                    margin = min(margin, float(gap.min()) / top)
    return margin, diff


@functools.lru_cache(maxsize=None)
def _margin_ok(case, modes, dseed):
    m, d = margins(case, dict(modes), dseed)
    return m >= 4.0 * d


def margin_ok(case, bn_train, dseed):
    return _margin_ok(case, _modes_key(bn_train), dseed)


def find_seed(case, bn_train):
    for s in range(8):
        if margin_ok(case, bn_train, s):
            return s
    return None


def exact_budget(case, dseed=0):
    """Largest magnitude any activation, gradient or filter-gradient partial sum of an exact net can reach in any summation
    order: the magnitude network forward and backward (the upsample's backward window sum is part of it: the magnitude
    network's gradient of the coarse map is the sum of the window's magnitudes)."""
    model = make_model(case)
    names, params, bufs = model_state(model, torch.float64)
    for p in params.values():
        p.data.abs_()
    x = make_input(case, dseed).abs().double().requires_grad_(True)
    y, outs = ref_forward(model.blocks, names, params, bufs, x, False, absnet=True)
    for o in outs.values():
        if o.requires_grad and not o.is_leaf:
            o.retain_grad()
    (y * make_probe(case, dseed, y.shape).abs().double()).sum().backward()
    return max([float(x.grad.abs().max()), float(x.detach().abs().max())] +
               [float(o.detach().abs().max()) for o in outs.values()] +
               [float(o.grad.abs().max()) for o in outs.values() if o.grad is not None] +
               [float(p.grad.abs().max()) for p in params.values() if p.grad is not None])


# ------------------------------------------------------------------------------------------------ the schedule, restated
def expected(case, pat):
    """Per layer of the cfg what a backward under the pattern runs (test_finetune_cpu._expected: visited, data gradient per
    source, wgrad / bias / dgamma / dbeta / bn_reduce / fold_bn), with the BatchNorm pairs of PLANS: an [upsample] reads
    the previous layer, a depthwise or stride-2 block is never the consumer of a pair."""
    from test_finetune_cpu import _expected
    return _expected(T.blocks_of(case), case.B, case.H, case.W, pat.own, pat.want_input, pat.bn_train,
                     fuse=PLANS[case.id]['bn_pairs'])


def _block_kind(b):
    """'dw' (csrc/conv_depthwise.hip), 's2' (csrc/conv_strided.hip) or 'dense' of a [convolutional] block."""
    if int(b.get('groups', 1)) > 1:
        return 'dw'
    return 's2' if int(b['stride']) == 2 else 'dense'


def forward_forms(case, pat):
    """{conv layer: 'affine' | 'raw'} of a forward under model.train(): a block no backward visits, with its BatchNorm in
    eval(), un-pooled and with unpadded channels, is ONE launch with the running-statistics affine and the activation in its
    epilogue; every other block writes its raw output (and, in eval mode, applies the affine in ssp_bn_act_fwd)."""
    exp = expected(case, pat)
    out = {}
    for i, b in enumerate(T.blocks_of(case)[1:]):
        if b['type'] == 'convolutional':
            bn = bool(int(b['batch_normalize']))
            out[i] = 'affine' if (bn and not pat.bn_train[i] and not exp[i]['visited'] and (i + 1) not in PLANS[case.id]['fused_pool']
                                  and int(b['filters']) % 4 == 0) else 'raw'
    return out


def expected_launches(case, pat):
    """Launch counts of one training step under the pattern, from the restated schedule: the backward launches of the three
    block families, the BatchNorm / activation backward in its two forms, the statistics finalize of the forward, and the
    forward launch of each family in its two forms."""
    exp, forms = expected(case, pat), forward_forms(case, pat)
    n = collections.Counter()
    for i, b in enumerate(T.blocks_of(case)[1:]):
        e = exp[i]
        if b['type'] == 'upsample':
            n['ssp_upsample_bwd'] += int(e['visited'] and e['dgrad'][0])
        if b['type'] != 'convolutional':
            continue
        kind, bn = _block_kind(b), bool(int(b['batch_normalize']))
        n['ssp_bn_fwd_finalize'] += int(bn and pat.bn_train[i])
        fwd = {'dw': 'ssp_dwconv_fwd', 's2': 'ssp_conv_s2_fwd', 'dense': 'ssp_conv_fwd'}[kind]
        n[fwd + ('_affine' if forms[i] == 'affine' else '')] += 1
        if not e['visited']:
            continue
        if kind != 'dense':
            stem = 'ssp_dwconv_' if kind == 'dw' else 'ssp_conv_s2_'
            n[stem + 'wgrad'] += int(e['wgrad'])
            n[stem + 'dgrad'] += int(e['dgrad'][0])
        if bn or b['activation'] != 'linear':
            n['ssp_bn_act_bwd_affine' if bn and not e['bn_reduce'] else 'ssp_bn_act_bwd(+_partials)'] += 1
    return n


COUNTED = ('ssp_dwconv_wgrad', 'ssp_dwconv_dgrad', 'ssp_conv_s2_wgrad', 'ssp_conv_s2_dgrad', 'ssp_upsample_bwd',
           'ssp_bn_fwd_finalize', 'ssp_bn_act_bwd_affine', 'ssp_bn_act_bwd(+_partials)', 'ssp_dwconv_fwd', 'ssp_dwconv_fwd_affine',
           'ssp_conv_s2_fwd', 'ssp_conv_s2_fwd_affine', 'ssp_conv_fwd', 'ssp_conv_fwd_affine')


def counted(log):
    """The same counter from a recorded launch log (exact names)."""
    n = collections.Counter()
    for name in log:
        if name in ('ssp_bn_act_bwd', 'ssp_bn_act_bwd_partials'):
            n['ssp_bn_act_bwd(+_partials)'] += 1
        elif name in COUNTED:
            n[name] += 1
    return n

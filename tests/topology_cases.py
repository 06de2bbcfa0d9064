"""Small Darknet topologies for the execution plan (engine.Plan): hand-written and seeded random cfgs, a float64 CPU
restatement of the reference's block semantics (darknet.py:82-130), and `supported()` - which of them a plan must run and
which it must refuse when it is built.  Shared by tests/test_topology_cpu.py and tests/test_gpu_topology.py; nothing here
touches a GPU, and neither the reference forward nor `supported()` reads singleshotpose_amd.engine.

A case is a cfg body plus (B, H, W, channels) and a weight seed.  Three families:
  hand   one per line of Plan that the four shipped cfgs never reach (HAND_PROPS), three sizes each
  gen    random_cfg(seed): the block grammar with the constraints the reference itself has
  exact  the same grammar without BatchNorm / leaky / softmax, on integer data: every activation, gradient and
         filter-gradient partial sum is an integer (or a multiple of 1 / avgpool pixels) below 2^24 grid steps
         (exact_budget), so fp32 in any summation order is exact and the product must be torch.equal to float64
  gs2 / xs2  the gen and exact families with stride-2 convolutions in the grammar (random_case(seed, exact, strided=True)), on
         maps that are also odd
Float cases carry a data seed (SEEDS) under which every leaky / relu sign and every max-pool winner has a margin of at
least 4x the float32-against-float64 forward difference of the CPU reference: a flipped decision moves a gradient by far
more than rounding does, and the bars of the GPU test are rounding bars.
"""
import collections
import copy
import functools
import os
import tempfile
import zlib

import numpy as np
import torch
import torch.nn.functional as F

Case = collections.namedtuple('Case', 'id family body B H W channels wseed')


# ------------------------------------------------------------------------------------------------ cfg text
def conv(f, k=3, bn=1, act='leaky', stride=1):
    return '[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n' % (
        'batch_normalize=1\n' if bn else '', f, k, stride, act)


def pool(stride=2):
    return '[maxpool]\nsize=2\nstride=%d\n\n' % stride


def reorg():
    return '[reorg]\nstride=2\n\n'


def route(*layers):
    return '[route]\nlayers=%s\n\n' % ','.join(str(l) for l in layers)


def shortcut(frm, act='linear'):
    return '[shortcut]\nfrom=%d\nactivation=%s\n\n' % (frm, act)


def avgpool():
    return '[avgpool]\n\n'


def connected(out, act='linear'):
    return '[connected]\noutput=%d\nactivation=%s\n\n' % (out, act)


def softmax():
    return '[softmax]\ngroups=1\n\n'


def head(f=8):
    return conv(f, 1, 0, 'linear')


def cfg_text(case):
    return '[net]\nheight=%d\nwidth=%d\nchannels=%d\n\n' % (case.H, case.W, case.channels) + case.body


def parse(text):
    """cfg text -> [net] + block dicts (cfg.py:4-34 of the reference: every value a string, batch_normalize defaults to 0)."""
    blocks = []
    for line in text.splitlines():
        line = line.strip()
        if not line or line[0] == '#':
            continue
        if line[0] == '[':
            blocks.append({'type': line[1:-1]})
            if blocks[-1]['type'] == 'convolutional':
                blocks[-1]['batch_normalize'] = 0
        else:
            k, v = line.split('=')
            blocks[-1][k.strip()] = v.strip()
    return blocks


def blocks_of(case):
    return parse(cfg_text(case))


# ------------------------------------------------------------------------------------------------ cfg analysis
def _pad4(c):
    return (c + 3) // 4 * 4


def _resolve(spec, ind):
    return [int(i) if int(i) > 0 else int(i) + ind for i in str(spec).split(',')]


Layer = collections.namedtuple('Layer', 'type C H W ld srcs block')


def layer_info(blocks, H, W):
    """Per layer: output shape, the row stride an NHWC fp32 map of it has under the ABI (channel counts padded to 4; a
    concat and a reorg write exactly their channels; a pool and a one-layer route keep their source's), and the layers it
    reads (-1 = the network input; a shortcut reads `from` and the previous layer, in that order)."""
    c, h, w = int(blocks[0].get('channels', 3)), H, W
    ld = _pad4(c)
    out = []
    for ind, b in enumerate(blocks[1:]):
        t = b['type']
        srcs = [ind - 1]
        if t == 'convolutional':
            c = int(b['filters'])
            ld = _pad4(c)
            if int(b['stride']) == 2:      # nn.Conv2d(stride=2, padding=k // 2 with pad=1): odd maps round up
                k = int(b['size'])
                p = k // 2 if int(b['pad']) else 0
                h, w = (h + 2 * p - k) // 2 + 1, (w + 2 * p - k) // 2 + 1
        elif t == 'maxpool':
            if int(b['stride']) == 2:
                h, w = h // 2, w // 2
        elif t == 'reorg':
            c, h, w = 4 * c, h // 2, w // 2
            ld = c
        elif t == 'route':
            srcs = _resolve(b['layers'], ind)
            c = sum(out[l].C for l in srcs)
            h, w = out[srcs[0]].H, out[srcs[0]].W
            ld = out[srcs[0]].ld if len(srcs) == 1 else c
        elif t == 'shortcut':
            srcs = [_resolve(b['from'], ind)[0], ind - 1]
            ld = _pad4(c)
        elif t == 'avgpool':
            h, w, ld = 1, 1, _pad4(c)
        elif t == 'connected':
            c, h, w = int(b['output']), 1, 1
            ld = _pad4(c)
        elif t == 'softmax':
            ld = _pad4(c)
        out.append(Layer(t, c, h, w, ld, srcs, b))
    return out


def consumers_of(info):
    cons = [[] for _ in info]
    for ind, l in enumerate(info):
        for s in l.srcs:
            if s >= 0:
                cons[s].append(ind)
    return cons


def _is_bn(l):
    return l.type == 'convolutional' and int(l.block['batch_normalize']) != 0


def _is_s2(l):
    return l.type == 'convolutional' and int(l.block['stride']) == 2


def _in_shape(info, ind, blocks, H, W):
    if ind == 0:
        return int(blocks[0].get('channels', 3)), H, W, _pad4(int(blocks[0].get('channels', 3)))
    p = info[ind - 1]
    return p.C, p.H, p.W, p.ld


def supported(blocks, B, H, W):
    """[] when a plan must run this cfg, else [(class, block index), ...]: what the reference's semantics and the ABI
    (include/ssp_hip.h) rule out.  Classes: 'route3' a route of more than two layers (darknet.py:99-106 handles one or two),
    'route_first' a two-layer route whose first is not the previous layer (darknet.py:206), 'concat4' a concatenated map with
    C % 4 != 0 (ssp_copy_channels), 'odd' a standalone 2x2/2 max-pool or a reorg of a map with odd H or W (the network input's,
    or one a stride-2 conv made odd: 26 -> 13), 'last4' a network output with C % 4 != 0, 'narrow' a conv or connected block
    whose input rows are narrower than its padded Cin, 'reorg4' a reorg of a map with C % 4 != 0, 'first_s2' a stride-2 conv
    as block 0 (the first block's kernel family is stride 1 only; ssp_conv_s2_* serve every later position)."""
    info = layer_info(blocks, H, W)
    bad = []
    for ind, l in enumerate(info):
        c, h, w, ld = _in_shape(info, ind, blocks, H, W)
        if l.type == 'route':
            if len(l.srcs) > 2:
                bad.append(('route3', ind))
            elif len(l.srcs) == 2:
                if l.srcs[0] != ind - 1:
                    bad.append(('route_first', ind))
                if any(info[s].C % 4 for s in l.srcs):
                    bad.append(('concat4', ind))
        elif l.type == 'maxpool' and int(l.block['stride']) == 2 and (h % 2 or w % 2):
            bad.append(('odd', ind))      # (a pool folded into its BatchNorm block needs an even map as well)
        elif l.type == 'reorg':
            if h % 2 or w % 2:
                bad.append(('odd', ind))
            if c % 4:
                bad.append(('reorg4', ind))
        elif l.type in ('convolutional', 'connected'):
            if ld < _pad4(c):
                bad.append(('narrow', ind))
            if ind == 0 and _is_s2(l):
                bad.append(('first_s2', ind))
    last = max(i for i, l in enumerate(info) if l.type not in ('region', 'cost'))
    if info[last].C % 4:
        bad.append(('last4', last))
    return bad


def expected_fused_pool(blocks, B, H, W):
    """Pool layers a plan folds into the BatchNorm block in front of them: the block's only consumer, on an even map (the
    map the block WRITES: a stride-2 block's output, l.H x l.W of layer_info)."""
    info = layer_info(blocks, H, W)
    cons = consumers_of(info)
    return set(i + 1 for i, l in enumerate(info[:-1])
               if _is_bn(l) and info[i + 1].type == 'maxpool' and int(info[i + 1].block['stride']) == 2 and
               int(info[i + 1].block['size']) == 2 and cons[i] == [i + 1] and l.H % 2 == 0 and l.W % 2 == 0)


def expected_bn_fuse(blocks, B, H, W):
    """{consumer: source}: un-pooled BatchNorm blocks with unpadded channels whose only consumer is the conv / connected
    block right behind them (their BatchNorm-backward sums ride in that block's data-gradient launch).  A stride-2 block is
    never the consumer - its data gradient has no fused sums - but may be the source: the sums then run over its output map."""
    info = layer_info(blocks, H, W)
    cons = consumers_of(info)
    return {i + 1: i for i, l in enumerate(info[:-1])
            if _is_bn(l) and l.C % 4 == 0 and info[i + 1].type in ('convolutional', 'connected') and cons[i] == [i + 1] and
            not _is_s2(info[i + 1])}


def _bn_pair_but_for_stride(info, cons, i):
    """Layer i would be the source of a fused BatchNorm-backward pair if the block behind it were not a stride-2 conv."""
    l = info[i]
    return _is_bn(l) and l.C % 4 == 0 and i + 1 < len(info) and _is_s2(info[i + 1]) and cons[i] == [i + 1]


def _alias_root(info, i):
    """The layer whose buffer layer i is: one-layer routes followed back (-1 = the network input)."""
    while i >= 0 and info[i].type == 'route' and len(info[i].srcs) == 1:
        i = info[i].srcs[0]
    return i


def live_layers(info):
    """Layers with a path to the network output."""
    last = max(i for i, l in enumerate(info) if l.type not in ('region', 'cost'))
    live, todo = set(), [last]
    while todo:
        i = todo.pop()
        if i < 0 or i in live:
            continue
        live.add(i)
        todo += info[i].srcs
    return live


# the hand-written cases' properties: each names a line of Plan that the shipped cfgs never reach
HAND_PROPS = ('alias_pool_2cons', 'concat_src_shortcut_src', 'shortcut_m1_alias', 'dead_branch', 'reorg_alias_pool',
              'bn_pad_to_conv', 'bn_fuse_pair', 'channels1', 'softmax_map_conv', 'pool_after_relu_nobn', 'concat_same',
              'pool_not_fused_2cons',
              # ... and that no net with a stride-2 block reached before this table had one
              's2_after_pad', 's2_reads_concat', 's2_alias_two_s2_consumers', 's2_bn_pair_producer', 's2_bn_pair_not_consumer',
              's2_fused_pool', 's2_chain_odd', 's2_reorg_pool_s1', 's2_dead_and_head', 's2_classifier')
S2_GRAMMAR = ('conv3_s2', 'conv1_s2', 's2_bn', 's2_bias', 's2_odd_in', 's2_head', 's2_fused_pool')
GRAMMAR = S2_GRAMMAR + ('conv1', 'conv3', 'bn', 'bias', 'leaky', 'linear', 'relu', 'maxpool2', 'maxpool_s1', 'reorg', 'route1_rel',
           'route1_abs', 'route2', 'shortcut', 'shortcut_m1', 'shortcut_leaky', 'shortcut_linear', 'shortcut_relu', 'head',
           'classifier', 'connected2', 'softmax', 'B1', 'B2', 'B3', 'W16', 'Wnot16', 'first32_fused', 'first32_unfused',
           'channels1', 'channels3', 'pad_before_conv', 'fused_pool')


def features(blocks, B, H, W):
    info = layer_info(blocks, H, W)
    cons = consumers_of(info)
    fused = expected_fused_pool(blocks, B, H, W)
    f = set(['B%d' % B, 'W16' if W % 16 == 0 else 'Wnot16', 'channels%d' % int(blocks[0].get('channels', 3))])
    live = live_layers(info)
    for ind, l in enumerate(info):
        b, t = l.block, l.type
        nxt = info[ind + 1] if ind + 1 < len(info) else None
        if t == 'convolutional':
            f.add('conv%s' % b['size'])
            f.add('bn' if _is_bn(l) else 'bias')
            f.add(b['activation'])
            if ind == 0 and _is_bn(l) and l.C == 32 and b['size'] == '3' and 1 in fused:
                f.add('first32_fused' if W % 16 == 0 else 'first32_unfused')
            if ind == len(info) - 1 and not _is_bn(l) and b['activation'] == 'linear':
                f.add('head')
            if nxt is not None and nxt.type == 'convolutional' and l.C % 4:
                f.add('pad_before_conv')
                if _is_bn(l) and cons[ind] == [ind + 1]:
                    f.add('bn_pad_to_conv')
            if (not _is_bn(l) and b['activation'] == 'relu' and nxt is not None and nxt.type == 'maxpool' and
                    nxt.block['stride'] == '2'):
                f.add('pool_after_relu_nobn')
            if ind not in live:
                f.add('dead_branch')
            if (_is_bn(l) and nxt is not None and nxt.type == 'maxpool' and nxt.block['stride'] == '2' and
                    l.H % 2 == 0 and l.W % 2 == 0 and len(cons[ind]) >= 2):
                f.add('pool_not_fused_2cons')
            if _is_s2(l):
                _, hi, wi, _ = _in_shape(info, ind, blocks, H, W)
                prev = info[ind - 1] if ind > 0 else None
                f.add('conv%s_s2' % b['size'])
                f.add('s2_bn' if _is_bn(l) else 's2_bias')
                if hi % 2 or wi % 2:
                    f.add('s2_odd_in')
                if ind == len(info) - 1:
                    f.add('s2_head')
                if ind + 1 in fused:
                    f.add('s2_fused_pool')
                if prev is not None and prev.C % 4:
                    f.add('s2_after_pad')
                if prev is not None and prev.type == 'route' and len(prev.srcs) == 2:
                    f.add('s2_reads_concat')
                root = _alias_root(info, ind - 1)
                if root != ind - 1 and any(k != ind and _is_s2(o) and _alias_root(info, k - 1) == root
                                           for k, o in enumerate(info)):
                    f.add('s2_alias_two_s2_consumers')
                if ind > 0 and _bn_pair_but_for_stride(info, cons, ind - 1):
                    f.add('s2_bn_pair_not_consumer')
                if ind >= 3 and _is_s2(info[ind - 1]) and _is_s2(info[ind - 2]) and any(
                        o.H % 2 or o.W % 2 for o in info[ind - 3:ind]):      # three in a row, an odd map among those they read
                    f.add('s2_chain_odd')
                if nxt is not None and (nxt.type == 'reorg' or (nxt.type == 'maxpool' and nxt.block['stride'] == '1' and
                                                                  prev is not None and prev.type == 'maxpool' and
                                                                  prev.block['stride'] == '1')):
                    f.add('s2_reorg_pool_s1')
                if ind not in live or ind == len(info) - 1:
                    f.add('s2_dead_and_head')
                if nxt is not None and nxt.type == 'avgpool':
                    f.add('s2_classifier')
        elif t == 'maxpool':
            f.add('maxpool2' if b['stride'] == '2' else 'maxpool_s1')
        elif t == 'reorg':
            f.add('reorg')
            if ind > 0 and info[ind - 1].type == 'route' and len(info[ind - 1].srcs) == 1 and nxt is not None and \
                    nxt.type == 'maxpool' and nxt.block['stride'] == '2':
                f.add('reorg_alias_pool')
        elif t == 'route':
            if len(l.srcs) == 1:
                f.add('route1_abs' if int(b['layers']) > 0 else 'route1_rel')
                if l.srcs[0] in fused and len(cons[ind]) >= 2:
                    f.add('alias_pool_2cons')
            else:
                f.add('route2')
                k = l.srcs[1]
                if k == l.srcs[0]:
                    f.add('concat_same')
                if len(cons[k]) >= 3 and any(info[c].type == 'shortcut' for c in cons[k]):
                    f.add('concat_src_shortcut_src')
        elif t == 'shortcut':
            f.add('shortcut')
            f.add('shortcut_' + b['activation'])
            if l.srcs[0] == ind - 1:
                f.add('shortcut_m1')
                if info[ind - 1].type == 'route' and len(info[ind - 1].srcs) == 1:
                    f.add('shortcut_m1_alias')
        elif t == 'avgpool':
            f.add('classifier')
        elif t == 'connected':
            f.add(b['activation'])
            if ind > 0 and info[ind - 1].type == 'connected':
                f.add('connected2')
        elif t == 'softmax':
            f.add('softmax')
            if l.H * l.W > 1 and nxt is not None and nxt.type == 'convolutional':
                f.add('softmax_map_conv')
    if fused:
        f.add('fused_pool')
    pairs = expected_bn_fuse(blocks, B, H, W)
    if pairs:
        f.add('bn_fuse_pair')
    if any(_is_s2(info[s]) for s in pairs.values()):
        f.add('s2_bn_pair_producer')
    return f


# ------------------------------------------------------------------------------------------------ reference forward
def reorg2(x):
    """darknet.py:20-35 at stride 2: out[b, (dy*2+dx)*C + c, hy, wx] = in[b, c, 2*hy+dy, 2*wx+dx]."""
    B, C, H, W = x.shape
    x = x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4).contiguous()
    return x.view(B, 4 * C, H // 2, W // 2)


def _tap(taps, kind, ind, x):
    if taps is not None:
        taps.setdefault(kind, {})[ind] = x.detach().clone()


def ref_run(model, x, training, dtype=torch.float64, taps=None, absnet=False):
    """Forward of a Darknet cfg on a deep copy of the module tree, cast to `dtype`, on the CPU: the reference's block
    semantics (darknet.py:82-130).  Returns (y, the copied modules, {layer: output}).
    taps: a dict that receives {'pre': {layer: input of its leaky / relu}, 'pool': {layer: input of its max-pool}}.
    absnet: the magnitude network of exact_budget - |parameters|, activations replaced by the identity, and a max-pool
    whose backward hands the gradient to every member of the window (it then bounds the true one element by element)."""
    mods = copy.deepcopy(model.models).cpu().to(dtype)
    mods.train(training)
    if absnet:
        for p in mods.parameters():
            p.data.abs_()
    x = x.to(dtype)
    outputs = {}
    for ind, b in enumerate(model.blocks[1:]):
        t = b['type']
        if t == 'convolutional':
            for m in mods[ind]:
                if isinstance(m, (torch.nn.LeakyReLU, torch.nn.ReLU)):
                    _tap(taps, 'pre', ind, x)
                    if absnet:
                        continue
                if isinstance(m, torch.nn.Conv2d):
                    # stride and padding from the cfg (darknet.py:150-153: pad = (size - 1) // 2 if pad else 0), not from the
                    # module the product built: a stride it dropped would otherwise be on both sides
                    k = int(b['size'])
                    assert tuple(m.weight.shape[2:]) == (k, k), (ind, tuple(m.weight.shape))
                    s, p = int(b['stride']), (k - 1) // 2 if int(b['pad']) else 0
                    if k == 1 and s > 1:
                        # the same convolution on the pixels it reads (torch's float32 CPU backward of a strided 1x1
                        # convolution corrupted the heap on some of these shapes)
                        x, s = x[:, :, ::s, ::s], 1
                    x = F.conv2d(x, m.weight, m.bias, stride=s, padding=p)
                else:
                    x = m(x)
        elif t == 'maxpool':
            _tap(taps, 'pool', ind, x)
            s = int(b['stride'])
            xp = x if s > 1 else F.pad(x, (0, 1, 0, 1), mode='replicate')
            k = int(b['size']) if s > 1 else 2
            y = F.max_pool2d(xp, k, max(s, 1))
            if absnet:
                sm = F.avg_pool2d(xp, k, max(s, 1)) * (k * k)
                y = y.detach() + (sm - sm.detach())
            x = y
        elif t == 'avgpool':
            x = x.mean(dim=(2, 3))
        elif t == 'softmax':
            x = F.softmax(x, 1)
        elif t == 'connected':
            m = mods[ind]
            lin = m[0] if isinstance(m, torch.nn.Sequential) else m
            x = F.linear(x.view(x.size(0), -1), lin.weight, lin.bias)
            if isinstance(m, torch.nn.Sequential):
                _tap(taps, 'pre', ind, x)
                if not absnet:
                    x = F.leaky_relu(x, 0.1) if isinstance(m[1], torch.nn.LeakyReLU) else F.relu(x)
        elif t == 'reorg':
            x = reorg2(x)
        elif t == 'route':
            ls = _resolve(b['layers'], ind)
            x = outputs[ls[0]] if len(ls) == 1 else torch.cat([outputs[l] for l in ls], 1)
        elif t == 'shortcut':
            x = outputs[_resolve(b['from'], ind)[0]] + outputs[ind - 1]
            if b['activation'] in ('leaky', 'relu'):
                _tap(taps, 'pre', ind, x)
                if not absnet:
                    x = F.leaky_relu(x, 0.1) if b['activation'] == 'leaky' else F.relu(x)
        elif t in ('region', 'cost'):
            continue
        outputs[ind] = x
    return x, mods, outputs


def ref_generic(model, x, training, dtype=torch.float64):
    """The forward alone (what tests/test_gpu_input_grad.py differentiates)."""
    return ref_run(model, x, training, dtype)[0]


# ------------------------------------------------------------------------------------------------ models and data
def is_exact(case):
    return case.family == 'exact'


def init_params(model, case):
    """Seeded parameters.  Float families: filters N(0, 1) * 1.5 / sqrt(fan_in), biases and BatchNorm betas N(0, 0.1), gammas
    U(0.5, 1.5) of random sign with ONE exact zero per case, running means N(0, 0.1), running variances U(0.5, 1.5).  Exact
    family: at most four +-1 entries per output channel, biases in {-1, 0, 1}."""
    rs = np.random.RandomState(case.wseed)
    bns = []
    with torch.no_grad():
        for m in model.models.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
                shape = tuple(m.weight.shape)
                fan_in = int(np.prod(shape[1:]))
                if is_exact(case):
                    w = np.zeros((shape[0], fan_in), dtype=np.float32)
                    for co in range(shape[0]):
                        idx = rs.choice(fan_in, size=min(fan_in, int(rs.randint(1, 5))), replace=False)
                        w[co, idx] = rs.choice([-1.0, 1.0], size=len(idx))
                    w = w.reshape(shape)
                else:
                    w = (rs.standard_normal(shape) * (1.5 / np.sqrt(fan_in))).astype(np.float32)
                m.weight.copy_(torch.from_numpy(w))
                if m.bias is not None:
                    bias = rs.randint(-1, 2, shape[0]) if is_exact(case) else rs.standard_normal(shape[0]) * 0.1
                    m.bias.copy_(torch.from_numpy(bias.astype(np.float32)))
            elif isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(torch.from_numpy((rs.uniform(0.5, 1.5, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)))
                m.bias.copy_(torch.from_numpy((rs.standard_normal(n) * 0.1).astype(np.float32)))
                m.running_mean.copy_(torch.from_numpy((rs.standard_normal(n) * 0.1).astype(np.float32)))
                m.running_var.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, n).astype(np.float32)))
                bns.append(m)
        if bns:
            m = bns[int(rs.randint(len(bns)))]
            m.weight[int(rs.randint(m.num_features))] = 0.0


def make_model(case, init=True):
    """The product's Darknet module tree for the case, on the CPU, with the case's seeded parameters."""
    from singleshotpose_amd.darknet import Darknet
    fd, path = tempfile.mkstemp(suffix='.cfg')
    try:
        with os.fdopen(fd, 'w') as f:
            f.write(cfg_text(case))
        model = Darknet(path)
    finally:
        os.remove(path)
    if init:
        init_params(model, case)
    return model


def _rs(case, dseed, salt):
    return np.random.RandomState([zlib.crc32(case.id.encode()) & 0x7fffffff, case.wseed, dseed, salt])


def make_input(case, dseed):
    rs = _rs(case, dseed, 1)
    shape = (case.B, case.channels, case.H, case.W)
    if is_exact(case):
        return torch.from_numpy(rs.randint(-2, 3, shape).astype(np.float32))
    return torch.from_numpy(rs.uniform(-1, 1, shape).astype(np.float32))


def make_probe(case, dseed, shape):
    rs = _rs(case, dseed, 2)
    if is_exact(case):
        return torch.from_numpy(rs.randint(-1, 2, tuple(shape)).astype(np.float32))
    return torch.from_numpy(rs.standard_normal(tuple(shape)).astype(np.float32))


Ref = collections.namedtuple('Ref', 'y_eval y_train dx grads stats')


def _one_ref(model, case, dseed, dtype, taps_eval=None, taps_train=None):
    x = make_input(case, dseed)
    with torch.no_grad():
        y_eval = ref_run(model, x, False, dtype, taps_eval)[0]
    xr = x.to(dtype).requires_grad_(True)
    y, mods, _ = ref_run(model, xr, True, dtype, taps_train)
    probe = make_probe(case, dseed, y.shape)
    (y * probe.to(dtype)).sum().backward()
    names = [n for n, _ in model.models.named_parameters()]
    grads = {'models.' + n: (None if p.grad is None else p.grad.detach()) for n, p in zip(names, mods.parameters())}
    stats = {'models.' + n: b.detach() for n, b in mods.named_buffers() if 'running' in n}
    return Ref(y_eval.detach(), y.detach(), xr.grad.detach(), grads, stats)


@functools.lru_cache(maxsize=None)
def reference(case, dseed):
    """(float64 run, float32 run) of the CPU reference: eval output, training output, dL/dx and every parameter gradient
    of (y_train * probe).sum() (None for a parameter of a dead branch), running statistics after that training forward."""
    model = make_model(case)
    return _one_ref(model, case, dseed, torch.float64), _one_ref(model, case, dseed, torch.float32)


def _windows(x, stride):
    if stride == 1:
        x = F.pad(x, (0, 1, 0, 1), mode='replicate')
    u = x.unfold(2, 2, stride).unfold(3, 2, stride)
    return u.reshape(u.shape[:4] + (4,))


def margins(case, dseed):
    """(smallest decision margin, largest float32-against-float64 forward difference), both relative to their layer's
    largest magnitude, over the eval and the training forward.  A decision is the sign of a leaky / relu input or the
    winner of a max-pool window; candidates that are exactly equal in float64 are a tie, not a decision (the first in scan
    order wins on every side)."""
    model = make_model(case)
    taps = {}
    for dt in (torch.float64, torch.float32):
        for mode in ('eval', 'train'):
            taps[dt, mode] = {}
        _one_ref(model, case, dseed, dt, taps[dt, 'eval'], taps[dt, 'train'])
    margin, diff = float('inf'), 0.0
    for mode in ('eval', 'train'):
        t64, t32 = taps[torch.float64, mode], taps[torch.float32, mode]
        for kind in t64:
            for ind, a in t64[kind].items():
                top = max(float(a.abs().max()), 1e-300)
                diff = max(diff, float((a - t32[kind][ind].double()).abs().max()) / top)
                if kind == 'pre':
                    # (a zero that both runs hold exactly - relu zeros summed by a shortcut - is structural, not a decision)
                    z = a[(a != 0) | (t32[kind][ind] != 0)]
                    if z.numel():
                        margin = min(margin, float(z.abs().min()) / top)
                else:
                    stride = int(model.blocks[ind + 1]['stride'])
                    v = _windows(a, stride).sort(dim=-1, descending=True)[0]
                    gap = v[..., :1] - v[..., 1:]
                    gap = gap[gap > 0]
                    if gap.numel():
                        margin = min(margin, float(gap.min()) / top)
    return margin, diff


def margin_ok(case, dseed):
    m, d = margins(case, dseed)
    return m >= 4.0 * d


def find_seed(case):
    """The first data seed in 0..7 under which every decision of the case has its margin (what SEEDS records)."""
    for s in range(8):
        if margin_ok(case, s):
            return s
    return None


def exact_budget(case, dseed=0):
    """Largest magnitude, in grid units, any activation, gradient or filter-gradient partial sum of an exact case can
    reach in any summation order: the magnitude network (|x|, |parameters|, |probe|, identity activations, a max-pool that
    hands its gradient to the whole window) forward and backward.  The grid is 1, or 1 / (avgpool pixels) from the
    classifier tail on (and for every gradient behind it)."""
    model = make_model(case)
    x = make_input(case, dseed).abs().double().requires_grad_(True)
    y, mods, outputs = ref_run(model, x, True, torch.float64, absnet=True)
    for o in outputs.values():
        if o.requires_grad and not o.is_leaf:
            o.retain_grad()
    (y * make_probe(case, dseed, y.shape).abs().double()).sum().backward()
    info = layer_info(model.blocks, case.H, case.W)
    grid = 1
    for ind, l in enumerate(info):
        if l.type == 'avgpool':
            grid *= info[ind - 1].H * info[ind - 1].W
    top = max([float(x.grad.abs().max()), float(x.detach().abs().max())] +
              [float(o.detach().abs().max()) for o in outputs.values()] +
              [float(o.grad.abs().max()) for o in outputs.values() if o.grad is not None] +
              [float(p.grad.abs().max()) for p in mods.parameters() if p.grad is not None])
    return top * grid


# ------------------------------------------------------------------------------------------------ generator
_FILTERS = (6, 8, 12, 16, 18, 20, 24, 32, 64)
_EXACT_FILTERS = (6, 8, 12, 16, 20)


def random_case(seed, exact=False, strided=False):
    """One case from the block grammar: conv 1x1 / 3x3 (stride 1, pad 1, BatchNorm or bias, leaky | linear | relu), max-pool
    2/2 and stride 1, reorg 2, a route of one layer (relative or absolute) or of two whose first is -1, a shortcut from any
    earlier layer of the same shape (-1 included), softmax on a map; then a linear conv head with 4k channels, or
    avgpool -> connected -> [connected] -> softmax.  4..9 blocks, B in {1, 2, 3}, 16..32 px, 1 or 3 input channels, 6..64
    filters, BatchNorm only where B * H * W >= 32.  exact: no BatchNorm, linear | relu, no softmax, avgpool only over a
    power-of-two pixel count.
    strided (the gs2 / xs2 families, a random stream of their own): a conv behind block 0 has stride 2 with probability 0.25
    while its output stays at least 2 x 2; H and W are also drawn from 13, 15, 21, 26, so odd maps occur (a stride-2 conv
    writes ceil(H / 2) x ceil(W / 2)); BatchNorm only where the map the block WRITES has B * Ho * Wo >= 32."""
    rs = np.random.RandomState([seed, (11 if exact else 13) if strided else (7 if exact else 3)])
    B = int(rs.choice([1, 2, 3]))
    odd = [13, 15, 21, 26] if strided else []
    H, W = int(rs.choice([16, 20, 24, 32] + odd)), int(rs.choice([16, 20, 24, 28, 32] + odd))
    ch = int(rs.choice([1, 3]))
    n = int(rs.randint(4, 8 if exact else 10))
    classifier = rs.rand() < 0.3
    filters = _EXACT_FILTERS if exact else _FILTERS
    acts = ('linear', 'relu') if exact else ('leaky', 'linear', 'relu')
    shapes, body = [], []
    cur = (ch, H, W)

    def add(text, shape):
        body.append(text)
        shapes.append(shape)
        return shape

    def spell(l):      # a layer index as the cfg writes it: relative, or absolute where the syntax can say it (> 0)
        return l if (l > 0 and rs.rand() < 0.5) else l - len(shapes)

    if not exact and rs.rand() < 0.35 and B * H * W >= 32 and H % 2 == 0 and W % 2 == 0:
        cur = add(conv(32, 3, 1, 'leaky'), (32, H, W))      # the fused first block (W % 16 == 0) and its fallback
        cur = add(pool(2), (32, H // 2, W // 2))
    ntail = (3 + int(rs.rand() < 0.5)) if classifier else 1
    while True:
        c, h, w = cur
        if len(shapes) >= n - ntail and any(t.startswith('[conv') for t in body):
            if not (classifier and exact and (h * w) & (h * w - 1)):
                break
            classifier, ntail = False, 1      # no power-of-two map to average: a conv head, behind a body of full length
            continue
        kind = rs.choice(['conv', 'pool2', 'pool1', 'reorg', 'route1', 'route2', 'shortcut', 'softmax'],
                         p=[0.42, 0.12, 0.08, 0.07, 0.08, 0.09, 0.11, 0.03])
        ind = len(shapes)
        if kind == 'conv':
            f = int(rs.choice(filters))
            s = 1
            if strided and ind > 0 and h > 2 and w > 2 and rs.rand() < 0.25:
                s, h, w = 2, (h + 1) // 2, (w + 1) // 2      # 1x1 pad 0 and 3x3 pad 1 alike
            bn = int(not exact and B * h * w >= 32 and rs.rand() < 0.6)
            cur = add(conv(f, int(rs.choice([1, 3])), bn, str(rs.choice(acts)), s), (f, h, w))
        elif kind == 'pool2' and h % 2 == 0 and w % 2 == 0 and h >= 4 and w >= 4:
            cur = add(pool(2), (c, h // 2, w // 2))
        elif kind == 'pool1' and ind > 0:
            cur = add(pool(1), cur)
        elif kind == 'reorg' and c % 4 == 0 and h % 2 == 0 and w % 2 == 0 and h >= 4 and w >= 4 and 4 * c <= 128 and ind > 0:
            cur = add(reorg(), (4 * c, h // 2, w // 2))
        elif kind == 'route1' and ind > 1:
            l = int(rs.randint(0, ind))
            cur = add(route(spell(l)), shapes[l])
        elif kind == 'route2' and ind > 0 and c % 4 == 0:
            ks = [k for k in range(ind) if shapes[k][1:] == (h, w) and shapes[k][0] % 4 == 0 and shapes[k][0] + c <= 128]
            if ks:
                k = ks[int(rs.randint(len(ks)))]
                cur = add(route(-1, spell(k)), (c + shapes[k][0], h, w))
        elif kind == 'shortcut' and ind > 0:
            fs = [k for k in range(ind) if shapes[k] == cur]
            k = fs[int(rs.randint(len(fs)))]
            cur = add(shortcut(spell(k), str(rs.choice(acts))), cur)
        elif kind == 'softmax' and not exact and ind > 0:
            cur = add(softmax(), cur)
    if classifier:
        body.append(avgpool())
        nout = int(rs.choice([8, 16, 32]))
        if ntail == 4 or exact:
            body.append(connected(nout, str(rs.choice(acts))))
            body.append(connected(int(rs.choice([4, 8, 12])), 'linear'))
        else:
            body.append(connected(nout, str(rs.choice(acts))))
        if not exact:
            body.append(softmax())
    else:
        body.append(head(int(rs.choice([4, 8, 12, 20]))))
    name = ('xs2' if exact else 'gs2') if strided else ('exact' if exact else 'gen')
    return Case('%s%03d' % (name, seed), 'exact' if exact else 'gen', ''.join(body), B, H, W, ch,
                (300 if strided else 100) + seed)


def random_cfg(seed, exact=False, strided=False):
    return cfg_text(random_case(seed, exact, strided))


# ------------------------------------------------------------------------------------------------ the table
def _hand():
    c, out = conv, []

    def add(prop, i, body, B, H, W, ch=3):
        out.append(Case('%s-%d' % (prop, i), 'hand', body, B, H, W, ch, 500 + len(out)))

    sizes = [(2, 16, 16), (3, 16, 24), (1, 32, 20)]
    sact = ['linear', 'leaky', 'relu']
    for i, (B, H, W) in enumerate(sizes):
        ch = 1 if i == 2 else 3
        # a one-layer route of a pooled block's pool output, read by a conv and by a shortcut
        add('alias_pool_2cons', i, c(16) + pool() + route(1) + c(16, 3, 1, sact[i]) + shortcut(2, sact[i]) + head(8), B, H, W)
        # layer 1 is read by the next conv, by the shortcut and by the concat: three gradient contributions into one buffer
        add('concat_src_shortcut_src', i, c(16, 3, i != 1) + c(16, 1 + 2 * (i % 2), 1) + c(16, 3, i == 1, sact[i]) +
            shortcut(1, sact[(i + 1) % 3]) + route(-1, 1 if i else -3) + head(12), B, H, W, ch)
        # from = -1 behind a one-layer route: both summands are the aliased map
        add('shortcut_m1_alias', i, c(16, 3, i != 2) + c(12 + 4 * i, 3, 1) + route(-1 if i else -2) +
            shortcut(-1, sact[(i + 2) % 3]) + head(8), B, H, W)
        # a conv nothing downstream reads: no gradient for its parameters
        add('dead_branch', i, c(16, 3, 1) + c(20, 1 + 2 * (i % 2), i != 1, sact[i]) + route(-2) + head(4 + 4 * i), B, H, W, ch)
        # a reorg of an aliased map, then a pool no BatchNorm block can absorb
        add('reorg_alias_pool', i, c(8 + 4 * i, 3, 1) + (c(8, 1, 1) if i else '') + route(-2 if i else -1) + reorg() + pool() +
            head(8), B, H, W)
        # 18 (or 6) filters: a padded BatchNorm map in front of a conv - the BatchNorm-backward fusion has to skip it
        add('bn_pad_to_conv', i, c(18 if i < 2 else 6, 3, 1, sact[(i + 1) % 3]) + c(16, 1 + 2 * (i % 2), 1) + head(8), B, H, W, ch)
        # a single-consumer BatchNorm conv -> conv pair: the fusion has to take it
        add('bn_fuse_pair', i, c(16, 3, 1) + c(16 if i == 1 else 32, 1 + 2 * (i % 2), 1, sact[i]) + c(8, 3, 0, 'leaky') + head(20), B, H, W)
        add('channels1', i, c(8 + 8 * i, 3, 1) + pool(1 + i % 2) + c(16, 3, 0, 'relu') + head(8), B, H, W, 1)
        # softmax over the channels of every pixel, then a conv
        add('softmax_map_conv', i, c(8 + 4 * i, 3, i != 1) + softmax() + c(16, 3, 1) + head(8), B, H, W, ch)
        # a pool behind a conv block without BatchNorm: standalone, on the bias + relu path
        add('pool_after_relu_nobn', i, c(16, 3, 0, 'relu') + pool() + c(12, 3, 1, sact[i]) + head(8), B, H, W)
        # both halves of the concat are the same map: its gradient buffer gets two copies
        add('concat_same', i, c(16 if i else 8, 3, 1) + route(-1, -1) + c(16, 3, i == 0, sact[i]) + head(8), B, H, W, ch)
    # 64-channel 3x3 layers (the shapes the tuner times Winograd and split-K candidates on), for the tuned-plan runs
    # (behind a narrow stem and a pool: the decision count, and with it the chance of a marginless one, stays small)
    add('wide', 0, c(16) + pool() + c(64) + c(64, 3, 1) + shortcut(-2, 'leaky') + c(64, 3, 1, 'relu') + head(20), 2, 16, 16)
    add('wide', 1, c(16) + pool() + c(64) + c(128, 3, 1) + c(64, 1, 1) + c(128, 3, 1) + head(20), 1, 16, 24)
    add('wide', 2, c(32) + pool() + c(64) + c(64, 3, 1) + route(-1, -2) + c(64, 3, 0, 'leaky') + head(8), 2, 16, 16)
    add('wide', 3, c(16, 3, 0, 'relu') + reorg() + c(64, 3, 1) + pool(1) + c(64, 3, 1, 'linear') + head(12), 3, 16, 16)
    for i, (B, H, W) in enumerate(sizes):
        # a BatchNorm block in front of a 2x2/2 pool whose un-pooled map a route reads as well: the pool must stay standalone
        add('pool_not_fused_2cons', i, c(8, 3, i != 1) + c(16, 3, 1, sact[i]) + pool() + c(16, 1 + 2 * (i % 2), 1) + route(1) +
            pool() + route(-1, 3) + head(8), B, H, W)
    # ---- stride-2 blocks (ssp_conv_s2_*) meeting the rest of the plan.  Odd maps wherever the body allows them: a strided
    # block writes ceil(H / 2) x ceil(W / 2), and its data gradient walks four parity classes of unequal size
    odd = [(2, 16, 16), (1, 26, 22), (3, 13, 15)]
    s2 = lambda f, k=3, bn=1, act='leaky': c(f, k, bn, act, 2)
    for i, (B, H, W) in enumerate(odd):
        # 18 (or 6) filters in front: Cin_dx % 4 == 2 of the data gradient, into a 20- (8-) wide gradient buffer whose padding
        # columns nothing may write; forward and filter gradient read the padded map
        add('s2_after_pad', i, c(6 if i == 2 else 18, 3, i != 1, sact[(i + 1) % 3]) + s2(16, 1 if i == 1 else 3) + head(8), B, H, W)
        # the data gradient lands in a concat's gradient buffer and is split back to the two producers
        add('s2_reads_concat', i, c(8) + c(8, 1 + 2 * (i % 2)) + route(-1, -2) + s2(16, 3 - 2 * (i % 2), i != 2, 'relu') + head(8),
            B, H, W)
        # one map read through aliases by a 3x3 and by a 1x1 strided block: the data gradient that runs second accumulates.
        # The 1x1 form zeroes the three parity classes it has no tap for when it runs first (i = 0, 2: it is the later layer)
        # and must leave them alone when it runs second (i = 1: the mirrored body)
        ka, kb = (1, 3) if i == 1 else (3, 1)
        add('s2_alias_two_s2_consumers', i, c(16) + route(-1) + s2(16, ka) + route(1) + s2(16, kb, i != 2) +
            shortcut(-3, sact[i]) + head(8), B, H, W)
        # a strided block as the SOURCE of a fused BatchNorm-backward pair: the sums run over its (smaller, odd) output map
        add('s2_bn_pair_producer', i, c(8) + s2(16, 3 - 2 * (i % 2)) + c(16, 3, 1, sact[i]) + head(8), B, H, W)
        # ... and never its consumer: layer 1 keeps the two-pass BatchNorm backward
        add('s2_bn_pair_not_consumer', i, c(8) + c(16, 1 + 2 * (i % 2)) + s2(16, 3 - 2 * (i % 2), i != 1) + head(8), B, H, W)
    for i, (B, H, W) in enumerate(sizes):
        # a 2x2/2 pool folded into a strided BatchNorm block: the block's OUTPUT map is even
        add('s2_fused_pool', i, c(8) + s2(16, 3 - 2 * (i % 2), 1, sact[(i + 1) % 3]) + pool() + head(8), B, H, W)
    for i, (B, H, W) in enumerate([(2, 21, 15), (1, 26, 22), (3, 13, 15)]):
        # three in a row, 26 x 22 -> 13 x 11 -> 7 x 6 -> 4 x 3: BatchNorm while the map a block writes has 32 pixels
        add('s2_chain_odd', i, c(8) + s2(8, 3) + s2(12, 1) + s2(16, 3, 0, 'linear') + head(8), B, H, W)
    for i, (B, H, W) in enumerate(sizes):
        add('s2_reorg_pool_s1', i, c(8) + s2(8, 3, i == 1, 'relu') + reorg() + c(16, 1 + 2 * (i % 2)) + head(8), B, H, W)
    for i, (B, H, W) in enumerate(odd):
        add('s2_reorg_pool_s1', 3 + i, c(8) + pool(1) + s2(16, 3 - 2 * (i % 2), 1, sact[i]) + pool(1) + head(8), B, H, W)
    for i, (B, H, W) in enumerate(odd):
        # a strided block nothing downstream reads; a strided block as the network output (its dy is the caller's gradient)
        add('s2_dead_and_head', i, c(8) + s2(8, 3 - 2 * (i % 2), i != 2) + route(-2) + head(8), B, H, W)
        add('s2_dead_and_head', 3 + i, c(8, 3, 1, sact[i]) + s2(8, 1 + 2 * (i % 2), 0, 'linear'), B, H, W)
        # avgpool over a strided map (56 and 143 pixels: no power of two)
        add('s2_classifier', i, c(8) + s2(16, 3 - 2 * (i % 2)) + avgpool() + connected(8) + softmax(), B, H, W)
    # a stride-1 and a stride-2 64 -> 64 3x3 layer on the same 64 x 8 x 8 map (layers 6 and 3), and a stride-1 64 -> 64 3x3 layer on
    # the strided block's 4 x 4 output (layer 4): layers 3 and 4 launch data gradients of one shape key.  (Layers 4 and 6 are
    # linear: 8192 more leaky signs leave no data seed in 0..7 with every margin)
    add('wide', 4, c(16) + pool() + c(64) + s2(64) + c(64, 3, 1, 'linear') + route(2) + c(64, 3, 1, 'linear') + pool() +
        route(-1, -4) + c(64, 3, 1, 'relu') + head(20), 2, 16, 16)
    # ... behind a block without BatchNorm or activation: that block's own data gradient reads the gradient buffer as it is,
    # padding columns included
    add('s2_after_pad', 3, c(18, 3, 0, 'linear') + s2(16) + head(8), 1, 26, 22)
    return out


def _refused():
    c, out = conv, []

    def add(name, body, B=1, H=16, W=16, ch=3):
        out.append(Case('refused-' + name, 'refused', body, B, H, W, ch, 900 + len(out)))
    add('route3-a', c(8) + c(8) + c(8) + route(-1, -3, -1) + head(20))
    add('route3-b', c(16, 3, 0) + c(16, 1) + route(-1, -2, -1) + head(8), 2, 16, 24)
    add('route_first-a', c(8) + c(8) + route(-2, -1) + head(8))
    add('route_first-b', c(8) + c(8) + c(8) + route(1, -1) + head(8))
    add('concat4-a', c(18) + c(6) + route(-1, -2) + head(8))           # 18 + 6 = 24 channels
    add('concat4-b', c(6, 1, 0) + c(6) + route(-1, -2) + head(8), 2, 16, 24)
    add('odd-pool', c(8, 3, 0) + pool() + head(8), 1, 15, 13)
    add('odd-pool13', c(16) + pool() + c(16) + pool() + head(8), 1, 26, 26)       # the second pool meets a 13 x 13 map
    add('odd-reorg', c(8) + reorg() + head(8), 1, 15, 13)
    add('odd-reorg-w', c(8) + route(-1) + reorg() + head(8), 2, 16, 18 + 1)
    add('last4-a', c(8) + c(18, 1, 0, 'linear'))
    add('last4-b', c(8) + avgpool() + connected(10) + softmax(), 2)
    add('narrow-a', c(18) + c(5) + route(-1, -2) + c(8) + head(8))     # a 23-channel concat in front of a conv
    add('narrow-b', c(6) + c(5, 1) + route(-1, -2) + head(8), 2)
    add('first_s2-a', c(8, 3, 1, 'leaky', 2) + head(8))
    add('first_s2-b', c(8, 1, 0, 'linear', 2) + c(8) + head(8), 2, 16, 24)
    add('odd-s2-pool', c(8) + c(8, 3, 1, 'leaky', 2) + pool() + head(8), 1, 26, 22)       # 13 x 11 behind the strided block
    add('odd-s2-reorg', c(8) + c(8, 1, 0, 'relu', 2) + reorg() + head(8), 1, 26, 22)
    return out


def rank_one_first_block(case):
    """A 1x1 BatchNorm conv on a one-channel input: every channel of its normalised output is + or - ONE map.  Its dbeta is
    exactly zero and its dgamma a residue (gs2023: 5e-2 against 6e2 of summed |terms|, eps32 * 1.2e4 = 7e-4 of itself), so
    the float32 CPU reference's own distance to float64 there - the bar of the GPU test - is one draw of rounding noise (1.8e-4
    with torch's pairwise sums), not a measure of what fp32 can do.  The strided families leave such seeds out."""
    b = blocks_of(case)[1]
    return (case.channels == 1 and b['type'] == 'convolutional' and int(b['size']) == 1 and int(b['batch_normalize']) != 0)


HAND = _hand()
REFUSED = _refused()
# seeds of random_case whose cfg a plan must run (the first 30 of 0, 1, 2, ... that `supported` passes and that have a data
# seed in 0..7 with every decision margin, see SEEDS), and exact
# seeds that pass, stay within the 2^24 budget and keep a third of their output and a tenth of dL/dx non-zero (the first
# twelve such, then two classifier tails and two absolute routes)
GEN_SEEDS = (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 30, 31, 34, 35, 36)
EXACT_SEEDS = (0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 28, 41, 52, 63)
GEN = [random_case(s) for s in GEN_SEEDS]
EXACT = [random_case(s, True) for s in EXACT_SEEDS]
# the strided families, chosen the same way: the first seeds of random_case(s, exact, strided=True) that `supported` passes,
# that hold at least one stride-2 block, and that have a margin seed in 0..7 (gs2) or stay within the budget with a third of
# the output and a tenth of dL/dx non-zero (xs2).  One more condition on gs2, from the reference alone (rank_one_first_block):
# seeds 23 and 42 are passed over
GS2_SEEDS = (0, 5, 7, 14, 15, 18, 20, 28, 29, 30, 37, 43)
XS2_SEEDS = (0, 1, 2, 4, 6, 8, 12, 16, 18)
GS2 = [random_case(s, False, True) for s in GS2_SEEDS]
XS2 = [random_case(s, True, True) for s in XS2_SEEDS]
# (the hand cases with a strided block go behind the earlier families: tests that take "the first n of FLOAT with ..." -
# tests/test_finetune_cpu.py, tests/test_gpu_finetune.py - keep the cases they had)
HAND_S2 = [c for c in HAND if c.id.startswith('s2_') or c.id == 'wide-4']
FLOAT = [c for c in HAND if c not in HAND_S2] + GEN + HAND_S2 + GS2
CASES = {c.id: c for c in HAND + GEN + GS2 + EXACT + XS2 + REFUSED}

# cases the GPU test runs by more than one route (input-only backward, graph replay, a second step, both BatchNorm-backward
# forms, a second batch size and resolution) and with tuned plans
ROUTES = ('alias_pool_2cons-0', 'concat_src_shortcut_src-0', 'reorg_alias_pool-0', 'softmax_map_conv-0', 'channels1-0',
          'gen012', 'concat_same-0', 'bn_pad_to_conv-0', 's2_alias_two_s2_consumers-0', 'gs2020')
TUNED = ('wide-0', 'wide-1', 'wide-2', 'wide-3', 'wide-4')
VARIANTS = ('step2', 'b1', 'res2')


def variant(case, what):
    """'step2': the same topology with other weights (the second training step of a plan); 'b1': batch 1; 'res2': 8 px
    more in both directions (a second plan of the same model)."""
    if what == 'step2':
        return case._replace(id=case.id + '@step2', wseed=case.wseed + 1000)
    if what == 'b1':
        return case._replace(id=case.id + '@b1', B=1)
    return case._replace(id=case.id + '@res2', H=case.H + 8, W=case.W + 8)


# first data seed in 0..7 under which every decision has its margin (find_seed; test_topology_cpu.py checks each)
SEEDS = {
 'pool_not_fused_2cons-0': 0,
 'pool_not_fused_2cons-1': 1,
 'pool_not_fused_2cons-2': 0,
 'alias_pool_2cons-0': 1,
 'alias_pool_2cons-0@b1': 0,
 'alias_pool_2cons-0@res2': 2,
 'alias_pool_2cons-0@step2': 0,
 'alias_pool_2cons-1': 0,
 'alias_pool_2cons-2': 1,
 'bn_fuse_pair-0': 0,
 'bn_fuse_pair-1': 2,
 'bn_fuse_pair-2': 3,
 'bn_pad_to_conv-0': 1,
 'bn_pad_to_conv-0@b1': 0,
 'bn_pad_to_conv-0@res2': 0,
 'bn_pad_to_conv-0@step2': 0,
 'bn_pad_to_conv-1': 0,
 'bn_pad_to_conv-2': 0,
 'channels1-0': 0,
 'channels1-0@b1': 0,
 'channels1-0@res2': 0,
 'channels1-0@step2': 1,
 'channels1-1': 0,
 'channels1-2': 1,
 'concat_same-0': 0,
 'concat_same-0@b1': 0,
 'concat_same-0@res2': 0,
 'concat_same-0@step2': 0,
 'concat_same-1': 1,
 'concat_same-2': 1,
 'concat_src_shortcut_src-0': 2,
 'concat_src_shortcut_src-0@b1': 0,
 'concat_src_shortcut_src-0@res2': 2,
 'concat_src_shortcut_src-0@step2': 0,
 'concat_src_shortcut_src-1': 0,
 'concat_src_shortcut_src-2': 1,
 'dead_branch-0': 0,
 'dead_branch-1': 0,
 'dead_branch-2': 0,
 'gen000': 5,
 'gen001': 0,
 'gen002': 5,
 'gen004': 2,
 'gen005': 0,
 'gen006': 0,
 'gen007': 0,
 'gen008': 4,
 'gen009': 0,
 'gen010': 4,
 'gen011': 1,
 'gen012': 0,
 'gen012@b1': 0,
 'gen012@res2': 3,
 'gen012@step2': 1,
 'gen013': 0,
 'gen016': 0,
 'gen018': 0,
 'gen019': 0,
 'gen020': 0,
 'gen021': 0,
 'gen022': 0,
 'gen023': 0,
 'gen024': 0,
 'gen025': 6,
 'gen026': 0,
 'gen027': 0,
 'gen028': 0,
 'gen030': 0,
 'gen031': 0,
 'gen034': 0,
 'gen035': 4,
 'gen036': 2,
 'pool_after_relu_nobn-0': 0,
 'pool_after_relu_nobn-1': 0,
 'pool_after_relu_nobn-2': 1,
 'reorg_alias_pool-0': 0,
 'reorg_alias_pool-0@b1': 0,
 'reorg_alias_pool-0@res2': 0,
 'reorg_alias_pool-0@step2': 0,
 'reorg_alias_pool-1': 1,
 'reorg_alias_pool-2': 1,
 'shortcut_m1_alias-0': 1,
 'shortcut_m1_alias-1': 0,
 'shortcut_m1_alias-2': 2,
 'softmax_map_conv-0': 1,
 'softmax_map_conv-0@b1': 0,
 'softmax_map_conv-0@res2': 2,
 'softmax_map_conv-0@step2': 0,
 'softmax_map_conv-1': 0,
 'softmax_map_conv-2': 0,
 'wide-0': 4,
 'wide-1': 2,
 'wide-2': 4,
 'wide-3': 0,
 # the cases with stride-2 blocks
 's2_after_pad-0': 0,
 's2_reads_concat-0': 0,
 's2_alias_two_s2_consumers-0': 0,
 's2_bn_pair_producer-0': 0,
 's2_bn_pair_not_consumer-0': 1,
 's2_after_pad-1': 0,
 's2_reads_concat-1': 0,
 's2_alias_two_s2_consumers-1': 0,
 's2_bn_pair_producer-1': 0,
 's2_bn_pair_not_consumer-1': 0,
 's2_after_pad-2': 0,
 's2_after_pad-3': 0,
 's2_reads_concat-2': 0,
 's2_alias_two_s2_consumers-2': 0,
 's2_bn_pair_producer-2': 0,
 's2_bn_pair_not_consumer-2': 3,
 's2_fused_pool-0': 1,
 's2_fused_pool-1': 0,
 's2_fused_pool-2': 0,
 's2_chain_odd-0': 0,
 's2_chain_odd-1': 0,
 's2_chain_odd-2': 0,
 's2_reorg_pool_s1-0': 0,
 's2_reorg_pool_s1-1': 0,
 's2_reorg_pool_s1-2': 1,
 's2_reorg_pool_s1-3': 0,
 's2_reorg_pool_s1-4': 1,
 's2_reorg_pool_s1-5': 0,
 's2_dead_and_head-0': 0,
 's2_dead_and_head-3': 0,
 's2_classifier-0': 0,
 's2_dead_and_head-1': 0,
 's2_dead_and_head-4': 0,
 's2_classifier-1': 0,
 's2_dead_and_head-2': 0,
 's2_dead_and_head-5': 0,
 's2_classifier-2': 0,
 'wide-4': 0,
 'gs2000': 1,
 'gs2005': 0,
 'gs2007': 1,
 'gs2014': 0,
 'gs2015': 0,
 'gs2018': 2,
 'gs2020': 0,
 'gs2028': 0,
 'gs2029': 0,
 'gs2030': 1,
 'gs2037': 0,
 'gs2043': 5,
 'gs2020@b1': 1,
 'gs2020@res2': 1,
 'gs2020@step2': 0,
 's2_alias_two_s2_consumers-0@b1': 0,
 's2_alias_two_s2_consumers-0@res2': 0,
 's2_alias_two_s2_consumers-0@step2': 0
}


def seed_of(case):
    return 0 if is_exact(case) else SEEDS[case.id]

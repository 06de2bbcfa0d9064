"""Shared data of the depthwise-convolution tests (tests/test_depthwise_cpu.py, tests/test_gpu_depthwise.py): a numpy
statement of the three kernels of csrc/conv_depthwise.hip written from the header comment of the family in include/ssp_hip.h,
the kernel cases, small nets with depthwise blocks as cfg text, and a float64 torch reference of those nets that honours
`groups` and is a plain function of the model's parameters.  Nothing here touches a GPU or imports anything from oracle/.

Kernel semantics (include/ssp_hip.h): fp32 NHWC maps, filter w[c*9 + tap] = the (C, 1, 3, 3) parameter, tap = 3 r + t, padding 1,
input pixel of output pixel (yo, xo) and tap (r, t) = (stride*yo + r - 1, stride*xo + t - 1), zero outside the map;
  forward  out[po][c] = sum_tap in[gather(po, tap)][c] * w[c][tap] (+ bias[c])
  dgrad    dx[pi][c] (=|+=) sum over the (po, tap) pairs that read pi of dy[po][c] * w[c][tap]
  wgrad    dw[c][tap] (=|+=) sum_po dy[po][c] * in[gather(po, tap)][c]
Kernel cases hold integers (x, dy in [-8, 8], filters in [-3, 3], prefills in [-4, 4]): every partial sum stays below 2^24
(exactness_bound), so fp32 in any order is exact and the GPU tests compare with torch.equal.

Float nets carry a data seed (SEEDS, found here on the CPU with find_seed) under which every leaky sign and every max-pool
winner of the float64 reference keeps the margin tests/topology_cases.py demands (4x the float32-against-float64 forward
difference); the exact net has integer data and parameters with every partial sum below 2^24 (exact_budget).
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import topology_cases as T

SENTINEL = 77.0

# ------------------------------------------------------------------------------------------------ the kernels on the host
# side: which map is a channel slice [off, off + C) of rows of ld floats - 'in' (forward input / dx / the filter gradient's
# x) or 'out' (forward output / dy); the other map is dense (ld = C).  ld None = C.
KCase = collections.namedtuple('KCase', 'B H W C stride ld off side')


def _both(B, H, W, C, ld=None, off=0, side='in'):
    return [KCase(B, H, W, C, s, ld, off, side) for s in (1, 2)]


KERNEL_CASES = (
    _both(1, 1, 1, 4) +                       # only the centre tap is in range
    _both(2, 3, 5, 8) +                       # odd sizes and an image boundary: a tap must not read the neighbouring image
    [KCase(1, 2, 2, 4, 2, None, 0, 'in')] +   # a 1 x 1 output
    _both(1, 4, 19, 8) +                      # a row longer than any strip and not a multiple of one
    _both(2, 13, 13, 40) +                    # ten quads per pixel: they do not fill a wave evenly; 13 -> 7 at stride 2
    _both(1, 5, 5, 260) +                     # 65 quads: more than one wave of channels, several quad groups of the filter gradient
    _both(2, 26, 26, 32) +                    # several workgroups, statistics tiles and filter-gradient ranges; M = 1352
    _both(2, 6, 6, 16, 48, 16, 'in') +        # the input side is a slice of a wider buffer
    _both(2, 6, 6, 16, 48, 16, 'out'))        # the output side is


def kcase_id(k):
    return 'b%d_%dx%dx%d_s%d_ld%s_off%d_%s' % (k.B, k.H, k.W, k.C, k.stride, k.ld or k.C, k.off, k.side)


def out_hw(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def _windows(xp, Ho, Wo, s):
    """The nine (B, Ho, Wo, C) views of a zero-padded (B, H + 2, W + 2, C) map, by tap."""
    return [xp[:, r:r + s * (Ho - 1) + 1:s, t:t + s * (Wo - 1) + 1:s] for r in range(3) for t in range(3)]


def _padded(x):
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), np.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    return xp


def dw_fwd_ref(x, w, stride, bias=None):
    """x (B, H, W, C), w (C, 9) -> (B, Ho, Wo, C), float64."""
    Ho, Wo = out_hw(x.shape[1], x.shape[2], stride)
    out = np.zeros((x.shape[0], Ho, Wo, x.shape[3]), np.float64)
    for tap, v in enumerate(_windows(_padded(x), Ho, Wo, stride)):
        out += v * w[:, tap].astype(np.float64)
    return out if bias is None else out + bias.astype(np.float64)


def dw_dgrad_ref(dy, w, H, W, stride, pre=None):
    """dy (B, Ho, Wo, C) -> dx (B, H, W, C), float64: every (output pixel, tap) pair adds into the input pixel it read."""
    B, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == out_hw(H, W, stride)
    dxp = np.zeros((B, H + 2, W + 2, C), np.float64)
    for tap, v in enumerate(_windows(dxp, Ho, Wo, stride)):
        v += dy * w[:, tap].astype(np.float64)          # (a view: strided windows of one tap never overlap)
    dx = dxp[:, 1:H + 1, 1:W + 1]
    return dx if pre is None else dx + pre


def dw_wgrad_ref(dy, x, stride, pre=None):
    """-> (C, 9) float64."""
    B, Ho, Wo, C = dy.shape
    dw = np.stack([(dy.astype(np.float64) * v).sum((0, 1, 2)) for v in _windows(_padded(x), Ho, Wo, stride)], 1)
    return dw if pre is None else dw + pre


def exactness_bound(k):
    """Largest magnitude a partial sum of any of the three kernels can reach on the case's integer data, in any order."""
    x, dy, w, pre_out, pre_in, pre_w = kernel_data(k)
    ax, ady, aw = np.abs(x), np.abs(dy), np.abs(w)
    return max(float(dw_fwd_ref(ax, aw, k.stride, np.full(k.C, 3.0)).max()) + 4,
               float(dw_dgrad_ref(ady, aw, k.H, k.W, k.stride, np.abs(pre_in)).max()),
               float(dw_wgrad_ref(ady, ax, k.stride, np.abs(pre_w)).max()))


@functools.lru_cache(maxsize=None)
def kernel_data(k):
    """(x, dy, w (C, 9), prefill of the output, of dx, of dw) of a kernel case: float32 integers, shared, never written."""
    rs = np.random.RandomState([k.B, k.H, k.W, k.C, k.stride])
    Ho, Wo = out_hw(k.H, k.W, k.stride)
    i_, o_ = (k.B, k.H, k.W, k.C), (k.B, Ho, Wo, k.C)
    f = lambda lo, hi, s: rs.randint(lo, hi + 1, s).astype(np.float32)
    out = (f(-8, 8, i_), f(-8, 8, o_), f(-3, 3, (k.C, 9)), f(-4, 4, o_), f(-4, 4, i_), f(-4, 4, (k.C, 9)))
    for a in out:
        a.setflags(write=False)
    return out


def embed(x, ld, off, fill=None):
    """(..., C) values as rows of ld floats, columns [off, off + C); every other column holds SENTINEL.  fill: what the
    slice holds instead of x (a destination before the launch)."""
    C = x.shape[-1]
    buf = np.full((x.size // C, ld or C), SENTINEL, dtype=np.float32)
    buf[:, off:off + C] = x.reshape(-1, C) if fill is None else fill
    return buf


def sides(k):
    """(ld, off) of the input-side and of the output-side map of a kernel case."""
    sl = (k.ld or k.C, k.off)
    return (sl, (k.C, 0)) if k.side == 'in' else ((k.C, 0), sl)


def stats_depth(C):
    """Longest chain of fp32 Chan combines behind one (mean, M2) pair of a statistics tile (header comment of the family):
    a strip of <= 4 values, ceil(NS / parts) strips in a part, the parts - what the bars of the statistics test scale with."""
    ns = max(1, min(64, 1024 // (C // 4)))
    parts = max(1, 256 // C)
    return 3 + (ns + parts - 1) // parts + parts


# ------------------------------------------------------------------------------------------------ nets
def dw(c, bn=1, act='leaky', stride=1, groups=None, size=3, pad=1):
    return '[convolutional]\n%sfilters=%d\ngroups=%d\nsize=%d\nstride=%d\npad=%d\nactivation=%s\n\n' % (
        'batch_normalize=1\n' if bn else '', c, c if groups is None else groups, size, stride, pad, act)


conv, pool, route, shortcut, head = T.conv, T.pool, T.route, T.shortcut, T.head

# 0 conv 8 + 1 pool (fused) | 2 dw 8 | 3 1x1 16 | 4 dw 16 / 2 | 5 1x1 16 | 6 head
DW_SEP = T.Case('dw_sep', 'dw', conv(8) + pool() + dw(8) + conv(16, 1) + dw(16, stride=2) + conv(16, 1) + head(8), 2, 16, 16, 3, 21)
# every layer behind the input is a depthwise block or a 1x1: what the default-mode reproducibility test runs (no 3x3 dense
# filter gradient, whose atomic sums differ from run to run)
DW_ONLY = T.Case('dw_only', 'dw', conv(8, 1) + dw(8) + conv(16, 1) + dw(16, stride=2) + head(8), 2, 12, 12, 3, 22)
DW_BIAS = T.Case('dw_bias', 'dw', conv(8) + dw(8, 0, 'linear') + head(8), 2, 8, 8, 3, 23)
# inverted residual: 0 conv 8 | 1 1x1 expand 16 | 2 dw 16 | 3 1x1 linear 8 | 4 shortcut 0 + 3 | 5 head
DW_RES = T.Case('dw_res', 'dw', conv(8) + conv(16, 1) + dw(16) + conv(8, 1, 1, 'linear') + shortcut(-4) + head(8), 2, 8, 8, 3, 24)
# layer 0 feeds the depthwise block (1) and the shortcut (2): the depthwise data gradient accumulates into its gradient
DW_SHARED = T.Case('dw_shared', 'dw', conv(8) + dw(8) + shortcut(-2) + head(8), 2, 8, 8, 3, 25)
# 2 = the concatenation buffer of layers 1 and 0, read by the depthwise block 3
DW_ROUTE = T.Case('dw_route', 'dw', conv(8) + conv(8) + route(-1, -2) + dw(16) + head(8), 2, 8, 8, 3, 26)
DW_POOL = T.Case('dw_pool', 'dw', conv(8) + dw(8) + pool() + head(8), 2, 8, 8, 3, 27)
DW_LAST = T.Case('dw_last', 'dw', conv(8) + dw(8), 2, 8, 8, 3, 28)
# integers: no BatchNorm, relu / linear, parameters in {-1, 0, 1} (topology_cases.init_params' exact family)
DW_EXACT = T.Case('dw_exact', 'exact', conv(8, 3, 0, 'relu') + pool() + dw(8, 0, 'linear') + conv(16, 1, 0, 'relu') +
                  dw(16, 0, 'relu', stride=2) + head(8), 2, 16, 16, 3, 5)

# DW_SEP with other weights (what its model holds for the second step of one plan) and at batch 1
DW_SEP_STEP2 = DW_SEP._replace(id='dw_sep_step2', wseed=31)
DW_SEP_B1 = DW_SEP._replace(id='dw_sep_b1', B=1)

FLOAT = [DW_SEP, DW_ONLY, DW_BIAS, DW_RES, DW_SHARED, DW_ROUTE, DW_POOL, DW_LAST, DW_SEP_STEP2, DW_SEP_B1]
NETS = FLOAT + [DW_EXACT]
# what a plan records for each net: Plan.depthwise, Plan.fused_pool, and the (consumer <- source) pairs of _plan_bn_fusion -
# a depthwise block is never the consumer of a pair, it may be the source
PLANS = {
    'dw_sep': dict(depthwise=[2, 4], fused_pool={1}, bn_pairs={3: 2, 5: 4, 6: 5}),
    'dw_only': dict(depthwise=[1, 3], fused_pool=set(), bn_pairs={2: 1, 4: 3}),
    'dw_bias': dict(depthwise=[1], fused_pool=set(), bn_pairs={}),
    'dw_res': dict(depthwise=[2], fused_pool=set(), bn_pairs={3: 2}),
    'dw_shared': dict(depthwise=[1], fused_pool=set(), bn_pairs={}),
    'dw_route': dict(depthwise=[3], fused_pool=set(), bn_pairs={4: 3}),
    'dw_pool': dict(depthwise=[1], fused_pool={2}, bn_pairs={}),
    'dw_last': dict(depthwise=[1], fused_pool=set(), bn_pairs={}),
    'dw_exact': dict(depthwise=[2, 4], fused_pool=set(), bn_pairs={}),
}
PLANS['dw_sep_step2'] = PLANS['dw_sep_b1'] = PLANS['dw_sep']
# data seeds: find_seed(case) on the CPU (test_depthwise_cpu.py re-checks the margins under them)
SEEDS = {'dw_sep': 0, 'dw_only': 0, 'dw_bias': 0, 'dw_res': 0, 'dw_shared': 0, 'dw_route': 0, 'dw_pool': 0, 'dw_last': 0,
         'dw_sep_step2': 0, 'dw_sep_b1': 0, 'dw_exact': 0}

# (id, body, channels of the input, message pattern): what is refused when the plan is built
REFUSED = [
    ('groups2', conv(8) + dw(8, groups=2) + head(8), 3, r'block 1 \(convolutional\): groups=2 on a 8-channel map'),
    ('groups4_of_8', conv(8) + dw(8, groups=4) + head(8), 3, r'block 1 \(convolutional\): groups=4 on a 8-channel map'),
    ('groups3_of_8', conv(8) + dw(8, groups=3) + head(8), 3, r'block 1 \(convolutional\): groups=3 does not divide'),
    ('multiplier', conv(8) + dw(16, groups=8) + head(8), 3,
     r'block 1 \(convolutional\): a depthwise convolution with filters=16 on 8 channels \(a channel multiplier'),
    ('size1', conv(8) + dw(8, size=1) + head(8), 3, r'block 1 \(convolutional\): a depthwise convolution with size=1 pad=1'),
    ('pad0', conv(8) + dw(8, pad=0) + head(8), 3, r'block 1 \(convolutional\): a depthwise convolution with size=3 pad=0'),
    ('six_channels', conv(6) + dw(6) + head(8), 3, r'block 1 \(convolutional\): a depthwise convolution on a 6-channel map'),
    ('block0', dw(4) + head(8), 4, r'block 0 \(convolutional\): a depthwise convolution on the network input'),
]


def seed_of(case):
    return SEEDS[case.id]


make_model, make_input, make_probe = T.make_model, T.make_input, T.make_probe


# ------------------------------------------------------------------------------------------------ float64 reference
def _tap(taps, kind, ind, x):
    if taps is not None:
        taps.setdefault(kind, {})[ind] = x.detach().clone()


def ref_forward(blocks, names, params, bufs, x, training, taps=None, absnet=False):
    """The net as a function of its parameters.  blocks: the parsed cfg; names[ind]: the child names of block ind's
    nn.Sequential ('conv3', 'bn3', ...); params / bufs: {state_dict key without 'models.': tensor} (running statistics are
    updated in place by a training pass).  Returns (y, {layer: output}).  A [convolutional] block honours groups=.  absnet:
    the magnitude network of exact_budget (the caller passes |parameters| and |x|; identity activations, a max-pool whose
    backward hands the gradient to the whole window)."""
    outs = {}
    for ind, b in enumerate(blocks[1:]):
        t = b['type']
        if t == 'convolutional':
            cn = names[ind][0]
            k, s = int(b['size']), int(b['stride'])
            w, bias = params['%d.%s.weight' % (ind, cn)], params.get('%d.%s.bias' % (ind, cn))
            x = F.conv2d(x, w, bias, stride=s, padding=(k - 1) // 2 if int(b['pad']) else 0, groups=int(b.get('groups', 1)))
            if int(b['batch_normalize']):
                bn = '%d.%s.' % (ind, names[ind][1])
                x = F.batch_norm(x, bufs[bn + 'running_mean'], bufs[bn + 'running_var'], params[bn + 'weight'],
                                 params[bn + 'bias'], training, 0.1, 1e-4)
            if b['activation'] in ('leaky', 'relu'):
                _tap(taps, 'pre', ind, x)
                if not absnet:
                    x = F.leaky_relu(x, 0.1) if b['activation'] == 'leaky' else F.relu(x)
        elif t == 'maxpool':
            assert int(b['size']) == 2 and int(b['stride']) == 2
            _tap(taps, 'pool', ind, x)
            y = F.max_pool2d(x, 2, 2)
            if absnet:
                sm = F.avg_pool2d(x, 2, 2) * 4
                y = y.detach() + (sm - sm.detach())
            x = y
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


Ref = T.Ref


def run_ref(model, x, probe, dtype, taps_eval=None, taps_train=None):
    """Eval output, training output, dL/dx, parameter gradients of (y_train * probe).sum() and the running statistics after
    the training forward of `model` (any Darknet tree on the CPU) on input x."""
    names, params, bufs = model_state(model, dtype)
    with torch.no_grad():
        y_eval = ref_forward(model.blocks, names, params, bufs, x.to(dtype), False, taps_eval)[0]
    xr = x.to(dtype).requires_grad_(True)
    y, _ = ref_forward(model.blocks, names, params, bufs, xr, True, taps_train)
    (y * probe.to(dtype)).sum().backward()
    grads = {'models.' + n: (None if p.grad is None else p.grad.detach()) for n, p in params.items()}
    stats = {'models.' + n: b for n, b in bufs.items()}
    return Ref(y_eval.detach(), y.detach(), xr.grad.detach(), grads, stats)


def _one_ref(model, case, dseed, dtype, taps_eval=None, taps_train=None):
    x = make_input(case, dseed)
    names, params, bufs = model_state(model, dtype)
    with torch.no_grad():
        shape = ref_forward(model.blocks, names, params, bufs, x.to(dtype), False)[0].shape
    return run_ref(model, x, make_probe(case, dseed, shape), dtype, taps_eval, taps_train)


@functools.lru_cache(maxsize=None)
def reference(case, dseed):
    """(float64 run, float32 run) of a net.  Computed once, shared, never written."""
    model = make_model(case)
    return _one_ref(model, case, dseed, torch.float64), _one_ref(model, case, dseed, torch.float32)


def margins(case, dseed):
    """topology_cases.margins on this module's reference: (smallest decision margin, largest float32-against-float64
    forward difference), relative to their layer's largest magnitude, over the eval and the training forward."""
    model = make_model(case)
    taps = {}
    for dt in (torch.float64, torch.float32):
        taps[dt, 'eval'], taps[dt, 'train'] = {}, {}
        _one_ref(model, case, dseed, dt, taps[dt, 'eval'], taps[dt, 'train'])
    margin, diff = float('inf'), 0.0
    for mode in ('eval', 'train'):
        t64, t32 = taps[torch.float64, mode], taps[torch.float32, mode]
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


def margin_ok(case, dseed):
    m, d = margins(case, dseed)
    return m >= 4.0 * d


def find_seed(case):
    for s in range(8):
        if margin_ok(case, s):
            return s
    return None


def exact_budget(case, dseed=0):
    """Largest magnitude any activation, gradient or filter-gradient partial sum of the exact net can reach in any summation
    order (topology_cases.exact_budget on this module's reference)."""
    model = make_model(case)
    names, params, bufs = model_state(model, torch.float64)
    for p in params.values():
        p.data.abs_()
    x = make_input(case, dseed).abs().double().requires_grad_(True)
    y, outs = ref_forward(model.blocks, names, params, bufs, x, True, absnet=True)
    for o in outs.values():
        if o.requires_grad and not o.is_leaf:
            o.retain_grad()
    (y * make_probe(case, dseed, y.shape).abs().double()).sum().backward()
    return max([float(x.grad.abs().max()), float(x.detach().abs().max())] +
               [float(o.detach().abs().max()) for o in outs.values()] +
               [float(o.grad.abs().max()) for o in outs.values() if o.grad is not None] +
               [float(p.grad.abs().max()) for p in params.values() if p.grad is not None])

"""Shared data of the [upsample] tests (tests/test_upsample_cpu.py, tests/test_gpu_upsample.py): a numpy restatement of the
two kernels of csrc/upsample.hip, the kernel shapes, small nets with the block as cfg text, and a float64 torch reference of
those nets that is a plain function of the model's parameters.  Nothing here touches a GPU or imports anything from oracle/.

Kernel semantics (include/ssp_hip.h): forward out[b, y, x, c] = in[b, y // N, x // N, c]; backward dsrc[b, y, x, c] (=|+=)
the N x N window of g taken row-major with sequential float32 adds (s = g00; s += g01; ...), then dsrc + s when accumulating.

Float nets carry a data seed (SEEDS, found here on the CPU with find_seed) under which every leaky sign and every max-pool
winner of the float64 reference keeps the margin tests/topology_cases.py demands (4x the float32-against-float64 forward
difference); the exact net has integer data and parameters with every partial sum below 2^24 (exact_budget), so fp32 in
any order is exact.  test_upsample_cpu.py checks both with the reference alone.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import topology_cases as T

SENTINEL = 77.0

# ------------------------------------------------------------------------------------------------ the two kernels on the host
# side: which map is a channel slice [off, off + C) of rows of ld floats - 'fine' (forward destination, backward source) or
# 'coarse' (forward source, backward destination); the other map is dense (ld = C).  ld None = C.
KCase = collections.namedtuple('KCase', 'B H W C stride ld off side')
KERNEL_CASES = [
    KCase(1, 1, 1, 4, 2, None, 0, 'fine'),        # a single pixel
    KCase(2, 3, 5, 8, 2, None, 0, 'fine'),        # odd sizes, a batch boundary
    KCase(2, 13, 13, 40, 2, None, 0, 'fine'),     # rows of 10 quads: they do not fill a wave evenly; more than one workgroup
    KCase(1, 2, 3, 4, 3, None, 0, 'fine'),        # stride 3
    KCase(2, 4, 4, 8, 4, None, 0, 'fine'),        # stride 4
    KCase(1, 1, 2, 4, 8, None, 0, 'fine'),        # the largest stride
    KCase(2, 6, 6, 16, 2, 48, 16, 'fine'),        # the fine side is a slice of a wider buffer
    KCase(2, 6, 6, 16, 2, 48, 16, 'coarse'),      # the coarse side is
    KCase(2, 5, 4, 8, 2, 8, 0, 'fine'),           # C = the padded count of a 6-channel map
]


def kcase_id(k):
    return 'b%d_%dx%dx%d_s%d_ld%s_off%d_%s' % (k.B, k.H, k.W, k.C, k.stride, k.ld or k.C, k.off, k.side)


def up_fwd_ref(src, n):
    """(B, H, W, C) -> (B, nH, nW, C): an index copy."""
    ys, xs = np.arange(src.shape[1] * n) // n, np.arange(src.shape[2] * n) // n
    return src[:, ys][:, :, xs]


def up_bwd_ref(g, n, dsrc=None):
    """(B, nH, nW, C) float32 -> (B, H, W, C): the window row-major, sequential float32 adds; dsrc + s when accumulating."""
    assert g.dtype == np.float32 and (dsrc is None or dsrc.dtype == np.float32)
    s = g[:, 0::n, 0::n].copy()
    for i in range(n):
        for j in range(n):
            if i or j:
                s = s + g[:, i::n, j::n]
    return s if dsrc is None else dsrc + s


def kernel_data(k, integer):
    """(coarse map, gradient of the fine map, earlier content of the coarse gradient) of a kernel case, float32."""
    rs = np.random.RandomState([k.B, k.H, k.W, k.C, k.stride, int(integer)])
    coarse, fine = (k.B, k.H, k.W, k.C), (k.B, k.H * k.stride, k.W * k.stride, k.C)
    if integer:
        return [rs.randint(-8, 9, s).astype(np.float32) for s in (coarse, fine, coarse)]
    return [rs.standard_normal(s).astype(np.float32) for s in (coarse, fine, coarse)]


def embed(x, ld, off, fill=None):
    """(..., C) values as rows of ld floats, columns [off, off + C); every other column holds SENTINEL.  fill: what the
    slice holds instead of x (a destination before the launch)."""
    C = x.shape[-1]
    buf = np.full((x.size // C, ld or C), SENTINEL, dtype=np.float32)
    buf[:, off:off + C] = x.reshape(-1, C) if fill is None else fill
    return buf


# ------------------------------------------------------------------------------------------------ nets
def up(stride=2):
    return '[upsample]\nstride=%d\n\n' % stride


REGION = ('[region]\nanchors =\nclasses=1\ncoords=18\nnum=1\nobject_scale=5\nnoobject_scale=0.1\nclass_scale=1\ncoord_scale=1\n'
          'thresh = .6\n')
conv, pool, route, shortcut, head = T.conv, T.pool, T.route, T.shortcut, T.head

# 0 conv 8 + 1 pool (fused) | 2 conv 16 = the lateral map, 16 x 16 | 3 pool | 4 conv 32 | 5 1x1 conv 16 | 6 upsample |
# 7 route 6, 2 | 8 conv 16 | 9 head 20 | 10 region
UP_NET = T.Case('up_net', 'up', conv(8) + pool() + conv(16) + pool() + conv(32) + conv(16, 1) + up() + route(-1, 2) + conv(16) +
                head(20) + REGION, 2, 32, 32, 3, 11)
# a 6-filter block, upsampled in a buffer of its own with two padding channels, then a conv
UP_PAD = T.Case('up_pad', 'up', conv(6) + up() + conv(8) + head(8), 2, 8, 8, 3, 12)
# layer 2 feeds the upsample (3), a shortcut (7) and a one-layer route (8): its gradient accumulates
UP_SHARED = T.Case('up_shared', 'up', conv(8) + pool() + conv(8) + up() + route(-1, -4) + conv(8) + pool() + shortcut(2) +
                   route(2) + conv(8) + shortcut(7) + head(8), 2, 16, 16, 3, 13)
# stride 4: the 8 x 8 map of layer 4 joins the 32 x 32 map of layer 0
UP_S4 = T.Case('up_s4', 'up', conv(8) + pool() + conv(8) + pool() + conv(16) + up(4) + route(-1, -6) + conv(8) + head(8),
               2, 32, 32, 3, 14)
UP_INPUT = T.Case('up_input', 'up', up() + conv(8) + head(8), 2, 8, 8, 3, 15)
UP_LAST = T.Case('up_last', 'up', conv(8) + head(8) + up(), 2, 8, 8, 3, 16)
# UP_NET on integers: no BatchNorm, relu / linear, parameters in {-1, 0, 1} (topology_cases.init_params' exact family)
UP_EXACT = T.Case('up_exact', 'exact', conv(8, 3, 0, 'relu') + pool() + conv(16, 3, 0, 'linear') + pool() + conv(32, 3, 0, 'relu') +
                  conv(16, 1, 0, 'linear') + up() + route(-1, 2) + conv(16, 3, 0, 'linear') + head(20), 2, 32, 32, 3, 3)

FLOAT = [UP_NET, UP_PAD, UP_SHARED, UP_S4, UP_INPUT, UP_LAST]
NETS = FLOAT + [UP_EXACT]
# {layer: form} Plan.upsample records for each net ('own' everywhere under SSP_UPSAMPLE_FUSE=0)
FORMS = {'up_net': {6: 'route'}, 'up_pad': {1: 'own'}, 'up_shared': {3: 'route'}, 'up_s4': {5: 'route'}, 'up_input': {0: 'own'},
         'up_last': {2: 'own'}, 'up_exact': {6: 'route'}}
# data seeds: find_seed(case) on the CPU (test_upsample_cpu.py re-checks the margins under them)
SEEDS = {'up_net': 1, 'up_pad': 0, 'up_shared': 0, 'up_s4': 2, 'up_input': 0, 'up_last': 0, 'up_exact': 0}

# (id, body, message pattern): what Plan refuses when it is built
REFUSED = [
    ('stride9', conv(8) + '[upsample]\nstride=9\n\n' + head(8), r'block 1 \(upsample\): stride=9 is outside 1\.\.8'),
    ('stride0', conv(8) + '[upsample]\nstride=0\n\n' + head(8), r'block 1 \(upsample\): stride=0 is outside 1\.\.8'),
    ('scale2', conv(8) + '[upsample]\nstride=2\nscale=2\n\n' + head(8), r'block 1 \(upsample\): scale=2'),
    ('flat', conv(8) + T.avgpool() + up() + T.connected(8), r'block 2 \(upsample\): its input is a flat \(B, 8\) map'),
    ('last6', conv(6) + up(), r'block 1 \(upsample\): the network output has 6 channels'),
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
    updated in place by a training pass).  Returns (y, {layer: output}).  absnet: the magnitude network of exact_budget
    (the caller passes |parameters| and |x|; identity activations, a max-pool whose backward hands the gradient to the whole
    window)."""
    outs = {}
    for ind, b in enumerate(blocks[1:]):
        t = b['type']
        if t == 'convolutional':
            cn = names[ind][0]
            k, s = int(b['size']), int(b['stride'])
            w, bias = params['%d.%s.weight' % (ind, cn)], params.get('%d.%s.bias' % (ind, cn))
            x = F.conv2d(x, w, bias, stride=s, padding=(k - 1) // 2 if int(b['pad']) else 0)
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
        elif t == 'upsample':
            x = F.interpolate(x, scale_factor=int(b.get('stride', 2)), mode='nearest')
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


def _one_ref(model, case, dseed, dtype, taps_eval=None, taps_train=None, absnet=False):
    x = make_input(case, dseed)
    names, params, bufs = model_state(model, dtype)
    with torch.no_grad():
        y_eval = ref_forward(model.blocks, names, params, bufs, x.to(dtype), False, taps_eval)[0]
    xr = x.to(dtype).requires_grad_(True)
    y, _ = ref_forward(model.blocks, names, params, bufs, xr, True, taps_train)
    (y * make_probe(case, dseed, y.shape).to(dtype)).sum().backward()
    grads = {'models.' + n: (None if p.grad is None else p.grad.detach()) for n, p in params.items()}
    stats = {'models.' + n: b for n, b in bufs.items()}
    return Ref(y_eval.detach(), y.detach(), xr.grad.detach(), grads, stats)


@functools.lru_cache(maxsize=None)
def reference(case, dseed):
    """(float64 run, float32 run): eval output, training output, dL/dx and every parameter gradient of
    (y_train * probe).sum(), running statistics after that training forward.  Computed once, shared, never written."""
    model = make_model(case)
    return _one_ref(model, case, dseed, torch.float64), _one_ref(model, case, dseed, torch.float32)


def margins(case, dseed):
    """topology_cases.margins on this module's reference: (smallest decision margin, largest float32-against-float64
    forward difference), relative to their layer's largest magnitude, over the eval and the training forward.  The
    upsample block decides nothing; it replicates decisions made before it, which are tapped where they are made."""
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
    order (topology_cases.exact_budget on this module's reference; the upsample's backward window sum is part of it: the
    magnitude network's gradient of the coarse map is the sum of the window's magnitudes)."""
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

"""Execution plan for a Darknet cfg on the HIP kernels (libssp_hip.so).

Walks the block list the way Darknet.forward does (/root/reference/darknet.py:82-130) but emits kernel launches
through the C ABI instead of torch.nn modules.  Activations live in NHWC fp32 buffers owned by torch (allocated once
per input shape and reused every step); every launch goes to torch's current HIP stream.

Forward per conv block (darknet.py:145-167):
    repack filters -> ssp_conv_fwd (MFMA implicit GEMM, BN partial statistics in the epilogue)
    -> ssp_bn_fwd_finalize (train) | ssp_bn_eval_prepare (eval) -> ssp_bn_act_fwd (BN + leaky [+ fused 2x2 max-pool])
A max-pool block is fused into the preceding conv block when nothing else consumes the un-pooled map.
route = alias or ssp_copy_channels into a concat buffer; reorg = ssp_reorg.
upsample = ssp_upsample_fwd / ssp_upsample_bwd (csrc/upsample.hip): nearest-neighbour replication, written straight into the
concatenation buffer of the two-layer route behind it when that route is its only consumer (Plan.upsample).
A [convolutional] block with groups = channels = filters (depthwise 3x3, stride 1 or 2) runs ssp_dwconv_fwd / _dgrad / _wgrad
(csrc/conv_depthwise.hip) on the (C, 1, 3, 3) parameter itself, inside the same BatchNorm / activation / pool chain (Plan.depthwise).
The other Darknet blocks (darknet.py:8-47, :107-118, :168-229) run on csrc/generic_blocks.hip: stride-1 max-pool, shortcut,
global average pool, softmax over channels; a connected block is planned as a 1x1 convolution of its (B, Cin) input on a 1x1
map (M = B rows: the conv kernels, bias and activation path of a non-BN conv block).

Backward mirrors it in reverse: ssp_bn_act_bwd (in place over the raw conv output) -> ssp_conv_wgrad ->
ssp_unpack_grad, and ssp_conv_dgrad into the producer's gradient buffer (accumulating when a map has two consumers).

Every BatchNorm block runs in its own module's mode (a trunk in eval() under model.train()), and a backward runs only what
the parameters that want a gradient need: Plan.backward_schedule lists, per executed op, which launches that is; blocks
no backward visits take the forward chain of a pass without gradient bookkeeping.
"""
import collections
import os
import weakref

import torch

from . import _lib
from .cfg import layer_shapes, resolve_layers, upsample_stride

from .tuning import (BF16X3, BN_EPS, BN_MOMENTUM, CONV_MATHS, IGEMM_CANDS, IGEMM_LATENCY_CANDS, TUNE_REJECTED,  # noqa: F401
                     WGRAD_FUSED, WINO, WINO4, WINO_GEMM_CANDS, WINOF, _HEAD_BUDGET_CACHE, _HEAD_BUDGET_PINNED, _TUNE_CACHE,
                     _TUNE_CACHE_FILE, _TUNE_FAMILY, _TUNE_VERIFIED, _TUNE_VERIFIED_ALSO, _pad4, _tune_cache_load, _tune_cache_save,
                     _tune_tag, conv_math_env, conv_math_of, form_allowed, knobs, tune_convs, tune_wgrad, wino_fused, wino_tile, x3_key,
                     x3_wino, x3_wino_key)
# (tuning.py holds the plan codes, the process-wide tune state and the passes that choose the codes; bench.py, the tests and
# the tools reach them as engine.X - the same objects)

# A layer whose data gradient AND filter gradient both run in the through-memory Winograd domain of one tile size takes the
# data gradient in its adjoint form (ssp_conv_dgrad_adj): it contracts the dM = A dY A^T planes the filter gradient
# transforms dY into anyway, so dY is transformed once per step instead of twice.  A rule of the plan, like the shared V -
# not a tuner choice, no plan code, not part of the tune tag.  SSP_WINO_SHARE_DM=0 (read once) switches it off for A/Bs.
_SHARE_DM = os.environ.get('SSP_WINO_SHARE_DM', '1') != '0'

# bumped by writers that change parameter memory without going through torch ops (singleshotpose_amd.optim.SGD's
# fused launch): part of the packed-filter cache key
_WEIGHTS_EPOCH = [0]


def _storage_refs(t):
    """Reference count of t's storage (the tensor itself, every live view of it, the Python storage wrapper), or None
    when this torch build does not expose it."""
    fn = getattr(torch._C, '_storage_Use_Count', None)
    return fn(t.untyped_storage()._cdata) if fn is not None else None


def _storage_shared(t, refs_alone, params):
    """True when something besides `t` itself still views t's storage (refs_alone = _storage_refs(t) right after t was
    allocated).  Without the storage counter: true when a parameter's .grad aliases it (views held elsewhere are then
    not seen: the conservative answer would cost a 202 MB allocation per backward)."""
    refs = _storage_refs(t)
    if refs is not None and refs_alone is not None:
        return refs != refs_alone
    sp = t.untyped_storage().data_ptr()
    return any(p.grad is not None and p.grad.untyped_storage().data_ptr() == sp for p in params)


_SIDE_STREAMS = {}


def _side_stream(device):
    """The second stream (filter repacks / transforms in forward, filter gradients in backward), at the HIGH HIP stream
    priority: its launches then win the dispatch slots that free up next to the main stream's, which shortened the step by
    0.2-0.3 ms (0.6 %) in two interleaved A/B rounds (profiles/r03_step_ab_winograd.txt).  SSP_SIDE_PRIORITY=0 restores the
    runtime's default (the device offers 0 and -1).

    ONE per device and process, shared by every plan, and created as early as possible (dist.init_distributed creates it
    BEFORE the RCCL process group): HIP multiplexes its streams over a few hardware queues (GPU_MAX_HW_QUEUES, 4 by
    default) in creation order, and a side stream created after RCCL's own streams landed on the main stream's queue -
    the two chains then ran one after the other instead of side by side (single-rank rehearsal, profiles/r04_rccl_queues.txt:
    forward 12.1 ms with no two kernels ever overlapping against 10.1 ms, step 35.7 ms against 28.7 ms)."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device, priority=int(os.environ.get('SSP_SIDE_PRIORITY', '-1')))
    return st


def weights_changed():
    _WEIGHTS_EPOCH[0] += 1


def _is_packed(wt, cinp):
    """True when the (Cout,Cin,kh,kw) parameter is stored channels-last, i.e. [Cout][kh][kw][Cin] in memory with no channel
    padding needed: that is the forward operand layout and the layout the filter gradient is accumulated in, so the
    kernels read / write the parameter (and its gradient) in place."""
    if wt.dim() == 2:      # nn.Linear weight (Cout, Cin): the same bytes as a channels-last (Cout, Cin, 1, 1) filter
        return wt.size(1) == cinp and wt.is_contiguous()
    return wt.size(1) == cinp and wt.permute(0, 2, 3, 1).is_contiguous()


def _ptr(t, offset=0):
    return t.data_ptr() + 4 * offset


def choose_under_budget(table, budget):
    """The error-aware choice of Plan._apply_head_budget, as a pure function (tests/test_host.py).

    table: {layer: [(family, plan code, launch ms, head deviation), ...]} - the candidates of every layer, FASTEST FIRST, the
    direct code (deviation 0 by definition: it is the reference the deviations are measured against) among them.  The
    deviations of different layers are independent roundings and add in quadrature.  Starting from the fastest candidate
    everywhere, the layer that buys the most squared deviation per millisecond is moved to its next more accurate candidate
    until sqrt(sum d^2) <= budget (or nothing is left to move).  Returns ({layer: index into its list}, [(layer, family
    left, family taken), ...])."""
    choice = {i: 0 for i in table}
    moved = []
    total = lambda: sum(table[i][choice[i]][3] ** 2 for i in table) ** 0.5
    while total() > budget:
        best, gain = None, 0.0
        for i, rows in table.items():
            k = choice[i]
            for k2 in range(k + 1, len(rows)):
                if rows[k2][3] < rows[k][3]:      # the next candidate that is actually more accurate
                    dt = max((rows[k2][2] or 0.0) - (rows[k][2] or 0.0), 1e-6)
                    g = (rows[k][3] ** 2 - rows[k2][3] ** 2) / dt
                    if g > gain:
                        best, gain = (i, k2), g
                    break
        if best is None:
            break
        moved.append((best[0], table[best[0]][choice[best[0]]][0], table[best[0]][best[1]][0]))
        choice[best[0]] = best[1]
    return choice, moved


_SLOPES = {'leaky': 0.1, 'linear': 1.0, 'relu': 0.0}      # negative-side slope of each supported activation


class _Act(object):
    """A [pixels][ld] fp32 view: tensor + channel offset.

    producer: the layer whose gradient buffer (Plan.grads) receives this map's gradient - the FIRST layer whose forward
    output it is (Plan._place): a fused 2x2 pool's output belongs to the pool, a one-layer route (or a region block) passes
    its source's map on and keeps its producer; INPUT (-1) for the network input.  flat: the reference holds this map as a 2-D
    (B, C) tensor (avgpool, connected, and softmax / shortcut / route of those)."""
    __slots__ = ('t', 'off', 'C', 'H', 'W', 'ld', 'flat', 'producer')

    def __init__(self, t, off, C, H, W, ld, flat=False):
        self.t, self.off, self.C, self.H, self.W, self.ld = t, off, C, H, W, ld
        self.flat = flat
        self.producer = None

    @property
    def ptr(self):
        return _ptr(self.t, self.off)


INPUT = -1      # Plan.grads key (and _Act.producer) of the network input's gradient

# One executed op of a backward pass (Plan.backward_schedule): `visited` = the op gets backward launches at all; `dgrad` =
# per input map, whether a gradient is written into its producer; for conv blocks the filter gradient, the bias column sum,
# which BatchNorm-parameter gradients are handed out, whether the BatchNorm-backward reductions run, and whether the
# block's data gradient folds its producer's BatchNorm-backward sums (ssp_conv_dgrad_bnbwd).
OpSchedule = collections.namedtuple('OpSchedule', 'ind kind visited dgrad wgrad bias dgamma dbeta bn_reduce fold_bn')


class _Op(object):
    """One executed block other than a conv / connected block (those are _ConvSpec records): its kind ('maxpool',
    'maxpool_s1', 'reorg', 'upsample', 'shortcut', 'avgpool', 'softmax', 'alias' = one-layer route or stride-1 upsample,
    'concat'), layer index, input maps, output map and, for a shortcut, the activation's slope; for an upsample `stride`; for
    a concat `inplace` = its first source is an upsample that writes its columns of the buffer itself (Plan.upsample)."""
    __slots__ = ('kind', 'ind', 'srcs', 'out', 'slope', 'stride', 'inplace')

    def __init__(self, kind, ind, srcs, out, slope=None, stride=None):
        self.kind, self.ind, self.srcs, self.out, self.slope = kind, ind, srcs, out, slope
        self.stride, self.inplace = stride, False

    @property
    def oind(self):
        """Layer index holding the output (acts / grads entry)."""
        return self.ind


class _ConvSpec(object):
    """One conv block of a plan.  `raw` (the block's raw conv output, kept for backward) is allocated on first use: the
    fused first block (csrc/conv_first.hip) recomputes its convolution in every pass and never touches it - 1.42 GB at
    batch 64, 416 x 416 that a plan (and the plan cache's memory budget) does not have to carry."""
    kind = 'conv'
    _raw = None
    _raw_spec = None     # (allocator, floats, tensor kwargs)
    plan_fwd = plan_dgrad = 0      # explicit igemm plan codes (0 = library heuristic): changed through Plan.set_code alone
    # set later, by the tuner, the first forward / backward or _plan_bn_fusion
    wbuf = gbuf = None             # forward-operand / filter-gradient staging of a parameter that is not channels-last
    wino_u = wino_ud = None        # {tile: Winograd-transformed forward / data-gradient filters}
    wino_ws = wino_ws_floats = None    # per-layer workspace of a Winograd filter gradient, and its size
    wgrad_wino = 0                 # filter gradient: 0 = direct, else the Winograd tile (or WGRAD_FUSED)
    dgrad_adj = False              # data gradient in the adjoint form, from the filter gradient's dM (_adjoint_rule)
    ws_dgrad = 0                   # split-K workspace floats of the data-gradient plan
    fwd_fams = None                # {family: (code, ms)} the head-error budget chooses from
    x3_fwd = x3_dgrad = 0          # bf16x3 mode: the code the tuner admitted for the launch (0 = its fp32 code stays)
    x3w_fwd = x3w_dgrad = None     # bf16x3-wino mode: {Winograd tile: the twin code the tuner admitted for that family, or 0}
    fp32_fwd = fp32_dgrad = None   # ... and the fp32 code a substituted launch goes back to (None = not substituted)
    stats = None                   # per-tile BatchNorm partial statistics
    first_fused = False
    first_partial = first_wpart = None     # fused first block: BatchNorm / filter-gradient partials
    bnp = bn_fuse_src = None       # BatchNorm-backward sums folded into the consumer's dgrad (_plan_bn_fusion)
    v_live = False                 # the forward left the transformed input V in wino_ws for the filter gradient
    packed = False                 # the parameter is channels-last: used (and its gradient accumulated) in place
    bn_train = False               # the last forward normalised this block with batch statistics (its BatchNorm's own mode)
    has_raw = False                # ... and left the raw conv output behind (what a backward through the block needs)
    fsched = None                  # the block's OpSchedule of the last forward that kept gradient bookkeeping
    depthwise = False              # groups = channels = filters, 3x3: csrc/conv_depthwise.hip on the parameter's own memory -
                                   # no packed / transformed operand, no plan code, no tuner entry (as a stride-2 block)

    @property
    def oind(self):
        """Layer index holding the output (acts / grads entry): the fused pool's, when there is one."""
        return self.ind + 1 if self.pool else self.ind

    @property
    def raw(self):
        if self._raw is None:
            alloc, n, kw = self._raw_spec
            self._raw = alloc(n, **kw)
        return self._raw


class Plan(object):
    """Buffers + launch sequence for one (batch, height, width) input shape."""

    def __init__(self, net, B, H, W, device):
        self.net = net
        self.B, self.H, self.W = B, H, W
        self.device = device
        # conv math of this plan, fixed when it is built: the model's attribute (Darknet.conv_math), else SSP_CONV_MATH.
        # The record of what the mode did (Plan._apply_conv_math): layers = {layer: (forward code, data-gradient code)} of
        # the blocks that run a bf16x3 launch, head_deviation = what those add at the head (fraction of its range),
        # taken_back = layers the head budget sent back to fp32
        mode = getattr(net, 'conv_math', None) or conv_math_env()
        if mode not in CONV_MATHS:
            raise ValueError("conv_math %r: expected one of %s" % (mode, ', '.join(CONV_MATHS)))
        self.conv_math = dict(mode=mode, layers={}, head_deviation=0.0, taken_back=[])
        self._cm_done = False
        # bitwise-reproducible training mode of this plan, fixed when it is built: the model's attribute
        # (Darknet.deterministic), else SSP_DETERMINISTIC.  On: every gradient launch whose sum order the hardware would
        # decide runs its ordered form.  The record (Plan._det_record): layers = {layer: {'wgrad':
        # (form, route or tile, pixel ranges), 'dgrad': form, 'bn_sums': where the block's BatchNorm-backward sums come
        # from}}, taken_back = [(layer, what)] fusions the mode undid
        det = getattr(net, 'deterministic', None)
        self.deterministic = dict(mode=bool(knobs().deterministic if det is None else det), layers={}, taken_back=[])
        self._wgrad_ws = None      # slabs of the ordered direct filter gradients: one buffer, they share a stream
        blocks = net.blocks
        self.shapes = layer_shapes(blocks, W, H)  # (w, h, c) per layer
        nl = len(blocks) - 1
        self.nl = nl

        # ---- consumer analysis (who reads layer l's output) ----
        consumers = [[] for _ in range(nl)]
        for ind, block in enumerate(blocks[1:]):
            t = block['type']
            if t in ('convolutional', 'maxpool', 'reorg', 'upsample', 'avgpool', 'softmax', 'connected'):
                if ind > 0:
                    consumers[ind - 1].append(ind)
            elif t == 'route':
                for l in resolve_layers(block['layers'], ind):
                    consumers[l].append(ind)
            elif t == 'shortcut':
                # reads `from` and ind-1 (the same map twice for from = -1): a shortcut source has two consumers, which keeps
                # it out of the single-consumer fusions (pool into the producing block, BN-backward sums into a dgrad)
                if ind == 0:
                    raise NotImplementedError("shortcut as the first block (it needs two earlier layers)")
                consumers[resolve_layers(block['from'], ind)[0]].append(ind)
                consumers[ind - 1].append(ind)
            elif t in ('region', 'cost'):
                pass
            else:
                raise NotImplementedError(
                    "block type '%s' is outside the yolo-pose hot path (SURVEY.md section 8); not built" % t)
        self.consumers = consumers
        # the network output is the last non-region layer
        self.last = max(i for i, b in enumerate(blocks[1:]) if b['type'] not in ('region', 'cost'))

        f32 = dict(dtype=torch.float32, device=device)
        in_c = int(blocks[0].get('channels', 3))
        self.in_c = in_c
        self.in_cp = _pad4(in_c)
        self.x_nhwc = torch.empty(B * H * W * self.in_cp, **f32)
        # (C = the real channel count: a first block that reads C - reorg, softmax - must not see the padding channel)
        self.input_act = _Act(self.x_nhwc, 0, in_c, H, W, self.in_cp)
        self.input_act.producer = INPUT
        self._dpack_in = None     # first conv's data-gradient operand [in_cp][k*k][coutp]: only plans asked for dL/dx

        self.convs = {}      # layer index -> _ConvSpec
        self.fused_pool = set()   # maxpool layers folded into the preceding conv block
        # the form each upsample block took: 'route' = its output IS columns [0, C) of the concatenation buffer of the
        # two-layer route behind it (no copy of the fine map in either direction), 'own' = a buffer of its own,
        # 'alias' = stride 1, nothing to run.  SSP_UPSAMPLE_FUSE=0 (read when the plan is built) forces 'own' (A/B runs)
        self.upsample = {}
        up_fuse = os.environ.get('SSP_UPSAMPLE_FUSE', '1') != '0'
        route_buf = {}            # route layer -> the concatenation buffer its upsample source already writes into
        self.acts = [None] * nl   # forward outputs
        self.ops = []        # one record per executed block (_ConvSpec or _Op), in forward order; backward runs it reversed
        wsz = dsz = 0
        prev = self.input_act
        for ind, block in enumerate(blocks[1:]):
            t = block['type']
            w, h, c = self.shapes[ind]
            zeros_or_empty = torch.empty if _pad4(c) == c else torch.zeros     # padding channels stay zero
            if t in ('convolutional', 'connected'):
                groups = 1
                if t == 'convolutional':
                    k, s = int(block['size']), int(block['stride'])
                    groups = int(block.get('groups', 1))
                    if groups != 1:
                        # depthwise 3x3 (csrc/conv_depthwise.hip) is the one grouped convolution that is built
                        cin_ = in_c if prev is self.input_act else prev.C
                        why = None
                        if groups != cin_:
                            why = "groups=%d on a %d-channel map (only groups=1 and the depthwise groups=%d are built)" % (
                                groups, cin_, cin_)
                        elif c != cin_:
                            why = "a depthwise convolution with filters=%d on %d channels (a channel multiplier is not built)" % (
                                c, cin_)
                        elif k != 3 or not int(block['pad']):
                            why = "a depthwise convolution with size=%d pad=%s (only size=3 pad=1 is built)" % (k, block['pad'])
                        elif prev is self.input_act:
                            why = ("a depthwise convolution on the network input (the first block's kernels are dense; "
                                   "csrc/conv_depthwise.hip serves every later position)")
                        elif cin_ % 4:
                            why = "a depthwise convolution on a %d-channel map (ssp_dwconv_fwd needs a multiple of 4)" % cin_
                        elif s not in (1, 2):
                            why = "a depthwise convolution with stride=%d (1 or 2)" % s
                        if why is not None:
                            raise NotImplementedError("block %d (convolutional): %s" % (ind, why))
                    if s not in (1, 2) or k not in (1, 3) or (k == 3 and not int(block['pad'])):
                        raise NotImplementedError("conv size=%d stride=%d pad=%s is outside the yolo-pose hot path" % (k, s, block['pad']))
                    if s == 2 and prev is self.input_act:
                        # the first block runs on the 4-channel kernel family of its own (csrc/conv_first.hip), stride 1 only
                        raise NotImplementedError("block %d (convolutional): a stride-2 convolution on the network input "
                                                  "(the first block's kernels are stride 1; csrc/conv_strided.hip serves "
                                                  "every later position)" % ind)
                    bn = int(block['batch_normalize']) != 0
                    seq = net.models[ind]
                    conv, bnm = seq[0], (seq[1] if bn else None)
                else:
                    # connected (darknet.py:215-229): nn.Linear(prev_filters, out) only works on a (B, Cin) input, i.e. after a
                    # 1x1 map; its (Cout, Cin) weight has the bytes of a channels-last (Cout, Cin, 1, 1) filter, so it runs as
                    # a 1x1 convolution with M = B rows
                    if prev.H != 1 or prev.W != 1:
                        raise NotImplementedError("connected block %d on a %d x %d map: nn.Linear needs a (B, C) input - put "
                                                  "an avgpool (or a 1x1 map) in front of it" % (ind, prev.H, prev.W))
                    k, s, bn, bnm = 1, 1, False, None
                    m = net.models[ind]
                    conv = m[0] if isinstance(m, torch.nn.Sequential) else m
                cs = _ConvSpec()
                cs.ind, cs.k, cs.stride = ind, k, s
                cs.bn = bn
                act = block['activation']
                if act not in _SLOPES:
                    raise NotImplementedError("activation '%s'" % act)
                cs.slope = _SLOPES[act]
                cs.inp = prev
                cs.first = prev is self.input_act
                cs.cin = in_c if cs.first else prev.C
                cs.cinp = _pad4(cs.cin)
                cs.cout = c
                cs.depthwise = groups != 1
                if conv.weight.shape[1] * groups != cs.cin or getattr(conv, 'groups', 1) != groups:
                    raise NotImplementedError("block %d (%s): its parameter takes %d input channels in %d group(s) but the map "
                                              "it is given has %d (cfg groups=%d)" % (ind, t, conv.weight.shape[1] * getattr(
                                                  conv, 'groups', 1), getattr(conv, 'groups', 1), cs.cin, groups))
                if prev.ld < cs.cinp:
                    raise NotImplementedError("block %d (%s): its %d-channel input map has a row stride of %d floats, narrower "
                                              "than the padded channel count %d" % (ind, t, cs.cin, prev.ld, cs.cinp))
                # Hi x Wi: the map the block reads; H x W: the map its convolution writes (raw output, BatchNorm / activation /
                # fused pool input, M pixels).  The two differ for a stride-2 block only (csrc/conv_strided.hip).
                cs.Hi, cs.Wi = prev.H, prev.W
                cs.H, cs.W = (h, w) if s == 2 else (prev.H, prev.W)
                if s == 2 and (cs.H, cs.W) != ((cs.Hi + 2 * (k // 2) - k) // 2 + 1, (cs.Wi + 2 * (k // 2) - k) // 2 + 1):
                    raise NotImplementedError("block %d (convolutional): layer_shapes gives a %d x %d output for a %d x %d "
                                              "input at stride 2" % (ind, w, h, cs.Wi, cs.Hi))
                cs.coutp = _pad4(c)
                cs.conv, cs.bnm = conv, bnm
                # fuse a following 2x2/2 max-pool when it is the only consumer
                nxt = blocks[ind + 2] if ind + 2 < len(blocks) else None
                cs.pool = bool(cs.bn and nxt is not None and nxt['type'] == 'maxpool' and int(nxt['size']) == 2 and
                               int(nxt['stride']) == 2 and consumers[ind] == [ind + 1] and cs.H % 2 == 0 and cs.W % 2 == 0)
                M = B * cs.H * cs.W
                cs.M = M
                alloc = torch.empty if cs.coutp == c else torch.zeros
                cs._raw_spec = (alloc, M * cs.coutp, f32)      # raw conv output (kept for backward), see _ConvSpec.raw
                cs.ldraw = cs.coutp
                cs.needs_act = cs.bn or cs.slope != 1.0
                if cs.needs_act:
                    Ho, Wo = (cs.H // 2, cs.W // 2) if cs.pool else (cs.H, cs.W)
                    cs.out = _Act(alloc(B * Ho * Wo * cs.coutp, **f32), 0, c, Ho, Wo, cs.coutp)
                else:
                    cs.out = _Act(cs.raw, 0, c, cs.H, cs.W, cs.coutp)
                cs.out.flat = t == 'connected'
                # per-channel vectors: mean, invstd, scale, shift, c1, c2, dgamma, dbeta
                cs.vec = torch.zeros(8, cs.coutp, **f32)
                if not cs.bn:
                    cs.vec[1].fill_(1.0)
                    cs.vec[2].fill_(1.0)
                cs.woff, cs.doff = wsz, dsz
                wsz += c * k * k * cs.cinp
                dsz += cs.cinp * k * k * cs.coutp if not (cs.first or cs.depthwise) else 0
                self.convs[ind] = cs
                if cs.pool:
                    self.fused_pool.add(ind + 1)
                op = cs
            elif t == 'maxpool':
                if ind in self.fused_pool:
                    continue        # prev is the conv block's pooled output
                k, s = int(block['size']), int(block['stride'])
                # s == 1: MaxPoolStride1 (darknet.py:8-14): 2x2 window over the right / bottom replicate-padded map, H x W
                # out; the cfg's size is ignored, as in the reference
                if s != 1 and (k != 2 or s != 2):
                    raise NotImplementedError("maxpool size=%d stride=%d (MaxPoolStride1, darknet.py:8-14) is not instantiated by the pose cfgs; not built" % (k, s))
                if s == 2 and (prev.H % 2 or prev.W % 2):
                    # (a pool fused into its BatchNorm block never gets here; the fusion itself needs an even map)
                    raise NotImplementedError("block %d (maxpool): a standalone 2x2/2 max-pool of a %d x %d map "
                                              "(ssp_maxpool_fwd needs even H and W)" % (ind, prev.W, prev.H))
                op = _Op('maxpool_s1' if s == 1 else 'maxpool', ind, [prev],
                         _Act(torch.empty(B * h * w * prev.ld, **f32), 0, c, h, w, prev.ld))
            elif t == 'reorg':
                if int(block['stride']) != 2:
                    raise NotImplementedError("reorg stride != 2")
                if prev.C % 4:
                    raise NotImplementedError("reorg of a %d-channel map (ssp_reorg needs a multiple of 4)" % prev.C)
                if prev.H % 2 or prev.W % 2:
                    raise NotImplementedError("block %d (reorg): reorg of a %d x %d map (ssp_reorg needs even H and W)"
                                              % (ind, prev.W, prev.H))
                op = _Op('reorg', ind, [prev], _Act(torch.empty(B * h * w * c, **f32), 0, c, h, w, c))
            elif t == 'upsample':
                n = upsample_stride(block, ind)       # (refuses scale != 1 by name; layer_shapes above already did)
                if not 1 <= n <= 8:
                    raise NotImplementedError("block %d (upsample): stride=%d is outside 1..8 (ssp_upsample_fwd)" % (ind, n))
                if prev.flat:
                    raise NotImplementedError("block %d (upsample): its input is a flat (B, %d) map (behind avgpool / "
                                              "connected); there is no H x W to replicate" % (ind, prev.C))
                if n == 1:
                    self.upsample[ind] = 'alias'
                    op = _Op('alias', ind, [prev], prev)
                else:
                    # write-through: the only consumer is the two-layer route right behind it (one block of look-ahead, as
                    # cs.pool does), both of its sources have whole channel quads and the lateral map has the fine shape
                    nxt = blocks[ind + 2] if ind + 2 < len(blocks) else None
                    lat = None
                    if up_fuse and nxt is not None and nxt['type'] == 'route' and consumers[ind] == [ind + 1]:
                        layers = resolve_layers(nxt['layers'], ind + 1)
                        if len(layers) == 2 and layers[0] == ind and 0 <= layers[1] < ind:
                            lat = self.acts[layers[1]]
                    if lat is not None and c % 4 == 0 and lat.C % 4 == 0 and (lat.H, lat.W) == (h, w) and not lat.flat:
                        ct = c + lat.C
                        buf = route_buf[ind + 1] = torch.empty(B * h * w * ct, **f32)
                        out = _Act(buf, 0, c, h, w, ct)
                        self.upsample[ind] = 'route'
                    else:
                        out = _Act(zeros_or_empty(B * h * w * _pad4(c), **f32), 0, c, h, w, _pad4(c))
                        self.upsample[ind] = 'own'
                    op = _Op('upsample', ind, [prev], out, stride=n)
            elif t == 'shortcut':
                f = resolve_layers(block['from'], ind)[0]
                a, b = self.acts[f], prev
                if a is None:
                    raise RuntimeError("shortcut from a layer whose output was fused away")
                if (a.C, a.H, a.W) != (b.C, b.H, b.W):
                    raise NotImplementedError("shortcut %d adds layer %d (%d x %d x %d) to layer %d (%d x %d x %d): the "
                                              "maps must have the same shape" % (ind, f, a.W, a.H, a.C, ind - 1, b.W, b.H, b.C))
                act = block['activation']
                if act not in _SLOPES:
                    raise NotImplementedError("shortcut activation '%s'" % act)
                out = _Act(zeros_or_empty(B * h * w * _pad4(c), **f32), 0, c, h, w, _pad4(c), b.flat)
                op = _Op('shortcut', ind, [a, b], out, _SLOPES[act])
            elif t == 'avgpool':
                # GlobalAvgPool2d (darknet.py:37-47): (B, H, W, C) -> (B, C), a 1x1 map downstream
                op = _Op('avgpool', ind, [prev], _Act(zeros_or_empty(B * _pad4(c), **f32), 0, c, 1, 1, _pad4(c), True))
            elif t == 'softmax':
                # nn.Softmax() (darknet.py:181-184): implicit dim 1 = the channels of each (B, C) row or NHWC pixel
                out = _Act(zeros_or_empty(B * h * w * _pad4(c), **f32), 0, c, h, w, _pad4(c), prev.flat)
                op = _Op('softmax', ind, [prev], out)
            elif t == 'route':
                layers = resolve_layers(block['layers'], ind)
                if len(layers) > 2:
                    raise NotImplementedError("block %d (route): %d layers (the reference's darknet.py:99-106 handles one "
                                              "or two)" % (ind, len(layers)))
                if len(layers) == 2 and layers[0] != ind - 1:
                    raise NotImplementedError("block %d (route): the first of two layers must be the previous layer "
                                              "(darknet.py:206), got %d" % (ind, layers[0]))
                srcs = [self.acts[l] for l in layers]
                if any(s is None for s in srcs):
                    raise RuntimeError("route to a layer whose output was fused away")
                if len(layers) == 1:
                    op = _Op('alias', ind, srcs, srcs[0])
                else:
                    for l, s in zip(layers, srcs):
                        if s.C % 4:
                            raise NotImplementedError("block %d (route): concatenates layer %d with %d channels "
                                                      "(ssp_copy_channels needs multiples of 4)" % (ind, l, s.C))
                    buf = route_buf.get(ind)
                    op = _Op('concat', ind, srcs, _Act(torch.empty(B * h * w * c, **f32) if buf is None else buf, 0, c, h, w, c,
                                                       srcs[0].flat))
                    op.inplace = buf is not None      # (srcs[0] is columns [0, srcs[0].C) of buf already)
            else:  # region / cost: not executed in forward (darknet.py:119-127)
                self._place(ind, prev)
                continue
            self.ops.append(op)
            self._place(op.oind, op.out)
            prev = op.out
        # the depthwise 3x3 blocks (csrc/conv_depthwise.hip), by layer: the record tools/show_plans.py prints
        self.depthwise = sorted(i for i, cs in self.convs.items() if cs.depthwise)
        self._dw_ws = None         # partial sums of the depthwise filter gradients: one buffer, they share a stream
        o = self.acts[self.last]
        if o.ld > o.C:
            # (the gradient of the output arrives NCHW and is laid out with ld = C by Plan.backward)
            raise NotImplementedError("block %d (%s): the network output has %d channels, not a multiple of 4"
                                      % (self.last, blocks[self.last + 1]['type'], o.C))
        # Filter staging buffers are allocated when first needed: channels-last parameters are used in place, so only the
        # padded first layer (or a filter a caller replaced by a plain contiguous tensor) gets a forward / gradient
        # staging copy, and the data-gradient operands (202 MB) exist only in plans that run a backward.
        self._dpack_floats = max(dsz, 1)
        self._dpack = None
        self._dgrad_tuned = False
        self._dgrad_fallback = False     # Plan.backward's no-tuning fallback made its choices (once per plan)
        self.bn_partial = torch.empty(_lib.query('ssp_bn_bwd_blocks') * 2 * max(cs.coutp for cs in self.convs.values()), **f32)
        self._tune = device.type == 'cuda' and knobs().autotune
        self._stale = set()        # what set_code changed since the last _settle: 'fwd' / 'dgrad'
        if self._tune:
            tune_convs(self, 'fwd')
        # statistics / split-K workspaces follow the (tuned or heuristic) plan of each launch
        for cs in self.convs.values():
            M = cs.M
            # First block in training mode: conv + BN + leaky + pool with the convolution recomputed by every pass
            # instead of stored (csrc/conv_first.hip): the 32-channel full-resolution map (1.42 GB at batch 64, the
            # largest tensor of the net, written and re-read five times by the generic path) never exists.
            cs.first_fused = bool(cs.first and cs.bn and cs.pool and cs.k == 3 and cs.cinp == 4 and cs.cout == 32 and
                                  cs.H % 2 == 0 and cs.W % 16 == 0 and M * 16 < (1 << 31) and
                                  (M // 4) * cs.out.ld * 4 < (1 << 31) and device.type == 'cuda' and
                                  os.environ.get('SSP_FIRST_FUSED', '1') != '0')
            cs.first_live = False        # the last forward took the fused path (its backward must as well)
            if cs.first_fused:
                cs.first_groups = _lib.query('ssp_first_groups', B, cs.H, cs.W)
                cs.first_tile = _lib.query('ssp_first_tile_pixels')
                cs.first_partial = torch.empty(cs.first_groups * 64, **f32)
            self._size_layer(cs)
        # split-K partial tiles (13x13 layers): one scratch buffer shared by every conv launch of the plan
        self.ws_floats = max([1] + [cs.ws_fwd for cs in self.convs.values()])
        self.ws = torch.empty(self.ws_floats, **f32)
        self._stale.clear()        # (everything above was sized for the tuned codes: nothing to settle)
        self._head_budget_done = False
        self._hb_gains = None
        self._hb_gains_after_forward = False
        self._hb_checked = 0
        self.head_budget = None      # record of Plan._apply_head_budget (what was measured, what was chosen)
        self.bn_momentum = BN_MOMENTUM
        self.wversion = {}
        self.wino_version = {}
        self.bnversion = {}
        self.generation = 0
        # flat gradient buffer layout, in backward (reverse layer) order so that all-reduce buckets close early:
        # per conv block: weight | bias  or  weight | bn.weight | bn.bias   (each 16-byte aligned)
        self.grad_layout = {}   # id(param) -> (offset, numel, shape)
        goff = 0
        for ind in sorted(self.convs.keys(), reverse=True):
            cs = self.convs[ind]
            plist = [cs.conv.weight]
            if cs.conv.bias is not None:
                plist.append(cs.conv.bias)
            if cs.bn:
                plist += [cs.bnm.weight, cs.bnm.bias]
            cs.grad_lo = goff
            for prm in plist:
                self.grad_layout[id(prm)] = (goff, prm.numel(), tuple(prm.shape))
                goff += (prm.numel() + 3) // 4 * 4
            cs.grad_hi = goff
        self.grad_total = goff
        self.reducer = None      # singleshotpose_amd.dist.GradReducer (multi-GPU): notified as layers finish
        self.side_stream = None
        self.serial_backward = False   # measurement aid (bench.py): filter gradients on the MAIN stream, so that every
                                       # backward launch runs alone and its HIP-event duration is kernel-exclusive
        self.dgrad_ready = None
        self.grads = {}      # layer index -> _Act gradient buffers, allocated on first backward
        self._schedules = {}     # backward schedules by what is trainable (_schedule)
        self.out_act = self.acts[self.last]
        self.out_flat = self.out_act.flat      # forward returns (B, C) instead of (B, C, h, w), as the reference
        self.consumed = False
        self._graph = self._graph_key = self._x_static = self._y_static = None
        self._graph_failed = False
        if self.deterministic['mode']:
            self._plan_bn_fusion()      # (what the record says about the BatchNorm sums; redone with the data-gradient codes)
            self._det_record()

    # ------------------------------------------------------------------ deterministic mode (SSP_DETERMINISTIC / Darknet.deterministic)
    def _wgrad_split(self, cs):
        """(form, route / tile, pixel ranges) of a layer's ordered filter gradient: pure host queries, the library's split -
        recorded here and passed to the launch explicitly."""
        B = self.B
        if cs.first_fused:
            return ('first-block', 0, _lib.query('ssp_first_groups', B, cs.H, cs.W))      # per-workgroup partials, float64 finalize
        if cs.depthwise:      # its only form: per-range partials, float64 finish (the ranges follow from the shape)
            return ('depthwise', 0, _lib.query('ssp_dwconv_wgrad_workspace_floats', B, cs.Hi, cs.Wi, cs.cin, cs.stride) // (9 * cs.cin))
        if cs.wgrad_wino:
            return ('winograd-ordered', cs.wgrad_wino,
                    _lib.query('ssp_conv_wgrad_wino_ordered_split', B, cs.H, cs.W, cs.cinp, cs.cout, cs.wgrad_wino, 0))
        args = (B, cs.Hi, cs.Wi, cs.cinp, cs.cout, cs.ldraw, cs.inp.ld, cs.k)
        route = (_lib.query('ssp_conv_wgrad_route', *args) if cs.stride == 1 else
                 200000000 + 30000000 + (128 if cs.cout > 64 else 64 if cs.cout > 32 else 32) * 1000 +
                 (128 if cs.cinp > 64 else 64 if cs.cinp > 32 else 32))
        return ('direct-ordered' if cs.stride == 1 else 'stride2-ordered', route,
                _lib.query('ssp_conv_wgrad_ordered_split', *(args + (cs.stride, 0))))

    def _det_record(self):
        rec = self.deterministic
        if not rec['mode']:
            return
        rec['layers'] = {}
        for i, cs in sorted(self.convs.items()):
            cs.wgrad_det = self._wgrad_split(cs)
            if cs.first:
                dg = 'first-block' if cs.first_fused else 'direct'
            elif cs.depthwise:
                dg = 'depthwise' if cs.stride == 1 else 'depthwise-stride2'      # one thread per element, no atomics
            elif cs.stride == 2:
                dg = 'stride2-ordered'
            else:
                dg = 'plan %d' % cs.plan_dgrad
            bn = None
            if cs.bn:
                bn = ('consumer-dgrad rows=%d' % cs.bnp[1]) if cs.bnp is not None else ('first-block' if cs.first_fused else 'two-level')
            rec['layers'][i] = dict(wgrad=cs.wgrad_det, dgrad=dg, bn_sums=bn)

    def _wino_ws_query(self, cs, t):
        """Workspace floats of the layer's Winograd filter gradient at tile value t (the ordered layout in the mode)."""
        if self.deterministic['mode']:
            return _lib.query('ssp_conv_wgrad_wino_ordered_workspace_floats', self.B, cs.H, cs.W, cs.cinp, cs.cout, t, 0)
        return _lib.query('ssp_conv_wgrad_wino_workspace_floats_t', self.B, cs.H, cs.W, cs.cinp, cs.cout, t)

    def _wgrad_ordered_ws(self):
        """The slabs of the ordered direct filter gradients, allocated on the first backward: sized for the largest layer -
        the launches of one backward are queued on one stream."""
        if self._wgrad_ws is None:
            need = max([1] + [_lib.query('ssp_conv_wgrad_ordered_workspace_floats', self.B, cs.Hi, cs.Wi, cs.cinp, cs.cout,
                                         cs.ldraw, cs.inp.ld, cs.k, cs.stride, 0)
                              for cs in self.convs.values() if not (cs.first_fused or cs.depthwise)])
            self._wgrad_ws = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._wgrad_ws

    def _dwconv_ws(self):
        """The per-range partial sums of the depthwise filter gradients (ssp_dwconv_wgrad), allocated on the first backward
        and sized for the largest layer: the launches of one backward are queued on one stream."""
        if self._dw_ws is None:
            need = max([1] + [_lib.query('ssp_dwconv_wgrad_workspace_floats', self.B, cs.Hi, cs.Wi, cs.cin, cs.stride)
                              for cs in self.convs.values() if cs.depthwise])
            self._dw_ws = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._dw_ws

    def _place(self, ind, act):
        """acts[ind] = act; the first layer to hold a map is its producer (see _Act)."""
        self.acts[ind] = act
        if act.producer is None:
            act.producer = ind

    def _size_layer(self, cs):
        """Statistics / split-K bookkeeping of one conv block for its CURRENT forward plan code (after tuning, and again
        when the error budget moves the layer to another family): tile height of the per-tile BatchNorm partials (0 = the
        counted format of a Winograd launch), their count, the launch's workspace need; the statistics buffer is sized
        for the largest format any timed family of the layer uses, so a plan change never re-allocates it."""
        B = self.B
        if cs.depthwise:         # no plan codes, no workspace: the counted format (tile_m = 0)
            cs.tile_m = _lib.query('ssp_dwconv_stats_tile_m', B, cs.Hi, cs.Wi, cs.cin, cs.stride)
            cs.ntile = _lib.query('ssp_dwconv_stats_tiles', B, cs.Hi, cs.Wi, cs.cin, cs.stride)
            cs.ws_fwd = 0
            if cs.bn and cs.stats is None:
                cs.stats = torch.empty(_lib.query('ssp_dwconv_stats_floats', B, cs.Hi, cs.Wi, cs.cin, cs.stride),
                                       dtype=torch.float32, device=self.device)
            return
        if cs.stride == 2:       # no plan codes, no workspace: one tile format (ssp_conv_s2_stats_tile_m)
            cs.tile_m = _lib.query('ssp_conv_s2_stats_tile_m', B, cs.Hi, cs.Wi, cs.cinp, cs.cout, cs.k)
            cs.ntile = _lib.query('ssp_conv_s2_stats_tiles', B, cs.Hi, cs.Wi, cs.cinp, cs.cout, cs.k)
            cs.ws_fwd = 0
            if cs.bn and cs.stats is None:
                cs.stats = torch.empty(cs.ntile * cs.cout * 2, dtype=torch.float32, device=self.device)
            return
        q = lambda name, code: _lib.query(name, B, cs.H, cs.W, cs.cinp, cs.cout, cs.k, code)
        cs.tile_m = q('ssp_conv_stats_tile_m', cs.plan_fwd)
        cs.ws_fwd = q('ssp_conv_workspace_floats', cs.plan_fwd)
        cs.ntile = q('ssp_conv_stats_tiles', cs.plan_fwd)
        codes = set([cs.plan_fwd, 0] + [c for c, _ in (cs.fwd_fams or {}).values()])
        nstat = max(q('ssp_conv_stats_floats', c) for c in codes)
        if cs.first_fused:
            nstat = max(nstat, cs.first_groups * 64)
        if cs.bn and (cs.stats is None or cs.stats.numel() < nstat):
            cs.stats = torch.empty(nstat, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ plan codes: one writer, one settle step
    def set_code(self, cs, which, code, fp32=None):
        """The one place a launch's code changes.  which = 'fwd' / 'dgrad': the plan code and the fp32 code a substituted launch
        goes back to (None = not substituted; kept for a bf16x3 code only: an fp32 code needs none); 'wgrad': the filter
        gradient's form (0 = direct, else the Winograd tile or WGRAD_FUSED).  What follows for the layer alone is done at
        once; what follows for the plan waits for _settle, which the caller runs once per group of writes."""
        if which == 'wgrad':
            if code != cs.wgrad_wino:
                cs.wgrad_wino = code
                if code:
                    cs.wino_ws_floats = self._wino_ws_query(cs, code)
                cs.wino_ws = None
                self._stale.add('dgrad')
            return
        fp32 = fp32 if conv_math_of(code) == 'bf16x3' else None
        if which == 'fwd' and (code, fp32) != (cs.plan_fwd, cs.fp32_fwd):
            cs.plan_fwd, cs.fp32_fwd = code, fp32
            self._size_layer(cs)
            self._stale.add('fwd')
        elif which == 'dgrad' and (code, fp32) != (cs.plan_dgrad, cs.fp32_dgrad):
            cs.plan_dgrad, cs.fp32_dgrad = code, fp32
            self._stale.add('dgrad')

    def _settle(self, dgrad=False):
        """Brings the plan-wide state up to date with the codes, once per group of set_code calls (a workspace that grows
        synchronises the stream).  After a data-gradient code or a filter-gradient form changed (dgrad=True: or on their
        first sizing): the split-K need of every data gradient and the BatchNorm-backward fusion, whose buffers follow the
        data-gradient tiles.  After a forward code changed or a transformed forward filter was released: a captured
        inference chain holds the old codes and pointers - the next forward_graph call captures again."""
        stale, self._stale = self._stale, set()
        if dgrad or 'dgrad' in stale:
            for cs in self.convs.values():
                cs.ws_dgrad = 0 if (cs.first or cs.stride == 2 or cs.depthwise) else _lib.query(
                    'ssp_conv_workspace_floats', self.B, cs.H, cs.W, cs.coutp, cs.cin, cs.k, cs.plan_dgrad)
            self._plan_bn_fusion()
        self._fit_workspace()
        if 'fwd' in stale:
            self._graph = None
        self._conv_math_record()
        self._det_record()

    def _release_filters(self, which, layers):
        """The transformed forward / data-gradient filters of the tile sizes a layer's launch is not on go back to the allocator:
        after the layer was tuned and at the end of _apply_head_budget (whose forwards re-use them); _settle follows."""
        for cs in layers:
            have = (cs.wino_u if which == 'fwd' else cs.wino_ud) or {}
            keep = {t: b for t, b in have.items() if t == wino_tile(cs.plan_fwd if which == 'fwd' else cs.plan_dgrad)}
            if which == 'fwd':
                cs.wino_u = keep
                if len(keep) < len(have):
                    self._stale.add('fwd')
            else:
                cs.wino_ud = keep

    def _apply_head_budget(self):
        """Error-aware admission of the forward plans: a NETWORK-level rounding budget, measured on the live batch.

        A Winograd F(4x4) launch carries ~2.5e-7 (rms, of the output's range) of rounding that no summation order removes
        - every M = sum_c U.V element is ONE fp32 number 3-4 x the size of the output it is cancelled into
        (tools/wino_error_budget.py) - against 4e-8 for the direct kernel with chunked accumulation and ~1e-7 for F(2x2).
        What that costs at the network output depends on WHERE the layer sits: BatchNorm re-normalises every block, so a
        perturbation of an early block's output is amplified layer after layer (measured in float64 on the CPU,
        tools/head_amplification.py: white noise of 1e-6 of the range on layer 4's raw output moves the head by 1.7e-4 of its
        range, on layer 23's by 6e-6) - F(4x4) on the 104 x 104 and 52 x 52 layers IS the head error of the step (6e-5 of
        the 1e-4 bar), F(4x4) on the 13 x 13 layers, where it saves the most time, costs nothing measurable.

        So, once per plan, on the first training batch: one forward with every eligible layer on its fastest DIRECT code
        gives the reference head; then, layer by layer, one forward with that layer alone on its Winograd candidate
        gives d_l = max|head - reference| / max|reference| - the head deviation that candidate is responsible for, on the
        live operands and weights.  The deviations of different layers are independent roundings: they add in quadrature.
        Starting from the fastest code everywhere, the layer with the largest (d^2 saved per millisecond lost) is moved to
        its next more accurate family (F(4x4) -> F(2x2) -> direct) until sqrt(sum d_l^2) <= SSP_HEAD_ERR_BUDGET (default
        3.5e-5 of the head's range; 0 = off: always the fastest code).  BatchNorm running statistics are not touched by the
        measurement forwards (momentum 0).  The record is kept in `plan.head_budget` (bench.py prints it)"""
        self._head_budget_done = True
        self._hb_gains = None
        self._hb_gains_after_forward = False
        self._hb_checked = self.generation
        budget = knobs().head_budget
        if budget <= 0 or not self._tune:
            return
        cand = [cs for cs in self.convs.values() if wino_tile(cs.plan_fwd) and 0 in (cs.fwd_fams or {})]
        if not cand:
            return
        # the NETWORK is part of the key: the deviations are properties of this stack of layers (another cfg at the same input
        # shape - tiny-pose against yolo-pose, the multi-object cfg - must not run under this one's budget decisions)
        import zlib
        net_fp = zlib.crc32(repr([(i, cs.cin, cs.cout, cs.k, cs.H, cs.W, bool(cs.bn), bool(cs.pool))
                                  for i, cs in sorted(self.convs.items())]).encode())
        ckey = (self.B, self.H, self.W, _tune_tag(), budget, id(self.net))
        pkey = (self.B, self.H, self.W, _tune_tag(), budget, net_fp)
        rec = _HEAD_BUDGET_CACHE.get(ckey)
        pinned = _HEAD_BUDGET_PINNED.get(pkey)
        if rec is None and pinned is not None and _TUNE_CACHE_FILE[0] and all(
                any(c == pinned.get(cs.ind) for c, _ in cs.fwd_fams.values()) for cs in cand):
            # (entry -1 of a pinned record: the measured deviation of the chosen plans, in units of 1e-12)
            rec = dict(budget=budget, head_deviation=pinned.get(-1, 0) * 1e-12 if -1 in pinned else float('nan'),
                       fastest={cs.ind: cs.plan_fwd for cs in cand}, chosen={i: c for i, c in pinned.items() if i >= 0},
                       cost_ms=float('nan'), moved=[(cs.ind, wino_tile(cs.plan_fwd), wino_tile(pinned[cs.ind])) for cs in cand
                                                    if pinned[cs.ind] != cs.plan_fwd], table={}, pinned=True)
            _HEAD_BUDGET_CACHE[ckey] = rec
        if rec is None:
            o = self.out_act
            head = lambda: o.t[o.off:o.off + self.B * o.H * o.W * o.ld].clone()
            fastest = {cs.ind: cs.plan_fwd for cs in cand}

            def run(assign):
                for cs in cand:
                    self.set_code(cs, 'fwd', assign[cs.ind])
                self._settle()
                self._forward_body(True, False, False, bn_force=True)
                return head()
            mom, self.bn_momentum = self.bn_momentum, 0.0
            try:
                direct = {cs.ind: cs.fwd_fams[0][0] for cs in cand}
                ref = run(direct)
                den = max(float(ref.abs().max()), 1e-30)
                table = {}         # layer -> [(family, code, ms, deviation)], fastest first; the direct entry has deviation 0
                for cs in cand:
                    rows = []
                    for f_, (c_, t_) in cs.fwd_fams.items():
                        if f_ == 0:
                            rows.append((0, c_, t_, 0.0))
                            continue
                        if t_ is not None and cs.fwd_fams[0][1] is not None and t_ >= cs.fwd_fams[0][1]:
                            continue      # slower than the direct code: never an option
                        assign = dict(direct)
                        assign[cs.ind] = c_
                        d = float((run(assign) - ref).abs().max()) / den
                        rows.append((f_, c_, t_, d))
                    # fastest first; the code the tuner actually chose (near-tie rule) leads among equals, so that `moved`
                    # and `cost_ms` describe moves the layer really makes
                    rows.sort(key=lambda r: (0 if r[1] == fastest[cs.ind] else 1, r[2] if r[2] is not None else 0.0))
                    table[cs.ind] = rows
            finally:
                self.bn_momentum = mom
            choice, moved = choose_under_budget(table, budget)
            total = lambda: sum(table[i][choice[i]][3] ** 2 for i in table) ** 0.5
            rec = dict(budget=budget, head_deviation=total(), fastest=fastest,
                       chosen={i: table[i][choice[i]][1] for i in table},
                       cost_ms=sum((table[i][choice[i]][2] or 0.0) - (table[i][0][2] or 0.0) for i in table),
                       moved=moved, table={i: [(f_, c_, None if t_ is None else round(t_, 4), float('%.3g' % d))
                                               for f_, c_, t_, d in rows] for i, rows in table.items()})
            _HEAD_BUDGET_CACHE[ckey] = rec
            if _TUNE_CACHE_FILE[0]:
                _HEAD_BUDGET_PINNED[pkey] = dict(rec['chosen'])
                _HEAD_BUDGET_PINNED[pkey][-1] = int(round(rec['head_deviation'] * 1e12))
                _tune_cache_save()
        for cs in cand:
            self.set_code(cs, 'fwd', rec['chosen'].get(cs.ind, cs.plan_fwd))
        self._release_filters('fwd', cand)
        self._settle()
        self.head_budget = rec
        # the amplification the decisions were measured under (head_budget_drifted).  A record adopted from the cache ran no
        # measurement forward here: the scale vectors of this batch exist only after the forward body (forward() takes them)
        self._hb_gains = None if rec.get('pinned') else self._bn_gains()
        self._hb_gains_after_forward = bool(rec.get('pinned'))

    # The deviations the budget admits a plan under are measured ONCE, on the weights and BatchNorm statistics of the plan's
    # first training batch - and the amplification of a layer's rounding on the way to the head is a product of BatchNorm gains
    # (|gamma| / sigma per block), which training moves.  Two triggers re-measure:
    #   * load_weights / load_weights_until_last (Darknet._load_blocks): another network as far as rounding goes;
    #   * every SSP_HEAD_BUDGET_EVERY (default 256) training forwards the largest |gamma * invstd| of every BatchNorm block is
    #     compared with its value at measurement time (one stacked reduction, one 88-byte read): a block that moved by more
    #     than 2x either way invalidates the record.  The re-measurement costs ~0.3 s (<= 27 forwards), like the first one.
    def head_budget_stale(self):
        if self._head_budget_done:
            self._head_budget_done = False
            self._conv_math_revert()         # (bf16x3 mode: its substitutions are redone after the budget, see forward)
            for k in [k for k in _HEAD_BUDGET_CACHE if k[:3] == (self.B, self.H, self.W) and k[-1] == id(self.net)]:
                _HEAD_BUDGET_CACHE.pop(k, None)
            # (a pinned decision read from SSP_TUNE_CACHE belongs to the weights it was measured on, too)
            for k in [k for k in _HEAD_BUDGET_PINNED if k[:3] == (self.B, self.H, self.W)]:
                _HEAD_BUDGET_PINNED.pop(k, None)
            # every timed family is a candidate again
            for cs in self.convs.values():
                fams = cs.fwd_fams
                if fams:
                    best = min((v for v in fams.values() if v[1] is not None), key=lambda v: v[1], default=None)
                    if best is not None:
                        self.set_code(cs, 'fwd', best[0])
            self._settle()

    def _bn_gains(self):
        bn = [cs for _, cs in sorted(self.convs.items()) if cs.bn]
        if not bn:
            return None
        return torch.stack([cs.vec[2][:cs.cout].abs().max() for cs in bn]).cpu()

    def head_budget_drifted(self):
        """True when a BatchNorm block's largest |gamma * invstd| moved by more than 2x since the budget was measured."""
        if self._hb_gains is None:
            return False
        now = self._bn_gains()
        r = (now / self._hb_gains.clamp_min(1e-30)).clamp_min(1e-30)
        return bool(((r > 2.0) | (r < 0.5)).any())

    # ------------------------------------------------------------------ bf16x3 fast mode (SSP_CONV_MATH / Darknet.conv_math)
    # The tuner and the head budget decide first, exactly as with the mode off (so the Winograd decisions are measured
    # against an fp32 reference); then every forward and data-gradient launch that ended on a DIRECT code and that the
    # kernel fits is moved to a bf16x3 code: with the tuner on the one tuning.tune_convs timed faster than the launch's fp32
    # code and verified (cs.x3_fwd / cs.x3_dgrad), with SSP_AUTOTUNE=0 the code with the tile rows and split of the
    # library's own plan.  Filter gradients, the first block, stride-2 blocks and Winograd launches stay fp32.
    # Mode 'bf16x3-wino' is that plus: every forward and data-gradient launch (adjoint form included) that ended on a
    # THROUGH-MEMORY Winograd code is moved to the twin code (tuning.x3_wino_twins: the same plan with its batched GEMM on the
    # bf16 matrix cores) the tuner timed faster than it and verified (cs.x3w_fwd / cs.x3w_dgrad, per Winograd tile, so the
    # substitution follows a layer the head budget moves to another family).  With SSP_AUTOTUNE=0 no Winograd plan exists and
    # the mode equals 'bf16x3'.  The on-chip codes stay fp32.
    def _x3_default(self, cs, which):
        K, N = (cs.cinp, cs.cout) if which == 'fwd' else (cs.coutp, cs.cin)
        args = (self.B, cs.H, cs.W, K, N, cs.k)
        bm = min(_lib.query('ssp_conv_stats_tile_m', *(args + (0,))), 128)
        ks = _lib.query('ssp_conv_workspace_floats', *(args + (0,))) // (cs.M * N)
        for k_ in (min(max(ks, 1), 9), 1):
            code = BF16X3 + bm * 100 + k_ * 10 + 3
            if _lib.query('ssp_conv_bf16x3_fits', *(args + (code,))):
                return code
        return 0

    @staticmethod
    def _own_code(cs, which):
        """The launch's own fp32 code: the one it runs, or goes back to while it is substituted."""
        code, fp32 = (cs.plan_fwd, cs.fp32_fwd) if which == 'fwd' else (cs.plan_dgrad, cs.fp32_dgrad)
        return code if fp32 is None else fp32

    def _x3_code(self, cs, which):
        """The rule above as one function of a layer's forward / data-gradient launch: the code to run instead of the
        launch's own fp32 code, or 0 = that one stays."""
        if self.conv_math['mode'] == 'fp32' or cs.first or cs.stride != 1 or cs.depthwise:
            return 0
        own = self._own_code(cs, which)
        if wino_tile(own):
            if self.conv_math['mode'] != 'bf16x3-wino' or wino_fused(own):
                return 0
            return ((cs.x3w_fwd if which == 'fwd' else cs.x3w_dgrad) or {}).get(wino_tile(own), 0)
        if self._tune:
            return cs.x3_fwd if which == 'fwd' else cs.x3_dgrad
        return self._x3_default(cs, which)

    def _conv_math_record(self):
        self.conv_math['layers'] = {i: (cs.plan_fwd, cs.plan_dgrad) for i, cs in sorted(self.convs.items())
                                    if 'bf16x3' in (conv_math_of(cs.plan_fwd), conv_math_of(cs.plan_dgrad))}

    def _conv_math_revert(self, which=None):
        """Every substituted launch (of one direction, or of both) back on its fp32 code: what the head budget measures and
        measures against, and what the data-gradient choices start from."""
        for w in ('fwd', 'dgrad') if which is None else (which,):
            for cs in self.convs.values():
                self.set_code(cs, w, self._own_code(cs, w))
        self._settle()

    def _apply_conv_math(self, training):
        """The forward substitutions and their budget: one forward on the live batch measures the head deviation d the
        substituted launches add against the head before them (fraction of its range); while
        sqrt(head_budget.head_deviation^2 + d^2) exceeds SSP_HEAD_ERR_BUDGET the substitution nearest the network input
        is taken back (the amplification is largest there), one forward per step.  Runs where the
        head budget runs (the plan's first training batch, and again on its re-measurement triggers), or - a plan that
        only ever infers - on its first forward, in that forward's mode."""
        self._cm_done = True
        rec = self.conv_math
        if rec['mode'] == 'fp32':
            return
        self._conv_math_revert()
        rec.update(layers={}, head_deviation=0.0, taken_back=[])
        subs = [cs for _, cs in sorted(self.convs.items()) if self._x3_code(cs, 'fwd')]

        def substitute():
            for cs in subs:
                self.set_code(cs, 'fwd', self._x3_code(cs, 'fwd'), cs.plan_fwd)
            self._settle()

        budget = knobs().head_budget
        if subs and budget > 0:
            o = self.out_act

            def head():
                if training:
                    self._forward_body(True, False, False, bn_force=True)
                else:
                    self._forward_body(False, False, False)
                return o.t[o.off:o.off + self.B * o.H * o.W * o.ld].clone()
            base = (self.head_budget or {}).get('head_deviation', 0.0)
            base = base if base == base else 0.0          # (a pinned record without a measured figure)
            mom, self.bn_momentum = self.bn_momentum, 0.0
            try:
                ref = head()
                den = max(float(ref.abs().max()), 1e-30)
                substitute()
                while True:
                    d = float((head() - ref).abs().max()) / den
                    if not subs or (base * base + d * d) ** 0.5 <= budget:      # (false for NaN: everything goes back)
                        break
                    cs = subs.pop(0)
                    self.set_code(cs, 'fwd', cs.fp32_fwd)
                    self._settle()
                    rec['taken_back'].append(cs.ind)
                rec['head_deviation'] = d
            finally:
                self.bn_momentum = mom
        else:
            substitute()
        if self._dgrad_fallback:         # the data-gradient choices exist already (a re-measurement): same layers there
            self._conv_math_dgrad()
            self._settle()

    def _conv_math_dgrad(self):
        """The data-gradient substitutions (Plan._prepare_backward, after the tuner; the caller settles): the layers the head
        budget took back keep fp32 in both directions."""
        for ind, cs in sorted(self.convs.items()):
            own = self._own_code(cs, 'dgrad')
            code = 0 if ind in self.conv_math['taken_back'] else self._x3_code(cs, 'dgrad')
            self.set_code(cs, 'dgrad', code or own, own)

    def _sync_codes(self, stage):
        """Multi-GPU: adopt rank 0's plan codes (singleshotpose_amd.dist.sync_plans installs the hook on the model).
        stage 0: forward codes (called once, on the plan's first training forward, after the head-error budget);
        stage 1: data-gradient codes and the filter gradients' direct / Winograd choice (after their tuning)."""
        fn = getattr(self.net, '_plan_sync', None)
        if fn is None:
            return
        order = sorted(self.convs)
        if stage == 0:
            mine = [self.convs[i].plan_fwd for i in order]
        else:
            mine = [self.convs[i].plan_dgrad for i in order] + [self.convs[i].wgrad_wino for i in order]
        head = [self.B, self.H, self.W, stage, len(order)]
        # (deterministic mode: one more entry, so a rank whose mode differs sees a message of another length and every rank
        # falls back - like a rank with a switched-off code; the mode-off message is unchanged)
        det = [1] if self.deterministic['mode'] else []
        got = fn(head + mine + det)
        # Adopt only when EVERY rank can: same plan shape everywhere, and every code one this rank's environment allows
        # (SSP_WINOGRAD / SSP_WINO_TILES / SSP_WINO_FUSED may differ between ranks' launch scripts).  Otherwise all ranks
        # fall back to the library's heuristic plans (code 0) for this stage - a fixed choice of algorithm, the same everywhere.
        ok = got[:5] == head and len(got) == len(head) + len(mine) + len(det)
        if ok:
            kn = knobs()
            for k, v in enumerate(got[5:5 + len(mine)]):
                if v == mine[k] or v == 0:
                    continue
                wg = stage == 1 and k >= len(order)                 # (the filter gradients' entries ARE tile sizes)
                t = (2 if v == WGRAD_FUSED else v) if wg else wino_tile(v)
                if not form_allowed(kn, t, onchip=(v == WGRAD_FUSED if wg else wino_fused(v))):
                    ok = False
                if wg and v == WGRAD_FUSED and det:
                    ok = False       # (the on-chip filter gradient has no ordered form)
                if not wg and conv_math_of(v) == 'bf16x3' and self.conv_math['mode'] not in (
                        ('bf16x3-wino',) if x3_wino(v) else ('bf16x3', 'bf16x3-wino')):
                    ok = False       # a bf16x3 code and this rank's mode is off: like a Winograd code it switched off
        all_ok = getattr(fn, 'all_ok', None)
        if all_ok is not None:
            ok = all_ok(ok)
        vals = got[5:5 + len(mine)] if ok else [0] * len(mine)
        for k, i in enumerate(order):
            cs = self.convs[i]
            # (an adopted bf16x3 code keeps this rank's own fp32 code to go back to)
            if stage == 0:
                self.set_code(cs, 'fwd', vals[k], self._own_code(cs, 'fwd'))
            else:
                self.set_code(cs, 'dgrad', vals[k], self._own_code(cs, 'dgrad'))
                self.set_code(cs, 'wgrad', vals[len(order) + k])
        self._settle()

    def _fit_workspace(self):
        need = max([1] + [cs.ws_fwd for cs in self.convs.values()] + [cs.ws_dgrad for cs in self.convs.values()])
        if need > self.ws_floats:
            torch.cuda.current_stream().synchronize()      # nothing in flight may still use the old workspace
            self.ws_floats = need
            self.ws = torch.empty(need, dtype=torch.float32, device=self.device)
            self._graph = None          # a captured inference chain holds the old workspace pointer

    def _forward_tensors(self):
        ts = [self.x_nhwc, self.ws, self.bn_partial] + [a.t for a in self.acts if a is not None]
        for cs in self.convs.values():
            ts += [cs._raw, cs.vec, cs.stats, cs.first_partial]
        return ts

    @staticmethod
    def _distinct_bytes(ts):
        """Bytes of the distinct storages among tensors ts (None entries skipped).  (An upsample written into its route's
        buffer shares that buffer, and its gradient the route's gradient buffer: footprint() and nbytes_now() count each once.)"""
        seen, total = set(), 0
        for t in ts:
            if t is not None and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                total += t.numel() * t.element_size()
        return total

    def footprint(self):
        """Bytes of device memory this plan's forward buffers hold or will hold after a training-mode forward (each storage
        counted once; raw conv outputs are allocated on first use - every block's but the fused first one's count here)."""
        pending = sum(cs._raw_spec[1] * 4 for cs in self.convs.values() if cs._raw is None and not cs.first_fused)
        return pending + self._distinct_bytes(self._forward_tensors())

    def nbytes_now(self):
        """Bytes of device memory the plan holds right now: forward buffers, and whatever the first backward and the tuner
        added since (gradient buffers, data-gradient operands, Winograd filters and per-layer workspaces)."""
        ts = self._forward_tensors() + [self._dpack, self._wgrad_ws, self._dw_ws] + [g.t for g in self.grads.values()]
        for cs in self.convs.values():
            ts += [cs.wbuf, cs.gbuf, cs.wino_ws, cs.first_wpart, cs.bnp[0] if cs.bnp is not None else None]
            ts += list((cs.wino_u or {}).values()) + list((cs.wino_ud or {}).values())
        return self._distinct_bytes(ts)

    # ------------------------------------------------------------------ lazily allocated filter staging
    def _wbuf(self, cs):
        if cs.wbuf is None:
            cs.wbuf = torch.empty(cs.cout * cs.k * cs.k * cs.cinp, dtype=torch.float32, device=self.device)
        return cs.wbuf

    def _wino_u(self, cs, tile):
        """Winograd-transformed forward filters [(tile+2)^2][Cout][Cin] of a layer whose forward plan is a Winograd code of
        that tile size (one buffer per tile size; the tuner drops the ones it did not choose)."""
        if cs.wino_u is None:
            cs.wino_u = {}
        if tile not in cs.wino_u:
            cs.wino_u[tile] = torch.empty((tile + 2) ** 2 * cs.cout * cs.cinp, dtype=torch.float32, device=self.device)
        return cs.wino_u[tile]

    def _wino_ud(self, cs, tile):
        """... and of the data-gradient operand [(tile+2)^2][Cin][Cout] (from the flipped / transposed [Cin][tap][Cout] layout)."""
        if cs.wino_ud is None:
            cs.wino_ud = {}
        if tile not in cs.wino_ud:
            cs.wino_ud[tile] = torch.empty((tile + 2) ** 2 * cs.cin * cs.coutp, dtype=torch.float32, device=self.device)
        return cs.wino_ud[tile]

    def _wino_ws(self, cs):
        """Per-layer Winograd workspace of a layer whose FILTER GRADIENT runs in the Winograd domain (V | dM | dU, on the
        side stream).  When the layer's forward plan is a Winograd code too, the training forward is handed this same
        buffer (V | M): the transformed input V it leaves at the head is what the filter gradient needs, so the layer
        input is transformed once per step (csrc/conv_wgrad.hip ssp_conv_wgrad_wino_launch, x == NULL)."""
        if cs.wino_ws is None:
            n = cs.wino_ws_floats
            if wino_tile(cs.plan_fwd) and not wino_fused(cs.plan_fwd):
                n = max(n, _lib.query('ssp_conv_workspace_floats', self.B, cs.H, cs.W, cs.cinp, cs.cout, cs.k, cs.plan_fwd))
            cs.wino_ws = torch.empty(n, dtype=torch.float32, device=self.device)
        return cs.wino_ws

    def _gbuf(self, cs):
        if cs.gbuf is None:
            cs.gbuf = torch.empty(cs.cout * cs.k * cs.k * cs.cinp, dtype=torch.float32, device=self.device)
        return cs.gbuf

    def _prepare_backward(self, tune=True):
        """First forward that will be followed by a backward: data-gradient operand buffer, dgrad plan tuning, and the
        split-K workspace those plans need.

        tune=False (Plan.backward's fallback, entered when the forward ran without gradient bookkeeping): the saved raw
        conv outputs are live - timing / verify-after-tune launches would overwrite them (they randomise their operands)
        - so the data-gradient launches only take choices that were timed AND verified earlier in this process, else the
        library's heuristic; a later forward with need_grad tunes them.  The fallback's own choices are made once per plan
        (not per backward)."""
        if self._dpack is None:
            self._dpack = torch.empty(self._dpack_floats, dtype=torch.float32, device=self.device)
        if self._dgrad_tuned or (not tune and self._dgrad_fallback):
            return
        self._dgrad_tuned = tune
        self._dgrad_fallback = True
        self._conv_math_revert('dgrad')      # (bf16x3 mode: the choices below start from the fp32 codes)
        if self._tune and tune:
            tune_convs(self, 'dgrad')
            tune_wgrad(self)
        elif self._tune:
            kn = knobs()
            for cs in self.convs.values():
                if cs.stride != 1 or cs.depthwise:      # no plan codes (and its key would be a stride-1 layer's of the same shape)
                    continue
                key = self._dgrad_key(cs)
                # (the code that was verified, not just the key: a cached Winograd code that SSP_WINOGRAD=0 kept out of
                # this process must not come back through this fallback)
                code = _TUNE_CACHE.get(key, 0)
                self.set_code(cs, 'dgrad', code if _TUNE_VERIFIED.get(key) == code and form_allowed(kn, wino_tile(code), wino_fused(code)) else 0)
                self.set_code(cs, 'wgrad', 0)
                xkey = x3_key(key)
                xcode = _TUNE_CACHE.get(xkey, 0)
                cs.x3_dgrad = xcode if xcode and _TUNE_VERIFIED.get(xkey) == xcode else 0
                t = wino_tile(cs.plan_dgrad)
                wkey = x3_wino_key(key, t)
                wcode = _TUNE_CACHE.get(wkey, 0)
                cs.x3w_dgrad = {t: wcode} if t and wcode and _TUNE_VERIFIED.get(wkey) == wcode else None
        self._conv_math_dgrad()              # bf16x3 mode: the direct data-gradient launches the kernel fits
        if tune:
            self._sync_codes(1)              # multi-GPU: ... and rank 0's data- / filter-gradient choices
        self._settle(dgrad=True)

    def _adjoint_rule(self, cs):
        """Whether the layer takes the adjoint form of the data gradient (see _SHARE_DM): its data-gradient plan is a
        through-memory Winograd code of tile n, its filter gradient runs at the same tile, and dY has no padding channels
        (the filter gradient's dM [P][T][cout] is then the data gradient's operand [P][T][coutp]).  A function of the
        layer's plan codes alone; applied where the layer's data-gradient operand is prepared (_repack_dgrad), so the
        operand and the launch that reads it always agree."""
        t = wino_tile(cs.plan_dgrad)
        return bool(_SHARE_DM and not cs.first and cs.stride == 1 and t and not wino_fused(cs.plan_dgrad) and cs.wgrad_wino == t and
                    cs.coutp == cs.cout)

    def _wgrad_key(self, cs):
        return ('wgrad', self.B, cs.H, cs.W, cs.cinp, cs.cout, cs.ldraw, cs.inp.ld, _tune_tag())

    def _dgrad_key(self, cs):
        return ('dgrad', self.B, cs.H, cs.W, cs.coutp, cs.cin, cs.k, cs.ldraw, cs.inp.ld, _tune_tag())

    def _plan_bn_fusion(self):
        """BatchNorm-backward reductions folded into the producing data-gradient launch (ssp_conv_dgrad_bnbwd).

        Block `src` qualifies when its (un-pooled) BN + leaky output feeds exactly one consumer and that consumer is a
        conv: the consumer's dgrad writes g = dL/d out(src) - the tile it just finished holds g, one extra read of
        src's raw conv output at the same positions gives sum(dy) and sum(dy * xhat) per tile, and the separate reduce
        pass over raw + g (bn_act_bwd_reduce_kernel: a third of the step's BatchNorm-backward traffic, on the critical
        stream) disappears.  Pooled blocks, blocks with two consumers (route sources) and blocks consumed through a
        route / reorg keep the two-pass form.  SSP_BN_FUSE=0 turns it off (A/B)."""
        on = os.environ.get('SSP_BN_FUSE', '1') != '0'
        for cs in self.convs.values():
            cs.bn_fuse_src = None
            cs.bnp = None
        if not on:
            return
        for cs in self.convs.values():
            # (the strided and the depthwise data gradients have no fused sums: their producers keep two passes; either may
            # be the SOURCE of a pair)
            if cs.first or cs.stride != 1 or cs.depthwise:
                continue
            src = cs.inp.producer
            scs = self.convs.get(src)
            if (scs is None or scs.pool or not scs.bn or not scs.needs_act or scs.out is not cs.inp or
                    self.consumers[src] != [cs.ind] or scs.coutp != scs.cout or cs.cin != scs.cout or
                    cs.inp.ld != scs.ldraw or cs.inp.off != 0 or cs.cin % 4):
                continue
            ntile = _lib.query('ssp_conv_stats_tiles', self.B, cs.H, cs.W, cs.coutp, cs.cin, cs.k, cs.plan_dgrad)
            if self.deterministic['mode'] and ntile > 1024:
                # the fold adds tile t into row t % 1024 with atomics: in the mode the block keeps its own two-level
                # reduction (ssp_bn_act_bwd: per-workgroup partials, float64 finalize) instead
                if (src, 'bn-sums-in-dgrad') not in self.deterministic['taken_back']:
                    self.deterministic['taken_back'].append((src, 'bn-sums-in-dgrad'))
                continue
            rows = min(ntile, 1024)       # more tiles than rows: folded with atomics into a buffer that stays zeroed
            cs.bn_fuse_src = scs
            scs.bnp = (torch.zeros(rows * scs.cout * 2, dtype=torch.float32, device=self.device), rows, ntile > rows)

    def _repack_dgrad(self, cs, stream):
        if cs.depthwise:      # ssp_dwconv_dgrad reads the parameter itself
            return
        src = cs.conv.weight.detach()
        if not cs.packed:
            with torch.cuda.stream(stream):
                src = src.contiguous()       # the plain-layout kernel reads (Cout,Cin,kh,kw) order
                src.record_stream(stream)
        _lib.call('ssp_repack_dgrad_packed' if cs.packed else 'ssp_repack_dgrad', src.data_ptr(),
                  _ptr(self._dpack, cs.doff), cs.cout, cs.cin, cs.coutp, cs.k, stream.cuda_stream)
        tile = wino_tile(cs.plan_dgrad)
        cs.dgrad_adj = self._adjoint_rule(cs)
        if tile:      # Winograd data-gradient plan: its filter operand is the transform of that layout
            # (adjoint form: of the same layout with the taps read back to front - the forward transform, channels transposed)
            _lib.call('ssp_wino_filter_transform_adj_t' if cs.dgrad_adj else 'ssp_wino_filter_transform_t',
                      _ptr(self._dpack, cs.doff), self._wino_ud(cs, tile).data_ptr(), cs.cin, cs.coutp, tile,
                      stream.cuda_stream)

    # ------------------------------------------------------------------ forward
    def forward(self, x, training, need_grad=False, inline_repack=False, trainable=None, want_input=True):
        """training: the model's mode (the autograd node, the repack policy and the head budget follow it); every BatchNorm
        block normalises by its OWN module's mode.  need_grad: a backward will follow - for the parameters whose ids are in
        `trainable` (None = all of them) and, with want_input, the input: blocks that backward will not visit
        (backward_schedule) run the chain of a forward without gradient bookkeeping."""
        B, H, W = self.B, self.H, self.W
        st = torch.cuda.current_stream().cuda_stream
        call = _lib.call
        if x.dtype == torch.uint8:     # (B,H,W,C) image bytes: ToTensor's /255 and the NHWC padding in one pass
            call('ssp_u8hwc_to_nhwc', x.data_ptr(), self.x_nhwc.data_ptr(), B, H, W, self.in_c, self.in_cp, self.in_cp, st)
        else:
            call('ssp_nchw_to_nhwc', x.data_ptr(), self.x_nhwc.data_ptr(), B, self.in_c, H, W, self.in_cp, self.in_cp, st)
        if training and need_grad and self._head_budget_done and self._tune:
            every = int(os.environ.get('SSP_HEAD_BUDGET_EVERY', '256'))
            if every > 0 and self.generation - self._hb_checked >= every:
                self._hb_checked = self.generation
                drifted = self.head_budget_drifted()
                sync = getattr(self.net, '_plan_sync', None)      # multi-GPU: BatchNorm statistics are per replica, the plan set
                if sync is not None and hasattr(sync, 'all_ok'):  # is not - every rank re-measures when any rank drifted
                    drifted = not sync.all_ok(not drifted)
                if drifted:
                    self.head_budget_stale()
        if training and need_grad and not self._head_budget_done:
            self._conv_math_revert()         # (bf16x3 mode: the budget below measures fp32 launches against fp32 launches)
            self._apply_head_budget()        # on the plan's first training batch, after load_weights, and when the BatchNorm
                                             # gains drifted (network-level rounding budget)
            self._apply_conv_math(True)      # bf16x3 mode: the direct launches it fits, under the same budget
            self._sync_codes(0)              # multi-GPU: every rank runs rank 0's forward codes
        elif not self._cm_done:
            self._apply_conv_math(training)  # a plan that has not trained yet: on its first forward
        # (The whole training step as two captured hipGraphs was built and measured in round 4 - profiles/r04_step_graph.txt:
        # a replayed two-stream chain of ~300 nodes is SLOWER than launching it, 9.1 ms against 6.0 ms at batch 8 - and
        # removed in round 5: it mirrored this method's host-side state by hand.  Inference keeps its graph, forward_graph.)
        self._forward_body(training, need_grad, inline_repack, trainable=trainable, want_input=want_input)
        if training and getattr(self, '_hb_gains_after_forward', False):
            self._hb_gains_after_forward = False
            self._hb_gains = self._bn_gains()
        o = self.out_act
        y = torch.empty(*((B, o.C) if self.out_flat else (B, o.C, o.H, o.W)), dtype=torch.float32, device=self.device)
        call('ssp_nhwc_to_nchw', o.ptr, y.data_ptr(), B, o.C, o.H, o.W, o.ld, st)
        self.consumed = False
        self.was_training = training
        self.generation += 1
        return y

    def _forward_body(self, training, need_grad, inline_repack, bn_force=None, trainable=None, want_input=True):
        """bn_force: None = every BatchNorm block in its module's own mode; True / False = all of them (the head budget
        measures with batch statistics everywhere)."""
        B, H, W = self.B, self.H, self.W
        st = torch.cuda.current_stream().cuda_stream
        call = _lib.call
        for cs in self.convs.values():
            cs.bn_train = bool(cs.bn and (cs.bnm.training if bn_force is None else bn_force))
        # Filter repacks depend only on the weights, not on the activations: they run on the side stream, ahead of the
        # convolutions that use them, instead of as one more dependent launch
        # in front of every conv on the main stream.  Forward operands first (two events: the first four layers, then
        # the rest), then - when a backward will follow - the flipped/transposed data-gradient operands, which hide
        # under the MFMA-bound forward convs instead of sitting on the critical path of backward.
        # eval: repack only when a parameter changed (in-place updates bump _version, the fused SGD bumps the weights
        # epoch, load_weights invalidates explicitly); training: weights change every step, always repack.
        # Parameters stored channels-last (Darknet builds them that way) ARE the forward operand: nothing to repack.
        stale = []
        for cs in self.convs.values():
            wt = cs.conv.weight
            if cs.depthwise:
                # the (C, 1, 3, 3) parameter IS the operand, w[c*9 + tap], and its gradient is written in that layout in place
                if not wt.is_contiguous():
                    raise RuntimeError("block %d (convolutional): the depthwise filter is not contiguous (ssp_dwconv_fwd reads "
                                       "the (C, 1, 3, 3) parameter in place)" % cs.ind)
                cs.packed = True
                continue
            cs.packed = _is_packed(wt, cs.cinp)
            if cs.packed:
                continue
            key = (wt.data_ptr(), wt._version, _WEIGHTS_EPOCH[0])
            if inline_repack:
                # graph capture: the repack is part of the captured chain (stays on this stream, runs every replay)
                call('ssp_repack_fwd', wt.detach().contiguous().data_ptr(), self._wbuf(cs).data_ptr(), cs.cout,
                     cs.cin, cs.cinp, cs.k, st)
                self.wversion.pop(cs.ind, None)
            elif training or self.wversion.get(cs.ind) != key:
                stale.append((cs, key))
        if need_grad:
            self._prepare_backward()        # (the schedule reads the BatchNorm fusion it plans)
            sched = self._schedule(trainable, want_input, {cs.ind: cs.bn_train for cs in self.convs.values()})
            for op, s_ in zip(self.ops, sched):
                if op.kind == 'conv':
                    op.fsched = s_
        else:
            for cs in self.convs.values():
                cs.fsched = None
        # Winograd-plan layers read TRANSFORMED filters: re-derived when the weights may have changed (every training
        # step; in eval when a parameter version / the weights epoch moved), on the side stream like the repacks
        wino = []
        for cs in self.convs.values():
            if wino_tile(cs.plan_fwd):
                wt = cs.conv.weight
                wkey = (wt.data_ptr(), wt._version, _WEIGHTS_EPOCH[0])
                if inline_repack or training or self.wino_version.get(cs.ind) != wkey:
                    wino.append((cs, wkey))
        wait_for = {}
        if inline_repack:
            for cs, _ in wino:       # graph capture: part of the captured chain
                src = cs.conv.weight if cs.packed else self._wbuf(cs)
                tile = wino_tile(cs.plan_fwd)
                call('ssp_wino_filter_transform_t', src.data_ptr(), self._wino_u(cs, tile).data_ptr(), cs.cout, cs.cinp, tile, st)
                self.wino_version.pop(cs.ind, None)
            wino = []
        if stale or need_grad or wino:
            if self.side_stream is None:
                self.side_stream = _side_stream(self.device)
            side = self.side_stream
            side.wait_stream(torch.cuda.current_stream())
            for group in (stale[:4], stale[4:]):
                for cs, key in group:
                    with torch.cuda.stream(side):
                        src = cs.conv.weight.detach().contiguous()      # the repack kernels read (Cout,Cin,kh,kw) order
                        src.record_stream(side)
                    call('ssp_repack_fwd', src.data_ptr(), self._wbuf(cs).data_ptr(), cs.cout, cs.cin,
                         cs.cinp, cs.k, side.cuda_stream)
                    self.wversion[cs.ind] = key
                if group:
                    ev = side.record_event()
                    for cs, _ in group:
                        wait_for[cs.ind] = ev
        if stale or need_grad or wino:
            # the forward filter transforms of every Winograd layer, queued up front: they depend on the weights only and
            # run under the first block and layer 2.  (Queueing them layer by layer just ahead of their convs, and the
            # data-gradient operands after the last forward launch, was tried for the host-bound look of a traced batch-8
            # step - profiles/r04_timeline_b8.txt: first kernel 0.65 ms late - and bought nothing: the host queues a step in
            # 3.6 ms, tools/host_issue_time.py, against 6 ms of GPU time at batch 8 and 28 ms at batch 64 - it runs ahead of the
            # GPU either way and the step time did not move.)
            if wino:
                for cs, wkey in wino:
                    src = cs.conv.weight if cs.packed else self._wbuf(cs)
                    tile = wino_tile(cs.plan_fwd)
                    call('ssp_wino_filter_transform_t', src.data_ptr(), self._wino_u(cs, tile).data_ptr(), cs.cout, cs.cinp,
                         tile, side.cuda_stream)
                    self.wino_version[cs.ind] = wkey
                # ONE event behind all of them: the side stream is through by ~1.4 ms, the main stream reaches layer 4 at
                # ~1.6 ms, and every cross-stream wait costs ~17 us of GPU idle even when its event has long fired (one
                # event per layer: 13 such gaps, forward idle 0.68 ms instead of 0.3-0.6, profiles/r04_timeline.txt)
                ev = side.record_event()
                for cs, _ in wino:
                    wait_for[cs.ind] = ev
        if need_grad:
            # (queueing these BEHIND the last on-chip Winograd forward launch - that kernel is persistent, one workgroup per CU,
            # and shares the chip badly - was measured: 26.17 / 25.93 ms against 25.85 / 25.97 ms as is, nothing)
            for ind in sorted(self.convs.keys(), reverse=True):
                cs = self.convs[ind]
                if not cs.first and cs.fsched.dgrad[0]:      # (a block whose producer gets no gradient needs no operand)
                    self._repack_dgrad(cs, side)
            self.dgrad_ready = side.record_event()
        else:
            self.dgrad_ready = None
        waited = set()
        if any(cs.bn_train for cs in self.convs.values()):
            self.net._bn_epoch += 1       # running statistics change below: every plan's inference constants are stale
        for op in self.ops:
            kind = op.kind
            if kind == 'conv':
                self._conv_fwd(op, training, need_grad, inline_repack, wait_for, waited, st)
                continue
            out = op.out
            src = op.srcs[0]
            if kind == 'maxpool':
                call('ssp_maxpool_fwd', src.ptr, src.ld, out.ptr, out.ld, _pad4(src.C), B, src.H, src.W, st)
            elif kind == 'maxpool_s1':
                call('ssp_maxpool_s1_fwd', src.ptr, src.ld, out.ptr, out.ld, _pad4(src.C), B, src.H, src.W, st)
            elif kind == 'reorg':
                call('ssp_reorg', src.ptr, src.ld, out.ptr, out.ld, src.C, B, src.H, src.W, 0, 0, st)
            elif kind == 'upsample':
                call('ssp_upsample_fwd', src.ptr, src.ld, out.ptr, out.ld, _pad4(src.C), B, src.H, src.W, op.stride, st)
            elif kind == 'shortcut':
                a, b = op.srcs
                call('ssp_shortcut_fwd', a.ptr, a.ld, b.ptr, b.ld, out.ptr, out.ld, _pad4(out.C), B * out.H * out.W, op.slope,
                     st)
            elif kind == 'avgpool':
                call('ssp_avgpool_fwd', src.ptr, src.ld, out.ptr, out.ld, _pad4(src.C), B, src.H, src.W, st)
            elif kind == 'softmax':
                call('ssp_softmax_fwd', src.ptr, src.ld, out.ptr, out.ld, src.C, B * src.H * src.W, st)
            elif kind == 'concat':
                off = 0
                for n, s in enumerate(op.srcs):
                    if not (n == 0 and op.inplace):      # (an upsample wrote its columns of the buffer itself)
                        call('ssp_copy_channels', s.ptr, s.ld, _ptr(out.t, off), out.ld, s.C, B * s.H * s.W, 0, st)
                    off += s.C
            # ('alias', a one-layer route: its output is the source's map, nothing to run)

    def _conv_fwd(self, cs, training, need_grad, inline_repack, wait_for, waited, st):
        """Forward launches of conv block `cs` (waiting first for its filters from the side stream, see _forward_body)."""
        B = self.B
        call = _lib.call
        ev = wait_for.get(cs.ind)
        if ev is not None and id(ev) not in waited:
            torch.cuda.current_stream().wait_event(ev)      # this layer's packed filters are ready
            waited.add(id(ev))
        bias = cs.conv.bias.data_ptr() if cs.conv.bias is not None else None
        bn_train = cs.bn_train                               # this block's own BatchNorm mode, not the model's
        keep = cs.fsched is not None and cs.fsched.visited   # a backward will come through this block
        use_stats = bn_train
        v = cs.vec
        if cs.bn and not bn_train:
            # inference-mode BatchNorm is a per-channel affine map of constants: recomputed only when one of
            # its four tensors changed (in-place updates bump _version; load_weights / fused SGD bump the epoch)
            bn = cs.bnm
            # (a training-mode forward rewrites running_mean / running_var through raw pointers and reuses the
            # scale / shift vectors for the batch statistics: it bumps the net's BN epoch, also part of the key)
            bkey = tuple((t.data_ptr(), t._version) for t in (bn.weight, bn.bias, bn.running_mean,
                                                             bn.running_var)) + (_WEIGHTS_EPOCH[0],
                                                                                 self.net._bn_epoch)
            if inline_repack or self.bnversion.get(cs.ind) != bkey:
                call('ssp_bn_eval_prepare', cs.cout, bn.weight.data_ptr(), bn.bias.data_ptr(),
                     bn.running_mean.data_ptr(), bn.running_var.data_ptr(), BN_EPS, v[0].data_ptr(),
                     v[1].data_ptr(), v[2].data_ptr(), v[3].data_ptr(), st)
                self.bnversion[cs.ind] = None if inline_repack else bkey
        wptr = cs.conv.weight.data_ptr() if cs.packed else self._wbuf(cs).data_ptr()
        if wino_tile(cs.plan_fwd):
            wptr = self._wino_u(cs, wino_tile(cs.plan_fwd)).data_ptr()
        cs.first_live = False
        cs.has_raw = False
        if cs.first_fused and not cs.packed and (bn_train or not keep):
            # training: statistics pass + apply pass; inference: the apply pass alone with the running-statistics
            # affine (v[2], v[3] from ssp_bn_eval_prepare above) - conv + BN + leaky + pool in one launch, the
            # full-resolution map is never written (672 x 672, batch 1: 12 us instead of 23 + 12).  A BatchNorm in eval()
            # under a training model takes the apply-only form when no backward comes through the block, else the generic
            # kernels below (the fused backward passes are the batch-statistics ones).
            if bn_train:
                bn = cs.bnm
                call('ssp_first_fwd_stats', cs.inp.ptr, wptr, cs.stats.data_ptr(), B, cs.H, cs.W, st)
                call('ssp_bn_fwd_finalize', cs.stats.data_ptr(), cs.first_groups, cs.first_tile, cs.M, cs.cout,
                     bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                     bn.running_var.data_ptr(), self.bn_momentum, BN_EPS, v[0].data_ptr(), v[1].data_ptr(),
                     v[2].data_ptr(), v[3].data_ptr(), st)
            call('ssp_first_fwd_apply', cs.inp.ptr, wptr, v[2].data_ptr(), v[3].data_ptr(), cs.slope,
                 cs.out.ptr, cs.out.ld, B, cs.H, cs.W, st)
            cs.first_live = bn_train        # only a batch-statistics forward can be followed by the fused backward
            return
        if (not bn_train and not keep and (cs.bn or not training) and cs.needs_act and not cs.pool and
                cs.coutp == cs.cout):
            # inference, un-pooled block: BatchNorm affine + leaky folded into the conv epilogue - one launch,
            # no raw-output round trip (backward needs the raw output, so training / autograd keep two steps).  Also
            # a block with its BatchNorm in eval() that no backward will visit (a frozen trunk under model.train()).
            if cs.depthwise:
                call('ssp_dwconv_fwd_affine', cs.inp.ptr, wptr, cs.out.ptr, v[2].data_ptr() if cs.bn else None,
                     v[3].data_ptr() if cs.bn else bias, cs.slope, B, cs.Hi, cs.Wi, cs.cin, cs.inp.ld, cs.out.ld, cs.stride, st)
                return
            if cs.stride == 2:
                call('ssp_conv_s2_fwd_affine', cs.inp.ptr, wptr, cs.out.ptr, v[2].data_ptr() if cs.bn else None,
                     v[3].data_ptr() if cs.bn else bias, cs.slope, B, cs.Hi, cs.Wi, cs.cinp, cs.cout, cs.inp.ld,
                     cs.out.ld, cs.k, st)
                return
            call('ssp_conv_fwd_affine', cs.inp.ptr, wptr, cs.out.ptr, v[2].data_ptr() if cs.bn else None,
                 v[3].data_ptr() if cs.bn else bias, cs.slope, B, cs.H, cs.W, cs.cinp, cs.cout, cs.inp.ld,
                 cs.out.ld, cs.k, cs.plan_fwd, self.ws.data_ptr(), self.ws_floats, st)
            return
        ws_t = self.ws
        cs.v_live = False
        share_v = os.environ.get('SSP_WINO_SHARE_V', '1') != '0'
        cs.has_raw = True
        want_v = keep and cs.fsched.wgrad      # the transformed input is kept for the filter gradient only
        if (want_v and wino_tile(cs.plan_fwd) and not wino_fused(cs.plan_fwd) and
                cs.wgrad_wino == wino_tile(cs.plan_fwd) and share_v):
            ws_t = self._wino_ws(cs)         # V stays at the head of this buffer for the layer's filter gradient
            cs.v_live = True
        elif (want_v and cs.wgrad_wino and share_v and self.side_stream is not None and
                os.environ.get('SSP_WINO_EARLY_V', '0') == '1'):
            # The filter gradient runs in the Winograd domain but this forward launch does not leave its V behind (the
            # error budget moved the layer to a direct code, or to the other tile size): the input transform the
            # filter gradient needs CAN be queued now on the second stream (SSP_WINO_EARLY_V=1) - an HBM-bound pass next
            # to the forward launches instead of inside the backward pass.  Measured on one box, two interleaved rounds
            # (profiles/r05_step_ab.txt): 27.48 / 27.57 ms with it, 27.38 / 27.47 without - the transform slows the
            # MFMA-bound direct launches it runs beside by as much as it saves later; off by default.
            wws = self._wino_ws(cs)
            ready = torch.cuda.current_stream().record_event()      # the layer's input is complete on the main stream
            self.side_stream.wait_event(ready)
            call('ssp_wino_input_transform_t', cs.inp.ptr, cs.inp.ld, wws.data_ptr(), B, cs.H, cs.W, cs.cinp,
                 cs.wgrad_wino, self.side_stream.cuda_stream)
            cs.v_live = True
        if cs.depthwise:
            call('ssp_dwconv_fwd', cs.inp.ptr, wptr, cs.raw.data_ptr(), bias, cs.stats.data_ptr() if use_stats else None,
                 B, cs.Hi, cs.Wi, cs.cin, cs.inp.ld, cs.ldraw, cs.stride, st)
        elif cs.stride == 2:
            call('ssp_conv_s2_fwd', cs.inp.ptr, wptr, cs.raw.data_ptr(), bias, cs.stats.data_ptr() if use_stats else None,
                 B, cs.Hi, cs.Wi, cs.cinp, cs.cout, cs.inp.ld, cs.ldraw, cs.k, 0, st)
        else:
            call('ssp_conv_fwd', cs.inp.ptr, wptr, cs.raw.data_ptr(), bias,
                 cs.stats.data_ptr() if use_stats else None, B, cs.H, cs.W, cs.cinp, cs.cout, cs.inp.ld, cs.ldraw,
                 cs.k, 0, cs.plan_fwd, ws_t.data_ptr(), ws_t.numel(), st)
        if bn_train:
            bn = cs.bnm
            call('ssp_bn_fwd_finalize', cs.stats.data_ptr(), cs.ntile, cs.tile_m, cs.M, cs.cout,
                 bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                 bn.running_var.data_ptr(), self.bn_momentum, BN_EPS, v[0].data_ptr(), v[1].data_ptr(),
                 v[2].data_ptr(), v[3].data_ptr(), st)
        if cs.needs_act:
            call('ssp_bn_act_fwd', cs.raw.data_ptr(), cs.ldraw, cs.out.ptr, cs.out.ld, v[2].data_ptr(),
                 v[3].data_ptr(), cs.coutp, B, cs.H, cs.W, 1 if cs.pool else 0, cs.slope, st)

    # ------------------------------------------------------------------ inference as one hipGraph
    def _graph_tensors(self):
        ts = []
        for cs in self.convs.values():
            ts.append(cs.conv.weight)
            if cs.conv.bias is not None:
                ts.append(cs.conv.bias)
            if cs.bn:
                ts += [cs.bnm.weight, cs.bnm.bias, cs.bnm.running_mean, cs.bnm.running_var]
        return ts

    def forward_graph(self, x):
        """Eval-mode forward replayed from a captured hipGraph: the ~75 launches of a forward pass are launch-bound at
        small batch (valid.py runs B = 1: 1.8 ms eager for 0.6 ms of kernels).  The kernels read parameters and BN
        running statistics from their own memory, so in-place weight updates need no re-capture; a parameter that moved
        (new data_ptr), another input dtype, or a non-contiguous first-layer filter does."""
        if self._graph_failed:
            return self.forward(x, False)
        key = (x.dtype,) + tuple((t.data_ptr(), tuple(t.stride())) for t in self._graph_tensors())
        if self._graph is None or self._graph_key != key:
            try:
                self._x_static = torch.empty_like(x)
                self._x_static.copy_(x)
                self.forward(self._x_static, False, inline_repack=True)      # eager warm-up (lazy per-kernel set-up)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    y = self.forward(self._x_static, False, inline_repack=True)
                self._graph, self._y_static, self._graph_key = g, y, key
            except Exception as e:      # capture unsupported in this runtime: keep the eager HIP launches
                import warnings
                warnings.warn("hipGraph capture of the inference chain failed (%s); using eager launches" % (e,))
                self._graph, self._graph_failed = None, True
                torch.cuda.synchronize(self.device)
                return self.forward(x, False)
        self._x_static.copy_(x)
        self._graph.replay()
        self.consumed = True          # no backward on a graph replay
        return self._y_static.clone()

    # ------------------------------------------------------------------ backward
    def backward_schedule(self, trainable_ids=None, want_input=False, bn_training=None):
        """What a backward pass runs, per executed op (one OpSchedule per entry of self.ops): pure bookkeeping, no launch.

        trainable_ids: ids of the parameters that want a gradient (None = every parameter); want_input: the network input
        wants one; bn_training: None = every BatchNorm module's own `training` flag, a bool = all of them, or
        {conv layer index: bool}.

        A block is upstream-relevant when it owns a trainable parameter or any map it reads derives from one that is (with
        want_input the network input counts); it is visited iff it is upstream-relevant and reaches the output.  A data
        gradient into a producer runs iff that producer is visited (or is the wanted input); filter gradient, bias column
        sum, dgamma / dbeta follow their parameters; the BatchNorm-backward reductions of a visited block run when its
        BatchNorm normalised with batch statistics (dx needs them) or gamma / beta is trainable - otherwise the block's
        backward is the affine map's; a consumer's data gradient folds those sums only where they run."""
        T = None if trainable_ids is None else frozenset(trainable_ids)

        def has(p):
            return p is not None and (T is None or id(p) in T)

        def bn_mode(cs):
            if not cs.bn:
                return False
            if bn_training is None:
                return bool(cs.bnm.training)
            if isinstance(bn_training, dict):
                return bool(bn_training[cs.ind])
            return bool(bn_training)

        def srcs_of(op):
            return [op.inp] if op.kind == 'conv' else op.srcs

        rel = {INPUT: bool(want_input)}
        own = {}
        for op in self.ops:
            mine = False
            if op.kind == 'conv':
                own[op.ind] = (has(op.conv.weight), has(op.conv.bias), bool(op.bn) and has(op.bnm.weight),
                               bool(op.bn) and has(op.bnm.bias))
                mine = any(own[op.ind])
            rel[op.oind] = mine or any(rel[a.producer] for a in srcs_of(op))

        def bn_reduce(cs):
            return bool(cs.bn) and (bn_mode(cs) or own[cs.ind][2] or own[cs.ind][3])

        reach = set([self.last])
        out = [None] * len(self.ops)
        for i in range(len(self.ops) - 1, -1, -1):
            op = self.ops[i]
            srcs = srcs_of(op)
            if not (op.oind in reach and rel[op.oind]):
                out[i] = OpSchedule(op.ind, op.kind, False, (False,) * len(srcs), False, False, False, False, False, False)
                continue
            dgrad = tuple(rel[a.producer] for a in srcs)
            for a, d in zip(srcs, dgrad):
                if d:
                    reach.add(a.producer)
            if op.kind != 'conv':
                out[i] = OpSchedule(op.ind, op.kind, True, dgrad, False, False, False, False, False, False)
                continue
            w, b, dg, db = own[op.ind]
            fold = bool(dgrad[0] and op.bn_fuse_src is not None and bn_reduce(op.bn_fuse_src))
            out[i] = OpSchedule(op.ind, 'conv', True, dgrad, w, b, dg, db, bn_reduce(op), fold)
        return out

    def _schedule(self, trainable, want_input, modes=None):
        """backward_schedule, remembered per (trainable set, want_input, BatchNorm modes): a training loop asks for the same
        one every step."""
        if modes is None:
            modes = {cs.ind: bool(cs.bn and cs.bnm.training) for cs in self.convs.values()}
        # (keyed by what the rules read - which parameters of which block are trainable - not by object ids, which a
        # replaced parameter may reuse)
        own = None if trainable is None else tuple(
            tuple(p is not None and id(p) in trainable for p in (
                cs.conv.weight, cs.conv.bias, cs.bnm.weight if cs.bn else None, cs.bnm.bias if cs.bn else None))
            for cs in self.convs.values())
        key = (own, bool(want_input), tuple(sorted(modes.items())), tuple(
            None if cs.bn_fuse_src is None else cs.bn_fuse_src.ind for cs in self.convs.values()))
        sched = self._schedules.get(key)
        if sched is None:
            if len(self._schedules) >= 32:
                self._schedules.clear()
            sched = self._schedules[key] = self.backward_schedule(trainable, want_input, modes)
        return sched

    def _grad_buf(self, ind, like):
        g = self.grads.get(ind)
        if g is None:
            g = _Act(torch.empty(self.B * like.H * like.W * like.ld, dtype=torch.float32, device=self.device), 0,
                     like.C, like.H, like.W, like.ld)
            self.grads[ind] = g
        return g

    def _dgrad(self, cs, src, dy_ptr, dy_ld, written, fused_stats, st, fold=True, dm_ptr=None):
        """Data gradient of conv block `cs` into the gradient buffer of its input's producer `src` (with the producer's
        BatchNorm-backward sums folded in where _plan_bn_fusion arranged it).  dm_ptr: a layer in the adjoint form
        (cs.dgrad_adj) whose dM = A dY A^T is already in memory; None there = the launch transforms dY itself."""
        call = _lib.call
        B = self.B
        gin = self._grad_buf(src, cs.inp)
        if cs.depthwise:
            # csrc/conv_depthwise.hip: H x W of the INPUT map, the parameter itself as the operand, one thread per element
            # at both strides (the same bits every run: deterministic mode needs no other form)
            call('ssp_dwconv_dgrad', dy_ptr, cs.conv.weight.data_ptr(), gin.ptr, B, cs.Hi, cs.Wi, cs.cin, dy_ld, gin.ld,
                 cs.stride, 1 if src in written else 0, st)
            written.add(src)
            return
        if cs.stride == 2:
            # parity-decomposed data gradient (csrc/conv_strided.hip): H x W of the INPUT map, no plan, no workspace, no
            # fused BatchNorm-backward sums (_plan_bn_fusion never makes a strided block the consumer)
            # (deterministic mode: one thread per pixel on small grids too - their tap split sums with atomics)
            call('ssp_conv_s2_dgrad_ordered' if self.deterministic['mode'] else 'ssp_conv_s2_dgrad', dy_ptr,
                 _ptr(self._dpack, cs.doff), gin.ptr, B, cs.Hi, cs.Wi, cs.coutp, cs.cin, dy_ld, gin.ld, cs.k,
                 1 if src in written else 0, st)
            written.add(src)
            return
        scs = cs.bn_fuse_src
        dwt = (self._wino_ud(cs, wino_tile(cs.plan_dgrad)).data_ptr() if wino_tile(cs.plan_dgrad)
               else _ptr(self._dpack, cs.doff))
        adj = (dm_ptr, st) if cs.dgrad_adj else (st,)
        if scs is not None and fold and src not in written:
            sv = scs.vec
            call('ssp_conv_dgrad_adj_bnbwd' if cs.dgrad_adj else 'ssp_conv_dgrad_bnbwd', dy_ptr, dwt, gin.ptr, B, cs.H, cs.W,
                 cs.coutp, cs.cin, dy_ld, gin.ld, cs.k, cs.plan_dgrad, self.ws.data_ptr(), self.ws_floats,
                 scs.raw.data_ptr(), scs.ldraw, sv[2].data_ptr(), sv[3].data_ptr(), sv[0].data_ptr(),
                 sv[1].data_ptr(), scs.slope, scs.bnp[0].data_ptr(),
                 -scs.bnp[1] if self.deterministic['mode'] else scs.bnp[1], *adj)      # (< 0: a fold is an error, never atomics)
            fused_stats.add(src)
        else:
            call('ssp_conv_dgrad_adj' if cs.dgrad_adj else 'ssp_conv_dgrad', dy_ptr, dwt, gin.ptr, B, cs.H, cs.W, cs.coutp,
                 cs.cin, dy_ld, gin.ld, cs.k, 1 if src in written else 0, cs.plan_dgrad, self.ws.data_ptr(),
                 self.ws_floats, *adj)
        written.add(src)

    def backward(self, grad_out, want_input=False, want_params=True):
        """grad_out: (B, C, h, w) NCHW, or (B, C) when the network ends in avgpool / connected / softmax.  Returns
        ({param tensor id: grad tensor}, dL/dx as (B, in_c, H, W) fp32 or None).

        want_input: also compute the gradient of the network input.  want_params: True = every parameter gets a gradient;
        a collection of parameter ids = those parameters do, the others are frozen - the pass runs what
        backward_schedule lists for them, the dict holds their gradients only and the frozen ranges of the flat
        gradient buffer stay zero; False or empty (only with want_input): the input-only backward - the data-gradient
        chain and the BatchNorm-backward reductions it needs, no filter / bias / BatchNorm-parameter gradients, no flat
        gradient buffer, no reducer call; the dict is empty."""
        if want_params is True:
            trainable = None
        elif want_params is False:
            trainable = frozenset()
        else:
            trainable = frozenset(want_params) & frozenset(self.grad_layout)
            if len(trainable) == len(self.grad_layout):
                trainable = None
        want_params = trainable is None or len(trainable) > 0
        if not (want_input or want_params):
            raise ValueError("Plan.backward: neither the input nor the parameter gradients are wanted")
        if self.consumed:
            raise RuntimeError("Darknet backward called twice on the same forward: the HIP path rewrites the saved "
                               "conv outputs in place (no retain_graph support)")
        self.consumed = True
        B = self.B
        st = torch.cuda.current_stream().cuda_stream
        call = _lib.call
        o = self.out_act
        if tuple(grad_out.shape) != ((B, o.C) if self.out_flat else (B, o.C, o.H, o.W)):
            raise ValueError("Darknet backward: gradient of shape %s for an output of shape %s" % (
                tuple(grad_out.shape), (B, o.C) if self.out_flat else (B, o.C, o.H, o.W)))
        g_last = self._grad_buf(self.last, o)
        call('ssp_nchw_to_nhwc', grad_out.data_ptr(), g_last.ptr, B, o.C, o.H, o.W, o.C, o.ld, st)
        if self.side_stream is None:
            self.side_stream = _side_stream(self.device)
        # the BatchNorm modes are the ones the forward ran in, whatever the modules say by now
        sched = self._schedule(trainable, want_input, {cs.ind: cs.bn_train for cs in self.convs.values()})
        for op, s in zip(self.ops, sched):
            if s.visited and op.kind == 'conv' and not (op.has_raw or op.first_live):
                raise RuntimeError("Darknet backward: block %d was run without gradient bookkeeping by the last forward "
                                   "(it was frozen then, or the forward ran in inference form) - its raw conv output "
                                   "does not exist" % op.ind)
        if not want_params:
            return self._backward_body(None, want_input, sched)
        # ONE flat gradient buffer per model and device, reused by every backward of every plan (the layout depends on the
        # model only): the returned gradients are views of it.  Reuse is safe only while nothing else still views the
        # buffer (optimizer.zero_grad(set_to_none=True) - torch's default - drops the .grad views; a caller that keeps or
        # accumulates gradients across backwards gets a fresh buffer, the old one stays with the tensors that view it).
        # Zeroed (in the body): the filter-gradient kernel accumulates channels-last parameters' gradients straight into it.
        ent = self.net._flat_grads.get(self.device)
        flat = None
        if ent is not None and ent[0].numel() == self.grad_total and not _storage_shared(ent[0], ent[1], self.net._params()):
            flat = ent[0]
        if flat is None:
            flat = torch.empty(self.grad_total, dtype=torch.float32, device=self.device)
            self.net._flat_grads[self.device] = (flat, _storage_refs(flat))
        flat.record_stream(self.side_stream)
        self.last_flat_grad = flat
        return self._backward_body(flat, want_input, sched)

    def _backward_body(self, flat, want_input, sched):
        """flat None: input-only backward (see backward).  sched: the pass's backward_schedule."""
        B = self.B
        st = torch.cuda.current_stream().cuda_stream
        call = _lib.call
        written = set()
        fused_stats = set()      # blocks whose BatchNorm-backward reductions were produced by their consumer's dgrad launch
        written.add(self.last)
        if flat is not None:
            flat.zero_()
            for op, s in zip(self.ops, sched):      # gradient staging of the parameters that are not channels-last
                # (the fused first block's filter gradient is WRITTEN, not accumulated)
                if s.wgrad and not op.packed and not op.first_live:
                    self._gbuf(op).zero_()
        # Filter gradients run on a second stream: wgrad(l) only needs dY(l) and the saved input activation, so it
        # overlaps the dgrad(l) -> BN-backward(l-1) chain of the main stream and fills the idle CUs of its last wave.
        main = torch.cuda.current_stream()
        side = main if self.serial_backward else self.side_stream
        if self.dgrad_ready is not None:
            main.wait_event(self.dgrad_ready)       # dgrad filter repacks were queued during forward
        else:
            self._prepare_backward(tune=False)      # the saved conv outputs are live: no timing / verify launches now
            by_ind = {s.ind: s for s in sched if s.kind == 'conv'}
            for ind in sorted(self.convs.keys(), reverse=True):   # forward ran without grad bookkeeping: repack now
                cs = self.convs[ind]
                if not cs.first and by_ind[ind].dgrad[0]:
                    self._repack_dgrad(cs, main)
        out_grads = {}
        tail_sched = side is not main and os.environ.get('SSP_TAIL_SCHED', '1') != '0'
        if self.reducer is not None and flat is not None:
            self.reducer.begin(flat)

        def gview(prm, channels_last=False):
            off, n, shape = self.grad_layout[id(prm)]
            if channels_last:      # the parameter's own strides: [Cout][kh][kw][Cin] in memory
                return torch.as_strided(flat, shape, prm.stride(), off)
            return flat[off:off + n].view(shape)

        def grad_in(a):
            """Gradient buffer of map a's producer, and whether the launch accumulates into it (marks it written)."""
            gin = self._grad_buf(a.producer, a)
            acc = 1 if a.producer in written else 0
            written.add(a.producer)
            return gin, acc

        def grad_scratch(a):
            """... of a producer that gets no gradient (a frozen branch): its buffer is written and never read."""
            return self._grad_buf(a.producer, a), 0

        for op, s in zip(reversed(self.ops), reversed(sched)):
            if not s.visited or op.oind not in written:
                # nothing downstream of this block reaches the output, or nothing upstream of it wants a gradient: no
                # launch - its (zero) range of the flat buffer is complete, and the reducer's buckets close in order
                if op.kind == 'conv' and flat is not None and self.reducer is not None:
                    with torch.cuda.stream(side):
                        self.reducer.layer_done(flat, op.grad_lo, op.grad_hi)
                continue
            g = self.grads[op.oind]
            kind = op.kind
            if kind == 'conv':
                self._conv_bwd(op, s, g, flat, gview, out_grads, written, fused_stats, main, side, tail_sched)
            elif kind == 'shortcut':
                a, b = op.srcs
                ga, acc_a = grad_in(a) if s.dgrad[0] else grad_scratch(a)
                # (from = -1: one buffer - the kernel adds 2 g')
                gb, acc_b = (ga, acc_a) if b is a else (grad_in(b) if s.dgrad[1] else grad_scratch(b))
                out = op.out
                call('ssp_shortcut_bwd', g.ptr, g.ld, out.ptr, out.ld, ga.ptr, ga.ld, acc_a, gb.ptr, gb.ld, acc_b,
                     _pad4(out.C), B * out.H * out.W, op.slope, st)
            elif kind in ('alias', 'concat'):
                off = 0
                for n, (a, d) in enumerate(zip(op.srcs, s.dgrad)):
                    if d and n == 0 and kind == 'concat' and op.inplace:
                        # the upsample's gradient IS columns [0, C) of this buffer: ssp_upsample_bwd reads it in place
                        # (its only consumer is this route, so nothing else adds to it)
                        self.grads[a.producer] = _Act(g.t, g.off, a.C, a.H, a.W, g.ld)
                        written.add(a.producer)
                    elif d:
                        gin, acc = grad_in(a)
                        call('ssp_copy_channels', _ptr(g.t, g.off + off), g.ld, gin.ptr, gin.ld, a.C, B * a.H * a.W, acc, st)
                    off += a.C
            elif s.dgrad[0]:
                src = op.srcs[0]
                gin, acc = grad_in(src)
                if kind in ('maxpool', 'maxpool_s1'):
                    call('ssp_maxpool_bwd' if kind == 'maxpool' else 'ssp_maxpool_s1_bwd', src.ptr, src.ld, g.ptr, g.ld,
                         gin.ptr, gin.ld, _pad4(src.C), B, src.H, src.W, acc, st)
                elif kind == 'reorg':
                    call('ssp_reorg', g.ptr, g.ld, gin.ptr, gin.ld, src.C, B, src.H, src.W, 1, acc, st)
                elif kind == 'upsample':
                    call('ssp_upsample_bwd', g.ptr, g.ld, gin.ptr, gin.ld, _pad4(src.C), B, src.H, src.W, op.stride, acc, st)
                elif kind == 'avgpool':
                    call('ssp_avgpool_bwd', g.ptr, g.ld, gin.ptr, gin.ld, _pad4(src.C), B, src.H, src.W, acc, st)
                else:
                    call('ssp_softmax_bwd', op.out.ptr, op.out.ld, g.ptr, g.ld, gin.ptr, gin.ld, src.C, B * src.H * src.W,
                         acc, st)
        dx = None
        if want_input:
            # NHWC [B*H*W][in_cp] -> the (B, C, H, W) input gradient
            o = self.input_act
            dx = torch.empty(B, self.in_c, self.H, self.W, dtype=torch.float32, device=self.device)
            if INPUT in written:
                call('ssp_nhwc_to_nchw', self.grads[INPUT].ptr, dx.data_ptr(), B, self.in_c, o.H, o.W, o.ld, st)
            else:
                dx.zero_()          # no path from the input reaches the output
        if flat is not None:
            main.wait_stream(side)              # every filter gradient is complete before autograd hands them out
        return out_grads, dx

    def _conv_bwd(self, cs, s, g, flat, gview, out_grads, written, fused_stats, main, side, tail_sched):
        """Backward launches of conv block `cs` from the gradient g of its (pooled) output, as its schedule entry `s` lists
        them: BatchNorm / activation backward, bias gradient, filter gradient on the side stream, data gradient into the
        producer of its input (for the first block: into the input's gradient buffer).  flat None: input-only backward,
        no parameter gradient work."""
        B = self.B
        call = _lib.call
        st, st2 = main.cuda_stream, side.cuda_stream
        training = cs.bn_train          # the mode this block's forward ran in
        v = cs.vec
        params = flat is not None

        def hand_out(prm):
            gv = gview(prm)
            out_grads[id(prm)] = gv
            return gv

        if cs.coutp != cs.cout:
            # The padding columns of g are whatever its writers left: a strided data gradient writes cin of the cinp columns
            # (the rest is torch.empty memory - NaN in a poisoned allocator), a stride-1 one the products of an unpacked
            # operand's padding.  Every pass below reads coutp columns, and the in-place BatchNorm / activation backward
            # writes them into the raw output, where the next forward's activation pass picks them up (the conv launch
            # writes cout columns): 0 * NaN in this block's data gradient or in the consumer's forward.  Define them here.
            with torch.cuda.stream(main):
                g.t.view(-1, g.ld)[:, g.off + cs.cout:g.off + cs.coutp].zero_()
        if cs.first_live:
            # first block, fused form: every backward pass recomputes the convolution from the input.  The reductions
            # feed dy_raw, which each of the passes below needs (a frozen gamma / beta lands in scratch).
            dg_ptr = hand_out(cs.bnm.weight).data_ptr() if s.dgamma else v[6].data_ptr()
            db_ptr = hand_out(cs.bnm.bias).data_ptr() if s.dbeta else v[7].data_ptr()
            wptr = self._wbuf(cs).data_ptr()
            call('ssp_first_bwd_reduce', cs.inp.ptr, wptr, g.ptr, g.ld, v[2].data_ptr(), v[3].data_ptr(),
                 v[0].data_ptr(), v[1].data_ptr(), cs.slope, cs.first_partial.data_ptr(), B, cs.H, cs.W, st)
            call('ssp_bn_bwd_finalize', cs.first_partial.data_ptr(), cs.first_groups, cs.cout, cs.M,
                 1 if training else 0, 0, dg_ptr, db_ptr, v[4].data_ptr(), v[5].data_ptr(), st)
            if s.dgrad[0]:          # main stream, after the finalize: it reads what the filter gradient below reads
                self._first_input_dgrad(cs, g, written, st)
            if not params:
                return
            # The step's tail is a dependency chain: dgrad of the block's consumer -> this reduce -> this filter
            # gradient (HBM-bound: it re-reads the 1.4 GB output gradient).  With the tail schedule the consumer's
            # filter gradient (MFMA-bound) was held back behind its data gradient and is running on the side
            # stream NOW: this pass stays on the main stream and overlaps it, instead of queueing behind it.
            fst = st if tail_sched else st2
            if s.wgrad:
                if not tail_sched:
                    side.wait_stream(main)
                gw = gview(cs.conv.weight, False)
                if cs.first_wpart is None:      # per-workgroup partial gradients, summed in float64
                    cs.first_wpart = torch.empty(_lib.query('ssp_first_wgrad_workspace_floats', B, cs.H, cs.W),
                                                 dtype=torch.float32, device=self.device)
                call('ssp_first_bwd_wgrad', cs.inp.ptr, wptr, g.ptr, g.ld, v[2].data_ptr(), v[3].data_ptr(),
                     v[0].data_ptr(), v[1].data_ptr(), v[4].data_ptr(), v[5].data_ptr(), cs.slope,
                     self._gbuf(cs).data_ptr(), cs.first_wpart.data_ptr(), cs.first_wpart.numel(), B, cs.H, cs.W, fst)
                call('ssp_unpack_grad', self._gbuf(cs).data_ptr(), gw.data_ptr(), cs.cout, cs.cin, cs.cinp, cs.k, fst)
                out_grads[id(cs.conv.weight)] = gw
            if self.reducer is not None:
                if tail_sched or not s.wgrad:
                    side.wait_stream(main)
                with torch.cuda.stream(side):
                    self.reducer.layer_done(flat, cs.grad_lo, cs.grad_hi)
            return
        if cs.needs_act:
            if cs.bn and not s.bn_reduce:
                # BatchNorm in eval() with gamma and beta frozen: the block is an affine map + activation, its backward
                # one apply pass - no reduction, no finalize
                call('ssp_bn_act_bwd_affine', cs.raw.data_ptr(), cs.ldraw, g.ptr, g.ld, cs.raw.data_ptr(), cs.ldraw,
                     v[2].data_ptr(), v[3].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), cs.coutp, B, cs.H, cs.W,
                     1 if cs.pool else 0, cs.slope, st)
            else:
                # two-level reduction (per-workgroup partials -> fp64 finalize).  The single-pass form of
                # ssp_bn_act_bwd (atomics into the zeroed gradient, no finalize launch) measured 1.1 ms SLOWER
                # per step: 1024 workgroups hammering the same 2*C addresses serialise in the L2.
                direct = cs.bn and cs.coutp == cs.cout      # the reductions land in the gradients themselves
                dg_ptr = hand_out(cs.bnm.weight).data_ptr() if (direct and s.dgamma) else v[6].data_ptr()
                db_ptr = hand_out(cs.bnm.bias).data_ptr() if (direct and s.dbeta) else v[7].data_ptr()
                partial = self.bn_partial.data_ptr()
                if cs.ind in fused_stats:
                    # the two reductions came out of the consumer's data-gradient launch: finalize + apply only
                    ptile, rows, folded = cs.bnp
                    call('ssp_bn_act_bwd_partials', cs.raw.data_ptr(), cs.ldraw, g.ptr, g.ld, cs.raw.data_ptr(),
                         cs.ldraw, v[2].data_ptr(), v[3].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), cs.coutp, B,
                         cs.H, cs.W, cs.slope, 1 if training else 0, ptile.data_ptr(), rows, 1 if folded else 0,
                         dg_ptr, db_ptr, v[4].data_ptr(), v[5].data_ptr(), st)
                else:
                    call('ssp_bn_act_bwd', cs.raw.data_ptr(), cs.ldraw, g.ptr, g.ld, cs.raw.data_ptr(), cs.ldraw,
                         v[2].data_ptr(), v[3].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), cs.coutp, B, cs.H, cs.W,
                         1 if cs.pool else 0, cs.slope, 1 if training else 0, partial,
                         dg_ptr, db_ptr, v[4].data_ptr(), v[5].data_ptr(), st)
                if cs.bn and not direct:
                    if s.dgamma:
                        hand_out(cs.bnm.weight).copy_(v[6][:cs.cout])
                    if s.dbeta:
                        hand_out(cs.bnm.bias).copy_(v[7][:cs.cout])
            dy_ptr, dy_ld = cs.raw.data_ptr(), cs.ldraw
        else:
            dy_ptr, dy_ld = g.ptr, g.ld
        if s.bias:
            db = hand_out(cs.conv.bias)
            call('ssp_colsum', dy_ptr, dy_ld, cs.M, cs.cout, db.data_ptr(), st)
        src = None if cs.first else cs.inp.producer
        # tail schedule: the consumer of the fused first block (layer 2) runs its data gradient - the head of the
        # chain that ends the step - BEFORE its filter gradient is released on the side stream
        owner = None if src is None else (self.convs.get(src - 1) if src in self.fused_pool else self.convs.get(src))
        defer = params and tail_sched and owner is not None and owner.first_live and s.dgrad[0]
        # adjoint-form layer whose filter gradient runs too: dY is transformed ONCE, on the main stream, into the dM slot
        # of the layer's filter-gradient workspace - both gradients contract those planes.  (No filter gradient in this
        # schedule - frozen parameters, input-only backward: the data-gradient launch transforms dY into its own workspace.)
        dm_ptr = None
        if cs.dgrad_adj and s.dgrad[0] and s.wgrad and cs.packed and cs.wgrad_wino:
            t = cs.wgrad_wino        # V [P][T][cinp] | dM | dU (csrc/conv_wgrad.hip)
            dm_ptr = _ptr(self._wino_ws(cs), (t + 2) ** 2 * _lib.query('ssp_conv_wino_tiles', B, cs.H, cs.W, t) * cs.cinp)
            call('ssp_wino_outgrad_transform_t', dy_ptr, dy_ld, dm_ptr, B, cs.H, cs.W, cs.cout, cs.wgrad_wino, st)
        if defer:
            self._dgrad(cs, src, dy_ptr, dy_ld, written, fused_stats, st, s.fold_bn, dm_ptr)
        if params:
            side.wait_stream(main)          # dY(l) (and the zeroed packed-gradient buffer) are ready
        if s.wgrad:
            gw = gview(cs.conv.weight, cs.packed)
            wg_name = 'ssp_conv_s2_wgrad' if cs.stride == 2 else 'ssp_conv_wgrad'      # (both take the INPUT map's H x W)
            det = self.deterministic['mode']

            def run_direct(dst):
                if det:      # ordered form: per-range slabs, summed in order (the split is the recorded one)
                    ows = self._wgrad_ordered_ws()
                    call('ssp_conv_wgrad_ordered', dy_ptr, cs.inp.ptr, dst, B, cs.Hi, cs.Wi, cs.cinp, cs.cout, dy_ld, cs.inp.ld,
                         cs.k, cs.stride, cs.wgrad_det[2], 0, ows.data_ptr(), ows.numel(), st2)
                else:
                    call(wg_name, dy_ptr, cs.inp.ptr, dst, B, cs.Hi, cs.Wi, cs.cinp, cs.cout, dy_ld, cs.inp.ld, cs.k, st2)
            if cs.depthwise:
                # per-range partials, then a float64 finish that WRITES the (C, 1, 3, 3) gradient in place (no atomics: the
                # launch is its own ordered form)
                dws = self._dwconv_ws()
                call('ssp_dwconv_wgrad', dy_ptr, cs.inp.ptr, gw.data_ptr(), B, cs.Hi, cs.Wi, cs.cin, dy_ld, cs.inp.ld, cs.stride,
                     0, dws.data_ptr(), dws.numel(), st2)
            elif cs.packed and cs.wgrad_wino:
                wws = self._wino_ws(cs)
                # (dy = NULL: dM is in its slot of wws already, see above)
                wargs = (None if dm_ptr is not None else dy_ptr, None if cs.v_live else cs.inp.ptr, gw.data_ptr(), B, cs.H, cs.W,
                         cs.cinp, cs.cout, dy_ld, cs.inp.ld, cs.wgrad_wino)
                if det:
                    call('ssp_conv_wgrad_wino_ordered', *(wargs + (cs.wgrad_det[2], wws.data_ptr(), wws.numel(), st2)))
                else:
                    call('ssp_conv_wgrad_wino_t', *(wargs + (wws.data_ptr(), wws.numel(), st2)))
                cs.v_live = False
            elif cs.packed:       # accumulate in place: the gradient has the parameter's channels-last layout
                run_direct(gw.data_ptr())
            else:
                run_direct(self._gbuf(cs).data_ptr())
                call('ssp_unpack_grad', self._gbuf(cs).data_ptr(), gw.data_ptr(), cs.cout, cs.cin, cs.cinp, cs.k, st2)
            out_grads[id(cs.conv.weight)] = gw
        if params and self.reducer is not None:
            with torch.cuda.stream(side):   # the all-reduce of a finished bucket is ordered after its wgrads
                self.reducer.layer_done(flat, cs.grad_lo, cs.grad_hi)
        if s.dgrad[0] and not defer:
            if cs.first:
                self._input_dgrad(cs, dy_ptr, dy_ld, written, st)
            else:
                self._dgrad(cs, src, dy_ptr, dy_ld, written, fused_stats, st, s.fold_bn, dm_ptr)

    def _input_gbuf(self, written):
        """The input's gradient buffer, NHWC [B*H*W][in_cp], and whether a launch accumulates into it (marks it written)."""
        gin = self._grad_buf(INPUT, self.input_act)
        acc = 1 if INPUT in written else 0
        written.add(INPUT)
        return gin, acc

    def _input_dgrad(self, cs, dy_ptr, dy_ld, written, st):
        """dL/dx of an un-fused first conv: ssp_conv_dgrad into the 4-channel input gradient (Cin_dx = in_cp; the operand's
        padding rows stay zero, so the padding channel is written as zero).  The operand is built here, on first use - a
        plan that is never asked for an input gradient neither holds nor repacks it."""
        call = _lib.call
        if self._dpack_in is None:
            self._dpack_in = torch.zeros(self.in_cp * cs.k * cs.k * cs.coutp, dtype=torch.float32, device=self.device)
        src = cs.conv.weight.detach()
        if not cs.packed:
            src = src.contiguous()
        call('ssp_repack_dgrad_packed' if cs.packed else 'ssp_repack_dgrad', src.data_ptr(), self._dpack_in.data_ptr(),
             cs.cout, cs.cin, cs.coutp, cs.k, st)
        gin, acc = self._input_gbuf(written)
        # plan 0: the library's heuristic (the tuner never times this launch); no split-K workspace is needed at K = 9 * Cout
        call('ssp_conv_dgrad', dy_ptr, self._dpack_in.data_ptr(), gin.ptr, self.B, cs.H, cs.W, cs.coutp, self.in_cp,
             dy_ld, gin.ld, cs.k, acc, 0, None, 0, st)

    def _first_input_dgrad(self, cs, g, written, st):
        """dL/dx of the fused first block (ssp_first_bwd_dgrad): recomputes the convolution per tile, never stores it."""
        gin, acc = self._input_gbuf(written)
        if acc:
            raise NotImplementedError("the network input feeds the fused first block and another block: its gradient "
                                      "would need an accumulating ssp_first_bwd_dgrad")
        v = cs.vec
        _lib.call('ssp_first_bwd_dgrad', cs.inp.ptr, self._wbuf(cs).data_ptr(), g.ptr, g.ld, v[2].data_ptr(),
                  v[3].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), v[4].data_ptr(), v[5].data_ptr(), cs.slope, gin.ptr,
                  self.B, cs.H, cs.W, st)


def _trainable(params, needs):
    """ids of the parameters autograd wants a gradient for."""
    return frozenset(id(p) for p, n in zip(params, needs) if n)


class _DarknetFn(torch.autograd.Function):
    """One autograd node for the whole network: forward/backward are sequences of HIP launches."""

    @staticmethod
    def forward(ctx, plan, training, x, *params):
        ctx.plan = plan
        ctx.params = params
        need = ctx.needs_input_grad
        y = plan.forward(x, training, need_grad=True, trainable=_trainable(params, need[3:]), want_input=need[2])
        ctx.generation = plan.generation
        return y

    @staticmethod
    def backward(ctx, grad_out):
        plan = ctx.plan if ctx.plan is not None else ctx.plan_ref()
        if plan is None:
            raise RuntimeError("Darknet backward called twice on the same forward, and the plan of that input shape has "
                               "left the plan cache since (another resolution took its memory): run the forward again")
        if plan.generation != ctx.generation:
            raise RuntimeError("Darknet backward after a newer forward on the same input shape: the plan's saved "
                               "activations were overwritten")
        want_x = ctx.needs_input_grad[2]
        want_p = _trainable(ctx.params, ctx.needs_input_grad[3:])
        grads, dx = plan.backward(grad_out.contiguous(), want_input=want_x, want_params=want_p if (want_p or want_x) else True)
        # Until its backward has run the node keeps its plan alive (forward at shape A, forward at shape B, backward of A
        # works whatever the cache evicted).  Afterwards only the cache does: a caller that still holds the loss tensor of the
        # previous resolution (every training loop does, until it assigns the next one) must not keep that resolution's
        # 30 - 65 GB of buffers next to the new plan's - that pair was the peak of the multi-scale soak.
        ctx.plan_ref = weakref.ref(plan)
        ctx.plan = None
        res = [None, None, dx]
        for p in ctx.params:
            res.append(grads.get(id(p)))
        return tuple(res)


class _DarknetEvalFn(torch.autograd.Function):
    """Inference-mode forward with autograd enabled - what the reference's unchanged valid.py / train.py test() run:
    `Variable(data, volatile=True)` (valid.py:113) is a no-op on current torch, so grad mode stays on.  The forward takes
    the cheap inference chain (fused conv + BN affine + leaky launches, cached BN constants, no data-gradient operand
    repacks); in the rare case that somebody does call backward on it (frozen-BN fine-tuning), backward first re-runs
    the forward in its activation-keeping form and then the normal backward chain."""

    @staticmethod
    def forward(ctx, plan, x, *params):
        ctx.plan = plan
        ctx.params = params
        ctx.x = x
        ctx.xver = x._version
        return plan.forward(x, False)

    @staticmethod
    def backward(ctx, grad_out):
        plan = ctx.plan
        if ctx.x._version != ctx.xver:
            raise RuntimeError("Darknet (eval mode) backward: the input tensor was modified in place after the forward")
        want_x = ctx.needs_input_grad[1]
        want_p = _trainable(ctx.params, ctx.needs_input_grad[2:])
        if not (want_p or want_x):
            want_p = _trainable(ctx.params, [True] * len(ctx.params))
        # recompute, keeping the raw conv outputs of the blocks the backward visits
        plan.forward(ctx.x, False, need_grad=True, trainable=want_p, want_input=want_x)
        grads, dx = plan.backward(grad_out.contiguous(), want_input=want_x, want_params=want_p)
        res = [None, dx]
        for p in ctx.params:
            res.append(grads.get(id(p)))
        return tuple(res)

"""SGD on one fused HIP launch - the optimizer side of the training step.

The reference trains with `optim.SGD(model.parameters(), lr=learning_rate/batch_size, momentum=momentum, dampening=0,
weight_decay=decay*batch_size)` (train.py:388), `optimizer.zero_grad()` / `optimizer.step()` per batch
(train.py:89,106) and rewrites `param_group['lr']` every batch (train.py:44-45).  `SGD` below keeps that constructor,
`param_groups`, `zero_grad`, `state_dict` (it is a torch.optim.Optimizer) and the update rule of torch.optim.SGD, but
runs the whole step as ONE ssp_sgd_step launch:

* Plan.backward (engine.py) already returns every parameter gradient as a view of one flat fp32 buffer, in reverse
  layer order (the buffer the RCCL all-reduce works on).  At the first step the optimizer adopts exactly that layout:
  it moves the parameters into one flat buffer (each `p.data` becomes a view of it - the module tree is unchanged)
  and allocates one flat momentum buffer, so parameter i, its gradient and its momentum sit at the same offset.
* A step whose gradients are such views (the normal case) is then a single pass over 3 x 202 MB; gradients that are
  not (accumulated over several backwards, clipped copies, ...) are handled per parameter with the same kernel.

* Parameter groups with different hyper-parameters (the group list train.py:381-387 builds: no weight decay on the
  BatchNorm / bias parameters) and an optimizer that holds only part of a model (a fine-tuned head under a frozen trunk)
  are still ONE launch, ssp_sgd_step_table: a device-resident table of segments {parameter offset, gradient offset,
  momentum offset, length, hyper-parameter tuple} over the optimizer's OWN flat parameter / momentum buffers (sized by
  what it holds: `flat_numel`) and the backward's flat gradient buffer.  The at most 16 distinct tuples travel by value
  with the launch, so the per-batch `lr` rewrite uploads nothing; the table is rebuilt only when the layout or the group
  membership changes.  Parameters the optimizer does not hold are never read or written.

`Adam` / `AdamW` (further down) keep torch.optim.Adam's constructor, state keys and update rule on the same flat layout -
one ssp_adam_step launch, or one ssp_adam_step_table launch for groups, subsets and differing step counts - and
`clip_grad_norm_` clips the global 2-norm of the flat gradient views in two launches without a host synchronisation
(DESIGN.md section 1b).

No CPU path: parameters must be on the GPU.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .engine import weights_changed


def _dense(t):
    """Contiguous, or channels-last (conv filters as Darknet keeps them): numel consecutive floats either way."""
    return t.is_contiguous() or (t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous())


def _same_layout(a, b):
    """Same shape and the same strides on every dimension that has more than one element."""
    return a.shape == b.shape and all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1)


MAX_TUPLES = 16      # SSP_SGD_MAX_TUPLES (include/ssp_hip.h)


def build_segment_table(entries, max_tuples=MAX_TUPLES):
    """The segment table of one ssp_sgd_step_table launch - a pure function of what the optimizer holds.

    entries: one (numel, gradient offset, hyper, has_momentum_state) per parameter that has a gradient, in optimizer
    order; gradient offset = the float offset of the parameter's gradient in the backward's flat buffer, or None when the
    gradient is no such view; hyper = (lr, momentum, dampening, weight_decay, nesterov).

    Returns None when the per-parameter launches must run instead: a gradient that is not a flat view (or misaligned),
    more than `max_tuples` distinct hyper-parameter tuples, or a tuple with momentum whose parameters partly have momentum
    state and partly do not (no single `first` flag).  Else (rows, tuples, flat_numel):
      rows    [[parameter offset, gradient offset, momentum offset, numel, tuple index]] - parameter and momentum offsets
              pack the held parameters in order, each rounded up to 4 floats; nothing else is named
      tuples  [(lr, momentum, dampening, weight_decay, nesterov, first)] in order of first use
      flat_numel  floats of the parameter (and momentum) buffer."""
    if not entries:
        return None
    index = {}
    state = {}
    rows = []
    off = 0
    for numel, goff, hyper, has_state in entries:
        if goff is None or goff % 4 or goff < 0 or numel < 1:
            return None
        hyper = (float(hyper[0]), float(hyper[1]), float(hyper[2]), float(hyper[3]), bool(hyper[4]))
        t = index.setdefault(hyper, len(index))
        if len(index) > max_tuples:
            return None
        if hyper[1] != 0:
            if state.setdefault(t, bool(has_state)) != bool(has_state):
                return None
        rows.append([off, int(goff), off, int(numel), t])
        off += (int(numel) + 3) // 4 * 4
    tuples = [None] * len(index)
    for hyper, t in index.items():
        first = hyper[1] != 0 and not state[t]
        tuples[t] = hyper[:4] + (1.0 if hyper[4] else 0.0, 1.0 if first else 0.0)
    return rows, tuples, off


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %s" % lr)
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %s" % momentum)
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %s" % weight_decay)
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super(SGD, self).__init__(params, defaults)
        self._flat_p = None      # flat parameter buffer (views handed to the modules)
        self._flat_m = None      # flat momentum buffer, same layout
        self._layout = None      # [(param, offset, numel)]
        self._first = True
        self.fused_steps = 0     # steps done as one launch (introspection / tests)
        self.table_steps = 0     # steps done as one ssp_sgd_step_table launch
        self._tab = None         # the table path's flat buffers, device table and what they were built for

    # ---- flat layout ---------------------------------------------------------------------------------------------
    def _all_params(self):
        return [p for g in self.param_groups for p in g['params']]

    @staticmethod
    def _flat_grads(params):
        """(storage base pointer, [(param, offset)], total) when every .grad is a float32 view of ONE storage with
        non-overlapping 16-byte aligned ranges, else None."""
        base = None
        items = []
        for p in params:
            g = p.grad
            if g is None or g.dtype != torch.float32 or not g.is_cuda:
                return None
            # dense in memory with the parameter's own strides (contiguous, or channels-last conv filters)
            if not (_dense(p) and _same_layout(g, p)):
                return None
            st = g.untyped_storage()
            if base is None:
                base = st
            elif st.data_ptr() != base.data_ptr():
                return None
            off = g.storage_offset()
            if off % 4:
                return None
            items.append((p, off))
        if base is None:
            return None
        order = sorted(items, key=lambda t: t[1])
        for (pa, oa), (pb, ob) in zip(order[:-1], order[1:]):
            if oa + pa.numel() > ob:
                return None
        total = base.nbytes() // 4
        return base, items, total

    def _adopt_layout(self, items, total, device):
        flat_p = torch.zeros(total, dtype=torch.float32, device=device)
        flat_m = torch.zeros(total, dtype=torch.float32, device=device)
        layout = []
        for p, off in items:
            n = p.numel()
            # views with the parameter's own strides (channels-last filters stay channels-last), element for element
            # at the offsets of the gradient views
            pv = torch.as_strided(flat_p, p.shape, p.stride(), off)
            mv = torch.as_strided(flat_m, p.shape, p.stride(), off)
            pv.copy_(p.data)
            old = self.state.get(p, {}).get('momentum_buffer')
            if old is not None:
                mv.copy_(old)
                self._first = False      # momentum carried over (per-parameter steps or load_state_dict): not a first step
            p.data = pv
            self.state[p]['momentum_buffer'] = mv
            layout.append((p, off, n))
        self._flat_p, self._flat_m, self._layout = flat_p, flat_m, layout
        self._tab = None         # (a segment-table layout, if any, is gone)

    def _layout_valid(self, items):
        if self._layout is None or len(items) != len(self._layout):
            return False
        base = self._flat_p.data_ptr()
        mbase = self._flat_m.data_ptr()
        for (p, off), (q, qoff, n) in zip(items, self._layout):
            if p is not q or off != qoff or p.data_ptr() != base + 4 * off:
                return False      # model.cuda()/load_state_dict replaced a tensor, or the plan's layout changed
            m = self.state.get(p, {}).get('momentum_buffer')
            if m is None or m.data_ptr() != mbase + 4 * off:
                return False      # optimizer.load_state_dict() swapped the momentum tensors: re-adopt (copies them in)
        return True

    def _uniform_hyper(self):
        g0 = self.param_groups[0]
        keys = ('lr', 'momentum', 'dampening', 'weight_decay', 'nesterov')
        for g in self.param_groups[1:]:
            if any(g[k] != g0[k] for k in keys):
                return None
        return g0

    # ---- segment table ---------------------------------------------------------------------------------------------
    @property
    def flat_numel(self):
        """Floats of the flat parameter buffer the optimizer works on (0 before its first fused step)."""
        if self._tab is not None:
            return self._tab['numel']
        return 0 if self._flat_p is None else self._flat_p.numel()

    def _table_step(self, params, flat, st):
        """One ssp_sgd_step_table launch over the optimizer's own segments; False = the per-parameter launches must run."""
        base, items, total = flat
        goff = {id(p): off for p, off in items}
        held, entries = [], []
        for group in self.param_groups:
            hyper = (group['lr'], group['momentum'], group['dampening'], group['weight_decay'], group['nesterov'])
            for p in group['params']:
                if p.grad is None:
                    continue
                held.append(p)
                entries.append((p.numel(), goff[id(p)], hyper, self.state.get(p, {}).get('momentum_buffer') is not None))
        built = build_segment_table(entries)
        if built is None:
            return False
        rows, tuples, numel = built
        tab = self._tab
        key = (tuple(id(p) for p in held), tuple(map(tuple, rows)))
        ok = tab is not None and tab['key'] == key
        if ok:
            pb, mb = tab['p'].data_ptr(), tab['m'].data_ptr()
            for p, row in zip(held, rows):
                m = self.state.get(p, {}).get('momentum_buffer')
                if p.data_ptr() != pb + 4 * row[0] or (m is not None and m.data_ptr() != mb + 4 * row[2]):
                    ok = False      # model.cuda() / load_state_dict replaced a tensor: adopt again (copies them in)
                    break
        if not ok:
            dev = held[0].device
            flat_p = torch.zeros(numel, dtype=torch.float32, device=dev)
            flat_m = torch.zeros(numel, dtype=torch.float32, device=dev)
            for p, row in zip(held, rows):
                pv = torch.as_strided(flat_p, p.shape, p.stride(), row[0])
                pv.copy_(p.data)
                p.data = pv
                if tuples[row[4]][1] != 0:
                    mv = torch.as_strided(flat_m, p.shape, p.stride(), row[2])
                    old = self.state.get(p, {}).get('momentum_buffer')
                    if old is not None:
                        mv.copy_(old)
                    self.state[p]['momentum_buffer'] = mv
            host = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
            tab = self._tab = dict(key=key, p=flat_p, m=flat_m, numel=numel, host=host,
                                   dev=torch.from_numpy(host).to(dev), held=held)
            self._flat_p = self._flat_m = self._layout = None      # the single-range layout (if any) is gone
        hyper = (ctypes.c_float * (6 * len(tuples)))(*[v for t in tuples for v in t])
        g0 = held[0].grad
        _lib.call('ssp_sgd_step_table', tab['p'].data_ptr(), g0.data_ptr() - 4 * g0.storage_offset(), tab['m'].data_ptr(),
                  numel, total, numel, tab['dev'].data_ptr(), tab['host'].ctypes.data, len(rows),
                  ctypes.cast(hyper, ctypes.c_void_p), len(tuples), st)
        self._first = False
        self.table_steps += 1
        weights_changed()
        return True

    # ---- step ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = [p for p in self._all_params() if p.grad is not None]
        if not params:
            return loss
        for p in params:
            if not p.is_cuda:
                raise RuntimeError("singleshotpose_amd.optim.SGD runs on the MI355X HIP kernel only: parameter on %s" % p.device)
        st = torch.cuda.current_stream(params[0].device).cuda_stream
        hyper = self._uniform_hyper()
        flat = self._flat_grads(params)
        # one range: uniform hyper-parameters over parameters that fill the backward's whole gradient layout
        whole = (flat is not None and hyper is not None and len(params) == len(self._all_params()) and
                 sum((p.numel() + 3) // 4 * 4 for p in params) == flat[2])
        if flat is not None and not whole and self._table_step(params, flat, st):
            return loss
        if whole:
            base, items, total = flat
            if not self._layout_valid(items):
                self._adopt_layout(items, total, params[0].device)
                # momentum carried over from per-parameter steps keeps `first` as it was
            g0 = params[0].grad
            gbase = g0.data_ptr() - 4 * g0.storage_offset()
            first = 1 if (self._first and hyper['momentum'] != 0) else 0
            _lib.call('ssp_sgd_step', self._flat_p.data_ptr(), gbase, self._flat_m.data_ptr(), total,
                      float(hyper['lr']), float(hyper['momentum']), float(hyper['dampening']),
                      float(hyper['weight_decay']), 1 if hyper['nesterov'] else 0, first, st)
            self._first = False
            self.fused_steps += 1
            weights_changed()      # raw-pointer writes do not bump tensor versions: invalidate packed-filter caches
            return loss
        # per-parameter launches: mixed hyper-parameters, missing or non-flat gradients
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                g = p.grad
                if not _dense(p.data):
                    raise RuntimeError("SGD: parameter is neither contiguous nor channels-last")
                if g.dtype != torch.float32 or not _same_layout(g, p):
                    g = torch.empty_like(p.data).copy_(g)      # same memory order as the parameter
                state = self.state[p]
                buf = state.get('momentum_buffer')
                first = 0
                if group['momentum'] != 0 and buf is None:
                    buf = torch.zeros_like(p.data)
                    state['momentum_buffer'] = buf
                    first = 1
                if (p.data_ptr() | g.data_ptr() | (buf.data_ptr() if buf is not None else 0)) & 15:
                    raise RuntimeError("SGD: parameter / gradient storage is not 16-byte aligned")
                _lib.call('ssp_sgd_step', p.data_ptr(), g.data_ptr(), buf.data_ptr() if buf is not None else None,
                          p.numel(), float(group['lr']), float(group['momentum']), float(group['dampening']),
                          float(group['weight_decay']), 1 if group['nesterov'] else 0, first, st)
        self._first = False
        weights_changed()
        return loss


# ---- Adam / AdamW ------------------------------------------------------------------------------------------------------
# torch.optim.Adam's update (single-tensor order, include/ssp_hip.h: ssp_adam_step) on the same flat layout: a step is ONE
# ssp_adam_step launch when uniform hyper-parameters and equal step counts cover the backward's whole gradient layout,
# ONE ssp_adam_step_table launch for groups, a held subset or differing step counts, per-parameter launches of the same
# kernel otherwise.  The state keeps torch's keys (`step`: a 0-dim float32 CPU tensor, `exp_avg`, `exp_avg_sq`,
# `max_exp_avg_sq`), so state_dict() loads into torch.optim.Adam / AdamW and theirs into these classes.
def _bias_corrections(lr, beta1, beta2, step):
    """(step_size, bc2_sqrt) in Python doubles, exactly as torch/optim/adam.py's single-tensor path forms them."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return lr / bias_correction1, bias_correction2 ** 0.5


def build_adam_segment_table(entries, max_tuples=MAX_TUPLES):
    """The segment table of one ssp_adam_step_table launch - a pure function of what the optimizer holds.

    entries: one (numel, gradient offset, key) per parameter that has a gradient, in optimizer order; gradient offset as
    in build_segment_table; key = (lr, beta1, beta2, eps, weight_decay, decoupled, amsgrad, step) with step the
    parameter's step count AFTER this step (parameters whose counts differ need different bias corrections).

    Returns None when the per-parameter launches must run instead (a gradient that is no aligned flat view, more than
    `max_tuples` distinct keys).  Else (rows, keys, flat_numel): rows [[parameter offset, gradient offset, state offset,
    numel, tuple index]] - parameter and state offsets pack the held parameters in order, each rounded up to 4 floats;
    keys in order of first use; flat_numel = floats of the parameter (and of each state) buffer."""
    if not entries:
        return None
    index = {}
    rows = []
    off = 0
    for numel, goff, key in entries:
        if goff is None or goff % 4 or goff < 0 or numel < 1:
            return None
        key = tuple(float(k) for k in key[:5]) + (bool(key[5]), bool(key[6]), float(key[7]))
        t = index.setdefault(key, len(index))
        if len(index) > max_tuples:
            return None
        rows.append([off, int(goff), off, int(numel), t])
        off += (int(numel) + 3) // 4 * 4
    return rows, list(index), off


def _hyper9(key):
    lr, beta1, beta2, eps, wd, decoupled, amsgrad, step = key
    step_size, bc2_sqrt = _bias_corrections(lr, beta1, beta2, step)
    return (lr, beta1, beta2, eps, wd, step_size, bc2_sqrt, 1.0 if decoupled else 0.0, 1.0 if amsgrad else 0.0)


class Adam(torch.optim.Optimizer):
    _decoupled = False
    _name = 'Adam'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("%s: a tensor lr is not supported (lr travels by value with the launch)" % self._name)
        for name, value in (('maximize', maximize), ('capturable', capturable), ('differentiable', differentiable),
                            ('foreach', foreach), ('fused', fused)):
            if value:
                raise ValueError("%s: %s=%r is not supported: the step is this project's own fused HIP launch"
                                 % (self._name, name, value))
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %s" % lr)
        if not 0.0 < eps:
            raise ValueError("Invalid epsilon value: %s (the HIP kernel needs eps > 0)" % eps)
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: %s" % betas[0])
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: %s" % betas[1])
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %s" % weight_decay)
        # torch's own group keys, so that a state_dict moves between these classes and torch's in both directions
        defaults = dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay,
                        amsgrad=bool(amsgrad), maximize=False, foreach=None, capturable=False, differentiable=False,
                        fused=None, decoupled_weight_decay=self._decoupled)
        super(Adam, self).__init__(params, defaults)
        self.fused_steps = 0     # steps done as one ssp_adam_step launch
        self.table_steps = 0     # steps done as one ssp_adam_step_table launch
        self._lay = None         # the flat parameter / state buffers, the device table and what they were built for

    def __setstate__(self, state):
        super(Adam, self).__setstate__(state)
        for group in self.param_groups:
            group.setdefault('amsgrad', False)
            group.setdefault('decoupled_weight_decay', self._decoupled)
            for name in ('maximize', 'capturable', 'differentiable', 'foreach', 'fused'):
                if group.setdefault(name, None if name in ('foreach', 'fused') else False):
                    raise ValueError("%s: a loaded group has %s=%r, which is not supported" % (self._name, name, group[name]))
            for p in group['params']:
                st = self.state.get(p, {})
                if len(st) and not (torch.is_tensor(st['step']) and st['step'].device.type == 'cpu'):
                    st['step'] = torch.tensor(float(st['step']), dtype=torch.float32)      # (a device tensor syncs here, once)

    @property
    def flat_numel(self):
        """Floats of the flat parameter buffer the optimizer works on (0 before its first one-launch step)."""
        return 0 if self._lay is None else self._lay['numel']

    def _key(self, group, step):
        if isinstance(group['lr'], torch.Tensor):
            raise ValueError("%s: a tensor lr is not supported" % self._name)
        return (float(group['lr']), float(group['betas'][0]), float(group['betas'][1]), float(group['eps']),
                float(group['weight_decay']), bool(group['decoupled_weight_decay']), bool(group['amsgrad']), float(step))

    def _init_state(self, p, group):
        """torch's lazy state initialisation; the moment tensors become views of the flat buffers when a layout adopts them."""
        state = self.state[p]
        if len(state) == 0:
            state['step'] = torch.tensor(0.0, dtype=torch.float32)
            state['exp_avg'] = torch.zeros_like(p.data, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p.data, memory_format=torch.preserve_format)
        if group['amsgrad'] and 'max_exp_avg_sq' not in state:
            state['max_exp_avg_sq'] = torch.zeros_like(p.data, memory_format=torch.preserve_format)
        return state

    _STATE = (('m', 'exp_avg'), ('v', 'exp_avg_sq'), ('x', 'max_exp_avg_sq'))

    def _ensure_layout(self, held, rows, any_ams):
        """The flat buffers for these rows: kept while nothing moved, else (re-)adopted with every value copied in."""
        lay = self._lay
        key = (tuple(id(p) for p in held), tuple(map(tuple, rows)), bool(any_ams))
        ok = lay is not None and lay['key'] == key
        if ok:
            for p, row in zip(held, rows):
                st = self.state[p]
                if p.data_ptr() != lay['p'].data_ptr() + 4 * row[0]:
                    ok = False      # model.cuda() / load_state_dict replaced a tensor: adopt again (copies them in)
                    break
                for short, name in self._STATE:
                    t = st.get(name)
                    if t is not None and t.data_ptr() != lay[short].data_ptr() + 4 * row[2]:
                        ok = False      # optimizer.load_state_dict() swapped the state tensors
                        break
                if not ok:
                    break
        if ok:
            return lay
        dev = held[0].device
        numel = max(r[0] + (r[3] + 3) // 4 * 4 for r in rows)
        bufs = dict(p=torch.zeros(numel, dtype=torch.float32, device=dev), m=torch.zeros(numel, dtype=torch.float32, device=dev),
                    v=torch.zeros(numel, dtype=torch.float32, device=dev),
                    x=torch.zeros(numel, dtype=torch.float32, device=dev) if any_ams else None)
        for p, row in zip(held, rows):
            pv = torch.as_strided(bufs['p'], p.shape, p.stride(), row[0])
            pv.copy_(p.data)
            p.data = pv
            st = self.state[p]
            for short, name in self._STATE:
                old = st.get(name)
                if old is None or bufs[short] is None:
                    continue
                sv = torch.as_strided(bufs[short], p.shape, p.stride(), row[2])
                sv.copy_(old)
                st[name] = sv
        host = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        lay = self._lay = dict(key=key, numel=numel, host=host, dev=torch.from_numpy(host).to(dev), held=held, **bufs)
        return lay

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        held, groups = [], []
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("singleshotpose_amd.optim.%s runs on the MI355X HIP kernel only: parameter on %s"
                                       % (self._name, p.device))
                if p.grad.is_sparse:
                    raise RuntimeError("%s does not support sparse gradients" % self._name)
                self._init_state(p, group)
                held.append(p)
                groups.append(group)
        if not held:
            return loss
        steps = [self.state[p]['step'] for p in held]
        torch._foreach_add_(steps, 1)      # (CPU tensors: no device synchronisation; one dispatch for all of them)
        gkey = {id(group): self._key(group, 0.0)[:7] for group in self.param_groups}
        keys = [gkey[id(group)] + (s.item(),) for group, s in zip(groups, steps)]
        st = torch.cuda.current_stream(held[0].device).cuda_stream
        any_ams = any(k[6] for k in keys)
        flat = SGD._flat_grads(held) if all(_dense(p.data) for p in held) else None
        if flat is not None:
            base, items, total = flat
            g0 = held[0].grad
            gbase = g0.data_ptr() - 4 * g0.storage_offset()
            whole = (len(set(keys)) == 1 and len(held) == sum(len(g['params']) for g in self.param_groups) and
                     sum((p.numel() + 3) // 4 * 4 for p in held) == total)
            if whole:
                # one range: parameters and state sit at the offsets of the gradient views
                rows = [[off, off, off, p.numel(), 0] for p, off in items]
                lay = self._ensure_layout(held, rows, any_ams)
                h = _hyper9(keys[0])
                _lib.call('ssp_adam_step', lay['p'].data_ptr(), gbase, lay['m'].data_ptr(), lay['v'].data_ptr(),
                          lay['x'].data_ptr() if any_ams else None, total, *(h[:7] + (int(h[7]), int(h[8]), st)))
                self.fused_steps += 1
                weights_changed()      # raw-pointer writes do not bump tensor versions: invalidate packed-filter caches
                return loss
            built = build_adam_segment_table([(p.numel(), off, k) for (p, off), k in zip(items, keys)])
            if built is not None:
                rows, tkeys, numel = built
                lay = self._ensure_layout(held, rows, any_ams)
                hyper = (ctypes.c_double * (9 * len(tkeys)))(*[v for k in tkeys for v in _hyper9(k)])
                _lib.call('ssp_adam_step_table', lay['p'].data_ptr(), gbase, lay['m'].data_ptr(), lay['v'].data_ptr(),
                          lay['x'].data_ptr() if any_ams else None, numel, total, numel, lay['dev'].data_ptr(),
                          lay['host'].ctypes.data, len(rows), ctypes.cast(hyper, ctypes.c_void_p), len(tkeys), st)
                self.table_steps += 1
                weights_changed()
                return loss
        # per-parameter launches of the same kernel: gradients that are no flat views, or more than 16 distinct tuples
        for p, k in zip(held, keys):
            g = p.grad
            if not _dense(p.data):
                raise RuntimeError("%s: parameter is neither contiguous nor channels-last" % self._name)
            if g.dtype != torch.float32 or not _same_layout(g, p):
                g = torch.empty_like(p.data).copy_(g)      # same memory order as the parameter
            state = self.state[p]
            ptrs = [p.data_ptr(), g.data_ptr(), state['exp_avg'].data_ptr(), state['exp_avg_sq'].data_ptr(),
                    state['max_exp_avg_sq'].data_ptr() if k[6] else None]
            if any(q is not None and q & 15 for q in ptrs):
                raise RuntimeError("%s: parameter / gradient / state storage is not 16-byte aligned" % self._name)
            for name in ('exp_avg', 'exp_avg_sq') + (('max_exp_avg_sq',) if k[6] else ()):
                if not (state[name].is_cuda and state[name].dtype == torch.float32 and _same_layout(state[name], p)):
                    raise RuntimeError("%s: state %s does not have the parameter's device, dtype and layout" % (self._name, name))
            h = _hyper9(k)
            _lib.call('ssp_adam_step', *(ptrs + [p.numel()] + list(h[:7]) + [int(h[7]), int(h[8]), st]))
        weights_changed()
        return loss


class AdamW(Adam):
    _decoupled = True
    _name = 'AdamW'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None):
        super(AdamW, self).__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize,
                                    capturable=capturable, differentiable=differentiable, fused=fused)


# ---- global-norm gradient clipping -------------------------------------------------------------------------------------
_CLIP_GRID = 2048            # partials one table launch writes at most (include/ssp_hip.h)
_CLIP_MAX_PARTIALS = 65536   # partials one ssp_grad_scale_table launch adds
_clip_tables = {}            # (device, segments) -> (host rows, device rows): rebuilt only when the layout changes


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for the 2-norm as two HIP launches (ssp_grad_sumsq_table, ssp_grad_scale_table)
    with no host synchronisation: returns the total norm as a 0-dim device tensor.  Gradients that are views of one flat
    buffer (what Plan.backward leaves) take one launch pair over a segment table; others one pair per tensor into one
    partial array.  Works in front of optim.SGD and optim.Adam alike (the views stay views); in multi-GPU runs call it
    after the reducer's all-reduce."""
    if float(norm_type) != 2.0:
        raise ValueError("clip_grad_norm_: norm_type=%r is not supported: only the 2-norm runs on the HIP kernels" % (norm_type,))
    if foreach:
        raise ValueError("clip_grad_norm_: foreach=%r is not supported" % (foreach,))
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    max_norm = float(max_norm)
    if not params:
        return torch.tensor(0.0)
    for p in params:
        g = p.grad
        if not g.is_cuda:
            raise RuntimeError("singleshotpose_amd.optim.clip_grad_norm_ runs on the MI355X HIP kernels only: gradient on %s" % g.device)
        if g.dtype != torch.float32:
            raise RuntimeError("clip_grad_norm_: gradient dtype %s (float32 only)" % g.dtype)
    dev = params[0].grad.device
    st = torch.cuda.current_stream(dev).cuda_stream
    result = torch.empty(2, dtype=torch.float32, device=dev)
    count = ctypes.c_int(0)
    flat = SGD._flat_grads(params) if all(_dense(p.data) for p in params) else None
    if flat is not None:
        base, items, total = flat
        segs = tuple((off, p.numel()) for p, off in items)
        tab = _clip_tables.get((dev, segs))
        if tab is None:
            if len(_clip_tables) > 8:
                _clip_tables.clear()
            host = np.ascontiguousarray(np.asarray([[0, off, 0, n, 0] for off, n in segs], dtype=np.int64))
            tab = _clip_tables[(dev, segs)] = (host, torch.from_numpy(host).to(dev))
        host, table = tab
        g0 = params[0].grad
        gbase = g0.data_ptr() - 4 * g0.storage_offset()
        partial = torch.empty(_CLIP_GRID, dtype=torch.float64, device=dev)
        _lib.call('ssp_grad_sumsq_table', gbase, total, table.data_ptr(), host.ctypes.data, len(segs), partial.data_ptr(),
                  _CLIP_GRID, ctypes.cast(ctypes.byref(count), ctypes.c_void_p), st)
        _lib.call('ssp_grad_scale_table', gbase, total, table.data_ptr(), host.ctypes.data, len(segs), partial.data_ptr(),
                  count.value, max_norm, result.data_ptr(), st)
    else:
        if len(params) > _CLIP_MAX_PARTIALS:
            raise RuntimeError("clip_grad_norm_: more than %d separate gradient tensors" % _CLIP_MAX_PARTIALS)
        for p in params:
            g = p.grad
            if not _dense(g) or g.data_ptr() & 15:
                raise RuntimeError("clip_grad_norm_: a gradient is not dense in memory or not 16-byte aligned")
        room = max(1, min(_CLIP_GRID, _CLIP_MAX_PARTIALS // len(params)))
        partial = torch.empty(room * len(params), dtype=torch.float64, device=dev)
        used = 0
        for p in params:
            _lib.call('ssp_grad_sumsq_table', p.grad.data_ptr(), p.grad.numel(), None, None, 1, partial.data_ptr() + 8 * used,
                      room, ctypes.cast(ctypes.byref(count), ctypes.c_void_p), st)
            used += count.value
        for p in params:
            _lib.call('ssp_grad_scale_table', p.grad.data_ptr(), p.grad.numel(), None, None, 1, partial.data_ptr(), used,
                      max_norm, result.data_ptr(), st)
    total_norm = result[0]
    if error_if_nonfinite and not bool(torch.isfinite(total_norm)):
        raise RuntimeError("The total norm of order %s for gradients from `parameters` is non-finite, so it cannot be "
                           "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`" % float(norm_type))
    return total_norm

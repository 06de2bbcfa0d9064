"""Shared definitions of the Adam / AdamW / gradient-clipping tests (test_adam_cpu.py, test_gpu_adam.py,
test_gpu_clip_grad.py): the float64 statement of the update and of the clipping, written from the comment in
include/ssp_hip.h (ssp_adam_step, ssp_grad_sumsq_table, ssp_grad_scale_table), the kernel case table and the seeds.
Nothing here imports the code under test."""
import collections

import numpy as np

SEED = 20261021
CHUNK = 4096          # floats per chunk of the table walk
GRID = 2048           # workgroups at most: a segment of more than GRID chunks makes the walk wrap
# every length at which the kernels take another path: below a quad, one quad, quad + tail, around one chunk, two chunks
# plus a quad, and more chunks than workgroups (with a scalar tail)
LENGTHS = [1, 3, 4, 5, 4095, 4096, 4097, 4099, 2 * 4096 + 4, 2049 * 4096 + 3]
POISON = 0x7fc0dead   # a quiet-NaN bit pattern for the floats between segments

Hyper = collections.namedtuple('Hyper', 'name decoupled amsgrad lr beta1 beta2 eps weight_decay')
# Adam and AdamW, amsgrad on and off, eps 1e-8 and 1e-3, beta2 0.99 and 0.999, weight decay 0 and not 0: every value of
# every axis with every value of every other axis at least once
HYPERS = [
    Hyper('adam', False, False, 1e-3, 0.9, 0.999, 1e-8, 0.0),
    Hyper('adam-wd-b99', False, False, 1e-3, 0.9, 0.99, 1e-8, 0.01),
    Hyper('adam-ams-eps3', False, True, 1e-3, 0.9, 0.999, 1e-3, 0.0),
    Hyper('adam-ams-wd-b99-eps3', False, True, 2e-3, 0.8, 0.99, 1e-3, 0.05),
    Hyper('adamw', True, False, 1e-3, 0.9, 0.999, 1e-8, 0.01),
    Hyper('adamw-wd0-b99-eps3', True, False, 1e-3, 0.9, 0.99, 1e-3, 0.0),
    Hyper('adamw-ams', True, True, 1e-3, 0.9, 0.999, 1e-8, 0.01),
    Hyper('adamw-ams-wd0-b99', True, True, 2e-3, 0.8, 0.99, 1e-8, 0.0),
    Hyper('adamw-ams-b99-eps3', True, True, 1e-3, 0.9, 0.99, 1e-3, 0.1),
    Hyper('adam-ams-wd-eps8', False, True, 1e-3, 0.9, 0.999, 1e-8, 0.01),
    Hyper('adamw-b999-eps3-wd', True, False, 1e-3, 0.9, 0.999, 1e-3, 0.01),
    Hyper('adam-b99-eps3-wd0', False, False, 1e-3, 0.9, 0.99, 1e-3, 0.0),
]
# (length, hyper) pairs of the kernel tests: every length with a plain and with the fullest case, every hyper case at the
# lengths with a tail
KERNEL_CASES = ([(n, HYPERS[0]) for n in LENGTHS] + [(n, HYPERS[8]) for n in LENGTHS] +
                [(n, h) for h in HYPERS[1:8] + HYPERS[9:] for n in (5, 4099)])
GRAD_SCALES = [1.0, 1e-2, 1e-4, 0.3, 1e-3, 1.0, 1e-1, 1e-4]      # per step: gradient magnitudes from 1e-4 to 1


def bias_corrections(h, step):
    """(step_size, bc2_sqrt) the host hands the kernel, in Python doubles (torch/optim/adam.py's single-tensor path)."""
    return h.lr / (1 - h.beta1 ** step), (1 - h.beta2 ** step) ** 0.5


def adam_statement(p, g, m, v, vmax, h, step, lr=None):
    """One step in float64, operation for operation as include/ssp_hip.h states it.  Returns (p, m, v, vmax)."""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    lr = h.lr if lr is None else lr
    step_size, bc2_sqrt = bias_corrections(h._replace(lr=lr), step)
    if h.weight_decay != 0:
        if h.decoupled:
            p = p * (1 - lr * h.weight_decay)
        else:
            g = g + h.weight_decay * p
    m = m + (1 - h.beta1) * (g - m)
    v = h.beta2 * v + ((1 - h.beta2) * g) * g
    if h.amsgrad:
        vmax = np.maximum(np.asarray(vmax, dtype=np.float64), v)
        d = vmax
    else:
        d = v
    denom = np.sqrt(d) / bc2_sqrt + h.eps
    p = p + (-step_size * m) / denom
    return p, m, v, vmax


def clip_statement(segments, max_norm):
    """Global-norm clipping in float64 over a list of gradient arrays: (norm, coef, [scaled arrays])."""
    segments = [np.asarray(s, dtype=np.float64) for s in segments]
    norm = float(np.sqrt(sum(float((s * s).sum()) for s in segments)))
    coef = min(1.0, max_norm / (norm + 1e-6))
    return norm, coef, [s * coef for s in segments]


def inputs(n, seed, steps):
    """fp32 start values and per-step gradients of one kernel case."""
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    grads = [(rs.standard_normal(n) * GRAD_SCALES[s % len(GRAD_SCALES)]).astype(np.float32) for s in range(steps)]
    return p, grads


def segment_layout(long_len, nshort=300, seed=SEED):
    """About 300 segments of lengths 1 ... 40 and one long one, with gaps, at DIFFERENT offsets in the parameter, gradient
    and state buffers.  Returns (rows [[param offset, grad offset, state offset, length]], param floats, grad floats,
    state floats)."""
    rs = np.random.RandomState(seed)
    lens = [int(v) for v in rs.randint(1, 41, nshort)]
    lens.insert(nshort // 2, int(long_len))
    rows = []
    po, go, so = 4, 8, 0
    for n in lens:
        rows.append([po, go, so, n])
        r4 = (n + 3) // 4 * 4
        po += r4 + 4 * int(rs.randint(0, 3))
        go += r4 + 4 * int(rs.randint(0, 3))
        so += r4 + 4 * int(rs.randint(0, 2))
    return rows, po + 4, go + 8, so + 4


def poisoned(nfloats):
    return np.full(nfloats, POISON, dtype=np.uint32).view(np.float32)

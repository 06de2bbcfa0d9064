#!/usr/bin/env python
"""What an optimizer step and a gradient clip cost on cfg/yolo-pose.cfg's parameter set.

One backward of the network (small batch: only the LAYOUT of the gradients matters here) leaves every gradient as a view
of one flat fp32 buffer.  Every variant below gets its own copy of the parameters and of that buffer, with the gradient
views at the same offsets and strides, so that all of them can be timed in ONE process, interleaved round by round:

  sgd                singleshotpose_amd.optim.SGD (momentum 0.9, weight decay)            20 B per parameter
  adam / adamw       singleshotpose_amd.optim.Adam / AdamW                                28 B per parameter
  adam_ams / adamw_ams  the same with amsgrad                                             36 B per parameter
  clip / clip_noop   singleshotpose_amd.optim.clip_grad_norm_, scaling (every call clips to 0.99 of the one before) /
                     max_norm = inf                                                       12 B / 4 B per parameter
  torch_adam         torch.optim.Adam (its default foreach path) on the same tensors
  torch_clip         torch.nn.utils.clip_grad_norm_ on the same tensors
  *_head             the same for an optimizer that holds the head conv alone (a segment table over the flat buffer)

Prints ONE JSON line: per variant the median and the minimum over the rounds of the mean time per call (device events
around `iters` calls), the achieved GB/s on the bytes the algorithm needs, the project's launches per call and the
fused_steps / table_steps counters.
  tools/optim_bench.py [--rounds 7] [--iters 20] [--warmup 3] [--variants a,b,...]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = {'sgd': 20, 'adam': 28, 'adamw': 28, 'adam_ams': 36, 'adamw_ams': 36, 'clip': 12, 'clip_noop': 4, 'torch_adam': 28,
         'torch_clip': 12}
VARIANTS = list(BYTES) + ['sgd_head', 'adam_head', 'clip_head', 'torch_adam_head', 'torch_clip_head']


def gradient_layout(cfg, device):
    """[(name, parameter, gradient view)] and the flat gradient buffer after one backward."""
    from bench import synthetic_batch
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.region_loss import RegionLoss
    torch.manual_seed(0)
    model = Darknet(cfg).to(device).train()
    crit = RegionLoss()
    crit.verbose = False
    x, tgt = synthetic_batch(2, 416, 416, 1000, device)
    crit(model(x), tgt, 20).backward()
    torch.cuda.synchronize()
    named = list(model.named_parameters())
    base = named[0][1].grad.untyped_storage()
    assert all(p.grad.untyped_storage().data_ptr() == base.data_ptr() for _, p in named), "gradients are not views of one buffer"
    total = base.nbytes() // 4
    flat = torch.empty(0, dtype=torch.float32, device=device).set_(base, 0, (total,), (1,))
    head = named[-1][0].rsplit('.', 1)[0].rsplit('.', 1)[0]
    return model, named, flat, head


def copies(named, flat, keep=None):
    """Own parameters and an own flat gradient buffer with the views at the model's offsets and strides."""
    mine = flat.clone()
    params = []
    for name, p in named:
        if keep is not None and not name.startswith(keep):
            continue
        q = torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format))
        q.grad = torch.as_strided(mine, p.grad.shape, p.grad.stride(), p.grad.storage_offset())
        params.append(q)
    return params, mine


def make(variant, named, flat, head):
    from singleshotpose_amd import optim
    keep = (head + '.') if variant.endswith('_head') else None
    kind = variant[:-5] if keep else variant
    params, mine = copies(named, flat, keep)
    opt = None
    bound = [1.0]

    def shrinking():
        # a clip to M leaves the norm at M, and a second clip to M would find nothing to scale: every call clips to 0.99 of
        # the call before, so that each one scales (coef about 0.99) without reading the norm back
        bound[0] *= 0.99
        return bound[0]
    if kind == 'sgd':
        opt = optim.SGD(params, lr=1e-3 / 64, momentum=0.9, dampening=0, weight_decay=0.0005 * 64)
    elif kind in ('adam', 'adam_ams'):
        opt = optim.Adam(params, lr=1e-4, weight_decay=0.0005, amsgrad=kind.endswith('_ams'))
    elif kind in ('adamw', 'adamw_ams'):
        opt = optim.AdamW(params, lr=1e-4, amsgrad=kind.endswith('_ams'))
    elif kind == 'torch_adam':
        opt = torch.optim.Adam(params, lr=1e-4, weight_decay=0.0005)
    if opt is not None:
        call = opt.step
    elif kind == 'clip':
        call = lambda: optim.clip_grad_norm_(params, shrinking())
    elif kind == 'clip_noop':
        call = lambda: optim.clip_grad_norm_(params, float('inf'))
    elif kind == 'torch_clip':
        call = lambda: torch.nn.utils.clip_grad_norm_(params, shrinking())
    else:
        raise SystemExit("unknown variant %s (of %s)" % (variant, ', '.join(VARIANTS)))
    return dict(name=variant, kind=kind, call=call, opt=opt, params=params, grads=mine,
                floats=sum(p.numel() for p in params), times=[])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--variants', default=','.join(VARIANTS))
    ap.add_argument('--cfg', default=os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_bench.py measures on the GPU; there is none")
    from singleshotpose_amd import _lib
    device = torch.device('cuda', 0)
    model, named, flat, head = gradient_layout(args.cfg, device)
    runs = [make(v, named, flat, head) for v in args.variants.split(',')]
    log = []
    orig = _lib.call
    for r in runs:
        for _ in range(args.warmup):
            r['call']()
        _lib.call = lambda name, *a: (log.append(name), orig(name, *a))[1]
        try:
            del log[:]
            r['call']()
        finally:
            _lib.call = orig
        r['launches'] = {k: log.count(k) for k in sorted(set(log))}
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for r in runs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.iters):
                r['call']()
            b.record()
            torch.cuda.synchronize()
            r['times'].append(a.elapsed_time(b) / args.iters)
    lines = []
    for r in runs:
        med, best = statistics.median(r['times']), min(r['times'])
        nbytes = BYTES[r['kind']] * r['floats']
        line = {'variant': r['name'], 'floats': r['floats'], 'ms': round(med, 4), 'ms_min': round(best, 4),
                'bytes_per_float': BYTES[r['kind']], 'GBps': round(nbytes / (med * 1e-3) / 1e9, 1),
                'launches_per_call': r['launches']}
        if r['opt'] is not None and hasattr(r['opt'], 'fused_steps'):
            calls = args.warmup + 1 + args.rounds * args.iters
            line.update(calls=calls, fused_steps=r['opt'].fused_steps, table_steps=r['opt'].table_steps)
        lines.append(line)
    print(json.dumps({'tool': 'optim_bench', 'cfg': os.path.basename(args.cfg), 'rounds': args.rounds, 'iters': args.iters,
                      'flat_gradient_floats': flat.numel(), 'head': head, 'device': torch.cuda.get_device_name(0),
                      'lines': lines}))


if __name__ == '__main__':
    main()

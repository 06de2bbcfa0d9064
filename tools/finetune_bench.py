#!/usr/bin/env python
"""What a fine-tuning step costs ("Training part of a network"): yolo-pose.cfg at the headline shape
(batch 64, 416 x 416), forward + RegionLoss + backward + singleshotpose_amd.optim.SGD step, for

  all            every parameter trainable, every BatchNorm in training mode (bench.py's step)
  head           only the head conv trainable, every BatchNorm of the trunk in eval()
  last3          the last three conv blocks trainable, the BatchNorm of the blocks before them in eval()
  groups         everything trainable under the parameter-group list of train.py:381-387 (no weight decay on BatchNorm
                 and bias parameters): 66 groups, two hyper-parameter tuples

One JSON line per scenario: ms per step, the launches of one backward pass and of one optimizer step.
  tools/finetune_bench.py [--batch 64] [--size 416] [--steps 10] [--warmup 3] [scenario ...]"""
import argparse
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENARIOS = ('all', 'head', 'last3', 'groups')


def build(name, cfg, device):
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.optim import SGD
    torch.manual_seed(0)
    model = Darknet(cfg).to(device).train()
    convs = [i for i, b in enumerate(model.blocks[1:]) if b['type'] == 'convolutional']
    first = {'all': convs[0], 'groups': convs[0], 'head': convs[-1], 'last3': convs[-3]}[name]
    for i in convs:
        if i < first:
            for p in model.models[i].parameters():
                p.requires_grad_(False)
            for m in model.models[i]:
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.eval()
    kw = dict(lr=1e-3 / 64, momentum=0.9, dampening=0, weight_decay=0.0005 * 64)
    if name == 'groups':
        params = []
        for key, value in model.named_parameters():
            bn_or_bias = key.find('.bn') >= 0 or key.find('.bias') >= 0
            params.append({'params': [value], 'weight_decay': 0.0 if bn_or_bias else kw['weight_decay']})
    else:
        params = [p for p in model.parameters() if p.requires_grad]
    return model, SGD(params, **kw)


def run(name, args, device):
    from bench import synthetic_batch
    from singleshotpose_amd import _lib
    from singleshotpose_amd.region_loss import RegionLoss
    model, opt = build(name, args.cfg, device)
    crit = RegionLoss()
    crit.verbose = False
    x, tgt = synthetic_batch(args.batch, args.size, args.size, 1000, device)
    phase = [None]
    counts = {'backward': {}, 'optimizer': {}}
    orig = _lib.call

    def rec(fn, *a):
        if phase[0] in counts:
            counts[phase[0]][fn] = counts[phase[0]].get(fn, 0) + 1
        return orig(fn, *a)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = crit(model(x), tgt, 20)
        if phase[0] == 'armed':
            phase[0] = 'backward'
        loss.backward()
        if phase[0] == 'backward':
            phase[0] = 'optimizer'
        opt.step()
        phase[0] = None

    for _ in range(args.warmup):
        step()
    _lib.call = rec
    try:
        phase[0] = 'armed'
        step()
    finally:
        _lib.call = orig
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    bw = counts['backward']
    return {'scenario': name, 'batch': args.batch, 'size': args.size, 'steps': args.steps, 'ms_per_step': round(ms, 3),
            'trainable_tensors': sum(1 for p in model.parameters() if p.requires_grad),
            'backward_launches': sum(bw.values()),
            'backward_filter_gradients': sum(v for k, v in bw.items() if k.startswith('ssp_conv_wgrad') or k == 'ssp_first_bwd_wgrad'),
            'backward_data_gradients': sum(v for k, v in bw.items() if k.startswith('ssp_conv_dgrad')),
            'optimizer_launches': sum(counts['optimizer'].values()), 'optimizer': counts['optimizer'],
            'optimizer_flat_floats': opt.flat_numel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('scenarios', nargs='*', default=list(SCENARIOS))
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cfg', default=os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    args = ap.parse_args()
    device = torch.device('cuda', 0)
    for name in args.scenarios:
        if name not in SCENARIOS:
            raise SystemExit("unknown scenario %s (one of %s)" % (name, ', '.join(SCENARIOS)))
        print(json.dumps(run(name, args, device)), flush=True)
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

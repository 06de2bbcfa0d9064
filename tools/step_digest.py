#!/usr/bin/env python
"""One seeded training step (or N) of a cfg on cuda:0, reduced to sha256 digests: the forward output, the loss, every
parameter gradient, the input gradient, the BatchNorm running statistics and the parameters after optim.SGD.step().

  python tools/step_digest.py cfg/yolo-pose.cfg --batch 4 --size 160 --steps 2 --deterministic 1 [--compare digests.json]

Parameters, input and labels come from --seed alone, so two processes digest the same step.  With --deterministic 1 (or
SSP_DETERMINISTIC=1) and the same plan codes (SSP_AUTOTUNE=0, a shared SSP_TUNE_CACHE, or dist.sync_plans) every digest is
the same from run to run and from process to process; with the mode off the gradients' last bits move.  --write FILE saves
the digests as JSON, --compare FILE exits 1 when any differs from that file (and prints which).
--wgrad-wino T puts the filter gradient of every layer the ordered Winograd form of tile T fits on it (test aid);
--freeze N freezes the first N conv blocks (BatchNorm in eval mode); --no-input-grad skips dL/dx."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seed_model(model, seed):
    """Parameters from a CPU generator: filters ~ N(0, 1/fan_in), BatchNorm weights in [0.5, 1.5], small biases."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
                fan = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def reset_state(model, seed):
    """Back to the seeded state: parameters re-drawn from the seed, running statistics to their initial values."""
    seed_model(model, seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.zero_()
                m.running_var.fill_(1.0)
                m.num_batches_tracked.zero_()


def make_batch(seed, B, C, H, W):
    """Input in [0, 1) and one ground-truth object per image in the single-object label layout (50 x 21 per image)."""
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.uniform(0, 1, (B, C, H, W)).astype(np.float32))
    t = np.zeros((B, 50, 21))
    for b in range(B):
        c = rs.uniform(0.2, 0.8, 2)
        t[b, 0, 1:3] = c
        t[b, 0, 3:19] = (c[None, :] + rs.uniform(-0.12, 0.12, (8, 2))).reshape(-1)
        t[b, 0, 19:21] = rs.uniform(0.1, 0.4, 2)
    return x, torch.from_numpy(t.reshape(B, -1))


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def force_wgrad_wino(plan, tile):
    """Every layer whose ordered Winograd filter gradient of that tile the library takes runs it (set on the plan)."""
    from singleshotpose_amd import _lib
    n = 0
    for cs in plan.convs.values():
        ok = (cs.k == 3 and cs.stride == 1 and not cs.first and cs.cinp == cs.cin and cs.coutp == cs.cout and
              _lib.query('ssp_conv_wgrad_wino_ordered_split', plan.B, cs.H, cs.W, cs.cinp, cs.cout, tile, 0) > 0)
        plan.set_code(cs, 'wgrad', tile if ok else 0)
        n += ok
    plan._settle(dgrad=True)
    return n


def run(cfg, B, H, W, steps=1, seed=0, deterministic=None, wgrad_wino=0, freeze=0, input_grad=True, state=None):
    """{name: sha256} of `steps` training steps, and the tensors of the last one (for callers that compare values).
    state: a model to run on (as it is: see reset_state) instead of a freshly seeded one; the optimizer is always new."""
    from singleshotpose_amd import optim
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.region_loss import RegionLoss
    if state is None:
        model = Darknet(cfg)
        seed_model(model, seed)
        if deterministic is not None:
            model.deterministic = bool(deterministic)
        model = model.cuda().train()
        convs = [m for m in model.models if isinstance(m, torch.nn.Sequential) and isinstance(m[0], torch.nn.Conv2d)]
        for m in convs[:freeze]:
            for p in m.parameters():
                p.requires_grad_(False)
            for sub in m:
                if isinstance(sub, torch.nn.BatchNorm2d):
                    sub.eval()
    else:
        model = state
    # (a fully frozen model has nothing to update: the input-only backward)
    train = [p for p in model.parameters() if p.requires_grad]
    opt = optim.SGD(train, lr=1e-3, momentum=0.9, weight_decay=5e-4) if train else None
    C = int(model.blocks[0].get('channels', 3))
    crit = RegionLoss()
    out, tensors = {}, {}
    for step in range(steps):
        x, tgt = make_batch(seed + 1000 * step, B, C, H, W)
        x = x.cuda().requires_grad_(input_grad)
        model.zero_grad(set_to_none=True)
        if wgrad_wino and step == 0 and state is None:
            # before the first forward: the plan's own backward preparation (tuning included) runs once, then the choice is set
            plan = model._plan((B, H, W), x.device)
            plan._prepare_backward()
            assert force_wgrad_wino(plan, wgrad_wino) > 0, "no layer takes the ordered Winograd filter gradient"
        y = model(x)
        loss = crit(y, tgt, 20)
        loss.backward()
        tensors = {'output': y.detach(), 'loss': loss.detach()}
        if input_grad:
            tensors['x.grad'] = x.grad
        for n, p in model.named_parameters():
            if p.grad is not None:
                tensors['grad:' + n] = p.grad.detach().clone()
        if opt is not None:
            opt.step()
        for n, b in model.named_buffers():
            if 'running' in n:
                tensors['stat:' + n] = b.detach().clone()
        for n, p in model.named_parameters():
            tensors['param:' + n] = p.detach().clone()
        torch.cuda.synchronize()
        for n, t in tensors.items():
            out['step%d/%s' % (step, n)] = digest(t)
    return out, tensors, model


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('cfg')
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--size', type=int, default=160, help='input height and width')
    ap.add_argument('--height', type=int, default=0)
    ap.add_argument('--width', type=int, default=0)
    ap.add_argument('--steps', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--deterministic', type=int, choices=(0, 1), default=None, help='default: SSP_DETERMINISTIC')
    ap.add_argument('--wgrad-wino', type=int, choices=(0, 2, 4), default=0)
    ap.add_argument('--freeze', type=int, default=0)
    ap.add_argument('--no-input-grad', action='store_true')
    ap.add_argument('--write')
    ap.add_argument('--compare')
    a = ap.parse_args()
    H, W = a.height or a.size, a.width or a.size
    out, _, model = run(a.cfg, a.batch, H, W, a.steps, a.seed, a.deterministic, a.wgrad_wino, a.freeze, not a.no_input_grad)
    plan = list(model._plans.values())[-1]
    print('deterministic: %s' % ('on' if plan.deterministic['mode'] else 'off'))
    for n in sorted(out):
        print('%s  %s' % (out[n], n))
    if a.write:
        with open(a.write, 'w') as f:
            json.dump(out, f, indent=0, sort_keys=True)
    if a.compare:
        with open(a.compare) as f:
            want = json.load(f)
        bad = sorted(n for n in set(out) | set(want) if out.get(n) != want.get(n))
        for n in bad:
            print('DIFFERS  %s' % n)
        return 1 if bad else 0
    return 0


if __name__ == '__main__':
    sys.exit(main())

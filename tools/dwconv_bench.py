"""The depthwise 3x3 kernels (csrc/conv_depthwise.hip) alone, and cfg/yolo-pose-dw.cfg in a training step.

1. ssp_dwconv_fwd (with BatchNorm statistics, as training runs it), ssp_dwconv_dgrad and ssp_dwconv_wgrad at every distinct
   depthwise shape cfg/yolo-pose-dw.cfg runs at batch 64, 416 x 416 (stride 1), and at one stride-2 shape: microseconds per
   launch and effective bandwidth = algorithmic bytes / time against the 8 TB/s HBM peak.  Algorithmic bytes: the forward
   reads x once and writes y once, the data gradient reads dy once and writes dx once, the filter gradient reads x and dy
   once.  Next to each shape, ssp_copy_channels on the same bytes (read one map, write the other) in the same session.
   Each case cycles through enough independent buffer sets (>= 1 GiB together) that its operands cannot stay in the 256 MB
   Infinity Cache between launches; time = HIP events around `--iters` back-to-back launches after a warm-up (launch gaps
   included; the filter gradient is its two launches).
2. One training step (forward, RegionLoss, backward, SGD) of cfg/yolo-pose-dw.cfg next to cfg/yolo-pose.cfg, two models in
   one process, `--rounds` alternating rounds of `--steps` steps each; the median round of each is reported.
3. --multiscale: cfg/yolo-pose-dw.cfg at batch 2 over the 20 multi-scale shapes (224 .. 832): one training step each -
   loss, whether every parameter gradient is finite, the length of the decoded box.

Prints one JSON line per measurement.

    python tools/dwconv_bench.py [--iters 200] [--batch 64] [--size 416] [--steps 10] [--rounds 3] [--no-step] [--no-kernels]
                                 [--multiscale]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from singleshotpose_amd import _lib  # noqa: E402

HBM_TBPS = 8.0
F32 = 4


def nsets(bytes_per_set):
    return max(1, -(-(1 << 30) // bytes_per_set))


def run(name, launches, nbytes, iters):
    for fn in launches:           # warm-up: every buffer set once
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        launches[i % len(launches)]()
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    gbps = nbytes / (us * 1e-6) / 1e9
    print(json.dumps(dict(kernel=name, bytes=nbytes, us_per_launch=round(us, 2), GBps=round(gbps, 1),
                          frac_of_hbm_peak=round(gbps / 1e3 / HBM_TBPS, 3), buffer_sets=len(launches))), flush=True)


def shapes_of_cfg(batch, size):
    """(H, W, C, stride) of every distinct depthwise block of cfg/yolo-pose-dw.cfg at this input size, largest map first."""
    from singleshotpose_amd.cfg import layer_shapes, parse_cfg
    blocks = parse_cfg(os.path.join(ROOT, 'cfg', 'yolo-pose-dw.cfg'))
    shapes = layer_shapes(blocks, size, size)
    out = []
    for ind, b in enumerate(blocks[1:]):
        if b['type'] == 'convolutional' and int(b.get('groups', 1)) > 1:
            w, h, c = shapes[ind - 1]
            if (h, w, c, int(b['stride'])) not in out:
                out.append((h, w, c, int(b['stride'])))
    return out


def kernels(iters, B, size):
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    call, query = _lib.call, _lib.query
    buf = lambda n: torch.randn(n, dtype=torch.float32, device=dev)
    for H, W, C, s in shapes_of_cfg(B, size) + [(104, 104, 128, 2)]:
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        Mi, Mo = B * H * W, B * Ho * Wo
        moved = (Mi + Mo) * C * F32
        nstat = query('ssp_dwconv_stats_floats', B, H, W, C, s)
        nws = query('ssp_dwconv_wgrad_workspace_floats', B, H, W, C, s)
        # per set: the input-side map, the output-side map, the filter, its gradient, statistics, the filter gradient's partials
        sets = [(buf(Mi * C), buf(Mo * C), buf(C * 9), buf(C * 9), buf(nstat), buf(nws)) for _ in range(nsets(moved))]
        tag = 'B%d %dx%dx%d / %d' % (B, H, W, C, s)
        run('dwconv_fwd+stats ' + tag, [lambda t=t: call('ssp_dwconv_fwd', t[0].data_ptr(), t[2].data_ptr(), t[1].data_ptr(), None,
                                                         t[4].data_ptr(), B, H, W, C, C, C, s, st) for t in sets], moved, iters)
        run('dwconv_fwd ' + tag, [lambda t=t: call('ssp_dwconv_fwd', t[0].data_ptr(), t[2].data_ptr(), t[1].data_ptr(), None, None,
                                                   B, H, W, C, C, C, s, st) for t in sets], moved, iters)
        run('dwconv_dgrad ' + tag, [lambda t=t: call('ssp_dwconv_dgrad', t[1].data_ptr(), t[2].data_ptr(), t[0].data_ptr(), B, H, W, C,
                                                     C, C, s, 0, st) for t in sets], moved, iters)
        run('dwconv_wgrad ' + tag + ' (%d ranges)' % (nws // (9 * C)),
            [lambda t=t: call('ssp_dwconv_wgrad', t[1].data_ptr(), t[0].data_ptr(), t[3].data_ptr(), B, H, W, C, C, C, s, 0,
                              t[5].data_ptr(), nws, st) for t in sets], moved, iters)
        # the same bytes through the route's copy kernel: read the smaller map, write as many rows of the larger one's buffer
        # as move the same total (Mi + Mo) * C floats
        half = (Mi + Mo) // 2
        csets = [(buf(half * C), buf(half * C)) for _ in range(nsets(2 * half * C * F32))]
        run('copy_channels, the same bytes as ' + tag,
            [lambda t=t: call('ssp_copy_channels', t[0].data_ptr(), C, t[1].data_ptr(), C, C, half, 0, st) for t in csets],
            2 * half * C * F32, iters)
        del sets, csets


def _targets(rs, batch):
    tgt = np.zeros((batch, 50, 21))
    for b in range(batch):
        c = rs.uniform(0.2, 0.8, 2)
        tgt[b, 0, 1:3] = c
        tgt[b, 0, 3:19] = (c[None, :] + rs.uniform(-0.12, 0.12, (8, 2))).reshape(-1)
        tgt[b, 0, 19:21] = rs.uniform(0.1, 0.4, 2)
    return torch.from_numpy(tgt.reshape(batch, -1))


def steps(batch, size, nsteps, rounds):
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.optim import SGD
    from singleshotpose_amd.region_loss import RegionLoss
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, (batch, 3, size, size)).astype(np.float32)).cuda()
    tgt = _targets(rs, batch)
    nets = {}
    for cfg in ('yolo-pose-dw.cfg', 'yolo-pose.cfg'):
        torch.manual_seed(0)
        model = Darknet(os.path.join(ROOT, 'cfg', cfg)).cuda().train()
        opt = SGD(model.parameters(), lr=1e-4, momentum=0.9, dampening=0, weight_decay=5e-4)
        crit = RegionLoss()

        def step(model=model, opt=opt, crit=crit):
            opt.zero_grad()
            loss = crit(model(x), tgt, 20)
            loss.backward()
            opt.step()
            return loss
        for _ in range(3):        # plan, tuner, first-backward allocations
            step()
        torch.cuda.synchronize()
        nets[cfg] = (step, [], sum(p.numel() for p in model.parameters()), list(model._plans.values())[0].depthwise)
    for _ in range(rounds):
        for cfg, (step, ms, _, _) in nets.items():
            step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(nsteps):
                loss = step()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / nsteps)
            assert np.isfinite(float(loss.detach()))
    for cfg, (_, ms, nparam, dwl) in nets.items():
        print(json.dumps(dict(step='%s B%d %dx%d' % (cfg, batch, size, size), parameters=nparam, depthwise_blocks=len(dwl),
                              ms_per_step=round(float(np.median(ms)), 3), rounds=[round(m, 3) for m in ms],
                              images_per_s=round(batch / float(np.median(ms)) * 1e3, 1))), flush=True)


def multiscale(batch=2):
    """cfg/yolo-pose-dw.cfg over the 20 multi-scale shapes: one training step each."""
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.region_loss import RegionLoss
    from singleshotpose_amd.utils import get_region_boxes
    os.environ.setdefault('SSP_AUTOTUNE', '0')
    torch.manual_seed(0)
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose-dw.cfg')).cuda().train()
    crit = RegionLoss()
    rs = np.random.RandomState(0)
    for side in range(224, 833, 32):
        x = torch.from_numpy(rs.uniform(0, 1, (batch, 3, side, side)).astype(np.float32)).cuda()
        model.zero_grad(set_to_none=True)
        out = model(x)
        loss = crit(out, _targets(rs, batch), 20)
        loss.backward()
        torch.cuda.synchronize()
        finite = all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        box = get_region_boxes(out.detach(), 1, 9)
        print(json.dumps(dict(multiscale='yolo-pose-dw.cfg B%d %dx%d' % (batch, side, side), grid=list(out.shape[2:]),
                              loss=round(float(loss.detach()), 4), loss_finite=bool(np.isfinite(float(loss.detach()))),
                              grads_finite=finite,
                              box_len=len(box))), flush=True)
        model._plans.clear()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-step', action='store_true', help='the kernels only')
    ap.add_argument('--no-kernels', action='store_true', help='the training step only')
    ap.add_argument('--multiscale', action='store_true', help='also one batch-2 training step at each of the 20 multi-scale shapes')
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    _lib.load()
    if not args.no_kernels:
        kernels(args.iters, args.batch, args.size)
    if not args.no_step:
        steps(args.batch, args.size, args.steps, args.rounds)
    if args.multiscale:
        multiscale()


if __name__ == '__main__':
    main()

"""The [upsample] block alone and in a training step.

1. ssp_upsample_fwd / ssp_upsample_bwd at the shape cfg/yolo-pose-up.cfg runs them at batch 64, 416 x 416 (13 x 13 x 256 ->
   26 x 26), standalone (dense maps) and as the plan's write-through launches them (the fine side is columns [0, 256) of the
   route's 768-column buffer): microseconds per launch and effective bandwidth = algorithmic bytes (one read of the source
   side, one write of the destination side) / time, against the 8 TB/s HBM peak.  Each case cycles through enough
   independent buffer sets (>= 1 GiB together) that its operands cannot stay in the 256 MB Infinity Cache between
   launches; time = HIP events around `--iters` back-to-back launches after a warm-up (launch gaps included).
2. One training step (forward, RegionLoss, backward, SGD) of cfg/yolo-pose-up.cfg with the upsample written into the
   route's buffer and with SSP_UPSAMPLE_FUSE=0, two models in one process, `--rounds` alternating rounds of `--steps` steps
   each; the median round of each form is reported.

Prints one JSON line per measurement.

    python tools/upsample_bench.py [--iters 200] [--batch 64] [--size 416] [--steps 10] [--rounds 3] [--no-step]
                                   [--no-kernels] [--own-first]
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


def kernels(iters, B=64, H=13, W=13, C=256, N=2, ld_route=768):
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    call = _lib.call
    buf = lambda n: torch.randn(n, dtype=torch.float32, device=dev)
    Mc, Mf = B * H * W, B * H * W * N * N
    moved = (Mc + Mf) * C * F32
    for form, ldf in (('standalone', C), ('slice of %d' % ld_route, ld_route)):
        sets = [(buf(Mc * C), buf(Mf * ldf)) for _ in range(nsets((Mc * C + Mf * ldf) * F32))]
        tag = 'B%d %dx%dx%d x%d %s' % (B, H, W, C, N, form)
        run('upsample_fwd ' + tag, [lambda s=s: call('ssp_upsample_fwd', s[0].data_ptr(), C, s[1].data_ptr(), ldf, C, B, H, W, N, st)
                                    for s in sets], moved, iters)
        run('upsample_bwd ' + tag, [lambda s=s: call('ssp_upsample_bwd', s[1].data_ptr(), ldf, s[0].data_ptr(), C, C, B, H, W, N,
                                                     0, st) for s in sets], moved, iters)
        del sets
    # what the write-through saves per direction: the route's copy of the fine map into (out of) its buffer
    sets = [(buf(Mf * C), buf(Mf * ld_route)) for _ in range(nsets(Mf * (C + ld_route) * F32))]
    run('copy_channels B%d %dx%dx%d into %d (the copy the write-through removes)' % (B, H * N, W * N, C, ld_route),
        [lambda s=s: call('ssp_copy_channels', s[0].data_ptr(), C, s[1].data_ptr(), ld_route, C, Mf, 0, st) for s in sets],
        2 * Mf * C * F32, iters)


def steps(batch, size, nsteps, rounds, own_first=False):
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.optim import SGD
    from singleshotpose_amd.region_loss import RegionLoss
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, (batch, 3, size, size)).astype(np.float32)).cuda()
    tgt = np.zeros((batch, 50, 21))
    for b in range(batch):
        c = rs.uniform(0.2, 0.8, 2)
        tgt[b, 0, 1:3] = c
        tgt[b, 0, 3:19] = (c[None, :] + rs.uniform(-0.12, 0.12, (8, 2))).reshape(-1)
        tgt[b, 0, 19:21] = rs.uniform(0.1, 0.4, 2)
    tgt = torch.from_numpy(tgt.reshape(batch, -1))
    forms = {}
    order = (('route', '1'), ('own', '0'))
    for form, env in (order[::-1] if own_first else order):
        os.environ['SSP_UPSAMPLE_FUSE'] = env          # read when the model's plan is built, in its first forward below
        torch.manual_seed(0)
        model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose-up.cfg')).cuda().train()
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
        plan = list(model._plans.values())[0]
        assert list(plan.upsample.values()) == [form], plan.upsample
        forms[form] = (step, [])
    os.environ.pop('SSP_UPSAMPLE_FUSE')
    for _ in range(rounds):
        for form, (step, ms) in forms.items():
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
    for form, (_, ms) in forms.items():
        print(json.dumps(dict(step='yolo-pose-up.cfg B%d %dx%d' % (batch, size, size), upsample=form,
                              ms_per_step=round(float(np.median(ms)), 3), rounds=[round(m, 3) for m in ms],
                              images_per_s=round(batch / float(np.median(ms)) * 1e3, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-step', action='store_true', help='the two kernels only')
    ap.add_argument('--no-kernels', action='store_true', help='the training step only')
    ap.add_argument('--own-first', action='store_true', help='build and time the standalone form first (order effects)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    _lib.load()
    if not args.no_kernels:
        kernels(args.iters)
    if not args.no_step:
        steps(args.batch, args.size, args.steps, args.rounds, args.own_first)


if __name__ == '__main__':
    main()

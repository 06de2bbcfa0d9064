"""Input gradient (dL/dx) on the MI355X: the fused first-block kernel ssp_first_bwd_dgrad alone, and what asking for x.grad
adds to a yolo-pose training step (time and peak memory).

    python tools/input_grad_bench.py [--batch 64] [--size 416] [--step-batch 32] [--steps 8] [--out FILE]
    python tools/input_grad_bench.py --trace-steps 4     # only input-gradient steps (for rocprofv3 --kernel-trace --stats)

Kernel: executed FLOPs count every MFMA the launch issues (the convolution recomputed on the tile plus its one-window border,
and the 32 x 32 product that forms the transposed-conv taps, 27 of its 32 columns used); algorithmic FLOPs are those of
the transposed convolution alone (3 input channels); the fraction is of the 157.3 TFLOP/s fp32 matrix peak."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from singleshotpose_amd import _lib  # noqa: E402

F32_PEAK = 157.3e12
TILE = 6            # pooled pixels per tile side (csrc/conv_first.hip DG_T)


def kernel_bench(B, H, W, reps=20):
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B * H * W, 4, device=dev, generator=g)
    x[:, 3] = 0
    wt = torch.randn(32 * 36, device=dev, generator=g) * 0.3
    gp = torch.randn(B * (H // 2) * (W // 2), 32, device=dev, generator=g)
    vec = torch.rand(6, 32, device=dev, generator=g) + 0.5
    dx = torch.empty(B * H * W, 4, device=dev)
    args = (x.data_ptr(), wt.data_ptr(), gp.data_ptr(), 32) + tuple(vec[i].data_ptr() for i in range(6)) + \
        (0.1, dx.data_ptr(), B, H, W, st)
    for _ in range(3):
        _lib.call('ssp_first_bwd_dgrad', *args)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call('ssp_first_bwd_dgrad', *args)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = float(np.median(ms))
    Ho, Wo = H // 2, W // 2
    nwg = B * -(-Ho // TILE) * -(-Wo // TILE)
    # per workgroup: (TILE + 2) blocks x (18 convolution + 16 tap-product MFMAs) x 32 x 32 x 2 x 2 FLOP
    executed = nwg * (TILE + 2) * (18 + 16) * 4096.0
    algorithmic = 2.0 * B * H * W * 32 * 27
    return dict(kernel='ssp_first_bwd_dgrad', B=B, H=H, W=W, ms=round(ms, 4),
                executed_gflop=round(executed / 1e9, 2), algorithmic_gflop=round(algorithmic / 1e9, 2),
                border_overhead=round(executed / (2.0 * B * H * W * 32 * (36 + 32)), 3),
                executed_tflops=round(executed / ms / 1e9, 1), frac_f32_peak=round(executed / ms / 1e9 / (F32_PEAK / 1e12), 3),
                hbm_gb=round((B * H * W * 16 * 2 + gp.numel() * 4) / 1e9, 3))


def _model():
    from oracle.darknet_ref import seeded_state
    from singleshotpose_amd.darknet import Darknet
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from helpers import load_state_into
    m = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    load_state_into(m, m.blocks, seeded_state(m.blocks, 0))
    return m.cuda().train()


def step_bench(B, S, steps):
    model = _model()
    x = torch.rand(B, 3, S, S, device='cuda')

    def run(want_x, n):
        ts = []
        for _ in range(n):
            model.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(want_x)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            y = model(xi)
            y.backward(torch.ones_like(y))
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
            del y, xi
        return float(np.median(ts))
    res = {}
    for want_x in (False, True, False, True):          # interleaved: warm-up pass, then the measured pair
        run(want_x, 2)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t = run(want_x, steps)
        res['with_x' if want_x else 'plain'] = dict(ms=round(t, 3),
                                                    peak_extra_gb=round((torch.cuda.max_memory_allocated() - base) / 1e9, 3))
    return dict(step='yolo-pose training step', B=B, size=S, steps=steps, plain=res['plain'], with_x=res['with_x'],
                extra_ms=round(res['with_x']['ms'] - res['plain']['ms'], 3),
                extra_peak_gb=round(res['with_x']['peak_extra_gb'] - res['plain']['peak_extra_gb'], 3),
                full_res_map_gb=round(B * S * S * 32 * 4 / 1e9, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--step-batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--trace-steps', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.trace_steps:
        model = _model()
        x = torch.rand(a.step_batch, 3, a.size, a.size, device='cuda')
        for _ in range(a.trace_steps):
            model.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = model(xi)
            y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
        print(json.dumps(dict(trace_steps=a.trace_steps, B=a.step_batch, size=a.size)))
        return
    out = [kernel_bench(a.batch, a.size, a.size), step_bench(a.step_batch, a.size, a.steps)]
    for r in out:
        print(json.dumps(r))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Ordered against atomic filter gradients, per launch: time (HIP events, best of --repeats) and, with --err, the error of the
atomic form and of the two finishing sums (float64, fp32) against a float64 reference on standard-normal operands.

  python tools/wgrad_ordered_bench.py [--batch 64] [--err] [--out FILE]

The shapes are the filter-gradient launches of cfg/yolo-pose.cfg at 416 x 416 (layer: map, Cin -> Cout, R), one per route
family and tile; the numbers behind DESIGN.md section 3d."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from singleshotpose_amd import _lib      # noqa: E402

# (layer, H = W, Cin (padded), Cout, R)
LAYERS = [(0, 416, 4, 32, 3), (2, 208, 32, 64, 3), (4, 104, 64, 128, 3), (5, 104, 128, 64, 1), (8, 52, 128, 256, 3),
          (12, 26, 256, 512, 3), (13, 26, 512, 256, 1), (18, 13, 512, 1024, 3), (23, 13, 1024, 1024, 3), (29, 13, 1280, 1024, 3),
          (30, 13, 1024, 20, 1)]


def time_ms(fn, repeats):
    fn()
    best = None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1)
        best = t if best is None else min(best, t)
    return best


def reference(x, dy, B, H, W, Cin, Cout, R):
    """float64 [Cout][R*R][Cin] on the device, one matmul per tap."""
    xp = torch.nn.functional.pad(x.view(B, H, W, Cin).double(), (0, 0, R // 2, R // 2, R // 2, R // 2))
    dyt = dy.view(-1, dy.shape[-1])[:, :Cout].double().t().contiguous()
    ref = torch.empty(Cout, R * R, Cin, dtype=torch.float64, device=x.device)
    for ky in range(R):
        for kx in range(R):
            ref[:, ky * R + kx, :] = dyt @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Cin)
    return ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--err', action='store_true')
    ap.add_argument('--out')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(1)
    lines = ['layer  map  Cin->Cout R  route      ranges  atomic ms  ordered ms (f64 sum)  (fp32 sum)  ratio' +
             ('   err atomic   err f64 sum   err fp32 sum' if a.err else '')]
    for layer, S, Cin, Cout, R in LAYERS:
        B, H, W = a.batch, S, S
        coutp = (Cout + 3) // 4 * 4
        x = torch.randn(B * H * W, Cin, device=dev, generator=g)
        dy = torch.zeros(B * H * W, coutp, device=dev)
        dy[:, :Cout] = torch.randn(B * H * W, Cout, device=dev, generator=g)
        geom = (B, H, W, Cin, Cout, coutp, Cin, R)
        route = _lib.query('ssp_conv_wgrad_route', *geom)
        ns = _lib.query('ssp_conv_wgrad_ordered_split', *(geom + (1, 0)))
        wsn = _lib.query('ssp_conv_wgrad_ordered_workspace_floats', *(geom + (1, 0)))
        ws = torch.empty(wsn, dtype=torch.float32, device=dev)
        dw = torch.zeros(Cout * R * R * Cin, dtype=torch.float32, device=dev)
        atomic = lambda: _lib.call('ssp_conv_wgrad', dy.data_ptr(), x.data_ptr(), dw.data_ptr(), *(geom + (st,)))
        ordered = lambda flags: _lib.call('ssp_conv_wgrad_ordered', dy.data_ptr(), x.data_ptr(), dw.data_ptr(),
                                          *(geom + (1, 0, flags, ws.data_ptr(), wsn, st)))
        ta, t64, t32 = time_ms(atomic, a.repeats), time_ms(lambda: ordered(0), a.repeats), time_ms(lambda: ordered(1), a.repeats)
        line = '%5d %4d %5d->%-5d %d  %9d %6d  %9.4f  %9.4f             %9.4f  %5.2f' % (layer, S, Cin, Cout, R, route, ns, ta, t64, t32, t64 / ta)
        if a.err:
            ref = reference(x, dy, B, H, W, Cin, Cout, R)
            den = float(ref.abs().max())
            errs = []
            for fn in (atomic, lambda: ordered(0), lambda: ordered(1)):
                dw.zero_()
                fn()
                torch.cuda.synchronize()
                errs.append(float((dw.view_as(ref).double() - ref).abs().max()) / den)
            line += '   %.3e    %.3e     %.3e' % tuple(errs)
            del ref
        print(line, flush=True)
        lines.append(line)
        del x, dy, ws, dw
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

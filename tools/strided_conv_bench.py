#!/usr/bin/env python
"""Stride-2 convolution launches (csrc/conv_strided.hip) next to the stride-1 direct launches they are measured against
(GPU only; medians of torch.cuda event pairs around single launches, every shape warmed up first).

  python tools/strided_conv_bench.py [--B 64,8] [--iters 20] [--out profiles/rNN_strided_conv.txt]

Per 3x3 layer Cin -> Cout on an H x H INPUT map:
  data gradient     ssp_conv_s2_dgrad against ssp_conv_dgrad (plan 0) on the SAME input map and channels - what a nine-tap
                    gather that masks the wrong-parity taps would cost.  The parity decomposition contracts 9/4 taps per
                    input pixel: ideal ratio 0.25, required < 0.5.
  forward           ssp_conv_s2_fwd against ssp_conv_fwd (plan 0) of the same M x N x K: the stride-1 layer on the Ho x Ho
                    OUTPUT map with the same channels.
  filter gradient   ssp_conv_s2_wgrad against ssp_conv_wgrad of the same M x N x K (the same stride-1 layer).
FLOPs are the algorithm's: 2 * M * N * K of each launch (strided data gradient: summed over the parity classes)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from singleshotpose_amd import _lib

LAYERS = [(104, 64, 128), (26, 256, 512), (13, 512, 1024)]      # (H of the input map, Cin, Cout), 3x3


def median_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', default='64,8')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("strided_conv_bench: needs the GPU (no timing without one)")
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    call, q = _lib.call, _lib.query
    lines = ['%-22s %3s | %-6s %10s %8s | %-14s %10s %8s | ratio' % ('layer (3x3, input map)', 'B', 'op', 'strided us', 'TF',
                                                                     'stride-1 launch', 'us', 'TF')]
    print(lines[0], flush=True)
    R = 3
    for B in [int(b) for b in args.B.split(',')]:
        for H, Cin, Cout in LAYERS:
            Ho = (H + 2 - R) // 2 + 1
            Mi, Mo = B * H * H, B * Ho * Ho
            g = torch.Generator(device='cpu').manual_seed(1)
            rnd = lambda n, s=1.0: ((torch.rand(n, generator=g) * 2 - 1) * s).to(dev)
            x, dyo, dyi = rnd(Mi * Cin), rnd(Mo * Cout), rnd(Mi * Cout)      # input map, output-map gradient, input-map-sized gradient
            w, wd = rnd(Cout * 9 * Cin, 0.05), rnd(Cin * 9 * Cout, 0.05)
            out_o, dx = torch.empty(Mo * Cout, device=dev), torch.empty(Mi * Cin, device=dev)
            xo = x[:Mo * Cin]                                                 # an Ho x Ho map of Cin channels
            dw = torch.zeros(Cout * 9 * Cin, device=dev)
            wsn = max(1, q('ssp_conv_workspace_floats', B, H, H, Cout, Cin, R, 0), q('ssp_conv_workspace_floats', B, Ho, Ho, Cin, Cout, R, 0))
            ws = torch.empty(wsn, device=dev)
            K = 9 * Cin
            taps = sum(((H - py + 1) // 2) * ((H - px + 1) // 2) * (1 + py) * (1 + px) for py in (0, 1) for px in (0, 1))
            rows = [
                ('dgrad', lambda: call('ssp_conv_s2_dgrad', dyo.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, H, H, Cout, Cin, Cout,
                                       Cin, R, 0, st), 2.0 * B * taps * Cin * Cout,
                 'dgrad %dx%d' % (H, H), lambda: call('ssp_conv_dgrad', dyi.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, H, H, Cout,
                                                      Cin, Cout, Cin, R, 0, 0, ws.data_ptr(), wsn, st), 2.0 * Mi * Cin * 9 * Cout),
                ('fwd', lambda: call('ssp_conv_s2_fwd', x.data_ptr(), w.data_ptr(), out_o.data_ptr(), None, None, B, H, H, Cin, Cout,
                                     Cin, Cout, R, 0, st), 2.0 * Mo * Cout * K,
                 'fwd %dx%d' % (Ho, Ho), lambda: call('ssp_conv_fwd', xo.data_ptr(), w.data_ptr(), out_o.data_ptr(), None, None, B, Ho,
                                                      Ho, Cin, Cout, Cin, Cout, R, 0, 0, ws.data_ptr(), wsn, st), 2.0 * Mo * Cout * K),
                ('wgrad', lambda: call('ssp_conv_s2_wgrad', dyo.data_ptr(), x.data_ptr(), dw.data_ptr(), B, H, H, Cin, Cout, Cout, Cin,
                                       R, st), 2.0 * Mo * Cout * K,
                 'wgrad %dx%d' % (Ho, Ho), lambda: call('ssp_conv_wgrad', dyo.data_ptr(), xo.data_ptr(), dw.data_ptr(), B, Ho, Ho, Cin,
                                                        Cout, Cout, Cin, R, st), 2.0 * Mo * Cout * K),
            ]
            for op, fn, flop, rname, rfn, rflop in rows:
                t, tr = median_us(fn, args.iters), median_us(rfn, args.iters)
                lines.append('%4d -> %4d @ %3d^2    %3d | %-6s %10.1f %8.1f | %-14s %10.1f %8.1f | %.3f' % (
                    Cin, Cout, H, B, op, t, flop / t / 1e6, rname, tr, rflop / tr / 1e6, t / tr))
                print(lines[-1], flush=True)
            del x, dyo, dyi, w, wd, out_o, dx, dw, ws
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

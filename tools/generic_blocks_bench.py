"""Bandwidth of the csrc/generic_blocks.hip kernels at sizes a user would run (B = 64 maps of a residual / tiny-YOLO /
Darknet-19 net): algorithmic bytes moved / time per launch, against the 8 TB/s HBM peak.

Each case cycles through enough independent buffer sets (>= 1 GiB together) that its operands cannot stay in the 256 MB
Infinity Cache between launches.  Time per launch = HIP events around `--iters` back-to-back launches after a warm-up
(it includes the launch gaps; run the same command under `rocprofv3 --kernel-trace --stats` for kernel-only times).
Prints one JSON line per case.

    python tools/generic_blocks_bench.py [--iters 200]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    tbps = nbytes / (us * 1e-6) / 1e12
    print(json.dumps(dict(kernel=name, bytes=nbytes, us_per_launch=round(us, 2), TBps=round(tbps, 3),
                          frac_of_hbm_peak=round(tbps / HBM_TBPS, 3), buffer_sets=len(launches))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    _lib.load()
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    call = _lib.call
    buf = lambda n: torch.randn(n, dtype=torch.float32, device=dev)

    # shortcut: out = leaky(a + b); backward reads g and out, writes both summands' gradients
    for (B, H, W, C) in ((64, 52, 52, 256), (64, 26, 26, 512)):
        M = B * H * W
        t = M * C * F32
        k = nsets(3 * t)
        sets = [[buf(M * C) for _ in range(3)] for _ in range(k)]
        run('shortcut_fwd B%d %dx%dx%d' % (B, H, W, C),
            [lambda s=s: call('ssp_shortcut_fwd', s[0].data_ptr(), C, s[1].data_ptr(), C, s[2].data_ptr(), C, C, M, 0.1, st)
             for s in sets], 3 * t, args.iters)
        del sets
        k = nsets(4 * t)
        sets = [[buf(M * C) for _ in range(4)] for _ in range(k)]
        run('shortcut_bwd B%d %dx%dx%d' % (B, H, W, C),
            [lambda s=s: call('ssp_shortcut_bwd', s[0].data_ptr(), C, s[1].data_ptr(), C, s[2].data_ptr(), C, 0,
                              s[3].data_ptr(), C, 0, C, M, 0.1, st) for s in sets], 4 * t, args.iters)
        del sets

    B, H, W, C = 64, 13, 13, 1024
    M = B * H * W
    t = M * C * F32
    # stride-1 max-pool: reads x, writes out (forward); reads x and g, writes dx (backward)
    sets = [[buf(M * C) for _ in range(2)] for _ in range(nsets(2 * t))]
    run('maxpool_s1_fwd B%d %dx%dx%d' % (B, H, W, C),
        [lambda s=s: call('ssp_maxpool_s1_fwd', s[0].data_ptr(), C, s[1].data_ptr(), C, C, B, H, W, st) for s in sets],
        2 * t, args.iters)
    del sets
    sets = [[buf(M * C) for _ in range(3)] for _ in range(nsets(3 * t))]
    run('maxpool_s1_bwd B%d %dx%dx%d' % (B, H, W, C),
        [lambda s=s: call('ssp_maxpool_s1_bwd', s[0].data_ptr(), C, s[1].data_ptr(), C, s[2].data_ptr(), C, C, B, H, W, 0, st)
         for s in sets], 3 * t, args.iters)
    del sets
    # global average pool: reads the map, writes B x C (forward); reads B x C, writes the map (backward)
    sets = [[buf(M * C), buf(B * C)] for _ in range(nsets(t))]
    run('avgpool_fwd B%d %dx%dx%d' % (B, H, W, C),
        [lambda s=s: call('ssp_avgpool_fwd', s[0].data_ptr(), C, s[1].data_ptr(), C, C, B, H, W, st) for s in sets],
        t + B * C * F32, args.iters)
    run('avgpool_bwd B%d %dx%dx%d' % (B, H, W, C),
        [lambda s=s: call('ssp_avgpool_bwd', s[1].data_ptr(), C, s[0].data_ptr(), C, C, B, H, W, 0, st) for s in sets],
        t + B * C * F32, args.iters)
    del sets

    # softmax over a 1000-class head at batch 64 (256 KB: launch-bound by construction)
    R, C = 64, 1000
    x, y, g, dx = buf(R * C), buf(R * C), buf(R * C), buf(R * C)
    run('softmax_fwd %dx%d' % (R, C), [lambda: call('ssp_softmax_fwd', x.data_ptr(), C, y.data_ptr(), C, C, R, st)],
        2 * R * C * F32, args.iters)
    run('softmax_bwd %dx%d' % (R, C),
        [lambda: call('ssp_softmax_bwd', y.data_ptr(), C, g.data_ptr(), C, dx.data_ptr(), C, C, R, 0, st)],
        3 * R * C * F32, args.iters)


if __name__ == '__main__':
    main()

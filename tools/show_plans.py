#!/usr/bin/env python
"""Prints the autotuned igemm plan of every conv launch of cfg/yolo-pose.cfg at a given batch / size
(plan code = tail*100000 + tile_rows*100 + ksplit*10 + ring_slots; 0 = library heuristic; 9xxxxxx = Winograd F(2x2), 8xxxxxx = Winograd F(4x4),
7xxxxxx = on-chip F(2x2), 6xxxxxx = bf16x3 (6000000 + tile_rows*100 + ksplit*10 + 3; only with SSP_CONV_MATH=bf16x3 / bf16x3-wino),
86xxxxx / 96xxxxx = a Winograd plan with its batched GEMM on the bf16x3 kernel (only with SSP_CONV_MATH=bf16x3-wino))."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from singleshotpose_amd.darknet import Darknet
from singleshotpose_amd.engine import conv_math_of, wino_fused, wino_tile, x3_wino


def family(code):
    if x3_wino(code):      # a Winograd plan with its batched GEMM on the bf16 matrix cores (only with SSP_CONV_MATH=bf16x3-wino)
        return 'F(%dx%d) bf16x3' % (wino_tile(code), wino_tile(code))
    if conv_math_of(code) == 'bf16x3':
        return 'bf16x3'
    if wino_fused(code):
        return 'F(2x2) on-chip'
    return 'F(%dx%d)' % (wino_tile(code), wino_tile(code)) if wino_tile(code) else 'direct'


B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
S = int(sys.argv[2]) if len(sys.argv) > 2 else 416
CFG = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'cfg', 'yolo-pose.cfg')      # (e.g. cfg/yolo-pose-up.cfg)
m = Darknet(CFG).cuda().train()
x = torch.rand(B, 3, S, S, device='cuda')
m(x).sum().backward()
plan = list(m._plans.values())[0]
for ind, cs in sorted(plan.convs.items()):
    print('layer %2d  %4dx%-4d %4d->%-4d k%d  fwd %7d %-14s  dgrad %7d %-14s  wgrad %s' % (
        ind, cs.H, cs.W, cs.cin, cs.cout, cs.k, cs.plan_fwd, family(cs.plan_fwd), cs.plan_dgrad, family(cs.plan_dgrad),
        ('winograd F(%dx%d)' % (cs.wgrad_wino, cs.wgrad_wino)) if getattr(cs, 'wgrad_wino', 0) else 'direct'))
for ind in plan.depthwise:      # groups = channels: csrc/conv_depthwise.hip at all three launches (the codes above do not apply)
    cs = plan.convs[ind]
    print('layer %2d  depthwise 3x3 / %d on %dx%d x%d -> %dx%d, statistics tiles %d' % (
        ind, cs.stride, cs.Hi, cs.Wi, cs.cin, cs.H, cs.W, cs.ntile))
for ind, form in sorted(plan.upsample.items()):      # 'route': written into the concatenation buffer of the route behind it
    a = plan.acts[ind]
    print('layer %2d  upsample x%s -> %dx%d x%d, row stride %d: %s' % (
        ind, m.blocks[ind + 1].get('stride', 2), a.H, a.W, a.C, a.ld, form))
print('conv math: %r' % (plan.conv_math,))
det = plan.deterministic
print('deterministic: %s' % ('on' if det['mode'] else 'off'))
for ind, rec in sorted(det['layers'].items()):      # (mode on: form, route code or Winograd tile and pixel ranges of every filter gradient)
    form, code, nsplit = rec['wgrad']
    print('layer %2d  wgrad %-16s %-10s ranges %-5d dgrad %-16s bn sums %s' % (
        ind, form, ('tile %d' % code) if form == 'winograd-ordered' else (code or '-'), nsplit, rec['dgrad'], rec['bn_sums']))
for ind, what in det['taken_back']:
    print('layer %2d  taken back: %s' % (ind, what))

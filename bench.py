#!/usr/bin/env python
"""Hot-path benchmark: yolo-pose.cfg training step (zero_grad, forward, RegionLoss, backward, grad all-reduce, SGD) on
synthetic 416x416 batches, 64 images per GPU (BASELINE.json metric).

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0.  `value` = images/s of the whole job (all ranks), max-over-ranks time of exactly K
steps between barrier + synchronize pairs, inputs resident in HBM; `ms_per_step` = that time / K.  Every step starts
from the same seeded weights, and the metric's workload runs the committed plan set cfg/bench_tune_cache.json (unless
SSP_TUNE_CACHE names another): with the same arguments, each run computes the same step up to fp32 rounding.

A plain run does only what that headline needs: set-up, W warm-up steps, the K timed steps, the outputs (--dump-outputs)
and the result line.  --dump-outputs DIR writes what the last timed step computed, as a caller of the step receives it:
the head output, the loss, a fixed seeded sample of the updated parameters and of their gradients, the BatchNorm
running statistics (DIR/<name>.npy, float32 / float64, about 35 MB).

Everything else is measured with --full only: the oracle check of one step before timing (`verify`), the per-launch HIP
event timers in the timed region and the further untimed passes behind the rooflines and `kernel_ms_per_step`, the
multi-rank gradient check and `comm` diagnostics, the other configurations (`extra`) and `cpu_baseline`.

With --full: `roofline` is for the dominant kernel (the
implicit-GEMM conv kernel, forward launches): the FLOPs its MFMA pipe EXECUTED (a Winograd-plan layer counts its batched
GEMMs, not the direct convolution) / the HIP-event time of those launches, against the fp32 MFMA peak (157.3 TFLOP/s,
MI355X_MICROARCH.md), from HIP events inside the timed region (on every 5th step of it: `roofline.timed_steps` - carried by
every step the ~66 event pairs cost 0.37 ms of the step they measure); `launch_units` in it charges the HBM-bound Winograd
transform / finishing launches to the same FLOPs, `effective` is the algorithmic (direct-convolution) rate.
`roofline_wino_transforms` is the HBM roofline of those passes.  `roofline_dgrad` / `roofline_wgrad` (kernel-exclusive) and
`roofline_bwd` (the two backward streams as they overlap in the step) come - like `kernel_ms_per_step` - from further,
untimed passes with the launches bracketed by events.  `cpu_baseline` times the reference's own modules (or the CPU
oracle of the same step, oracle/) on this host for a bounded batch - rank 0, N=1 only.
"""
import argparse
import json
import os
import re
import sys
import time

# HIP multiplexes a process's streams over GPU_MAX_HW_QUEUES hardware queues (4 by default).  RCCL brings its own streams:
# with 4 queues the step's two compute streams then share one and run one after the other (measured on one rank with a live
# process group, profiles/r04_rccl_queues.txt: 35.7 ms per step against 28.4 ms; 28.9 ms with 8 queues).  Read when the HIP
# runtime initialises, so it is set before torch is imported; an explicit setting in the environment wins.
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3   # 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz
PEAK_HBM_GBS = 8000.0           # HBM3E, MI355X_MICROARCH.md (~6.3 TB/s achievable)


def synthetic_batch(B, H, W, seed, device):
    """images ~ U[0,1) (what ToTensor yields), one label per image: class 0, 9 keypoints in (0.25,0.75), ranges 0.2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=g)
    t = torch.zeros(B, 50, 21, dtype=torch.float64)
    t[:, 0, 1:19] = torch.rand(B, 18, generator=g, dtype=torch.float64) * 0.5 + 0.25
    t[:, 0, 19:21] = 0.2
    return x.to(device), t.view(B, -1)   # labels stay on the host (float64), as train.py:83 leaves them


def _cpu_port_step_fn(cfgfile, B, H, W):
    """One training step on the CPU oracle (oracle/: the reference's semantics restated on PyTorch-CPU kernels)."""
    from oracle.darknet_ref import forward_ref, seeded_state
    from oracle.region_loss_ref import region_loss_ref
    from singleshotpose_amd.cfg import parse_cfg
    blocks = parse_cfg(cfgfile)
    state = seeded_state(blocks, 0)
    for e in state:
        if e is not None:
            for k, v in e.items():
                if not k.startswith('running'):
                    v.requires_grad_(True)
    x, tgt = synthetic_batch(B, H, W, 0, 'cpu')

    def one_step():
        t0 = time.time()
        y = forward_ref(blocks, state, x, training=True)
        r = region_loss_ref(y.detach(), tgt, 20)
        y.backward(r['grad'])
        for e in state:
            if e is not None:
                for v in e.values():
                    v.grad = None
        return time.time() - t0
    return one_step


def _reference_times(cfgfile, B, size, threads, repeats=1, timeout=240):
    """seconds per step of the REFERENCE's own Darknet + RegionLoss on this host's CPU for each thread count
    (oracle/time_reference_cpu.py in its own process - it redirects torch.cuda.* to the CPU), or None."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, 'oracle', 'time_reference_cpu.py'), cfgfile, str(B), str(size),
           ','.join(str(t) for t in threads), str(repeats)]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=timeout,
                             env=dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES=''))
        rec = json.loads(out.stdout.strip().splitlines()[-1])
    except Exception:
        return None
    if 'seconds_per_step' not in rec:
        return None
    rec['seconds_per_step'] = {int(k): v for k, v in rec['seconds_per_step'].items()}
    return rec


def cpu_baseline(cfgfile, B, H, W, budget_s=30.0, big_batch=64):
    """The same training step (forward, RegionLoss, backward) on this host's CPU cores - a reported baseline, not a target.

    kind "reference": the reference's OWN modules (darknet.Darknet, region_loss.RegionLoss with the three torch >= 0.5
    patches of SURVEY.md 8(c)), staged under oracle/_ref by oracle/stage_reference.py and timed in a separate process.
    kind "port" (only when nothing was staged): the oracle/ restatement - the same ATen / oneDNN kernels underneath.

    A B = 8 step (the cfg's own batch, yolo-pose.cfg:3) does not scale to every hardware thread of a 2-socket host
    (128 threads measured SLOWER than 8 in round 1): one warm-up + one timed step per thread count in {8, 16, 32, 64,
    all}, then the best count is timed again (median of 3) and reported with the count that won; the metric's own batch
    (64) is timed at the two largest counts only (one warm-up + one step each: ~7 s per step)."""
    all_threads = torch.get_num_threads()
    ncpu = os.cpu_count() or all_threads
    quota = None          # CPU-bandwidth limit of this container (cgroup v2 cpu.max "quota period"): the cores a step can really use
    try:
        q, per = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        quota = None if q == 'max' else round(float(q) / float(per), 2)
    except Exception:
        pass
    cands = sorted(set(t for t in (8, 16, 32, 64, all_threads) if t <= max(all_threads, 8)))
    t_begin = time.time()
    ref = _reference_times(cfgfile, B, H, cands)
    if ref is not None:
        sweep = ref['seconds_per_step']
        best = min(sweep, key=sweep.get)
        again = _reference_times(cfgfile, B, H, [best], repeats=3)
        med = again['seconds_per_step'][best] if again else sweep[best]
        res = {"value": round(B / med, 3), "unit": "images/s", "cores": int(best), "kind": "reference", "batch": B,
               "sample": "reference darknet.Darknet + region_loss.RegionLoss (patched for torch >= 0.5, CPU): median of 3 "
                         "steps of fwd+RegionLoss+bwd at batch %d, %dx%d with %d threads - the fastest of a one-step sweep "
                         "over %s threads" % (B, H, W, best, sorted(sweep)),
               "modules": ref['modules'],
               "sweep_images_per_s": {str(k): round(B / v, 3) for k, v in sorted(sweep.items())}, "host_cpus": ncpu,
               "cgroup_cpu_quota_cores": quota}
        if big_batch and big_batch != B and time.time() - t_begin < budget_s + 30:
            big = _reference_times(cfgfile, big_batch, H, sorted(set(cands[-2:])), timeout=300)
            if big is not None:
                bs = big['seconds_per_step']
                bb = min(bs, key=bs.get)
                res["batch%d" % big_batch] = {"value": round(big_batch / bs[bb], 3), "unit": "images/s", "cores": int(bb),
                                              "sample": "1 step after 1 warm-up at batch %d, threads %s" % (big_batch, sorted(bs)),
                                              "sweep_images_per_s": {str(k): round(big_batch / v, 3) for k, v in sorted(bs.items())}}
        res["seconds"] = round(time.time() - t_begin, 1)
        return res
    one_step = _cpu_port_step_fn(cfgfile, B, H, W)
    sweep = {}
    for nt in cands:
        torch.set_num_threads(nt)
        one_step()                                  # warm-up at this thread count (oneDNN primitive caches)
        sweep[nt] = one_step()
        if time.time() - t_begin > budget_s:
            break
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    one_step()                                      # the thread count changed again: warm up before timing
    times = []
    while len(times) < 3 and (not times or time.time() - t_begin < budget_s + 15):
        times.append(one_step())
    torch.set_num_threads(all_threads)
    med = float(np.median(times))
    return {"value": round(B / med, 3), "unit": "images/s", "cores": int(best), "kind": "port", "batch": B,
            "sample": "oracle/ restatement (no oracle/_ref/modules.zip staged): %d steps of fwd+RegionLoss+bwd at batch %d, "
                      "%dx%d (median) with %d threads - the fastest of a one-step sweep over %s threads"
                      % (len(times), B, H, W, best, sorted(sweep)),
            "sweep_images_per_s": {str(k): round(B / v, 3) for k, v in sorted(sweep.items())},
            "host_cpus": ncpu}


def forward_traffic_per_launch():
    """HBM bytes per forward launch of the conv kernel, from the PMC passes committed under profiles/ (FETCH_SIZE
    doubled per MI355X_MICROARCH.md + WRITE_SIZE; tools/gpu_check.sh, tools/traffic_summary.py).  PMC counters cannot
    be read from inside this process, so the figure is that of the last committed profile of this same command - and
    only while the kernels are the ones that were profiled: the summary records a digest of singleshotpose_amd/csrc at
    profile time, and a digest that no longer matches drops the figure (null) instead of reporting a stale one."""
    import glob
    from singleshotpose_amd._lib import csrc_digest
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_traffic.json')))
    if not files:
        return None, None
    data = json.load(open(files[-1]))
    src = os.path.relpath(files[-1], ROOT)
    meta = data.pop('_meta', {})
    if meta.get('csrc_sha1') != csrc_digest():
        return None, "%s is stale: kernels changed since it was taken (csrc digest %s, now %s)" % (
            src, str(meta.get('csrc_sha1'))[:10], csrc_digest()[:10])
    tot, n = 0.0, 0
    for name, v in data.items():
        # conv_igemm_dma_kernel<BM, BN, PASS, ...> and conv_igemm_kernel<BM, BN, WM, WN, BK, ABL, PASS> (first layer):
        # PASS 0 = forward launches, 1 = data-gradient launches of the same code
        fwd = (re.search(r'conv_igemm_dma_kernel<\d+, \d+, 0[,>]', name) is not None or
               re.search(r'conv_igemm_kernel<(\d+, ){6}0>', name) is not None)
        if fwd:
            tot += v['launches'] * (v['fetch_bytes_per_launch_corrected'] + v['write_bytes_per_launch_reported'])
            n += v['launches']
    return (round(tot / n) if n else None), src


def wino_traffic_per_step():
    """Fabric bytes per training step of the Winograd transform / finishing kernels, from the committed PMC passes
    (profiles/r*_traffic.json: launches there cover `steps_profiled` steps), or None when the kernels changed since."""
    import glob
    from singleshotpose_amd._lib import csrc_digest
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_traffic.json')))
    if not files:
        return None, None
    data = json.load(open(files[-1]))
    src = os.path.relpath(files[-1], ROOT)
    meta = data.pop('_meta', {})
    if meta.get('csrc_sha1') != csrc_digest():
        return None, "%s is stale: kernels changed since it was taken" % src
    steps = float(meta.get('steps_profiled', 2))
    tot = 0.0
    for name, v in data.items():
        if name.startswith('wino_') and 'wino_filter' not in name:
            tot += v['launches'] * (v['fetch_bytes_per_launch_corrected'] + v['write_bytes_per_launch_reported'])
    return round(tot / steps), src


def _budget_record(model):
    for plan in model._plans.values():
        hb = getattr(plan, 'head_budget', None)
        if hb:
            if hb.get('pinned'):
                return {"budget": hb['budget'], "pinned": "decisions read from SSP_TUNE_CACHE (measured by the process that wrote it)",
                        "chosen": {str(i): c for i, c in hb['chosen'].items()}}
            return {"budget": hb['budget'], "head_deviation_of_the_chosen_plans": float('%.3g' % hb['head_deviation']),
                    "moved": [{"layer": i, "from": "F(%dx%d)" % (a, a), "to": ("F(%dx%d)" % (b, b)) if b else "direct"} for i, a, b in hb['moved']],
                    "cost_ms_per_forward": round(hb['cost_ms'], 4),
                    "per_layer_candidates": {str(i): [{"family": ("F(%dx%d)" % (f, f)) if f else "direct", "plan": c, "ms": t, "head_deviation": d}
                                                      for f, c, t, d in rows] for i, rows in hb['table'].items()},
                    "env": "SSP_HEAD_ERR_BUDGET (0 = always the fastest code)"}
    return None


def verify_step(model, crit, B, H, W, seed, exact=False):
    """One training step of THIS model on THIS batch against the CPU oracle (oracle/step_check.py), before anything is
    timed: head / loss / running statistics vs an independent oracle forward, every conv launch vs the oracle's
    convolution, parameter gradients vs the decision-frozen oracle backward.  The autotuned plans are the ones the timed
    steps run.  Returns (verified, details)."""
    from oracle.step_check import check_train_step
    x_cpu, tgt = synthetic_batch(B, H, W, seed, 'cpu')
    t0 = time.time()
    r = check_train_step(model, crit, x_cpu, tgt, 20, exact=exact)
    bars = {'head': 1e-4, 'loss': 1e-4, 'running': 1e-4, 'conv': 1e-4, 'grad_out': 1e-4, 'grad': 1e-4}   # north_star's 1e-4; the
    # tests assert tighter ones on this batch (tests/test_gpu_fullsize.py: head 5e-5, every gradient 7e-5) - `margin` below
    ok = all(r[k] < bars[k] for k in bars)
    # yardstick: distance to a float64 evaluation of the same raw-output-frozen network - the product's worst parameter
    # and the fp32 oracle's own (the product must be within 1e-4 or 3x the oracle's distance, parameter by parameter)
    # (--verify-exact: adds ~50 s of float64 CPU work; tests/test_gpu_fullsize.py always runs it)
    if exact:
        ok = ok and all(a <= max(1e-4, 3.0 * b) for a, b in r['grad64_by_param'].values())
    det = {k: float('%.3g' % r[k]) for k in list(bars) + (['grad64', 'grad64_ref', 'head64', 'head64_ref'] if exact else [])}
    # margin = bar / error per quantity (how much headroom each parity bar has on this batch with this box's plan set), the
    # parameter gradients split into the first layer's filter (bar 5e-4, see above) and every other parameter (bar 1e-4)
    others = {n: e for n, e in r['grad_by_param'].items() if n != '0.weight'}
    worst = sorted(others.items(), key=lambda kv: -kv[1])[:3]
    det['grad_other_params'] = float('%.3g' % max(others.values()))
    det['grad_first_filter'] = float('%.3g' % r['grad_by_param'].get('0.weight', 0.0))
    det['margin'] = {k: round(bars[k] / max(r[k], 1e-30), 1) for k in ('head', 'loss', 'running', 'conv', 'grad_out')}
    det['margin']['grad_other_params'] = round(1e-4 / max(det['grad_other_params'], 1e-30), 1)
    det['margin']['grad_first_filter'] = round(1e-4 / max(det['grad_first_filter'], 1e-30), 1)
    det['worst_grad_params'] = [[n, float('%.3g' % e)] for n, e in worst]
    det['conv_worst_layer'] = max(r['conv_by_layer'].items(), key=lambda kv: kv[1])[0] if r.get('conv_by_layer') else None
    det.update(bars={k: v for k, v in bars.items()}, seconds=round(time.time() - t0, 1),
               tuned_plans=sum(1 for _, f, d in r['plans'] if f or d),
               what="1 train step, batch %d, %dx%d, vs oracle/step_check.py (CPU, reference semantics)" % (B, H, W))
    model.zero_grad(set_to_none=True)
    return ok, det


def dump_outputs(out_dir, model, loss, head, sample=1 << 22):
    """What the last timed step handed its caller, as DIR/<name>.npy: the head output, the loss, the BatchNorm running
    statistics, and of the updated parameters and their gradients (50.5 M floats each, in model.parameters() order and
    logical NCHW order) the same `sample` positions, drawn with a fixed seed - about 35 MB in all."""
    os.makedirs(out_dir, exist_ok=True)
    params = list(model.parameters())
    flat_p = torch.cat([p.detach().reshape(-1) for p in params])
    flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1) for p in params])
    n = flat_p.numel()
    if n > sample:
        idx = torch.randint(0, n, (sample,), generator=torch.Generator().manual_seed(0)).sort().values.to(flat_p.device)
        flat_p, flat_g = flat_p[idx], flat_g[idx]
    running = [b.detach().reshape(-1).float() for name, b in model.named_buffers() if name.endswith(('running_mean', 'running_var'))]
    arrays = {'head': head, 'loss': loss.detach().reshape(1), 'params_sample': flat_p, 'grads_sample': flat_g,
              'bn_running_stats': torch.cat(running)}
    for name, t in arrays.items():
        a = t.cpu().numpy()
        np.save(os.path.join(out_dir, name + '.npy'), a if a.dtype == np.float64 else a.astype(np.float32))


def extras(device, steps=5):
    """Driver-record lines for BASELINE configs 4 and 5 (not the metric): the multi-object cfg's training step and the
    inference path at valid.py's 672 x 672 operating point."""
    from singleshotpose_amd.darknet import Darknet, DarknetMulti
    from singleshotpose_amd.optim import SGD
    from singleshotpose_amd.region_loss import RegionLossMulti
    from singleshotpose_amd.utils import get_region_boxes
    out = {}

    def timed(fn, n, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    torch.manual_seed(0)
    B = 64
    model = DarknetMulti(os.path.join(ROOT, 'cfg', 'yolo-pose-multi.cfg')).to(device).train()
    crit = RegionLossMulti(num_keypoints=9, num_classes=13, anchors=model.anchors, num_anchors=5, pretrain_num_epochs=0)
    crit.verbose = False
    opt = SGD(model.parameters(), lr=1e-3 / B, momentum=0.9, dampening=0, weight_decay=0.0005 * B)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 3, 416, 416, generator=g).to(device)
    t = torch.zeros(B, 50, 21, dtype=torch.float64)
    for k in range(8):                      # 8 labels per image (1 object + 7 occluders, image_multi.py:8-36)
        c = torch.rand(B, 2, generator=g, dtype=torch.float64) * 0.6 + 0.2
        t[:, k, 0] = torch.randint(0, 13, (B,), generator=g).double()
        t[:, k, 1:3] = c
        t[:, k, 3:19] = (c[:, None, :] + (torch.rand(B, 8, 2, generator=g, dtype=torch.float64) - 0.5) * 0.24).reshape(B, 16)
        t[:, k, 19:21] = torch.rand(B, 2, generator=g, dtype=torch.float64) * 0.3 + 0.1
    tgt = t.view(B, -1)

    def step():
        opt.zero_grad(set_to_none=True)
        crit(model(x), tgt, 1).backward()
        opt.step()
    dt = timed(step, steps)
    out['multi_cfg_train_step'] = {"workload": "cfg/yolo-pose-multi.cfg train step, 416x416, batch 64, 8 labels/image",
                                   "ms_per_step": round(dt * 1e3, 3), "images_per_s": round(B / dt, 1)}
    del model, opt
    torch.cuda.empty_cache()
    # the shipped cfg's own batch (yolo-pose.cfg:3, what the reference's unmodified train.py runs): launch- / ramp-bound
    from singleshotpose_amd.region_loss import RegionLoss
    torch.manual_seed(0)
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg')).to(device).train()
    crit1 = RegionLoss()
    crit1.verbose = False
    opt = SGD(model.parameters(), lr=1e-3 / 8, momentum=0.9, dampening=0, weight_decay=0.0005 * 8)
    x8, t8 = synthetic_batch(8, 416, 416, 77, device)

    def step8():
        opt.zero_grad(set_to_none=True)
        crit1(model(x8), t8, 20).backward()
        opt.step()
    dt = timed(step8, 20, warm=3)
    out['train_416_b8'] = {"workload": "cfg/yolo-pose.cfg train step, 416x416, batch 8 (the cfg's own batch)",
                           "ms_per_step": round(dt * 1e3, 3), "images_per_s": round(8 / dt, 1)}
    del model, opt, x8
    torch.cuda.empty_cache()
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg')).to(device).eval()
    with torch.no_grad():
        for b, n in ((1, 30), (64, 5)):
            xi = torch.rand(b, 3, 672, 672, generator=g).to(device)
            dt = timed(lambda: model(xi), n, warm=3)
            out['eval_672_b%d' % b] = {"workload": "cfg/yolo-pose.cfg eval forward, 672x672, batch %d" % b,
                                        "ms": round(dt * 1e3, 4), "images_per_s": round(b / dt, 1)}
            if b == 1:
                y = model(xi)
                dt = timed(lambda: get_region_boxes(y, 1, 9), 50, warm=5)
                out['get_region_boxes_b1_us'] = round(dt * 1e6, 1)
    return out


def multiscale_extras(device, B=64, sizes=(224, 608, 832), steps=4):
    """SURVEY.md 8(f) row 2 (train.py after epoch 10 draws H = W from 224..832 every 10 batches, dataset.py:66-90): the
    training step at other resolutions - images/s and conv-FLOP fraction of the fp32-MFMA peak (87.673 GFLOP per image
    scales with the pixel count) - and what the FIRST visit of a new shape costs (plan build + per-launch autotune +
    verify-after-tune, forward and backward) with (a) nothing cached, (b) the timed choices known (what a process started
    with SSP_TUNE_CACHE=<file> sees: choices loaded, each verified once), (c) choices known and verified (a shape whose
    plan was evicted from the LRU and is rebuilt)."""
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.optim import SGD
    from singleshotpose_amd.region_loss import RegionLoss
    torch.manual_seed(0)
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg')).to(device).train()
    crit = RegionLoss()
    crit.verbose = False
    opt = SGD(model.parameters(), lr=1e-3 / B, momentum=0.9, dampening=0, weight_decay=0.0005 * B)
    out = {}
    for size in sizes:
        x, tgt = synthetic_batch(B, size, size, 2000 + size, device)

        def step():
            opt.zero_grad(set_to_none=True)
            crit(model(x), tgt, 20).backward()
            opt.step()

        def first_visit():
            model._plans.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        keep = dict(engine._TUNE_CACHE), dict(engine._TUNE_VERIFIED)
        cache_file, engine._TUNE_CACHE_FILE[0] = engine._TUNE_CACHE_FILE[0], None     # the experiment must not rewrite SSP_TUNE_CACHE
        if cache_file:
            os.environ.pop('SSP_TUNE_CACHE', None)
        engine._TUNE_CACHE.clear()
        engine._TUNE_VERIFIED.clear()
        cold = first_visit()
        engine._TUNE_VERIFIED.clear()
        warm_file = first_visit()
        rebuilt = first_visit()
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        engine._TUNE_CACHE.update(keep[0])
        engine._TUNE_VERIFIED.update(keep[1])
        if cache_file:
            os.environ['SSP_TUNE_CACHE'] = cache_file
            engine._TUNE_CACHE_FILE[0] = cache_file
        flop = 87.673e9 * (size / 416.0) ** 2
        plan = next(iter(model._plans.values()))
        out['train_%d_b%d' % (size, B)] = {
            "workload": "cfg/yolo-pose.cfg train step, %dx%d, batch %d" % (size, size, B),
            "ms_per_step": round(dt * 1e3, 3), "images_per_s": round(B / dt, 1),
            "step_conv_effective_flop_frac_of_peak": round(B / dt * flop / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
            "first_visit_ms": {"cold_tune_cache": round(cold, 1), "warm_tune_cache_unverified": round(warm_file, 1),
                               "warm_tune_cache_verified": round(rebuilt, 1)},
            "tuned_launches": sum(1 for cs in plan.convs.values() if cs.plan_fwd or cs.plan_dgrad)}
        del x
        model._plans.clear()
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64, help='images per GPU')
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--cfg', default=os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-verify', action='store_true', help='skip the one-step oracle check that runs before timing (N=1)')
    ap.add_argument('--verify-exact', action='store_true', help='also the float64 yardstick of oracle/step_check.py (+~50 s)')
    ap.add_argument('--no-extras', action='store_true', help='skip the multi-cfg / 672x672 inference lines (N=1)')
    ap.add_argument('--cpu-batch', type=int, default=8)
    ap.add_argument('--timers', default='conv', choices=['conv', 'all', 'none'],
                    help='launches bracketed by HIP events INSIDE the timed region: conv = forward conv launches only '
                         '(what the roofline needs), all = every launch, none')
    ap.add_argument('--profile-run', action='store_true',
                    help='for runs under rocprofv3: only the warm-up and the timed steps (no per-family breakdown pass, no '
                         'kernel-exclusive pass), so the trace holds nothing but real training steps')
    ap.add_argument('--opt', default='', help='kernel experiment knobs, name=value,... (ssp_set_option); default: none')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed to DIR/<name>.npy (rank 0)')
    ap.add_argument('--full', action='store_true',
                    help='also the oracle check, the rooflines / per-kernel breakdown, the multi-rank diagnostics, the other '
                         'configurations and the CPU baseline (the --no-* / --timers / --profile-run options refine it)')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')

    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if args.gpus != world and world > 1:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))
    if args.gpus > 1 and world == 1:
        # `python bench.py --gpus N` without a launcher must never measure ONE rank and print it as N: start the N ranks here
        # (one process per GPU through torch.distributed.run, as the driver does) - or stop with a non-zero status
        have = torch.cuda.device_count()
        if have < args.gpus:
            raise SystemExit("bench.py --gpus %d: this node shows %d GPU(s); nothing measured (launch one rank per GPU: "
                             "tools/launch_dp.sh %d, or python -m torch.distributed.run --nnodes=1 --nproc-per-node %d "
                             "--master-addr 127.0.0.1 --master-port P bench.py --gpus %d ...)"
                             % (args.gpus, have, args.gpus, args.gpus, args.gpus))
        import socket
        sock = socket.socket()
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
        sock.close()
        os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
        sys.stdout.flush()
        # a child process, not exec: this process has already opened the GPU runtime (device_count above)
        import subprocess
        rc = subprocess.call([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
                              '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:])
        sys.exit(rc)
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)

    from singleshotpose_amd import _lib
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.dist import GradReducer, init_distributed
    from singleshotpose_amd.engine import weights_changed
    from singleshotpose_amd.optim import SGD
    from singleshotpose_amd.region_loss import RegionLoss

    # SSP_BENCH_FORCE_REDUCER=1: run the collective path (process group, bucketed all-reduce from the filter-gradient
    # stream, `comm` diagnostics) on ONE rank - a rehearsal of everything the N > 1 run does except the second GPU
    dist_on = world > 1 or os.environ.get('SSP_BENCH_FORCE_REDUCER') == '1'
    if dist_on:
        init_distributed()
    for kv in filter(None, args.opt.split(',')):
        name, val = kv.split('=')
        _lib.call('ssp_set_option', name.encode(), int(val))

    if not os.environ.get('SSP_TUNE_CACHE') and (args.cfg, args.batch, args.size) == (ap.get_default('cfg'), 64, 416):
        # the metric's workload runs a committed plan set (cfg/bench_tune_cache.json: what the autotuner timed on an MI355X
        # for exactly this workload): timing-based choices differ from run to run in the last bits of their sums.  A copy,
        # because the engine rewrites the file whenever it times a new shape.
        import shutil
        import tempfile
        import atexit
        tmp = tempfile.mkdtemp(prefix='ssp_bench_')
        atexit.register(shutil.rmtree, tmp, True)
        tc = os.path.join(tmp, 'tune_cache.json')
        shutil.copy(os.path.join(ROOT, 'cfg', 'bench_tune_cache.json'), tc)
        os.environ['SSP_TUNE_CACHE'] = tc
    torch.manual_seed(0)                       # identical initial weights on every rank
    model = Darknet(args.cfg).to(device).train()
    crit = RegionLoss()
    crit.verbose = False                        # status line (one host sync per step) off inside the timed region
    B, H, W = args.batch, args.size, args.size
    global_batch = B * world
    # the reference's sum-loss convention (train.py:45,388): lr / batch, decay * batch with the GLOBAL batch
    # torch.optim.SGD's update rule (train.py:388) as one fused launch over the flat parameter/gradient/momentum buffers
    opt = SGD(model.parameters(), lr=1e-3 / global_batch, momentum=0.9, dampening=0, weight_decay=0.0005 * global_batch)
    reducer = GradReducer(model, world, force=dist_on and world == 1)
    if world > 1:
        from singleshotpose_amd.dist import sync_plans
        sync_plans(model)        # every rank runs rank 0's plan set (same shape on every rank here: the broadcasts pair up)
    x, tgt = synthetic_batch(B, H, W, 1000 + rank, device)
    last_out = [None]
    # Every step trains from the SAME seeded weights: the dynamics of this randomly initialised network amplify the last-bit
    # differences of the filter gradients' fp32 atomics (~1e-6) to O(1) within ~20 SGD steps, so with evolving weights the
    # step a run ends on differs from run to run.  The optimizer's flat parameter buffer (it exists after the first
    # opt.step) is reset to the initial weights before each later step - one 202 MB device copy; momentum and the BatchNorm
    # running statistics carry over (they do not feed back into the gradients).
    init_params = [p.detach().clone() for p in model.parameters()]
    init_flat = [None]

    def step():
        if init_flat[0] is None and opt._flat_p is not None:
            with torch.no_grad():
                for p, p0 in zip(model.parameters(), init_params):
                    p.copy_(p0)
            init_flat[0] = opt._flat_p.clone()
            init_params.clear()
        elif init_flat[0] is not None:
            opt._flat_p.copy_(init_flat[0])
        if init_flat[0] is not None:
            weights_changed()                   # raw parameter memory changed: packed-filter caches must not be reused
        opt.zero_grad(set_to_none=True)
        out = model(x)
        loss = crit(out, tgt, 20)               # epoch 20 > pretrain: confidence term active
        loss.backward()
        reducer.all_reduce()                    # RCCL SUM over ranks (no-op for world 1)
        opt.step()
        last_out[0] = out.detach()
        return loss

    def barrier():
        if dist_on:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    grad_check = None
    if args.full and dist_on and os.environ.get('SSP_BENCH_SKIP_GRAD_CHECK') != '1':
        # SURVEY.md 8(d) config 3, untimed: every rank runs the SAME batch (same seed, same initial weights), once with the
        # reducer standing aside and once through it - the reduced flat gradient must be world x the local one (<= 1e-5 of
        # its range; the filter-gradient kernels' fp32 atomics make two evaluations differ in the last bits)
        try:
            x0, t0_ = synthetic_batch(B, H, W, 1000, device)
            reducer.enabled = False
            opt.zero_grad(set_to_none=True)
            crit(model(x0), t0_, 20).backward()
            plan_ = next(iter(model._plans.values()))
            local = plan_.last_flat_grad.clone()
            reducer.enabled = True
            for p_ in model._plans.values():
                p_.reducer = reducer if reducer.active else None
            opt.zero_grad(set_to_none=True)
            crit(model(x0), t0_, 20).backward()
            reducer.all_reduce()
            red_ = plan_.last_flat_grad
            err = float((red_ - world * local).abs().max() / local.abs().max().clamp_min(1e-30))
            errt = torch.tensor([err], dtype=torch.float64, device=device)
            if world > 1:
                torch.distributed.all_reduce(errt, op=torch.distributed.ReduceOp.MAX)
            grad_check = {"reduced_vs_world_x_local_rel": float(errt.item()), "bar": 1e-5, "ok": bool(errt.item() <= 1e-5),
                          "floats": int(local.numel())}
            # (reported, not asserted: a scaling run must not die on a diagnostic - `comm.grad_check.ok` says what happened)
            if not grad_check["ok"] and rank == 0:
                print("WARNING: reduced gradients differ from world x local gradients: %r" % (grad_check,), file=sys.stderr)
            opt.zero_grad(set_to_none=True)
            del x0, local
        except Exception as e:      # a diagnostic must never cost the scaling run its line
            reducer.enabled = True
            for p_ in model._plans.values():
                p_.reducer = reducer if reducer.active else None
            grad_check = {"error": repr(e)}

    verified, verify_detail = None, None
    if args.full and world == 1 and not args.no_verify:
        verified, verify_detail = verify_step(model, crit, B, H, W, 1000 + rank, exact=args.verify_exact)
    for _ in range(args.warmup):
        step()
    barrier()
    import ctypes
    nk = _lib.query('ssp_prof_nkinds')

    def collect():
        ms = (ctypes.c_double * nk)()
        work = (ctypes.c_double * nk)()
        cnt = (ctypes.c_int64 * nk)()
        _lib.call('ssp_prof_collect', ctypes.cast(ms, ctypes.c_void_p), ctypes.cast(work, ctypes.c_void_p),
                  ctypes.cast(cnt, ctypes.c_void_p))
        return list(ms), list(work), list(cnt)

    # Timed region: HIP events only around the FORWARD launches of the dominant kernel (what `roofline` needs; every
    # timed launch adds two event packets to its stream: all ~240 launches of a step timed cost 0.9 ms, these 23 cost
    # <0.1 ms).  --timers all / none change that.
    # (bit 0 = the forward conv launch units, bit 9 = the Winograd transform / finishing launches inside them: the dominant
    # kernel's own time is the difference; bit 12 = the on-chip Winograd forward launches, a family of their own)
    # The event pairs are SAMPLED: every 5th step of the timed region carries them (steps 0, 5, 10, ...; ~66 pairs per step
    # with the Winograd and on-chip families).  On every step they cost 0.37 ms of the step (same box: 25.20 / 25.22 ms with,
    # 24.82 / 24.86 ms without them; a plain loop without the profiler hooks 24.69 ms) - an instrument should not move the
    # number it sits next to.  `roofline.timed_steps` says how many steps the per-launch averages come from.
    # (a plain run carries none: nothing in its result line reads them)
    timer_mask = {'conv': (1 << 0) | (1 << 9) | (1 << 12), 'all': -1, 'none': 0}[args.timers] if args.full else 0
    n_timed = 0
    t0 = time.perf_counter()
    for i in range(args.steps):
        if timer_mask:
            on = (i % 5 == 0)
            _lib.call('ssp_prof_enable', timer_mask if on else 0)
            n_timed += 1 if on else 0
        loss = step()
    barrier()
    dt = time.perf_counter() - t0
    _lib.call('ssp_prof_enable', 0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, loss, last_out[0])
    n_timed = max(n_timed, 1)
    ms, work, cnt = collect()
    # Per-family breakdown (kernel_ms_per_step, roofline_bwd): a separate, untimed pass of the same steps with every
    # launch bracketed by events.
    # Collected step by step and reduced with the MEDIAN over steps: one stretched event (a clock ramp, another process
    # on the host) would otherwise add milliseconds to a family's mean.
    nb = min(args.steps, 5)
    no_passes = args.profile_run or not args.full
    per_step = []
    if no_passes:
        per_step = [([0.0] * nk, [0.0] * nk, [0] * nk)]
    for _ in range(0 if no_passes else nb):
        _lib.call('ssp_prof_enable', -1)
        loss = step()
        barrier()
        _lib.call('ssp_prof_enable', 0)
        per_step.append(collect())
    bms = [float(np.median([p[0][k] for p in per_step])) * nb for k in range(nk)]
    bwork = [float(np.median([p[1][k] for p in per_step])) * nb for k in range(nk)]
    bcnt = [float(np.median([p[2][k] for p in per_step])) * nb for k in range(nk)]
    # Kernel-exclusive durations of the BACKWARD conv families: the same steps once more with the filter gradients queued
    # on the main stream (Plan.serial_backward) - every launch then runs alone, as the forward launches always do, and its
    # HIP-event duration is the kernel's own (in the real step dgrad and wgrad share the CUs on two streams and stretch
    # each other's events: that pair is `roofline_bwd`).  Untimed, after the measurement; same operands, same plans.
    for plan in model._plans.values():
        plan.serial_backward = True
    ex_step = [([0.0] * nk, [0.0] * nk, [0] * nk)] if no_passes else []
    for _ in range(0 if no_passes else 3):
        _lib.call('ssp_prof_enable', (1 << 1) | (1 << 2) | (1 << 10) | (1 << 11) | (1 << 13) | (1 << 14))      # dgrad, wgrad, their Winograd passes, the on-chip forms
        loss = step()
        barrier()
        _lib.call('ssp_prof_enable', 0)
        ex_step.append(collect())
    for plan in model._plans.values():
        plan.serial_backward = False
    ex = {k: (float(np.median([p[0][k] for p in ex_step])), float(np.median([p[1][k] for p in ex_step])),
              float(np.median([p[2][k] for p in ex_step]))) for k in (1, 2, 10, 11, 13, 14)}
    if args.full and dist_on:
        # communication diagnostics (untimed): per-bucket all-reduce issue -> done times and the exposed tail of one step
        reducer.profile = True
        loss = step()
        barrier()
        reducer.profile = False
        comm = reducer.report()
        comm["grad_check"] = grad_check
        try:
            comm["rccl_version"] = '.'.join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            pass
    final_loss = float(loss.detach())

    tmax = torch.tensor([dt], dtype=torch.float64, device=device)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = float(tmax.item())
    images_per_s = global_batch * args.steps / dt
    headline = {
        "metric": "images/sec (fwd+bwd) yolo-pose 416x416 bs=64/GPU",
        "value": round(images_per_s, 2),
        "unit": "images/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "cfg/yolo-pose.cfg train step (zero_grad+fwd+RegionLoss+bwd+grad all-reduce+SGD), "
                               "%dx%d, batch %d/GPU, random-init weights, 1 label/image" % (H, W, B),
                   "global_batch": global_batch, "parallelism": "dp%d" % world},
        # headline fraction of the step: ALL conv FLOPs of fwd+bwd (87.673 GFLOP per image) over the whole step's
        # wall time - BatchNorm / activation / loss / optimizer time included in the denominator
        "step_conv_effective_flop_frac_of_peak": round(images_per_s / world * 87.673e9 / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
    }

    if rank == 0 and not args.full:
        res = dict(headline, final_loss=final_loss, head_budget=_budget_record(model))
    elif rank == 0:
        kinds = _lib.PROF_KINDS
        prof = {kinds[k]: {"ms_per_step": bms[k] / nb, "launches_per_step": bcnt[k] / nb,
                           "work_per_step": bwork[k] / nb} for k in range(nk)}
        # Dominant kernel family = the implicit-GEMM conv kernel.  Its FORWARD launches run alone on the GPU, so their
        # HIP-event durations are kernel-exclusive and are taken INSIDE the timed region.
        ig_ms, ig_flop, ig_n, ig_steps, ig_wino = ms[0], work[0], cnt[0], n_timed, ms[9]
        if ig_ms <= 0:      # --timers none: take the forward launches of the breakdown pass
            ig_ms, ig_flop, ig_n, ig_steps, ig_wino = bms[0], bwork[0], bcnt[0], nb, bms[9]
        achieved = ig_flop / (ig_ms * 1e-3) / 1e12 if ig_ms > 0 else 0.0
        # on-chip Winograd forward launches (kind 12): same source as the dominant kernel's
        oc_fwd = (ms[12] / n_timed, cnt[12] / n_timed) if ms[0] > 0 else (bms[12] / nb, bcnt[12] / nb)
        # the two streams run concurrently: wall time of the conv backward ~ the longer one (on-chip launches with their stream)
        bwd_ms = max(bms[1] + bms[13], bms[2] + bms[14])
        bwd_tf = (bwork[1] + bwork[2] + bwork[13] + bwork[14]) / (bwd_ms * 1e-3) / 1e12 if bwd_ms > 0 else 0.0
        traffic, traffic_src = forward_traffic_per_launch()

        # FLOP accounting.  ALGORITHMIC = direct convolution, 2*M*Cout*k*k*Cin (what images/s converts to).
        # EXECUTED = what the MFMA pipe really issued: a layer the autotuner runs in the Winograd F(n x n, 3x3) domain
        # (plan codes 9xxxxxx: n = 2, 8xxxxxx: n = 4; csrc/conv_wino.hip) multiplies (n+2)^2 GEMMs of tiles x Cin x Cout,
        # tiles = B * ceil(H/n) * ceil(W/n) - 16/36 resp. 36/144 of the direct multiplies, times the map's tile padding.
        # Every roofline object's `achieved` / `frac` is the EXECUTED rate (a fraction of the roofline it names, never > 1);
        # the algorithmic rate is reported next to it as `effective` (it can exceed the peak: fewer multiplies were needed).
        from singleshotpose_amd.engine import wino_fused, wino_tile
        plan0 = next(iter(model._plans.values()))
        alg = {'fwd': 0.0, 'dgrad': 0.0, 'wgrad': 0.0}
        exe = {'fwd': 0.0, 'dgrad': 0.0, 'wgrad': 0.0}      # executed FLOPs of the implicit-GEMM / filter-gradient kernel launches
        exe_oc = {'fwd': 0.0, 'dgrad': 0.0, 'wgrad': 0.0}   # ... of the on-chip Winograd launches (families of their own)
        alg_oc = {'fwd': 0.0, 'dgrad': 0.0, 'wgrad': 0.0}
        wino_layers = {f: {2: [], 4: []} for f in alg}
        fused_layers = {f: [] for f in alg}      # ... of the F(2x2) layers, the ones that run the on-chip kernel (wino2_fused_kernel)
        for ind, cs in sorted(plan0.convs.items()):
            if cs.first:
                continue
            direct = 2.0 * cs.M * cs.cout * cs.k * cs.k * cs.cin
            for fam, n in (('fwd', wino_tile(cs.plan_fwd)), ('dgrad', wino_tile(cs.plan_dgrad)),
                           ('wgrad', int(getattr(cs, 'wgrad_wino', 0) or 0))):
                alg[fam] += direct
                code = {'fwd': cs.plan_fwd, 'dgrad': cs.plan_dgrad}.get(fam, 0)
                if fam == 'wgrad' and n == 12:
                    # on-chip F(2x2) filter gradient (csrc/conv_wino_wgrad_fused.hip): 16 planes, two tiles per k-step
                    tiles = B * ((cs.H + 1) // 2) * 2 * (((cs.W + 1) // 2 + 1) // 2)
                    exe_oc[fam] += 2.0 * 16 * tiles * cs.cin * cs.cout
                    alg_oc[fam] += direct
                    wino_layers[fam][2].append(ind)
                    fused_layers[fam].append(ind)
                elif n and wino_fused(code):
                    # on-chip F(2x2) (csrc/conv_wino_fused.hip): 16 planes x 128 tile slots per patch block (the launch's
                    # statistics group) - partial patches at the map's edge multiply zeros like any tile padding
                    ci, co = (cs.cinp, cs.cout) if fam == 'fwd' else (cs.coutp, cs.cin)
                    tiles = 128 * _lib.query('ssp_conv_stats_tiles', B, cs.H, cs.W, ci, co, 3, code)
                    exe_oc[fam] += 2.0 * 16 * tiles * cs.cin * cs.cout
                    alg_oc[fam] += direct
                    wino_layers[fam][2].append(ind)
                    fused_layers[fam].append(ind)
                elif n:
                    tiles = _lib.query('ssp_conv_wino_tiles', B, cs.H, cs.W, n)      # (the 2 x 2 image mosaic included)
                    exe[fam] += 2.0 * (n + 2) ** 2 * tiles * cs.cin * cs.cout
                    wino_layers[fam][n].append(ind)
                else:
                    exe[fam] += direct
        IGEMM = ("conv_igemm_dma_kernel<BM, BN, %d, NSLOT, WM, WN>(ConvArgs) - the instantiations rocprof lists for this "
                 "workload: <64, 128, %d, 3|4, 2, 2> (batched Winograd GEMMs and mid-size grids), <128, 128, %d, 3, 2, 2>, "
                 "<128, 64, %d, 3, 2, 2> (Cout <= 64), <256, 32, %d, 4, 4, 1> (Cout <= 32)")

        def family(fam, kernel, ms_, n_, note, wino_ms, oc_ms=0.0):
            """MFMA roofline object of one conv family.  The DOMINANT KERNEL is the implicit-GEMM / filter-gradient MFMA
            kernel itself: achieved = EXECUTED FLOPs / the HIP-event time of its launches (= the launch units' time minus the
            HBM-bound Winograd transform / finishing launches inside them, which have their own roofline object).  The same
            FLOPs over the whole units - transforms included - are `launch_units`."""
            gemm_ms = ms_ - (wino_ms or 0.0)
            tf = exe[fam] / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
            utf = exe[fam] / (ms_ * 1e-3) / 1e12 if ms_ > 0 else 0.0
            eff = alg[fam] / ((ms_ + oc_ms) * 1e-3) / 1e12 if ms_ + oc_ms > 0 else 0.0      # every layer of the pass, on-chip launches included
            return {"bound": "mfma", "kernel": kernel, "achieved": round(tf, 2), "peak": PEAK_FP32_MFMA_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(tf / PEAK_FP32_MFMA_TFLOPS, 4),
                    "flop_per_step": exe[fam], "ms_per_step": round(gemm_ms, 3), "launches_per_step": n_,
                    "avg_launch_ms": round(gemm_ms / max(n_, 1), 4),
                    "launch_units": {"achieved": round(utf, 2), "frac": round(utf / PEAK_FP32_MFMA_TFLOPS, 4),
                                     "ms_per_step": round(ms_, 3),
                                     "note": "the same executed FLOPs / the time of the whole launch units: a Winograd layer's "
                                             "input transform, batched GEMM and finishing launches together (the HBM-bound "
                                             "passes charged to the matrix pipe)"},
                    "effective": {"tflops": round(eff, 2), "frac_of_peak": round(eff / PEAK_FP32_MFMA_TFLOPS, 4),
                                  "flop_per_step": alg[fam],
                                  "note": "ALGORITHMIC (direct-convolution) FLOPs / the launch units' time: not a roofline "
                                          "fraction - Winograd layers need fewer multiplies than it counts"},
                    "winograd_layers": {"F(2x2,3x3)": wino_layers[fam][2], "F(4x4,3x3)": wino_layers[fam][4],
                                        "of F(2x2): on-chip (wino2_fused_kernel<FLAGS>: one persistent launch, no transform passes)": fused_layers[fam]},
                    "note": note}

        def hbm_family(fam, ms_, bytes_, n_):
            """HBM roofline object of the Winograd transform / finishing passes of one conv family."""
            gbs = bytes_ / (ms_ * 1e-3) / 1e9 if ms_ > 0 else 0.0
            return {"family": fam, "achieved": round(gbs, 1), "frac": round(gbs / PEAK_HBM_GBS, 4), "ms_per_step": round(ms_, 3),
                    "bytes_per_step": bytes_, "launches_per_step": n_}

        wk = {'fwd': 9, 'dgrad': 10, 'wgrad': 11}
        wino_traffic, wino_traffic_src = wino_traffic_per_step()
        # (forward passes: from the timed region itself when its timers are on, else from the untimed all-timers pass)
        fw = (ms[9] / n_timed, work[9] / n_timed, cnt[9] / n_timed) if ms[0] > 0 else (bms[9] / nb, bwork[9] / nb, bcnt[9] / nb)
        hb = [hbm_family('fwd', *fw), hbm_family('dgrad', *ex[10]),
              hbm_family('wgrad', *ex[11])]
        hb_ms = sum(h["ms_per_step"] for h in hb)
        hb_bytes = sum(h["bytes_per_step"] for h in hb)
        step_exec = sum(exe.values()) + sum(exe_oc.values()) + 4 * 2.0 * B * H * W * 32 * 27
        res = dict(headline, **{
            # the FLOPs the MFMA pipe really issued in a step (Winograd layers counted as their GEMMs; the first block's
            # four recomputing passes included) over the step's wall time: whole-step pipe utilisation
            "step_mfma_executed_frac_of_peak": round(step_exec / (dt / args.steps) / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
            "roofline": dict(family("fwd", IGEMM % (0, 0, 0, 0, 0) + "; the forward launch units of layers 2-30 (the first block's "
                                    "two passes are first_block_kernel<0|1>: kernel_ms_per_step.first_block_fwd)",
                                    ig_ms / max(ig_steps, 1), ig_n / max(ig_steps, 1),
                                    "HIP events around exactly these launches INSIDE the timed region, on every 5th step "
                                    "(timed_steps; they run alone on the GPU): one pair per launch unit and one per Winograd "
                                    "transform / finishing launch inside it; "
                                    "achieved / frac = EXECUTED MFMA FLOPs / the GEMM launches' own time",
                                    ig_wino / max(ig_steps, 1), oc_fwd[0]),
                             traffic=traffic, traffic_source=traffic_src, timed_steps=ig_steps),
            "roofline_dgrad": family("dgrad", IGEMM % (1, 1, 1, 1, 1) + " (+ conv_igemm_kernel<64, 128, 2, 2, 4, 0, 1> for the "
                                     "20-channel head)", ex[1][0], ex[1][2],
                                     "kernel-exclusive: untimed pass with the filter gradients on the same stream "
                                     "(Plan.serial_backward); includes the fused BatchNorm-backward epilogues", ex[10][0], ex[13][0]),
            "roofline_wgrad": family("wgrad", "conv_wgrad_dma_kernel<BMO, BNI, NSLOT, FOLD, BVEC>(WgradArgs): <256, 128, 3, false, "
                                     "false>, <128, 128, 3, ...>, <128, 64, 4, ...>, <64, 128, 4, ...>, <64, 64, 4, true, false>",
                                     ex[2][0], ex[2][2], "kernel-exclusive: untimed pass with the filter gradients on the same "
                                     "stream (Plan.serial_backward); the first layer's filter gradient is first_block_kernel<3> "
                                     "(kernel_ms_per_step.first_block_bwd)", ex[11][0], ex[14][0]),
            # the on-chip Winograd F(2x2) kernels (round 6): persistent launches that keep V and M in registers / LDS - their own
            # families, so that `roofline` stays the implicit-GEMM kernel's launches and nothing else
            "roofline_onchip": {
                "bound": "mfma",
                "kernel": "wino2_fused_kernel<FLAGS> (csrc/conv_wino_fused.hip: forward and data gradient), wino2_wgrad_fused_kernel "
                          "(csrc/conv_wino_wgrad_fused.hip: filter gradient)",
                "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                "by_pass": {f: {"layers": fused_layers[f], "ms_per_step": round(m_, 3), "launches_per_step": n_,
                                "achieved": round(exe_oc[f] / (m_ * 1e-3) / 1e12 if m_ > 0 else 0.0, 2),
                                "frac": round(exe_oc[f] / (m_ * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS if m_ > 0 else 0.0, 4),
                                "flop_per_step": exe_oc[f],
                                "effective_tflops": round(alg_oc[f] / (m_ * 1e-3) / 1e12 if m_ > 0 else 0.0, 2)}
                            for f, (m_, n_) in (('fwd', oc_fwd), ('dgrad', (ex[13][0], ex[13][2])), ('wgrad', (ex[14][0], ex[14][2])))},
                "note": "achieved / frac = EXECUTED MFMA FLOPs (16 planes x 128 tile slots per patch block; 16/36 of the direct "
                        "multiplies) / HIP-event time of the launches - forward inside the timed region, backward kernel-exclusive "
                        "(Plan.serial_backward); effective_tflops = the layers' ALGORITHMIC FLOPs over the same time.  The input / "
                        "output-gradient transforms run on the SIMD's vector lanes inside these kernels (the fp32 MFMA shares them), "
                        "which is why the executed fraction is lower than the implicit-GEMM kernel's while the launches are faster "
                        "than the direct and the through-HBM Winograd forms of the same layers"},
            "roofline_bwd": {"bound": "mfma", "kernel": "in the real step: conv dgrad launch units (main stream) overlapped with "
                                                        "conv_wgrad_dma_kernel launch units (second stream)",
                             "achieved": round((exe['dgrad'] + exe['wgrad'] + exe_oc['dgrad'] + exe_oc['wgrad']) / (bwd_ms / nb * 1e-3) / 1e12 if bwd_ms > 0 else 0.0, 2),
                             "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                             "frac": round((exe['dgrad'] + exe['wgrad'] + exe_oc['dgrad'] + exe_oc['wgrad']) / (bwd_ms / nb * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS
                                           if bwd_ms > 0 else 0.0, 4),
                             "effective": {"tflops": round(bwd_tf, 2), "frac_of_peak": round(bwd_tf / PEAK_FP32_MFMA_TFLOPS, 4)},
                             "note": "EXECUTED dgrad+wgrad FLOPs / max(sum of dgrad event times, sum of wgrad event times); "
                                     "from a separate untimed pass with every launch timed, as kernel_ms_per_step"},
            # the HBM-bound passes around the Winograd GEMMs: input / output-gradient transforms, finishing passes (inverse
            # transform + statistics / affine / fused BatchNorm-backward sums), filter-gradient finishing
            "roofline_wino_transforms": {
                "bound": "hbm",
                "kernel": "wino_input_kernel<2, 4>|<4, 2>, wino_output_kernel<2>|<4>, wino_outgrad_kernel<2, 4>|<4, 2>, "
                          "wino_wgrad_finish_kernel<2>|<4> (conv_wino.hip)",
                "achieved": round(hb_bytes / (hb_ms * 1e-3) / 1e9 if hb_ms > 0 else 0.0, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": round(hb_bytes / (hb_ms * 1e-3) / 1e9 / PEAK_HBM_GBS if hb_ms > 0 else 0.0, 4),
                "ms_per_step": round(hb_ms, 3), "bytes_per_step": hb_bytes, "by_family": hb,
                "traffic": wino_traffic, "traffic_source": wino_traffic_src,
                "note": "achieved = ALGORITHMIC bytes of these passes (each operand read once, each result written once) / their "
                        "HIP-event time: forward passes inside the timed region (they run alone), backward ones "
                        "kernel-exclusive in an untimed pass (Plan.serial_backward); traffic = fabric bytes per step of the same kernels from the "
                        "committed PMC passes (FETCH_SIZE x2 + WRITE_SIZE), null while the kernels differ from the profiled ones"},
            "kernel_ms_per_step": {k: round(v["ms_per_step"], 3) for k, v in prof.items()},
            "final_loss": final_loss,
            "verified": verified,
            "verify": verify_detail,
            # error-aware admission of the forward plans (engine.Plan._apply_head_budget): head deviation of every Winograd
            # candidate measured on the first batch, the layers that were moved to a more accurate family to keep the
            # budget, and the launch time that cost
            "head_budget": _budget_record(model),
        })
        if dist_on:
            res["comm"] = comm
        if world == 1 and not args.no_extras:
            del opt, x
            model._plans.clear()
            torch.cuda.empty_cache()
            res["extra"] = extras(device)
            res["extra"].update(multiscale_extras(device))
        if world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(args.cfg, args.cpu_batch, H, W)
    else:
        res = None
    if dist_on:
        torch.distributed.destroy_process_group()
    if res is not None:
        # ONE JSON line, and the LAST line of stdout: RCCL writes its version banner through C stdio, which would otherwise
        # flush at exit - after this line
        import ctypes
        sys.stdout.flush()
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

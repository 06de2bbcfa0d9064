"""Which kernel variant every convolution launch of a plan runs: plan codes, the tune state shared by every plan of the
process, the environment knobs, and the passes that time and verify the candidates (tune_convs, tune_wgrad) on an engine.Plan
and its _ConvSpec records `cs`.  engine.py imports this module and re-exports its names; nothing here imports engine.
Each rule is stated once: knobs() reads the environment, wino_forms() / form_allowed() are eligibility, *_candidates() list what
is timed, time_launch() times, select() (beats, credited) decides, a Probe holds a layer's launches, admit() verifies."""
import collections
import json
import os
import warnings

import torch

from . import _lib

WINO = 9000000       # plan codes WINO + tile_rows*100 + 10 + ring_slots: Winograd F(2x2, 3x3) evaluation (csrc/conv_wino.hip)
WINO4 = 8000000      # ... and WINO4 + the same: F(4x4, 3x3)
WGRAD_FUSED = 12     # `tile` value of ssp_conv_wgrad_wino_t: F(2x2) filter gradient with both transforms on the chip
WINOF = 7000001      # F(2x2, 3x3) with the transform domain kept on the chip (csrc/conv_wino_fused.hip): one persistent launch,
                     # no workspace; same transformed filters, same arithmetic (and error family) as a WINO plan
# Direct plan codes tune_convs times (include/ssp_hip.h: tail*100000 + tile_rows*100 + ksplit*10 + ring_slots): tile
# rows x split-K x ring depth; 2xxxxx / 3xxxxx / 4xxxxx = hybrid launches (whole resident waves un-split, the tiles of the
# last partial wave split 2 / 3 / 4 ways over K)
IGEMM_CANDS = (12813, 12814, 6414, 6413, 12824, 12834, 306413, 306414, 312813, 312814, 206413, 212814,
               12823, 6423, 6424, 206414, 212813, 406413, 406414, 412813)
# ring depth 8 = the latency form (one workgroup per CU, 7 chunks in flight): for grids that give a CU one workgroup anyway
IGEMM_LATENCY_CANDS = (6418, 12818, 6428, 12828, 6438)
# GEMM tilings tried under a Winograd base (WINO / WINO4 + code)
WINO_GEMM_CANDS = (6413, 6414, 12813, 12814)
# bf16x3 fast mode of the direct kernel (csrc/conv_igemm_bf16x3.hip): plan codes BF16X3 + tile_rows*100 + ksplit*10 + 3.
# Opt-in (SSP_CONV_MATH=bf16x3 / Darknet.conv_math); with the mode off no such code is ever timed, cached or run.
BF16X3 = 6000000
# ... and of the batched GEMM of a through-memory Winograd plan: the plan's code + X3_WINO with GEMM code tile_rows*100 + 13
# (8612813, 9606413, ...: its "twin").  Only under SSP_CONV_MATH=bf16x3-wino, which is 'bf16x3' plus these.
X3_WINO = 600000
X3_WINO_GEMM_CANDS = (12813, 6413)
CONV_MATHS = ('fp32', 'bf16x3', 'bf16x3-wino')
BN_EPS = 1e-4        # darknet.py:157
BN_MOMENTUM = 0.1    # nn.BatchNorm2d default
NEAR_TIE = 0.985     # a later candidate must be this much faster than the best so far: near-ties go to the earlier (simpler) one


def x3_wino(code):
    """True for the twin codes: a through-memory Winograd plan (8xxxxxx / 9xxxxxx) with its GEMM on the bf16 matrix cores."""
    return 8000000 <= code < 10000000 and (code // 100000) % 10 == 6


def conv_math_of(code):
    """'bf16x3' for a 6xxxxxx plan code and for a Winograd twin code (x3_wino tells the two families apart), 'fp32' for every
    other (direct and Winograd) code."""
    return 'bf16x3' if BF16X3 <= code < BF16X3 + 1000000 or x3_wino(code) else 'fp32'


def x3_wino_twins(code):
    """The twin codes of a through-memory fp32 Winograd code, tile rows 128 then 64; () for every other code."""
    if not wino_tile(code) or wino_fused(code) or (code // 100000) % 10:
        return ()
    return tuple(code - code % 100000 + X3_WINO + c for c in X3_WINO_GEMM_CANDS)


def conv_math_env():
    """SSP_CONV_MATH: 'fp32' (default, also when unset or empty), 'bf16x3' or 'bf16x3-wino'."""
    mode = os.environ.get('SSP_CONV_MATH', '') or 'fp32'
    if mode not in CONV_MATHS:
        raise ValueError("SSP_CONV_MATH=%r: expected one of %s" % (mode, ', '.join(CONV_MATHS)))
    return mode


def wino_fused(code):
    """True for the on-chip F(2x2) plan codes (7xxxxxx)."""
    return 7000000 <= code < 8000000


def wino_tile(code):
    """Output-tile edge of a plan code: 2 / 4 for a Winograd plan, 0 for a direct one (ssp_conv_plan_wino_tile).  The on-chip
    F(2x2) codes count as tile 2: same filter transform, same error family."""
    return 2 if (WINO <= code < WINO + 1000000 or wino_fused(code)) else (4 if WINO4 <= code < WINO4 + 1000000 else 0)


def _pad4(c):
    return (c + 3) // 4 * 4


# ---------------------------------------------------------------------- tune state, shared by every Plan of the process
# (engine re-exports these objects; bench.py and the tests mutate them in place: never rebind one, clear() / update() only)
# autotuned igemm plan per launch shape: multi-scale training (dataset.py:66-90 draws a new resolution every 10 batches)
# revisits the same ~20 shapes, each is timed once
_TUNE_CACHE = {}
# ... and per FAMILY of that launch (0 = direct kernels, 2 / 4 = Winograd F(2x2) / F(4x4)): launch shape -> {family: (fastest code
# of the family, its time in ms)} - what the error budget of the forward plans chooses from (Plan._apply_head_budget)
_TUNE_FAMILY = {}
_HEAD_BUDGET_CACHE = {}        # (plan shape, tag, budget, model) -> record: a rebuilt plan re-measures nothing
_HEAD_BUDGET_PINNED = {}       # (plan shape, tag, budget) -> {layer: forward plan code}: decisions read from / written to the
                               # SSP_TUNE_CACHE file - a process started with that file runs the SAME plan set without measuring
                               # (profiled runs hold training steps only; multi-process jobs can share one file)
_TUNE_VERIFIED = {}            # launch shape -> the plan code(s) that passed verify-after-tune in this process
_TUNE_VERIFIED_ALSO = set()    # (launch shape, code) pairs verified besides the chosen one (the other families' fastest codes)
TUNE_REJECTED = []             # (shape key, plan code) pairs verify-after-tune refused
_TUNE_CACHE_FILE = [None]      # SSP_TUNE_CACHE=<json file>: loaded once, rewritten whenever a new shape was timed


def _tune_cache_load():
    path = os.environ.get('SSP_TUNE_CACHE')
    if not path or _TUNE_CACHE_FILE[0] == path:
        return
    _TUNE_CACHE_FILE[0] = path
    if os.path.isfile(path):
        with open(path) as f:
            for k, v in json.load(f).items():
                if k.startswith('fam|'):
                    _TUNE_FAMILY.setdefault(tuple(json.loads(k[4:])), {int(f_): (int(c), t) for f_, (c, t) in v.items()})
                elif k.startswith('budget|'):      # a pinned error-budget decision (layer -> forward code) of a plan shape
                    _HEAD_BUDGET_PINNED.setdefault(tuple(json.loads(k[7:])), {int(i): int(c) for i, c in v.items()})
                else:
                    _TUNE_CACHE.setdefault(tuple(json.loads(k)), int(v))


def _tune_cache_save():
    path = _TUNE_CACHE_FILE[0]
    if path:
        tmp = path + '.tmp.%d' % os.getpid()
        with open(tmp, 'w') as f:
            out = {json.dumps(list(k)): v for k, v in _TUNE_CACHE.items()}
            out.update({'fam|' + json.dumps(list(k)): {str(f_): [c, t] for f_, (c, t) in v.items()} for k, v in _TUNE_FAMILY.items()})
            out.update({'budget|' + json.dumps(list(k)): {str(i): c for i, c in v.items()} for k, v in _HEAD_BUDGET_PINNED.items()})
            json.dump(out, f, indent=0, sort_keys=True)
        os.replace(tmp, path)


def _finish_pass(n_known):
    """End of a pass: the cache file follows what was timed; the timing / verification scratch goes back to the driver (left
    in the caching allocator it sits reserved next to the plan's own buffers: multi-scale soak)."""
    torch.cuda.synchronize()
    if len(_TUNE_CACHE) != n_known:
        _tune_cache_save()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------- the environment knobs
Knobs = collections.namedtuple('Knobs', 'autotune verify wino_on tiles min2 min4 fused_on credit_ms wgrad_credit dgrad_credit head_budget tag '
                                         'deterministic')


def knobs():
    """The tuner's environment, read in this one place at the start of every tuning pass (never at import: tests and A/B
    scripts change it between plan builds).  SSP_AUTOTUNE=0: no timing, the library's heuristic plans run; SSP_TUNE_VERIFY=0: no
    verify-after-tune; SSP_WINOGRAD=0: no Winograd form; SSP_WINO_TILES (2,4): the tile sizes tried, =2 or =4 restricts them;
    SSP_WINO_FUSED=0: no on-chip F(2x2) form (WINOF, WGRAD_FUSED); the credits: see credited(); head_budget: SSP_HEAD_ERR_BUDGET.
    min2 / min4 = SSP_WINO_MIN_CHANNELS (128) / SSP_WINO4_MIN_CHANNELS (64), the channels on both sides from which F(2x2) /
    F(4x4) are timed: F(2x2) is 16/36 of the multiplies at the price of two HBM-bound transform passes, and with 64 channels the
    tuner never picked one - the transforms of the wide maps cost more than the short-K GEMMs save (measured,
    profiles/r03_step_ab_winograd.txt); F(4x4) is 36/144 of the multiplies and 2.25 instead of 4 transform floats per pixel.
    tag = the candidate-set tag, part of every tune-cache key: a cache entry written before a family of candidates existed, or
    in a process that had it switched off, must not keep that family from ever being timed - and must not hand a Winograd code
    to a process that switched it off.  It spells the knobs as the environment does (an unset credit as ''): the keys of
    cfg/bench_tune_cache.json carry it.
    deterministic = SSP_DETERMINISTIC (unset, '0' or '1'; anything else is a ValueError): the bitwise-reproducible training
    mode (engine.Plan.deterministic).  NOT part of the tag: the mode changes no forward or data-gradient
    candidate, and its filter-gradient decisions live under keys of their own (det_key)."""
    env = os.environ.get
    det = env('SSP_DETERMINISTIC', '')
    if det not in ('', '0', '1'):
        raise ValueError("SSP_DETERMINISTIC=%r: expected unset, 0 or 1" % det)
    wino_on = env('SSP_WINOGRAD', '1') != '0'
    tiles, min2, min4, fused = env('SSP_WINO_TILES', '2,4'), env('SSP_WINO_MIN_CHANNELS', '128'), \
        env('SSP_WINO4_MIN_CHANNELS', '64'), env('SSP_WINO_FUSED', '1')
    tag = 'r5-direct' if not wino_on else 'r6-w%s-c%s-%s-f%s' % (
        tiles, min2, min4, fused + env('SSP_WGRAD_FUSED_PREFER', '') + env('SSP_ONCHIP_PREFER', '') + env('SSP_ONCHIP_CREDIT_MS', ''))
    return Knobs(autotune=env('SSP_AUTOTUNE', '1') != '0', verify=env('SSP_TUNE_VERIFY', '1') != '0', wino_on=wino_on,
                 tiles=tuple(int(t) for t in tiles.split(',') if t), min2=int(min2), min4=int(min4), fused_on=fused != '0',
                 credit_ms=float(env('SSP_ONCHIP_CREDIT_MS', '0.25')), wgrad_credit=float(env('SSP_WGRAD_FUSED_PREFER', '0.8')),
                 dgrad_credit=float(env('SSP_ONCHIP_PREFER', '0.85')), head_budget=float(env('SSP_HEAD_ERR_BUDGET', '3.5e-5')),
                 tag=tag, deterministic=det == '1')


def _tune_tag():
    return knobs().tag


def form_allowed(kn, tile, onchip=False):
    """Whether this process may run a launch of Winograd tile `tile` (0 = direct: always): the check of an adopted or cached code."""
    return not tile or (kn.wino_on and tile in kn.tiles and (kn.fused_on or not onchip))


def wino_forms(kn, cs, B, min_channels=0, min_tiles=0, halo_rows=0):
    """(tile sizes, on-chip) of the Winograd forms that may be timed on a launch of this layer: a stride-1 3x3 layer behind
    the first block, no channel padding, channels multiples of 16; a tile size from its channel floor (knobs) on both sides;
    the on-chip F(2x2) kernels at 32-channel granularity while every byte offset of the maps stays below 2^31.  Forward and data
    gradient take the defaults; the filter gradient asks min_channels=64 and min_tiles=16 (B * ceil(H/t) * ceil(W/t)) of its
    through-memory forms, and its on-chip form (csrc/conv_wino_wgrad_fused.hip) reads halo_rows = W + 1 pixels past the map."""
    if not (kn.wino_on and cs.k == 3 and cs.stride == 1 and not cs.first and not cs.depthwise and cs.cinp == cs.cin and cs.coutp == cs.cout and
            cs.cin % 16 == 0 and cs.cout % 16 == 0):
        return (), False
    cmin = min(cs.cin, cs.cout)
    tiles = tuple(t for t in (2, 4) if t in kn.tiles and cmin >= max(min_channels, kn.min2 if t == 2 else kn.min4) and
                  B * ((cs.H + t - 1) // t) * ((cs.W + t - 1) // t) >= min_tiles)
    onchip = (kn.fused_on and 2 in kn.tiles and cs.cin % 32 == 0 and cs.cout % 32 == 0 and
              (B * cs.H * cs.W + halo_rows) * max(cs.inp.ld, cs.ldraw) * 4 < (1 << 31))
    return tiles, onchip


# ---------------------------------------------------------------------- candidates (pure: shape fields, knobs, host queries)
def direct_candidates(mn, thin):
    """Direct plan codes timed on a launch writing mn = M * N floats.  thin (N <= 64): the launch ignores plan codes, its
    heuristic plan alone is timed against the Winograd forms.  Small-batch inference (valid.py runs B = 1): a few dozen tiles
    cannot stream the filters at HBM speed, `deep` K splits put every CU on the weight stream.  The biggest maps get no split-K."""
    deep = tuple(bm * 100 + ks * 10 + sl for bm in (64, 128) for ks in (4, 5, 6, 8, 9) for sl in (3, 4, 8)) if mn <= (1 << 21) else ()
    codes = (0,) if thin else IGEMM_CANDS + (IGEMM_LATENCY_CANDS if mn <= (1 << 23) else ()) + deep
    if mn > (1 << 25):
        codes = tuple(c for c in codes if not ((c // 10) % 10 > 1 or c >= 100000))
    return codes


def wino_candidates(kn, cs, B, small=False):
    """Winograd plan codes timed on a forward / data-gradient launch: every GEMM tiling under each eligible base, on small
    grids (batch-1 inference) also the 8-slot latency ring, as for the direct plans; then the on-chip form."""
    tiles, onchip = wino_forms(kn, cs, B)
    codes = []
    for t in tiles:
        base = WINO if t == 2 else WINO4
        codes += [base + c for c in WINO_GEMM_CANDS] + ([base + 6418, base + 12818] if small else [])
    return tuple(codes) + ((WINOF,) if onchip else ())


def conv_candidates(kn, cs, B, which):
    """(direct codes, Winograd codes) timed for the 'fwd' / 'dgrad' launch of a layer, in that order; None when the launch is
    not tuned: a thin launch is tuned only against a Winograd form (forward: the on-chip one)."""
    if which == 'fwd':
        wc = wino_candidates(kn, cs, B, cs.M * cs.coutp <= (1 << 23))
        return (direct_candidates(cs.M * cs.coutp, cs.cout <= 64), wc) if cs.cout > 64 or WINOF in wc else None
    if cs.first or cs.coutp % 16:
        return None
    wc = wino_candidates(kn, cs, B)
    return (direct_candidates(cs.M * cs.cinp, cs.cin <= 64), wc) if cs.cin > 64 or wc else None


def x3_candidates(cs, B, K, N):
    """bf16x3 codes timed against the fp32 code of a K -> N launch: tile rows 128 / 64 x the split depths the direct list
    tries at this grid size, those the kernel fits."""
    mn = cs.M * _pad4(N)
    splits = (1,) if mn > (1 << 25) else (1, 2, 3) + ((4, 5, 6, 8, 9) if mn <= (1 << 21) else ())
    codes = [BF16X3 + bm * 100 + ks * 10 + 3 for bm in (128, 64) for ks in splits]
    return tuple(c for c in codes if _lib.query('ssp_conv_bf16x3_fits', B, cs.H, cs.W, K, N, cs.k, c))


def wgrad_candidates(kn, cs, B, deterministic=False):
    """Winograd forms of the filter gradient timed against the direct kernel (`tile` values of ssp_conv_wgrad_wino_t).
    deterministic: the ordered forms (ssp_conv_wgrad_wino_ordered) - tiles 2 and 4; the on-chip form finishes with atomics
    and has no ordered counterpart, its layers fall to tile 2 / 4 or the direct kernel."""
    tiles, onchip = wino_forms(kn, cs, B, min_channels=64, min_tiles=16, halo_rows=cs.W + 1)
    return tiles + ((WGRAD_FUSED,) if onchip and not deterministic else ())


def fwd_key(plan, cs):
    return ('fwd', plan.B, cs.H, cs.W, cs.cinp, cs.cout, cs.k, cs.inp.ld, cs.ldraw, bool(cs.bn), _tune_tag())


def x3_key(key):
    """The bf16x3 decision of a launch has a key of its own: nothing of the fp32 passes reads it."""
    return (key[0] + '-bf16x3',) + key[1:]


def x3_wino_key(key, tile):
    """... and so has the twin decision of a launch, per Winograd tile (a forward launch may be moved between the families by
    the head budget: each family's decision is made, and kept, on its own)."""
    return (key[0] + '-bf16x3-wino',) + key[1:] + (tile,)


def det_key(key):
    """The deterministic mode's decision of a launch has a key of its own ('wgrad-det', ...): its candidates and kernels are
    not those of the mode-off decision, and neither reads the other's entry."""
    return (key[0] + '-det',) + key[1:]


def time_launch(launch, repeats):
    """Warm once, time `repeats` launches with HIP events, the best in ms; None when the library refuses the launch."""
    try:
        launch()
        ts = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return min(ts)
    except _lib.SspError:
        return None


def credited(kn, kind, code, ms):
    """The on-chip credit of a data-gradient (WINOF) or filter-gradient (WGRAD_FUSED) launch.  Data gradient: ONE launch against the three of a through-HBM Winograd plan (transform, GEMM, finishing pass), and in the
    step those run next to the filter-gradient stream: measured alone the two forms are within noise of each other on the
    104 x 104 layers (0.50-0.61 against 0.64 ms), in the step the on-chip form is the faster one (three layers on it: 25.8 ms;
    one: 26.4 ms - a box whose timings fell the other way).  SSP_ONCHIP_PREFER (default 0.85) credits it accordingly; 1 = the
    isolated timing decides.
    Filter gradient: timed alone, the HBM-bound transform passes of the other Winograd forms run at full bandwidth; in the step
    they share it with the data-gradient stream.  SSP_WGRAD_FUSED_PREFER (default 0.8) credits the on-chip form (no such
    passes) with that difference: same-box A/B of the whole step, two interleaved rounds, 26.64 / 26.45 ms with 1.0 (layers
    4 / 6 stay on the F(4x4) chain) against 26.12 / 26.13 ms with 0.8 (profiles/r06_step_ab.txt).
    Big launches only (>= SSP_ONCHIP_CREDIT_MS, 0.25 ms alone): at batch 8 the on-chip launches are 0.15 ms of mostly fixed
    cost (1024 waves x 144 atomics of flush) and the credit picked them for eight layers - 6.49 / 6.48 ms per step against
    6.33 / 6.32 without it (same box)."""
    factor = kn.dgrad_credit if kind == 'dgrad' and wino_fused(code) else (
        kn.wgrad_credit if kind == 'wgrad' and code == WGRAD_FUSED else None)
    return ms * factor if factor is not None and ms >= kn.credit_ms else ms


def beats(ms, best_ms):
    """A candidate replaces the best so far only when it is clearly faster: near-ties go to the earlier (simpler) one."""
    return best_ms is None or ms < best_ms * NEAR_TIE


def select(kn, kind, timed):
    """From [(code, ms or None)] in candidate order: (winner, {family: (fastest code of the family, its ms)}), families
    being 0 (direct) and the Winograd tiles 2 / 4.  Winner 0 when nothing could be timed."""
    best, best_ms, fams = 0, None, {}
    for code, ms in ((c, credited(kn, kind, c, t)) for c, t in timed if t is not None):
        if beats(ms, best_ms):
            best, best_ms = code, ms
        f = wino_tile(code)
        if beats(ms, fams[f][1] if f in fams else None):
            fams[f] = (code, ms)
    return best, fams


def pick(kn, key, probe, direct, wino):
    """The code of launch shape `key`: the cached one, else the fastest of direct + wino (timed now, cached per family)."""
    keep = True
    if key in _TUNE_CACHE:       # the same launch shape was timed before (another plan, another model)
        if not wino_tile(_TUNE_CACHE[key]) or _TUNE_CACHE[key] in wino:
            return _TUNE_CACHE[key]
        keep = False             # a cached Winograd choice whose family is off in this process: time the rest, leave the entry
    for t in sorted(set(wino_tile(c) for c in wino)) if keep else ():
        probe.prep(t)
    best, fams = select(kn, key[0], [(code, time_launch(lambda: probe.launch(code), 2)) for code in direct + wino])
    if keep:
        _TUNE_CACHE[key] = best
        _TUNE_FAMILY[key] = fams
    return best


# ---------------------------------------------------------------------- probes: the launches of one layer on the plan's buffers
# launch(code); out_of() -> its output; operands = what admit() randomises (tensors, or (tensor, ld, first column, columns));
# bn_of(code) -> [mean, 1/std] from the launch's BatchNorm partials, or None; prep(tile) transforms the filters for a Winograd code
Probe = collections.namedtuple('Probe', 'launch out_of operands bn_of prep')
Scratch = collections.namedtuple('Scratch', 'ws ws_floats stats gscratch stream gen')


def fwd_probe(plan, cs, sc):
    B, call, st = plan.B, _lib.call, sc.stream
    # operand contents are irrelevant for timing: a channels-last-sized parameter stands in for itself
    wop = cs.conv.weight if cs.cinp == cs.cin else plan._wbuf(cs)

    def prep(tile):
        call('ssp_wino_filter_transform_t', wop.data_ptr(), plan._wino_u(cs, tile).data_ptr(), cs.cout, cs.cinp, tile, st)

    def launch(code):
        wt = plan._wino_u(cs, wino_tile(code)) if wino_tile(code) else wop
        call('ssp_conv_fwd', cs.inp.ptr, wt.data_ptr(), cs.raw.data_ptr(), None, sc.stats.data_ptr() if cs.bn else None,
             B, cs.H, cs.W, cs.cinp, cs.cout, cs.inp.ld, cs.ldraw, cs.k, 0, code, sc.ws.data_ptr(), sc.ws_floats, st)

    def bn_of(code):
        # batch statistics from this plan's per-tile (mean, M2) partials: mean and 1/std per channel
        tm = _lib.query('ssp_conv_stats_tile_m', B, cs.H, cs.W, cs.cinp, cs.cout, cs.k, code)
        nt = _lib.query('ssp_conv_stats_tiles', B, cs.H, cs.W, cs.cinp, cs.cout, cs.k, code)
        tmp = torch.zeros(8, cs.coutp, dtype=torch.float32, device=plan.device)
        tmp[0].fill_(1.0)
        tmp[3].fill_(1.0)
        call('ssp_bn_fwd_finalize', sc.stats.data_ptr(), nt, tm, cs.M, cs.cout, tmp[0].data_ptr(), tmp[1].data_ptr(),
             tmp[2].data_ptr(), tmp[3].data_ptr(), BN_MOMENTUM, BN_EPS, tmp[4].data_ptr(), tmp[5].data_ptr(),
             tmp[6].data_ptr(), tmp[7].data_ptr(), st)
        return [tmp[4, :cs.cout].clone(), tmp[5, :cs.cout].clone()]

    a = cs.inp
    operands = [(a.t, a.ld, a.off % a.ld, cs.cinp)] + ([] if wop is cs.conv.weight else [wop])
    return Probe(launch, lambda: cs.raw, operands, bn_of if cs.bn else None, prep)


def dgrad_probe(plan, cs, sc):
    B, call, st = plan.B, _lib.call, sc.stream
    wptr = plan._dpack.data_ptr() + 4 * cs.doff

    def prep(tile):
        call('ssp_wino_filter_transform_t', wptr, plan._wino_ud(cs, tile).data_ptr(), cs.cin, cs.coutp, tile, st)

    def launch(code):
        wt = plan._wino_ud(cs, wino_tile(code)).data_ptr() if wino_tile(code) else wptr
        call('ssp_conv_dgrad', cs.raw.data_ptr(), wt, sc.gscratch.data_ptr(), B, cs.H, cs.W, cs.coutp, cs.cin, cs.ldraw,
             cs.inp.ld, cs.k, 0, code, sc.ws.data_ptr(), sc.ws_floats, st)

    wslice = plan._dpack[cs.doff:cs.doff + cs.cinp * cs.k * cs.k * cs.coutp]
    return Probe(launch, lambda: sc.gscratch[:cs.M * cs.inp.ld], [(cs.raw, cs.ldraw, 0, cs.cout), wslice], None, prep)


def admit(kn, gen, code, key, probe, primary=True):
    """Verify-after-tune: a non-default plan is admitted only after its output on seeded random operands agrees with the default
    plan's output of the same launch (max|a-b| / max|b| <= 1e-5: the plans differ in fp32 summation order only) and, for BN
    layers, after the batch statistics finalized from its per-tile partials agree too.  A Winograd plan is another ALGORITHM,
    not another summation order: its bar is 3e-5 of the output's range (measured ~1e-6).  A code that fails is refused (plan 0
    runs) and reported in TUNE_REJECTED.  Cached choices (this process or the JSON file) are re-verified once per process."""
    if code == 0 or not kn.verify or _TUNE_VERIFIED.get(key) == code or (key, code) in _TUNE_VERIFIED_ALSO:
        return code
    # Operands are the plan's own buffers (no data yet: tuning runs before the first forward, Plan.backward's fallback never
    # tunes).  Only the columns a launch owns are randomised: the channel padding of a zeros-allocated map must stay zero.
    for t in probe.operands:
        (t[0].view(-1, t[1])[:, t[2]:t[2] + t[3]] if isinstance(t, tuple) else t).uniform_(-1.0, 1.0, generator=gen)
    if wino_tile(code):
        probe.prep(wino_tile(code))      # operands changed: derived operands (Winograd-transformed filters) follow
    bar = 3e-5 if wino_tile(code) else 1e-5
    res = []
    for c in (0, code):
        probe.launch(c)
        res.append([probe.out_of().clone()] + (probe.bn_of(c) if probe.bn_of is not None else []))
    if all(float((a - b).abs().max()) <= bar * max(float(a.abs().max()), 1e-30) for a, b in zip(*res)):      # (false for NaN)
        if primary:
            _TUNE_VERIFIED[key] = code
        else:
            _TUNE_VERIFIED_ALSO.add((key, code))
        return code
    TUNE_REJECTED.append((key, code))
    if primary:
        _TUNE_CACHE[key] = 0
    warnings.warn("singleshotpose_amd: verify-after-tune refused plan %d for launch %s (result differs from the "
                  "default plan's); the default plan runs" % (code, key))
    return 0


# ---------------------------------------------------------------------- the forward / data-gradient pass
def _scratch(plan, kn, elig, which):
    """What the launches of a pass share: split-K scratch of the deepest candidate of any layer (x9 small, x4 mid, none big),
    statistics scratch for the finest tiling (Winograd plans: groups of 16 tiles, counts behind the pairs), the data gradients'
    output, the stream, the generator of verify-after-tune."""
    B, need = plan.B, 1
    wsq = lambda cs, K, N, code: _lib.query('ssp_conv_workspace_floats', B, cs.H, cs.W, K, N, cs.k, code)
    for cs in elig:
        mc = cs.M * max(cs.coutp, cs.cinp)
        need = max(need, 9 * mc if mc <= (1 << 21) else (4 * mc if mc <= (1 << 25) else 1))
        # ... and what the library's own heuristic (plan 0: the reference launch of verify-after-tune) asks for: it may
        # split K on a shape the candidate list does not (batch 64 at 832 x 832: the 26 x 26 layers, x3)
        bases = [WINO if t == 2 else WINO4 for t in wino_forms(kn, cs, B)[0]]
        for code in [0] + [b + 6413 for b in bases]:
            need = max(need, wsq(cs, cs.cinp, cs.cout, code))
            if code or not cs.first:
                need = max(need, wsq(cs, cs.coutp, cs.cin, code))
    f32 = dict(dtype=torch.float32, device=plan.device)
    stats = torch.empty(max(((cs.M + 15) // 16 + 16) * (cs.cout * 2 + 1) for cs in elig), **f32) if which == 'fwd' else None
    gscratch = torch.zeros(max(cs.M * max(cs.inp.ld, cs.ldraw) for cs in elig), **f32) if which == 'dgrad' else None
    gen = torch.Generator(device=plan.device).manual_seed(1234)
    return Scratch(torch.empty(need, **f32), need, stats, gscratch, torch.cuda.current_stream().cuda_stream, gen)


def _tune_fwd(plan, kn, sc, cs, probe, direct, wino):
    key = fwd_key(plan, cs)
    code = pick(kn, key, probe, direct, wino)
    chosen = admit(kn, sc.gen, code, key, probe)
    # The fastest code of every OTHER family that was timed (direct / F(2x2) / F(4x4)), verified the same way: what the error
    # budget of the forward plans may fall back to (_apply_head_budget); a refused one is dropped.
    fams = _TUNE_FAMILY.get(key) or {}
    cs.fwd_fams = {}
    for f, (c, ms) in fams.items():
        if c == chosen or (c != code and admit(kn, sc.gen, c, key, probe, primary=False) == c):
            cs.fwd_fams[f] = (c, ms)
    # (a direct family whose tuned code was refused still has the heuristic plan, code 0: the budget can always go direct)
    if 0 not in cs.fwd_fams and 0 in fams:
        cs.fwd_fams[0] = (0, fams[0][1])
    plan.set_code(cs, 'fwd', chosen)      # (after fwd_fams: the layer's statistics buffer is sized for every family)
    plan._release_filters('fwd', [cs])    # not chosen: the transformed-filter buffers go back to the allocator


def _tune_dgrad(plan, kn, sc, cs, probe, direct, wino):
    key = plan._dgrad_key(cs)
    plan.set_code(cs, 'dgrad', admit(kn, sc.gen, pick(kn, key, probe, direct, wino), key, probe))
    plan._release_filters('dgrad', [cs])


def x3_launch(plan, cs, which):
    """(tune key, K, N, fp32 code) of the bf16x3 decision of a layer's forward / data-gradient launch; None for the first block,
    a launch the kernel does not fit, a data gradient that ended on a Winograd code."""
    K, N = (cs.cinp, cs.cout) if which == 'fwd' else (cs.coutp, cs.cin)
    if cs.first or (which == 'dgrad' and wino_tile(cs.plan_dgrad)) or not _lib.query(
            'ssp_conv_bf16x3_fits', plan.B, cs.H, cs.W, K, N, cs.k, BF16X3 + 12813):
        return None
    if which == 'dgrad':
        return x3_key(plan._dgrad_key(cs)), K, N, cs.plan_dgrad
    # the direct code the layer runs when it ends on one (now, or when the head budget moves it there)
    return x3_key(fwd_key(plan, cs)), K, N, (cs.fwd_fams or {}).get(0, (0 if wino_tile(cs.plan_fwd) else cs.plan_fwd, None))[0]


def _tune_x3(plan, kn, sc, cs, probe, key, K, N, fp32_code):
    """bf16x3 mode, after (and apart from) the fp32 decisions: the launch's direct fp32 code against the bf16x3 codes, same timing,
    near-ties to fp32, verified against plan 0 at the direct 1e-5.  Plan._apply_conv_math / _conv_math_dgrad substitute."""
    if key not in _TUNE_CACHE:
        timed = [(code, time_launch(lambda: probe.launch(code), 2)) for code in (fp32_code,) + x3_candidates(cs, plan.B, K, N)]
        _TUNE_CACHE[key] = select(kn, key[0], [(0, timed[0][1])] + timed[1:])[0]      # (0 = the fp32 code stays)
    return admit(kn, sc.gen, _TUNE_CACHE[key], key, probe)


def x3_wino_launches(plan, cs, which):
    """[(tile, tune key, fp32 Winograd code)] of the twin decisions of a layer's forward / data-gradient launch: the
    through-memory Winograd code the launch ended on and, forward, the one of every other family the head budget may move the
    layer to (cs.fwd_fams) - those whose twins the kernel fits."""
    if which == 'dgrad':
        key, codes, K, N = plan._dgrad_key(cs), [cs.plan_dgrad], cs.coutp, cs.cin
    else:
        key, K, N = fwd_key(plan, cs), cs.cinp, cs.cout
        codes = [cs.plan_fwd] + [c for f, (c, _) in sorted((cs.fwd_fams or {}).items()) if f != wino_tile(cs.plan_fwd)]
    out = []
    for code in codes:
        twins = x3_wino_twins(code)
        if twins and not cs.first and _lib.query('ssp_conv_bf16x3_fits', plan.B, cs.H, cs.W, K, N, cs.k, twins[0]):
            out.append((wino_tile(code), x3_wino_key(key, wino_tile(code)), code))
    return out


def _tune_x3_wino(plan, kn, sc, cs, probe, key, fp32_code):
    """bf16x3-wino mode, after (and apart from) the fp32 decisions and the head budget's families: the Winograd code against its
    twins, same timing, near-ties to fp32, verified against plan 0 at the Winograd 3e-5.  Plan._apply_conv_math /
    _conv_math_dgrad substitute."""
    if key not in _TUNE_CACHE:
        probe.prep(wino_tile(fp32_code))
        timed = [(code, time_launch(lambda: probe.launch(code), 2)) for code in (fp32_code,) + x3_wino_twins(fp32_code)]
        _TUNE_CACHE[key] = select(kn, key[0], [(0, timed[0][1])] + timed[1:])[0]      # (0 = the fp32 code stays)
    return admit(kn, sc.gen, _TUNE_CACHE[key], key, probe)


def tunable(plan):
    """The layers whose forward / data-gradient launches take plan codes: dense, stride 1, input channels a multiple of 16."""
    return [cs for cs in plan.convs.values() if cs.cinp % 16 == 0 and cs.stride == 1 and not cs.depthwise]


def tune_convs(plan, which):
    """Times the candidate plans (tile rows x split-K x LDS ring depth, the Winograd forms) of every eligible forward
    (which = 'fwd') or data-gradient ('dgrad') launch of this input shape on the plan's own buffers and keeps the fastest
    (SURVEY.md section 8f rank 2).  The library's shape heuristic is within ~5-15 % of the best choice on some layers; which
    plan wins depends on how the grid fills the 256 CUs.  One-off cost per (B,H,W): ~1 s for yolo-pose.cfg.  SSP_AUTOTUNE=0
    disables; SSP_TUNE_CACHE=<file> keeps the timed choices across processes (JSON).  Every choice passes admit() before it runs."""
    kn = knobs()
    _tune_cache_load()
    n_known = len(_TUNE_CACHE)
    elig = tunable(plan)
    if not elig:
        return
    sc = _scratch(plan, kn, elig, which)
    make_probe, tune = (fwd_probe, _tune_fwd) if which == 'fwd' else (dgrad_probe, _tune_dgrad)
    probes = {cs.ind: make_probe(plan, cs, sc) for cs in elig}      # (the fp32 and the bf16x3 decisions share them)
    for cs in elig:
        cands = conv_candidates(kn, cs, plan.B, which)
        if cands is not None:
            tune(plan, kn, sc, cs, probes[cs.ind], *cands)
    for cs in elig if plan.conv_math['mode'] != 'fp32' else ():
        x3 = x3_launch(plan, cs, which)
        if x3 is not None:
            setattr(cs, 'x3_' + which, _tune_x3(plan, kn, sc, cs, probes[cs.ind], *x3))
    for cs in elig if plan.conv_math['mode'] == 'bf16x3-wino' else ():
        setattr(cs, 'x3w_' + which, {t: _tune_x3_wino(plan, kn, sc, cs, probes[cs.ind], key, code)
                                     for t, key, code in x3_wino_launches(plan, cs, which)})
        # (the transformed filters of a family the layer is not on go back to the allocator, as after the fp32 pass)
        plan._release_filters(which, [cs])
    _finish_pass(n_known)


# ---------------------------------------------------------------------- the filter-gradient pass
def _time_wgrad(plan, kn, cs, key, forms, ws_floats, gen, det=False):
    """The fastest admitted filter-gradient form of one layer (0 = direct): each Winograd form that beats the best so far is
    verified at once, and a refused one does not move the bar.  det: the ordered entry points, the library's split."""
    B, call, st = plan.B, _lib.call, torch.cuda.current_stream().cuda_stream
    f32 = dict(dtype=torch.float32, device=plan.device)
    ws = torch.empty(ws_floats, **f32)
    dw = [torch.zeros(cs.cout * 9 * cs.cinp, **f32) for _ in range(2)]
    a = cs.inp
    a.t.view(-1, a.ld)[:, a.off % a.ld:a.off % a.ld + cs.cinp].uniform_(-1.0, 1.0, generator=gen)
    cs.raw.view(-1, cs.ldraw)[:, :cs.cout].uniform_(-1.0, 1.0, generator=gen)

    def launch(out, t):
        if det and t == 0:
            call('ssp_conv_wgrad_ordered', cs.raw.data_ptr(), cs.inp.ptr, out.data_ptr(), B, cs.H, cs.W, cs.cinp, cs.cout, cs.ldraw,
                 cs.inp.ld, cs.k, 1, 0, 0, ws.data_ptr(), ws.numel(), st)
        elif det:
            call('ssp_conv_wgrad_wino_ordered', cs.raw.data_ptr(), cs.inp.ptr, out.data_ptr(), B, cs.H, cs.W, cs.cinp, cs.cout,
                 cs.ldraw, cs.inp.ld, t, 0, ws.data_ptr(), ws.numel(), st)
        elif t == 0:
            call('ssp_conv_wgrad', cs.raw.data_ptr(), cs.inp.ptr, out.data_ptr(), B, cs.H, cs.W, cs.cinp, cs.cout, cs.ldraw,
                 cs.inp.ld, cs.k, st)
        else:
            call('ssp_conv_wgrad_wino_t', cs.raw.data_ptr(), cs.inp.ptr, out.data_ptr(), B, cs.H, cs.W, cs.cinp, cs.cout,
                 cs.ldraw, cs.inp.ld, t, ws.data_ptr(), ws.numel(), st)

    use, best_ms = 0, time_launch(lambda: launch(torch.empty_like(dw[0]), 0), 3)
    if best_ms is None:
        return 0
    dw[0].zero_()
    launch(dw[0], 0)
    den = float(dw[0].abs().max())
    for t in forms:
        ms = time_launch(lambda: launch(torch.empty_like(dw[0]), t), 3)
        ms = ms if ms is None else credited(kn, 'wgrad', t, ms)
        if ms is None or not beats(ms, best_ms):
            continue
        dw[1].zero_()          # verification pair: one accumulation each into zeroed buffers
        launch(dw[1], t)
        if float((dw[0] - dw[1]).abs().max()) <= 3e-5 * max(den, 1e-30):
            use, best_ms = t, ms
        else:
            TUNE_REJECTED.append((key, 'wgrad_wino%d' % t))
            warnings.warn("singleshotpose_amd: verify-after-tune refused the Winograd F(%dx%d) filter gradient for %s" % (t, t, key))
    return use


def tune_wgrad(plan):
    """Filter gradients of the deep 3x3 layers: direct kernel or Winograd domain (ssp_conv_wgrad_wino_t, tile 2 or 4, or
    WGRAD_FUSED), whichever is fastest on this shape; a Winograd form is admitted only after its result on seeded operands
    agrees with the direct kernel's to 3e-5 of the gradient's range.  Runs before the first forward of the plan (its operands
    are the plan's own, still empty, buffers).  The choice (0 = direct, else the tile value) is cached per launch shape."""
    kn = knobs()
    gen = torch.Generator(device=plan.device).manual_seed(4321)
    n_known = len(_TUNE_CACHE)
    det = bool(getattr(plan, 'deterministic', None) and plan.deterministic['mode'])
    for cs in plan.convs.values():
        forms = wgrad_candidates(kn, cs, plan.B, det)
        if not forms:
            plan.set_code(cs, 'wgrad', 0)
            continue
        key = plan._wgrad_key(cs)
        if det:      # ordered candidates, ordered kernels, keys of their own: the two modes' caches never mix
            key = det_key(key)
            wsn = {t: _lib.query('ssp_conv_wgrad_wino_ordered_workspace_floats', plan.B, cs.H, cs.W, cs.cinp, cs.cout, t, 0) for t in forms}
            wsn[0] = _lib.query('ssp_conv_wgrad_ordered_workspace_floats', plan.B, cs.H, cs.W, cs.cinp, cs.cout, cs.ldraw, cs.inp.ld, cs.k, 1, 0)
        else:
            wsn = {t: _lib.query('ssp_conv_wgrad_wino_workspace_floats_t', plan.B, cs.H, cs.W, cs.cinp, cs.cout, t) for t in forms}
        cached = _TUNE_CACHE.get(key)
        if cached is not None and (cached == 0 or (cached in forms and (not kn.verify or _TUNE_VERIFIED.get(key) == cached))):
            form = cached
        else:
            form = _TUNE_CACHE[key] = _TUNE_VERIFIED[key] = _time_wgrad(plan, kn, cs, key, forms, max(wsn.values()), gen, det)
        plan.set_code(cs, 'wgrad', form)       # (sizes the layer's workspace for the form: wsn[form])
    _finish_pass(n_known)

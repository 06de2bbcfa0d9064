"""What the convolution tuner DOES, pinned as a transcript: which candidates it times for every tune key and in which
order, under which cache keys, what it verifies, and the plan set it leaves behind.

The GPU tests elsewhere check the numbers a tuned plan produces; this one checks the tuner's decisions, so that its code can
be moved and deduplicated under a pin.  It reaches the tuner only through names that do not depend on where the tuner lives:
`_lib.call`, `torch.cuda.Event.elapsed_time`, the tune-state containers re-exported by `engine`, and the per-layer fields of
a plan.

  recorder   wraps `_lib.call` and appends (name, arguments without the pointer positions of `_lib._SIGS`) BEFORE forwarding,
             so a launch that raises SspError is recorded too.  Ints stay ints, floats are recorded as repr.
  clock      `torch.cuda.Event.elapsed_time` returns 0.05 + 0.95 * crc32(repr((seed, last recorded call))) / 2^32 ms: a
             candidate's "time" is a fixed function of what was launched.  The range straddles the 0.25 ms threshold of the
             on-chip credit.  Real launches still run and verify-after-tune still compares real outputs.
  attempts   a timed launch is one that the clock was read after (or that raised); the codes timed since the last new
             `_TUNE_CACHE` key belong to that key.

Four transcripts of one small net (NET below; batch 2, 24 x 24): (a) default environment, cold; (b) the same model with its
plans dropped, in the same process (cached and already-verified paths); (c) SSP_CONV_MATH=bf16x3, cold; (d)
SSP_WINO_TILES=4 SSP_WINO_FUSED=0, cold.  Each records the model's construction and one training forward with parameters
that require gradients (forward, data-gradient and filter-gradient tuning); a backward afterwards, outside the recording,
runs the chosen plan set once.

The fixture tests/golden/tuner_transcript.json was written by `python tests/test_gpu_tuner_transcript.py --record <file>`
on an MI355X (twice, byte-identical), before the tuner was moved out of engine.py; it is never re-recorded for a change
that is meant to leave the tuner's behaviour alone.
"""
import functools
import hashlib
import json
import os
import sys
import zlib

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import topology_cases as tc      # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'tuner_transcript.json')

# layer: what of the tuner it shows
#  0 first block (4 input channels: never a tune key); its pool (layer 1) is folded into it
#  2 32 -> 64: Cout <= 64, the heuristic plan (0,) against the on-chip form alone
#  3 64 -> 64: F(4x4) eligible, F(2x2) not; Cout <= 64 forward, Cin <= 64 data gradient
#  4 64 -> 128: direct list + F(4x4) + on-chip forward; a thin data gradient
#  5 128 -> 128: F(2x2), F(4x4), on-chip, all three filter-gradient forms, the adjoint rule
#  6 128 -> 128 1x1
#  7 128 -> 128 stride 2 (12 x 12 -> 6 x 6): skipped; shares the data-gradient key of layer 8
#  8 128 -> 128 on 6 x 6: 2 * ceil(6/4)^2 = 8 < 16 tiles excludes the F(4x4) filter gradient, 2 * 3^2 = 18 keeps F(2x2)
#  9 128 -> 18 1x1, no BatchNorm: an output map with padding channels (never a tune key, in either direction)
# 10 18 -> 20 head (the network output must be a multiple of 4 channels wide)
# every map is small enough for the `deep` split list and the latency ring
NET = tc.Case('tuner-transcript', 'hand',
              tc.conv(32) + tc.pool() + tc.conv(64) + tc.conv(64) + tc.conv(128) + tc.conv(128) + tc.conv(128, 1) +
              tc.conv(128, 3, 1, 'leaky', 2) + tc.conv(128) + tc.conv(18, 1, 0, 'linear') + tc.head(20), 2, 24, 24, 3, 777)

KNOBS = ('SSP_TUNE_CACHE', 'SSP_AUTOTUNE', 'SSP_TUNE_VERIFY', 'SSP_CONV_MATH', 'SSP_WINOGRAD', 'SSP_WINO_TILES',
         'SSP_WINO_MIN_CHANNELS', 'SSP_WINO4_MIN_CHANNELS', 'SSP_WINO_FUSED', 'SSP_WGRAD_FUSED_PREFER', 'SSP_ONCHIP_PREFER',
         'SSP_ONCHIP_CREDIT_MS', 'SSP_FIRST_FUSED', 'SSP_BN_FUSE')
# transcript -> (environment on top of the defaults, clock seed)
RUNS = {'a': ({}, 11), 'b': ({}, 11), 'c': ({'SSP_CONV_MATH': 'bf16x3'}, 23),
        'd': ({'SSP_WINO_TILES': '4', 'SSP_WINO_FUSED': '0'}, 37)}
STATE = ('_TUNE_CACHE', '_TUNE_FAMILY', '_TUNE_VERIFIED', '_TUNE_VERIFIED_ALSO', 'TUNE_REJECTED')
# position of the plan code among the non-pointer arguments of the launches the tuner times
CODE_POS = {'ssp_conv_fwd': 9, 'ssp_conv_dgrad': 9, 'ssp_conv_wgrad_wino_t': 7, 'ssp_conv_wgrad': None}


class Recorder(object):
    def __init__(self, seed, real_call):
        from singleshotpose_amd import _lib, engine
        self._lib, self.engine, self.real = _lib, engine, real_call
        self.seed = seed
        self.on = True
        self.events = []
        self.last = None
        self.armed = None          # plan code of the last recorded call when it is a launch the tuner times
        self.pending = []          # codes timed since the last new tune key
        self.attempts = []         # [(tune key, [codes])], in the order the keys were timed
        self.seen = set(engine._TUNE_CACHE)

    def _strip(self, name, args):
        sig = self._lib._SIGS[name]
        out = []
        for t, a in zip(sig, args):
            if t is self._lib.P:
                continue
            out.append(a if isinstance(a, int) and not isinstance(a, bool) else repr(a))
        return out

    def _flush(self):
        new = [k for k in self.engine._TUNE_CACHE if k not in self.seen]
        if new:
            self.attempts.append((new[0], self.pending))
            self.attempts += [(k, []) for k in new[1:]]
            self.pending = []
            self.seen.update(new)

    def _attempt(self, code):
        if not self.pending or self.pending[-1] != code:
            self.pending.append(code)

    def call(self, name, *args):
        if not self.on:
            return self.real(name, *args)
        self._flush()
        ev = [name, self._strip(name, args)]
        self.events.append(ev)
        self.last = ev
        self.armed = None
        if name in CODE_POS:
            self.armed = 0 if CODE_POS[name] is None else ev[1][CODE_POS[name]]
        try:
            return self.real(name, *args)
        except self._lib.SspError:
            if self.armed is not None:
                self._attempt(self.armed)
                self.armed = None
            raise

    def clock(self):
        if self.on and self.armed is not None:
            self._attempt(self.armed)
        return 0.05 + 0.95 * zlib.crc32(repr((self.seed, self.last)).encode()) / 2.0 ** 32

    def stop(self):
        self._flush()
        if self.pending:
            self.attempts.append((None, self.pending))
        self.on = False


def _chain(events):
    """sha1 of the whole event list, and a running 16-bit digest per event (what locates the first differing event)."""
    h = hashlib.sha1()
    out = []
    for ev in events:
        h.update(json.dumps(ev).encode())
        out.append(h.hexdigest()[:4])
    return h.hexdigest(), ''.join(out)


def _key(k):
    return json.dumps(list(k)) if k is not None else 'null'


def _summary(rec, plan, engine):
    layers = {}
    for i, cs in sorted(plan.convs.items()):
        layers[str(i)] = dict(plan_fwd=cs.plan_fwd, plan_dgrad=cs.plan_dgrad, wgrad_wino=cs.wgrad_wino, x3_fwd=cs.x3_fwd,
                              x3_dgrad=cs.x3_dgrad, dgrad_adj=bool(cs.dgrad_adj),
                              fwd_fams={str(f): c for f, (c, _) in sorted((cs.fwd_fams or {}).items())})
    sha, chain = _chain(rec.events)
    return dict(
        attempts=[[_key(k), codes] for k, codes in rec.attempts],
        layers=layers,
        tune_cache=sorted([_key(k), v] for k, v in engine._TUNE_CACHE.items()),
        tune_family=sorted([_key(k), {str(f): [c, repr(t)] for f, (c, t) in sorted(v.items())}]
                           for k, v in engine._TUNE_FAMILY.items()),
        verified=sorted([_key(k), v] for k, v in engine._TUNE_VERIFIED.items()),
        verified_also=sorted([_key(k), c] for k, c in engine._TUNE_VERIFIED_ALSO),
        rejected=[[_key(k), c] for k, c in engine.TUNE_REJECTED],
        events=len(rec.events), sha1=sha, chain=chain)


def _record_one(mp, name, model, keep_events):
    """One recorded training forward of `model` (its plans dropped first), then an unrecorded backward."""
    from singleshotpose_amd import _lib, engine
    env, seed = RUNS[name]
    for k in KNOBS:
        mp.delenv(k, raising=False)
    mp.setenv('SSP_HEAD_ERR_BUDGET', '0')
    for k, v in env.items():
        mp.setenv(k, v)
    model._plans.clear()
    rec = Recorder(seed, _lib.call)
    with pytest.MonkeyPatch.context() as mp2:
        mp2.setattr(_lib, 'call', rec.call)
        mp2.setattr(torch.cuda.Event, 'elapsed_time', lambda e0, e1: rec.clock())
        x = tc.make_input(NET, 0).cuda()
        y = model(x)
        rec.stop()
        plan = next(iter(model._plans.values()))
        out = _summary(rec, plan, engine)
        (y * tc.make_probe(NET, 0, y.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
    keep_events[name] = rec.events
    return out


def _model():
    model = tc.make_model(NET).cuda().train()
    for p in model.parameters():
        p.requires_grad_(True)
    return model


def _with_clean_state(fn):
    """fn() with the module-level tune state saved, cleared in place, and restored in place afterwards."""
    from singleshotpose_amd import engine
    saved = {n: type(getattr(engine, n))(getattr(engine, n)) for n in STATE}
    cache_file = engine._TUNE_CACHE_FILE[0]
    try:
        for n in STATE:
            getattr(engine, n).clear()
        engine._TUNE_CACHE_FILE[0] = None
        return fn()
    finally:
        engine._TUNE_CACHE_FILE[0] = cache_file
        for n in STATE:
            c = getattr(engine, n)
            c.clear()
            (c.extend if isinstance(c, list) else c.update)(saved[n])


EVENTS = {}      # transcript -> the events of this process's run (for the report of a failure)


@functools.lru_cache(maxsize=None)
def transcripts(group):
    """'ab' -> {'a': ..., 'b': ...} (one process state), 'c' / 'd' -> {that one}."""
    def run():
        with pytest.MonkeyPatch.context() as mp:
            model = _model()
            return {name: _record_one(mp, name, model, EVENTS) for name in group}
    return _with_clean_state(run)


def _first_difference(name, got, want):
    n = min(len(got['chain']), len(want['chain'])) // 4
    for i in range(n):
        if got['chain'][4 * i:4 * i + 4] != want['chain'][4 * i:4 * i + 4]:
            break
    else:
        i = n
    ev = EVENTS.get(name, [])
    lines = ['transcript (%s): %d events against %d recorded; the first differing event is number %d'
             % (name, got['events'], want['events'], i)]
    lines += ['  %s %d: %s' % ('>>' if j == i else '  ', j, json.dumps(ev[j])) for j in range(max(0, i - 3), min(len(ev), i + 2))]
    return '\n'.join(lines)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(RUNS))
def test_tuner_transcript(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = transcripts('ab' if name in 'ab' else name)[name]
    got = json.loads(json.dumps(got))
    for part in ('attempts', 'layers', 'tune_cache', 'tune_family', 'verified', 'verified_also', 'rejected'):
        if got[part] != want[part]:
            print(_first_difference(name, got, want))
        assert got[part] == want[part], 'transcript (%s): %s differs' % (name, part)
    if got['sha1'] != want['sha1']:
        print(_first_difference(name, got, want))
    assert (got['events'], got['sha1']) == (want['events'], want['sha1'])
    assert got['chain'] == want['chain']


if __name__ == '__main__':
    assert sys.argv[1] == '--record', 'usage: test_gpu_tuner_transcript.py --record <file>'
    out = {}
    for group in ('ab', 'c', 'd'):
        out.update(transcripts(group))
    with open(sys.argv[2], 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    for name in sorted(out):
        print(name, out[name]['events'], 'events,', len(out[name]['attempts']), 'keys, rejected', out[name]['rejected'],
              out[name]['sha1'])

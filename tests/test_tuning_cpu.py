"""singleshotpose_amd.tuning without a GPU: the candidate lists it generates for the net of
tests/test_gpu_tuner_transcript.py are the lists the recorded transcripts show being timed (same fixture), and the selection
rule on hand-written (code, ms) tables."""
import json

import pytest
import torch

from singleshotpose_amd import tuning
from singleshotpose_amd.engine import Plan
from test_gpu_tuner_transcript import GOLDEN, KNOBS, NET, RUNS, tc


def _generated(plan, kn, layers):
    """[(tune key, codes)] in the order tune_convs('fwd'), tune_convs('dgrad') and tune_wgrad time them on a cold cache.
    `layers`: the recorded final state (the bf16x3 pass of the data gradients skips a layer that ended on a Winograd code)."""
    out, seen = [], set()

    def add(key, codes):
        if key not in seen:
            seen.add(key)
            out.append((key, list(codes)))
    for which in ('fwd', 'dgrad'):
        for cs in tuning.tunable(plan):
            cands = tuning.conv_candidates(kn, cs, plan.B, which)
            if cands is not None:
                add(tuning.fwd_key(plan, cs) if which == 'fwd' else plan._dgrad_key(cs), cands[0] + cands[1])
        if plan.conv_math['mode'] == 'bf16x3':
            for cs in tuning.tunable(plan):
                cs.plan_dgrad = layers[str(cs.ind)]['plan_dgrad']
                x3 = tuning.x3_launch(plan, cs, which)
                if x3 is not None:
                    add(x3[0], (None,) + tuning.x3_candidates(cs, plan.B, x3[1], x3[2]))
    for cs in plan.convs.values():
        forms = tuning.wgrad_candidates(kn, cs, plan.B)
        if forms:
            add(plan._wgrad_key(cs), (0,) + forms)
    return out


@pytest.mark.parametrize('name', ['a', 'c', 'd'])
def test_generated_candidates_are_the_recorded_attempts(name, monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in RUNS[name][0].items():
        monkeypatch.setenv(k, v)
    plan = Plan(tc.make_model(NET), NET.B, NET.H, NET.W, torch.device('cpu'))
    got = _generated(plan, tuning.knobs(), want['layers'])
    assert [json.dumps(list(k)) for k, _ in got] == [k for k, _ in want['attempts']]
    for (key, codes), (_, timed) in zip(got, want['attempts']):
        if codes[0] is None:      # a bf16x3 decision: the launch's fp32 code (a timing result) leads the list
            assert tuning.conv_math_of(timed[0]) == 'fp32', key
            codes, timed = codes[1:], timed[1:]
        assert codes == timed, key
    assert len(got) >= 12


def _kn(**kw):
    return tuning.knobs()._replace(credit_ms=0.25, wgrad_credit=0.8, dgrad_credit=0.85, **kw)


def test_select_keeps_the_earlier_candidate_on_a_near_tie():
    kn = _kn()
    assert tuning.NEAR_TIE == 0.985
    assert tuning.select(kn, 'fwd', [(12813, 1.0), (12814, 0.99), (6414, 0.986)])[0] == 12813
    assert tuning.select(kn, 'fwd', [(12813, 1.0), (12814, 0.99), (6414, 0.984)])[0] == 6414
    # the bar moves with the winner, not with every candidate
    assert tuning.select(kn, 'fwd', [(12813, 1.0), (12814, 0.98), (6414, 0.97)])[0] == 12814
    # a launch the library refused is no candidate; nothing timed: the heuristic plan
    assert tuning.select(kn, 'fwd', [(12813, None), (12814, 0.5)])[0] == 12814
    assert tuning.select(kn, 'fwd', [(12813, None)]) == (0, {})
    assert tuning.beats(0.5, None) and not tuning.beats(0.985, 1.0) and tuning.beats(0.9849, 1.0)


def test_select_fills_the_family_table():
    kn = _kn()
    W, W4, F = tuning.WINO, tuning.WINO4, tuning.WINOF
    best, fams = tuning.select(kn, 'fwd', [(12813, 0.60), (6413, 0.595), (6414, 0.50), (W + 6413, 0.40), (W + 6414, 0.399),
                                             (W4 + 6413, 0.45), (W4 + 12813, 0.30), (F, 0.395)])
    assert best == W4 + 12813
    # per family the same near-tie rule; the on-chip code belongs to family 2 (it has to beat F(2x2) clearly)
    assert fams == {0: (6414, 0.50), 2: (W + 6413, 0.40), 4: (W4 + 12813, 0.30)}
    assert tuning.select(kn, 'fwd', [(0, 0.5), (F, 0.3)])[1] == {0: (0, 0.5), 2: (F, 0.3)}


def test_credit_only_for_big_onchip_gradient_launches():
    kn = _kn()
    F, G = tuning.WINOF, tuning.WGRAD_FUSED
    assert tuning.credited(kn, 'dgrad', F, 0.25) == 0.25 * 0.85 and tuning.credited(kn, 'dgrad', F, 0.2499) == 0.2499
    assert tuning.credited(kn, 'wgrad', G, 0.25) == 0.25 * 0.8 and tuning.credited(kn, 'wgrad', G, 0.2499) == 0.2499
    # not the forward, not a through-memory Winograd or direct code, not tile 2 / 4 of the filter gradient, not a bf16x3 key
    for kind, code in (('fwd', F), ('dgrad', tuning.WINO + 6413), ('dgrad', tuning.WINO4 + 6413), ('dgrad', 12813),
                       ('wgrad', 2), ('wgrad', 4), ('wgrad', 0), ('dgrad-bf16x3', tuning.BF16X3 + 12813), ('fwd-bf16x3', F)):
        assert tuning.credited(kn, kind, code, 0.5) == 0.5, (kind, code)
    # the credit decides a data-gradient race at or above the threshold only
    table = [(tuning.WINO4 + 6413, 0.50), (F, 0.55)]
    assert tuning.select(kn, 'dgrad', table)[0] == F and tuning.select(kn, 'fwd', table)[0] == tuning.WINO4 + 6413
    small = [(tuning.WINO4 + 6413, 0.20), (F, 0.22)]
    assert tuning.select(kn, 'dgrad', small)[0] == tuning.WINO4 + 6413
    assert tuning.select(kn, 'dgrad', table)[1][2] == (F, 0.55 * 0.85)


def test_knobs_are_read_per_call_and_spell_the_tag(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    kn = tuning.knobs()
    assert (kn.wino_on, kn.tiles, kn.min2, kn.min4, kn.fused_on, kn.verify, kn.autotune) == (True, (2, 4), 128, 64, True, True, True)
    assert (kn.credit_ms, kn.wgrad_credit, kn.dgrad_credit) == (0.25, 0.8, 0.85)
    assert kn.tag == tuning._tune_tag() == 'r6-w2,4-c128-64-f1'
    monkeypatch.setenv('SSP_WINO_TILES', '4')
    monkeypatch.setenv('SSP_ONCHIP_CREDIT_MS', '0.3')
    assert tuning.knobs().tiles == (4,) and tuning._tune_tag() == 'r6-w4-c128-64-f10.3'
    assert tuning.form_allowed(tuning.knobs(), 4) and not tuning.form_allowed(tuning.knobs(), 2)
    monkeypatch.setenv('SSP_WINO_FUSED', '0')
    monkeypatch.setenv('SSP_WINO_TILES', '2,4')
    kn = tuning.knobs()
    assert tuning.form_allowed(kn, 2) and not tuning.form_allowed(kn, 2, onchip=True) and tuning.form_allowed(kn, 0)
    monkeypatch.setenv('SSP_WINOGRAD', '0')
    assert tuning._tune_tag() == 'r5-direct' and not tuning.form_allowed(tuning.knobs(), 4)

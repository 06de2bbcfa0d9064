"""The bf16x3 twin codes of the through-memory Winograd plans (mode 'bf16x3-wino'), without a GPU: the properties of the
exact-integer operands of tests/exact_wino_bf16x3.py that tests/test_gpu_wino_bf16x3.py relies on, the host queries over a table of
twin codes, and the engine's switch (mode value, code families, tune tag, the refusal between ranks)."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import exact_wino as XW
import exact_wino_bf16x3 as XB


# ------------------------------------------------------------------------------------------------ the operand classes
def _entries(c):
    return [(e, cls) for e in XB.ENTRIES for cls in XB.CLASSES if not (e == 'adj-own' and c.tile == 4)]


@pytest.mark.parametrize("c", XB.CASES, ids=lambda c: c.id)
def test_every_class_needs_its_products_and_stays_exact(c):
    """Per case, entry point and class, asserted and not assumed: V (the float64 transform model) is exactly an fp32; the
    three dropped products vanish at every (plane, tile, channel); each product the class is there to pin is needed (the
    model without it differs from the full sum); sum_k |U| |V| < 2^24, so every partial sum in any order is an exact fp32."""
    for entry, cls in _entries(c):
        V, U, _ = XB.gemm_operands(cls, c, entry)
        what = (c.id, entry, cls)
        XW.f32(V), XW.f32(U)                                   # (asserts that nothing is lost)
        assert np.array_equal(V, np.round(V)) and np.array_equal(U, np.round(U)), what
        tv, tu = XB.terms(V), XB.terms(U)
        assert np.array_equal(tv[0] + tv[1] + tv[2], V) and np.array_equal(tu[0] + tu[1] + tu[2], U), what
        for a, b in XB.DROPPED:
            assert not XW.contract(tv[a], tu[b]).any(), what + ((a, b),)
        full = XB.model(V, U)
        assert np.array_equal(full, XW.contract(V, U)), what
        for prod in XB.PINNED[cls]:
            assert not np.array_equal(XB.model(V, U, [p for p in XB.PRODUCTS if p != prod]), full), what + (prod,)
        assert XB.abs_bound(V, U) < XW.TWO24, what


def test_the_f4_adjoint_with_its_own_dm_runs_on_exact_one_term_operands():
    for c in XB.CASES:
        if c.tile != 4:
            continue
        dM, Ut, dy = XB.gemm_operands('v3u1', c, 'adj-own')
        assert set(np.unique(dy)) <= {-1.0, 0.0, 1.0} and set(np.unique(Ut)) <= {-1.0, 0.0, 1.0}
        XW.f32(dM)
        assert XB.abs_bound(dM, Ut) * XW.GRID[4]['dM'] < XW.TWO24
        assert np.abs(XW.contract(dM, Ut)).max() > 0


def test_the_classes_cover_all_six_products_and_the_cases_every_path():
    assert set(p for cls in XB.CLASSES for p in XB.PINNED[cls]) == set(XB.PRODUCTS)
    assert {c.tile for c in XB.CASES} == {2, 4}
    assert {c.K // 16 for c in XB.CASES} == {1, 3, 7} and {c.N for c in XB.CASES} == {64, 68, 132}
    ts = {(c.tile, XB.geom(c).T) for c in XB.CASES}
    assert any(t == 4 and 64 < T <= 128 for t, T in ts) and any(T > 128 for _, T in ts) and any(T < 64 for _, T in ts)
    assert any(XB.geom(c).mosaic for c in XB.CASES)


# ------------------------------------------------------------------------------------------------ host queries
def _lib():
    from singleshotpose_amd import _lib
    return _lib


def test_fits_query_over_the_table_of_twin_codes():
    L = _lib()
    for B, H, W, Cin, Cout, R, plan, fits in XB.FITS_TABLE:
        assert L.query('ssp_conv_bf16x3_fits', B, H, W, Cin, Cout, R, plan) == fits, (B, H, W, Cin, Cout, R, plan)
    assert len(XB.MISFITS) == 10
    assert XB.twin(4, 128) == 8612813 and XB.twin(2, 64) == 9606413


def test_the_fits_table_of_the_direct_family_keeps_its_answers():
    import exact_bf16x3 as X3
    L = _lib()
    for B, H, W, Cin, Cout, R, plan, fits in X3.FITS_TABLE:
        assert L.query('ssp_conv_bf16x3_fits', B, H, W, Cin, Cout, R, plan) == fits, (B, H, W, Cin, Cout, R, plan)


@pytest.mark.parametrize("shape", [(2, 5, 7, 16, 64), (5, 13, 13, 112, 132), (8, 13, 13, 48, 68), (64, 13, 13, 1024, 1024),
                                   (64, 52, 52, 128, 256)])
def test_tile_workspace_and_statistics_queries_equal_the_fp32_twins(shape):
    L = _lib()
    B, H, W, Cin, Cout = shape
    for tile in (2, 4):
        for bm in XB.BMS:
            code = XB.twin(tile, bm)
            f32c = XB.fp32_twin(code)
            assert f32c == (8000000 if tile == 4 else 9000000) + bm * 100 + 13
            assert L.query('ssp_conv_plan_wino_tile', code) == tile == L.query('ssp_conv_plan_wino_tile', f32c)
            for q in ('ssp_conv_workspace_floats', 'ssp_conv_stats_tile_m', 'ssp_conv_stats_tiles', 'ssp_conv_stats_floats'):
                assert L.query(q, B, H, W, Cin, Cout, 3, code) == L.query(q, B, H, W, Cin, Cout, 3, f32c), (q, code)
            for own in (0, 1):
                assert L.query('ssp_conv_dgrad_adj_workspace_floats', B, H, W, Cin, Cout, code, own) == \
                    L.query('ssp_conv_dgrad_adj_workspace_floats', B, H, W, Cin, Cout, f32c, own) > 0


# ------------------------------------------------------------------------------------------------ the engine's switch
def test_conv_math_of_and_the_family_helper():
    from singleshotpose_amd import engine, tuning
    twins = [XB.twin(t, bm) for t in (2, 4) for bm in XB.BMS]
    for code in twins:
        assert engine.conv_math_of(code) == 'bf16x3' and tuning.x3_wino(code) and engine.wino_tile(code) in (2, 4)
        assert not engine.wino_fused(code)
    for code in (6012813, 6006493):
        assert engine.conv_math_of(code) == 'bf16x3' and not tuning.x3_wino(code)
    for code in (0, 12813, 306413, 612813, engine.WINOF, 7612813, 8012813, 8006414, 9012818, 8512813, 9712813):
        assert engine.conv_math_of(code) == 'fp32' and not tuning.x3_wino(code), code
    assert tuning.x3_wino_twins(8012814) == (8612813, 8606413) and tuning.x3_wino_twins(9006418) == (9612813, 9606413)
    for code in (0, 12813, engine.WINOF, 6012813, 8612813):
        assert tuning.x3_wino_twins(code) == ()
    key = ('fwd', 4, 16, 16, 64, 128, 3, 64, 128, True, 'tag')
    assert tuning.x3_wino_key(key, 4) == ('fwd-bf16x3-wino',) + key[1:] + (4,)
    assert tuning.x3_wino_key(key, 4) != tuning.x3_wino_key(key, 2) and tuning.x3_key(key)[0] == 'fwd-bf16x3'


def test_tune_tag_and_candidates_do_not_depend_on_the_knob(monkeypatch):
    from singleshotpose_amd import engine
    seen = []
    for mode in (None, 'bf16x3', 'bf16x3-wino'):
        if mode is None:
            monkeypatch.delenv('SSP_CONV_MATH', raising=False)
        else:
            monkeypatch.setenv('SSP_CONV_MATH', mode)
        assert engine.conv_math_env() == (mode or 'fp32')
        seen.append((engine._tune_tag(), engine.IGEMM_CANDS, engine.IGEMM_LATENCY_CANDS, engine.WINO_GEMM_CANDS))
    assert seen[0] == seen[1] == seen[2]
    assert seen[0][3] == (6413, 6414, 12813, 12814)
    assert engine.CONV_MATHS == ('fp32', 'bf16x3', 'bf16x3-wino')
    monkeypatch.setenv('SSP_CONV_MATH', 'bf16x3-winograd')
    with pytest.raises(ValueError):
        engine.conv_math_env()


def test_mode_value_through_the_environment_and_the_model_attribute(monkeypatch):
    from helpers import ROOT
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    monkeypatch.delenv('SSP_CONV_MATH', raising=False)
    model = Darknet(os.path.join(ROOT, 'tests', 'golden', 'tiny-pose.cfg'))
    monkeypatch.setenv('SSP_CONV_MATH', 'bf16x3-wino')
    assert model.conv_math == 'bf16x3-wino'
    plan = engine.Plan(model, 2, 96, 96, torch.device('cpu'))
    assert plan.conv_math == dict(mode='bf16x3-wino', layers={}, head_deviation=0.0, taken_back=[])
    model._plans['x'] = plan
    model.conv_math = 'bf16x3-wino'                          # no change: the plans stay
    assert 'x' in model._plans
    model.conv_math = 'bf16x3'                               # the attribute wins over the environment, and drops the plans
    assert model.conv_math == 'bf16x3' and not model._plans
    monkeypatch.delenv('SSP_CONV_MATH', raising=False)
    model._plans['x'] = plan
    model.conv_math = 'bf16x3-wino'
    assert model.conv_math == 'bf16x3-wino' and not model._plans
    assert engine.Plan(model, 2, 96, 96, torch.device('cpu')).conv_math['mode'] == 'bf16x3-wino'


def test_without_the_tuner_the_mode_equals_bf16x3(monkeypatch):
    """SSP_AUTOTUNE=0 (and every plan on a CPU device): no Winograd plan exists, the substitutions are those of 'bf16x3'."""
    from helpers import ROOT
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    codes = {}
    for mode in ('bf16x3', 'bf16x3-wino'):
        monkeypatch.setenv('SSP_CONV_MATH', mode)
        plan = engine.Plan(model, 4, 160, 160, torch.device('cpu'))
        assert plan.conv_math['mode'] == mode
        assert all(cs.x3w_fwd is None and cs.x3w_dgrad is None for cs in plan.convs.values())
        codes[mode] = {i: (plan._x3_default(cs, 'fwd'), plan._x3_default(cs, 'dgrad')) for i, cs in plan.convs.items()}
    assert codes['bf16x3'] == codes['bf16x3-wino'] and any(f for f, _ in codes['bf16x3'].values())


# ------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q, rank1_mode):
    """Rank 0 runs 'bf16x3-wino' and carries twin codes; rank 1 runs `rank1_mode`."""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ['SSP_CONV_MATH'] = 'bf16x3-wino' if rank == 0 else rank1_mode
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers import ROOT
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.dist import init_distributed, sync_plans
    import torch.distributed as dist
    init_distributed('gloo')
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    fn = sync_plans(model)
    assert fn is not None and hasattr(fn, 'all_ok')
    plan = engine.Plan(model, 4, 160, 160, torch.device('cpu'))
    if rank == 0:
        plan.set_code(plan.convs[13], 'fwd', 12813)
        plan.set_code(plan.convs[4], 'fwd', 8612813, 8012813)
        plan.set_code(plan.convs[8], 'dgrad', 9606413, 9006413)
    plan._sync_codes(0)
    plan._sync_codes(1)
    q.put((rank, {i: (cs.plan_fwd, cs.plan_dgrad, cs.fp32_fwd, cs.fp32_dgrad) for i, cs in plan.convs.items()},
           dict(plan.conv_math)))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(rank1_mode):
    world = 2
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, rank1_mode)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: (a, b) for r, a, b in (q.get(timeout=240) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("rank1_mode", ['fp32', 'bf16x3'])
def test_a_rank_whose_mode_is_not_bf16x3_wino_refuses_twin_codes_and_every_rank_falls_back(rank1_mode):
    res = _two_ranks(rank1_mode)
    for r in (0, 1):
        assert all(v == (0, 0, None, None) for v in res[r][0].values()), (r, res[r][0])
        assert res[r][1]['layers'] == {}
    assert res[0][0] == res[1][0]


def test_two_ranks_in_the_mode_share_rank0_twin_codes():
    res = _two_ranks('bf16x3-wino')
    assert {i: v[:2] for i, v in res[0][0].items()} == {i: v[:2] for i, v in res[1][0].items()}
    assert res[0][0][4][2] == 8012813 and res[0][0][8][3] == 9006413      # (each rank goes back to its OWN fp32 code)
    a = res[1][0]
    assert a[4][0] == 8612813 and a[8][1] == 9606413 and a[13][0] == 12813
    assert a[4][2] == 0 and a[8][3] == 0                     # (rank 1's own fp32 codes to go back to)
    assert res[1][1]['layers'] == {4: (8612813, 0), 8: (0, 9606413)}

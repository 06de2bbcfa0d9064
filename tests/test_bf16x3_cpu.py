"""bf16x3 fast mode, everything that needs no GPU: the host model of the three-term split, the properties of the
exact-integer operands of tests/exact_bf16x3.py (every case class NEEDS the products it is there to pin), the host
queries of the plan family, and the engine's switch (conv_math_of, untouched tune keys, the _sync_codes refusal)."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import exact_bf16x3 as X
import exact_conv as E


# ------------------------------------------------------------------------------------------------ the split
def _random_fp32(n, seed):
    """n fp32 values, both signs, magnitudes spread over 40 binades (2^-20 .. 2^20), full 24-bit significands."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(1.0, 2.0, n) * np.exp2(rs.randint(-20, 20, n)) * rs.choice([-1.0, 1.0], n)
    return torch.from_numpy(v.astype(np.float32))


def test_split_is_exact_and_every_term_is_a_bf16():
    x = _random_fp32(1 << 20, 1)
    assert x.numel() >= 10 ** 6
    e = torch.frexp(x)[1]
    assert int(e.max()) - int(e.min()) >= 39
    for cvt in (X.bf16_rne, X.bf16_trunc):
        h, m, l = X.split3(x, cvt)
        assert X.is_bf16(h) and X.is_bf16(m) and X.is_bf16(l)
        assert torch.equal((h + m) + l, x)                                   # bit for bit, in fp32
        assert torch.equal(h.double() + m.double() + l.double(), x.double())
    h, m, l = X.split3(x)
    # round to nearest: each term is at most half an ulp (2^-9) of the one before it
    assert bool((m.abs() <= h.abs() * 2.0 ** -8).all()) and bool((l.abs() <= h.abs() * 2.0 ** -16).all())


def test_dropped_products_stay_below_2_to_the_minus_24():
    """m*l + l*m + l*l of a product x*w, as a fraction of |x*w|, on random pairs (round-to-nearest split); and the same
    figure for the truncating split, which is why the kernel does not use it."""
    x, w = _random_fp32(1 << 20, 2), _random_fp32(1 << 20, 3)
    out = {}
    for name, cvt in (('rne', X.bf16_rne), ('trunc', X.bf16_trunc)):
        (xh, xm, xl), (wh, wm, wl) = [tuple(t.double() for t in X.split3(v, cvt)) for v in (x, w)]
        dropped = xm * wl + xl * wm + xl * wl
        rel = (dropped / (x.double() * w.double())).abs()
        out[name] = (float(rel.max()), float((rel ** 2).mean().sqrt()))
    print('dropped terms, max / rms: rne 2^%.1f / 2^%.1f, trunc 2^%.1f / 2^%.1f'
          % tuple(np.log2(v) for v in out['rne'] + out['trunc']))
    assert out['rne'][0] <= 2.0 ** -24
    assert out['trunc'][0] > 2.0 * out['rne'][0]


def test_test_integers_split_the_same_way_under_both_roundings():
    want = {257: (256, 1, 0), 385: (384, 1, 0), 513: (512, 1, 0), 262657: (262144, 512, 1)}
    for v in range(-E.XMAX, E.XMAX + 1):
        want[v] = (v, 0, 0)
    for v, (h, m, l) in list(want.items()):
        want[-v] = (-h, -m, -l)
    for v, t in want.items():
        for cvt in (X.bf16_rne, X.bf16_trunc):
            got = tuple(int(s) for s in X.split3(torch.tensor([float(v)]), cvt))
            assert got == t, (v, got, t)
    # an integer that only LOOKS right: 65793 = 2^16 + 2^8 + 1 rounds its first term UP (257 > half an ulp of 512), so
    # round-to-nearest gives (66048, -256, 1) where truncation gives (65536, 256, 1)
    v = torch.tensor([65793.0])
    assert tuple(int(s) for s in X.split3(v, X.bf16_rne)) != tuple(int(s) for s in X.split3(v, X.bf16_trunc))


# ------------------------------------------------------------------------------------------------ exact-integer cases
@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_every_class_needs_its_products_and_stays_exact(case):
    B, H, W, K, N, R = case
    for cls in X.CLASSES:
        inp, w = X.operands(cls, case, B, H, W, K, N, R)
        ref = X.conv(inp, w, R)
        # 1. every partial sum of every term product, in any order, is an exact fp32 - with the prefill added as well
        bound = X.abs_bound(inp, w, R)
        assert bound + E.PREFILL < E.TWO24, (cls, bound)
        # 2. the dropped products vanish identically, so the six evaluated ones ARE the product
        ti, tw = X.terms(inp), X.terms(w)
        for a, b in X.DROPPED:
            assert not bool(ti[a].any()) or not bool(tw[b].any()), (cls, a, b)
            assert not bool(X.conv(ti[a], tw[b], R).any())
        assert torch.equal(X.model(inp, w, R), ref)
        # 3. each product the class pins is needed: without it the model misses the reference somewhere
        for prod in X.PINNED[cls]:
            rest = tuple(p for p in X.PRODUCTS if p != prod)
            assert not torch.equal(X.model(inp, w, R, rest), ref), (cls, prod)


def test_the_classes_cover_all_six_products():
    assert set(p for c in X.CLASSES for p in X.PINNED[c]) == set(X.PRODUCTS)
    assert len(X.PRODUCTS) == 6 and not set(X.PRODUCTS) & set(X.DROPPED)


# ------------------------------------------------------------------------------------------------ host queries
def _lib():
    from singleshotpose_amd import _lib
    return _lib


def test_fits_query_over_the_table():
    L = _lib()
    assert 'ssp_conv_bf16x3_fits' in L.exported_symbols()
    for B, H, W, Cin, Cout, R, plan, fits in X.FITS_TABLE:
        assert L.query('ssp_conv_bf16x3_fits', B, H, W, Cin, Cout, R, plan) == fits, (B, H, W, Cin, Cout, R, plan)
    assert X.MISFIT_LAUNCHES


@pytest.mark.parametrize("shape", [(2, 5, 7, 16, 64, 3), (3, 9, 11, 48, 132, 3), (64, 104, 104, 32, 64, 3),
                                   (64, 13, 13, 1024, 64, 1), (64, 13, 13, 512, 1024, 3), (4, 26, 26, 256, 512, 3)])
def test_statistics_and_workspace_queries_match_the_direct_plan(shape):
    """For Cout > 64 the direct kernel honours tile rows and split of an explicit code, so the two families can be compared
    code by code; for Cout <= 64 (where the direct kernel ignores codes) the figures follow from the code itself."""
    L = _lib()
    B, H, W, Cin, Cout, R = shape
    M = B * H * W
    niter = R * R * Cin // 16
    for bm in (64, 128):
        for ks in (1, 2, 3, 8):
            code = X.plan_code(bm, ks)
            if not L.query('ssp_conv_bf16x3_fits', B, H, W, Cin, Cout, R, code):
                assert ks > 1 and niter // ks < 8
                continue
            assert L.query('ssp_conv_plan_wino_tile', code) == 0
            got = [L.query(n, B, H, W, Cin, Cout, R, code) for n in
                   ('ssp_conv_stats_tile_m', 'ssp_conv_stats_tiles', 'ssp_conv_stats_floats', 'ssp_conv_workspace_floats')]
            tiles = (M + bm - 1) // bm
            assert got == [bm, tiles, tiles * Cout * 2, ks * M * Cout if ks > 1 else 0]
            if Cout > 64:
                direct = bm * 100 + ks * 10 + 3
                assert got == [L.query(n, B, H, W, Cin, Cout, R, direct) for n in
                               ('ssp_conv_stats_tile_m', 'ssp_conv_stats_tiles', 'ssp_conv_stats_floats',
                                'ssp_conv_workspace_floats')]


def test_adjoint_workspace_query_knows_no_bf16x3_plan():
    assert _lib().query('ssp_conv_dgrad_adj_workspace_floats', 2, 13, 13, 128, 128, X.plan_code(128), 1) == 0


# ------------------------------------------------------------------------------------------------ the engine's switch
def test_conv_math_of():
    from singleshotpose_amd import engine
    assert engine.BF16X3 == X.BF16X3
    for code in (X.plan_code(64), X.plan_code(128, 9), 6000000, 6999999):
        assert engine.conv_math_of(code) == 'bf16x3'
    for code in (0, 12813, 306413, 5999999, engine.WINOF, engine.WINO + 6413, engine.WINO4 + 12814):
        assert engine.conv_math_of(code) == 'fp32'


def test_tune_tag_and_candidates_do_not_depend_on_the_knob(monkeypatch):
    from singleshotpose_amd import engine
    monkeypatch.delenv('SSP_CONV_MATH', raising=False)
    off = (engine._tune_tag(), engine.IGEMM_CANDS, engine.IGEMM_LATENCY_CANDS, engine.WINO_GEMM_CANDS)
    assert engine.conv_math_env() == 'fp32'
    monkeypatch.setenv('SSP_CONV_MATH', 'bf16x3')
    assert engine.conv_math_env() == 'bf16x3'
    assert (engine._tune_tag(), engine.IGEMM_CANDS, engine.IGEMM_LATENCY_CANDS, engine.WINO_GEMM_CANDS) == off
    assert off[1] == (12813, 12814, 6414, 6413, 12824, 12834, 306413, 306414, 312813, 312814, 206413, 212814,
                      12823, 6423, 6424, 206414, 212813, 406413, 406414, 412813)
    assert not any(engine.conv_math_of(c) == 'bf16x3' for c in off[1] + off[2] + off[3])
    monkeypatch.setenv('SSP_CONV_MATH', 'fp16')
    with pytest.raises(ValueError):
        engine.conv_math_env()


def test_model_attribute_follows_the_environment_and_drops_plans(monkeypatch):
    from helpers import ROOT
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    monkeypatch.delenv('SSP_CONV_MATH', raising=False)
    model = Darknet(os.path.join(ROOT, 'tests', 'golden', 'tiny-pose.cfg'))
    assert model.conv_math == 'fp32'
    plan = engine.Plan(model, 2, 96, 96, torch.device('cpu'))
    assert plan.conv_math == dict(mode='fp32', layers={}, head_deviation=0.0, taken_back=[])
    monkeypatch.setenv('SSP_CONV_MATH', 'bf16x3')
    assert model.conv_math == 'bf16x3'                       # read when a plan is built, not when the model was
    assert engine.Plan(model, 2, 96, 96, torch.device('cpu')).conv_math['mode'] == 'bf16x3'
    model._plans['x'] = plan
    model.conv_math = 'bf16x3'                               # no change: the plans stay
    assert 'x' in model._plans
    model.conv_math = 'fp32'                                 # the attribute wins over the environment, and drops the plans
    assert model.conv_math == 'fp32' and not model._plans
    assert engine.Plan(model, 2, 96, 96, torch.device('cpu')).conv_math['mode'] == 'fp32'
    with pytest.raises(ValueError):
        model.conv_math = 'tf32'


def test_heuristic_codes_of_a_plan_built_without_the_tuner(monkeypatch):
    """SSP_AUTOTUNE=0 (and every plan on a CPU device): each launch that fits gets the code with the tile rows and split of
    the library's own plan for it; the first block, thin outputs and stride-2 blocks get none."""
    from helpers import ROOT
    from singleshotpose_amd import _lib, engine
    from singleshotpose_amd.darknet import Darknet
    monkeypatch.setenv('SSP_CONV_MATH', 'bf16x3')
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    plan = engine.Plan(model, 4, 160, 160, torch.device('cpu'))
    n = 0
    for ind, cs in sorted(plan.convs.items()):
        for which, (K, N) in (('fwd', (cs.cinp, cs.cout)), ('dgrad', (cs.coutp, cs.cin))):
            code = plan._x3_default(cs, which)
            args = (4, cs.H, cs.W, K, N, cs.k)
            fits = cs.stride == 1 and K % 16 == 0 and N > 32 and N % 4 == 0
            assert bool(code) == fits, (ind, which, code)
            if code:
                n += 1
                assert engine.conv_math_of(code) == 'bf16x3' and _lib.query('ssp_conv_bf16x3_fits', *(args + (code,)))
                assert _lib.query('ssp_conv_stats_tile_m', *(args + (code,))) == min(128, _lib.query('ssp_conv_stats_tile_m', *(args + (0,))))
                assert _lib.query('ssp_conv_workspace_floats', *(args + (code,))) == _lib.query('ssp_conv_workspace_floats', *(args + (0,)))
    assert n >= 30


# ------------------------------------------------------------------------------------------------ two ranks, one with the mode off
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker_sync_refused(rank, world, port, q, both_on):
    """Rank 0 runs the bf16x3 mode and carries 6xxxxxx codes; rank 1's mode is off (unless both_on): it must not adopt them,
    so NO rank does - every rank falls back to plan 0 for that stage, as for a Winograd code a rank has switched off."""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.pop('SSP_CONV_MATH', None)
    if rank == 0 or both_on:
        os.environ['SSP_CONV_MATH'] = 'bf16x3'
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
        plan.set_code(plan.convs[4], 'fwd', X.plan_code(128), 0)
        plan.set_code(plan.convs[8], 'dgrad', X.plan_code(64), 0)
    else:
        plan.set_code(plan.convs[13], 'fwd', 6414)
    plan._sync_codes(0)
    plan._sync_codes(1)
    q.put((rank, {i: (cs.plan_fwd, cs.plan_dgrad, cs.fp32_fwd, cs.fp32_dgrad, cs.tile_m, cs.ntile) for i, cs in plan.convs.items()},
           dict(plan.conv_math)))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(both_on):
    world = 2
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_sync_refused, args=(r, world, port, q, both_on)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: (a, b) for r, a, b in (q.get(timeout=240) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_a_rank_with_the_mode_off_refuses_bf16x3_codes_and_every_rank_falls_back():
    res = _two_ranks(False)
    for r in (0, 1):
        assert all(v[:4] == (0, 0, None, None) for v in res[r][0].values()), (r, res[r][0])
        assert res[r][1]['layers'] == {}
    assert res[0][0] == res[1][0]


def test_two_ranks_with_the_mode_on_share_rank0_codes():
    res = _two_ranks(True)
    assert res[0][0] == res[1][0]
    a = res[1][0]
    assert a[4][0] == X.plan_code(128) and a[4][2] == 0 and a[8][1] == X.plan_code(64) and a[8][3] == 0 and a[13][0] == 12813
    assert res[1][1]['layers'] == {4: (X.plan_code(128), 0), 8: (0, X.plan_code(64))}

"""The bitwise-reproducible training mode, the part that needs no GPU: the appended entry points, the pure-host split /
workspace queries, the knob, the model attribute, the tune-cache keys, the plan's record and the multi-rank fallback."""
import multiprocessing as mp
import os
import re
import socket

import pytest
import torch

import exact_conv as E
import strided_cases as S

NEW = {'ssp_conv_wgrad_ordered_split': 10, 'ssp_conv_wgrad_ordered_workspace_floats': 10, 'ssp_conv_wgrad_ordered': 17,
       'ssp_conv_wgrad_wino_ordered_split': 7, 'ssp_conv_wgrad_wino_ordered_workspace_floats': 7,
       'ssp_conv_wgrad_wino_ordered': 15, 'ssp_conv_s2_dgrad_ordered': 13}


def _lib():
    from singleshotpose_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ ABI
def test_new_symbols_in_header_and_exports_with_matching_argument_counts():
    from helpers import ROOT
    lib = _lib()
    with open(os.path.join(ROOT, 'include', 'ssp_hip.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, name + ' is not declared in include/ssp_hip.h'
        assert len(m.group(1).split(',')) == nargs, name
        assert name in lib.exported_symbols() and len(lib._SIGS[name]) == nargs, name
        assert hasattr(lib.load(), name), name + ' is not exported by the library'
    assert lib.query('ssp_abi_version') == 5


# ------------------------------------------------------------------------------------------------ pure-host queries
def _queries(geom, stride, split):
    q = _lib().query
    return (q('ssp_conv_wgrad_ordered_split', *(geom + (stride, split))),
            q('ssp_conv_wgrad_ordered_workspace_floats', *(geom + (stride, split))))


@pytest.mark.parametrize("c", E.WGRAD_CASES, ids=lambda c: c.id)
def test_stride1_workspace_is_split_times_the_gradient(c):
    B, H, W, Cin, Cout, R = c.shape
    cinp = E.pad4(Cin)
    geom = (B, H, W, cinp, Cout, c.lddy, c.ldx, R)
    assert _lib().query('ssp_conv_wgrad_route', *geom) != 0
    for split in (0, 1, 2, 3, 7, 1 << 20):
        ns, ws = _queries(geom, 1, split)
        assert ns >= 1 and ws == ns * Cout * R * R * cinp, (split, ns, ws)
        assert split == 0 or ns <= split
        assert _queries(geom, 1, split) == (ns, ws)              # a function of its arguments alone
    assert _queries(geom, 1, 1)[0] == 1


@pytest.mark.parametrize('c', S.CASES, ids=S.case_id)
def test_stride2_workspace_is_split_times_the_gradient(c):
    B, H, W, Cin, Cout, R = c.shape
    ldx, ldy, _ = S.buffers(c)
    geom = (B, H, W, E.pad4(Cin), Cout, ldy, ldx, R)
    Ho, Wo = S.out_hw(H, W, R)
    for split in (0, 1, 3, 1 << 20):
        ns, ws = _queries(geom, 2, split)
        assert ns >= 1 and ws == ns * Cout * R * R * E.pad4(Cin)
        assert ns <= max(1, (B * Ho * Wo + 15) // 16)            # never more ranges than 16-pixel chunks


@pytest.mark.parametrize("tile,shape", E.WINO_WGRAD_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_winograd_workspace_grows_by_the_slabs_only(tile, shape):
    q = _lib().query
    B, H, W, Cin, Cout = shape
    base = q('ssp_conv_wgrad_wino_workspace_floats_t', B, H, W, Cin, Cout, tile)
    for split in (0, 1, 2, 3, 1 << 20):
        ns = q('ssp_conv_wgrad_wino_ordered_split', B, H, W, Cin, Cout, tile, split)
        ws = q('ssp_conv_wgrad_wino_ordered_workspace_floats', B, H, W, Cin, Cout, tile, split)
        if tile == 12 or min(Cin, Cout) < 64:
            assert (ns, ws) == (0, 0)                            # the on-chip form has no ordered counterpart
            continue
        assert ns >= 1 and ws == base + (ns - 1) * (tile + 2) ** 2 * Cin * Cout
        assert split == 0 or ns <= split
        assert ns <= (E.wino_tiles(B, H, W, tile) + 15) // 16
    # the un-ordered query is what it was
    assert base == (0 if tile == 12 else (tile + 2) ** 2 * (E.wino_tiles(B, H, W, tile) * (Cin + Cout) + Cin * Cout))


def test_a_refused_shape_returns_zero_like_the_route_query():
    q = _lib().query
    for geom in [(2, 5, 5, 6, 8, 8, 8, 3), (2, 5, 5, 8, 8, 8, 4, 3), (2, 5, 5, 8, 10, 8, 8, 3), (2, 5, 5, 8, 8, 8, 8, 5),
                 (0, 5, 5, 8, 8, 8, 8, 3), (1 << 11, 1 << 10, 1 << 10, 8, 8, 8, 8, 3)]:
        assert q('ssp_conv_wgrad_route', *geom) == 0
        for stride in (1, 2):
            assert _queries(geom, stride, 0) == (0, 0), (geom, stride)
    ok = (2, 5, 5, 8, 8, 8, 8, 3)
    assert _queries(ok, 1, 0)[0] >= 1 and _queries(ok, 3, 0) == (0, 0) and _queries(ok, 1, -1) == (0, 0)


# ------------------------------------------------------------------------------------------------ knob and attribute
def test_knob_is_parsed_in_tuning_knobs(monkeypatch):
    from singleshotpose_amd import tuning
    monkeypatch.delenv('SSP_DETERMINISTIC', raising=False)
    assert tuning.knobs().deterministic is False
    for v, want in (('', False), ('0', False), ('1', True)):
        monkeypatch.setenv('SSP_DETERMINISTIC', v)
        assert tuning.knobs().deterministic is want
    for v in ('2', 'true', 'yes', '-1'):
        monkeypatch.setenv('SSP_DETERMINISTIC', v)
        with pytest.raises(ValueError):
            tuning.knobs()


def test_attribute_wins_over_the_environment_and_drops_cached_plans(monkeypatch):
    from helpers import ROOT
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    monkeypatch.delenv('SSP_DETERMINISTIC', raising=False)
    model = Darknet(os.path.join(ROOT, 'tests', 'golden', 'tiny-pose.cfg'))
    assert model.deterministic is False
    plan = engine.Plan(model, 2, 96, 96, torch.device('cpu'))
    assert plan.deterministic == dict(mode=False, layers={}, taken_back=[])
    monkeypatch.setenv('SSP_DETERMINISTIC', '1')
    assert model.deterministic is True                        # read when a plan is built, not when the model was
    assert engine.Plan(model, 2, 96, 96, torch.device('cpu')).deterministic['mode'] is True
    model._plans['x'] = plan
    model.deterministic = True                                # no change: the plans stay
    assert 'x' in model._plans
    model.deterministic = False                               # the attribute wins over the environment, the plans go
    assert not model._plans and model.deterministic is False
    assert engine.Plan(model, 2, 96, 96, torch.device('cpu')).deterministic['mode'] is False
    with pytest.raises(ValueError):
        model.deterministic = 'yes'


def test_tune_tag_candidates_and_mode_off_keys_do_not_depend_on_the_knob(monkeypatch):
    from helpers import ROOT
    from singleshotpose_amd import engine, tuning
    from singleshotpose_amd.darknet import Darknet

    def snapshot():
        model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
        model.deterministic = False                          # a mode-off plan, whatever the environment says
        plan = engine.Plan(model, 4, 160, 160, torch.device('cpu'))
        kn = tuning.knobs()
        keys = []
        for cs in plan.convs.values():
            keys += [tuning.fwd_key(plan, cs), plan._dgrad_key(cs), plan._wgrad_key(cs), tuning.wgrad_candidates(kn, cs, plan.B),
                     tuning.conv_candidates(kn, cs, plan.B, 'fwd'), tuning.conv_candidates(kn, cs, plan.B, 'dgrad')]
        return (engine._tune_tag(), engine.IGEMM_CANDS, engine.IGEMM_LATENCY_CANDS, engine.WINO_GEMM_CANDS, keys)
    monkeypatch.delenv('SSP_DETERMINISTIC', raising=False)
    off = snapshot()
    monkeypatch.setenv('SSP_DETERMINISTIC', '1')
    assert snapshot() == off
    # the mode's own decisions live under keys of their own and never offer the on-chip form
    key = ('wgrad', 4, 20, 20, 256, 512, 512, 256, off[0])
    assert tuning.det_key(key) == ('wgrad-det',) + key[1:]
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    plan = engine.Plan(model, 4, 160, 160, torch.device('cpu'))
    kn = tuning.knobs()
    some = False
    for cs in plan.convs.values():
        a, b = tuning.wgrad_candidates(kn, cs, plan.B), tuning.wgrad_candidates(kn, cs, plan.B, True)
        assert tuning.WGRAD_FUSED not in b and b == tuple(t for t in a if t != tuning.WGRAD_FUSED)
        some = some or tuning.WGRAD_FUSED in a
    assert some


def test_cached_bench_tune_keys_are_untouched():
    """cfg/bench_tune_cache.json holds mode-off decisions: no key of the mode in it."""
    from helpers import ROOT
    with open(os.path.join(ROOT, 'cfg', 'bench_tune_cache.json')) as f:
        assert '-det' not in f.read()


# ------------------------------------------------------------------------------------------------ the plan's record
def test_cpu_plan_record_names_an_ordered_route_for_every_filter_gradient(monkeypatch):
    from helpers import ROOT
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    monkeypatch.delenv('SSP_DETERMINISTIC', raising=False)
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    model.deterministic = True
    plan = engine.Plan(model, 4, 160, 160, torch.device('cpu'))
    rec = plan.deterministic
    assert rec['mode'] is True and sorted(rec['layers']) == sorted(plan.convs)
    for i, cs in plan.convs.items():
        form, route, ns = rec['layers'][i]['wgrad']
        assert form in ('direct-ordered', 'stride2-ordered', 'winograd-ordered', 'first-block'), (i, form)
        assert ns >= 1 and (form == 'first-block' or route != 0), (i, rec['layers'][i])
        if form == 'direct-ordered':
            assert route == _lib().query('ssp_conv_wgrad_route', 4, cs.H, cs.W, cs.cinp, cs.cout, cs.ldraw, cs.inp.ld, cs.k)
        # no folded BatchNorm-sum launch: a block whose sums ride on a data gradient has a row per tile
        if cs.bnp is not None:
            assert cs.bnp[2] is False and rec['layers'][i]['bn_sums'] == 'consumer-dgrad rows=%d' % cs.bnp[1]
    assert any(cs.bnp is not None for cs in plan.convs.values())
    # a shape whose early layers have more than 1024 tiles: the mode takes the fusion back instead of folding
    big = engine.Plan(model, 16, 416, 416, torch.device('cpu'))
    assert all(cs.bnp is None or cs.bnp[2] is False for cs in big.convs.values())
    off = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    off.deterministic = False
    ref = engine.Plan(off, 16, 416, 416, torch.device('cpu'))
    ref._plan_bn_fusion()
    folded = sorted(i for i, cs in ref.convs.items() if cs.bnp is not None and cs.bnp[2])
    assert folded and sorted(i for i, what in big.deterministic['taken_back']) == folded
    assert all(big.deterministic['layers'][i]['bn_sums'] == 'two-level' for i in folded)


# ------------------------------------------------------------------------------------------------ two ranks, differing modes
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q, modes):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ['SSP_DETERMINISTIC'] = '1' if modes[rank] else '0'
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers import ROOT
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.dist import init_distributed, sync_plans
    import torch.distributed as dist
    init_distributed('gloo')
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    sync_plans(model)
    plan = engine.Plan(model, 4, 160, 160, torch.device('cpu'))
    for cs in plan.convs.values():
        cs.plan_dgrad, cs.wgrad_wino = 0, 0
    if rank == 0:
        plan.convs[13].plan_fwd = 12813
        plan._size_layer(plan.convs[13])
        plan.convs[8].plan_dgrad = 6414
        plan.convs[13].wgrad_wino = 4
    plan._sync_codes(0)
    plan._sync_codes(1)
    q.put((rank, {i: (cs.plan_fwd, cs.plan_dgrad, cs.wgrad_wino) for i, cs in plan.convs.items()}, plan.deterministic['mode'],
           {i: v['wgrad'][0] for i, v in plan.deterministic['layers'].items()}))
    dist.barrier()
    dist.destroy_process_group()


def _two_ranks(modes):
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, modes)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (a, m, rec) for r, a, m, rec in (q.get(timeout=240) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("modes", [(True, False), (False, True)], ids=['rank0-on', 'rank1-on'])
def test_ranks_with_differing_modes_fall_back_together(modes):
    res = _two_ranks(modes)
    for r in (0, 1):
        assert res[r][1] is modes[r]
        assert all(v == (0, 0, 0) for v in res[r][0].values()), (r, res[r][0])
    assert res[0][0] == res[1][0]


def test_ranks_with_the_mode_on_share_rank0_codes():
    res = _two_ranks((True, True))
    assert res[0][0] == res[1][0]
    assert res[1][0][13] == (12813, 0, 4) and res[1][0][8][1] == 6414
    assert res[1][2][13] == 'winograd-ordered' and res[1][2] == res[0][2]

"""Depthwise 3x3 blocks without a GPU: the host statements of tests/depthwise_cases.py against F.conv2d(groups=C) and its
autograd in float64, the exactness bound of the kernel cases, the module tree and parameter count, .weights I/O, the plan a
Plan builds for every net (on the CPU device: nothing is launched), every refusal, the seed conditions of the float and the
exact nets, the shipped cfg and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depthwise_cases as D
import topology_cases as T

ids = lambda cases: [c.id for c in cases]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- 1. host statements
@pytest.mark.parametrize('k', D.KERNEL_CASES, ids=D.kcase_id)
def test_host_statements_agree_with_conv2d_and_autograd(k):
    x, dy, w, pre_out, pre_in, pre_w = D.kernel_data(k)
    xt = torch.from_numpy(x.copy()).permute(0, 3, 1, 2).double().requires_grad_(True)
    wt = torch.from_numpy(w.copy()).double().view(k.C, 1, 3, 3).requires_grad_(True)
    bias = np.arange(k.C, dtype=np.float32) % 7 - 3
    y = F.conv2d(xt, wt, torch.from_numpy(bias).double(), stride=k.stride, padding=1, groups=k.C)
    Ho, Wo = D.out_hw(k.H, k.W, k.stride)
    assert tuple(y.shape) == (k.B, k.C, Ho, Wo)
    assert np.array_equal(D.dw_fwd_ref(x, w, k.stride, bias), y.detach().permute(0, 2, 3, 1).numpy())
    (y * torch.from_numpy(dy.copy()).permute(0, 3, 1, 2).double()).sum().backward()
    assert np.array_equal(D.dw_dgrad_ref(dy, w, k.H, k.W, k.stride), xt.grad.permute(0, 2, 3, 1).numpy())
    assert np.array_equal(D.dw_dgrad_ref(dy, w, k.H, k.W, k.stride, pre_in), xt.grad.permute(0, 2, 3, 1).numpy() + pre_in)
    assert np.array_equal(D.dw_wgrad_ref(dy, x, k.stride), wt.grad.view(k.C, 9).numpy())
    assert np.array_equal(D.dw_wgrad_ref(dy, x, k.stride, pre_w), wt.grad.view(k.C, 9).numpy() + pre_w)


def test_gather_is_the_documented_one():
    """One hand-checked element per rule of the header comment: the tap index, the stride-2 gather, zero outside the map and
    no read across an image boundary."""
    k = D.KCase(2, 3, 5, 8, 2, None, 0, 'in')
    x, dy, w, _, _, _ = D.kernel_data(k)
    out = D.dw_fwd_ref(x, w, 2)
    # output pixel (yo, xo) = (1, 2) of image 0: rows 1..3 (3 is outside), columns 3..5 (5 is outside)
    want = sum(x[0, 2 * 1 + r - 1, 2 * 2 + t - 1, 3] * w[3, 3 * r + t] for r in range(2) for t in range(2))
    assert out[0, 1, 2, 3] == want
    # output pixel (0, 0) of image 1 reads nothing of image 0
    want = sum(x[1, r - 1, t - 1, 0] * w[0, 3 * r + t] for r in (1, 2) for t in (1, 2))
    assert out[1, 0, 0, 0] == want
    # stride 2: an even input coordinate is reached by tap 1 only, an odd one by taps 0 and 2
    dx = D.dw_dgrad_ref(dy, w, 3, 5, 2)
    assert dx[0, 0, 2, 1] == dy[0, 0, 1, 1] * w[1, 4]
    assert dx[0, 1, 1, 1] == (dy[0, 1, 1, 1] * w[1, 0] + dy[0, 1, 0, 1] * w[1, 2] + dy[0, 0, 1, 1] * w[1, 6] + dy[0, 0, 0, 1] * w[1, 8])


def test_every_partial_sum_of_the_kernel_cases_is_exact_in_fp32():
    assert len(D.KERNEL_CASES) == 17
    for k in D.KERNEL_CASES:
        Ho, Wo = D.out_hw(k.H, k.W, k.stride)
        M = k.B * Ho * Wo
        b = D.exactness_bound(k)
        assert M <= 1352 and b <= M * 64 + 4 and b < 2 ** 24, (D.kcase_id(k), M, b)
        x, dy, w, pre_out, pre_in, pre_w = D.kernel_data(k)
        assert np.abs(x).max() <= 8 and np.abs(dy).max() <= 8 and np.abs(w).max() <= 3
        for a in (x, dy, w, pre_out, pre_in, pre_w):
            assert np.array_equal(a, np.round(a))


# ---------------------------------------------------------------------------------------------------- 2. module tree, .weights
def test_create_network_honours_groups():
    """(Before groups= was read, a depthwise block silently became a dense C -> C convolution with C times the filters.)"""
    model = D.make_model(D.DW_SEP, init=False)
    assert tuple(model.models[2][0].weight.shape) == (8, 1, 3, 3) and model.models[2][0].groups == 8
    assert tuple(model.models[4][0].weight.shape) == (16, 1, 3, 3) and model.models[4][0].stride == (2, 2)
    assert model.models[2][0].weight.is_contiguous() and model.models[2][0].bias is None
    assert [n for n, _ in model.models[2].named_children()] == ['conv2', 'bn2', 'leaky2']
    assert 'models.4.conv4.weight' in model.state_dict() and 'models.4.bn4.running_var' in model.state_dict()
    # conv 3->8 3x3 | dw 8 | 1x1 8->16 | dw 16 | 1x1 16->16 | head 16->8 (+ bias); every BatchNorm block: gamma, beta
    want = 8 * 27 + 8 * 9 + 16 * 8 + 16 * 9 + 16 * 16 + (8 * 16 + 8) + 2 * (8 + 8 + 16 + 16 + 16)
    assert sum(p.numel() for p in model.parameters()) == want
    b = D.make_model(D.DW_BIAS, init=False)
    assert tuple(b.models[1][0].weight.shape) == (8, 1, 3, 3) and tuple(b.models[1][0].bias.shape) == (8,)
    assert [n for n, _ in b.models[1].named_children()] == ['conv2']
    # a dense block is built exactly as before: channels-last in memory
    assert model.models[3][0].groups == 1 and model.models[3][0].weight.permute(0, 2, 3, 1).is_contiguous()


def test_weights_round_trip_is_byte_exact(tmp_path):
    a, b = D.make_model(D.DW_SEP), D.make_model(D.DW_SEP, init=False)
    path, again = str(tmp_path / 'dw.weights'), str(tmp_path / 'dw2.weights')
    a.save_weights(path)
    # (a net without a region block lists its last module a second time as `loss`: count the `models.` entries)
    n = sum(t.numel() for k, t in a.state_dict().items() if k.startswith('models.') and 'num_batches' not in k)
    assert n == 1208 and os.path.getsize(path) == 16 + 4 * n      # a depthwise block holds C * 9 filter floats, as Darknet's format
    b.load_weights(path)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        if 'num_batches' not in k:
            assert torch.equal(sa[k], sb[k]), k
    b.save_weights(again)
    with open(path, 'rb') as f, open(again, 'rb') as g:
        assert f.read() == g.read()
    # the depthwise filter of block 2 sits where Darknet puts it: behind the block's four BatchNorm vectors, C * 9 floats
    raw = np.fromfile(path, dtype=np.float32, offset=16)
    off = (4 * 8 + 8 * 27) + 4 * 8
    assert np.array_equal(raw[off:off + 72], a.models[2][0].weight.detach().numpy().reshape(-1))


# ---------------------------------------------------------------------------------------------------- 3. plans
def _no_launch(monkeypatch):
    from singleshotpose_amd import _lib

    def call(name, *args):
        raise AssertionError("planning launched %s" % name)
    monkeypatch.setattr(_lib, 'call', call)


def _plan(case, monkeypatch, det=False):
    from singleshotpose_amd import engine
    monkeypatch.delenv('SSP_BN_FUSE', raising=False)
    _no_launch(monkeypatch)
    model = D.make_model(case, init=False)
    model.deterministic = det
    return engine.Plan(model, case.B, case.H, case.W, torch.device('cpu'))


@pytest.mark.parametrize('case', D.NETS, ids=ids(D.NETS))
def test_plan_of_every_net(case, monkeypatch):
    from singleshotpose_amd import _lib, tuning
    plan = _plan(case, monkeypatch)
    want = D.PLANS[case.id]
    assert plan.depthwise == want['depthwise'] and plan.fused_pool == want['fused_pool']
    plan._plan_bn_fusion()
    assert {i: cs.bn_fuse_src.ind for i, cs in plan.convs.items() if cs.bn_fuse_src is not None} == want['bn_pairs']
    for i, cs in plan.convs.items():
        assert cs.depthwise == (i in want['depthwise'])
        if not cs.depthwise:
            continue
        C = cs.cin
        assert cs.cout == C and cs.k == 3 and cs.plan_fwd == 0 and cs.plan_dgrad == 0 and cs.wgrad_wino == 0
        assert cs.bn_fuse_src is None                              # never the consumer of a BatchNorm-backward pair
        assert (cs.H, cs.W) == D.out_hw(cs.Hi, cs.Wi, cs.stride)
        assert cs.tile_m == 0 and cs.ws_fwd == 0
        assert cs.ntile == _lib.query('ssp_dwconv_stats_tiles', plan.B, cs.Hi, cs.Wi, C, cs.stride) > 0
        if cs.bn:
            assert cs.stats.numel() == cs.ntile * (2 * C + 1)
        # flat weight and gradient ranges of 9 C floats, the parameter's own layout
        off, n, shape = plan.grad_layout[id(cs.conv.weight)]
        assert n == 9 * C and shape == (C, 1, 3, 3) and off % 4 == 0 and off == cs.grad_lo
        assert cs not in tuning.tunable(plan) and tuning.wgrad_candidates(tuning.knobs(), cs, plan.B) == ()
    assert plan.grad_total == sum((p.numel() + 3) // 4 * 4 for p in plan.net._params())
    assert plan._dpack_floats == max(1, sum(cs.cinp * cs.k * cs.k * cs.coutp for cs in plan.convs.values()
                                            if not (cs.first or cs.depthwise)))


def test_consumers_schedule_and_frozen_filter(monkeypatch):
    plan = _plan(D.DW_SHARED, monkeypatch)
    assert plan.consumers[0] == [1, 2] and plan.consumers[1] == [2]
    assert [op.kind for op in plan.ops] == ['conv', 'conv', 'shortcut', 'conv']
    sched = {s.ind: s for s in plan.backward_schedule()}
    assert sched[1].visited and sched[1].wgrad and sched[1].dgrad == (True,) and sched[1].bn_reduce
    # the depthwise filter frozen: no filter-gradient launch for it, everything else as before
    frozen = set(id(p) for p in plan.net._params()) - {id(plan.net.models[1][0].weight)}
    sched = {s.ind: s for s in plan.backward_schedule(frozen)}
    assert sched[1].visited and not sched[1].wgrad and sched[1].dgrad == (True,) and sched[1].dgamma and sched[0].wgrad
    # block 1 frozen altogether with its BatchNorm in eval(): visited only for the gradient it passes on
    frozen -= set(id(p) for p in plan.net.models[1].parameters())
    sched = {s.ind: s for s in plan.backward_schedule(frozen, bn_training={0: True, 1: False, 3: False})}
    assert sched[1].visited and not (sched[1].wgrad or sched[1].dgamma or sched[1].dbeta or sched[1].bn_reduce)


def test_deterministic_record_names_the_forms(monkeypatch):
    plan = _plan(D.DW_SEP, monkeypatch, det=True)
    rec = plan.deterministic['layers']
    assert rec[2]['wgrad'][0] == 'depthwise' and rec[2]['wgrad'][2] >= 1 and rec[2]['dgrad'] == 'depthwise'
    assert rec[4]['wgrad'][0] == 'depthwise' and rec[4]['dgrad'] == 'depthwise-stride2'
    assert rec[2]['bn_sums'].startswith('consumer-dgrad') and rec[3]['wgrad'][0] == 'direct-ordered'
    assert plan.deterministic['taken_back'] == []


def test_yolo_pose_cfg_is_untouched_by_the_feature(monkeypatch):
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    _no_launch(monkeypatch)
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg'))
    plan = engine.Plan(model, 1, 416, 416, torch.device('cpu'))
    assert plan.depthwise == [] and not any(cs.depthwise for cs in plan.convs.values())
    assert all(m[0].groups == 1 for m in model.models if isinstance(m, torch.nn.Sequential))


# ---------------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize('rid,body,channels,pattern', D.REFUSED, ids=[r[0] for r in D.REFUSED])
def test_refused_when_the_plan_is_built(rid, body, channels, pattern, monkeypatch):
    """(groups=2 on 8 channels used to build - silently, as a dense convolution.)"""
    from singleshotpose_amd import engine
    _no_launch(monkeypatch)
    case = T.Case('refused_' + rid, 'dw', body, 2, 8, 8, channels, 1)
    with pytest.raises(NotImplementedError, match=pattern):
        model = D.make_model(case, init=False)
        engine.Plan(model, case.B, case.H, case.W, torch.device('cpu'))


# ---------------------------------------------------------------------------------------------------- 5. seeds
@pytest.mark.parametrize('case', D.FLOAT, ids=ids(D.FLOAT))
def test_float_seed_keeps_every_decision_margin(case):
    m, d = D.margins(case, D.seed_of(case))
    print('DW %s seed %d margin %.3e diff %.3e' % (case.id, D.seed_of(case), m, d))
    assert m >= 4.0 * d
    assert D.find_seed(case) == D.seed_of(case)
    r64, r32 = D.reference(case, D.seed_of(case))
    assert set(r64.grads) == set('models.' + n for n, _ in D.make_model(case, init=False).models.named_parameters())
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in r64.grads.values())


def test_reference_honours_groups():
    """ref_forward's depthwise layer is F.conv2d(groups=C) of the layer before it, channel by channel."""
    model = D.make_model(D.DW_BIAS)
    names, params, bufs = D.model_state(model, torch.float64)
    x = D.make_input(D.DW_BIAS, 0).double()
    _, outs = D.ref_forward(model.blocks, names, params, bufs, x, False)
    w, b = params['1.conv2.weight'], params['1.conv2.bias']
    for c in (0, 5):
        want = F.conv2d(outs[0][:, c:c + 1], w[c:c + 1], b[c:c + 1], padding=1)
        assert torch.equal(outs[1][:, c:c + 1], want)


def test_exact_net_is_exact_and_not_trivial():
    case = D.DW_EXACT
    assert D.exact_budget(case) < 2 ** 24
    r64, r32 = D.reference(case, 0)
    for a, b, what in [(r64.y_eval, r32.y_eval, 'y_eval'), (r64.y_train, r32.y_train, 'y_train'), (r64.dx, r32.dx, 'dx')] + \
            [(r64.grads[n], r32.grads[n], n) for n in r64.grads]:
        assert torch.equal(a.float(), b) and torch.equal(a, b.double()), what
    assert torch.equal(r64.y_eval, r64.y_train)
    assert float((r64.y_train != 0).double().mean()) >= 1 / 3.0 and float((r64.dx != 0).double().mean()) >= 0.1
    assert all(float(r64.grads[n].abs().max()) > 0 for n in ('models.2.conv2.weight', 'models.4.conv4.weight'))


# ---------------------------------------------------------------------------------------------------- 6. ABI, shipped cfg
def test_symbols_and_abi_version():
    from singleshotpose_amd import _lib
    P, I, F_, L = _lib.P, _lib.I, _lib.F, _lib.L
    assert _lib._SIGS['ssp_dwconv_fwd'] == [P] * 5 + [I] * 7 + [P]
    assert _lib._SIGS['ssp_dwconv_fwd_affine'] == [P] * 5 + [F_] + [I] * 7 + [P]
    assert _lib._SIGS['ssp_dwconv_dgrad'] == [P] * 3 + [I] * 8 + [P]
    assert _lib._SIGS['ssp_dwconv_wgrad'] == [P] * 3 + [I] * 8 + [P, L, P]
    names = ('ssp_dwconv_fwd', 'ssp_dwconv_fwd_affine', 'ssp_dwconv_stats_tile_m', 'ssp_dwconv_stats_tiles',
             'ssp_dwconv_stats_floats', 'ssp_dwconv_dgrad', 'ssp_dwconv_wgrad_workspace_floats', 'ssp_dwconv_wgrad')
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'ssp_hip.h')) as f:
        header = f.read()
    for name in names:
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert re.search(r'(int|int64_t) %s\(' % name, header), name
        assert _lib._SIGS[name] == [I] * 5 or not name.endswith(('tile_m', 'tiles', 'floats'))
    assert 'ssp_dwconv_stats_floats' in _lib._RET64 and 'ssp_dwconv_wgrad_workspace_floats' in _lib._RET64
    assert _lib.query('ssp_abi_version') == 5
    # the queries are pure host functions of the shape: the counted format, tiles of <= 64 strips of four output pixels
    assert _lib.query('ssp_dwconv_stats_tile_m', 2, 26, 26, 32, 1) == 0
    assert _lib.query('ssp_dwconv_stats_tiles', 2, 26, 26, 32, 1) == (2 * 26 * 7 + 63) // 64
    assert _lib.query('ssp_dwconv_stats_tiles', 1, 5, 5, 260, 2) == (3 * 1 + 14) // 15
    assert _lib.query('ssp_dwconv_stats_floats', 2, 26, 26, 32, 1) == 6 * 65
    assert _lib.query('ssp_dwconv_wgrad_workspace_floats', 2, 26, 26, 32, 1) % (32 * 9) == 0
    assert _lib.query('ssp_dwconv_wgrad_workspace_floats', 2, 26, 26, 32, 1) // (32 * 9) > 1
    assert _lib.query('ssp_dwconv_stats_tiles', 2, 26, 26, 30, 1) == 0 and _lib.query('ssp_dwconv_stats_tiles', 2, 26, 26, 32, 3) == 0


def test_shipped_cfg_is_yolo_pose_with_separable_blocks():
    from singleshotpose_amd.cfg import layer_shapes, parse_cfg
    base, sep = (parse_cfg(os.path.join(ROOT, 'cfg', n)) for n in ('yolo-pose.cfg', 'yolo-pose-dw.cfg'))
    assert sep[0] == base[0] and sep[1] == base[1] and sep[-2:] == base[-2:]      # [net], block 0, the head conv, the region block
    want = []
    for i, b in enumerate(base[1:]):
        if b['type'] == 'convolutional' and int(b['size']) == 3 and i > 0:
            want += ['dw', 'pw']
        else:
            want.append(b['type'])
    got, prev_c = [], 3
    shapes = layer_shapes(sep)
    for i, b in enumerate(sep[1:]):
        if b['type'] == 'convolutional' and 'groups' in b:
            assert int(b['groups']) == int(b['filters']) == prev_c and int(b['size']) == 3 and int(b['stride']) == 1
            assert int(b['batch_normalize']) == 1 and b['activation'] == 'leaky' and prev_c % 4 == 0
            got.append('dw')
        elif b['type'] == 'convolutional' and got and got[-1] == 'dw':
            assert int(b['size']) == 1 and int(b['batch_normalize']) == 1 and b['activation'] == 'leaky'
            got.append('pw')
        else:
            assert not (b['type'] == 'convolutional' and int(b['size']) == 3 and i > 0)
            got.append(b['type'])
        prev_c = shapes[i][2]
    assert got == want
    # the renumbered routes reach the maps the old ones did: 26 x 26 x 512, then 13 x 13 x (256 + 1024)
    assert shapes[38] == (26, 26, 512) and shapes[41] == (13, 13, 1280) and shapes[44] == (13, 13, 20)
    assert layer_shapes(base)[-2] == shapes[-2]

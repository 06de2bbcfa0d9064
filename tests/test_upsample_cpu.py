"""The [upsample] block without a GPU: cfg surface, module tree, .weights I/O, the shared references of
tests/upsample_cases.py against torch's own nearest-neighbour interpolation, the plan a Plan builds for every net (on the CPU
device: nothing is launched), every refusal, the seed conditions of the float and the exact nets, and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import topology_cases as T
import upsample_cases as U

ids = lambda cases: [c.id for c in cases]


def _write(tmp_path, text, name='n.cfg'):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


# ---------------------------------------------------------------------------------------------------- 1. cfg surface
def test_parse_layer_shapes_and_print(tmp_path, capsys):
    from singleshotpose_amd.cfg import layer_shapes, parse_cfg, print_cfg
    blocks = parse_cfg(_write(tmp_path, T.cfg_text(U.UP_NET)))
    assert [b['type'] for b in blocks[1:]] == ['convolutional', 'maxpool', 'convolutional', 'maxpool', 'convolutional',
                                               'convolutional', 'upsample', 'route', 'convolutional', 'convolutional', 'region']
    assert blocks[7] == {'type': 'upsample', 'stride': '2'}
    shapes = layer_shapes(blocks)
    assert shapes[5] == (8, 8, 16) and shapes[6] == (16, 16, 16) and shapes[7] == (16, 16, 32) and shapes[9] == (16, 16, 20)
    assert layer_shapes(blocks, 48, 64)[6] == (24, 32, 16)
    print_cfg(blocks)
    out = capsys.readouterr().out
    assert 'unknown type' not in out
    line = [l for l in out.splitlines() if 'upsample' in l]
    assert line == ['    6 upsample           * 2     8 x   8 x  16   ->    16 x  16 x  16'], line
    # the default stride is Darknet's 2; stride 4 multiplies by 4; the channel count never moves
    d = parse_cfg(_write(tmp_path, T.cfg_text(T.Case('d', 'up', T.conv(8) + '[upsample]\n\n' + T.head(8), 1, 8, 12, 3, 0)), 'd.cfg'))
    assert layer_shapes(d)[1] == (24, 16, 8)
    assert layer_shapes(parse_cfg(_write(tmp_path, T.cfg_text(U.UP_S4), 's4.cfg')))[5] == (32, 32, 16)


def test_scale_other_than_one_is_refused_by_name(tmp_path):
    from singleshotpose_amd.cfg import layer_shapes, parse_cfg
    from singleshotpose_amd.darknet import Darknet
    text = T.cfg_text(T.Case('s', 'up', T.conv(8) + '[upsample]\nstride=2\nscale=0.5\n\n' + T.head(8), 1, 8, 8, 3, 0))
    path = _write(tmp_path, text)
    with pytest.raises(NotImplementedError, match=r'block 1 \(upsample\): scale=0\.5'):
        layer_shapes(parse_cfg(path))
    with pytest.raises(NotImplementedError, match=r'block 1 \(upsample\): scale=0\.5'):
        Darknet(path)
    ok = _write(tmp_path, text.replace('scale=0.5', 'scale=1'), 'ok.cfg')
    assert layer_shapes(parse_cfg(ok))[1] == (16, 16, 8)


# ---------------------------------------------------------------------------------------------------- 2. module tree
def test_module_tree_and_state_dict_alignment():
    from singleshotpose_amd.darknet import EmptyModule, Upsample, _HipOnly
    assert issubclass(Upsample, _HipOnly)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dropin', 'darknet.py')) as f:
        assert re.search(r'from singleshotpose_amd\.darknet import \([^)]*\bUpsample\b', f.read())      # the drop-in re-exports it
    model = U.make_model(U.UP_NET, init=False)
    assert len(model.models) == len(model.blocks) - 1
    up = model.models[6]
    assert isinstance(up, Upsample) and up.stride == 2 and list(up.parameters()) == []
    with pytest.raises(RuntimeError, match='Upsample is executed by the HIP plan'):
        up(torch.zeros(1, 4, 2, 2))
    assert isinstance(model.models[7], EmptyModule)
    assert U.make_model(U.UP_S4, init=False).models[5].stride == 4
    keys = list(model.state_dict().keys())
    # the blocks behind the upsample keep their own indices (8: the fifth conv, reading 16 + 16 channels; 9: the head)
    assert 'models.8.conv5.weight' in keys and 'models.9.conv6.bias' in keys and not any(k.startswith('models.6.') for k in keys)
    assert tuple(model.models[8][0].weight.shape) == (16, 32, 3, 3)
    assert model.models[10] is model.loss and model.num_anchors == 1


def test_unknown_block_keeps_the_indices_aligned(tmp_path, capsys):
    from singleshotpose_amd.darknet import Darknet, EmptyModule
    text = T.cfg_text(T.Case('u', 'up', T.conv(8) + '[crop]\n\n' + T.head(8), 1, 8, 8, 3, 0))
    model = Darknet(_write(tmp_path, text))
    assert 'unknown type crop' in capsys.readouterr().out
    assert len(model.models) == 3 and isinstance(model.models[1], EmptyModule)
    assert 'models.2.conv2.weight' in model.state_dict() and tuple(model.models[2][0].weight.shape) == (8, 8, 1, 1)


# ---------------------------------------------------------------------------------------------------- 3. .weights
def test_weights_round_trip(tmp_path):
    a, b = U.make_model(U.UP_NET), U.make_model(U.UP_NET, init=False)
    path = str(tmp_path / 'up.weights')
    a.save_weights(path)
    n = sum(t.numel() for k, t in a.state_dict().items() if 'num_batches' not in k)
    assert os.path.getsize(path) == 16 + 4 * n          # header + every parameter and running statistic, nothing for the block
    b.load_weights(path)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        if 'num_batches' not in k:
            assert torch.equal(sa[k], sb[k]), k


# ---------------------------------------------------------------------------------------------------- 4. / 5. references
@pytest.mark.parametrize('n', [1, 2, 3, 4, 8])
def test_numpy_reference_against_interpolate_and_autograd(n):
    rs = np.random.RandomState(n)
    x = rs.randint(-8, 9, (2, 3, 5, 4)).astype(np.float32)          # (B, H, W, C)
    g = rs.randint(-8, 9, (2, 3 * n, 5 * n, 4)).astype(np.float32)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).double().requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=n, mode='nearest')
    y = U.up_fwd_ref(x, n)
    assert y.shape == (2, 3 * n, 5 * n, 4) and y.dtype == np.float32
    assert np.array_equal(y, yt.detach().permute(0, 2, 3, 1).numpy().astype(np.float32))
    for b, yy, xx, c in [(0, 0, 0, 0), (1, 3 * n - 1, 5 * n - 1, 3), (1, n, 2 * n - 1, 2)]:
        assert y[b, yy, xx, c] == x[b, yy // n, xx // n, c]
    (yt * torch.from_numpy(g).permute(0, 3, 1, 2).double()).sum().backward()
    want = xt.grad.permute(0, 2, 3, 1).numpy()
    # integers: the float32 sum in the documented order IS the float64 sum, with and without accumulation
    assert np.array_equal(U.up_bwd_ref(g, n).astype(np.float64), want)
    assert np.array_equal(U.up_bwd_ref(g, n, x).astype(np.float64), want + x)
    # and the order is the documented one: row-major, sequential, the earlier content added last
    gf = rs.standard_normal(g.shape).astype(np.float32)
    s = gf[:, 0::n, 0::n].copy()
    for k in range(1, n * n):
        s = (s + gf[:, k // n::n, k % n::n]).astype(np.float32)
    assert np.array_equal(U.up_bwd_ref(gf, n), s) and np.array_equal(U.up_bwd_ref(gf, n, x), (x + s).astype(np.float32))
    assert np.abs(U.up_bwd_ref(gf, n).astype(np.float64) - gf.astype(np.float64).reshape(2, 3, n, 5, n, 4).sum((2, 4))).max() < 1e-4


def test_reference_net_is_interpolate_and_cat():
    """ref_forward of UP_NET: layer 6 is F.interpolate of layer 5, layer 7 their concatenation with the lateral map, and the
    gradient the upsample hands to layer 5 is the 2 x 2 window sum of the first 16 channels of layer 7's gradient."""
    model = U.make_model(U.UP_NET)
    names, params, bufs = U.model_state(model, torch.float64)
    x = U.make_input(U.UP_NET, 1).double()
    y, outs = U.ref_forward(model.blocks, names, params, bufs, x, True)
    assert tuple(y.shape) == (2, 20, 16, 16) and tuple(outs[6].shape) == (2, 16, 16, 16) and tuple(outs[7].shape) == (2, 32, 16, 16)
    assert torch.equal(outs[6], outs[5][:, :, torch.arange(16) // 2][:, :, :, torch.arange(16) // 2])
    assert torch.equal(outs[7][:, :16], outs[6]) and torch.equal(outs[7][:, 16:], outs[2])
    for i in (5, 7):
        outs[i].retain_grad()
    (y * U.make_probe(U.UP_NET, 1, y.shape).double()).sum().backward()
    win = outs[7].grad[:, :16].reshape(2, 16, 8, 2, 8, 2).sum((3, 5))
    assert float((outs[5].grad - win).abs().max()) <= 1e-12 * float(win.abs().max())


# ---------------------------------------------------------------------------------------------------- 6. plans
def _no_launch(monkeypatch):
    from singleshotpose_amd import _lib

    def call(name, *args):
        raise AssertionError("planning launched %s" % name)
    monkeypatch.setattr(_lib, 'call', call)


def _plan(case, monkeypatch, fuse=None, shape=None):
    from singleshotpose_amd import engine
    if fuse is None:
        monkeypatch.delenv('SSP_UPSAMPLE_FUSE', raising=False)
    else:
        monkeypatch.setenv('SSP_UPSAMPLE_FUSE', fuse)
    _no_launch(monkeypatch)
    B, H, W = shape or (case.B, case.H, case.W)
    return engine.Plan(U.make_model(case, init=False), B, H, W, torch.device('cpu'))


@pytest.mark.parametrize('case', U.NETS, ids=ids(U.NETS))
def test_plan_of_every_net(case, monkeypatch):
    for fuse in (None, '0'):
        plan = _plan(case, monkeypatch, fuse)
        want = U.FORMS[case.id] if fuse is None else {l: 'own' for l in U.FORMS[case.id]}
        assert plan.upsample == want, (case.id, fuse, plan.upsample)
        kinds = {op.ind: op.kind for op in plan.ops}
        for l, form in want.items():
            op = [o for o in plan.ops if o.ind == l][0]
            n = int(plan.net.blocks[l + 1]['stride'])
            src, out = op.srcs[0], op.out
            assert kinds[l] == 'upsample' and op.stride == n
            assert (out.C, out.H, out.W) == (src.C, n * src.H, n * src.W) and out.producer == l and plan.acts[l] is out
            assert plan.shapes[l] == (out.W, out.H, out.C)
            if form == 'route':
                cat = [o for o in plan.ops if o.ind == l + 1][0]
                assert cat.kind == 'concat' and cat.inplace and cat.srcs[0] is out
                assert out.t is cat.out.t and out.off == 0 and out.ld == cat.out.C == cat.out.ld == out.C + cat.srcs[1].C
                assert out.t.numel() == plan.B * out.H * out.W * cat.out.C
            else:
                assert out.ld == T._pad4(out.C) and out.off == 0 and out.t.numel() == plan.B * out.H * out.W * out.ld
                nxt = [o for o in plan.ops if o.ind == l + 1]
                assert not (nxt and nxt[0].kind == 'concat' and nxt[0].inplace)
        # what the form costs: the fused plan holds one fine map less
        if fuse is None:
            fused_bytes = plan.footprint()
        elif 'route' in U.FORMS[case.id].values():
            l = [k for k, v in U.FORMS[case.id].items() if v == 'route'][0]
            a = plan.acts[l]
            assert plan.footprint() - fused_bytes == 4 * plan.B * a.H * a.W * a.ld
        else:
            assert plan.footprint() == fused_bytes


def test_plan_consumers_and_schedule_of_up_net(monkeypatch):
    plan = _plan(U.UP_NET, monkeypatch)
    assert plan.consumers[5] == [6] and plan.consumers[6] == [7] and plan.consumers[2] == [3, 7] and plan.fused_pool == {1}
    assert [op.kind for op in plan.ops] == ['conv', 'conv', 'maxpool', 'conv', 'conv', 'upsample', 'concat', 'conv', 'conv']
    sched = {s.ind: s for s in plan.backward_schedule()}
    assert sched[6].visited and sched[6].dgrad == (True,) and sched[7].dgrad == (True, True)
    # everything below the upsample frozen: the block gets no backward launch
    head = set(id(p) for i in (8, 9) for p in plan.net.models[i].parameters())
    sched = {s.ind: s for s in plan.backward_schedule(head, bn_training=False)}
    assert not sched[6].visited and not sched[7].visited and sched[8].visited and sched[8].dgrad == (False,) and sched[8].wgrad
    # ... unless the input wants its gradient
    sched = {s.ind: s for s in plan.backward_schedule(head, want_input=True, bn_training=False)}
    assert sched[6].visited and sched[6].dgrad == (True,)


def test_second_shape_gives_the_same_record(monkeypatch):
    for shape in ((1, 32, 32), (2, 48, 64)):
        plan = _plan(U.UP_NET, monkeypatch, shape=shape)
        assert plan.upsample == {6: 'route'} and plan.acts[6].H == shape[1] // 2 and plan.acts[6].W == shape[2] // 2


def test_stride_one_is_an_alias(monkeypatch):
    case = T.Case('s1', 'up', T.conv(8) + U.up(1) + T.head(8), 2, 8, 8, 3, 1)
    plan = _plan(case, monkeypatch)
    assert plan.upsample == {1: 'alias'} and [op.kind for op in plan.ops] == ['conv', 'alias', 'conv']
    assert plan.acts[1] is plan.acts[0] and plan.acts[1].producer == 0


def test_further_consumer_or_odd_channels_keep_the_standalone_form(monkeypatch):
    # the upsampled map is read again by a later route: the route behind it is not its only consumer
    again = T.Case('again', 'up', T.conv(8) + T.pool() + T.conv(8) + U.up() + T.route(-1, -4) + T.conv(8) + T.route(3) + T.head(8),
                   2, 8, 8, 3, 1)
    plan = _plan(again, monkeypatch)
    assert plan.upsample == {3: 'own'} and plan.consumers[3] == [4, 6]
    # a 6-channel upsample in front of the route: refused by the route's own rule, in either form
    odd = T.Case('odd', 'up', T.conv(8) + T.pool() + T.conv(6) + U.up() + T.route(-1, -4) + T.head(8), 2, 8, 8, 3, 1)
    with pytest.raises(NotImplementedError, match=r'block 4 \(route\): concatenates layer 3 with 6 channels'):
        _plan(odd, monkeypatch)


# ---------------------------------------------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize('rid,body,pattern', U.REFUSED, ids=[r[0] for r in U.REFUSED])
def test_refused_when_the_plan_is_built(rid, body, pattern, monkeypatch):
    from singleshotpose_amd import engine
    _no_launch(monkeypatch)
    case = T.Case('refused_' + rid, 'up', body, 2, 8, 8, 3, 1)
    with pytest.raises(NotImplementedError, match=pattern):
        model = U.make_model(case, init=False)
        engine.Plan(model, case.B, case.H, case.W, torch.device('cpu'))


# ---------------------------------------------------------------------------------------------------- 8. seeds
@pytest.mark.parametrize('case', U.FLOAT, ids=ids(U.FLOAT))
def test_float_seed_keeps_every_decision_margin(case):
    m, d = U.margins(case, U.seed_of(case))
    print('UP %s seed %d margin %.3e diff %.3e' % (case.id, U.seed_of(case), m, d))
    assert m >= 4.0 * d
    assert U.find_seed(case) == U.seed_of(case)
    r64, r32 = U.reference(case, U.seed_of(case))
    assert set(r64.grads) == set('models.' + n for n, _ in U.make_model(case, init=False).models.named_parameters())
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in r64.grads.values())


def test_exact_net_is_exact_and_not_trivial():
    case = U.UP_EXACT
    assert U.exact_budget(case) < 2 ** 24
    r64, r32 = U.reference(case, 0)
    for a, b, what in [(r64.y_eval, r32.y_eval, 'y_eval'), (r64.y_train, r32.y_train, 'y_train'), (r64.dx, r32.dx, 'dx')] + \
            [(r64.grads[n], r32.grads[n], n) for n in r64.grads]:
        assert torch.equal(a.float(), b) and torch.equal(a, b.double()), what
    assert torch.equal(r64.y_eval, r64.y_train)
    assert float((r64.y_train != 0).double().mean()) >= 1 / 3.0 and float((r64.dx != 0).double().mean()) >= 0.1


# ---------------------------------------------------------------------------------------------------- 9. ABI
def test_symbols_and_abi_version():
    from singleshotpose_amd import _lib
    assert _lib._SIGS['ssp_upsample_fwd'] == [_lib.P, _lib.I, _lib.P, _lib.I] + [_lib.I] * 5 + [_lib.P]
    assert _lib._SIGS['ssp_upsample_bwd'] == [_lib.P, _lib.I, _lib.P, _lib.I] + [_lib.I] * 6 + [_lib.P]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('ssp_upsample_fwd', 'ssp_upsample_bwd'):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
    assert _lib.query('ssp_abi_version') == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'ssp_hip.h')) as f:
        header = f.read()
    assert re.search(r'int ssp_upsample_fwd\(const float\* src, int lds, float\* dst, int ldd, int C, int B, int H, int W, '
                     r'int stride, void\* stream\);', header)
    assert re.search(r'int ssp_upsample_bwd\(const float\* g, int ldg, float\* dsrc, int ldds, int C, int B, int H, int W, '
                     r'int stride,\s+int accumulate, void\* stream\);', header)


def test_shipped_cfg_moves_the_head_to_the_finer_grid(monkeypatch):
    from singleshotpose_amd.cfg import layer_shapes, parse_cfg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base, up = (parse_cfg(os.path.join(root, 'cfg', n)) for n in ('yolo-pose.cfg', 'yolo-pose-up.cfg'))
    assert up[:30] == base[:30] and up[-2:] == base[-2:]            # the trunk through layer 28, the head conv and the region block
    assert [b['type'] for b in up[30:-2]] == ['convolutional', 'convolutional', 'upsample', 'route', 'convolutional']
    shapes = layer_shapes(up)
    assert shapes[30] == (13, 13, 256) and shapes[31] == (26, 26, 256) and shapes[32] == (26, 26, 768) and shapes[34] == (26, 26, 20)
    for side in range(224, 833, 32):                                 # the 20 multi-scale shapes: at most 52 x 52 = 2704 cells
        w, h, c = layer_shapes(up, side, side)[34]
        assert (w, h, c) == (side // 16, side // 16, 20) and w * h <= 4096

"""The [upsample] block on the MI355X: the two kernels of csrc/upsample.hip through the C ABI against the numpy reference of
tests/upsample_cases.py (bit for bit: the forward is a copy, the backward's add order is part of the contract), and every net
of that module through Darknet + engine.Plan against its float64 CPU reference - eval and training forward, running
statistics, dL/dx and every parameter gradient at the bars of tests/test_gpu_topology.py: max(floor, 3 x the float32 CPU
reference's own distance to float64), floors 1e-4 (outputs, dL/dx) and 3e-4 (parameter gradients); the exact-integer net bit
for bit.  Then the plan's other routes through the block: written into the route's buffer against a buffer of its own, the
region loss on the finer grid, a frozen trunk, the input-only backward, graph replay, the reproducible mode, a second shape,
and the shipped cfg.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import topology_cases as T
import upsample_cases as U
from exact_conv import first_diffs
from helpers import make_targets, rel_err

pytestmark = pytest.mark.gpu
FLOOR_Y, FLOOR_G = 1e-4, 3e-4
ids = lambda cases: [c.id for c in cases]
NAN = float('nan')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------- kernels, C ABI
def _sides(k):
    """(ld, off) of the coarse and of the fine map of a kernel case."""
    sl = (k.ld or k.C, k.off)
    return ((k.C, 0), sl) if k.side == 'fine' else (sl, (k.C, 0))


@pytest.mark.parametrize('k', U.KERNEL_CASES, ids=U.kcase_id)
def test_forward_is_a_copy(k):
    from singleshotpose_amd import _lib
    (ldc, offc), (ldf, offf) = _sides(k)
    x = U.kernel_data(k, False)[0]
    src = _dev(U.embed(x, ldc, offc))
    fine = np.zeros((k.B, k.H * k.stride, k.W * k.stride, k.C), np.float32)
    dst = _dev(U.embed(fine, ldf, offf, fill=NAN))
    _lib.call('ssp_upsample_fwd', src.data_ptr() + 4 * offc, ldc, dst.data_ptr() + 4 * offf, ldf, k.C, k.B, k.H, k.W, k.stride, _st())
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(U.embed(U.up_fwd_ref(x, k.stride), ldf, offf)))      # values and every sentinel column
    assert np.array_equal(_bits(src.cpu().numpy()), _bits(U.embed(x, ldc, offc)))


@pytest.mark.parametrize('integer', [True, False], ids=['int', 'float'])
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('k', U.KERNEL_CASES, ids=U.kcase_id)
def test_backward_sums_in_the_documented_order(k, accumulate, integer):
    from singleshotpose_amd import _lib
    (ldc, offc), (ldf, offf) = _sides(k)
    _, g, pre = U.kernel_data(k, integer)
    gd = _dev(U.embed(g, ldf, offf))
    dsrc = _dev(U.embed(pre, ldc, offc, fill=None if accumulate else NAN))
    _lib.call('ssp_upsample_bwd', gd.data_ptr() + 4 * offf, ldf, dsrc.data_ptr() + 4 * offc, ldc, k.C, k.B, k.H, k.W, k.stride,
              accumulate, _st())
    torch.cuda.synchronize()
    want = U.up_bwd_ref(g, k.stride, pre if accumulate else None)
    got = dsrc.cpu().numpy()
    diff = np.abs(got[:, offc:offc + k.C].reshape(want.shape).astype(np.float64) - want.astype(np.float64)).max()
    print('UPK %s acc %d %s maxabs %.3e' % (U.kcase_id(k), accumulate, 'int' if integer else 'float', diff))
    assert np.array_equal(_bits(got), _bits(U.embed(want, ldc, offc)))
    assert np.array_equal(_bits(gd.cpu().numpy()), _bits(U.embed(g, ldf, offf)))
    if integer:      # ... which on integers is the float64 sum
        w64 = g.astype(np.float64).reshape(k.B, k.H, k.stride, k.W, k.stride, k.C).sum((2, 4)) + (pre if accumulate else 0)
        assert np.array_equal(want.astype(np.float64), w64)


BAD = [   # (what, C, lds, ldd, B, H, W, stride, source pointer offset in bytes, destination pointer offset in bytes)
    ('C not a multiple of 4', 6, 8, 8, 1, 2, 2, 2, 0, 0),
    ('source stride not a multiple of 4', 4, 6, 8, 1, 2, 2, 2, 0, 0),
    ('destination stride below C', 8, 8, 4, 1, 2, 2, 2, 0, 0),
    ('stride 0', 4, 4, 4, 1, 2, 2, 0, 0, 0),
    ('stride 9', 4, 4, 4, 1, 2, 2, 9, 0, 0),
    ('empty batch', 4, 4, 4, 0, 2, 2, 2, 0, 0),
    ('2^31 destination pixels', 4, 4, 4, 1 << 13, 1 << 8, 1 << 8, 2, 0, 0),
    ('unaligned source', 4, 8, 8, 1, 2, 2, 2, 4, 0),
    ('unaligned destination', 4, 8, 8, 1, 2, 2, 2, 0, 8),
    ('null source', 4, 4, 4, 1, 2, 2, 2, None, 0),
]


@pytest.mark.parametrize('bad', BAD, ids=[b[0].replace(' ', '_') for b in BAD])
def test_out_of_range_arguments_are_refused(bad):
    from singleshotpose_amd import _lib
    what, C, lds, ldd, B, H, W, n, so, do = bad
    a = torch.full((1024,), U.SENTINEL, dtype=torch.float32, device='cuda')
    b = torch.full((1024,), U.SENTINEL, dtype=torch.float32, device='cuda')
    ap = None if so is None else a.data_ptr() + so
    for name, args in (('ssp_upsample_fwd', (ap, lds, b.data_ptr() + do, ldd, C, B, H, W, n, _st())),
                       ('ssp_upsample_bwd', (ap, lds, b.data_ptr() + do, ldd, C, B, H, W, n, 0, _st())),
                       ('ssp_upsample_bwd', (ap, lds, b.data_ptr() + do, ldd, C, B, H, W, n, 1, _st()))):
        with pytest.raises(_lib.SspError, match='upsample_'):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert bool((a == U.SENTINEL).all()) and bool((b == U.SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- nets
def _poison():
    """NaNs in the caching allocator's free blocks: what a plan allocates with torch.empty and never writes reads as NaN."""
    t = torch.full((16 << 20,), NAN, dtype=torch.float32, device='cuda')
    del t


def _model(case, monkeypatch, fuse=None):
    monkeypatch.setenv('SSP_AUTOTUNE', '0')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    if fuse is None:
        monkeypatch.delenv('SSP_UPSAMPLE_FUSE', raising=False)
    else:
        monkeypatch.setenv('SSP_UPSAMPLE_FUSE', fuse)
    return U.make_model(case).cuda()


def _plan_of(model, case):
    return model._plans[(case.B, case.H, case.W, 0)]


def _check(case, what, got, want64, want32, floor):
    err, own = rel_err(got, want64.numpy()), rel_err(want32.numpy(), want64.numpy())
    bar = max(floor, 3.0 * own)
    print('UP %s %s err %.3e ref32 %.3e bar %.3e' % (case.id, what, err, own, bar))
    assert tuple(got.shape) == tuple(want64.shape), (case.id, what, got.shape, want64.shape)
    assert err <= bar, (case.id, what, err, bar)      # (a NaN fails: not <=)


def _padding_is_zero(model, case):
    """The padding channels [C, ld) of every map the plan allocated with torch.zeros are still exactly zero (their consumers
    read them as Cin padding): an upsample that wrote or summed the wrong columns of a padded map shows here."""
    plan = _plan_of(model, case)
    n = 0
    for ind, a in enumerate(plan.acts):
        if a is not None and a.off == 0 and a.C % 4 and a.ld == T._pad4(a.C) and a.t.numel() % a.ld == 0:
            assert not bool(a.t.view(-1, a.ld)[:, a.C:].ne(0).any()), (case.id, ind, 'padding channels written')
            n += 1
    return n


def _eval(model, case, seed):
    r64, r32 = U.reference(case, seed)
    model.eval()
    _poison()
    with torch.no_grad():
        y = model(U.make_input(case, seed).cuda())
    _check(case, 'y_eval', y.cpu().numpy(), r64.y_eval, r32.y_eval, FLOOR_Y)
    return y.cpu()


def _train_step(model, case, seed, stats=True, params=True):
    """One training forward + backward of (y * probe).sum() against the reference; returns (y, dL/dx)."""
    r64, r32 = U.reference(case, seed)
    model.train()
    model.zero_grad(set_to_none=True)
    xg = U.make_input(case, seed).cuda().requires_grad_(True)
    _poison()
    y = model(xg)
    _check(case, 'y_train', y.detach().cpu().numpy(), r64.y_train, r32.y_train, FLOOR_Y)
    if stats:
        for n, b in model.named_buffers():
            if 'running' in n:
                print('UP %s stat:%s maxabs %.3e' % (case.id, n, float((b.cpu().double() - r64.stats[n]).abs().max())))
                np.testing.assert_allclose(b.cpu().numpy(), r64.stats[n].numpy(), rtol=1e-4, atol=1e-5, err_msg=n)
    _poison()
    (y * U.make_probe(case, seed, y.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    _check(case, 'dx', xg.grad.cpu().numpy(), r64.dx, r32.dx, FLOOR_Y)
    for n, p in model.named_parameters():
        if not params:
            assert p.grad is None, n
        else:
            assert p.grad is not None, (case.id, n)
            _check(case, 'grad:' + n, p.grad.cpu().numpy(), r64.grads[n], r32.grads[n], FLOOR_G)
    return y.detach().cpu(), xg.grad.detach().cpu()


@pytest.mark.parametrize('fuse', [None, '0'], ids=['fused', 'own'])
@pytest.mark.parametrize('case', U.FLOAT, ids=ids(U.FLOAT))
def test_float_net(case, fuse, monkeypatch):
    model = _model(case, monkeypatch, fuse)
    seed = U.seed_of(case)
    _eval(model, case, seed)
    _train_step(model, case, seed)
    want = U.FORMS[case.id] if fuse is None else {l: 'own' for l in U.FORMS[case.id]}
    assert _plan_of(model, case).upsample == want
    assert _padding_is_zero(model, case) or case.id not in ('up_pad', 'up_input')


@pytest.mark.parametrize('fuse', [None, '0'], ids=['fused', 'own'])
def test_exact_net_equals_float64(fuse, monkeypatch):
    """Integer data below the 2^24 budget: fp32 is exact in any summation order, so the product's numbers ARE float64's."""
    case = U.UP_EXACT
    model = _model(case, monkeypatch, fuse)
    r64, _ = U.reference(case, 0)
    x = U.make_input(case, 0).cuda()
    model.eval()
    _poison()
    with torch.no_grad():
        y_eval = model(x).cpu()
    model.train()
    xg = x.clone().requires_grad_(True)
    _poison()
    y = model(xg)
    _poison()
    (y * U.make_probe(case, 0, y.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert _plan_of(model, case).upsample == ({6: 'route'} if fuse is None else {6: 'own'})
    for what, got, want in [('y_eval', y_eval, r64.y_eval), ('y_train', y.detach().cpu(), r64.y_train),
                            ('dx', xg.grad.cpu(), r64.dx)]:
        assert torch.equal(got, want.float()), (what, first_diffs(got, want.float(), ('b', 'c', 'y', 'x')))
    for n, p in model.named_parameters():
        got, want = p.grad.cpu().contiguous(), r64.grads[n].float()
        assert torch.equal(got, want), (n, first_diffs(got, want, ('co', 'ci', 'ky', 'kx')[:got.dim()]))


def _record(monkeypatch):
    from singleshotpose_amd import _lib
    log = []
    orig = _lib.call

    def rec(name, *args):
        log.append(name)
        return orig(name, *args)
    monkeypatch.setattr(_lib, 'call', rec)
    return log


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
def test_fused_against_standalone(det, monkeypatch):
    """The same arithmetic at other addresses: one ssp_copy_channels less in each direction, otherwise the same launches, and
    bitwise the same y and dL/dx in either mode.  Every parameter gradient is bitwise the same in the reproducible mode.  In
    the default mode the filter gradients are summed in an order the hardware decides, so two runs of
    ONE form already differ there (measured on the MI355X: two runs of the fused form differ in 136 of the 216 elements of
    models.0.conv1.weight.grad and in 1662 of models.8.conv5.weight.grad, the two forms in 162 and 1935, all at 1.4e-7 of the
    tensor's largest element or less): there the third run below - the fused form again - is printed next to the
    comparison, and the gradients of both forms are held to the float64 reference by test_float_net."""
    case, seed = U.UP_NET, U.seed_of(U.UP_NET)
    runs = []
    log = _record(monkeypatch)
    for fuse in (None, '0', None):
        model = _model(case, monkeypatch, fuse)
        model.deterministic = det
        model.train()
        xg = U.make_input(case, seed).cuda().requires_grad_(True)
        del log[:]
        y = model(xg)
        (y * U.make_probe(case, seed, y.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((y.detach().cpu(), xg.grad.cpu(), {n: p.grad.cpu().contiguous() for n, p in model.named_parameters()},
                     list(log)))
        assert _plan_of(model, case).upsample == {6: 'route' if fuse is None else 'own'}
    (ya, dxa, ga, la), (yb, dxb, gb, lb), (yc, dxc, gc, _) = runs
    print('UP fused/own copy_channels %d / %d, upsample fwd %d / %d, bwd %d / %d' % (
        la.count('ssp_copy_channels'), lb.count('ssp_copy_channels'), la.count('ssp_upsample_fwd'), lb.count('ssp_upsample_fwd'),
        la.count('ssp_upsample_bwd'), lb.count('ssp_upsample_bwd')))
    assert la.count('ssp_copy_channels') == 2 and lb.count('ssp_copy_channels') == 4
    for l in (la, lb):
        assert l.count('ssp_upsample_fwd') == 1 and l.count('ssp_upsample_bwd') == 1
    assert [n for n in la if n != 'ssp_copy_channels'] == [n for n in lb if n != 'ssp_copy_channels']
    for n in ga:
        print('UP %s %s: fused vs own %d elements differ (rel %.2e), fused vs fused again %d' % (
            'deterministic' if det else 'default', n, int((ga[n] != gb[n]).sum()), rel_err(ga[n].numpy(), gb[n].numpy()),
            int((ga[n] != gc[n]).sum())))
    assert torch.equal(ya, yb), first_diffs(ya, yb, ('b', 'c', 'y', 'x'))
    assert torch.equal(dxa, dxb), first_diffs(dxa, dxb, ('b', 'c', 'y', 'x'))
    assert torch.equal(ya, yc) and torch.equal(dxa, dxc)
    if det:
        for n in ga:
            assert torch.equal(ga[n], gb[n]), (n, first_diffs(ga[n], gb[n], ('co', 'ci', 'ky', 'kx')[:ga[n].dim()]))


def test_region_loss_on_the_finer_grid(monkeypatch):
    from singleshotpose_amd.region_loss import RegionLoss
    from singleshotpose_amd.utils import get_region_boxes
    case = U.UP_NET
    model = _model(case, monkeypatch).train()
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.uniform(0, 1, (2, 3, 32, 32)).astype(np.float32)).cuda().requires_grad_(True)
    tgt = torch.from_numpy(make_targets(rs, 2, [1, 1]))
    out = model(x)
    assert tuple(out.shape) == (2, 20, 16, 16)
    loss = RegionLoss()(out, tgt, 20)
    loss.backward()
    torch.cuda.synchronize()
    print('UP region loss %.6f' % float(loss))
    assert np.isfinite(float(loss)) and float(loss) > 0
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    box = get_region_boxes(out.detach(), 1, 9)
    assert len(box) == 21 and all(np.isfinite(float(v)) for v in box)


def _trunk_bn_eval(model):
    for ind in range(6):
        m = model.models[ind]
        if isinstance(m, torch.nn.Sequential) and len(m) > 1 and isinstance(m[1], torch.nn.BatchNorm2d):
            m[1].eval()


def test_frozen_trunk_launches_no_upsample_backward(monkeypatch):
    """Layers 0-5 (everything below the upsample) with their BatchNorm in eval(): with their parameters frozen as well the
    backward stops at the route - no ssp_upsample_bwd - and the head's gradients are those of the run that went all the way."""
    case, seed = U.UP_NET, U.seed_of(U.UP_NET)
    model = _model(case, monkeypatch)
    model.deterministic = True          # (the two runs are compared bit for bit)
    model.train()
    _trunk_bn_eval(model)
    x = U.make_input(case, seed).cuda()

    def step():
        model.zero_grad(set_to_none=True)
        y = model(x)
        (y * U.make_probe(case, seed, y.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}

    log = _record(monkeypatch)
    full = step()
    assert log.count('ssp_upsample_fwd') == 1 and log.count('ssp_upsample_bwd') == 1
    assert len(full) == len(list(model.parameters()))
    for ind in range(6):
        for p in model.models[ind].parameters():
            p.requires_grad_(False)
    del log[:]
    head = step()
    assert log.count('ssp_upsample_fwd') == 1 and log.count('ssp_upsample_bwd') == 0 and log.count('ssp_copy_channels') == 1, log
    assert sorted(head) == sorted(n for n in full if n.startswith('models.8.') or n.startswith('models.9.'))
    for n in head:
        assert torch.equal(head[n], full[n]), (n, first_diffs(head[n], full[n], ('co', 'ci', 'ky', 'kx')[:head[n].dim()]))


@pytest.mark.parametrize('case', [U.UP_NET, U.UP_SHARED, U.UP_INPUT], ids=ids([U.UP_NET, U.UP_SHARED, U.UP_INPUT]))
def test_input_only_backward_gives_the_same_dx(case, monkeypatch):
    model = _model(case, monkeypatch)
    seed = U.seed_of(case)
    _, full = _train_step(model, case, seed, stats=False)
    for p in model.parameters():
        p.requires_grad_(False)
    # (the running statistics moved, the batch statistics the training forward normalises with did not)
    _, only = _train_step(model, case, seed, stats=False, params=False)
    err = rel_err(only.numpy(), full.numpy())
    print('UP %s dx_only_vs_full err %.3e' % (case.id, err))
    assert err <= FLOOR_Y


@pytest.mark.parametrize('case', [U.UP_NET, U.UP_LAST], ids=ids([U.UP_NET, U.UP_LAST]))
def test_graph_replay_equals_eager_eval(case, monkeypatch):
    model = _model(case, monkeypatch).eval()
    x = U.make_input(case, U.seed_of(case)).cuda()
    with torch.no_grad():
        model.graph_inference = False
        eager = model(x).cpu()
        model.graph_inference = True
        first = model(x).cpu()          # captures
        again = model(x).cpu()          # replays
    plan = _plan_of(model, case)
    assert plan._graph is not None and not plan._graph_failed
    assert torch.equal(first, eager) and torch.equal(again, eager)
    model.graph_inference = False


def test_deterministic_mode_repeats_bit_for_bit(monkeypatch):
    from singleshotpose_amd.optim import SGD
    case, seed = U.UP_NET, U.seed_of(U.UP_NET)
    runs = []
    for _ in range(2):
        model = _model(case, monkeypatch)
        model.deterministic = True
        model.train()
        opt = SGD(model.parameters(), lr=1e-2, momentum=0.9, dampening=0, weight_decay=5e-4)
        opt.zero_grad()
        xg = U.make_input(case, seed).cuda().requires_grad_(True)
        _poison()
        y = model(xg)
        (y * U.make_probe(case, seed, y.shape).cuda()).sum().backward()
        grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
        opt.step()
        torch.cuda.synchronize()
        assert _plan_of(model, case).deterministic['mode'] and _plan_of(model, case).upsample == {6: 'route'}
        runs.append((y.detach().cpu(), xg.grad.cpu(), grads, {n: p.detach().cpu().clone() for n, p in model.named_parameters()}))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n
        assert torch.equal(a[3][n], b[3][n]), n
        assert not torch.equal(a[3][n], U.make_model(case).state_dict()[n]), n          # the step moved the parameter


def test_second_batch_size_and_resolution(monkeypatch):
    """Another batch size and another (non-square) resolution on the same model: a plan each, the same record, and forwards
    at the bars (the forward is continuous in its decisions, so it needs no margin under the new data)."""
    case = U.UP_NET
    model = _model(case, monkeypatch)
    _train_step(model, case, U.seed_of(case))
    for v in (case._replace(id='up_net_b1', B=1), case._replace(id='up_net_res2', H=40, W=48)):
        fresh = U.make_model(v)
        with torch.no_grad():
            for (_, t), (_, s) in zip(model.named_buffers(), fresh.named_buffers()):
                t.copy_(s)
        r64, r32 = U.reference(v, 0)
        y = _eval(model, v, 0)
        assert tuple(y.shape) == (v.B, 20, v.H // 2, v.W // 2)
        model.train()
        with torch.no_grad():
            yt = model(U.make_input(v, 0).cuda())
        _check(v, 'y_train', yt.cpu().numpy(), r64.y_train, r32.y_train, FLOOR_Y)
        assert _plan_of(model, v).upsample == {6: 'route'}
    assert set(k[:3] for k in model._plans) == {(2, 32, 32), (1, 32, 32), (2, 40, 48)}


def test_shipped_cfg_trains_on_the_26_grid(monkeypatch):
    """cfg/yolo-pose-up.cfg at batch 2, 416 x 416: one training step with its RegionLoss; shapes and finiteness only."""
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.region_loss import RegionLoss
    monkeypatch.setenv('SSP_AUTOTUNE', '0')
    monkeypatch.delenv('SSP_TUNE_CACHE', raising=False)
    monkeypatch.delenv('SSP_UPSAMPLE_FUSE', raising=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    model = Darknet(os.path.join(root, 'cfg', 'yolo-pose-up.cfg')).cuda().train()
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, (2, 3, 416, 416)).astype(np.float32)).cuda()
    out = model(x)
    assert tuple(out.shape) == (2, 20, 26, 26)
    loss = RegionLoss()(out, torch.from_numpy(make_targets(rs, 2, [1, 1])), 20)
    loss.backward()
    torch.cuda.synchronize()
    plan = model._plans[(2, 416, 416, 0)]
    assert plan.upsample == {31: 'route'} and plan.acts[31].t is plan.acts[32].t and plan.acts[32].C == 768
    print('UP yolo-pose-up loss %.6f' % float(loss))
    assert np.isfinite(float(loss)) and bool(torch.isfinite(out).all())
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n

"""Darknet blocks outside the yolo-pose cfgs on the MI355X: the csrc/generic_blocks.hip kernels through the C ABI against
PyTorch on the CPU, and whole networks (tests/golden/generic-{pose,cls}.cfg) against the reference Darknet's goldens
(tools/gen_generic_blocks_golden.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLD, gold, make_targets, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


def _poisoned(rows, ld):
    return torch.full((rows, ld), float('nan'), dtype=torch.float32, device=torch.device('cuda', 0))


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('B,C,H,W,extra', [(2, 8, 5, 5, 4), (2, 12, 6, 4, 0), (1, 4, 1, 1, 0), (3, 8, 7, 6, 8),
                                           (1, 4, 13, 13, 0), (2, 16, 2, 3, 4)])
def test_maxpool_stride1_bit_exact(B, C, H, W, extra):
    """max_pool2d(pad(x, (0,1,0,1), 'replicate'), 2, stride=1): forward bit-exact; backward bit-exact on inputs quantised to
    three levels (real ties: the first maximum in row-then-column order takes the gradient), write and accumulate."""
    G, _lib = _imports()
    rs = np.random.RandomState(B * 1000 + C * 100 + H * 10 + W)
    x = torch.from_numpy(rs.randint(0, 3, (B, C, H, W)).astype(np.float32)).requires_grad_(True)
    y = F.max_pool2d(F.pad(x, (0, 1, 0, 1), mode='replicate'), 2, stride=1)
    g = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
    y.backward(g)
    ld = C + extra
    xd, gd = G.to_nhwc(x.detach(), ld=ld), G.to_nhwc(g, ld=ld)
    yd = _poisoned(B * H * W, ld)
    _lib.call('ssp_maxpool_s1_fwd', xd.data_ptr(), ld, yd.data_ptr(), ld, C, B, H, W, G.stream())
    assert torch.equal(G.from_nhwc(yd, B, C, H, W), y.detach())
    dx = _poisoned(B * H * W, ld)
    _lib.call('ssp_maxpool_s1_bwd', xd.data_ptr(), ld, gd.data_ptr(), ld, dx.data_ptr(), ld, C, B, H, W, 0, G.stream())
    assert torch.equal(G.from_nhwc(dx, B, C, H, W), x.grad)
    d0 = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
    dx = G.to_nhwc(d0, ld=ld)
    _lib.call('ssp_maxpool_s1_bwd', xd.data_ptr(), ld, gd.data_ptr(), ld, dx.data_ptr(), ld, C, B, H, W, 1, G.stream())
    assert torch.equal(G.from_nhwc(dx, B, C, H, W), d0 + x.grad)


@pytest.mark.parametrize('slope', [1.0, 0.1, 0.0])
@pytest.mark.parametrize('alias', [False, True])
def test_shortcut_bit_exact(slope, alias):
    """out = act(a + b), act = linear / leaky 0.1 / relu; backward g' = g * act'(out) from out > 0 into both summands'
    gradients (aliased a == b: 2 g'), written or accumulated."""
    G, _lib = _imports()
    rs = np.random.RandomState(int(slope * 10) + 7 * alias)
    B, C, H, W, lda, ldb, ldo = 2, 12, 5, 7, 16, 12, 20
    M = B * H * W
    a = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
    b = a if alias else torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
    s = a + b
    ref = s if slope == 1.0 else (F.leaky_relu(s, 0.1) if slope == 0.1 else F.relu(s))
    ad = G.to_nhwc(a, ld=lda)
    bd = ad if alias else G.to_nhwc(b, ld=ldb)
    ldb_ = lda if alias else ldb
    out = _poisoned(M, ldo)
    _lib.call('ssp_shortcut_fwd', ad.data_ptr(), lda, bd.data_ptr(), ldb_, out.data_ptr(), ldo, C, M, slope, G.stream())
    assert torch.equal(G.from_nhwc(out, B, C, H, W), ref)
    g = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
    gp = g if slope == 1.0 else torch.where(ref > 0, g, g * slope if slope else torch.zeros_like(g))
    gd = G.to_nhwc(g, ld=ldo)
    for acc_a, acc_b in ((0, 0), (1, 1)) if alias else ((0, 0), (1, 0), (0, 1), (1, 1)):
        d0a = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
        d0b = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
        da = G.to_nhwc(d0a, ld=lda) if acc_a else _poisoned(M, lda)
        db = da if alias else (G.to_nhwc(d0b, ld=ldb) if acc_b else _poisoned(M, ldb))
        _lib.call('ssp_shortcut_bwd', gd.data_ptr(), ldo, out.data_ptr(), ldo, da.data_ptr(), lda, acc_a, db.data_ptr(),
                  lda if alias else ldb, acc_b, C, M, slope, G.stream())
        if alias:
            assert torch.equal(G.from_nhwc(da, B, C, H, W), (d0a if acc_a else 0) + (gp + gp))
        else:
            assert torch.equal(G.from_nhwc(da, B, C, H, W), d0a + gp if acc_a else gp)
            assert torch.equal(G.from_nhwc(db, B, C, H, W), d0b + gp if acc_b else gp)


@pytest.mark.parametrize('H,W', [(1, 1), (7, 7), (13, 13), (26, 26)])
def test_avgpool(H, W):
    G, _lib = _imports()
    rs = np.random.RandomState(H)
    B, C, ld, ldo = 3, 72, 76, 80
    x = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
    xd = G.to_nhwc(x, ld=ld)
    out = _poisoned(B, ldo)
    _lib.call('ssp_avgpool_fwd', xd.data_ptr(), ld, out.data_ptr(), ldo, C, B, H, W, G.stream())
    ref = F.avg_pool2d(x.double(), (H, W)).view(B, C)
    assert rel_err(out.cpu()[:, :C].numpy(), ref.numpy()) < 1e-6
    again = _poisoned(B, ldo)
    _lib.call('ssp_avgpool_fwd', xd.data_ptr(), ld, again.data_ptr(), ldo, C, B, H, W, G.stream())
    assert torch.equal(again[:, :C], out[:, :C])          # fixed summation order
    # backward: g / (H * W) broadcast, bit-exact against avg_pool2d's own backward
    xr = x.clone().requires_grad_(True)
    g = torch.from_numpy(rs.standard_normal((B, C)).astype(np.float32))
    F.avg_pool2d(xr, (H, W)).view(B, C).backward(g)
    gd = torch.zeros(B, ldo, dtype=torch.float32, device=G.dev())
    gd[:, :C] = g.to(G.dev())
    dx = _poisoned(B * H * W, ld)
    _lib.call('ssp_avgpool_bwd', gd.data_ptr(), ldo, dx.data_ptr(), ld, C, B, H, W, 0, G.stream())
    assert torch.equal(G.from_nhwc(dx, B, C, H, W), xr.grad)
    d0 = torch.from_numpy(rs.standard_normal((B, C, H, W)).astype(np.float32))
    dx = G.to_nhwc(d0, ld=ld)
    _lib.call('ssp_avgpool_bwd', gd.data_ptr(), ldo, dx.data_ptr(), ld, C, B, H, W, 1, G.stream())
    assert torch.equal(G.from_nhwc(dx, B, C, H, W), d0 + xr.grad)


@pytest.mark.parametrize('C', [4, 10, 16, 1000, 1024])
@pytest.mark.parametrize('four_d', [False, True])
def test_softmax(C, four_d):
    """Softmax over channels of (B, C) rows and of NHWC pixels, entries up to +-80 (exp overflows without the row maximum
    subtracted): forward within 2e-6 of float64; backward y * (g - sum g y), written and accumulated."""
    G, _lib = _imports()
    rs = np.random.RandomState(C + 5 * four_d)
    shape = (2, C, 5, 3) if four_d else (64, C, 1, 1)
    B, _, H, W = shape
    ld = (C + 3) // 4 * 4 + 4
    x = torch.from_numpy(rs.uniform(-80, 80, shape).astype(np.float32))
    xd = G.to_nhwc(x, ld=ld)
    M = B * H * W
    y = _poisoned(M, ld)
    _lib.call('ssp_softmax_fwd', xd.data_ptr(), ld, y.data_ptr(), ld, C, M, G.stream())
    ref = torch.softmax(x.double(), dim=1)
    yg = G.from_nhwc(y, B, C, H, W)
    assert rel_err(yg.numpy(), ref.numpy()) < 2e-6
    assert torch.isnan(y.cpu()[:, C:]).all()             # channels past C are not written
    g = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    gd = G.to_nhwc(g, ld=ld)
    yd = G.to_nhwc(yg, ld=ld)
    y64 = yg.double()
    dref = y64 * (g.double() - (g.double() * y64).sum(1, keepdim=True))
    dx = _poisoned(M, ld)
    _lib.call('ssp_softmax_bwd', yd.data_ptr(), ld, gd.data_ptr(), ld, dx.data_ptr(), ld, C, M, 0, G.stream())
    assert rel_err(G.from_nhwc(dx, B, C, H, W).numpy(), dref.numpy()) < 1e-5
    d0 = torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    dx = G.to_nhwc(d0, ld=ld)
    _lib.call('ssp_softmax_bwd', yd.data_ptr(), ld, gd.data_ptr(), ld, dx.data_ptr(), ld, C, M, 1, G.stream())
    assert rel_err(G.from_nhwc(dx, B, C, H, W).numpy(), (d0.double() + dref).numpy()) < 1e-5


# ---------------------------------------------------------------------------------------------------- whole networks
CFGS = {'pose': ('generic-pose.cfg', 2, 80, 80), 'cls': ('generic-cls.cfg', 4, 64, 64)}


def _golden_model(tag, tmp_path):
    from singleshotpose_amd.darknet import Darknet
    g = gold('generic_%s.npz' % tag)
    p = str(tmp_path / ('%s.weights' % tag))
    with open(p, 'wb') as f:
        f.write(g['weights'].tobytes())
    model = Darknet(os.path.join(GOLD, CFGS[tag][0]))
    model.load_weights(p)
    return model.cuda(), g


def _grad_stats(model, g):
    """Per-parameter distances to the golden's float64 gradients: (norm error, element error) of this run and of the
    reference's own fp32 run (as tests/test_gpu_darknet.py)."""
    dn_mine, dn_ref, de_mine, de_ref = [], [], [], []
    for n, p in model.named_parameters():
        gr = p.grad.detach().cpu().numpy()
        n64, n32 = float(g['g64norm/' + n][0]), float(g['gnorm/' + n][0])
        got = float(np.sqrt((gr.astype(np.float64) ** 2).sum()))
        if 'g64/' + n in g.files:
            ref64, ref32, mine = g['g64/' + n], g['grad/' + n], gr
        else:
            ref64, ref32 = g['g64slice/' + n], g['gslice/' + n]
            k = len(ref64)
            mine = gr.reshape(-1)[:: max(1, gr.size // k)][:k]
        dn_mine.append(abs(got / n64 - 1)); dn_ref.append(abs(n32 / n64 - 1))
        de_mine.append(rel_err(mine, ref64)); de_ref.append(rel_err(ref32, ref64))
    return dn_mine, dn_ref, de_mine, de_ref


@pytest.mark.parametrize('tag', sorted(CFGS))
def test_network_matches_reference(tag, tmp_path):
    model, g = _golden_model(tag, tmp_path)
    x = torch.from_numpy(g['x']).cuda()
    model.eval()
    with torch.no_grad():
        y = model(x)
    assert tuple(y.shape) == tuple(g['y_eval'].shape) and y.is_contiguous()
    assert rel_err(y.cpu().numpy(), g['y_eval']) < TOL
    model.train()
    y = model(x)
    assert tuple(y.shape) == tuple(g['y_train'].shape)
    assert rel_err(y.detach().cpu().numpy(), g['y_train']) < TOL
    for n, b in model.named_buffers():
        if 'running' in n:
            np.testing.assert_allclose(b.cpu().numpy(), g['buf/' + n], rtol=1e-4, atol=1e-5)
    (y * torch.from_numpy(g['probe']).cuda()).sum().backward()
    assert all(p.grad is not None for p in model.parameters())
    dn_mine, dn_ref, de_mine, de_ref = _grad_stats(model, g)
    envelope = max(3.0 * max(de_ref), 3e-4), max(3.0 * max(dn_ref), 3e-4)
    assert max(de_mine) <= envelope[0] and max(dn_mine) <= envelope[1], (max(de_mine), max(dn_mine), max(de_ref), max(dn_ref))


def test_classifier_sgd_step_matches_torch_sgd(tmp_path):
    """One fused singleshotpose_amd.optim.SGD step on the classifier moves every parameter - the Linear ones included - as
    torch.optim.SGD does on the same gradients."""
    from singleshotpose_amd.optim import SGD
    model, g = _golden_model('cls', tmp_path)
    model.train()
    kw = dict(lr=1e-2, momentum=0.9, dampening=0, weight_decay=5e-4)
    opt = SGD(model.parameters(), **kw)
    shadow = [torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters()]
    sopt = torch.optim.SGD(shadow, **kw)
    opt.zero_grad()
    y = model(torch.from_numpy(g['x']).cuda())
    (y * torch.from_numpy(g['probe']).cuda()).sum().backward()
    for p, q in zip(model.parameters(), shadow):
        q.grad = p.grad.detach().cpu().clone()
    before = [p.detach().cpu().clone() for p in model.parameters()]
    opt.step()
    sopt.step()
    names = [n for n, _ in model.named_parameters()]
    for n, p, q, p0 in zip(names, model.parameters(), shadow, before):
        assert not torch.equal(p.detach().cpu(), p0), n
        assert rel_err(p.detach().cpu().numpy(), q.detach().numpy()) < 1e-6, n
    assert opt.fused_steps == 1
    # the next forward sees the moved Linear weights
    with torch.no_grad():
        y2 = model.eval()(torch.from_numpy(g['x']).cuda())
    assert not torch.equal(y2.cpu(), torch.from_numpy(g['y_eval']))


def test_pose_train_step_with_region_loss(tmp_path):
    """generic-pose.cfg with the product's RegionLoss: one training step gives a finite loss and finite gradients."""
    from singleshotpose_amd.region_loss import RegionLoss
    model, g = _golden_model('pose', tmp_path)
    model.train()
    B = 2
    rs = np.random.RandomState(3)
    tgt = torch.from_numpy(make_targets(rs, B, [1] * B))
    crit = RegionLoss()
    crit.verbose = False
    out = model(torch.from_numpy(g['x']).cuda())
    loss = crit(out, tgt, 20)
    loss.backward()
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert any(float(p.grad.abs().max()) > 0 for p in model.parameters())

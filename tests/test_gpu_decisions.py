"""Per-element decisions of the BatchNorm + leaky + max-pool family, pinned with exact-arithmetic data.

Every kernel of that family decides, per element, which side of zero scale*raw + shift falls on and which of four
pixels wins a pooled window.  The other test files feed continuous random data (no ties, no zeros) with positive scales,
and the network-level tests hand the oracle the product's own decisions - so a wrong decision is invisible there.  Here
the inputs sit on coarse dyadic grids (tests/exact_data.py): every intermediate is exactly representable in fp32, fp32
and float64 agree on every decision, ties and y == 0 are frequent, scales are negative, zero and positive inside every
group of four channels, the reference is plain torch float64 autograd taking its OWN decisions, and results are compared
bit for bit (torch.equal).  Where one rounding is unavoidable the bar is derived: slope 0.1 is not dyadic, the kernels
form fl32(y * fl32(0.1)) - relative error <= 2^-24 + |fl32(0.1) / 0.1 - 1| = 7.5e-8 < 1.3 fp32 spacings - bar 2 ulp.
Sums over pixels (dgamma, dbeta, partial rows, filter gradients) keep the 1e-4 / 2e-4 bars of the other kernel tests.
X.assert_exact runs on the float64 reference before any launch: a badly built case is a construction error."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_data as X
from helpers import rel_err

pytestmark = pytest.mark.gpu

DYADIC = (1.0, 0.0, 0.125)
SLOPES = (0.1, 1.0, 0.0, 0.125)


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


def _same(got32, ref64, slope, what):
    """Bit-exact for a dyadic slope, within 2 ulp (one rounding of y * 0.1f, see the module docstring) for 0.1."""
    if slope in DYADIC:
        assert torch.equal(got32.double(), ref64), '%s: %d elements differ' % (what, int((got32.double() != ref64).sum()))
    else:
        assert X.ulp_diff(got32, ref64) <= 2.0, what


def _vecs(G, *vs):
    """Per-channel float64 vectors -> rows of one device buffer (rows 16-byte aligned: channel counts are multiples of 4)."""
    buf = torch.stack([v.float() for v in vs]).contiguous().to(G.dev())
    return [buf[i] for i in range(len(vs))]


# ------------------------------------------------------------------------------------------------ 1. bn_act.hip
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("C,B,H,W,ld,off", [(c, b, h, w, c, 0) for c, b, h, w in X.BN_SHAPES] + [(24, 2, 6, 10, 40, 8)])
def test_bn_act_exact(C, B, H, W, ld, off, pool, slope):
    """ssp_bn_act_fwd / ssp_bn_act_bwd (two-pass, in place, single-pass), training 0 and 1, on exact data.  scale / shift /
    mean / invstd are inputs of the ABI and are passed straight in."""
    G, _lib = _imports()
    d = X.bn_case(C, B, H, W, pool)
    sc, sh, mu, istd = d['scale'], d['shift'], d['mean'], d['invstd']
    y, out = X.block_ref(d['raw'], sc, sh, slope, pool)
    out.backward(d['g'])
    dy = y.grad
    if slope in DYADIC:
        X.assert_exact(out, 1.0 / 32)
        X.assert_exact(X.per_channel(sc) * dy, 1.0 / 16)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    M = B * H * W
    st = G.stream()
    scd, shd, mud, isd = _vecs(G, sc, sh, mu, istd)
    xd = G.to_nhwc(d['raw'].float(), ld, off)
    gd = G.to_nhwc(d['g'].float(), ld, off)
    od = torch.full((B * Ho * Wo, ld), float('nan'), device=G.dev())
    _lib.call('ssp_bn_act_fwd', G.p(xd, off), ld, G.p(od, off), ld, scd.data_ptr(), shd.data_ptr(), C, B, H, W, pool, slope, st)
    torch.cuda.synchronize()
    _same(G.from_nhwc(od, B, C, Ho, Wo, off), out.detach(), slope, 'forward')
    if ld > C:
        o = od.cpu()
        assert torch.isnan(o[:, :off]).all() and torch.isnan(o[:, off + C:]).all()

    xhat = (d['raw'] - X.per_channel(mu)) * X.per_channel(istd)
    dbeta, dgamma = dy.sum(dim=(0, 2, 3)), (dy * xhat).sum(dim=(0, 2, 3))
    nblk = _lib.query('ssp_bn_bwd_blocks')
    for training in (0, 1):
        c1, c2 = (dbeta / M, dgamma / M) if training else (torch.zeros(C, dtype=torch.float64),) * 2
        dx_ref = X.per_channel(sc) * (dy - X.per_channel(c1) - xhat * X.per_channel(c2))

        def check(dxbuf, dgam, dbet, what):
            got = G.from_nhwc(dxbuf, B, C, H, W, off)
            if training:
                assert rel_err(got.numpy(), dx_ref.numpy()) < 2e-4, what
            else:       # dx = scale * dy: sign and winner of every element, ties and zeros included
                _same(got, dx_ref, slope, what)
            assert rel_err(dgam.cpu().numpy(), dgamma.numpy()) < 1e-4, what
            assert rel_err(dbet.cpu().numpy(), dbeta.numpy()) < 1e-4, what

        partial = torch.empty(nblk * C * 2, device=G.dev())
        vec = torch.zeros(4, C, device=G.dev())
        dx = torch.full((M, ld), float('nan'), device=G.dev())
        _lib.call('ssp_bn_act_bwd', G.p(xd, off), ld, G.p(gd, off), ld, G.p(dx, off), ld, scd.data_ptr(), shd.data_ptr(),
                  mud.data_ptr(), isd.data_ptr(), C, B, H, W, pool, slope, training, partial.data_ptr(), vec[0].data_ptr(),
                  vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), st)
        torch.cuda.synchronize()
        check(dx, vec[0], vec[1], 'two-pass, training=%d' % training)
        x2 = xd.clone()                                                                  # in place, as the engine runs it
        _lib.call('ssp_bn_act_bwd', G.p(x2, off), ld, G.p(gd, off), ld, G.p(x2, off), ld, scd.data_ptr(), shd.data_ptr(),
                  mud.data_ptr(), isd.data_ptr(), C, B, H, W, pool, slope, training, partial.data_ptr(), vec[0].data_ptr(),
                  vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), st)
        torch.cuda.synchronize()
        assert torch.equal(x2[:, off:off + C], dx[:, off:off + C])
        x3 = xd.clone()                                                                  # single pass (partial = NULL)
        acc = torch.zeros(2, C, device=G.dev())
        _lib.call('ssp_bn_act_bwd', G.p(x3, off), ld, G.p(gd, off), ld, G.p(x3, off), ld, scd.data_ptr(), shd.data_ptr(),
                  mud.data_ptr(), isd.data_ptr(), C, B, H, W, pool, slope, training, None, acc[0].data_ptr(),
                  acc[1].data_ptr(), None, None, st)
        torch.cuda.synchronize()
        check(x3, acc[0], acc[1], 'single-pass, training=%d' % training)


# ------------------------------------------------------------------------------------------------ 2. first block
@pytest.mark.parametrize("B,H,W", X.FIRST_SHAPES)
def test_first_block_exact(B, H, W):
    """conv_first.hip: raw map, forward apply, and the three backward passes, each of which recomputes the convolution and
    re-derives leaky signs and pool winners.  With c1 = c2 = 0 the input gradient is conv_transpose(scale * leaky' *
    scatter(g)) and exact: a wrong tie-break or a transposed window order in bwd_dgrad moves whole elements."""
    G, _lib = _imports()
    d = X.first_case(B, H, W)
    x, w, sc, sh, mu, istd, g = d['x'], d['w'], d['scale'], d['shift'], d['mean'], d['invstd'], d['g']
    raw = X.conv_exact(x, w, 0.25, 0.125)
    X.assert_exact(raw * X.per_channel(sc) + X.per_channel(sh), 1.0 / 64)
    xhat = (raw - X.per_channel(mu)) * X.per_channel(istd)
    st = G.stream()
    M, P = B * H * W, B * (H // 2) * (W // 2)
    xp = torch.zeros(B, 4, H, W)
    xp[:, :3] = x.float()
    xdev = G.to_nhwc(xp)
    wdev = G.pack_fwd(w.float(), 4)
    scd, shd, mud, isd, c1d, c2d, zero = _vecs(G, sc, sh, mu, istd, d['c1'], d['c2'], torch.zeros(32, dtype=torch.float64))
    rawdev = torch.full((M, 36), float('nan'), device=G.dev())
    _lib.call('ssp_first_conv_raw', xdev.data_ptr(), wdev.data_ptr(), rawdev.data_ptr(), 36, B, H, W, st)
    torch.cuda.synchronize()
    assert torch.equal(G.from_nhwc(rawdev, B, 32, H, W).double(), raw)
    ldo = 40
    gdev = G.to_nhwc(g.float(), ldo)
    groups = _lib.query('ssp_first_groups', B, H, W)
    wsn = _lib.query('ssp_first_wgrad_workspace_floats', B, H, W)
    for slope in SLOPES:
        y, out = X.block_ref(raw, sc, sh, slope, 1)
        out.backward(g)
        dy = y.grad
        odev = torch.full((P, ldo), float('nan'), device=G.dev())
        _lib.call('ssp_first_fwd_apply', xdev.data_ptr(), wdev.data_ptr(), scd.data_ptr(), shd.data_ptr(), slope,
                  odev.data_ptr(), ldo, B, H, W, st)
        torch.cuda.synchronize()
        _same(G.from_nhwc(odev, B, 32, H // 2, W // 2), out.detach(), slope, 'fwd_apply slope %g' % slope)
        # bwd_reduce -> finalize: the sums of the reference's own dy
        partial = torch.full((groups * 64,), float('nan'), device=G.dev())
        _lib.call('ssp_first_bwd_reduce', xdev.data_ptr(), wdev.data_ptr(), gdev.data_ptr(), ldo, scd.data_ptr(), shd.data_ptr(),
                  mud.data_ptr(), isd.data_ptr(), slope, partial.data_ptr(), B, H, W, st)
        torch.cuda.synchronize()
        ps = partial.cpu().double().view(groups, 32, 2).sum(0)
        dbeta, dgamma = dy.sum(dim=(0, 2, 3)), (dy * xhat).sum(dim=(0, 2, 3))
        assert rel_err(ps[:, 0].numpy(), dbeta.numpy()) < 1e-4 and rel_err(ps[:, 1].numpy(), dgamma.numpy()) < 1e-4
        fin = torch.zeros(4, 32, device=G.dev())
        _lib.call('ssp_bn_bwd_finalize', partial.data_ptr(), groups, 32, M, 1, 0, fin[0].data_ptr(), fin[1].data_ptr(),
                  fin[2].data_ptr(), fin[3].data_ptr(), st)
        torch.cuda.synchronize()
        assert rel_err(fin[0].cpu().numpy(), dgamma.numpy()) < 1e-4 and rel_err(fin[1].cpu().numpy(), dbeta.numpy()) < 1e-4
        assert rel_err(fin[2].cpu().numpy(), (dbeta / M).numpy()) < 1e-4 and rel_err(fin[3].cpu().numpy(), (dgamma / M).numpy()) < 1e-4
        for k1d, k2d, k1, k2 in ((zero, zero, torch.zeros(32, dtype=torch.float64), torch.zeros(32, dtype=torch.float64)),
                                 (c1d, c2d, d['c1'], d['c2'])):
            nonzero = bool(k1.abs().max() > 0)
            dx_raw = X.per_channel(sc) * (dy - X.per_channel(k1) - xhat * X.per_channel(k2))
            exact = slope in DYADIC and not nonzero
            if exact:
                dx_ref = X.conv_exact(dx_raw, w, 1.0 / 16, 0.125, transpose=True)
            else:
                dx_ref = F.conv_transpose2d(dx_raw, w, None, padding=1)
            dw_ref = torch.nn.grad.conv2d_weight(x, w.shape, dx_raw, padding=1)
            res = []
            for _ in range(2):
                dx = torch.full((M, 4), float('nan'), device=G.dev())
                _lib.call('ssp_first_bwd_dgrad', xdev.data_ptr(), wdev.data_ptr(), gdev.data_ptr(), ldo, scd.data_ptr(),
                          shd.data_ptr(), mud.data_ptr(), isd.data_ptr(), k1d.data_ptr(), k2d.data_ptr(), slope, dx.data_ptr(),
                          B, H, W, st)
                dw = torch.full((32 * 36,), float('nan'), device=G.dev())
                wsp = torch.full((wsn,), float('nan'), device=G.dev())
                _lib.call('ssp_first_bwd_wgrad', xdev.data_ptr(), wdev.data_ptr(), gdev.data_ptr(), ldo, scd.data_ptr(),
                          shd.data_ptr(), mud.data_ptr(), isd.data_ptr(), k1d.data_ptr(), k2d.data_ptr(), slope, dw.data_ptr(),
                          wsp.data_ptr(), wsn, B, H, W, st)
                torch.cuda.synchronize()
                res.append((dx.cpu(), dw.cpu()))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])      # run twice: bitwise equal
            dxc, dwc = res[0]
            assert float(dxc[:, 3].abs().max()) == 0.0
            got = dxc[:, :3].reshape(B, H, W, 3).permute(0, 3, 1, 2)
            what = 'bwd_dgrad slope %g, c1/c2 %s' % (slope, 'dyadic' if nonzero else '0')
            if exact:
                assert torch.equal(got.double(), dx_ref), '%s: %d elements differ' % (what, int((got.double() != dx_ref).sum()))
            else:
                assert rel_err(got.numpy(), dx_ref.numpy()) < 1e-4, what
            dwp = dwc.view(32, 9, 4)
            assert float(dwp[:, :, 3].abs().max()) == 0.0
            got_dw = dwp[:, :, :3].permute(0, 2, 1).reshape(32, 3, 3, 3)
            assert rel_err(got_dw.numpy(), dw_ref.numpy()) < 2e-4, what.replace('bwd_dgrad', 'bwd_wgrad')


# ------------------------------------------------------------------------------------ 3. conv epilogues on exact data
WINO, WINO4, FUSED = 9006413, 8006413, 7000001


def _operand(G, _lib, packed, rows, K, plan):
    """The filter operand of a plan: the packed filters, or their Winograd transform for a 9xxxxxx / 8xxxxxx / 7000001 code."""
    tile = _lib.query('ssp_conv_plan_wino_tile', plan)
    if not tile:
        return packed
    U = torch.empty((tile + 2) ** 2 * rows * K, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_wino_filter_transform_t', packed.data_ptr(), U.data_ptr(), rows, K, tile, G.stream())
    return U


def _conv_exact_any(x64, w64, gx, gw, plan, transpose=False):
    """The float64 convolution, asserted exact for the evaluation the plan runs.  A direct plan sums products on the grid
    gx * gw.  F(2x2, 3x3) forms U = G g G^T (entries of G: 1, 1/2 - grid gw / 4, |U| <= 9/4 max|g|), V = B^T d B (four
    signed terms, |V| <= 4 max|d|) and sums nine transform-domain products per output: grid gx * gw / 4 and at most
    81 * K * max|d| * max|g| per sum of |terms|.  F(4x4) has thirds in its transforms: not exact (returns False)."""
    pad = w64.shape[-1] // 2
    op = F.conv_transpose2d if transpose else F.conv2d
    out = op(x64, w64, None, padding=pad)
    if plan // 1000000 == 8:
        return out, False
    if plan // 1000000 in (9, 7):
        K = w64.shape[0] if transpose else w64.shape[1]
        X.assert_exact(out, gx * gw / 4, 81.0 * K * float(x64.abs().max()) * float(w64.abs().max()))
    else:
        X.assert_exact(out, gx * gw, op(x64.abs(), w64.abs(), None, padding=pad).max())
    return out, True


DGRAD_CASES = [
    # B, H, W, Cdy, Cdx, R, plan
    (4, 13, 13, 64, 128, 3, 0),            # direct epilogue
    (4, 13, 13, 128, 64, 1, 0),            # 1 x 1
    (16, 13, 13, 512, 256, 3, 12834),      # split-K x3: the sums come out of the partial-sum pass
    (16, 52, 52, 128, 256, 3, 306413),     # hybrid launch: epilogue (un-split tiles) + tail pass
    (2, 13, 13, 20, 1024, 1, 0),           # the head's data gradient (20 channels)
    (2, 13, 13, 256, 128, 3, WINO),        # Winograd F(2x2) finishing pass, odd map
    (2, 13, 13, 256, 128, 3, WINO4),       # F(4x4): thirds in the transforms, compared at the Winograd file's 1e-4
    (3, 10, 14, 128, 256, 3, FUSED),       # on-chip F(2x2)
]


@pytest.mark.parametrize("B,H,W,Cdy,Cdx,R,plan", DGRAD_CASES)
def test_conv_dgrad_bnbwd_exact(B, H, W, Cdy, Cdx, R, plan):
    """ssp_conv_dgrad_bnbwd: the data gradient bit for bit, and the (sum dy', sum dy' * xhat) rows - whose leaky sign every
    epilogue re-derives from the producer's raw map - against float64 sums with the reference's own signs; plain-store and
    atomic-fold forms of the rows."""
    G, _lib = _imports()
    rs = X.rng(B, H, W, Cdy, Cdx, R, plan + 1)
    M = B * H * W
    dy = X.sparse_map(rs, (B, Cdy, H, W))
    wt = X.filters(rs, Cdy, Cdx, R, denom=4, kmax=2)
    raw = X.int_map(rs, (B, Cdx, H, W), -4, 4)
    sc, sh, mu, istd = X.scale(rs, Cdx), X.shift(rs, Cdx), X.mean(rs, Cdx), X.invstd(rs, Cdx)
    g_ref, exact = _conv_exact_any(dy, wt, 1.0, 0.25, plan, transpose=True)
    y = raw * X.per_channel(sc) + X.per_channel(sh)
    X.assert_exact(y, 0.25)
    assert float((y == 0).double().mean()) >= 0.01
    xhat = (raw - X.per_channel(mu)) * X.per_channel(istd)
    coutp = (Cdy + 3) // 4 * 4
    dyp = torch.zeros(B, coutp, H, W)
    dyp[:, :Cdy] = dy.float()
    dyd = G.to_nhwc(dyp)
    wd = _operand(G, _lib, G.pack_dgrad(wt.float(), coutp), Cdx, coutp, plan)
    rawdev = G.to_nhwc(raw.float())
    scd, shd, mud, isd = _vecs(G, sc, sh, mu, istd)
    ntile = _lib.query('ssp_conv_stats_tiles', B, H, W, coutp, Cdx, R, plan)
    wsn = max(1, _lib.query('ssp_conv_workspace_floats', B, H, W, coutp, Cdx, R, plan))
    ws = torch.empty(wsn, device=G.dev())
    for slope in (0.1, 0.125, 0.0, 1.0):        # 0 = relu: the sharpest detector of y == 0 handling
        dyq = torch.where(y > 0, g_ref, g_ref * slope)
        s1, s2 = dyq.sum(dim=(0, 2, 3)), (dyq * xhat).sum(dim=(0, 2, 3))
        for rows in sorted({ntile, min(ntile, 3)}):          # ntile rows: plain stores; 3 rows: tiles folded with atomics
            partial = torch.zeros(rows * Cdx * 2, device=G.dev())
            gx = torch.full((M, Cdx), float('nan'), device=G.dev())
            _lib.call('ssp_conv_dgrad_bnbwd', dyd.data_ptr(), wd.data_ptr(), gx.data_ptr(), B, H, W, coutp, Cdx, coutp, Cdx, R,
                      plan, ws.data_ptr(), wsn, rawdev.data_ptr(), Cdx, scd.data_ptr(), shd.data_ptr(), mud.data_ptr(),
                      isd.data_ptr(), slope, partial.data_ptr(), rows, G.stream())
            torch.cuda.synchronize()
            got = G.from_nhwc(gx, B, Cdx, H, W)
            if exact:
                assert torch.equal(got.double(), g_ref), '%d elements differ' % int((got.double() != g_ref).sum())
            else:
                assert rel_err(got.numpy(), g_ref.numpy()) < 1e-4
            ps = partial.cpu().double().view(rows, Cdx, 2).sum(0)
            what = 'slope %g, %d rows for %d tiles' % (slope, rows, ntile)
            assert rel_err(ps[:, 0].numpy(), s1.numpy()) < 1e-4, what
            assert rel_err(ps[:, 1].numpy(), s2.numpy()) < 1e-4, what


AFFINE_CASES = [
    # B, H, W, Cin, Cout, R, plan
    (2, 13, 13, 64, 128, 3, 0),
    (3, 10, 14, 128, 256, 3, 12834),
    (16, 52, 52, 128, 256, 3, 306413),
    (2, 9, 9, 64, 20, 1, 0),               # the 20-channel head
    (2, 10, 12, 128, 64, 1, 0),            # 1 x 1
    (1, 12, 12, 3, 32, 3, 0),              # first layer (4-channel kernel)
    (1, 21, 21, 128, 256, 3, WINO),
    (1, 21, 21, 128, 256, 3, WINO4),
    (1, 21, 21, 128, 256, 3, FUSED),
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,R,plan", AFFINE_CASES)
def test_conv_fwd_affine_exact(B, H, W, Cin, Cout, R, plan):
    """ssp_conv_fwd_affine = leaky(scale * conv + shift): every epilogue's leaky sign, mixed-sign / zero scales, y == 0."""
    G, _lib = _imports()
    rs = X.rng(B, H, W, Cin, Cout, R, plan + 1, 1)
    x = X.sparse_map(rs, (B, Cin, H, W))
    w = X.filters(rs, Cout, Cin, R, denom=4, kmax=2)
    sc, sh = X.scale(rs, Cout), X.shift(rs, Cout)
    conv, exact = _conv_exact_any(x, w, 1.0, 0.25, plan)
    cinp = (Cin + 3) // 4 * 4
    xp = torch.zeros(B, cinp, H, W)
    xp[:, :Cin] = x.float()
    xd = G.to_nhwc(xp)
    wd = _operand(G, _lib, G.pack_fwd(w.float(), cinp), Cout, cinp, plan)
    wsn = max(1, _lib.query('ssp_conv_workspace_floats', B, H, W, cinp, Cout, R, plan))
    ws = torch.empty(wsn, device=G.dev())
    scd, shd = _vecs(G, sc, sh)
    for with_scale in (True, False):
        y = (conv * X.per_channel(sc) if with_scale else conv) + X.per_channel(sh)
        X.assert_exact(y, 1.0 / 32)
        assert float((y == 0).double().mean()) > 0.002
        for slope in (0.1, 1.0, 0.0):
            ref = X.leaky(y, slope)
            out = torch.full((B * H * W, Cout), float('nan'), device=G.dev())
            _lib.call('ssp_conv_fwd_affine', xd.data_ptr(), wd.data_ptr(), out.data_ptr(), scd.data_ptr() if with_scale else None,
                      shd.data_ptr(), slope, B, H, W, cinp, Cout, cinp, Cout, R, plan, ws.data_ptr(), wsn, G.stream())
            torch.cuda.synchronize()
            got = G.from_nhwc(out, B, Cout, H, W)
            what = 'slope %g, scale %s' % (slope, 'given' if with_scale else 'NULL')
            if exact:
                _same(got, ref, slope, what)
            else:
                assert rel_err(got.numpy(), ref.numpy()) < 1e-4, what


# ------------------------------------------------------------------------------ 4. statistics under a common offset
# floor of the variance bar: 3 x the largest err_kernel measured on the MI355X (1.490e-05, the split-K producer; table in
# profiles/r08_decisions.txt), below the cap of 1e-3.  A sum / sum-of-squares formulation is off by ~6e-2 on such data.
STATS_FLOOR = 4.5e-5

STATS_CASES = [
    # producer, B, H, W, Cin, Cout, R, plan     (every producer has a case whose M is ragged against its tile)
    ('direct', 2, 13, 13, 64, 128, 3, 0),
    ('split-K', 3, 10, 14, 128, 256, 3, 12834),
    ('hybrid', 16, 52, 52, 128, 256, 3, 306413),      # 676 whole 64-row tiles
    ('hybrid', 15, 52, 52, 128, 256, 3, 306413),      # 633 tiles + 48 rows: the ragged tile is in the split tail
    ('thin split', 1, 42, 42, 512, 64, 1, 0),
    ('Cin=4', 1, 20, 24, 3, 32, 3, 0),
    ('F(2x2)', 2, 13, 13, 64, 128, 3, WINO),
    ('F(4x4)', 2, 13, 13, 64, 128, 3, WINO4),
    ('on-chip F(2x2)', 2, 13, 13, 64, 128, 3, FUSED),
    ('first block', 1, 100, 112, 3, 32, 3, -1),
    ('first block', 2, 64, 128, 3, 32, 3, -1),        # 8 whole groups
]


def _offset_inputs(rs, B, H, W, Cin, Cout, R):
    """x = 1 + 0.01 n; filters = a positive centre tap of sum 1 + 0.33 * (unit-norm noise with zero sum over the input
    channels of every tap).  The constant part of x then meets the positive part only - the zero padding at the map border
    does not move the mean - and the raw output has mean 1, std 0.01 * sqrt(sum P^2 + 0.33^2): |mean| / std of 140 .. 300."""
    x = 1 + 0.01 * rs.standard_normal((B, Cin, H, W))
    P = np.zeros((Cout, Cin, R, R))
    P[:, :, R // 2, R // 2] = rs.uniform(0.5, 1.5, (Cout, Cin))
    P /= P.sum(axis=(1, 2, 3), keepdims=True)
    N = rs.standard_normal((Cout, Cin, R, R))
    N -= N.mean(axis=1, keepdims=True)
    N /= np.sqrt((N ** 2).sum(axis=(1, 2, 3), keepdims=True))
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy((P + 0.33 * N).astype(np.float32))


def _emulated_variance(m32, tile_m):
    """The documented statistics format, emulated: fp32 two-pass (mean, M2) per tile of tile_m rows, float64 Chan combine."""
    n, mean, m2 = 0.0, np.zeros(m32.shape[1]), np.zeros(m32.shape[1])
    for r0 in range(0, m32.shape[0], tile_m):
        t = m32[r0:r0 + tile_m]
        mb = t.mean(axis=0, dtype=np.float32)
        m2b = ((t - mb) ** 2).sum(axis=0, dtype=np.float32).astype(np.float64)
        nb = float(t.shape[0])
        dlt = mb.astype(np.float64) - mean
        mean = mean + dlt * nb / (n + nb)
        m2 = m2 + m2b + dlt * dlt * n * nb / (n + nb)
        n += nb
    return m2 / n


@pytest.mark.parametrize("producer,B,H,W,Cin,Cout,R,plan", STATS_CASES)
def test_bn_statistics_under_common_offset(producer, B, H, W, Cin, Cout, R, plan):
    """Per-tile (mean, M2) pairs of every producer on a raw map with |mean| / std of 100 .. 1000 (a bright, flat input),
    finalized by ssp_bn_fwd_finalize, against float64 statistics of the fp32 map the launch itself stored.  A sum /
    sum-of-squares formulation or a pivot taken from a masked lane is invisible on zero-mean data and off by percent here.
    Bar: max(10 x the error of the emulated documented format, STATS_FLOOR); 10 x because the in-lane Welford / Chan order
    of a kernel differs from the emulation's two-pass tiles."""
    G, _lib = _imports()
    rs = X.rng(B, H, W, Cin, Cout, R, plan + 1, 2)
    x, w = _offset_inputs(rs, B, H, W, Cin, Cout, R)
    sub = list(range(0, Cout, max(1, Cout // 8)))
    r64 = F.conv2d(x.double(), w.double()[sub], None, padding=R // 2)
    ratio = r64.mean(dim=(0, 2, 3)).abs() / r64.std(dim=(0, 2, 3))
    assert 100 <= float(ratio.min()) and float(ratio.max()) <= 1000
    M = B * H * W
    cinp = (Cin + 3) // 4 * 4
    xp = torch.zeros(B, cinp, H, W)
    xp[:, :Cin] = x
    xd = G.to_nhwc(xp)
    packed = G.pack_fwd(w, cinp)
    st = G.stream()
    out = torch.full((M, Cout), float('nan'), device=G.dev())
    if plan < 0:
        ntile, tile_m = _lib.query('ssp_first_groups', B, H, W), _lib.query('ssp_first_tile_pixels')
        stats = torch.full((ntile * 64,), float('nan'), device=G.dev())
        _lib.call('ssp_first_fwd_stats', xd.data_ptr(), packed.data_ptr(), stats.data_ptr(), B, H, W, st)
        _lib.call('ssp_first_conv_raw', xd.data_ptr(), packed.data_ptr(), out.data_ptr(), Cout, B, H, W, st)
    else:
        wd = _operand(G, _lib, packed, Cout, cinp, plan)
        tile_m = _lib.query('ssp_conv_stats_tile_m', B, H, W, cinp, Cout, R, plan)
        ntile = _lib.query('ssp_conv_stats_tiles', B, H, W, cinp, Cout, R, plan)
        assert (tile_m == 0) == (plan >= 7000000)
        stats = torch.zeros(_lib.query('ssp_conv_stats_floats', B, H, W, cinp, Cout, R, plan), device=G.dev())
        wsn = max(1, _lib.query('ssp_conv_workspace_floats', B, H, W, cinp, Cout, R, plan))
        if 2 <= plan // 100000 <= 9:            # the hybrid code fits the shape: its tail rows park in the workspace
            assert wsn >= (plan // 100000) * M * Cout
        ws = torch.empty(wsn, device=G.dev())
        _lib.call('ssp_conv_fwd', xd.data_ptr(), wd.data_ptr(), out.data_ptr(), None, stats.data_ptr(), B, H, W, cinp, Cout,
                  cinp, Cout, R, 0, plan, ws.data_ptr(), wsn, st)
    vec = torch.zeros(4, Cout, device=G.dev())
    ones, zeros = torch.ones(Cout, device=G.dev()), torch.zeros(Cout, device=G.dev())
    rm, rv = torch.zeros(Cout, device=G.dev()), torch.ones(Cout, device=G.dev())
    # momentum 1, eps 0: running_var = the unbiased variance itself and invstd = var^-1/2, nothing hides the variance
    _lib.call('ssp_bn_fwd_finalize', stats.data_ptr(), ntile, tile_m, M, Cout, ones.data_ptr(), zeros.data_ptr(), rm.data_ptr(),
              rv.data_ptr(), 1.0, 0.0, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), st)
    torch.cuda.synchronize()
    m32 = out.cpu().numpy()
    assert np.isfinite(m32).all()
    m64 = m32.astype(np.float64)
    mean, var = m64.mean(axis=0), m64.var(axis=0)
    assert 100 <= (np.abs(mean) / np.sqrt(var)).min() and (np.abs(mean) / np.sqrt(var)).max() <= 1000
    err_emul = float((np.abs(_emulated_variance(m32, tile_m if tile_m else -(-M // ntile)) - var) / var).max())
    got_istd = vec[1].cpu().numpy().astype(np.float64)
    err_istd = float((np.abs(1.0 / got_istd ** 2 - var) / var).max())
    err_rvar = float((np.abs(rv.cpu().numpy().astype(np.float64) - var * M / (M - 1)) / (var * M / (M - 1))).max())
    err_kernel = max(err_istd, err_rvar)
    print('STATS %-16s %-22s tile_m %4d tiles %4d err_emulation %.3e err_kernel %.3e (invstd %.3e, running_var %.3e)'
          % (producer, (B, H, W, Cin, Cout, R, plan), tile_m, ntile, err_emul, err_kernel, err_istd, err_rvar))
    np.testing.assert_allclose(vec[0].cpu().numpy(), mean, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rm.cpu().numpy(), mean, rtol=1e-4, atol=1e-5)
    assert err_kernel <= max(10 * err_emul, STATS_FLOOR)


# ------------------------------------------------------------------------------------------ 5. one network-level case
def _bordered_input(B, H, W, seed):
    """uniform(0, 1) image with a zero-filled border of 13 rows / 11 columns (odd: pool windows straddle its edge)."""
    x = torch.from_numpy(np.random.RandomState(seed).uniform(0, 1, (B, 3, H, W)).astype(np.float32))
    x[:, :, :13] = 0
    x[:, :, :, :11] = 0
    return x


def _mix_signs(gamma, rs):
    """BatchNorm weights as trained Darknet nets have them: a seeded random sign on each, a few exactly zero."""
    c = gamma.numel()
    gamma *= torch.from_numpy((rs.randint(0, 2, c) * 2 - 1).astype(np.float32))
    gamma[torch.from_numpy(rs.choice(c, max(1, c // 8), replace=False))] = 0.0


def _assert_constant_region_winners(act_ref, idx_prod):
    """Pooled rows 0..5 / columns 0..4 see only zero input (13 rows / 11 columns of zeros, one row / column of filter reach):
    every window there is a true four-way tie, no rounding involved, and the product's winners must be ATen's."""
    idx_ref = F.max_pool2d(act_ref, 2, 2, return_indices=True)[1]
    B, C, H, W = act_ref.shape
    win = act_ref.view(B, C, H // 2, 2, W // 2, 2)
    tied = (win.amax(dim=(3, 5)) == win.amin(dim=(3, 5)))
    assert bool(tied[:, :, :6].all()) and bool(tied[:, :, :, :5].all())
    assert torch.equal(idx_prod[:, :, :6], idx_ref[:, :, :6]) and torch.equal(idx_prod[:, :, :, :5], idx_ref[:, :, :, :5])


def test_network_mixed_sign_gammas_tiny_pose():
    """tiny-pose.cfg in training mode, every bn_weight of seeded_state given a random sign and a few set to 0, input with a
    zero-filled border: head, every parameter gradient and x.grad against forward_ref with the decision-frozen recipe of
    tests/test_gpu_input_grad.py at the existing bars (1e-4 head, 3e-4 gradients) - the engine's BatchNorm fold and backward
    under negative and zero gammas end to end."""
    from oracle.darknet_ref import forward_ref, seeded_state
    from helpers import clone_state, load_state_into
    from singleshotpose_amd.darknet import Darknet
    from test_gpu_input_grad import TINY, _decisions, _probe
    B, H, W = 2, 96, 96
    model = Darknet(TINY)
    state = seeded_state(model.blocks, 3)
    rs = np.random.RandomState(21)
    for e in state:
        if e is not None and 'bn_weight' in e:
            _mix_signs(e['bn_weight'], rs)
    load_state_into(model, model.blocks, state)
    model = model.cuda().train()
    x = _bordered_input(B, H, W, 1)
    xg = x.cuda().requires_grad_(True)
    y = model(xg)
    frozen = _decisions(model, B, H, W)
    probe = _probe(y)
    (y * probe.cuda()).sum().backward()

    def dstate(grad):
        out = []
        for e in clone_state(state):
            out.append(None if e is None else {k: (v.double().requires_grad_(True) if grad and not k.startswith('running')
                                                   else v.double()) for k, v in e.items()})
        return out
    st = dstate(True)
    xr = x.double().requires_grad_(True)
    yr = forward_ref(model.blocks, st, xr, training=True, **frozen)
    assert rel_err(y.detach().cpu().numpy(), yr.detach().numpy()) < 1e-4
    yr.backward(probe.double())
    for ind, e in enumerate(st):
        if e is None:
            continue
        seq = model.models[ind]
        assert rel_err(seq[0].weight.grad.cpu().numpy(), e['weight'].grad.numpy()) < 3e-4, ind
        if 'bn_weight' in e:
            assert rel_err(seq[1].weight.grad.cpu().numpy(), e['bn_weight'].grad.numpy()) < 3e-4, ind
            assert rel_err(seq[1].bias.grad.cpu().numpy(), e['bn_bias'].grad.numpy()) < 3e-4, ind
        else:
            assert rel_err(seq[0].bias.grad.cpu().numpy(), e['bias'].grad.numpy()) < 3e-4, ind
    assert rel_err(xg.grad.cpu().numpy(), xr.grad.numpy()) < 3e-4
    # first block: the frozen winners against ATen's on the oracle's OWN activations (no override) in the constant region
    with torch.no_grad():
        _, outs = forward_ref(model.blocks, dstate(False), x.double(), training=True, keep=True)
    _assert_constant_region_winners(outs[0], frozen['pool_override'][1])


def test_network_mixed_sign_gammas_generic_pose():
    """generic-pose.cfg (fused first block, shortcuts, relu / leaky convolutions without BatchNorm, stride-1 max-pool) the
    same way.  forward_ref does not interpret shortcut blocks, so the reference is the float64 module-tree forward that
    tests/test_gpu_input_grad.py::test_generic_cfg_input_grad uses, taking its own decisions, at that test's bars."""
    import copy
    from helpers import GOLD
    import os
    from singleshotpose_amd.cfg import resolve_layers
    from singleshotpose_amd.darknet import Darknet
    from test_gpu_input_grad import _decisions, _probe
    B, H, W = 2, 80, 80
    model = Darknet(os.path.join(GOLD, 'generic-pose.cfg'))
    torch.manual_seed(0)
    rs = np.random.RandomState(22)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
                _mix_signs(m.weight, rs)
    mods = copy.deepcopy(model.models).cpu().double().train()
    model = model.cuda().train()
    x = _bordered_input(B, H, W, 2)
    xg = x.cuda().requires_grad_(True)
    y = model(xg)
    frozen = _decisions(model, B, H, W)
    probe = _probe(y)
    (y * probe.cuda()).sum().backward()
    xr = x.double().requires_grad_(True)
    h, outs = xr, {}
    for ind, b in enumerate(model.blocks[1:]):
        t = b['type']
        if t == 'convolutional':
            h = mods[ind](h)
            if ind == 0:
                act0 = h.detach()
        elif t == 'maxpool':
            s = int(b['stride'])
            h = F.max_pool2d(h, int(b['size']), s) if s > 1 else F.max_pool2d(F.pad(h, (0, 1, 0, 1), mode='replicate'), 2, 1)
        elif t == 'shortcut':
            h = outs[resolve_layers(b['from'], ind)[0]] + outs[ind - 1]
            h = F.leaky_relu(h, 0.1) if b['activation'] == 'leaky' else F.relu(h) if b['activation'] == 'relu' else h
        elif t in ('region', 'cost'):
            continue
        else:
            raise NotImplementedError(t)
        outs[ind] = h
    assert rel_err(y.detach().cpu().numpy(), h.detach().numpy()) < 1e-4
    h.backward(probe.double())
    for (name, p), q in zip(model.models.named_parameters(), mods.parameters()):
        assert rel_err(p.grad.cpu().numpy(), q.grad.numpy()) < 3e-4, name
    assert rel_err(xg.grad.cpu().numpy(), xr.grad.numpy()) < 3e-4
    _assert_constant_region_winners(act0, frozen['pool_override'][1])

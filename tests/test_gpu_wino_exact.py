"""The through-memory Winograd pipeline, F(4x4) and F(2x2), bit for bit on hand-built operands (tests/exact_wino.py; the
bounds and the geometry model are pinned without a GPU by tests/test_exact_wino_cpu.py).

The conv entry points take the TRANSFORMED filter, so these tests hand in a U of integers in {-1, 0, 1}: with x, dy in
{-1, 0, 1} the input and output-gradient transforms, the batched GEMM, A^T M A, the adjoint B dV B^T with its overlap-add,
the fused epilogues and the transform-domain filter-gradient contraction are arithmetic on a dyadic grid, exact in fp32
whatever the summation order.  Every comparison is torch.equal against a float64 reference evaluated on the tiled canvas,
except
  * the two kernels that apply G (thirds and fifteenths at F(4x4)): an elementwise a-priori bound gamma_n * |G| |g| |G|^T,
    n counted from the kernel text (see test_filter_transform_within_its_rounding_bound / test_filter_gradient_tile4);
  * slope 0.1: one rounding of y * 0.1f, 2 ulp as in tests/test_gpu_decisions.py; sums of such terms: a bound of the same kind.
Outputs are NaN-filled or integer-prefilled, workspaces and transform-domain buffers are carved out of NaN guard bands,
sliced operands hold NaN outside their slice.  The `wino_variant` experiment instantiations (4 channels per thread,
non-temporal stores, 256-channel slabs) run here under a test for the first time."""
import contextlib

import numpy as np
import pytest
import torch

import exact_conv as E
import exact_data as X
import exact_wino as XW

pytestmark = pytest.mark.gpu
NAN = float('nan')
GUARD = 1 << 16               # NaN floats in front of and behind every carved buffer
PLANE = ('plane', 'tile', 'channel')
PIXEL = ('pixel', 'channel')
E_SLOPE01 = 7.5e-8            # relative error of fl32(y * fl32(0.1)): 2^-24 + |fl32(0.1) / 0.1 - 1| (test_gpu_decisions.py)


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


@contextlib.contextmanager
def _variant(_lib, v):
    """The wino_variant experiment knob for the launches inside; back to 0 afterwards."""
    try:
        _lib.call('ssp_set_option', b'wino_variant', v)
        yield
    finally:
        _lib.call('ssp_set_option', b'wino_variant', 0)


def _carve(G, n):
    """n floats out of the middle of a NaN-filled buffer: (whole buffer, view of the middle)."""
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device=G.dev())
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _eq(got, want, names, what=''):
    assert torch.equal(got, want), '%s: %s' % (what, E.first_diffs(got, want, names))


def _sliced_out(G, M, ld, off, N, pre):
    """[M][ld] NaN, the slice [off, off + N) = `pre` (float64 array) when given."""
    out = torch.full((M, ld), NAN, dtype=torch.float32)
    if pre is not None:
        out[:, off:off + N] = XW.f32(pre)
    return out.to(G.dev())


def _slice_of(out, off, N, what):
    o = out.cpu()
    assert torch.isnan(o[:, :off]).all() and torch.isnan(o[:, off + N:]).all(), '%s: wrote outside its channel slice' % what
    return o[:, off:off + N].contiguous()


# ------------------------------------------------------------------------------------------------ the transforms alone
@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("B,H,W", XW.TILINGS)
def test_transforms_alone(B, H, W, tile):
    """ssp_wino_input_transform_t / ssp_wino_outgrad_transform_t with ld > C at a channel offset, under wino_variant 0..3
    (2 / 4 channels per thread x plain / non-temporal stores): the planes are the reference's, the guards stay NaN."""
    G, _lib = _imports()
    C, ld, off = XW.TRANSFORM_C, XW.TRANSFORM_C + 12, 8
    g = XW.geom(B, H, W, tile)
    P = (tile + 2) ** 2
    assert g.T == _lib.query('ssp_conv_wino_tiles', B, H, W, tile)
    x = XW.int_map((B, H, W, tile, 1), B, H, W, C, border=True, patch=True)
    dy = XW.int_map((B, H, W, tile, 2), B, H, W, C)
    wantV, wantM = XW.f32(XW.ref_V(x, g)), XW.f32(XW.ref_dM(dy, g))
    xd, dyd = XW.nhwc(x, ld, off).to(G.dev()), XW.nhwc(dy, ld, off).to(G.dev())
    for wv in (0, 1, 2, 3):
        vbuf, V = _carve(G, P * g.T * C)
        mbuf, dM = _carve(G, P * g.T * C)
        with _variant(_lib, wv):
            _lib.call('ssp_wino_input_transform_t', G.p(xd, off), ld, V.data_ptr(), B, H, W, C, tile, G.stream())
            _lib.call('ssp_wino_outgrad_transform_t', G.p(dyd, off), ld, dM.data_ptr(), B, H, W, C, tile, G.stream())
            torch.cuda.synchronize()
        _eq(V.cpu().view(P, g.T, C), wantV, PLANE, 'V, wino_variant %d' % wv)
        _eq(dM.cpu().view(P, g.T, C), wantM, PLANE, 'dM, wino_variant %d' % wv)
        assert _guards_intact(vbuf) and _guards_intact(mbuf)


# ------------------------------------------------------------------------------------------------ forward form
@pytest.mark.parametrize("direction", ['fwd', 'dgrad'])
@pytest.mark.parametrize("c", XW.CONV_CASES, ids=lambda c: c.id)
def test_forward_form_on_hand_built_filters(c, direction):
    """ssp_conv_fwd (integer bias) and ssp_conv_dgrad (the older form: the same contraction on dy) at F(4x4) on channel
    slices, plain and accumulating; the head of the workspace holds exactly the reference V afterwards (what the filter
    gradient reuses with x == NULL); a 256-wide output, F(4x4) and F(2x2), also under wino_variant 4: the same bits as
    under 0."""
    G, _lib = _imports()
    B, H, W = c.shape
    K, N, plan, M = c.K, c.N, c.plan, B * H * W
    tile = _lib.query('ssp_conv_plan_wino_tile', plan)
    g = XW.geom(B, H, W, tile)
    P = (tile + 2) ** 2
    v, U = XW.case_operands(c, tile)
    Vref = XW.ref_V(v, g)
    ref = XW.ref_fwd(Vref, U, g).reshape(M, N)
    pre = XW.prefill(c.shape + (K, N), (M, N))
    b = XW.bias(c.shape + (K, N), N) if direction == 'fwd' else None
    ldin, inoff, ldout, outoff = K + 16, 8, N + 12, 4
    ind, Ud = XW.nhwc(v, ldin, inoff).to(G.dev()), XW.f32(U).to(G.dev())
    bd = XW.f32(b).to(G.dev()) if b is not None else None
    wsn = _lib.query('ssp_conv_workspace_floats', B, H, W, K, N, 3, plan)
    assert wsn == P * g.T * (K + N)
    for accumulate in (0, 1):
        want = XW.f32(ref + (b if b is not None else 0) + (pre if accumulate else 0))
        bits = []
        for wv in ((0, 4) if c.wide else (0,)):
            out = _sliced_out(G, M, ldout, outoff, N, pre if accumulate else None)
            wbuf, ws = _carve(G, wsn)
            with _variant(_lib, wv):
                if direction == 'fwd':
                    _lib.call('ssp_conv_fwd', G.p(ind, inoff), Ud.data_ptr(), G.p(out, outoff), bd.data_ptr(), None, B, H, W, K, N,
                              ldin, ldout, 3, accumulate, plan, ws.data_ptr(), wsn, G.stream())
                else:
                    _lib.call('ssp_conv_dgrad', G.p(ind, inoff), Ud.data_ptr(), G.p(out, outoff), B, H, W, K, N, ldin, ldout, 3,
                              accumulate, plan, ws.data_ptr(), wsn, G.stream())
                torch.cuda.synchronize()
            what = '%s accumulate %d wino_variant %d' % (direction, accumulate, wv)
            got = _slice_of(out, outoff, N, what)
            _eq(got, want, PIXEL, what)
            _eq(ws[:P * g.T * K].cpu().view(P, g.T, K), XW.f32(Vref), PLANE, what + ', V at the workspace head')
            assert _guards_intact(wbuf), what
            bits.append(got)
        assert all(torch.equal(bits[0], o) for o in bits[1:])


# ------------------------------------------------------------------------------------------------ adjoint
@pytest.mark.parametrize("c", XW.ADJ_CASES, ids=lambda c: c.id)
def test_adjoint_on_hand_built_filters(c):
    """ssp_conv_dgrad_adj, F(4x4) with both tile heights and F(2x2) (where the corner coefficients differ in sign), on a
    hand-built Ut: dM from ssp_wino_outgrad_transform_t (dy is then a NaN buffer: not read) and dM = NULL (the launch's own
    dM behind dV in the workspace); plain and accumulating; guards intact; a 256-wide dx also under wino_variant 4."""
    G, _lib = _imports()
    B, H, W = c.shape
    K, N, plan, M = c.K, c.N, c.plan, B * H * W
    tile = _lib.query('ssp_conv_plan_wino_tile', plan)
    P = (tile + 2) ** 2
    g = XW.geom(B, H, W, tile)
    dy, Ut = XW.case_operands(c, tile)
    dMref = XW.ref_dM(dy, g)
    ref = XW.ref_adj(dMref, Ut, g).reshape(M, N)
    assert float(np.abs(ref).max()) > 0
    pre = XW.prefill(c.shape + (K, N, tile), (M, N))
    lddy, dyoff, lddx, dxoff = K + 12, 4, N + 16, 8
    dyd, Ud = XW.nhwc(dy, lddy, dyoff).to(G.dev()), XW.f32(Ut).to(G.dev())
    nodata = torch.full((M, lddy), NAN, dtype=torch.float32, device=G.dev())
    bits = []
    for shared in (True, False):
        wsn = _lib.query('ssp_conv_dgrad_adj_workspace_floats', B, H, W, K, N, plan, 0 if shared else 1)
        assert wsn == P * g.T * (N + (0 if shared else K))
        for wv in ((0, 4) if c.wide else (0,)):
            wbuf, ws = _carve(G, wsn)
            mbuf, dM = _carve(G, P * g.T * K)
            if shared:
                _lib.call('ssp_wino_outgrad_transform_t', G.p(dyd, dyoff), lddy, dM.data_ptr(), B, H, W, K, tile, G.stream())
            for accumulate in (0, 1):
                what = 'dM %s, accumulate %d, wino_variant %d' % ('given' if shared else 'NULL', accumulate, wv)
                dx = _sliced_out(G, M, lddx, dxoff, N, pre if accumulate else None)
                with _variant(_lib, wv):
                    _lib.call('ssp_conv_dgrad_adj', G.p(nodata if shared else dyd, dyoff), Ud.data_ptr(), G.p(dx, dxoff), B, H, W, K, N,
                              lddy, lddx, 3, accumulate, plan, ws.data_ptr(), wsn, dM.data_ptr() if shared else None, G.stream())
                    torch.cuda.synchronize()
                got = _slice_of(dx, dxoff, N, what)
                _eq(got, XW.f32(ref + (pre if accumulate else 0)), PIXEL, what)
                assert _guards_intact(wbuf) and _guards_intact(mbuf), what
                if shared:
                    _eq(dM.cpu().view(P, g.T, K), XW.f32(dMref), PLANE, what + ', dM')
                else:
                    assert bool(torch.isnan(dM).all()), what + ': dM not given, yet touched'
                    _eq(ws[P * g.T * N:].cpu().view(P, g.T, K), XW.f32(dMref), PLANE, what + ', own dM behind dV')
                if not accumulate:
                    bits.append(got)
    assert all(torch.equal(bits[0], o) for o in bits[1:])


@pytest.mark.parametrize("shape", XW.ADJ_F2_REAL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_adjoint_f2_on_real_filters_against_int64(shape):
    """The F(2x2) adjoint with REAL filters, multiples of 4, through ssp_wino_filter_transform_adj_t: as exact as the other
    F(2x2) forms already are (tests/test_gpu_conv_exact.py) - torch.equal against exact_conv.ref_dgrad in int64."""
    G, _lib = _imports()
    B, H, W, Cin, Cout, _ = shape
    M, plan, tile, P = B * H * W, XW.W2, 2, 16
    _, dy, w = E.operands(shape, *shape, wino=True)
    ref = E.ref_dgrad(dy, w).reshape(M, Cin)
    pre = E.prefill(shape + (plan, 1), ref.shape)
    wd = E.pack_dgrad(w).float().to(G.dev())                          # [Cin][tap, rotated][Cout]
    Ut = torch.full((P * Cin * Cout,), NAN, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_wino_filter_transform_adj_t', wd.data_ptr(), Ut.data_ptr(), Cin, Cout, tile, G.stream())
    lddy, dyoff, lddx, dxoff = Cout + 12, 4, Cin + 16, 8
    dyd = E.nhwc_buffer(dy, lddy, dyoff).to(G.dev())
    T = _lib.query('ssp_conv_wino_tiles', B, H, W, tile)
    for shared in (True, False):
        wsn = _lib.query('ssp_conv_dgrad_adj_workspace_floats', B, H, W, Cout, Cin, plan, 0 if shared else 1)
        wbuf, ws = _carve(G, wsn)
        mbuf, dM = _carve(G, P * T * Cout)
        if shared:
            _lib.call('ssp_wino_outgrad_transform_t', G.p(dyd, dyoff), lddy, dM.data_ptr(), B, H, W, Cout, tile, G.stream())
        for accumulate, want in ((0, ref), (1, ref + pre)):
            dx = torch.full((M, lddx), NAN, dtype=torch.float32)
            if accumulate:
                dx[:, dxoff:dxoff + Cin] = pre.float()
            dx = dx.to(G.dev())
            _lib.call('ssp_conv_dgrad_adj', G.p(dyd, dyoff), Ut.data_ptr(), G.p(dx, dxoff), B, H, W, Cout, Cin, lddy, lddx, 3,
                      accumulate, plan, ws.data_ptr(), wsn, dM.data_ptr() if shared else None, G.stream())
            torch.cuda.synchronize()
            what = 'dM %s, accumulate %d' % ('given' if shared else 'NULL', accumulate)
            _eq(_slice_of(dx, dxoff, Cin, what), want.float(), PIXEL, what)
            assert _guards_intact(wbuf) and _guards_intact(mbuf), what


# ------------------------------------------------------------------------------------------------ fused epilogues
def _same(got, ref64, slope, what):
    """Bit-exact for a dyadic slope, within 2 ulp (one rounding of y * 0.1f) for 0.1."""
    ref = torch.from_numpy(np.ascontiguousarray(ref64))
    if slope != 0.1:
        _eq(got, XW.f32(ref64), PIXEL, what)
    else:
        d = X.ulp_diff(got, ref)
        assert d <= 2.0, '%s: %.2f ulp' % (what, d)


@pytest.mark.parametrize("c", XW.EPI_CASES, ids=lambda c: c.id)
def test_fused_epilogues_f4(c):
    """ssp_conv_fwd_affine, ssp_conv_dgrad_bnbwd and ssp_conv_dgrad_adj_bnbwd at F(4x4): the leaky sign at y == 0 and the zero /
    negative scales are decided on exact values.  dx of the bnbwd entry points bit for bit; the column sums over the
    `partial` rows (summed on the host in float64: no dependence on the group layout) bit for bit with as many rows as the
    launch has groups (plain stores into a NaN-filled buffer) and with fewer (the atomic fold, from a zeroed buffer)."""
    G, _lib = _imports()
    B, H, W = c.shape
    K, N, plan, M, P = c.K, c.N, c.plan, B * H * W, 36
    r = XW.epilogue_refs(c)
    g = r['g']
    ldin, inoff, ldout, outoff, ldraw, rawoff = K + 16, 8, N + 12, 4, N + 8, 4
    ind, Ud = XW.nhwc(r['v'], ldin, inoff).to(G.dev()), XW.f32(r['U']).to(G.dev())
    nodata = torch.full((M, ldin), NAN, dtype=torch.float32, device=G.dev())
    rawd = XW.nhwc(r['raw'], ldraw, rawoff).to(G.dev())
    scd, shd, mud, isd = (XW.f32(r[k]).to(G.dev()) for k in ('sc', 'sh', 'mu', 'istd'))
    wsn = _lib.query('ssp_conv_workspace_floats', B, H, W, K, N, 3, plan)
    # ---- eval-mode affine + leaky
    conv = r['conv'].reshape(M, N)
    for with_scale in (True, False):
        y = (conv * r['sc'] if with_scale else conv) + r['sh']
        for slope in XW.SLOPES:
            out = _sliced_out(G, M, ldout, outoff, N, None)
            wbuf, ws = _carve(G, wsn)
            _lib.call('ssp_conv_fwd_affine', G.p(ind, inoff), Ud.data_ptr(), G.p(out, outoff), scd.data_ptr() if with_scale else None,
                      shd.data_ptr(), slope, B, H, W, K, N, ldin, ldout, 3, plan, ws.data_ptr(), wsn, G.stream())
            torch.cuda.synchronize()
            what = 'affine, slope %g, scale %s' % (slope, 'given' if with_scale else 'NULL')
            _same(_slice_of(out, outoff, N, what), XW.leaky(y, slope), slope, what)
            assert _guards_intact(wbuf), what
    # ---- data gradient + BatchNorm-backward sums, the older form and the adjoint
    ntile = _lib.query('ssp_conv_stats_tiles', B, H, W, K, N, 3, plan)
    assert ntile == (g.T + 15) // 16 >= 2
    mbuf, dM = _carve(G, P * g.T * K)
    _lib.call('ssp_wino_outgrad_transform_t', G.p(ind, inoff), ldin, dM.data_ptr(), B, H, W, K, 4, G.stream())
    wsn_adj = _lib.query('ssp_conv_dgrad_adj_workspace_floats', B, H, W, K, N, plan, 1)
    for form, given in (('conv', None), ('adj', True), ('adj', False)):
        gref = r[form].reshape(M, N)
        raw = r['raw'].reshape(1, 1, M, N)
        for slope in XW.SLOPES:
            s1, s2, a1, a2 = XW.bn_sums(gref.reshape(1, 1, M, N), raw, r['sc'], r['sh'], r['mu'], r['istd'], slope)
            for rows in (ntile, ntile - 1):
                what = '%s (dM %s), slope %g, %d partial rows for %d groups' % (form, given, slope, rows, ntile)
                part = torch.full((rows * N * 2,), NAN if rows >= ntile else 0.0, dtype=torch.float32, device=G.dev())
                dx = _sliced_out(G, M, ldout, outoff, N, None)
                wbuf, ws = _carve(G, wsn if form == 'conv' else wsn_adj)
                tail = (rawd.data_ptr() + 4 * rawoff, ldraw, scd.data_ptr(), shd.data_ptr(), mud.data_ptr(), isd.data_ptr(), slope,
                        part.data_ptr(), rows)
                if form == 'conv':
                    _lib.call('ssp_conv_dgrad_bnbwd', G.p(ind, inoff), Ud.data_ptr(), G.p(dx, outoff), B, H, W, K, N, ldin, ldout, 3,
                              plan, ws.data_ptr(), wsn, *tail, G.stream())
                else:
                    _lib.call('ssp_conv_dgrad_adj_bnbwd', G.p(nodata if given else ind, inoff), Ud.data_ptr(), G.p(dx, outoff), B, H, W,
                              K, N, ldin, ldout, 3, plan, ws.data_ptr(), wsn_adj, *tail, dM.data_ptr() if given else None, G.stream())
                torch.cuda.synchronize()
                _eq(_slice_of(dx, outoff, N, what), XW.f32(gref), PIXEL, what)
                assert _guards_intact(wbuf) and _guards_intact(mbuf), what
                ps = part.cpu().double().view(rows, N, 2).sum(0)
                for k, (s, a) in enumerate(((s1, a1), (s2, a2))):
                    got, want = ps[:, k], torch.from_numpy(s)
                    if slope != 0.1:
                        _eq(got, want, ('channel',), what + ', sum %d' % (k + 1))
                    else:
                        # M terms, each off by E_SLOPE01 (+ one rounding of the product with xhat), added in at most M + 1
                        # roundings of partial sums that never exceed the sum of the |terms|
                        bound = (E_SLOPE01 + (M + 2) * XW.U32) * torch.from_numpy(a) * (1 + 1e-6)
                        assert bool(((got - want).abs() <= bound).all()), what + ', sum %d' % (k + 1)


# ------------------------------------------------------------------------------------------------ filter gradient
@pytest.mark.parametrize("shape,Cin,Cout", XW.WGRAD_CASES)
def test_filter_gradient_tile4(shape, Cin, Cout):
    """ssp_conv_wgrad_wino_t at tile 4.  After the launch the workspace (V | dM | dU, include/ssp_hip.h) holds the reference's
    V, dM and - at offset 36 T (Cin + Cout), layout [36][Cout][Cin] - dU, bit for bit; the same bits with dy == NULL (dM
    pre-placed by ssp_wino_outgrad_transform_t) and with x == NULL (V pre-placed by ssp_wino_input_transform_t).
    dw itself goes through G^T . G (wino_wgrad_finish_kernel<4>): per output a[a'][b'] += G[i][a'] h[b'] over six rows i with
    h[b'] = sum_j G[j][b'] u[j] - every term carries the rounded coefficient (1), its product (1) and at most four further
    additions of its pass (the first lands on a zero), 6 per pass, and the final read-add-write one more: m = 13, so
    |dw - (pre + G^T dU G)| <= gamma_13 (|G^T| |dU| |G|) + u |pre| elementwise."""
    G, _lib = _imports()
    B, H, W = shape
    M, P, tile = B * H * W, 36, 4
    g = XW.geom(B, H, W, tile)
    x, dy = XW.wgrad_operands(shape, Cin, Cout)
    Vref, dMref = XW.ref_V(x, g), XW.ref_dM(dy, g)
    dUref = XW.ref_dU(dMref, Vref)
    pre = XW.prefill(shape + (Cin, Cout), (Cout, 9, Cin))
    want = torch.from_numpy(pre + XW.back_filter(dUref, tile))
    bound = torch.from_numpy(XW.gamma(XW.N_WGRAD_FINISH) * XW.back_filter(np.abs(dUref), tile, XW.mats(tile, absolute=True)) +
                             XW.U32 * np.abs(pre))
    ldx, xoff, lddy, dyoff = Cin + 16, 8, Cout + 12, 4
    xd, dyd = XW.nhwc(x, ldx, xoff).to(G.dev()), XW.nhwc(dy, lddy, dyoff).to(G.dev())
    wsn = _lib.query('ssp_conv_wgrad_wino_workspace_floats_t', B, H, W, Cin, Cout, tile)
    assert wsn == P * (g.T * (Cin + Cout) + Cin * Cout)
    oV, oM, oU = 0, P * g.T * Cin, P * g.T * (Cin + Cout)
    bits = []
    for mode in ('both given', 'dy NULL', 'x NULL'):
        wbuf, ws = _carve(G, wsn)
        if mode == 'dy NULL':
            _lib.call('ssp_wino_outgrad_transform_t', G.p(dyd, dyoff), lddy, G.p(ws, oM), B, H, W, Cout, tile, G.stream())
        if mode == 'x NULL':
            _lib.call('ssp_wino_input_transform_t', G.p(xd, xoff), ldx, G.p(ws, oV), B, H, W, Cin, tile, G.stream())
        dw = XW.f32(pre).to(G.dev())
        _lib.call('ssp_conv_wgrad_wino_t', None if mode == 'dy NULL' else G.p(dyd, dyoff), None if mode == 'x NULL' else G.p(xd, xoff),
                  dw.data_ptr(), B, H, W, Cin, Cout, lddy, ldx, tile, ws.data_ptr(), wsn, G.stream())
        torch.cuda.synchronize()
        w = ws.cpu()
        _eq(w[oV:oM].view(P, g.T, Cin), XW.f32(Vref), PLANE, mode + ', V')
        _eq(w[oM:oU].view(P, g.T, Cout), XW.f32(dMref), PLANE, mode + ', dM')
        _eq(w[oU:].view(P, Cout, Cin), XW.f32(dUref), ('plane', 'cout', 'cin'), mode + ', dU')
        assert _guards_intact(wbuf), mode
        got = dw.cpu().view(Cout, 9, Cin)
        err = (got.double() - want).abs()
        print('%s: dw off by at most %.3g of its bound (largest |error| %.3g, largest bound %.3g)' % (
            mode, float((err / bound.clamp_min(1e-300)).max()), float(err.max()), float(bound.max())))
        assert bool((err <= bound).all()), '%s: %d of %d outside the rounding bound' % (mode, int((err > bound).sum()), err.numel())
        bits.append(got)
    assert all(torch.equal(bits[0], o) for o in bits[1:])


# ------------------------------------------------------------------------------------------------ the kernels that hold G
@pytest.mark.parametrize("adj", [False, True], ids=['forward', 'adjoint'])
def test_filter_transform_within_its_rounding_bound(adj):
    """ssp_wino_filter_transform_t / _adj_t on integer filters.  wino_filter_kernel<4>: h = G g, then U = h G^T, each a sum of
    at most three terms c * x per output: the rounded coefficient (1), the product (1) and at most two further additions (the
    first lands on a zero) - 4 roundings per pass, n = 8: |U - G g G^T| <= gamma_8 (|G| |g| |G|^T) elementwise (plus 2^-50 of
    it for the float64 reference itself).  Tile 2 on multiples of 4: G holds halves, torch.equal."""
    G, _lib = _imports()
    rows, K = 72, 80
    w9 = X.rng(rows, K, int(adj)).randint(-8, 9, (rows, 9, K)).astype(np.float64)
    plain = w9[:, ::-1, :] if adj else w9                                      # _adj_t: taps stored rotated by 180 degrees
    name = 'ssp_wino_filter_transform_adj_t' if adj else 'ssp_wino_filter_transform_t'
    for tile, scale in ((4, 1.0), (2, 4.0)):
        P = (tile + 2) ** 2
        wd = XW.f32(w9 * scale).to(G.dev())
        ubuf, U = _carve(G, P * rows * K)
        _lib.call(name, wd.data_ptr(), U.data_ptr(), rows, K, tile, G.stream())
        torch.cuda.synchronize()
        assert _guards_intact(ubuf)
        got = U.cpu().view(P, rows, K)
        ref = XW.filter_transform(plain * scale, tile)
        if tile == 2:
            _eq(got, XW.f32(ref), ('plane', 'row', 'k'), 'tile 2')
            continue
        S = XW.filter_transform(np.abs(plain), tile, XW.mats(tile, absolute=True))
        bound = torch.from_numpy((XW.gamma(XW.N_FILTER) + 2.0 ** -50) * S)
        err = (got.double() - torch.from_numpy(ref)).abs()
        print('tile 4: U off by at most %.3g of its bound (largest |error| %.3g)' % (
            float((err / bound.clamp_min(1e-300)).max()), float(err.max())))
        assert bool((err <= bound).all()), '%d of %d outside the rounding bound' % (int((err > bound).sum()), err.numel())
        assert float(err.max()) > 0, "thirds cannot come out exact: the reference or the kernel is not what this test thinks"

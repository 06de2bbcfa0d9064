"""Properties of tests/exact_wino.py that keep tests/test_gpu_wino_exact.py from passing vacuously - no GPU: where the
dyadic / non-dyadic split of the Winograd matrices lies, the per-case and per-stage bounds (every sum of |terms| below 2^24
grid steps, printed), the geometry model against float64 F.conv2d and its autograd (with U = G g G^T of a real filter the
model IS a convolution), float64 against an int64 scaled-grid evaluation, the tile count against the library's host query,
and the wrong models each case must tell from the right one (coverage table printed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_conv as E
import exact_wino as XW
from exact_data import rng


def _is_int(m):
    return bool(np.all(m == np.round(m)))


def _dyadic(m):
    return _is_int(m * 2.0 ** 20)


def test_where_the_exact_split_lies():
    BT, G, AT = XW.mats(4)
    assert _is_int(4 * BT) and _is_int(2 * BT) and not _is_int(BT)
    assert _is_int(8 * AT) and not _is_int(4 * AT)
    assert not _dyadic(G), "G of F(4x4) holds thirds: the kernels that apply it get a rounding bound, not torch.equal"
    assert _is_int(15 * G)
    BT, G, AT = XW.mats(2)
    assert _is_int(BT) and _is_int(AT) and _is_int(2 * G) and not _is_int(G)
    # the grids exact_wino.GRID states follow: two passes of each matrix
    assert XW.GRID[4] == dict(V=2 * 2, dM=8 * 8, Y=4 * 64, dX=64 * 4, dU=64 * 4)
    # columns 0 and n+1 of B^T are unit vectors; the corner coefficients differ at tile 2 only
    for tile in (2, 4):
        BT = XW.mats(tile)[0]
        a = tile + 2
        assert np.count_nonzero(BT[:, 0]) == 1 and np.count_nonzero(BT[:, a - 1]) == 1
    assert XW.mats(4)[0][0][0] == XW.mats(4)[0][5][5] == 1 and XW.mats(2)[0][3][3] == -1


def _tile(plan):
    return 2 if plan >= 9000000 else 4


def _show(name, b):
    print('%-44s %s' % (name, '  '.join('%s %.3g' % (k, v) for k, v in b.items())))
    for k, v in b.items():
        assert v < XW.TWO24, (name, k, v)


@pytest.mark.parametrize("c", XW.CONV_CASES, ids=lambda c: c.id)
def test_bounds_forward_form(c):
    tile = _tile(c.plan)
    g = XW.geom(*c.shape, tile)
    v, U = XW.case_operands(c)
    b = XW.bound_fwd(v, U, g)
    b['Y+bias+prefill'] = b['Y'] + (XW.BIAS + XW.PREFILL) * XW.GRID[tile]['Y']
    _show(c.id, b)
    assert ((U != 0).sum(-1) > 0).all() and float(np.abs(v).max()) == 1


@pytest.mark.parametrize("c", XW.ADJ_CASES, ids=lambda c: c.id)
def test_bounds_adjoint(c):
    tile = _tile(c.plan)
    g = XW.geom(*c.shape, tile)
    dy, Ut = XW.case_operands(c)
    b = XW.bound_adj(dy, Ut, g)
    b['dX+prefill'] = b['dX'] + XW.PREFILL * XW.GRID[tile]['dX']
    _show(c.id, b)
    assert ((Ut != 0).sum(-1) > 0).all()


@pytest.mark.parametrize("shape,Cin,Cout", XW.WGRAD_CASES)
def test_bounds_filter_gradient(shape, Cin, Cout):
    g = XW.geom(*shape, 4)
    assert g.T >= 16
    x, dy = XW.wgrad_operands(shape, Cin, Cout)
    _show('wgrad-%dx%dx%d-%dto%d' % (shape + (Cin, Cout)), XW.bound_wgrad(x, dy, g))


@pytest.mark.parametrize("c", XW.EPI_CASES, ids=lambda c: c.id)
def test_bounds_fused_epilogues(c):
    r = XW.epilogue_refs(c)
    g = r['g']
    assert cdiv16(g.T) >= 2, "needs more than one group of 16 tiles: fewer partial rows than groups must exist"
    b = XW.bound_fwd(r['v'], r['U'], g)
    b.update({'adj ' + k: v for k, v in XW.bound_adj(r['v'], r['U'], g).items()})
    # affine: y = scale * conv + shift on the grid 1/512, leaky(y, 0.125) on 1/4096 - one exact operation each on the values
    y = r['conv'] * r['sc'] + r['sh']
    b['affine y'] = float(np.abs(y).max()) * 512
    b['leaky(y, 1/8)'] = float(np.abs(y).max()) * 4096
    assert float((y == 0).mean()) > 0.01 and (r['sc'] == 0).any() and (r['sc'] < 0).any()
    # BatchNorm-backward sums over ALL pixels of a channel (the atomic fold adds every group into few rows): dy' on the grid
    # 1/2048 at slope 1/8, xhat = (raw - mean) * invstd an integer
    for name in ('conv', 'adj'):
        s1, s2, a1, a2 = XW.bn_sums(r[name], r['raw'], r['sc'], r['sh'], r['mu'], r['istd'], 0.125)
        b[name + ' sum|dy|'] = float(a1.max()) * 2048
        b[name + ' sum|dy xhat|'] = float(a2.max()) * 2048
        assert float(np.abs(s2).max()) > 0 and float(np.abs(r[name]).max()) > 0
    _show(c.id, b)


@pytest.mark.parametrize("shape", XW.ADJ_F2_REAL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bounds_adjoint_f2_real_filters(shape):
    """The F(2x2) adjoint on exact_conv's operands (|dy| <= 3, filters multiples of 4 up to 8): worst case of every stage."""
    B, H, W, Cin, Cout, _ = shape
    g = XW.geom(B, H, W, 2)
    wabs = np.full((Cin, 9, Cout), float(E.WMAX_WINO))
    Ut = XW.filter_transform(wabs, 2, XW.mats(2, absolute=True))
    _show('adj-f2-real-' + 'x'.join(map(str, shape)), XW.bound_adj(np.full((B, H, W, Cout), float(E.XMAX)), Ut, g))
    assert np.array_equal(XW.filter_transform(4 * np.ones((3, 9, 4)), 2), np.round(XW.filter_transform(4 * np.ones((3, 9, 4)), 2)))


def cdiv16(T):
    return (T + 15) // 16


# ------------------------------------------------------------------------------------------------ the model is a convolution
def _real_filter_case(shape, Cin, Cout, tile, seed):
    rs = rng(seed, tile, *shape)
    x = rs.standard_normal(shape + (Cin,))
    dy = rs.standard_normal(shape + (Cout,))
    w = rs.standard_normal((Cout, Cin, 3, 3))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    y = F.conv2d(xt, wt, None, padding=1)
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).numpy()
    return x, dy, w, nhwc(y), nhwc(xt.grad), wt.grad.numpy()


@pytest.mark.parametrize("shape,tile", [((3, 10, 7), 4), ((3, 10, 7), 2), ((7, 13, 13), 4), ((4, 13, 9), 4), ((8, 5, 5), 4)])
def test_model_is_a_convolution_for_real_filters(shape, tile):
    Cin, Cout = 5, 6
    g = XW.geom(*shape, tile)
    assert g.mosaic == (shape != (3, 10, 7))
    x, dy, w, y, dx, dw = _real_filter_case(shape, Cin, Cout, tile, 3)
    w9 = w.transpose(0, 2, 3, 1).reshape(Cout, 9, Cin)                       # [Cout][tap][Cin]
    U = XW.filter_transform(w9, tile)                                        # [P][Cout][Cin]
    V, dM = XW.ref_V(x, g), XW.ref_dM(dy, g)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    e_f = rel(XW.ref_fwd(V, U, g), y)
    e_a = rel(XW.ref_adj(dM, np.ascontiguousarray(U.transpose(0, 2, 1)), g), dx)
    e_w = rel(XW.back_filter(XW.ref_dU(dM, V), tile), dw.transpose(0, 2, 3, 1).reshape(Cout, 9, Cin))
    # the older data-gradient form: the forward form on dy with the rotated, transposed filters
    wd = w9[:, ::-1, :].transpose(2, 1, 0)                                   # [Cin][tap rotated][Cout]
    e_d = rel(XW.ref_fwd(XW.ref_V(dy, g), XW.filter_transform(wd, tile), g), dx)
    print('%s tile %d (%s): forward %.1e adjoint %.1e filter gradient %.1e older dgrad %.1e' % (
        shape, tile, 'mosaic' if g.mosaic else 'plain', e_f, e_a, e_w, e_d))
    assert max(e_f, e_a, e_w, e_d) < 1e-12


def test_float64_against_an_int64_grid_evaluation():
    """The smallest case again with 2 B^T and 8 A^T as int64 matrices and int64 operands: the float64 references lose nothing."""
    c = XW.CONV_CASES[0]
    g = XW.geom(*c.shape, 4)
    v, U = XW.case_operands(c)
    BT, G, AT = XW.mats(4)
    mi = ((2 * BT).astype(np.int64), None, (8 * AT).astype(np.int64))
    vi, Ui = v.astype(np.int64), U.astype(np.int64)
    toi = lambda a, s: np.round(a * s).astype(np.int64)
    Vi = _int_V(vi, g, mi)
    assert np.array_equal(Vi, toi(XW.ref_V(v, g), 4))
    dMi = _int_dM(vi, g, mi)
    assert np.array_equal(dMi, toi(XW.ref_dM(v, g), 64))
    Mi = np.einsum('ptk,prk->ptr', Vi, Ui)
    Yi = np.einsum('pi,nyxijc,qj->nyxpqc', mi[2], XW._from_planes(Mi, g), mi[2])
    cv = Yi.transpose(0, 1, 3, 2, 4, 5).reshape(g.nb, 4 * g.th, 4 * g.tw, -1)[:, :g.Hc, :g.Wc]
    assert np.array_equal(XW.from_canvas(cv, g), toi(XW.ref_fwd(XW.ref_V(v, g), U, g), 256))
    dVi = XW._from_planes(np.einsum('ptk,prk->ptr', dMi, Ui), g)
    ddi = np.einsum('ik,nyxijc,jl->nyxklc', mi[0], dVi, mi[0])               # one window per image here: no overlap
    assert g.th == g.tw == 1
    assert np.array_equal(ddi[:, 0, 0, 1:5, 1:5], toi(XW.ref_adj(XW.ref_dM(v, g), U, g), 256))
    assert np.array_equal(np.einsum('ptc,ptk->pck', dMi, Vi), toi(XW.ref_dU(XW.ref_dM(v, g), XW.ref_V(v, g)), 256))


def _int_V(vi, g, mi):
    pad = np.zeros((g.nb, 4 * g.th + 2, 4 * g.tw + 2, vi.shape[-1]), dtype=np.int64)
    pad[:, 1:g.Hc + 1, 1:g.Wc + 1] = vi
    d = np.stack([np.stack([pad[:, 4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6] for tx in range(g.tw)], 1) for ty in range(g.th)], 1)
    return XW._to_planes(np.einsum('ik,nyxklc,jl->nyxijc', mi[0], d, mi[0]))


def _int_dM(vi, g, mi):
    pad = np.zeros((g.nb, 4 * g.th, 4 * g.tw, vi.shape[-1]), dtype=np.int64)
    pad[:, :g.Hc, :g.Wc] = vi
    d = pad.reshape(g.nb, g.th, 4, g.tw, 4, -1).transpose(0, 1, 3, 2, 4, 5)
    return XW._to_planes(np.einsum('pi,nyxpqc,qj->nyxijc', mi[2], d, mi[2]))


# ------------------------------------------------------------------------------------------------ tile count
def test_tile_count_is_the_librarys():
    """geom().T == ssp_conv_wino_tiles (a host function of the shape) for every case and both tile sizes."""
    from singleshotpose_amd import _lib
    shapes = set(XW.TILINGS) | {c.shape for c in XW.CONV_CASES + XW.ADJ_CASES + XW.EPI_CASES} | {s for s, _, _ in XW.WGRAD_CASES}
    for shape in sorted(shapes):
        for tile in (2, 4):
            g = XW.geom(*shape, tile)
            assert g.T == _lib.query('ssp_conv_wino_tiles', *shape, tile) == E.wino_tiles(*shape, tile), (shape, tile)
    mos = {s: XW.geom(*s, 4).mosaic for s in XW.TILINGS}
    assert mos == {(1, 4, 4): False, (2, 8, 12): False, (3, 10, 7): False, (4, 13, 13): True, (7, 13, 13): True,
                   (4, 13, 9): True, (2, 13, 13): False}
    assert XW.geom(8, 5, 5, 4).mosaic and XW.geom(7, 13, 13, 4).nb * 4 - 7 == 1


# ------------------------------------------------------------------------------------------------ can-fail properties
def _adj_case(shape, tile):
    return next(c for c in XW.ADJ_CASES if c.shape == shape and _tile(c.plan) == tile)


def _conv_case(shape):
    return next(c for c in XW.CONV_CASES if c.shape == shape and _tile(c.plan) == 4)


def test_wrong_models_change_the_reference():
    """Each wrong model changes the reference result of the case that claims to cover it: a kernel with that bug fails it."""
    table = []

    def differs(what, case, a, b):
        n = int((a != b).sum())
        table.append((what, case, n, a.size))
        assert n > 0, (what, case)

    # one of the eight neighbour contributions of the adjoint dropped: the exact tiling (every neighbour in the interior)
    for tile in (4, 2):
        c = _adj_case((2, 8, 12), tile)
        g = XW.geom(*c.shape, tile)
        dy, Ut = XW.case_operands(c)
        dM = XW.ref_dM(dy, g)
        good = XW.ref_adj(dM, Ut, g)
        for nb in XW.NEIGHBOURS:
            differs('adjoint without neighbour %s, tile %d' % (nb, tile), c.id, XW.ref_adj(dM, Ut, g, skip=nb), good)
    # with every neighbour absent nothing can be dropped: the one-tile case has no such term
    c = _adj_case((1, 4, 4), 4)
    g = XW.geom(*c.shape, 4)
    dy, Ut = XW.case_operands(c)
    dM = XW.ref_dM(dy, g)
    assert all(np.array_equal(XW.ref_adj(dM, Ut, g, skip=nb), XW.ref_adj(dM, Ut, g)) for nb in XW.NEIGHBOURS)
    # corner coefficients c0l / cll exchanged: visible at tile 2 only (B^T[3][3] = -1), invisible at tile 4 (both 1)
    for shape in ((2, 8, 12), (7, 13, 13)):
        c = _adj_case(shape, 2)
        g = XW.geom(*c.shape, 2)
        dy, Ut = XW.case_operands(c)
        dM = XW.ref_dM(dy, g)
        differs('adjoint corners c0l / cll exchanged, tile 2', c.id, XW.ref_adj(dM, Ut, g, corner_swap=True), XW.ref_adj(dM, Ut, g))
    c = _adj_case((2, 8, 12), 4)
    g = XW.geom(*c.shape, 4)
    dy, Ut = XW.case_operands(c)
    dM = XW.ref_dM(dy, g)
    assert np.array_equal(XW.ref_adj(dM, Ut, g, corner_swap=True), XW.ref_adj(dM, Ut, g))
    table.append(('adjoint corners c0l / cll exchanged, tile 4', c.id, 0, dM.size))
    # mosaic geometry: second image one pixel off; the gap read as data - forward form and adjoint on both mosaic cases
    for shape in ((4, 13, 13), (7, 13, 13), (4, 13, 9)):
        c = _conv_case(shape)
        g = XW.geom(*c.shape, 4)
        assert g.mosaic
        v, U = XW.case_operands(c)
        good = XW.ref_fwd(XW.ref_V(v, g), U, g)
        differs('second mosaic image shifted by one pixel', c.id, XW.ref_fwd(XW.ref_V(v, g, shift=(0, 1)), U, g), good)
        differs('gap column / row read as data', c.id, XW.ref_fwd(XW.ref_V(v, g, gap=1.0), U, g), good)
    # the last tile row dropped: ragged plain tiling and a mosaic
    for shape in ((3, 10, 7), (4, 13, 9)):
        c = _conv_case(shape)
        g = XW.geom(*c.shape, 4)
        v, U = XW.case_operands(c)
        V = XW.ref_V(v, g)
        differs('last tile row dropped', c.id, XW.ref_fwd(V, U, g, last_row=False), XW.ref_fwd(V, U, g))
    # every single plane of U matters (forward form) and of Ut (adjoint)
    c = _conv_case((2, 8, 12))
    g = XW.geom(*c.shape, 4)
    v, U = XW.case_operands(c)
    V = XW.ref_V(v, g)
    good = XW.ref_fwd(V, U, g)
    worst = None
    for xi in range(36):
        U0 = U.copy()
        U0[xi] = 0
        n = int((XW.ref_fwd(V, U0, g) != good).sum())
        assert n > 0, xi
        worst = n if worst is None else min(worst, n)
    table.append(('one plane of U zeroed (the least visible of 36)', c.id, worst, good.size))
    for tile in (4, 2):
        c = _adj_case((3, 10, 7), tile)
        g = XW.geom(*c.shape, tile)
        dy, Ut = XW.case_operands(c)
        dM = XW.ref_dM(dy, g)
        good = XW.ref_adj(dM, Ut, g)
        worst = None
        for xi in range((tile + 2) ** 2):
            U0 = Ut.copy()
            U0[xi] = 0
            n = int((XW.ref_adj(dM, U0, g) != good).sum())
            assert n > 0, xi
            worst = n if worst is None else min(worst, n)
        table.append(('one plane of Ut zeroed (the least visible), tile %d' % tile, c.id, worst, good.size))
    print('\n%-58s %-34s %s' % ('wrong model', 'case', 'elements changed'))
    for what, case, n, tot in table:
        print('%-58s %-34s %d of %d' % (what, case, n, tot))


def test_phase_dependence_of_a_hand_built_operand():
    """A hand-built U is no filter transform: the forward-form result of the mosaic differs from the per-image tiling, which
    is why the references work on the canvas (a real filter gives the same result either way - the convolution test)."""
    c = _conv_case((4, 13, 13))
    v, U = XW.case_operands(c)
    gm, gp = XW.geom(*c.shape, 4), XW.geom(*c.shape, 4, mosaic=False)
    assert not np.array_equal(XW.ref_fwd(XW.ref_V(v, gm), U, gm), XW.ref_fwd(XW.ref_V(v, gp), U, gp))


def test_g_kernels_reference_and_bound():
    """The a-priori bound of the two G kernels is far below the 1e-4 bar it replaces, and non-trivial: gamma_8 and gamma_13 of
    the absolute-value transform.  On multiples of 4 the tile-2 transform is an integer."""
    rs = rng(5)
    w9 = rs.randint(-2, 3, (8, 9, 12)).astype(np.float64)
    U = XW.filter_transform(w9, 4)
    S = XW.filter_transform(np.abs(w9), 4, XW.mats(4, absolute=True))
    assert (S >= np.abs(U) - 1e-12).all()
    assert XW.gamma(XW.N_FILTER) * float(S.max()) < 1e-5 * float(np.abs(U).max())
    assert XW.gamma(XW.N_WGRAD_FINISH) < 8e-7
    assert np.array_equal(XW.filter_transform(4 * w9, 2), np.round(XW.filter_transform(4 * w9, 2)))

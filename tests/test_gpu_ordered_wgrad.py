"""The ordered (bitwise-reproducible) gradient kernels: ssp_conv_wgrad_ordered on every route family and the stride-2
filter gradient, ssp_conv_wgrad_wino_ordered (tiles 2 and 4), ssp_conv_s2_dgrad_ordered and the refused BatchNorm-sum fold.

Exact integers (tests/exact_conv.py, tests/strided_cases.py): torch.equal against the int64 references on top of an integer
prefill, with the library's split and forced ones, a NaN-poisoned workspace whose every owned float must be written and
whose guard floats - like those around dw - must keep their NaN bits.  Real data: standard-normal operands, three launches
into fresh buffers must be torch.equal (also with another kernel busy on a second stream), different splits agree with a
float64 reference at the 1e-4 bar of tests/test_gpu_kernels.py::test_conv_dgrad_wgrad."""
import functools

import numpy as np
import pytest
import torch

import exact_conv as E
import strided_cases as S
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAN = float('nan')
GUARD = 64
SPLITS = (0, 1, 2, 3, 7, 1 << 20)      # library's choice, forced ones, one far past what the pixel count allows (clamped)


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


def _assert_equal(got, want, names):
    assert torch.equal(got, want), E.first_diffs(got, want, names)


def _guarded(values, G):
    """values [n] fp32 between two NaN guards, on the device: (buffer, offset of the values)."""
    buf = torch.full((values.numel() + 2 * GUARD,), NAN, dtype=torch.float32)
    buf[GUARD:GUARD + values.numel()] = values.reshape(-1)
    return buf.to(G.dev()), GUARD


def _guards_kept(buf, n):
    b = buf.cpu()
    return bool(torch.isnan(b[:GUARD]).all() and torch.isnan(b[GUARD + n:]).all())


def _ordered(_lib, G, dyp, xp, dw0, geom, stride, split, flags=0):
    """One ssp_conv_wgrad_ordered launch onto a copy of dw0 (fp32 [n]) between NaN guards, with a NaN-poisoned, guarded
    workspace of exactly the queried size.  Returns (dw [n] on the CPU, nsplit) after the ownership checks."""
    B, H, W, cinp, Cout, lddy, ldx, R = geom
    ns = _lib.query('ssp_conv_wgrad_ordered_split', B, H, W, cinp, Cout, lddy, ldx, R, stride, split)
    need = _lib.query('ssp_conv_wgrad_ordered_workspace_floats', B, H, W, cinp, Cout, lddy, ldx, R, stride, split)
    n = dw0.numel()
    assert ns >= 1 and need == ns * n, (ns, need, n)
    ws, wo = _guarded(torch.full((need,), NAN), G)
    dw, do = _guarded(dw0, G)
    _lib.call('ssp_conv_wgrad_ordered', dyp, xp, G.p(dw, do), B, H, W, cinp, Cout, lddy, ldx, R, stride, split, flags,
              G.p(ws, wo), need, G.stream())
    torch.cuda.synchronize()
    assert _guards_kept(ws, need) and _guards_kept(dw, n), "wrote outside the workspace / gradient it owns"
    assert bool(torch.isfinite(ws[wo:wo + need]).all()), "a slab element of the workspace was not written"
    return dw.cpu()[do:do + n], ns


# ------------------------------------------------------------------------------------------------ exact integers, stride 1
def _plain_cases():
    """E.WGRAD_CASES without the experiment options (the ordered entry point does not read process state): one case per
    distinct operand form."""
    seen, out = set(), []
    for c in E.WGRAD_CASES:
        k = (c.shape, c.ldx, c.xoff, c.lddy, c.dyoff)
        if k not in seen:
            seen.add(k)
            out.append(c._replace(opts=(), id=c.id.split('-split')[0].split('-variant')[0]))
    return out


PLAIN = _plain_cases()


@pytest.mark.parametrize("c", PLAIN, ids=lambda c: c.id)
def test_ordered_wgrad_every_route_exact(c):
    """Library split and one forced split per case (rotating through SPLITS) on top of an integer prefill."""
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    cinp = E.pad4(Cin)
    x, dy, _ = E.operands(c.shape, *c.shape)
    ref = E.ref_wgrad(dy, x, R)
    pre = E.prefill(c.shape, ref.shape)
    xd = E.nhwc_buffer(x, c.ldx, c.xoff).to(G.dev())
    dyd = E.nhwc_buffer(dy, c.lddy, c.dyoff).to(G.dev())
    geom = (B, H, W, cinp, Cout, c.lddy, c.ldx, R)
    route = _lib.query('ssp_conv_wgrad_route', *geom)
    assert route != 0
    if not c.id.startswith(('var', 'split', 'xcd')):
        assert route == c.route, (route, c.route)
    forced = SPLITS[1 + PLAIN.index(c) % (len(SPLITS) - 1)]
    for split in (0, forced):
        got, ns = _ordered(_lib, G, G.p(dyd, c.dyoff), G.p(xd, c.xoff), pre.float(), geom, 1, split, flags=split & 1)
        assert split == 0 or ns <= split
        _assert_equal(got.reshape(ref.shape), (ref + pre).float(), ('co', 'tap', 'ci'))


@pytest.mark.parametrize("name,shape", [('lds128x128', (2, 13, 13, 128, 128, 3)), ('lds256x128', (2, 13, 13, 128, 256, 3)),
                                        ('fold128x64', (1, 9, 11, 32, 128, 3)), ('reg32x32', (3, 7, 9, 32, 20, 1)),
                                        ('reg64x32', (2, 9, 11, 32, 64, 1)), ('c4', (1, 20, 24, 3, 32, 3))])
def test_ordered_wgrad_forced_splits_exact(name, shape):
    """Splits 1, 2, 3 and 7 and one past the chunk count: 338 pixels in 16-pixel chunks make 7 ranges asked for 6 (the last
    one partial), the huge request is clamped to one chunk per range."""
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = shape
    cinp, coutp = E.pad4(Cin), E.pad4(Cout)
    x, dy, _ = E.operands(shape, *shape)
    ref = E.ref_wgrad(dy, x, R)
    pre = E.prefill(shape, ref.shape)
    xd = E.nhwc_buffer(x).to(G.dev())
    dyd = E.nhwc_buffer(dy).to(G.dev())
    geom = (B, H, W, cinp, Cout, coutp, cinp, R)
    M = B * H * W
    seen = {}
    for split in SPLITS:
        got, ns = _ordered(_lib, G, dyd.data_ptr(), xd.data_ptr(), pre.float(), geom, 1, split)
        seen[split] = ns
        _assert_equal(got.reshape(ref.shape), (ref + pre).float(), ('co', 'tap', 'ci'))
    assert seen[1] == 1 and seen[2] <= 2 and seen[7] <= 7
    assert seen[1 << 20] <= (M + 15) // 16 and seen[1 << 20] >= min(7, seen[7])      # clamped, not refused
    if shape[:3] == (2, 13, 13) and name.startswith('lds'):
        assert seen[7] == 6 and seen[1 << 20] == 22      # 64-pixel ranges: five whole and one of 18; 22 ranges of one chunk


# ------------------------------------------------------------------------------------------------ exact integers, stride 2
@functools.lru_cache(maxsize=None)
def _s2(shape):
    x, dy, w = S.operands(shape)
    B, H, W, Cin, Cout, R = shape
    return dict(x=x, dy=dy, w=w, wgrad=S.ref_wgrad(dy, x, R), dgrad=S.ref_dgrad(dy, w, H, W))


@pytest.mark.parametrize('c', S.CASES, ids=S.case_id)
def test_ordered_s2_wgrad_exact(c):
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    d = _s2(c.shape)
    ldx, ldy, off = S.buffers(c)
    xd = E.nhwc_buffer(d['x'], ldx, off).to(G.dev())
    dyd = E.nhwc_buffer(d['dy'], ldy, off).to(G.dev())
    pre = E.prefill(c.shape, d['wgrad'].shape)
    geom = (B, H, W, E.pad4(Cin), Cout, ldy, ldx, R)
    for split in (0, SPLITS[1 + S.CASES.index(c) % (len(SPLITS) - 1)]):
        got, _ = _ordered(_lib, G, G.p(dyd, off), G.p(xd, off), pre.float(), geom, 2, split)
        _assert_equal(got.reshape(d['wgrad'].shape), (d['wgrad'] + pre).float(), ('co', 'tap', 'ci'))


@pytest.mark.parametrize('accumulate', [0, 1], ids=['plain', 'acc'])
@pytest.mark.parametrize('c', S.CASES, ids=S.case_id)
def test_ordered_s2_dgrad_exact(c, accumulate):
    """Every table shape is a grid under 512 workgroups (S.dgrad_workgroups): the atomic entry point would split them by taps."""
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = c.shape
    d = _s2(c.shape)
    ldx, ldy, off = S.buffers(c)
    dyd = E.nhwc_buffer(d['dy'], ldy, off).to(G.dev())
    wd = E.pack_dgrad(d['w']).float().to(G.dev())
    M = B * H * W
    pre = E.prefill(c.shape, (M, Cin))
    dx = torch.full((M, ldx), NAN, dtype=torch.float32)
    if accumulate:
        dx[:, off:off + Cin] = pre.float()
    dx = dx.to(G.dev())
    before = dx.clone()
    _lib.call('ssp_conv_s2_dgrad_ordered', G.p(dyd, off), wd.data_ptr(), G.p(dx, off), B, H, W, E.pad4(Cout), Cin, ldy, ldx, R,
              accumulate, G.stream())
    torch.cuda.synchronize()
    want = d['dgrad'].reshape(M, Cin).float() + (pre.float() if accumulate else 0)
    _assert_equal(dx.cpu()[:, off:off + Cin], want, ('pixel', 'ci'))
    a, b = dx.cpu().view(torch.int32), before.cpu().view(torch.int32)
    assert torch.equal(a[:, :off], b[:, :off]) and torch.equal(a[:, off + Cin:], b[:, off + Cin:])


def test_ordered_s2_dgrad_run_to_run_equal():
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = 2, 13, 13, 64, 128, 3
    assert S.dgrad_workgroups((B, H, W, Cin, Cout, R))[1], "the shape must be one the atomic form splits by taps"
    rs = np.random.RandomState(5)
    Ho, Wo = S.out_hw(H, W, R)
    dy = torch.from_numpy(rs.standard_normal((B * Ho * Wo, Cout)).astype(np.float32)).to(G.dev())
    w = torch.from_numpy(rs.standard_normal((Cin, R * R, Cout)).astype(np.float32)).to(G.dev())
    outs = []
    for _ in range(3):
        dx = torch.full((B * H * W, Cin), NAN, dtype=torch.float32, device=G.dev())
        _lib.call('ssp_conv_s2_dgrad_ordered', dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, H, W, Cout, Cin, Cout, Cin, R, 0,
                  G.stream())
        torch.cuda.synchronize()
        outs.append(dx.cpu())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    ref = torch.full((B * H * W, Cin), NAN, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_conv_s2_dgrad', dy.data_ptr(), w.data_ptr(), ref.data_ptr(), B, H, W, Cout, Cin, Cout, Cin, R, 0, G.stream())
    torch.cuda.synchronize()
    assert rel_err(outs[0].numpy(), ref.cpu().numpy()) < TOL


# ------------------------------------------------------------------------------------------------ Winograd, tiles 2 and 4
@pytest.mark.parametrize("tile,shape", [(t, s) for t, s in E.WINO_WGRAD_CASES if t in (2, 4)], ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize("split", [2, 3])
def test_ordered_wino_wgrad_forced_split(tile, shape, split):
    """ssp_conv_wgrad_wino_ordered on channel slices into a non-zero dw, NaN-poisoned workspace: tile 2 bit for bit, tile 4
    (thirds in G) on the same inputs at 1e-4 - as tests/test_gpu_conv_exact.py::test_wino_wgrad_sliced_accumulating."""
    G, _lib = _imports()
    B, H, W, Cin, Cout = shape
    s6 = shape + (3,)
    x, dy, _ = E.operands(s6, *s6)
    ref = E.ref_wgrad(dy, x, 3)
    pre = E.prefill(s6, ref.shape)
    ldx, xoff, lddy, dyoff = Cin + 16, 8, Cout + 12, 4
    xd = E.nhwc_buffer(x, ldx, xoff).to(G.dev())
    dyd = E.nhwc_buffer(dy, lddy, dyoff).to(G.dev())
    ns = _lib.query('ssp_conv_wgrad_wino_ordered_split', B, H, W, Cin, Cout, tile, split)
    need = _lib.query('ssp_conv_wgrad_wino_ordered_workspace_floats', B, H, W, Cin, Cout, tile, split)
    base = _lib.query('ssp_conv_wgrad_wino_workspace_floats_t', B, H, W, Cin, Cout, tile)
    assert ns >= 2 and need == base + (ns - 1) * (tile + 2) ** 2 * Cin * Cout
    ws, wo = _guarded(torch.full((need,), NAN), G)
    dw, do = _guarded(pre.float(), G)
    _lib.call('ssp_conv_wgrad_wino_ordered', G.p(dyd, dyoff), G.p(xd, xoff), G.p(dw, do), B, H, W, Cin, Cout, lddy, ldx, tile,
              split, G.p(ws, wo), need, G.stream())
    torch.cuda.synchronize()
    assert _guards_kept(ws, need) and _guards_kept(dw, pre.numel())
    got, want = dw.cpu()[do:do + pre.numel()].reshape(ref.shape), (ref + pre).float()
    if tile == 4:
        err = rel_err(got.numpy(), want.numpy())
        print('ordered F(4x4) filter gradient vs int64: %.2e' % err)
        assert err < TOL
    else:
        _assert_equal(got, want, ('co', 'tap', 'ci'))


def test_ordered_wino_refuses_the_on_chip_tile():
    G, _lib = _imports()
    assert _lib.query('ssp_conv_wgrad_wino_ordered_split', 2, 13, 13, 64, 128, 12, 0) == 0
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=G.dev())
    with pytest.raises(_lib.SspError, match='tile must be 2 or 4'):
        _lib.call('ssp_conv_wgrad_wino_ordered', buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 8, 8, 64, 64, 64, 64, 12, 0,
                  buf.data_ptr(), buf.numel(), G.stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ order-fixed on real data
REAL = [('lds128x128', (2, 13, 13, 128, 128, 3), 1), ('lds64x128', (3, 9, 11, 128, 64, 3), 1), ('fold', (1, 9, 11, 32, 128, 3), 1),
        ('reg', (3, 7, 9, 32, 20, 1), 1), ('c4', (2, 20, 24, 4, 32, 3), 1), ('s2', (2, 13, 13, 64, 128, 3), 2)]


@functools.lru_cache(maxsize=None)
def _real(shape, stride):
    """Standard-normal dy / x (NHWC, padded channels zero) and the float64 filter gradient [Cout][R*R][cinp]."""
    B, H, W, Cin, Cout, R = shape
    rs = np.random.RandomState(sum(shape) + stride)
    Ho, Wo = S.out_hw(H, W, R) if stride == 2 else (H, W)
    coutp = E.pad4(Cout)
    x = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    dy = np.zeros((B, Ho, Wo, coutp), np.float32)
    dy[..., :Cout] = rs.standard_normal((B, Ho, Wo, Cout)).astype(np.float32)
    xp = np.pad(x.astype(np.float64), ((0, 0), (R // 2,) * 2, (R // 2,) * 2, (0, 0)))
    dyt = dy[..., :Cout].astype(np.float64).reshape(-1, Cout).T
    ref = np.zeros((Cout, R * R, Cin))
    for ky in range(R):
        for kx in range(R):
            win = xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride, :]
            ref[:, ky * R + kx, :] = dyt @ win.reshape(-1, Cin)
    return torch.from_numpy(x.reshape(-1, Cin)), torch.from_numpy(dy.reshape(-1, coutp)), ref


@pytest.mark.parametrize("name,shape,stride", REAL, ids=[r[0] for r in REAL])
def test_ordered_wgrad_same_bits_every_launch(name, shape, stride):
    G, _lib = _imports()
    B, H, W, Cin, Cout, R = shape
    x, dy, ref = _real(shape, stride)
    xd, dyd = x.to(G.dev()), dy.to(G.dev())
    geom = (B, H, W, Cin, Cout, dy.shape[1], Cin, R)
    n = Cout * R * R * Cin
    zero = torch.zeros(n)
    runs = [_ordered(_lib, G, dyd.data_ptr(), xd.data_ptr(), zero, geom, stride, 0)[0] for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    # an unrelated kernel busy on a second stream while the launch runs
    side = torch.cuda.Stream()
    a = torch.randn(1024, 1024, device=G.dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            a = a @ a * 1e-3
    busy = _ordered(_lib, G, dyd.data_ptr(), xd.data_ptr(), zero, geom, stride, 0)[0]
    torch.cuda.synchronize()
    assert torch.equal(busy, runs[0])
    # other splits: the same sum to rounding, each against float64
    for split in (0, 1, 3, 7):
        for flags in (0, 1):
            got = _ordered(_lib, G, dyd.data_ptr(), xd.data_ptr(), zero, geom, stride, split, flags)[0]
            err = rel_err(got.numpy().reshape(ref.shape), ref)
            print('%s split %d %s finishing sum: %.2e of the float64 reference' % (name, split, 'fp32' if flags else 'float64', err))
            assert err < TOL
            assert rel_err(got.numpy(), runs[0].numpy()) < TOL


# ------------------------------------------------------------------------------------------------ refused fold
@pytest.mark.parametrize("entry", ['ssp_conv_dgrad_bnbwd', 'ssp_conv_dgrad_adj_bnbwd'])
def test_refused_fold_is_an_error_and_writes_nothing(entry):
    G, _lib = _imports()
    B, H, W, C = 4, 16, 16, 64
    plan = 9006413 if 'adj' in entry else 0
    ntile = _lib.query('ssp_conv_stats_tiles', B, H, W, C, C, 3, plan)
    assert ntile > 1
    M = B * H * W
    dy = torch.randn(M, C, device=G.dev())
    wt = torch.randn(36 * C * C, device=G.dev())
    raw = torch.randn(M, C, device=G.dev())
    vec = torch.ones(4, C, device=G.dev())
    dx = torch.full((M, C), NAN, dtype=torch.float32, device=G.dev())
    partial = torch.full((ntile * C * 2,), NAN, dtype=torch.float32, device=G.dev())
    wsn = max(1, _lib.query('ssp_conv_workspace_floats', B, H, W, C, C, 3, plan))
    ws = torch.empty(wsn, dtype=torch.float32, device=G.dev())
    tail = (None, G.stream()) if 'adj' in entry else (G.stream(),)
    args = lambda rows: (dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), B, H, W, C, C, C, C, 3, plan, ws.data_ptr(), wsn,
                         raw.data_ptr(), C, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), 0.1,
                         partial.data_ptr(), rows) + tail
    with pytest.raises(_lib.SspError, match='folding'):
        _lib.call(entry, *args(-(ntile - 1)))
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(partial).all())
    _lib.call(entry, *args(-ntile))          # enough rows: plain stores, every row written
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(partial).all())

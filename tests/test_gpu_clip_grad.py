"""Global-norm gradient clipping on the GPU (ssp_grad_sumsq_table + ssp_grad_scale_table,
singleshotpose_amd.optim.clip_grad_norm_) against the float64 statement of adam_cases.py.

The bounds are derived, not measured: the squares of fp32 values are exact in double and their sum errs by at most
n * 2^-53 relative, so the returned fp32 norm is within one fp32 ulp of the float64 norm; a scaled element is g * coef with
coef rounded once to fp32 and the product rounded once: within 2^-23 relative of the float64 product."""
import ctypes

import numpy as np
import pytest
import torch

import adam_cases as A

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _clip(g, rows, max_norm, partial=None):
    """The two launches over a table (rows [[., grad offset, ., length, .]]) or, rows None, over the whole of g."""
    from singleshotpose_amd import _lib
    count = ctypes.c_int(0)
    partial = torch.full((2048,), float('nan'), dtype=torch.float64, device='cuda') if partial is None else partial
    result = torch.full((2,), -1.0, device='cuda')
    if rows is None:
        tab = (None, None, 1)
        dev = None
    else:
        host = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        dev = torch.from_numpy(host).cuda()
        tab = (dev.data_ptr(), host.ctypes.data, len(rows))
    _lib.call('ssp_grad_sumsq_table', g.data_ptr(), g.numel(), *(tab + (partial.data_ptr(), partial.numel(),
              ctypes.cast(ctypes.byref(count), ctypes.c_void_p), _stream())))
    _lib.call('ssp_grad_scale_table', g.data_ptr(), g.numel(), *(tab + (partial.data_ptr(), count.value, float(max_norm),
              result.data_ptr(), _stream())))
    torch.cuda.synchronize()
    return result.cpu().numpy(), partial[:count.value].cpu().numpy(), count.value


def _check(got, g0, segments, result, max_norm):
    """got / g0: the buffer after / before (numpy fp32); segments [(offset, length)]."""
    norm, coef, scaled = A.clip_statement([g0[o:o + n] for o, n in segments], max_norm)
    assert abs(float(result[0]) - norm) <= np.spacing(np.float32(norm)), (result[0], norm)
    assert abs(float(result[1]) - coef) <= 2.0 ** -23 * coef      # one rounding to fp32 (2^-24) and the double sum's error
    for (o, n), want in zip(segments, scaled):
        err = np.abs(got[o:o + n].astype(np.float64) - want)
        assert (err <= 2.0 ** -23 * np.abs(want)).all(), (o, n, float(err.max()))
    return norm, coef


@pytest.mark.parametrize('n', A.LENGTHS)
def test_one_range_against_the_float64_statement(n):
    rs = np.random.RandomState(A.SEED + n)
    g0 = (rs.standard_normal(n) * 0.3).astype(np.float32)
    ref_norm = A.clip_statement([g0], 1.0)[0]
    for max_norm in (0.25 * ref_norm, 4.0 * ref_norm):
        g = torch.from_numpy(g0.copy()).cuda()
        result, partial, count = _clip(g, None, max_norm)
        assert count == min((n + A.CHUNK - 1) // A.CHUNK, A.GRID)
        norm, coef = _check(g.cpu().numpy(), g0, [(0, n)], result, max_norm)
        if max_norm > ref_norm:
            # nothing to clip: coef is exactly 1 and the gradient comes back bit for bit
            assert result[1] == 1.0 and np.array_equal(g.cpu().numpy().view(np.uint32), g0.view(np.uint32))
        else:
            assert result[1] < 1.0
        # a second call on restored inputs: the same bits in the partial sums, the result and the gradient
        g2 = torch.from_numpy(g0.copy()).cuda()
        result2, partial2, _ = _clip(g2, None, max_norm)
        assert np.array_equal(result.view(np.uint32), result2.view(np.uint32))
        assert np.array_equal(partial.view(np.uint64), partial2.view(np.uint64))
        assert torch.equal(g.view(torch.int32), g2.view(torch.int32))


def test_segment_table_with_poisoned_gaps():
    """~300 short segments and one that wraps the grid; the floats between them carry a NaN bit pattern, which must neither
    reach the norm nor be written."""
    rows4, _, ng, _ = A.segment_layout(A.LENGTHS[-1])
    rows = [r + [0] for r in rows4]
    segments = [(r[1], r[3]) for r in rows]
    rs = np.random.RandomState(A.SEED + 8)
    g0 = A.poisoned(ng)
    gap = np.ones(ng, dtype=bool)
    for o, n in segments:
        g0[o:o + n] = rs.standard_normal(n) * 0.01
        gap[o:o + n] = False
    ref_norm = A.clip_statement([g0[o:o + n] for o, n in segments], 1.0)[0]
    outs = []
    for max_norm in (0.5 * ref_norm, 0.5 * ref_norm, 2.0 * ref_norm):
        g = torch.from_numpy(g0.copy()).cuda()
        result, partial, count = _clip(g, rows, max_norm)
        assert count == A.GRID and np.isfinite(result).all() and np.isfinite(partial).all()
        got = g.cpu().numpy()
        _check(got, g0, segments, result, max_norm)
        assert np.array_equal(got.view(np.uint32)[gap], g0.view(np.uint32)[gap])
        outs.append((result, partial, got))
    # run to run: identical bits
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # max_norm above the norm: bit-identical gradients
    assert outs[2][0][1] == 1.0 and np.array_equal(outs[2][2].view(np.uint32), g0.view(np.uint32))


def test_several_sumsq_launches_fill_one_partial_array():
    """The per-tensor form: each tensor's sum of squares goes to its own part of one partial array, one scale launch per
    tensor then uses the whole array."""
    from singleshotpose_amd import _lib
    rs = np.random.RandomState(A.SEED + 10)
    g0 = [(rs.standard_normal(n) * 0.2).astype(np.float32) for n in (5, 4099, 3 * 4096 + 1)]
    gs = [torch.from_numpy(a.copy()).cuda() for a in g0]
    partial = torch.full((64,), float('nan'), dtype=torch.float64, device='cuda')
    result = torch.zeros(2, device='cuda')
    count, used = ctypes.c_int(0), 0
    for g in gs:
        _lib.call('ssp_grad_sumsq_table', g.data_ptr(), g.numel(), None, None, 1, partial.data_ptr() + 8 * used, 2,
                  ctypes.cast(ctypes.byref(count), ctypes.c_void_p), _stream())
        assert 1 <= count.value <= 2      # never more partials than there is room for
        used += count.value
    ref_norm = A.clip_statement(g0, 1.0)[0]
    for g in gs:
        _lib.call('ssp_grad_scale_table', g.data_ptr(), g.numel(), None, None, 1, partial.data_ptr(), used, 0.5 * ref_norm,
                  result.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert used == 5 and torch.isnan(partial[used:]).all()
    norm, coef, scaled = A.clip_statement(g0, 0.5 * ref_norm)
    assert abs(float(result[0]) - norm) <= np.spacing(np.float32(norm))
    for g, want in zip(gs, scaled):
        assert (np.abs(g.cpu().numpy().astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want)).all()


BAD = [('null gradient', dict(g=None), 'null'), ('misaligned gradient', dict(shift=4), 'aligned'),
       ('row past the end', dict(row=[0, 60, 0, 8, 0]), 'outside the gradient'), ('row misaligned', dict(row=[0, 2, 0, 8, 0]), 'multiples of 4'),
       ('row negative', dict(row=[0, -4, 0, 8, 0]), 'multiples of 4'), ('row empty', dict(row=[0, 0, 0, 0, 0]), 'length'),
       ('no room', dict(room=0), 'room'), ('max_norm negative', dict(max_norm=-1.0), 'max_norm'),
       ('max_norm NaN', dict(max_norm=float('nan')), 'max_norm'), ('no partials', dict(npartial=0), 'partial sums'),
       ('too many partials', dict(npartial=65537), 'partial sums'), ('no result', dict(result=None), 'result')]


@pytest.mark.parametrize('what,spec,why', BAD, ids=[b[0].replace(' ', '-') for b in BAD])
def test_refusals_launch_nothing(what, spec, why):
    from singleshotpose_amd import _lib
    g = torch.full((64,), 3.0, device='cuda')
    partial = torch.full((8,), 7.0, dtype=torch.float64, device='cuda')
    result = torch.full((2,), -1.0, device='cuda')
    rows = [[0, 0, 0, 5, 0], spec.get('row', [0, 8, 0, 8, 0])]
    host = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
    dev = torch.from_numpy(host).cuda()
    gp = None if 'g' in spec else g.data_ptr() + spec.get('shift', 0)
    count = ctypes.c_int(-5)
    sumsq = lambda: _lib.call('ssp_grad_sumsq_table', gp, 64, dev.data_ptr(), host.ctypes.data, 2, partial.data_ptr(),
                              spec.get('room', 8), ctypes.cast(ctypes.byref(count), ctypes.c_void_p), _stream())
    scale = lambda: _lib.call('ssp_grad_scale_table', gp, 64, dev.data_ptr(), host.ctypes.data, 2, partial.data_ptr(),
                              spec.get('npartial', 2), spec.get('max_norm', 1.0),
                              None if 'result' in spec else result.data_ptr(), _stream())
    sumsq_fails = any(k in spec for k in ('g', 'shift', 'row', 'room'))
    scale_fails = any(k in spec for k in ('g', 'shift', 'row', 'max_norm', 'npartial', 'result'))
    if sumsq_fails:
        with pytest.raises(_lib.SspError, match=why):
            sumsq()
    if scale_fails:
        with pytest.raises(_lib.SspError, match=why):
            scale()
    torch.cuda.synchronize()
    assert count.value == -5 or not sumsq_fails
    assert (g == 3.0).all() and (partial == 7.0).all() and (result == -1.0).all()


# ------------------------------------------------------------------------------------------------ the Python surface
def _flat_params(shapes, rs, scale=0.1):
    """Parameters whose .grad are views of ONE flat buffer, as Plan.backward leaves them (offsets rounded up to 4)."""
    total = sum((int(np.prod(s)) + 3) // 4 * 4 for s in shapes)
    flat = torch.zeros(total, device='cuda')
    ps, off = [], 0
    for s in shapes:
        n = int(np.prod(s))
        p = torch.nn.Parameter(torch.from_numpy(rs.standard_normal(s).astype(np.float32)).cuda())
        flat[off:off + n] = torch.from_numpy((rs.standard_normal(n) * scale).astype(np.float32)).cuda()
        p.grad = flat[off:off + n].view(s)
        ps.append(p)
        off += (n + 3) // 4 * 4
    return ps, flat


SHAPES = [(16, 3, 3, 3), (16,), (33, 7), (5,), (4099,)]


@pytest.mark.parametrize('flat_views', [True, False], ids=['flat-views', 'separate-tensors'])
def test_clip_grad_norm_matches_the_statement_and_returns_a_device_tensor(flat_views, monkeypatch):
    from singleshotpose_amd import _lib, optim
    rs = np.random.RandomState(A.SEED + 11)
    ps, flat = _flat_params(SHAPES, rs)
    if not flat_views:
        for p in ps:
            p.grad = p.grad.clone()
    g0 = [p.grad.detach().cpu().numpy().ravel().copy() for p in ps]
    ref_norm = A.clip_statement(g0, 1.0)[0]
    log = []
    orig = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (log.append(name), orig(name, *a))[1])
    total = optim.clip_grad_norm_(ps, 0.5 * ref_norm)
    assert total.is_cuda and total.dim() == 0 and total.dtype == torch.float32
    launches = 1 if flat_views else len(ps)
    assert log.count('ssp_grad_sumsq_table') == launches and log.count('ssp_grad_scale_table') == launches
    norm, coef, scaled = A.clip_statement(g0, 0.5 * ref_norm)
    assert abs(float(total) - norm) <= np.spacing(np.float32(norm))
    for p, want in zip(ps, scaled):
        assert (np.abs(p.grad.cpu().numpy().ravel().astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want)).all()
    # above the norm: nothing changes, bit for bit; the norm is that of the clipped gradients now
    before = [p.grad.clone() for p in ps]
    total2 = optim.clip_grad_norm_(ps, 10.0 * ref_norm)
    assert all(torch.equal(a.view(torch.int32), p.grad.view(torch.int32)) for a, p in zip(before, ps))
    assert abs(float(total2) - 0.5 * ref_norm) <= 4 * np.spacing(np.float32(ref_norm))
    # a NaN gradient: the norm is NaN, error_if_nonfinite raises torch's message
    ps[2].grad.view(-1)[3] = float('nan')
    with pytest.raises(RuntimeError, match='non-finite'):
        optim.clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)


@pytest.mark.parametrize('which', ['SGD', 'Adam'])
def test_optimizers_accept_the_clipped_views_and_keep_their_one_launch_step(which):
    """clip_grad_norm_ in front of optim.SGD and optim.Adam: the gradients stay views of the flat buffer, the step stays
    one launch, and the update equals torch's optimizer fed the statement's clipped gradients (rel_err < 1e-6)."""
    from helpers import rel_err
    from singleshotpose_amd import optim
    rs = np.random.RandomState(A.SEED + 12)
    ps, flat = _flat_params(SHAPES, rs)
    sh = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    if which == 'SGD':
        kw = dict(lr=1e-2, momentum=0.9, weight_decay=0.01)
        opt, osh = optim.SGD(ps, **kw), torch.optim.SGD(sh, **kw)
    else:
        kw = dict(lr=1e-2, weight_decay=0.01)
        opt, osh = optim.Adam(ps, **kw), torch.optim.Adam(sh, **kw)
    for step in range(2):
        for p in ps:
            p.grad.copy_(torch.from_numpy((rs.standard_normal(tuple(p.shape)) * 0.1).astype(np.float32)).cuda())
        g0 = [p.grad.detach().cpu().numpy().copy() for p in ps]
        ref_norm = A.clip_statement(g0, 1.0)[0]
        optim.clip_grad_norm_(ps, 0.3 * ref_norm)
        for q, want in zip(sh, A.clip_statement(g0, 0.3 * ref_norm)[2]):
            q.grad = torch.from_numpy(want.astype(np.float32))
        opt.step()
        osh.step()
        for p, q in zip(ps, sh):
            assert rel_err(p.detach().cpu().numpy(), q.detach().numpy()) < 1e-6, step
    assert opt.fused_steps == 2 and opt.table_steps == 0

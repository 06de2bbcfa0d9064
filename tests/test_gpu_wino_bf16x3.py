"""The bf16x3 twin codes of the through-memory Winograd plans (base + 600000 + tile_rows * 100 + 13; mode 'bf16x3-wino') on
the GPU: the plan's batched GEMM on the bf16 matrix cores (csrc/conv_igemm_bf16x3.hip as a batched launch).

  1  the GEMM bit for bit: M (dV) read back from the caller's workspace equals sum_k U V evaluated in float64 from the V (dM)
     the launch itself left there, on the operand classes of tests/exact_wino_bf16x3.py that together need each of the six
     products (tests/test_wino_bf16x3_cpu.py pins that); nothing outside the planes and the output slice is written;
  2  the whole launch against its fp32 twin on the same operands: torch.equal (M is exact in both, the finishing pass is the
     same code) - plain, accumulating, ldout > Cout, BatchNorm statistics, fused BatchNorm-backward sums;
  3  every misfit row, on the three entry points: an error with a message, nothing written;
  4  accuracy on random operands against float64 and against the fp32 Winograd code;
  5  the mode through the engine, with the tuner driven by a scripted clock."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_conv as E
import exact_data as X
import exact_wino as XW
import exact_wino_bf16x3 as XB
from helpers import rel_err

pytestmark = pytest.mark.gpu
NAN = float('nan')
GUARD = 1 << 14               # NaN floats in front of and behind every carved buffer
PLANE = ('plane', 'tile', 'channel')
PIXEL = ('pixel', 'channel')


def _imports():
    import gpu_util as G
    from singleshotpose_amd import _lib
    return G, _lib


def _carve(G, n, fill=None):
    """n floats out of the middle of a NaN-filled buffer: (whole buffer, view of the middle); fill: float64 array."""
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device=G.dev())
    mid = buf[GUARD:GUARD + n]
    if fill is not None:
        mid.copy_(XW.f32(fill).reshape(-1))
    return buf, mid


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _eq(got, want, names, what=''):
    assert torch.equal(got, want), '%s: %s' % (what, E.first_diffs(got, want, names))


def _out(G, M, ld, off, N, pre=None):
    out = torch.full((M, ld), NAN, dtype=torch.float32)
    if pre is not None:
        out[:, off:off + N] = XW.f32(pre)
    return out.to(G.dev())


def _slice_of(out, off, N, what):
    o = out.cpu()
    assert torch.isnan(o[:, :off]).all() and torch.isnan(o[:, off + N:]).all(), '%s: wrote outside its channel slice' % what
    return o[:, off:off + N].contiguous()


def _contract(V, U):
    """exact_wino.contract ([P][T][K] x [P][N][K] -> [P][T][N]) as one batched matmul: integers below 2^53, exact in any order."""
    return np.matmul(V, np.swapaxes(U, 1, 2))


@functools.lru_cache(maxsize=None)
def _operands(cls, c, entry):
    """(V-like planes, U, pixel map or None, the float64 GEMM result [P][T][N]) - computed once, never changed."""
    V, U, px = XB.gemm_operands(cls, c, entry)
    return V, U, px, _contract(V, U)


class _Run(object):
    """One launch of an entry point on a case's operands: buffers carved out of NaN, the input / output maps sliced."""

    def __init__(self, G, _lib, c, entry, cls):
        self.G, self.L, self.c, self.entry = G, _lib, c, entry
        B, H, W = c.shape
        self.M, self.P, self.g = B * H * W, (c.tile + 2) ** 2, XB.geom(c)
        self.V, self.U, self.px, self.gemm = _operands(cls, c, entry)
        self.ldin, self.inoff, self.ldout, self.outoff = c.K + 16, 8, c.N + 12, 4
        self.Ud = XW.f32(self.U).to(G.dev())
        self.ind = XW.nhwc(self.px, self.ldin, self.inoff).to(G.dev()) if self.px is not None else \
            torch.full((self.M, self.ldin), NAN, dtype=torch.float32, device=G.dev())
        nPK, nPN = self.P * self.g.T * c.K, self.P * self.g.T * c.N
        self.nPK, self.nPN = nPK, nPN
        if entry in ('fwd', 'dgrad'):
            self.wsn = nPK + nPN
        else:
            self.wsn = nPN + (nPK if entry == 'adj-own' else 0)

    def launch(self, plan, accumulate=0, pre=None, ldout=None, outoff=None, stats=None, bnb=None):
        G, L, c = self.G, self.L, self.c
        B, H, W = c.shape
        ldout = self.ldout if ldout is None else ldout
        outoff = self.outoff if outoff is None else outoff
        self.out = _out(G, self.M, ldout, outoff, c.N, pre)
        self.wbuf, self.ws = _carve(G, self.wsn)
        self.mbuf, self.dM = _carve(G, self.nPK, self.V if self.entry == 'adj-dm' else None)
        inp, outp = G.p(self.ind, self.inoff), G.p(self.out, outoff)
        head = (inp, self.Ud.data_ptr(), outp)
        dims = (B, H, W, c.K, c.N, self.ldin, ldout, 3)
        wsa = (self.ws.data_ptr(), self.wsn)
        dm = (self.dM.data_ptr() if self.entry == 'adj-dm' else None,)
        if bnb is not None:
            if self.entry == 'dgrad':
                L.call('ssp_conv_dgrad_bnbwd', *head, *dims, plan, *wsa, *bnb, G.stream())
            else:
                L.call('ssp_conv_dgrad_adj_bnbwd', *head, *dims, plan, *wsa, *bnb, *dm, G.stream())
        elif self.entry == 'fwd':
            L.call('ssp_conv_fwd', *head[:3], None, stats, *dims, accumulate, plan, *wsa, G.stream())
        elif self.entry == 'dgrad':
            L.call('ssp_conv_dgrad', *head, *dims, accumulate, plan, *wsa, G.stream())
        else:
            L.call('ssp_conv_dgrad_adj', *head, *dims, accumulate, plan, *wsa, *dm, G.stream())
        torch.cuda.synchronize()
        what = '%s %s plan %d' % (c.id, self.entry, plan)
        got = _slice_of(self.out, outoff, c.N, what)
        assert _guards_intact(self.wbuf) and _guards_intact(self.mbuf), what + ': wrote outside its workspace'
        return got

    def planes(self):
        """(the V-like operand the launch left / was given, the GEMM's output planes), on the CPU."""
        P, T, K, N = self.P, self.g.T, self.c.K, self.c.N
        if self.entry in ('fwd', 'dgrad'):
            return self.ws[:self.nPK].cpu().view(P, T, K), self.ws[self.nPK:].cpu().view(P, T, N)
        if self.entry == 'adj-dm':
            return self.dM.cpu().view(P, T, K), self.ws.cpu().view(P, T, N)
        return self.ws[self.nPN:].cpu().view(P, T, K), self.ws[:self.nPN].cpu().view(P, T, N)


def _entries(c, cls):
    """adj-own at F(4x4) has one operand set (exact_wino_bf16x3: class 'ones'): it runs with the first class only."""
    return [e for e in XB.ENTRIES if not (e == 'adj-own' and c.tile == 4 and cls != XB.CLASSES[0])]


# ------------------------------------------------------------------------------------------------ 1. the GEMM, bit for bit
@pytest.mark.parametrize("cls", XB.CLASSES)
@pytest.mark.parametrize("c", XB.CASES, ids=lambda c: c.id)
def test_gemm_exact_on_every_class(c, cls):
    G, _lib = _imports()
    for entry in _entries(c, cls):
        run = _Run(G, _lib, c, entry, cls)
        for bm in XB.BMS:
            plan = XB.twin(c.tile, bm)
            what = '%s %s %s bm %d' % (c.id, entry, cls, bm)
            assert _lib.query('ssp_conv_bf16x3_fits', *c.shape, c.K, c.N, 3, plan) == 1
            got = run.launch(plan)
            assert not bool(torch.isnan(got).any()), what
            Vg, Mg = run.planes()
            _eq(Vg, XW.f32(run.V), PLANE, what + ': the transformed operand')
            want = _contract(Vg.double().numpy(), run.U)              # from the V the launch itself left there
            _eq(Mg, XW.f32(want), PLANE, what + ': GEMM output planes')
            assert float(np.abs(want).max()) > 0
            if entry != 'adj-dm':
                assert bool(torch.isnan(run.dM).all()), what + ': dM not given, yet touched'


# ------------------------------------------------------------------------------------------------ 2. against the fp32 twin
def _stats(G, _lib, c, plan):
    n = _lib.query('ssp_conv_stats_floats', *c.shape, c.K, c.N, 3, plan)
    return torch.full((n,), NAN, dtype=torch.float32, device=G.dev())


def _finalized(G, _lib, c, plan, stats):
    B, H, W = c.shape
    tm = _lib.query('ssp_conv_stats_tile_m', B, H, W, c.K, c.N, 3, plan)
    nt = _lib.query('ssp_conv_stats_tiles', B, H, W, c.K, c.N, 3, plan)
    tmp = torch.zeros(8, c.N, dtype=torch.float32, device=G.dev())
    tmp[0].fill_(1.0)
    tmp[3].fill_(1.0)
    _lib.call('ssp_bn_fwd_finalize', stats.data_ptr(), nt, tm, B * H * W, c.N, tmp[0].data_ptr(), tmp[1].data_ptr(),
              tmp[2].data_ptr(), tmp[3].data_ptr(), 0.1, 1e-4, tmp[4].data_ptr(), tmp[5].data_ptr(), tmp[6].data_ptr(),
              tmp[7].data_ptr(), G.stream())
    torch.cuda.synchronize()
    return tmp[4:6].cpu()


@pytest.mark.parametrize("ci", range(len(XB.CASES)), ids=[c.id for c in XB.CASES])
def test_whole_launch_equals_its_fp32_twin(ci):
    """Every entry point on exact operands (one class per case, in turn): plain, accumulating onto a prefill, and with
    another ldout; the forward's BatchNorm statistics (raw partials and finalized vectors); the data gradients' fused
    BatchNorm-backward sums (as many partial rows as groups: plain stores)."""
    G, _lib = _imports()
    c = XB.CASES[ci]
    cls = XB.CLASSES[ci % 3]
    B, H, W = c.shape
    M = B * H * W
    pre = XW.prefill(c.shape + (c.K, c.N), (M, c.N))
    key = c.shape + (c.K, c.N)
    sc, sh, mu, istd = (XW.f32(v).to(G.dev()) for v in XW.bn_vectors(key, c.N))
    raw = XW.nhwc(XW.raw_map(key, B, H, W, c.N), c.N + 8, 4).to(G.dev())
    for entry in XB.ENTRIES:
        run = _Run(G, _lib, c, entry, cls if not (entry == 'adj-own' and c.tile == 4) else XB.CLASSES[0])
        for bm in XB.BMS:
            plan = XB.twin(c.tile, bm)
            f32c = XB.fp32_twin(plan)
            what = '%s %s bm %d' % (c.id, entry, bm)
            for kw in (dict(), dict(accumulate=1, pre=pre), dict(ldout=c.N, outoff=0), dict(ldout=c.N + 64, outoff=32)):
                a = run.launch(f32c, **kw)
                b = run.launch(plan, **kw)
                assert not bool(torch.isnan(a).any())
                _eq(b, a, PIXEL, what + ' %r' % sorted(kw))
            if entry == 'fwd':
                res = []
                for code in (f32c, plan):
                    st = _stats(G, _lib, c, code)
                    out = run.launch(code, stats=st.data_ptr())
                    res.append((out, st.cpu(), _finalized(G, _lib, c, code, st)))
                for x, y, n in zip(res[0], res[1], ('output', 'statistics partials', 'finalized mean / invstd')):
                    assert not bool(torch.isnan(x).any()) and torch.equal(x, y), what + ': ' + n
            else:
                ntile = _lib.query('ssp_conv_stats_tiles', B, H, W, c.K, c.N, 3, plan)
                assert ntile == _lib.query('ssp_conv_stats_tiles', B, H, W, c.K, c.N, 3, f32c)
                res = []
                for code in (f32c, plan):
                    part = torch.full((ntile * c.N * 2,), NAN, dtype=torch.float32, device=G.dev())
                    bnb = (raw.data_ptr() + 16, c.N + 8, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), istd.data_ptr(), 0.125,
                           part.data_ptr(), ntile)
                    res.append((run.launch(code, bnb=bnb), part.cpu()))
                for x, y, n in zip(res[0], res[1], ('dx', 'BatchNorm-backward sums')):
                    assert not bool(torch.isnan(x).any()) and torch.equal(x, y), what + ': ' + n


# ------------------------------------------------------------------------------------------------ 3. misfits
def test_a_twin_code_that_does_not_fit_is_an_error_and_writes_nothing():
    G, _lib = _imports()
    assert len(XB.MISFITS) == 10
    for B, H, W, K, N, R, plan in XB.MISFITS:
        assert _lib.query('ssp_conv_bf16x3_fits', B, H, W, K, N, R, plan) == 0
        M, ldout = B * H * W, (N + 3) // 4 * 4
        T = _lib.query('ssp_conv_wino_tiles', B, H, W, 2)
        ind = torch.ones((M, K), dtype=torch.float32, device=G.dev())
        U = torch.ones((36 * N * K,), dtype=torch.float32, device=G.dev())
        dM = torch.ones((36 * T * K,), dtype=torch.float32, device=G.dev())
        for entry in ('fwd', 'dgrad', 'adj', 'adj-dm'):
            out = torch.full((M, ldout), NAN, dtype=torch.float32, device=G.dev())
            ws = torch.full((36 * T * (K + N),), NAN, dtype=torch.float32, device=G.dev())
            with pytest.raises(_lib.SspError) as e:
                if entry == 'fwd':
                    _lib.call('ssp_conv_fwd', ind.data_ptr(), U.data_ptr(), out.data_ptr(), None, None, B, H, W, K, N, K, ldout, R, 0,
                              plan, ws.data_ptr(), ws.numel(), G.stream())
                elif entry == 'dgrad':
                    _lib.call('ssp_conv_dgrad', ind.data_ptr(), U.data_ptr(), out.data_ptr(), B, H, W, K, N, K, ldout, R, 0, plan,
                              ws.data_ptr(), ws.numel(), G.stream())
                else:
                    _lib.call('ssp_conv_dgrad_adj', ind.data_ptr(), U.data_ptr(), out.data_ptr(), B, H, W, K, N, K, ldout, R, 0, plan,
                              ws.data_ptr(), ws.numel(), dM.data_ptr() if entry == 'adj-dm' else None, G.stream())
            assert str(e.value), (plan, entry)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()), (B, H, W, K, N, R, plan, entry)


# ------------------------------------------------------------------------------------------------ 4. accuracy
# The absolute bar is the one tests/test_gpu_wino.py holds every Winograd launch to, for both tiles.
TOL = 1e-4
# rho: e3 <= RHO * e0, e0 = the fp32 Winograd code of the same tile on the same operands.  Twice the largest e3 / e0 measured
# on the MI355X over the five cases below (twin accuracy table): the factor 2 is for operand seeds.
#   F(2x2)  256 -> 128  0.849     1024 -> 64  0.897
#   F(4x4)  256 -> 128  0.558     1024 -> 64  1.244     64 -> 64  0.781
# (e3 is the same for both tile heights: the K loop of a tile does not depend on its rows)
RHO = 2.0 * 1.244
ACCURACY_CASES = [(2, 256, 128), (2, 1024, 64), (4, 256, 128), (4, 1024, 64), (4, 64, 64)]


@pytest.mark.parametrize("tile,Cin,Cout", ACCURACY_CASES)
def test_accuracy_against_float64_and_the_fp32_winograd_code(tile, Cin, Cout):
    """Uniform(-1, 1) operands, B = 1, 8 x 8, float64 F.conv2d on the CPU: e = max|out - f64| / max|f64| for the twin (e3, the
    worse of its two tile heights) and for its fp32 Winograd code (e0).  (The exact tests above cannot tell the twin from its fp32
    code - both are exact there - so this one also asserts that the outputs differ in some bit.)"""
    G, _lib = _imports()
    B, H, W = 1, 8, 8
    rs = X.rng(23, tile, Cin, Cout)
    x = torch.from_numpy(rs.uniform(-1, 1, (B, Cin, H, W)).astype(np.float32))
    w = torch.from_numpy(rs.uniform(-1, 1, (Cout, Cin, 3, 3)).astype(np.float32))
    ref = F.conv2d(x.double(), w.double(), None, padding=1).numpy()
    xd, wd = G.to_nhwc(x), G.pack_fwd(w)
    U = torch.empty((tile + 2) ** 2 * Cout * Cin, dtype=torch.float32, device=G.dev())
    _lib.call('ssp_wino_filter_transform_t', wd.data_ptr(), U.data_ptr(), Cout, Cin, tile, G.stream())

    def err(plan):
        out = torch.full((B * H * W, Cout), NAN, dtype=torch.float32, device=G.dev())
        n = _lib.query('ssp_conv_workspace_floats', B, H, W, Cin, Cout, 3, plan)
        ws = torch.full((n,), NAN, dtype=torch.float32, device=G.dev())
        _lib.call('ssp_conv_fwd', xd.data_ptr(), U.data_ptr(), out.data_ptr(), None, None, B, H, W, Cin, Cout, Cin, Cout, 3, 0, plan,
                  ws.data_ptr(), n, G.stream())
        torch.cuda.synchronize()
        return rel_err(G.from_nhwc(out, B, Cout, H, W).numpy(), ref), out

    e0, out0 = err(XB.fp32_twin(XB.twin(tile, 128)))
    e3s, outs = zip(*[err(XB.twin(tile, bm)) for bm in XB.BMS])
    e3 = max(e3s)
    # another arithmetic, not an alias of the fp32 code: on random operands the roundings differ somewhere
    assert not any(torch.equal(o, out0) for o in outs)
    print('ACCURACY F(%dx%d) %4d -> %4d  e0 %.3e  e3 %.3e (bm 64 %.3e, bm 128 %.3e)  e3/e0 %.3f'
          % (tile, tile, Cin, Cout, e0, e3, e3s[0], e3s[1], e3 / e0))
    assert e3 <= TOL
    assert e3 <= RHO * e0


# ------------------------------------------------------------------------------------------------ 5. through the engine
_CFG = """[net]
batch=4
height=32
width=32
channels=3
num_keypoints=9

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2
""" + ''.join("""
[convolutional]
batch_normalize=1
filters=%d
size=%d
stride=1
pad=1
activation=leaky
""" % fk for fk in ((64, 3), (128, 3), (128, 3), (64, 1), (128, 3))) + """
[convolutional]
filters=20
size=1
stride=1
pad=1
activation=linear

[region]
anchors =
classes=1
coords=18
num=1
object_scale=5
noobject_scale=0.1
class_scale=1
coord_scale=1
thresh = .6
"""
# layer 0: first block (+ pool 1); 2: 32 -> 64; 3: 64 -> 128; 4: 128 -> 128; 5: 128 -> 64 (1x1); 6: 64 -> 128; 7: the head
WINO_LAYERS = (3, 4, 6)            # 3x3, both sides >= 64 channels: the layers with Winograd candidates
HEAD_BAR, GRAD_BAR = 3.5e-5, 7e-5  # the engine bars of tests/test_gpu_bf16x3.py
STATE = ('_TUNE_CACHE', '_TUNE_FAMILY', '_TUNE_VERIFIED', '_TUNE_VERIFIED_ALSO', 'TUNE_REJECTED', '_HEAD_BUDGET_CACHE',
         '_HEAD_BUDGET_PINNED')


def _scripted_ms(name, args, tuning):
    """The "time" of a launch the tuner times, a fixed function of what was launched: twins < F(4x4) < F(2x2) < bf16x3 direct <
    direct < on-chip; the filter gradient: F(4x4) < F(2x2) < direct < on-chip (so the adjoint rule applies)."""
    if name in ('ssp_conv_fwd', 'ssp_conv_dgrad'):
        code = args[14] if name == 'ssp_conv_fwd' else args[12]
        if tuning.x3_wino(code):
            return 0.1 if (code // 100) % 1000 == 128 else 0.2
        if tuning.wino_fused(code):
            return 2.0
        if tuning.wino_tile(code):
            return 0.5 if tuning.wino_tile(code) == 4 else 0.7
        return 0.9 if tuning.conv_math_of(code) == 'bf16x3' else 1.0
    if name == 'ssp_conv_wgrad_wino_t':
        return {4: 0.5, 2: 0.7}.get(args[10], 2.0)
    return 1.0


@pytest.fixture
def scripted_tuner(monkeypatch):
    """Winograd candidates for 64-channel layers, a clean tune state (restored afterwards), and the scripted clock."""
    from singleshotpose_amd import _lib, engine, tuning
    for k in ('SSP_CONV_MATH', 'SSP_TUNE_CACHE', 'SSP_WINOGRAD', 'SSP_WINO_TILES', 'SSP_WINO_FUSED', 'SSP_DETERMINISTIC',
              'SSP_HEAD_ERR_BUDGET', 'SSP_TUNE_VERIFY'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('SSP_AUTOTUNE', '1')
    monkeypatch.setenv('SSP_WINO_MIN_CHANNELS', '64')
    monkeypatch.setenv('SSP_WINO4_MIN_CHANNELS', '64')
    saved = {n: type(getattr(engine, n))(getattr(engine, n)) for n in STATE}
    cache_file = engine._TUNE_CACHE_FILE[0]
    for n in STATE:
        getattr(engine, n).clear()
    engine._TUNE_CACHE_FILE[0] = None
    last = [None]
    real = _lib.call

    def call(name, *args):
        last[0] = (name, args)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', call)
    monkeypatch.setattr(torch.cuda.Event, 'elapsed_time', lambda e0, e1: _scripted_ms(last[0][0], last[0][1], tuning))
    try:
        yield engine
    finally:
        engine._TUNE_CACHE_FILE[0] = cache_file
        for n in STATE:
            cont = getattr(engine, n)
            cont.clear()
            (cont.extend if isinstance(cont, list) else cont.update)(saved[n])


def _range_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _engine_model(tmp_path):
    from oracle.darknet_ref import seeded_state
    from helpers import load_state_into
    from singleshotpose_amd.darknet import Darknet
    cfg = tmp_path / 'wino_bf16x3.cfg'
    cfg.write_text(_CFG)
    model = Darknet(str(cfg))
    load_state_into(model, model.blocks, seeded_state(model.blocks, 5))
    return model.cuda()


def _step(model, x, gout):
    """One training-mode forward / backward from the same state: (head, {name: grad}, x.grad, plan)."""
    model.train()
    for p in model.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    y = model(xin)
    y.backward(gout)
    torch.cuda.synchronize()
    plan = list(model._plans.values())[-1]
    return (y.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
            xin.grad.detach().clone(), plan)


def _bn_state(model):
    return {n: b.detach().clone() for n, b in model.named_buffers()}


def _restore(model, state):
    with torch.no_grad():
        for n, b in model.named_buffers():
            b.copy_(state[n])


def _codes(plan):
    return {i: (cs.plan_fwd, cs.plan_dgrad) for i, cs in sorted(plan.convs.items())}


def _inputs():
    rs = X.rng(29)
    x = torch.from_numpy(rs.uniform(0, 1, (4, 3, 32, 32)).astype(np.float32)).cuda()
    gout = torch.from_numpy(rs.standard_normal((4, 20, 16, 16)).astype(np.float32)).cuda()
    return x, gout


def test_engine_mode_substitutes_the_winograd_launches(tmp_path, scripted_tuner):
    engine = scripted_tuner
    from singleshotpose_amd import _lib, tuning
    n_rej = len(engine.TUNE_REJECTED)
    model = _engine_model(tmp_path)
    x, gout = _inputs()
    bn0 = _bn_state(model)
    # ---- fp32: where the tuner and the head budget leave every launch
    model.conv_math = 'fp32'
    y0, g0, dx0, plan0 = _step(model, x, gout)
    c0 = _codes(plan0)
    assert all(engine.conv_math_of(c) == 'fp32' for fd in c0.values() for c in fd)
    through = lambda c: bool(engine.wino_tile(c)) and not engine.wino_fused(c)
    assert sum(through(f) for f, _ in c0.values()) >= 1 and sum(through(d) for _, d in c0.values()) >= 1, c0
    assert all(through(c0[i][1]) for i in WINO_LAYERS), c0                 # (the script: Winograd wins where it is timed; the
                                                                           # head budget may still move a FORWARD launch)
    adj0 = {i: cs.dgrad_adj for i, cs in plan0.convs.items()}
    assert any(adj0.values())
    # ---- bf16x3: every Winograd code untouched
    _restore(model, bn0)
    model.conv_math = 'bf16x3'
    y1, g1, dx1, plan1 = _step(model, x, gout)
    c1 = _codes(plan1)
    for i in c0:
        for a, b in zip(c0[i], c1[i]):
            assert (a == b) if engine.wino_tile(a) else not tuning.x3_wino(b), (i, c0[i], c1[i])
    assert not any(k[0].endswith('-bf16x3-wino') for k in engine._TUNE_CACHE)
    # ---- bf16x3-wino
    _restore(model, bn0)
    model.conv_math = 'bf16x3-wino'
    assert not model._plans
    y3, g3, dx3, plan3 = _step(model, x, gout)
    rec = plan3.conv_math
    c3 = _codes(plan3)
    assert rec['mode'] == 'bf16x3-wino'
    n_twin = [0, 0]
    for i, cs in sorted(plan3.convs.items()):
        for d, (a, b) in enumerate(zip(c0[i], c3[i])):
            K, N = (cs.cinp, cs.cout) if d == 0 else (cs.coutp, cs.cin)
            fits = through(a) and bool(_lib.query('ssp_conv_bf16x3_fits', 4, cs.H, cs.W, K, N, cs.k, tuning.x3_wino_twins(a)[0]))
            if fits and i not in rec['taken_back']:
                assert b == tuning.x3_wino_twins(a)[0], (i, d, a, b)      # (the script: the 128-row twin is the fastest)
                n_twin[d] += 1
            elif engine.wino_tile(a):
                assert b == a, (i, d, a, b)
            else:                                                         # direct launches: as in mode 'bf16x3'
                assert b == c1[i][d] or i in rec['taken_back'], (i, d, a, b, c1[i])
    assert n_twin[0] >= 1 and n_twin[1] >= 1, (c0, c3)
    assert {i: cs.dgrad_adj for i, cs in plan3.convs.items()} == adj0
    assert engine.TUNE_REJECTED[n_rej:] == []
    assert any(k[0] == 'fwd-bf16x3-wino' for k in engine._TUNE_CACHE) and any(k[0] == 'dgrad-bf16x3-wino' for k in engine._TUNE_CACHE)
    assert not any(engine.conv_math_of(v) == 'bf16x3' for k, v in engine._TUNE_CACHE.items() if k[0] in ('fwd', 'dgrad'))
    # the record
    assert rec['layers'] == {i: fd for i, fd in c3.items() if 'bf16x3' in map(engine.conv_math_of, fd)}
    assert all(i in rec['layers'] for i in WINO_LAYERS if i not in rec['taken_back'])
    assert 0.0 < rec['head_deviation'] <= HEAD_BAR
    # accuracy against the fp32 step from the same state
    e_head = _range_err(y3, y0)
    e_grads = {n: _range_err(g3[n], g0[n]) for n in g0}
    e_dx = _range_err(dx3, dx0)
    print('ENGINE head %.3e  worst grad %.3e  dx %.3e  record %r' % (e_head, max(e_grads.values()), e_dx, rec))
    assert e_head <= HEAD_BAR
    assert max(e_grads.values()) <= GRAD_BAR, e_grads
    assert e_dx <= GRAD_BAR
    # ---- eval: eager, and replayed from a captured graph
    _restore(model, bn0)
    model.eval()
    with torch.no_grad():
        ye = model(x).clone()
        model.graph_inference = True
        yg = model(x).clone()
        yg2 = model(x).clone()
        model.graph_inference = False
        plan_e = list(model._plans.values())[-1]
        assert sum(tuning.x3_wino(cs.plan_fwd) for cs in plan_e.convs.values()) == n_twin[0]
        assert torch.equal(ye, yg) and torch.equal(yg, yg2)
    # ---- a schedule with frozen layers, and the deterministic mode, with the mode on
    _restore(model, bn0)
    frozen = [p for n, p in model.named_parameters() if n.startswith('models.0.') or n.startswith('models.2.')]
    assert frozen
    for p in frozen:
        p.requires_grad_(False)
    yf, gf, dxf, _ = _step(model, x, gout)
    for p in frozen:
        p.requires_grad_(True)
    assert _range_err(yf, y0) <= HEAD_BAR and gf and all(_range_err(gf[n], g0[n]) <= GRAD_BAR for n in gf)
    _restore(model, bn0)
    model.deterministic = True
    runs = []
    for _ in range(2):
        _restore(model, bn0)
        runs.append(_step(model, x, gout))
    model.deterministic = False
    pd = runs[0][3]
    assert pd.conv_math['mode'] == 'bf16x3-wino' and any(tuning.x3_wino(c) for fd in _codes(pd).values() for c in fd)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(runs[0][1][n], runs[1][1][n]) for n in runs[0][1])
    assert _range_err(runs[0][0], y0) <= HEAD_BAR and all(_range_err(runs[0][1][n], g0[n]) <= GRAD_BAR for n in g0)
    # ---- back to fp32: the training head bit for bit
    _restore(model, bn0)
    model.conv_math = 'fp32'
    y0b, _, _, plan0b = _step(model, x, gout)
    assert torch.equal(y0b, y0)
    assert plan0b.conv_math['layers'] == {} and _codes(plan0b) == c0

"""The stride-2 convolution without a GPU: the int64 references of tests/strided_cases.py against F.conv2d(stride=2) and
its autograd in float64, the parity / tap decomposition of the data gradient restated on the host, and the plan of a net
with downsampling blocks built on the CPU device (planning launches nothing)."""
import pytest
import torch
import torch.nn.functional as F

import exact_conv as E
import strided_cases as S

ids = [S.case_id(c) for c in S.CASES]


ALL = S.CASES + S.PAD_OUT + S.PAD_DGRAD


@pytest.mark.parametrize('c', ALL, ids=[S.case_id(c) for c in ALL])
def test_references_equal_conv2d_and_its_autograd(c):
    B, H, W, Cin, Cout, R = c.shape
    x, dy, w = S.operands(c.shape)
    Ho, Wo = S.out_hw(H, W, R)
    assert dy.shape == (B, Ho, Wo, Cout)
    xt = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wt = w.permute(0, 3, 1, 2).double().requires_grad_(True)
    y = F.conv2d(xt, wt, stride=2, padding=R // 2)
    assert tuple(y.shape) == (B, Cout, Ho, Wo)
    assert torch.equal(S.ref_fwd(x, w).double(), y.detach().permute(0, 2, 3, 1))
    y.backward(dy.permute(0, 3, 1, 2).double())
    assert torch.equal(S.ref_dgrad(dy, w, H, W).double(), xt.grad.permute(0, 2, 3, 1))
    dw = S.ref_wgrad(dy, x, R)
    assert torch.equal(dw[:, :, :Cin].double(), wt.grad.permute(0, 2, 3, 1).reshape(Cout, R * R, Cin))
    assert not dw[:, :, Cin:].any()
    # every partial sum stays an exactly representable integer (the bit-for-bit bar of the GPU tests rests on it)
    assert R * R * Cin * E.XMAX * E.WMAX + E.PREFILL < E.TWO24
    assert R * R * Cout * E.XMAX * E.WMAX + E.PREFILL < E.TWO24
    assert B * Ho * Wo * E.XMAX * E.XMAX < E.TWO24


def test_case_table_covers_what_it_says():
    shapes = [c.shape for c in S.CASES]
    assert (1, 1, 1, 4, 8, 3) in shapes
    assert any(S.out_hw(s[1], s[2], s[5])[0] == 1 and s[1] == 2 for s in shapes)                  # Ho = 1 from H = 2
    assert any(s[1] % 2 == 1 and s[2] % 2 == 0 for s in shapes) and any(s[1] % 2 == 0 and s[2] % 2 == 1 for s in shapes)
    assert any(s[5] == 1 for s in shapes)
    assert any(c.ld and c.off for c in S.CASES)
    assert any(s[0] * S.out_hw(s[1], s[2], s[5])[0] * S.out_hw(s[1], s[2], s[5])[1] > 128 and s[4] > 128 for s in shapes)
    assert any(s[4] % 32 for s in shapes)


def test_padded_case_tables_cover_what_they_say():
    """C % 4 == 2 on the side that is written; the data-gradient table holds tap-split, unsplit and 1x1 launches, each into
    pad4(Cin_dx) columns and into a slice of a wider buffer, and the unsplit shapes are the smallest such."""
    for c in S.PAD_OUT:
        assert c.shape[4] % 4 == 2 and S.buffers(c)[1] == c.shape[4] + 2
    assert sorted(c.shape[5] for c in S.PAD_OUT) == [1, 3]
    kinds = set()
    for c in S.PAD_DGRAD:
        B, H, W, Cin, Cout, R = c.shape
        assert Cin in (6, 18) and c.off % 4 == 0 and c.off + E.pad4(Cin) <= c.lddx
        wgs, split = S.dgrad_workgroups(c.shape)
        kinds.add((R, split, c.lddx == E.pad4(Cin), Cin))
        if R == 3 and not split:
            assert wgs == 512 and S.dgrad_workgroups((B, H - 1, W, Cin, Cout, R))[1]
            assert B * H * W * c.lddx * 4 <= 8 << 20          # a few MB
    for Cin in (6, 18):
        assert set(k[:2] for k in kinds if k[3] == Cin) == {(3, True), (3, False), (1, False)}
    assert set((k[0], k[1], k[2]) for k in kinds) >= {(3, True, True), (3, True, False), (3, False, True), (3, False, False),
                                                      (1, False, True), (1, False, False)}
    assert S.dgrad_workgroups(S.DGRAD_UNSPLIT.shape) == (512, False)
    assert all(S.dgrad_workgroups(c.shape)[1] for c in S.CASES if c.shape[5] == 3)      # (as strided_cases says of them)


PARITY = S.CASES + [S.DGRAD_UNSPLIT] + S.PAD_DGRAD


@pytest.mark.parametrize('c', PARITY, ids=[S.case_id(c) for c in PARITY])
def test_parity_decomposition_reproduces_the_data_gradient(c):
    """Four dense contractions over 1, 2, 2 and 4 taps (3x3) - or one over the single tap (1x1) - give the scatter
    reference on odd and even maps; no class walks a tap that cannot reach it."""
    B, H, W, Cin, Cout, R = c.shape
    x, dy, w = S.operands(c.shape)
    dx, ntaps = S.dgrad_by_parity(dy, w, H, W)
    assert torch.equal(dx, S.ref_dgrad(dy, w, H, W))
    assert ntaps == ({(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 4} if R == 3 else {(0, 0): 1, (0, 1): 0, (1, 0): 0, (1, 1): 0})


def test_tap_table():
    assert S.parity_taps(3, 0) == [(1, 0)] and S.parity_taps(3, 1) == [(0, 1), (2, 0)]
    assert S.parity_taps(1, 0) == [(0, 0)] and S.parity_taps(1, 1) == []
    # yi = 2 * (yh + o) + r - pad for every pair of the table
    for R in (1, 3):
        for parity in (0, 1):
            for r, o in S.parity_taps(R, parity):
                assert 2 * o + r - R // 2 == parity


# ------------------------------------------------------------------------------------------------ the plan
def _no_launch(monkeypatch):
    from singleshotpose_amd import _lib

    def call(name, *args):
        raise AssertionError("planning launched %s" % name)
    monkeypatch.setattr(_lib, 'call', call)


def test_plan_builds_with_strided_blocks(tmp_path, monkeypatch):
    from singleshotpose_amd import engine
    from singleshotpose_amd.cfg import layer_shapes
    from singleshotpose_amd.darknet import Darknet
    monkeypatch.delenv('SSP_BN_FUSE', raising=False)
    _no_launch(monkeypatch)
    model = Darknet(S.write_cfg(tmp_path))
    B, _, H, W = S.NET_INPUT
    plan = engine.Plan(model, B, H, W, torch.device('cpu'))
    plan._plan_bn_fusion()
    shapes = layer_shapes(model.blocks, W, H)
    assert [(w, h, c) for w, h, c in shapes] == [(38, 26, 8), (19, 13, 16), (19, 13, 8), (19, 13, 16), (19, 13, 16), (10, 7, 24),
                                                  (19, 13, 16), (10, 7, 24), (10, 7, 24), (10, 7, 20)]
    for ind, (w, h, c) in enumerate(shapes):
        a = plan.acts[ind]
        assert (a.C, a.H, a.W) == (c, h, w) and a.ld == E.pad4(c), ind
    assert plan.consumers[1] == [2, 4, 6] and plan.consumers[6] == [7] and plan.consumers[5] == [8] and plan.consumers[7] == [8]
    assert plan.acts[6] is plan.acts[1]                       # the route aliases the strided block's output
    assert sorted(i for i, cs in plan.convs.items() if cs.stride == 2) == list(S.NET_STRIDED)
    for ind, cs in plan.convs.items():
        src = plan.acts[ind - 1] if ind else plan.input_act
        assert (cs.Hi, cs.Wi) == (src.H, src.W) and cs.inp is src
        assert (cs.H, cs.W) == (shapes[ind][1], shapes[ind][0]) and cs.M == B * cs.H * cs.W
        assert cs._raw_spec[1] == cs.M * cs.coutp
        if cs.stride == 2:
            assert (cs.H, cs.W) == S.out_hw(cs.Hi, cs.Wi, cs.k)
            assert cs.bn_fuse_src is None                     # never the consumer whose data gradient carries the sums
            assert cs.plan_fwd == 0 and cs.plan_dgrad == 0 and cs.wgrad_wino == 0 and not cs.wino_u and not cs.dgrad_adj
            assert cs.tile_m in (64, 128) and cs.ntile == (cs.M + cs.tile_m - 1) // cs.tile_m
            assert cs.stats.numel() >= cs.ntile * cs.cout * 2
    # a strided block may still be the PRODUCER of a fused pair: layer 7 (linear BN, no activation pass to fold) is not, and
    # layer 5's only consumer is a shortcut
    assert all(cs.bn_fuse_src is None or cs.bn_fuse_src.stride == 1 or cs.stride == 1 for cs in plan.convs.values())


def test_fused_pool_behind_a_strided_block(tmp_path, monkeypatch):
    """A 2x2/2 max-pool directly behind a strided BatchNorm block is fused as behind any other (its even OUTPUT map
    decides); behind an odd output map it is refused as a standalone pool of an odd map is."""
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    _no_launch(monkeypatch)
    net = '[net]\nheight=%d\nwidth=%d\nchannels=3\n\n'
    conv = '[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=3\nstride=%d\npad=1\nactivation=leaky\n\n'
    pool = '[maxpool]\nsize=2\nstride=2\n\n'
    head = '[convolutional]\nfilters=8\nsize=1\nstride=1\npad=1\nactivation=linear\n\n'
    path = S.write_cfg(tmp_path, net % (24, 24) + conv % (8, 1) + conv % (16, 2) + pool + head, 'pool.cfg')
    plan = engine.Plan(Darknet(path), 2, 24, 24, torch.device('cpu'))
    cs = plan.convs[1]
    assert cs.stride == 2 and cs.pool and plan.fused_pool == {2} and (cs.Hi, cs.H, cs.out.H) == (24, 12, 6)
    assert plan.acts[1] is None and (plan.acts[2].H, plan.acts[2].W) == (6, 6)
    path = S.write_cfg(tmp_path, net % (26, 26) + conv % (8, 1) + conv % (16, 2) + pool + head, 'pool_odd.cfg')
    with pytest.raises(NotImplementedError, match=r'block 2 \(maxpool\)'):
        engine.Plan(Darknet(path), 2, 26, 26, torch.device('cpu'))


def test_strided_first_block_is_still_refused(tmp_path, monkeypatch):
    from singleshotpose_amd import engine
    from singleshotpose_amd.darknet import Darknet
    _no_launch(monkeypatch)
    model = Darknet(S.write_cfg(tmp_path, S.first_block_strided_cfg(), 'first.cfg'))
    B, _, H, W = S.NET_INPUT
    with pytest.raises(NotImplementedError, match=r'block 0 \(convolutional\): a stride-2'):
        engine.Plan(model, B, H, W, torch.device('cpu'))
    # other strides stay outside
    with pytest.raises(NotImplementedError, match='stride=3'):
        engine.Plan(Darknet(S.write_cfg(tmp_path, S.NET_CFG.replace('stride=2', 'stride=3', 1), 's3.cfg')), B, H, W,
                    torch.device('cpu'))

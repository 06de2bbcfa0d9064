"""Exact-integer test data of the stride-2 convolution (csrc/conv_strided.hip), shared by tests/test_strided_cpu.py
(the references against F.conv2d, the parity decomposition restated on the host, the plan on the CPU device) and
tests/test_gpu_strided.py (the kernels and the plan on the GPU).

Method: that of tests/exact_conv.py, whose helpers are imported.  x and dy are integers in [-3, 3], filters integers in
[-2, 2]; pad columns are zero and every other column of a wider buffer is NaN.  Every partial sum of a forward, data-
gradient or filter-gradient contraction is then an integer far below 2^24 (CASES' largest: 9 taps * 128 channels * 6 =
6912 forward, 4 * 256 * 6 = 6144 data gradient, 4 * 13 * 13 pixels * 9 + 5 = 6089 filter gradient), so the int64
references must be met bit for bit in any summation order.

Geometry (nn.Conv2d(stride=2, padding=R // 2)): Ho = (H + 2*pad - R) // 2 + 1; input row of output row yo and tap r is
2*yo + r - pad, zero outside the map."""
import collections

import numpy as np
import torch

import exact_conv as E
from exact_data import rng

Case = collections.namedtuple('Case', 'shape ld off')      # ld / off: row stride and channel offset of BOTH maps (None = dense)

# (B, H, W, Cin, Cout, R)
CASES = [
    Case((1, 1, 1, 4, 8, 3), None, 0),           # a single pixel
    Case((1, 2, 2, 4, 4, 3), None, 0),           # Ho = 1; every tap but one block hits a border
    Case((2, 7, 10, 8, 20, 3), None, 0),         # odd H, even W, batch boundary inside a tile, Cout no multiple of 32
    Case((2, 8, 5, 16, 36, 3), None, 0),         # even H, odd W: for odd yi = H-1 the tap r = 0 maps to yo = Ho
    Case((3, 13, 13, 40, 24, 3), None, 0),       # M = 147 crosses a tile, partial last tile; several K chunks
    Case((2, 9, 12, 12, 8, 1), None, 0),         # 1x1 stride 2
    Case((2, 6, 6, 64, 64, 3), 96, 32),          # a channel slice of a wider buffer, read and written
    Case((4, 26, 26, 128, 256, 3), None, 0),     # several tiles in both GEMM dimensions
]

# Data gradient only: 512 workgroups, the smallest launch that keeps one thread per output element (smaller 3x3 launches -
# every case above - split their taps over workgroups and sum with atomics; include/ssp_hip.h, ssp_conv_s2_dgrad)
DGRAD_UNSPLIT = Case((4, 128, 128, 4, 8, 3), None, 0)


# Channel counts with C % 4 == 2, as an 18- or 6-filter block hands them to the plan.  Forward / filter gradient: Cout of
# 18 and 6 into ldout = lddy = pad4(Cout).  Data gradient: Cin_dx of 18 and 6 (the plan passes the unpadded count) into
# lddx = pad4(Cin_dx) and into a slice of a wider buffer; 3x3 on a small grid (taps split over workgroups, atomics), 3x3 on
# the smallest grid that is not split (four classes of 128 tiles of 128 pixels: 4 x 128 x 128, as DGRAD_UNSPLIT), and 1x1
# (the zero fill of the three parity classes without a tap).  Every column of the destination outside its C channels holds
# SENTINEL before the launch and after it.
SENTINEL = 77.0
PAD_OUT = [Case((2, 7, 10, 8, 18, 3), None, 0), Case((2, 8, 5, 12, 6, 1), None, 0)]
DgradPad = collections.namedtuple('DgradPad', 'shape lddx off')
PAD_DGRAD = [
    DgradPad((2, 7, 10, 18, 8, 3), 20, 0), DgradPad((2, 7, 10, 6, 12, 3), 8, 0),
    DgradPad((3, 13, 13, 18, 24, 3), 32, 8), DgradPad((2, 8, 5, 6, 8, 3), 16, 4),
    DgradPad((4, 128, 128, 18, 8, 3), 20, 0), DgradPad((4, 128, 128, 6, 8, 3), 12, 4),
    DgradPad((2, 9, 12, 18, 8, 1), 20, 0), DgradPad((2, 8, 5, 6, 12, 1), 16, 8),
]


def dgrad_workgroups(shape):
    """(workgroups of the unsplit data-gradient launch, whether it is split by taps): include/ssp_hip.h, ssp_conv_s2_dgrad -
    3x3 launches of fewer than 512 workgroups are; tiles of 128 rows, 64 where those would leave CUs of the 256 idle, and
    of 64 (Cin_dx <= 64) or 128 columns."""
    B, H, W, Cin, Cout, R = shape
    Ms = [B * ((H - py + 1) // 2) * ((W - px + 1) // 2) for py in (0, 1) for px in (0, 1) if R == 3 or not (py or px)]
    Ms = [m for m in Ms if m > 0]
    bn = 128 if Cin > 64 else 64
    ncol = (Cin + bn - 1) // bn
    bm = 64 if sum((m + 127) // 128 for m in Ms) * ncol < 256 else 128
    wgs = sum((m + bm - 1) // bm for m in Ms) * ncol
    return wgs, R == 3 and wgs < 512


def case_id(c):
    if isinstance(c, DgradPad):
        return '%dx%dx%d-%dto%d-r%d-ld%d+%d' % (c.shape + (c.lddx, c.off))
    return '%dx%dx%d-%dto%d-r%d%s' % (c.shape + ('-ld%d' % c.ld if c.ld else '',))


def out_hw(H, W, R):
    p = R // 2
    return (H + 2 * p - R) // 2 + 1, (W + 2 * p - R) // 2 + 1


def operands(shape):
    """(x [B,H,W,Cin], dy [B,Ho,Wo,Cout], w [Cout,R,R,Cin]) as int64 tensors, seeded by the shape."""
    B, H, W, Cin, Cout, R = shape
    Ho, Wo = out_hw(H, W, R)
    rs = rng(*(shape + (2,)))
    x = torch.from_numpy(rs.randint(-E.XMAX, E.XMAX + 1, (B, H, W, Cin)).astype(np.int64))
    dy = torch.from_numpy(rs.randint(-E.XMAX, E.XMAX + 1, (B, Ho, Wo, Cout)).astype(np.int64))
    w = torch.from_numpy(rs.randint(-E.WMAX, E.WMAX + 1, (Cout, R, R, Cin)).astype(np.int64))
    return x, dy, w


# ------------------------------------------------------------------------------------------------ int64 references
def ref_fwd(x, w):
    """out[b,yo,xo,co] = sum x[b, 2yo+ky-p, 2xo+kx-p, ci] * w[co,ky,kx,ci]; int64 NHWC [B,Ho,Wo,Cout]."""
    B, H, W, Cin = x.shape
    Cout, R = w.shape[0], w.shape[1]
    Ho, Wo = out_hw(H, W, R)
    xp = E._pad_hw(x, R // 2)
    out = torch.zeros(B * Ho * Wo, Cout, dtype=torch.int64)
    for ky in range(R):
        for kx in range(R):
            out += xp[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :].reshape(-1, Cin) @ w[:, ky, kx, :].t()
    return out.view(B, Ho, Wo, Cout)


def ref_dgrad(dy, w, H, W):
    """dx[b,yi,xi,ci] = sum over (yo, ky) with 2yo+ky-p = yi (and x likewise) of dy[b,yo,xo,co] * w[co,ky,kx,ci]; int64
    [B,H,W,Cin].  A scatter of every (output pixel, tap) pair - nothing of the parity decomposition in it."""
    B, Ho, Wo, Cout = dy.shape
    R, Cin = w.shape[1], w.shape[3]
    p = R // 2
    dxp = torch.zeros(B, H + 2 * p, W + 2 * p, Cin, dtype=torch.int64)
    for ky in range(R):
        for kx in range(R):
            dxp[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :] += (dy.reshape(-1, Cout) @ w[:, ky, kx, :]).view(B, Ho, Wo, Cin)
    return dxp[:, p:p + H, p:p + W, :].contiguous()


def ref_wgrad(dy, x, R):
    """dw[co][ky*R+kx][ci] = sum_{b,yo,xo} dy[b,yo,xo,co] * x[b, 2yo+ky-p, 2xo+kx-p, ci]; int64 [Cout][R*R][Cinp]."""
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    xp = E._pad_hw(x, R // 2)
    dyt = dy.reshape(-1, Cout).t().contiguous()
    dw = torch.zeros(Cout, R * R, E.pad4(Cin), dtype=torch.int64)
    for ky in range(R):
        for kx in range(R):
            dw[:, ky * R + kx, :Cin] = dyt @ xp[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :].reshape(-1, Cin)
    return dw


# ------------------------------------------------------------------------------------------------ parity decomposition
def parity_taps(R, parity):
    """Per dimension: the (tap r, offset o) pairs that reach a destination coordinate yi = 2*yh + parity, from output row
    yo = yh + o.  3x3 pad 1: even -> r = 1; odd -> r = 0 (yo = yh + 1) and r = 2 (yo = yh).  1x1: even -> r = 0, odd -> none."""
    if R == 1:
        return [(0, 0)] if parity == 0 else []
    return [(1, 0)] if parity == 0 else [(0, 1), (2, 0)]


def dgrad_by_parity(dy, w, H, W):
    """The data gradient as the kernel forms it: four dense contractions, one per parity class of the destination pixel,
    each over its own taps only; an output row yh + o == Ho contributes nothing."""
    B, Ho, Wo, Cout = dy.shape
    R, Cin = w.shape[1], w.shape[3]
    dx = torch.zeros(B, H, W, Cin, dtype=torch.int64)
    ntaps = {}
    for py in (0, 1):
        for px in (0, 1):
            Hr, Wr = (H - py + 1) // 2, (W - px + 1) // 2
            ty, tx = parity_taps(R, py), parity_taps(R, px)
            ntaps[(py, px)] = len(ty) * len(tx)
            if Hr <= 0 or Wr <= 0:
                continue
            acc = torch.zeros(B, Hr, Wr, Cin, dtype=torch.int64)
            for ry, oy in ty:
                for rx, ox in tx:
                    src = torch.zeros(B, Hr, Wr, Cout, dtype=torch.int64)
                    hv, wv = min(Hr, Ho - oy), min(Wr, Wo - ox)          # rows / columns whose source exists
                    if hv > 0 and wv > 0:
                        src[:, :hv, :wv] = dy[:, oy:oy + hv, ox:ox + wv]
                    acc += (src.reshape(-1, Cout) @ w[:, ry, rx, :]).view(B, Hr, Wr, Cin)
            dx[:, py::2, px::2, :] = acc
    return dx, ntaps


def buffers(c):
    """(ld of x, ld of dy, channel offset) of a case: dense padded maps, or the case's slice of a wider buffer."""
    B, H, W, Cin, Cout, R = c.shape
    if c.ld:
        return c.ld, c.ld, c.off
    return E.pad4(Cin), E.pad4(Cout), 0


# ------------------------------------------------------------------------------------------------ the residual network
NET_INPUT = (2, 3, 26, 38)
NET_CFG = """
[net]
batch=2
channels=3
height=26
width=38

[convolutional]
batch_normalize=1
filters=8
size=3
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=16
size=3
stride=2
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=8
size=1
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=16
size=3
stride=1
pad=1
activation=leaky

[shortcut]
from=-3
activation=linear

[convolutional]
batch_normalize=1
filters=24
size=3
stride=2
pad=1
activation=leaky

[route]
layers=-5

[convolutional]
batch_normalize=1
filters=24
size=1
stride=2
pad=1
activation=linear

[shortcut]
from=-3
activation=leaky

[convolutional]
filters=20
size=1
stride=1
pad=1
activation=linear
"""
# layer indices of NET_CFG
NET_STRIDED = (1, 5, 7)
NET_HEAD = 9


# The same network in blocks oracle/darknet_ref.forward_ref runs: it has no shortcut block, so act(a + b) is restated as a
# two-layer route followed by a 1x1 convolution whose fixed weight is [I | I] (bias 0) with the shortcut's activation - in
# float64 the same sum plus exact zeros.  Two extra layers shift the indices: ORACLE_INDEX[product layer] = oracle layer.
_CONV = '[convolutional]\nbatch_normalize=%d\nfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n'
ORACLE_CFG = ('[net]\nbatch=2\nchannels=3\nheight=26\nwidth=38\n\n' +
              _CONV % (1, 8, 3, 1, 'leaky') + _CONV % (1, 16, 3, 2, 'leaky') + _CONV % (1, 8, 1, 1, 'leaky') +
              _CONV % (1, 16, 3, 1, 'leaky') + '[route]\nlayers=1,3\n\n' + _CONV % (0, 16, 1, 1, 'linear') +
              _CONV % (1, 24, 3, 2, 'leaky') + '[route]\nlayers=1\n\n' + _CONV % (1, 24, 1, 2, 'linear') +
              '[route]\nlayers=6,8\n\n' + _CONV % (0, 24, 1, 1, 'leaky') + _CONV % (0, 20, 1, 1, 'linear'))
ORACLE_INDEX = {0: 0, 1: 1, 2: 2, 3: 3, 4: 5, 5: 6, 6: 7, 7: 8, 8: 10, 9: 11}
ORACLE_SUMS = {5: 16, 10: 24}          # oracle layer of a restated shortcut -> channels


def oracle_state(state, dtype=torch.float64, requires_grad=False):
    """The product's per-layer state (oracle.darknet_ref.seeded_state of NET_CFG's blocks) as the state of ORACLE_CFG's
    blocks: the conv entries moved to their oracle layers, the [I | I] sums added (never trainable)."""
    out = [None] * (max(ORACLE_INDEX.values()) + 1)
    for ind, e in enumerate(state):
        if e is not None:
            d = {k: v.clone().to(dtype) for k, v in e.items()}
            if requires_grad:
                for k, v in d.items():
                    if not k.startswith('running'):
                        v.requires_grad_(True)
            out[ORACLE_INDEX[ind]] = d
    for ind, c in ORACLE_SUMS.items():
        eye = torch.eye(c, dtype=dtype)
        out[ind] = {'weight': torch.cat([eye, eye], 1).reshape(c, 2 * c, 1, 1), 'bias': torch.zeros(c, dtype=dtype)}
    return out


def write_cfg(tmpdir, text=NET_CFG, name='strided.cfg'):
    import os
    path = os.path.join(str(tmpdir), name)
    with open(path, 'w') as f:
        f.write(text)
    return path


def first_block_strided_cfg():
    """NET_CFG with the first block's stride moved to 2 (still refused: the first block keeps its own kernel family)."""
    return NET_CFG.replace('stride=1', 'stride=2', 1)

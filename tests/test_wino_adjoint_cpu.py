"""The data gradient as the ADJOINT of the Winograd forward map (csrc/conv_wino.hip wino_dgrad_finish_kernel), restated in
numpy on oracle/wino_ref.py and pinned against float64 conv_transpose2d - no GPU.

  forward          Y  = A^T [ sum_ci U[co][ci] . (B^T d B)[ci] ] A          per n x n tile, U = G g G^T
  adjoint          dd = B [ sum_co U[co][ci] . (A dY A^T)[co] ] B^T         per tile: an (n+2) x (n+2) window of dX
                   dX = overlap-add of the windows at the tiles' input origins (n ty - 1, n tx - 1)

It needs the planes the filter gradient transforms dY into (A dY A^T) and the forward filter transform - no B^T dY B and no
flipped filter.  The kernel gathers the overlap-add per output tile; that is cheap only because columns 0 and n+1 of B^T
are unit vectors (a neighbour's edge row depends on one row of its planes), which the last test reads out of the kernel's
own tables."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import wino_ref

SHAPES = [(2, 64, 512, 13, 13), (2, 128, 256, 26, 26), (2, 64, 128, 9, 11)]      # (B, Cin_dx, Cout_dy, H, W)


def adjoint_dgrad(dy, w, tile):
    """dX (B, Cin, H, W) of the 'same' 3x3 cross-correlation with w (Cout, Cin, 3, 3) for dy (B, Cout, H, W)."""
    B, Cout, H, W = dy.shape
    Cin = w.shape[1]
    a = tile + 2
    th, tw = (H + tile - 1) // tile, (W + tile - 1) // tile
    dyp = np.zeros((B, Cout, tile * th, tile * tw), dtype=dy.dtype)
    dyp[:, :, :H, :W] = dy
    tiles = dyp.reshape(B, Cout, th, tile, tw, tile).transpose(0, 2, 4, 1, 3, 5)      # (B, th, tw, Cout, n, n)
    dM = wino_ref.outgrad_transform(tiles, tile)                                      # A dY A^T
    U = wino_ref.filter_transform(w, tile)                                            # (Cout, Cin, a, a)
    dV = np.einsum('btskij,kcij->btscij', dM, U)                                      # (n+2)^2 GEMMs over Cout
    BT, _, _ = wino_ref.matrices(tile)
    dd = wino_ref._apply(BT.T, wino_ref._apply(BT.T, dV, -2), -1)                     # B dV B^T
    dxp = np.zeros((B, Cin, tile * th + 2, tile * tw + 2), dtype=dy.dtype)            # padded by the window's one-pixel rim
    for ty in range(th):
        for tx in range(tw):
            dxp[:, :, tile * ty:tile * ty + a, tile * tx:tile * tx + a] += dd[:, ty, tx]
    return dxp[:, :, 1:H + 1, 1:W + 1]


@pytest.mark.parametrize('tile', [2, 4])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_adjoint_form_is_conv_transpose(shape, tile):
    B, Cin, Cout, H, W = shape
    rng = np.random.RandomState(7 + tile)
    dy = rng.randn(B, Cout, H, W)
    w = rng.randn(Cout, Cin, 3, 3) / np.sqrt(9.0 * Cout)
    ref = F.conv_transpose2d(torch.from_numpy(dy), torch.from_numpy(w), padding=1).numpy()
    got = adjoint_dgrad(dy, w, tile)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= 1e-12, err


def _kernel_bt(tile):
    """The BT initialiser of `template <> struct WinoMat<tile>` in conv_wino.hip, evaluated (as tests/test_oracle_wino.py does)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'singleshotpose_amd', 'csrc', 'conv_wino.hip')
    src = open(path).read()
    body = src[src.index('template <> struct WinoMat<%d>' % tile):]
    body = body[:body.index('\n};')]
    m = re.search(r'static constexpr float BT\[(\d+)\]\[(\d+)\] = (\{.*?\});', body, re.S)
    text = re.sub(r'(\d+\.?\d*)f', r'\1', m.group(3)).replace('{', '[').replace('}', ']')
    arr = np.array(eval(text), dtype=np.float64)      # literals only
    assert arr.shape == (int(m.group(1)), int(m.group(2))) == (tile + 2, tile + 2)
    return arr


@pytest.mark.parametrize('tile', [2, 4])
def test_edge_columns_of_bt_are_unit_vectors(tile):
    """Row 0 / row n+1 of a window dd = B dV B^T are sum_i B^T[i][0 / n+1] (...)[i]: with one non-zero of magnitude 1 in
    each of those columns - in rows 0 and n+1, where the kernel reads them - a neighbour tile's edge costs one row of planes."""
    BT = _kernel_bt(tile)
    assert np.array_equal(BT, wino_ref.matrices(tile)[0])
    for col in (0, tile + 1):
        nz = np.flatnonzero(BT[:, col])
        assert list(nz) == [col], (col, BT[:, col])
        assert abs(BT[col, col]) == 1.0

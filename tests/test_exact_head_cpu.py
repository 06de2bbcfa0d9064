"""Properties of the exact-arithmetic head data (tests/exact_head.py), pinned on the CPU against
oracle/region_loss_ref.py, which follows the reference line by line in float32 torch-CPU.  No GPU.

What tests/test_gpu_head_decisions.py relies on and this file establishes:
  - the float64 statement X.expect takes the reference's decisions: counts, the per-cell confidence-gradient map, the
    coordinate and class gradients equal the oracle's bit for bit (loss_x / loss_y too where the case is exact);
  - a perfect cell has cur == 1.0 and m hits of 9 give float32(m) / float32(9), at the cases' real cell counts;
  - margins.  Every comparison a case does not deliberately tie is separated:
      cur vs thresh        a cell whose cur has an inexact term keeps its decision when that term moves by 1e-3;
      tconf vs 0.5         >= 1e-3 (the cases sit at 0.444 / 0.556: 0.055; the 50-label image: 8.9e-3);
      conf vs 0.25         >= 1e-3 (raw confidences -ln 3 +- 1/64: 2.9e-3), device and host expf may differ by an ulp;
      IoU of the anchors   the best one beats every different one by >= 1e-6 (dyadic anchors: 6/11 vs 9/64 at the least);
      decode confidences   the winner beats every different confidence by >= 1e-3 relative;
    deliberate ties are bit-identical inputs: cur == thresh (float32(m)/9), IoU 6/11 twice, equal logits in the decode;
  - the float32 target statement (product rounded, then subtracted) is what the oracle stores, and a single rounding
    (fused multiply-add) would differ on more than a quarter of the labels of a 13-, 21- or 26-grid: the GPU test can see a contraction."""
import numpy as np
import pytest
import torch

import exact_head as X


def _oracle(name, dtype, thresh):
    from oracle.region_loss_ref import region_loss_ref
    c = X.case(name)
    return region_loss_ref(torch.from_numpy(c.head), torch.from_numpy(c.target(dtype)), X.EPOCH, num_classes=c.nC,
                           num_anchors=c.nA, anchors=c.anchors, multi=c.multi, pretrain_num_epochs=15,
                           **c.settings(thresh))


@pytest.mark.parametrize("run", X.RUNS, ids=X.run_id)
def test_statement_equals_oracle(run):
    name, dtype, thresh = run
    want = X.expected(*run)
    r = _oracle(*run)
    X.check_against(want, r['grad'].numpy(), r, X.run_id(run))
    mg = want['info']['margins']
    assert mg['cur'] > 0 and mg['tconf'] >= X.CONF_MARGIN and mg['prop'] >= X.CONF_MARGIN and mg['iou'] >= 1e-6, mg


def _oracle_cur(c, dtype):
    """cur of every cell by the oracle's own lines (corner_confidences_ref on float32 torch predictions)."""
    from oracle.region_loss_ref import corner_confidences_ref
    o = torch.from_numpy(c.head).view(c.nB, c.nA, -1, c.nH, c.nW)
    gx = torch.linspace(0, c.nW - 1, c.nW).repeat(c.nH, 1)
    gy = torch.linspace(0, c.nH - 1, c.nH).repeat(c.nW, 1).t()
    out = np.zeros((c.nB, c.nA, c.nH, c.nW), dtype=np.float32)
    tgt = c.labels.astype(dtype)
    for b in range(c.nB):
        rows = []
        for k in range(X.K):
            x, y = o[b, :, 2 * k], o[b, :, 2 * k + 1]
            if k == 0:
                x, y = torch.sigmoid(x), torch.sigmoid(y)
            rows += [((x + gx) / c.nW).reshape(-1), ((y + gy) / c.nH).reshape(-1)]
        pred = torch.stack(rows)                                          # (2K, cells)
        cur = torch.zeros(pred.shape[1])
        for t in range(X.MAX_GT):
            if tgt[b, t, 1] == 0:
                break
            g = torch.FloatTensor([float(v) for v in tgt[b, t, 1:1 + 2 * X.K]])
            cur = torch.max(cur, corner_confidences_ref(pred, g.repeat(pred.shape[1], 1).t()))
        out[b] = cur.view(c.nA, c.nH, c.nW).numpy()
    return out


@pytest.mark.parametrize("name,top", [('ladder8', 8), ('ladder16', 8), ('ladder8x2', 9), ('ladder32', 8), ('limit64', 8),
                                      ('multi3', 9), ('multi1', 9), ('overlap', 5)])
def test_hits_give_m_ninths(name, top):
    """In the oracle m exact hits of 9 give exactly float32(m) / float32(9) and a perfect cell 1.0 (the same exp(2) value
    in numerator and normaliser), a miss 160 px away exactly 0, at the real cell counts."""
    c = X.case(name)
    info = X.expected(name, np.float64, 0.6)['info']
    cur = _oracle_cur(c, np.float64)
    ninths = (np.arange(10, dtype=np.float32) / np.float32(9)).astype(np.float32)
    assert ninths[9] == 1.0
    exact = info['exact_cur']
    assert exact.mean() > 0.5
    assert np.array_equal(cur[exact], info['cur'][exact])
    assert np.isin(cur[exact], ninths).all()
    assert np.abs(cur[~exact] - info['cur'][~exact]).max(initial=0) < 1e-6
    own = np.zeros(cur.shape, dtype=bool)
    for key in info['owners']:
        own[key] = True
    seen = set(int(round(float(v) * 9)) for v in cur[exact & ~own])
    want = {0, 5} if name == 'overlap' else set(range(top + 1))     # overlap: max(5, 3), not 8 and not 3
    assert want <= seen and max(seen) == top, seen      # every rung is read at a cell that owns no ground truth


@pytest.mark.parametrize("run", [r for r in X.RUNS if r[2] not in (0.0, 0.6)], ids=X.run_id)
def test_threshold_runs_flip_exactly_the_tied_cells(run):
    """thresh = float32(m)/9 keeps the m-hit cells, its float32 predecessor silences them; nothing else changes."""
    name, dtype, thresh = run
    m = int(round(thresh * 9))
    tie, below = X.expected(name, dtype, X.thresh_tie(m)), X.expected(name, dtype, X.thresh_below(m))
    cur = tie['info']['cur']
    own = np.zeros(cur.shape, dtype=bool)
    for key in tie['info']['owners']:
        own[key] = True
    tied = (cur == np.float32(X.thresh_tie(m))) & ~own
    assert tied.sum() >= 1
    c = X.case(name)
    conf_t = tie['exact']['grad'].reshape(c.nB, c.nA, -1, c.nH, c.nW)[:, :, 2 * X.K]
    conf_b = below['exact']['grad'].reshape(c.nB, c.nA, -1, c.nH, c.nW)[:, :, 2 * X.K]
    assert np.all(conf_t[tied] == 0.5) and np.all(conf_b[tied] == 0.0)
    assert np.array_equal(conf_t[~tied], conf_b[~tied])
    free = ~own
    assert set(np.unique(conf_t[free]).tolist()) <= {0.0, 0.5}


@pytest.mark.parametrize("grid", [13, 21, 26])
def test_target_statement_is_what_the_oracle_stores(grid):
    """tx = target * nW - gi0 in the label's dtype, stored into a float32 tensor (region_loss.py, restated by the oracle's
    lines `gx[i] - gi0`): equal to X.target_xy; and the single-rounding value differs on more than a quarter of the float32
    labels (all key points are taken relative to the centroid's cell)."""
    rs = np.random.RandomState(grid)
    lab = rs.uniform(0.02, 0.98, (2000, X.NL))
    for dtype in (np.float32, np.float64):
        differ = n = 0
        for row in lab.astype(dtype)[:200]:
            t = torch.from_numpy(row)
            gi0, gj0 = int(t[1] * grid), int(t[2] * grid)
            store = torch.zeros(2 * X.K)
            for i in range(X.K):
                store[2 * i] = t[2 * i + 1] * grid - gi0
                store[2 * i + 1] = t[2 * i + 2] * grid - gj0
            tx, ty = X.target_xy(row, grid, grid, gi0, gj0)
            assert np.array_equal(store.numpy()[0::2], tx) and np.array_equal(store.numpy()[1::2], ty)
            fused = (row[1:19:2].astype(np.float64) * grid - gi0).astype(np.float32)     # exact product, one rounding
            differ += int((fused != tx).sum())
            n += X.K
        if dtype == np.float32:
            assert differ > n // 4, (differ, n)


def test_boundary_cells_follow_the_label_dtype():
    """15/26 * 26 floors to 14 in float64 (tx rounds to 1.0) and to 15 in float32 (tx == 0); k / nW and the largest float32
    below 1 land in the cell the oracle picks (the gradients of test_statement_equals_oracle sit at those cells)."""
    o64 = X.expected('grid26', np.float64, 0.6)['info']['owners']
    o32 = X.expected('grid26', np.float32, 0.6)['info']['owners']
    assert set(o64) == {(0, 0, 14, 14), (0, 0, 14, 7)} and set(o32) == {(0, 0, 15, 15), (0, 0, 15, 7)}
    assert o64[(0, 0, 14, 14)][1][0] == 1.0 and o32[(0, 0, 15, 15)][1][0] == 0.0
    for grid in (8, 16):
        own = X.expected('boundary%d' % grid, np.float32, 0.6)['info']['owners']
        assert set(own) == {(0, 0, 2, 3), (0, 0, grid - 1, grid // 2), (0, 0, grid // 2, 5), (1, 0, grid - 1, grid - 1),
                            (1, 0, 0, grid - 1)}


def test_case_shapes():
    """The branches the cases exist for are really taken."""
    own = X.expected('ownership', np.float64, 0.6)
    assert own['exact']['nGT'] == 2 + 1 + 50 + 0
    assert sum(1 for k in own['info']['owners'] if k[0] == 0) == 1             # two labels, one cell
    assert own['info']['owners'][(0, 0, 3, 2)][0] == 1                          # the later one has it
    m3 = X.expected('multi3', np.float64, 0.6)['info']['owners']
    assert sorted(k[1] for k in m3 if k[0] == 0) == [1, 3, 4]                   # tie -> first, 8x8 box, zero box -> last
    cnt = X.expected('counts', np.float64, 0.6)['exact']
    assert (cnt['nGT'], cnt['nCorrect'], cnt['nProposals']) == (5, 3, 10)


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("nH,nW,nA", [(8, 8, 1), (8, 8, 5), (32, 32, 1)])
@pytest.mark.parametrize("only_objectness", [1, 0])
def test_decode_statement(nH, nW, nA, only_objectness):
    from oracle.region_loss_ref import get_region_boxes_ref
    dc = X.decode_case(nH, nW, nA)
    exp = X.decode_expect(dc, only_objectness)
    assert exp[-1] is None and all(e is not None for e in exp[:-1])
    assert all(e['margin'] >= X.CONF_MARGIN for e in exp[:-1])
    assert all(exp[n]['ties'] >= 2 for n in (0, 1, 2))
    assert exp[4]['key'] == (12 if only_objectness else 45) and exp[4]['cls_id'] == (0 if only_objectness else 1)
    assert exp[3]['key'] == (21 if only_objectness else 33)
    assert all(e['cls_conf'] in (1.0, 0.5, 0.25) for e in exp[:-1])
    if nA == 1:
        for n, e in enumerate(exp[:-1]):
            box = get_region_boxes_ref(torch.from_numpy(dc.head[n:n + 1]), 4, X.K, only_objectness)
            assert np.array_equal(np.array(box[:2 * X.K], dtype=np.float32), e['coords'])
            assert abs(box[2 * X.K] - e['det']) < 1e-6 and box[2 * X.K + 1] == e['cls_conf'] and box[2 * X.K + 2] == e['cls_id']

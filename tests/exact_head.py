"""Exact-arithmetic heads and labels for the RegionLoss / decode kernels (singleshotpose_amd/csrc/region.hip), in the
style of tests/exact_data.py.  CPU only: numpy, no GPU import.  The properties claimed here are pinned against
oracle/region_loss_ref.py by tests/test_exact_head_cpu.py; tests/test_gpu_head_decisions.py runs the kernels on them.

Why the data is exact.  On a power-of-two grid (8, 16, 32, 64):
  - key points k >= 1 decode as (raw + i) / nW: raw values on the grid 1/8 give exactly representable predictions;
  - key point 0 goes through the sigmoid: raw = 0 gives 1 / (1 + expf(-0)) = 1 / (1 + 1) = 0.5.  This rests on
    expf(-0) == 1 exactly (true of every exp: the argument reduction leaves 2^0), so the centroid of a cell is predicted
    at the cell's centre;
  - ground-truth coordinates sit on (i + q/8) / nW;
  - the raw confidence is 0 wherever a decision is read: conf == 0.5;
  - noobject_scale = 4 and object_scale = 16 have the exact square roots 2 and 4.
A key point that hits its ground truth has d == 0 and contributes (exp(2) - 1) / (exp(2) - 1) == 1; one that misses sits
exactly 160 px away in x (0.25 of the image width) or further, is masked by d < 80 and contributes exactly 0 - without
the mask it would contribute exp(-2) - 1 = -0.865.  So a cell whose centre is also 0 or >= 80 px from the centroid has
cur == float32(m) / float32(9) for m hits, and the gradient on the confidence channel of a cell that owns no ground
truth is bitwise 0.5 (kept: (0.5 * 2 - 0) * 2 * 0.25) or 0.0 (silenced by cur > thresh): the readable map of that
decision.  At cells that own a ground truth the coordinate gradients are coord_scale * (p - t), times 0.25 for key point
0: exact dyadic numbers, and loss_x / loss_y are short sums of exact dyadic terms.

The expectation (`expect`) is a plain float64 / numpy statement of build_targets that takes its OWN decisions.  Three
float32 roundings are part of what is being specified and are stated as such: the ground-truth corners are cast to
float32 (torch.FloatTensor(gt)), cur of an exact cell is float32(m) / float32(9), and the targets are
tx = fl(fl(g * nW) - gi0) in the label's dtype (a rounded product, then a subtraction), then cast to float32.
"""
import functools

import numpy as np

from helpers import rel_err

TOL = 1e-4                       # the relative bar of tests/test_gpu_head.py, for everything that is not exact
K = 9
NL = 2 * K + 3
MAX_GT = 50
NOOBJECT_SCALE, OBJECT_SCALE = 4.0, 16.0
EPOCH = 20                       # > pretrain_num_epochs = 15: the confidence term is on
MISS = 0.25                      # a miss sits 0.25 of the image width = 160 px away in x
CONF_MARGIN = 1e-3               # every undeliberate comparison of a confidence is at least this far from its threshold
ANCHORS = [1.0, 1.0, 2.0, 4.0, 4.0, 2.0, 8.0, 8.0, 0.5, 0.5]      # dyadic; (2,4) and (4,2) tie against a 3 x 3 box
LN3 = float(np.float32(np.log(3.0)))


def thresh_tie(m):
    """float32(m) / float32(9): cur of a cell with m exact hits.  cur > thresh is false on the tie: the cell is kept."""
    return float(np.float32(m) / np.float32(9))


def thresh_below(m):
    """The float32 predecessor of thresh_tie(m): the same cell is silenced."""
    return float(np.nextafter(np.float32(m) / np.float32(9), np.float32(-1)))


class Head(object):
    """One case: head (nB, nA*(2K+1+nC), nH, nW) float32, labels (nB, 50, 21) float64, module settings."""

    def __init__(self, name, nB, nH, nW, nA=1, nC=1, multi=False, coord_scale=1.0, class_scale=1.0, exact_loss=True):
        self.name, self.nB, self.nH, self.nW, self.nA, self.nC, self.multi = name, nB, nH, nW, nA, nC, multi
        self.coord_scale, self.class_scale, self.exact_loss = coord_scale, class_scale, exact_loss
        self.anchors = list(ANCHORS) if multi else []
        self.raw = np.zeros((nB, nA, 2 * K + 1 + nC, nH, nW), dtype=np.float64)
        self.raw[:, :, 2:2 * K:2] = 2.0 * nW          # default: key points k >= 1 predicted two image widths away
        self.labels = np.zeros((nB, MAX_GT, NL), dtype=np.float64)
        self.ngt = [0] * nB
        self.reserved = set()

    # -------------------------------------------------------------------------------------------- building blocks
    def star(self, cell, q0=(4, 4), spread=6, turn=0):
        """(9, 2) normalised points: centroid at (i + q0/8) / nW and 8 key points within +-spread/8 of a cell around it."""
        i, j = cell
        pts = np.empty((K, 2))
        pts[0] = ((i + q0[0] / 8.0) / self.nW, (j + q0[1] / 8.0) / self.nH)
        for k in range(1, K):
            ox = ((k * 5 + turn) % (2 * spread + 1)) - spread
            oy = ((k * 3 + 2 * turn) % (2 * spread + 1)) - spread
            pts[k] = ((i + (4 + ox) / 8.0) / self.nW, (j + (4 + oy) / 8.0) / self.nH)
        return pts

    def add_gt(self, b, pts, cls=0, box=(0.25, 0.25)):
        t = self.ngt[b]
        self.labels[b, t, 0] = cls
        self.labels[b, t, 1:1 + 2 * K] = np.asarray(pts, dtype=np.float64).reshape(-1)
        self.labels[b, t, 1 + 2 * K:] = box
        self.ngt[b] = t + 1
        return t

    def aim(self, b, a, cell, pts, hits, reserve=True):
        """Cell (i, j) of anchor a predicts key point k exactly at pts[k] for k in hits and 160 px to its right otherwise
        (k >= 1; key point 0 always decodes to the cell's centre)."""
        i, j = cell
        for k in range(1, K):
            x = pts[k][0] + (0.0 if k in hits else MISS)
            self.raw[b, a, 2 * k, j, i] = x * self.nW - i
            self.raw[b, a, 2 * k + 1, j, i] = pts[k][1] * self.nH - j
        if reserve:
            self.reserved.add((b, a, j, i))

    def ladder(self, b, pts):
        """Every free cell whose centre is 0 or >= 80 px from pts[0] aims at pts with m' = (c + c // 256) % 9 hits among
        the key points 1..8, c = (a * nH + j) * nW + i the cell's index in the loss kernel (one thread handles c, c + 256,
        ...: the cells of one thread get different m), the subset rotating with c."""
        for a in range(self.nA):
            for j in range(self.nH):
                for i in range(self.nW):
                    if (b, a, j, i) in self.reserved:
                        continue
                    dx = ((i + 0.5) / self.nW - pts[0][0]) * 640
                    dy = ((j + 0.5) / self.nH - pts[0][1]) * 480
                    d0 = np.hypot(dx, dy)
                    if d0 != 0 and d0 < 80:
                        continue
                    c = (a * self.nH + j) * self.nW + i
                    m = (c + c // 256) % 9
                    self.aim(b, a, (i, j), pts, set(((c + r) % 8) + 1 for r in range(m)), reserve=False)

    # -------------------------------------------------------------------------------------------- what the tests use
    @property
    def head(self):
        return self.raw.astype(np.float32).reshape(self.nB, -1, self.nH, self.nW)

    def target(self, dtype):
        return self.labels.astype(dtype).reshape(self.nB, -1)

    def settings(self, thresh=0.6):
        return dict(coord_scale=self.coord_scale, noobject_scale=NOOBJECT_SCALE, object_scale=OBJECT_SCALE,
                    class_scale=self.class_scale, thresh=thresh)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _iou_centred(aw, ah, gw, gh):
    inter = min(aw, gw) * min(ah, gh)
    return inter / (aw * ah + gw * gh - inter) if inter > 0 else 0.0


def target_xy(g, nW, nH, gi0, gj0):
    """The targets of one label row g (its own dtype T): fl_T(fl_T(g * nW) - gi0), cast to float32.  Two roundings, as the
    reference's `target * nW - gi0`; a fused multiply-add would round once."""
    T = g.dtype.type
    tx = (g[1:1 + 2 * K:2] * T(nW)) - T(gi0)
    ty = (g[2:2 + 2 * K:2] * T(nH)) - T(gj0)
    assert tx.dtype == g.dtype
    return tx.astype(np.float32), ty.astype(np.float32)


def expect(case, dtype, thresh=0.6):
    """float64 / numpy statement of RegionLoss on `case` with labels of `dtype`.  Returns a dict:
      exact:   grad (float32, head-shaped), mask (bool, head-shaped: where grad is compared bit for bit), nGT, nCorrect,
               nProposals, loss_x, loss_y (the two losses only when case.exact_loss)
      approx:  grad (float64, head-shaped, everything), loss_x, loss_y, loss_conf, loss_cls, loss
      info:    owners {(b, a, j, i): t}, cur (float32 per cell), exact_cur (bool per cell), margins"""
    nB, nA, nC, nH, nW = case.nB, case.nA, case.nC, case.nH, case.nW
    labels = case.labels.astype(dtype)
    raw = case.head.astype(np.float64).reshape(nB, nA, 2 * K + 1 + nC, nH, nW)
    th32 = np.float32(thresh)
    px, py = raw[:, :, 0:2 * K:2].copy(), raw[:, :, 1:2 * K:2].copy()          # (nB, nA, K, nH, nW)
    px[:, :, 0], py[:, :, 0] = _sig(px[:, :, 0]), _sig(py[:, :, 0])
    predx = (px + np.arange(nW)[None, None, None, None, :]) / nW
    predy = (py + np.arange(nH)[None, None, None, :, None]) / nH
    conf = _sig(raw[:, :, 2 * K])
    e2 = np.exp(2.0) - 1.0

    def conf_terms(gx, gy, qx, qy, norm):
        d = np.sqrt(((gx - qx) * 640) ** 2 + ((gy - qy) * 480) ** 2)
        return d, np.where(d < 80, (np.exp(2 * (1 - d / 80)) - 1) / norm, 0.0)

    grad = np.zeros_like(raw)
    mask = np.ones(raw.shape, dtype=bool)
    cur_all = np.zeros((nB, nA, nH, nW), dtype=np.float32)
    exact_cur = np.ones((nB, nA, nH, nW), dtype=bool)
    owners = {}
    tconf = np.zeros((nB, nA, nH, nW))
    margins = dict(cur=np.inf, tconf=np.inf, prop=float(np.abs(conf - 0.25).min()), iou=np.inf)
    loss_conf = 0.0
    nGT = nCorrect = 0
    loss_x = loss_y = loss_cls = 0.0
    for b in range(nB):
        stop = np.nonzero(labels[b, :, 1] == 0)[0]
        ngt = int(stop[0]) if len(stop) else MAX_GT                     # the list ends at the first x0 == 0
        nGT += ngt
        g32 = labels[b, :ngt, 1:1 + 2 * K].astype(np.float32).astype(np.float64)
        hi = np.zeros((nA, nH, nW))
        lo = np.zeros((nA, nH, nW))
        for t in range(ngt):
            gx, gy = g32[t, 0::2][None, :, None, None], g32[t, 1::2][None, :, None, None]
            d, c = conf_terms(gx, gy, predx[b], predy[b], e2)                      # (nA, K, nH, nW)
            ex = np.all((d == 0) | (d >= 80), axis=1)
            m = (d == 0).sum(axis=1)
            c32 = np.where(ex, np.float32(m.astype(np.float32) / np.float32(K)), c.mean(axis=1).astype(np.float32))
            cur_all[b] = np.maximum(cur_all[b], c32)
            hi = np.maximum(hi, np.where(ex, c32, c32 + CONF_MARGIN))
            lo = np.maximum(lo, np.where(ex, c32, c32 - CONF_MARGIN))
            exact_cur[b] &= ex
        silenced = cur_all[b] > th32
        for t in range(ngt):
            g = labels[b, t]
            T = g.dtype.type
            gi0, gj0 = int(g[1] * T(nW)), int(g[2] * T(nH))
            assert 0 <= gi0 < nW and 0 <= gj0 < nH, "centroid outside the grid: the reference raises"
            tx, ty = target_xy(g, nW, nH, gi0, gj0)
            best_n, pb, pa = 0, b, 0
            if case.multi:
                gw, gh = float(g[NL - 2]) * nW, float(g[NL - 1]) * nH
                ious = [_iou_centred(case.anchors[2 * n], case.anchors[2 * n + 1], gw, gh) for n in range(nA)]
                best = max(ious)
                best_n = ious.index(best) if best > 0 else nA - 1              # first maximum; all zero: anchor "-1"
                for v in ious:
                    if v != best:
                        margins['iou'] = min(margins['iou'], best - v)
                pb, pa = (b - 1) % nB, nA - 1                                  # the last anchor of the previous image
            _, c = conf_terms(g32[t, 0::2], g32[t, 1::2], predx[pb, pa, :, gj0, gi0], predy[pb, pa, :, gj0, gi0], e2 + 1e-5)
            tc = float(c.mean())
            margins['tconf'] = min(margins['tconf'], abs(tc - 0.5))
            nCorrect += 1 if tc > 0.5 else 0
            owners[(b, best_n, gj0, gi0)] = (t, tx, ty, tc, int(g[0]))          # a later ground truth takes the cell
        cmask = np.where(silenced, 0.0, NOOBJECT_SCALE)
        for (bb, a, j, i), (t, tx, ty, tc, cls) in owners.items():
            if bb != b:
                continue
            cmask[a, j, i] = OBJECT_SCALE
            tconf[b, a, j, i] = tc
            p_x, p_y = px[b, a, :, j, i], py[b, a, :, j, i]
            ex_ = (p_x.astype(np.float32) - tx).astype(np.float64)              # fl32(p - t): one float32 subtraction
            ey_ = (p_y.astype(np.float32) - ty).astype(np.float64)
            gx_, gy_ = case.coord_scale * ex_, case.coord_scale * ey_
            gx_[0] *= p_x[0] * (1 - p_x[0])
            gy_[0] *= p_y[0] * (1 - p_y[0])
            grad[b, a, 0:2 * K:2, j, i], grad[b, a, 1:2 * K:2, j, i] = gx_, gy_
            loss_x += float((case.coord_scale * ex_ ** 2 / 2).sum())
            loss_y += float((case.coord_scale * ey_ ** 2 / 2).sum())
            if case.multi:
                z = raw[b, a, 2 * K + 1:, j, i]
                p = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
                grad[b, a, 2 * K + 1:, j, i] = case.class_scale * (p - (np.arange(nC) == cls))
                loss_cls += float(case.class_scale * -np.log(p[cls]))
        grad[b, :, 2 * K] = (conf[b] - tconf[b]) * cmask * conf[b] * (1 - conf[b])
        own = np.zeros((nA, nH, nW), dtype=bool)
        for (bb, a, j, i) in owners:
            if bb == b:
                own[a, j, i] = True
        mask[b, :, 2 * K] = ~own & (raw[b, :, 2 * K] == 0)
        loss_conf += float((cmask * (conf[b] - tconf[b]) ** 2 / 2).sum())
        # a cell that owns no ground truth and whose decision would change if its inexact terms moved by CONF_MARGIN
        # has no margin (d < 80 itself needs none: the term it masks goes to 0 continuously at d = 80)
        if np.any(((hi > th32) != (lo > th32)) & ~own):
            margins['cur'] = 0.0
    shape = (nB, -1, nH, nW)
    exact = dict(grad=grad.astype(np.float32).reshape(shape), mask=mask.reshape(shape), nGT=nGT, nCorrect=nCorrect,
                 nProposals=int((conf > 0.25).sum()))
    if case.exact_loss:
        exact.update(loss_x=loss_x, loss_y=loss_y)
    approx = dict(grad=grad.reshape(shape), loss_x=loss_x, loss_y=loss_y, loss_conf=loss_conf, loss_cls=loss_cls,
                  loss=loss_x + loss_y + loss_conf + (loss_cls if case.multi else 0.0))
    return dict(exact=exact, approx=approx,
                info=dict(owners=owners, cur=cur_all, exact_cur=exact_cur, margins=margins))


def check_against(want, got_grad, got, what):
    """The comparison both test files make: the exact part with ==, everything within the suite's relative bar TOL.  got: dict with nGT, nCorrect, nProposals, loss_x, loss_y, loss_conf, loss_cls,
    loss; got_grad: float32 array shaped like the head."""
    ex, ap = want['exact'], want['approx']
    assert not np.isnan(got_grad).any(), what
    assert (got['nGT'], got['nCorrect'], got['nProposals']) == (ex['nGT'], ex['nCorrect'], ex['nProposals']), what
    m = ex['mask']
    bad = (got_grad != ex['grad']) & m
    assert not bad.any(), '%s: %d gradient elements differ, first at %s' % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert rel_err(got_grad, ap['grad']) < TOL, what
    for k in ('loss_x', 'loss_y'):
        if k in ex:
            assert got[k] == ex[k], (what, k, got[k], ex[k])
    for k in ('loss_x', 'loss_y', 'loss_conf', 'loss_cls', 'loss'):
        assert abs(got[k] - ap[k]) <= TOL * abs(ap[k]), (what, k, got[k], ap[k])


# ------------------------------------------------------------------------------------------------ the loss cases
def _ladder_case(name, nB, nH, nW, nA, gt_cells):
    h = Head(name, nB, nH, nW, nA=nA)
    for b in range(nB):
        cell = gt_cells[b % len(gt_cells)]
        pts = h.star(cell, turn=b)
        h.add_gt(b, pts)
        h.aim(b, 0, cell, pts, {1, 2, 3, 4})            # the cell that owns the ground truth: 5 of 9 with the centroid
        if nA > 1:                                      # the same cell of the last anchor owns nothing: the 9-of-9 rung,
            h.aim(b, nA - 1, cell, pts, set(range(1, K)))       # which one anchor cannot have (key point 0 hits only there)
        h.ladder(b, pts)
    return h


def _overlap_case():
    """(b) one cell hits ground truth 0 with 5 key points and ground truth 1 with 3 others: cur = max = 5/9, not the sum
    8/9 and not the last 3/9.  A second cell does it the other way round (3 then 5)."""
    h = Head('overlap', 1, 8, 8)
    A, B = h.star((1, 1)), h.star((5, 5), turn=3)
    h.add_gt(0, A)
    h.add_gt(0, B)
    h.aim(0, 0, (1, 1), A, {1})
    h.aim(0, 0, (5, 5), B, {2})
    for cell, five, three in (((3, 3), A, B), ((6, 2), B, A)):
        i, j = cell
        for k in range(1, K):
            src = five if k <= 5 else three
            h.raw[0, 0, 2 * k, j, i] = src[k][0] * 8 - i
            h.raw[0, 0, 2 * k + 1, j, i] = src[k][1] * 8 - j
    return h


def _ownership_case():
    """(c) image 0: two ground truths in one cell, the later one owns it (targets and tconf) while both count; image 1:
    the list ends at the first x0 == 0 row although later rows are filled; image 2: 50 ground truths; image 3: none."""
    h = Head('ownership', 4, 8, 8, coord_scale=2.0)
    first = h.star((2, 3))
    later = first.copy()
    later[5:, 0] -= MISS                                     # the later one shares the centroid and 4 key points
    h.add_gt(0, first)
    h.add_gt(0, later)
    h.aim(0, 0, (2, 3), first, {1, 2, 3, 4, 5, 6, 7, 8})     # tconf ~ 1 for the first, ~ 5/9 for the later: both correct
    h.ladder(0, first)
    one = h.star((5, 2))
    h.add_gt(1, one)
    h.aim(1, 0, (5, 2), one, {1, 2})
    ghost = h.star((1, 6), turn=2)
    h.labels[1, 1, 0:1] = 0
    h.labels[1, 1, 1:] = np.concatenate([ghost.reshape(-1), [0.25, 0.25]])
    h.labels[1, 1, 1] = 0.0                                  # x0 == 0 ends the list ...
    for t in (2, 3):                                         # ... whatever follows
        h.labels[1, t, 1:] = np.concatenate([ghost.reshape(-1), [0.25, 0.25]])
    h.ladder(1, ghost)                                       # cells that would be silenced if the ghost rows counted
    rs = np.random.RandomState(50)
    for t in range(MAX_GT):
        cell = (t % 8, t // 8)
        pts = h.star(cell, q0=(int(rs.randint(1, 8)), int(rs.randint(0, 8))), turn=t)
        h.add_gt(2, pts)
        h.aim(2, 0, cell, pts, set(int(k) for k in rs.choice(np.arange(1, K), rs.randint(0, 9), replace=False)))
    return h


def _boundary_case(grid):
    """(d) centroids exactly on k / nW and at the largest float32 below 1."""
    h = Head('boundary%d' % grid, 2, grid, grid, exact_loss=False)
    for n, (cell, q0) in enumerate((((3, 2), (0, 0)), ((grid // 2, grid - 1), (0, 4)), ((5, grid // 2), (4, 0)))):
        pts = h.star(cell, q0=q0, turn=n)
        h.add_gt(0, pts)
        h.aim(0, 0, cell, pts, {n + 1})
    last = float(np.nextafter(np.float32(1), np.float32(0)))
    pts = h.star((grid - 1, grid - 1))
    pts[0] = (last, last)
    h.add_gt(1, pts)
    h.aim(1, 0, (grid - 1, grid - 1), pts, {1, 2})
    pts = h.star((grid - 1, 0), q0=(4, 0))
    pts[0] = (last, 0.5 / grid)
    h.add_gt(1, pts)
    h.aim(1, 0, (grid - 1, 0), pts, {3})
    return h


def _grid26_case():
    """(d) 15/26 on a 26-grid: float64 15/26*26 floors to 14 (tx rounds to 1.0), float32 gives 15.0 (cell 15, tx 0)."""
    h = Head('grid26', 1, 26, 26, exact_loss=False)
    h.raw[:, :, 2:2 * K] = 0.0
    pts = np.full((K, 2), 15.0 / 26.0)
    pts[1:, 0] = (np.arange(1, K) + 0.375) / 26.0
    pts[1:, 1] = 7.0 / 26.0
    h.add_gt(0, pts)
    pts = pts.copy()
    pts[0] = (7.0 / 26.0, 15.0 / 26.0)
    h.add_gt(0, pts)
    rs = np.random.RandomState(26)
    h.raw[0, 0, 2:2 * K, 13:17, :] = rs.randint(-8, 9, (2 * K - 2, 4, 26)) / 8.0
    h.raw[0, 0, 2:2 * K, :, 13:17] = rs.randint(-8, 9, (2 * K - 2, 26, 4)) / 8.0
    return h


def _rounding_case(grid):
    """(e) uniform labels on a grid that is no power of two: the targets carry float32 (or float64) roundings."""
    h = Head('rounding%d' % grid, 3, grid, grid, coord_scale=1.0, exact_loss=False)
    rs = np.random.RandomState(grid)
    h.raw[:, :, 2:2 * K] = rs.randint(-8, 9, (3, 1, 2 * K - 2, grid, grid)) / 8.0
    for b in range(3):
        for t in range(8):
            pts = rs.uniform(0.05, 0.95, (K, 2))
            h.add_gt(b, pts, box=tuple(rs.uniform(0.1, 0.4, 2)))
    return h


def _counts_case():
    """(f) nProposals: raw confidences CONF_STEP on either side of -ln 3 (sigmoid 0.25 +- 2.9e-3); nCorrect: 4 and 5 hits
    of 9 at the cells that own a ground truth (tconf ~ 0.444 and ~ 0.556)."""
    h = Head('counts', 2, 8, 8)
    h.raw[:, :, 2 * K] = -3.0
    step = 1.0 / 64
    above = [(0, 1, 2), (0, 7, 7), (1, 0, 0), (1, 3, 4), (1, 6, 1)]
    below = [(0, 2, 2), (0, 0, 7), (0, 5, 5), (1, 4, 4)]
    for b, j, i in above:
        h.raw[b, 0, 2 * K, j, i] = -LN3 + step
    for b, j, i in below:
        h.raw[b, 0, 2 * K, j, i] = -LN3 - step
    for b, cells in enumerate((((1, 1), (6, 3)), ((2, 5), (5, 1), (4, 6)))):
        for n, cell in enumerate(cells):
            pts = h.star(cell, turn=n + b)
            h.add_gt(b, pts)
            h.aim(b, 0, cell, pts, set(range(1, 4 + (n + b) % 2)))       # 3 or 4 key points + the centroid: 4 or 5 of 9
            h.raw[b, 0, 2 * K, cell[1], cell[0]] = 0.0
    return h


def _multi_case(nB):
    """(g) 5 anchors x 8 x 8, 4 classes.  Per image: ground truth 0 with a 3 x 3-cell box (IoU 6/11 with both (2,4) and
    (4,2): the first, anchor 1, owns it), ground truth 1 with a zero-size box (every IoU 0: the last anchor), ground truth
    2 with an 8 x 8 box (anchor 3).  tconf is read from the last anchor of the previous image: for ground truth 0 that
    cell is a perfect hit and the image's own cell a miss, for ground truth 2 the other way round."""
    h = Head('multi%d' % nB, nB, 8, 8, nA=5, nC=4, multi=True, class_scale=2.0)
    for b in range(nB):
        prev = (b - 1) % nB
        c0, c1, c2 = (1 + b, 1), (6, 4), (2 + b, 6)
        g0, g1, g2 = h.star(c0, turn=b), h.star(c1, turn=b + 1), h.star(c2, turn=b + 2)
        h.add_gt(b, g0, cls=1, box=(3.0 / 8, 3.0 / 8))
        h.add_gt(b, g1, cls=3, box=(0.0, 0.0))
        h.add_gt(b, g2, cls=0, box=(1.0, 1.0))
        h.aim(b, 1, c0, g0, set())
        h.aim(b, 0, c0, g0, set(range(1, K)))                # owns nothing (anchor 1 does): the 9-of-9 cell of the ladder
        h.aim(prev, 4, c0, g0, set(range(1, K)))
        h.aim(b, 3, c2, g2, set(range(1, K)))
        h.aim(prev, 4, c2, g2, set())
        if (b, 4, c1[1], c1[0]) not in h.reserved:
            h.aim(b, 4, c1, g1, {1, 2, 3, 4, 5})
    for b in range(nB):
        h.ladder(b, h.labels[b, 0, 1:1 + 2 * K].reshape(K, 2))
    return h


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'ladder8':
        return _ladder_case(name, 2, 8, 8, 1, [(1, 1), (6, 5)])
    if name == 'ladder16':
        return _ladder_case(name, 2, 16, 16, 1, [(2, 3), (13, 12)])
    if name == 'ladder8x2':                       # two anchors: the second anchor of the owning cell is a 9-of-9 cell
        return _ladder_case(name, 2, 8, 8, 2, [(1, 1), (6, 5)])
    if name == 'ladder32':                        # (i) 1024 cells: four passes of the 256 threads
        return _ladder_case(name, 1, 32, 32, 1, [(5, 4)])
    if name == 'limit64':                         # (h) 4096 cells, the ground truth in the last one
        return _ladder_case(name, 1, 64, 64, 1, [(63, 63)])
    if name == 'overlap':
        return _overlap_case()
    if name == 'ownership':
        return _ownership_case()
    if name in ('boundary8', 'boundary16'):
        return _boundary_case(int(name[8:]))
    if name == 'grid26':
        return _grid26_case()
    if name in ('rounding13', 'rounding21'):
        return _rounding_case(int(name[8:]))
    if name == 'counts':
        return _counts_case()
    if name in ('multi1', 'multi3'):
        return _multi_case(int(name[5:]))
    raise KeyError(name)


def _ladder_runs(name, ms):
    return [(name, np.float64, f(m)) for m in ms for f in (thresh_tie, thresh_below)]


# (case, label dtype, thresh): every run of both test files
RUNS = (_ladder_runs('ladder8', (1, 4, 8)) + _ladder_runs('ladder16', (2, 5, 7)) + _ladder_runs('ladder8x2', (3, 9))
        + _ladder_runs('ladder32', (1, 6, 8)) + _ladder_runs('limit64', (4,)) + _ladder_runs('overlap', (5,))
        + _ladder_runs('multi3', (5, 9)) + _ladder_runs('multi1', (9,))
        + [('ladder8', np.float32, 0.0), ('ladder16', np.float32, 0.6)]
        + [(n, dt, 0.6) for n in ('ownership', 'boundary8', 'boundary16', 'grid26', 'rounding13', 'rounding21', 'counts',
                                  'multi3', 'multi1') for dt in (np.float64, np.float32)])


def run_id(run):
    return '%s-%s-%.9g' % (run[0], np.dtype(run[1]).name, run[2])


@functools.lru_cache(maxsize=None)
def expected(name, dtype, thresh):
    return expect(case(name), dtype, thresh)


# ------------------------------------------------------------------------------------------------ the decode cases
NEG = -1000.0          # a class logit whose expf underflows to exactly 0: the soft-max maximum is exactly 1, 1/2 or 1/4
LOW = -3.0             # raw confidence of the cells that take no part


class DecodeCase(object):
    """head (nB, nA*(2K+1+nC), nH, nW) float32 with nC = 4; every image is one scenario (see decode_case)."""

    def __init__(self, nH, nW, nA):
        self.nH, self.nW, self.nA, self.nC = nH, nW, nA, 4
        self.notes = []
        self.images = []

    def image(self, note, cells):
        """cells: {key: (raw_conf, n_zero_logits, first_class)} in scan order key = (cy * nW + cx) * nA + anchor."""
        nH, nW, nA = self.nH, self.nW, self.nA
        rs = np.random.RandomState(len(self.images) + nH * nA)
        raw = np.zeros((nA, 2 * K + 1 + 4, nH, nW))
        raw[:, 2:2 * K] = rs.randint(-16, 17, (nA, 2 * K - 2, nH, nW)) / 8.0
        raw[:, 2 * K] = LOW
        raw[:, 2 * K + 1:] = NEG
        raw[:, 2 * K + 1 + 2] = 0.0                                    # everyone else: class 2, probability 1
        for key, (rc, nz, first) in cells.items():
            an, rem = key % nA, key // nA
            j, i = rem // nW, rem % nW
            raw[an, 2 * K, j, i] = rc
            raw[an, 2 * K + 1:, j, i] = NEG
            raw[an, 2 * K + 1 + first:2 * K + 1 + first + nz, j, i] = 0.0
        self.images.append(raw)
        self.notes.append(note)

    @property
    def head(self):
        return np.stack(self.images).astype(np.float32).reshape(len(self.images), -1, self.nH, self.nW)


@functools.lru_cache(maxsize=None)
def decode_case(nH, nW, nA):
    """Scenarios (keys are scan-order keys; the loss kernel's cell index is a different order when nA > 1):
      0  tie between two keys handled by the same thread (k, k + 256) - or two lanes of the one wave when ncell <= 256
      1  tie between keys in different waves, the larger key on the lower thread
      2  tie between two anchors of one cell, and with the first anchor of the NEXT cell (which comes first in memory)
      3  NaN confidences on part of the image, the would-be winner and key 0 among them
      4  the largest objectness has class probability 1/4, a smaller one probability 1: the winner depends on
         only_objectness; the winner's class arg-max is a tie of two classes (the first wins)
      5  every confidence NaN"""
    c = DecodeCase(nH, nW, nA)
    ncell = nA * nH * nW
    nan = float('nan')
    big = ncell > 256
    a, bkey = (7, 7 + 256) if big else (5, 40)
    c.image('same thread', {a: (1.0, 1, 1), bkey: (1.0, 1, 3), 3: (0.0, 1, 0)})
    w1, w2 = ((256 + 10, 200) if big else (50, 9))
    c.image('waves', {w1: (2.0, 1, 0), w2: (2.0, 1, 1), ncell - 1: (2.0, 1, 2)})
    cell = 11
    if nA > 1:
        c.image('anchors', {cell * nA + 3: (1.0, 1, 1), cell * nA + 1: (1.0, 1, 0), (cell + 1) * nA: (1.0, 1, 3),
                            (cell - 1) * nA + 2: (0.0, 1, 2)})
    else:
        c.image('anchors', {cell: (1.0, 1, 1), cell + 1: (1.0, 1, 0)})
    c.image('part NaN', {0: (nan, 1, 0), 20: (nan, 1, 1), ncell - 2: (nan, 1, 0), 33: (0.0, 1, 3), 21: (0.0, 2, 0),
                         60: (-1.0, 1, 2)})
    c.image('objectness', {12: (2.0, 4, 0), 45: (0.0, 2, 1), 30: (1.0, 4, 0), 50: (0.0, 2, 2)})
    c.images.append(c.images[0].copy())
    c.images[-1][:, 2 * K] = nan
    c.notes.append('all NaN')
    return c


def decode_expect(dc, only_objectness):
    """float64 statement of region_decode_argmax on every image: dict(key, coords (2K float32, exact), det, cls_conf
    (exact), cls_id, conf, margin) or None for an image without any comparable confidence.  margin: the smallest
    relative distance of the winning confidence from a different one."""
    out = []
    nH, nW, nA = dc.nH, dc.nW, dc.nA
    for raw in dc.images:
        raw = raw.astype(np.float32).astype(np.float64)
        z = raw[:, 2 * K + 1:]
        e = np.exp(z - z.max(axis=1, keepdims=True))
        prob = e / e.sum(axis=1, keepdims=True)
        det = _sig(raw[:, 2 * K])
        conf = det if only_objectness else det * prob.max(axis=1)
        best, bkey = -np.inf, None
        for key in range(nA * nH * nW):                       # the reference's scan: strict '>' keeps the first maximum
            an, rem = key % nA, key // nA
            v = conf[an, rem // nW, rem % nW]
            if v > best:
                best, bkey = v, key
        if bkey is None:
            out.append(None)
            continue
        an, rem = bkey % nA, bkey // nA
        j, i = rem // nW, rem % nW
        coords = np.empty(2 * K)
        coords[0::2] = (np.concatenate([[_sig(raw[an, 0, j, i])], raw[an, 2:2 * K:2, j, i]]) + i) / nW
        coords[1::2] = (np.concatenate([[_sig(raw[an, 1, j, i])], raw[an, 3:2 * K:2, j, i]]) + j) / nH
        other = conf[np.isfinite(conf) & (conf != best)]
        out.append(dict(key=bkey, coords=coords.astype(np.float32), det=float(det[an, j, i]),
                        cls_conf=float(prob[an, :, j, i].max()), cls_id=int(prob[an, :, j, i].argmax()), conf=float(best),
                        margin=float((np.abs(other - best) / best).min()) if other.size else np.inf,
                        ties=int((conf == best).sum())))
    return out

"""Inputs and CPU expectations shared by the batched multi-object validator tests (test_eval_multi_cpu.py,
test_gpu_eval_multi.py).  Everything here runs on the CPU: the heads, the labels, the decode the preconditions are
checked on, and the reference selection (oracle.region_loss_ref.get_multi_region_boxes_ref, one image at a time,
followed by valid_multi.py:118-123 restated).  Each case is built once per process and never modified.
"""
import functools
import sys

import numpy as np
import torch

from helpers import gold

K = 9
NL = 2 * K + 3
MAX_GT = 50
ANCHORS = [1.4820, 2.2412, 2.0501, 3.1265, 2.3946, 4.6891, 3.1018, 3.9910, 3.4879, 5.8851]
REL = 1e-5          # the margin every decision of a case must have (relative), see check_preconditions


_BUILT = {}       # name -> Case, filled as soon as a case's head exists (the labels are derived from the head)


class Case(object):
    def __init__(self, name, head, target, nA, nC, conf_thresh, im_size=(640, 480)):
        self.name, self.head, self.target = name, head, target            # float32 (B,C,H,W), float32 (B,50,21)
        self.nA, self.nC, self.conf_thresh, self.im_size = nA, nC, conf_thresh, im_size
        self.B, self.H, self.W = head.shape[0], head.shape[2], head.shape[3]
        self.ncell = nA * self.H * self.W
        _BUILT[name] = self

    def num_gts(self, b):
        stop = np.nonzero(self.target[b, :, 1] == 0)[0]
        return int(stop[0]) if len(stop) else MAX_GT

    def gts(self):
        """(b, k, class) of every label row below its image's ground-truth count."""
        return [(b, k, int(self.target[b, k, 0])) for b in range(self.B) for k in range(self.num_gts(b))]


def decode_cpu(case):
    """det (B,ncell), softmax (B,ncell,nC) in scan order key = (cy*W + cx)*nA + anchor: torch's CPU sigmoid / softmax,
    the operations oracle.region_loss_ref decodes with (test_eval_multi_cpu.py checks that the two agree to 1e-6)."""
    o = torch.from_numpy(case.head).view(case.B, case.nA, 2 * K + 1 + case.nC, case.H, case.W)
    o = o.permute(0, 3, 4, 1, 2).reshape(case.B, case.ncell, 2 * K + 1 + case.nC)
    det = torch.sigmoid(o[..., 2 * K])
    prob = torch.softmax(o[..., 2 * K + 1:], dim=2)
    return det.numpy(), prob.numpy(), o[..., 2 * K].numpy()


def _clear(a, b):
    return abs(float(a) - float(b)) > REL * max(abs(float(a)), abs(float(b)))


def check_preconditions(case):
    """An assertion about the DATA of a case (never a skip): every decision the validator takes on it has a margin far
    above what two fp32 evaluations of the same formulas can differ by, so that selecting another cell is a bug of the
    code under test and not a rounding accident.
      - no cell's conf = det * cls_max lies within 1e-5 (relative) of the threshold;
      - in the selection (largest det_conf among the kept cells of the class) and in every step of the fallback chain
        (`det > max_conf and p_c > max_cls_conf`; the second comparison runs when the first one passed, as in Python)
        the two values compared differ by more than 1e-5 relative.  The one exception is the deliberate tie: two
        det_conf values produced by bit-identical logits are equal on every path."""
    det, prob, det_logit = decode_cpu(case)
    cmax, cid = prob.max(axis=2), prob.argmax(axis=2)
    conf = det * cmax
    th = case.conf_thresh
    fin = np.isfinite(conf)
    assert np.all(np.abs(conf[fin] - th) > REL * abs(th)), case.name
    for b in range(case.B):
        for c in sorted(set(cls for bb, _, cls in case.gts() if bb == b and 0 <= cls < case.nC)):
            best, best_ind = -sys.maxsize, None
            for ind in np.nonzero((conf[b] > th) & (cid[b] == c))[0]:
                same_logit = best_ind is not None and det_logit[b, ind] == det_logit[b, best_ind]
                assert same_logit or _clear(det[b, ind], best), (case.name, b, c, ind)
                if det[b, ind] > best:
                    best, best_ind = det[b, ind], ind
            if best_ind is not None:
                continue            # a kept cell of class c exists: the chain's result is not used
            m, q = -1.0, -float(sys.maxsize)
            for ind in range(case.ncell):
                d, p = det[b, ind], prob[b, ind, c]
                if np.isnan(d):
                    continue
                assert _clear(d, m), (case.name, b, c, ind)
                if d > m:
                    assert _clear(p, q), (case.name, b, c, ind)
                    if p > q:
                        m, q = d, p


def select(boxes, c):
    """valid_multi.py:118-123: index of the box of class c with the largest det_conf, strict '>' (first one on a tie)."""
    best, pick = -sys.maxsize, None
    for j, bx in enumerate(boxes):
        if bx[2 * K] > best and bx[2 * K + 2] == c:
            best, pick = bx[2 * K], j
    return pick


@functools.lru_cache(maxsize=None)
def _reference_boxes(name, b, c):
    from oracle.region_loss_ref import get_multi_region_boxes_ref
    case = _BUILT[name]
    return get_multi_region_boxes_ref(torch.from_numpy(case.head[b:b + 1]), case.conf_thresh, case.nC, K, case.nA, c,
                                      only_objectness=0)[0]


def reference_row(case, b, c):
    """The box (2K+3 numbers) the reference's validator selects for class c on image b alone, or None when the image has
    no result: c outside [0, nC) (the reference indexes out of range) or det_conf NaN everywhere (it raises
    UnboundLocalError)."""
    if not 0 <= c < case.nC or np.all(np.isnan(decode_cpu(case)[0][b])):
        return None
    boxes = _reference_boxes(case.name, b, c)
    return boxes[select(boxes, c)]


def _label_rows(entries):
    """[(class, 18 corner coordinates)] -> (50, 21) float32 label block; the box width / height columns are not read."""
    t = np.zeros((MAX_GT, NL), dtype=np.float32)
    for k, (c, corners) in enumerate(entries):
        t[k, 0] = c
        t[k, 1:2 * K + 1] = corners
        t[k, 2 * K + 1:] = 0.2
    return t


def _with_corners_near_the_prediction(case, classes, rs):
    """Fill case.target: ground truth k of image b has class classes[b][k]; even rows lie within 0.02 of the box the
    reference selects (so `match` is non-zero), odd rows half an image away (match exactly 0)."""
    for b, cl in enumerate(classes):
        entries = []
        for k, c in enumerate(cl):
            ref = reference_row(case, b, c)
            base = np.asarray(ref[:2 * K]) if ref is not None else rs.uniform(0.2, 0.8, 2 * K)
            corners = base + (rs.uniform(-0.02, 0.02, 2 * K) if k % 2 == 0 else 0.5)
            entries.append((c, corners))
        case.target[b] = _label_rows(entries)
    return case


@functools.lru_cache(maxsize=None)
def golden_case():
    """tests/golden/decode_multi.npz: B=2, 5 anchors, 13 classes, 13x13 -> 845 cells (not a multiple of 64).  Class 7
    never wins the arg-max (fallback, source 2); classes 4 and 8 have kept cells (source 1); image 1 has three kept
    cells of class 4 and two ground truths of that class."""
    g = gold('decode_multi.npz')
    case = Case('golden', np.ascontiguousarray(g['output']), np.zeros((2, MAX_GT, NL), dtype=np.float32), 5, 13, 0.05)
    return _with_corners_near_the_prediction(case, [[4, 7, 11, 0], [8, 7, 4, 3, 4]], np.random.RandomState(5))


def _logit(p):
    return float(np.log(p / (1.0 - p)))


SMALL_SEED = 3


@functools.lru_cache(maxsize=None)
def small_case():
    """3x2 grid (H != W), 2 anchors, 3 classes: 12 cells, fewer than one wave; conf_thresh 0.99.
      images 0-2  seeded; nothing is kept, every class takes the fallback.  Image 0, class 1: the first four cells in
                  scan order are (det .3, p .2), (.9, .1), (.4, .5), (.35, .9) and every later one has det < .3, so the
                  chain ends on the third cell - neither the det arg-max (the second) nor the p arg-max (the fourth)
      image 3     every det logit NaN: no result
      image 4     two ground truths of class 2, one of class 0, one of class 5 (outside [0, 3): no result)
      image 5     three kept cells of class 1; keys 3 and 8 tie in det_conf (the same logit), key 3 must win although key 8
                  has the larger class confidence and key 1 comes first
      image 6     50 ground truths, no terminator row; one kept cell of class 2"""
    rs = np.random.RandomState(SMALL_SEED)
    B, nA, nC, H, W = 7, 2, 3, 3, 2
    nCh = 2 * K + 1 + nC
    cells = rs.standard_normal((B, H * W * nA, nCh)).astype(np.float32)       # scan order: key = (cy*W + cx)*nA + anchor
    cells[0, :, 2 * K] = [_logit(v) for v in (.3, .9, .4, .35)] + list(rs.uniform(-3.0, -1.5, 8))
    for key, p in enumerate((.2, .1, .5, .9)):
        cells[0, key, 2 * K + 1:] = np.log([(1 - p) * .6, p, (1 - p) * .4])
    cells[3, :, 2 * K] = np.nan
    cells[5, :, 2 * K] = rs.uniform(-2.0, 2.0, 12)
    for key, (dl, margin) in {1: (7.5, 14.0), 3: (8.0, 12.0), 8: (8.0, 14.0)}.items():
        cells[5, key, 2 * K] = dl
        cells[5, key, 2 * K + 1:] = [0.0, margin, 0.0]
    cells[6, 7, 2 * K] = 9.0
    cells[6, 7, 2 * K + 1:] = [0.0, 0.0, 13.0]
    head = cells.reshape(B, H, W, nA, nCh).transpose(0, 3, 4, 1, 2).reshape(B, nA * nCh, H, W)
    case = Case('small', np.ascontiguousarray(head), np.zeros((B, MAX_GT, NL), dtype=np.float32), nA, nC, 0.99, (320, 240))
    classes = [[0, 1, 2], [2, 0], [1], [0, 2], [2, 0, 2, 5], [1, 0], [k % 3 for k in range(MAX_GT)]]
    return _with_corners_near_the_prediction(case, classes, rs)


@functools.lru_cache(maxsize=None)
def chain_case():
    """The evaluation chain's input: 5 anchors, 13 classes, 13x13, B=3, poses of oracle.eval_ref.synthetic_eval_case.
    Every ground truth but one has a cell planted in the head (high det_conf, its class, corners = the projected box
    corners + up to 1.5 px of noise); the last ground truth of image 2 has none and takes the fallback."""
    from oracle.eval_ref import synthetic_eval_case
    from singleshotpose_amd.utils import get_3D_corners
    rs = np.random.RandomState(17)
    B, nA, nC, H, W = 3, 5, 13, 13, 13
    nCh = 2 * K + 1 + nC
    pts, Kc, R_gt, t_gt, _, _ = synthetic_eval_case(11, n_pose=7, n_vert=400)
    vertices = np.concatenate((pts.T, np.ones((1, 400))), axis=0)
    obj = np.concatenate((np.zeros((3, 1)), get_3D_corners(vertices)[:3, :]), axis=1)          # (3, 9): centroid + corners
    cells = (rs.standard_normal((B, H, W, nA, nCh)) * 0.5).astype(np.float32)
    cells[..., 2 * K] -= 3.0                                                                # det_conf around 0.05
    plan = [[(2, 0), (5, 1)], [(9, 2), (0, 3), (12, 4)], [(7, 5), (3, None)]]              # (class, pose or None)
    order = [0, 1, 3, 5, 7, 2, 4, 6, 8]                                                      # fix_corner_order
    target = np.zeros((B, MAX_GT, NL), dtype=np.float32)
    for b, gts in enumerate(plan):
        entries = []
        for k, (c, pose) in enumerate(gts):
            if pose is None:
                entries.append((c, rs.uniform(0.3, 0.7, 2 * K)))
                continue
            cam = Kc.dot(np.concatenate((R_gt[pose], t_gt[pose]), axis=1)).dot(np.concatenate((obj, np.ones((1, 9)))))
            uv = (cam[:2] / cam[2]).T / np.array([640.0, 480.0])                              # (9, 2), PnP order
            label = np.zeros((K, 2))
            label[order] = uv                                                                # fix_corner_order undoes this
            entries.append((c, label.reshape(-1)))
            pr = uv + rs.uniform(-1.5, 1.5, (K, 2)) / np.array([640.0, 480.0])
            cx, cy, an = int(pr[0, 0] * W), int(pr[0, 1] * H), (b + k) % nA
            raw = pr * np.array([W, H]) - np.array([cx, cy])
            raw[0] = np.log(raw[0] / (1.0 - raw[0]))                                         # keypoint 0 goes through the sigmoid
            cells[b, cy, cx, an, :2 * K] = raw.reshape(-1)
            cells[b, cy, cx, an, 2 * K] = 4.0 + k
            cells[b, cy, cx, an, 2 * K + 1:] = 0.0
            cells[b, cy, cx, an, 2 * K + 1 + c] = 12.0
        target[b] = _label_rows(entries)
    head = cells.transpose(0, 3, 4, 1, 2).reshape(B, nA * nCh, H, W)
    case = Case('chain', np.ascontiguousarray(head), target, nA, nC, 0.5)
    case.vertices, case.intrinsics, case.plan = vertices, Kc, plan
    return case


CASES = {'golden': golden_case, 'small': small_case, 'chain': chain_case}

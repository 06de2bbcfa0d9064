"""Inputs and CPU expectations of the label-free multi-object detector tests (test_detect_multi_cpu.py,
test_gpu_detect_multi.py).  The heads of eval_multi_cases.py queried for EVERY class, plus two heads of their own:
`tiny` (24 cells, fewer than one wave) and `edge` (845 cells; kept cells, an all-fallback image behind them, a tie of
bit-identical logits, a NaN image).  Everything here runs on the CPU; each case is built once per process and never
modified.  The expectation of (image b, class c) is eval_multi_cases.reference_row (oracle.region_loss_ref run on the
image alone + valid_multi.py:118-123) for the floats and `restated` below for source and key; test_detect_multi_cpu.py
holds the two against each other.
"""
import functools
import sys

import numpy as np

from eval_multi_cases import ANCHORS, CASES, K, REL, Case, decode_cpu, reference_row, select  # noqa: F401

MAX_GT = 50
NL = 2 * K + 3


def _clear(a, b):
    return abs(float(a) - float(b)) > REL * max(abs(float(a)), abs(float(b)))


def check_preconditions_all(case, classes):
    """eval_multi_cases.check_preconditions for every queried class of every image instead of the classes of the ground
    truths.  An assertion about the DATA (never a skip): no cell's conf = det * cls_max lies within 1e-5 (relative) of
    the threshold; in the selection among the kept cells of the class and in every step of the fallback chain
    (`det > max_conf and p_c > max_cls_conf`, the second comparison only when the first passed) the two values compared
    differ by more than 1e-5 relative.  The one allowed tie: det_conf values from bit-identical logits."""
    det, prob, det_logit = decode_cpu(case)
    cmax, cid = prob.max(axis=2), prob.argmax(axis=2)
    conf = det * cmax
    th = case.conf_thresh
    fin = np.isfinite(conf)
    assert np.all(np.abs(conf[fin] - th) > REL * abs(th)), case.name
    for b in range(case.B):
        for c in sorted(set(int(c) for c in classes)):
            assert 0 <= c < case.nC
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


def coords_cpu(case, b, key):
    """The 2K normalised corner coordinates of cell `key` (scan order) of image b: (v + cx) / W, (v + cy) / H, keypoint 0
    through the sigmoid first (utils_multi.py:300-330), in float32."""
    an, rem = key % case.nA, key // case.nA
    cy, cx = rem // case.W, rem % case.W
    nCh = 2 * K + 1 + case.nC
    v = case.head[b, an * nCh:an * nCh + 2 * K, cy, cx].astype(np.float32).copy()
    v[:2] = np.float32(1.0) / (np.float32(1.0) + np.exp(-v[:2]))
    v[0::2] = (v[0::2] + np.float32(cx)) / np.float32(case.W)
    v[1::2] = (v[1::2] + np.float32(cy)) / np.float32(case.H)
    return v


def restated(case, b, c):
    """(source, key, row) for class c on image b alone, restated plainly on decode_cpu: source 1 the kept cell
    (conf > thresh, arg-max class c) with the largest det_conf, the first in scan order on a tie; else source 2 the last
    cell the sequential `det > max_conf and p_c > max_cls_conf` walk takes; (0, -1, None) when it takes none or c is
    outside [0, nC).  row: 2K coordinates, det_conf, class confidence, class."""
    if not 0 <= c < case.nC:
        return 0, -1, None
    det, prob, _ = decode_cpu(case)
    det, prob = det[b], prob[b]
    cmax, cid = prob.max(axis=1), prob.argmax(axis=1)
    conf = det * cmax
    best, key = -float(sys.maxsize), None
    for ind in range(case.ncell):
        if conf[ind] > case.conf_thresh and cid[ind] == c and det[ind] > best:
            best, key = det[ind], ind
    if key is not None:
        return 1, key, np.concatenate((coords_cpu(case, b, key), [det[key], cmax[key], c])).astype(np.float32)
    m, q, key = -1.0, -float(sys.maxsize), None
    for ind in range(case.ncell):
        if det[ind] > m and prob[ind, c] > q:
            m, q, key = det[ind], prob[ind, c], ind
    if key is None:
        return 0, -1, None
    return 2, key, np.concatenate((coords_cpu(case, b, key), [m, q, c])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def table(name):
    """{(b, c): (reference_row or None, source, key)} for every image and every class of a case."""
    case = ALL_CASES[name]()
    res = {}
    for b in range(case.B):
        for c in range(case.nC):
            source, key, _ = restated(case, b, c)
            res[(b, c)] = (reference_row(case, b, c), source, key)
    return res


def _head_from_cells(cells):
    """(B, H, W, nA, nCh) cells in scan order -> the head (B, nA*nCh, H, W)."""
    B, H, W, nA, nCh = cells.shape
    return np.ascontiguousarray(cells.transpose(0, 3, 4, 1, 2).reshape(B, nA * nCh, H, W))


TINY_SEED = 1
EDGE_SEED = 2


@functools.lru_cache(maxsize=None)
def tiny_case():
    """B=2, 2 anchors, 3 classes, 3 rows x 4 columns: 24 cells, fewer than one wave - most lanes of the workgroup hold no
    cell and one of the four waves has no class to work on.  conf_thresh 0.5: image 0 keeps a few cells, image 1
    (det logits lowered by 4) keeps none."""
    rs = np.random.RandomState(TINY_SEED)
    B, nA, nC, H, W = 2, 2, 3, 3, 4
    cells = rs.standard_normal((B, H, W, nA, 2 * K + 1 + nC)).astype(np.float32)
    cells[0, ..., 2 * K] += 1.0
    cells[0, ..., 2 * K + 1:] *= 3.0
    cells[1, ..., 2 * K] -= 4.0
    return Case('tiny', _head_from_cells(cells), np.zeros((B, MAX_GT, NL), dtype=np.float32), nA, nC, 0.5)


@functools.lru_cache(maxsize=None)
def edge_case():
    """B=4, 5 anchors, 13 classes, 13x13: 845 cells, no multiple of 64.  Background det_conf around 0.05, conf_thresh 0.5.
      image 0  planted kept cells of classes 1, 4 (two cells), 9 and 12
      image 1  nothing over the threshold: every class takes the fallback - BEHIND image 0, so state carried from one
               image to the next would show
      image 2  class 6: two cells with bit-identical logits (keys 301 and 700, the first must win) above a third kept
               cell of that class that comes first in scan order (key 17)
      image 3  every det logit NaN: no class has a result"""
    rs = np.random.RandomState(EDGE_SEED)
    B, nA, nC, H, W = 4, 5, 13, 13, 13
    nCh = 2 * K + 1 + nC
    cells = (rs.standard_normal((B, H * W * nA, nCh)) * 0.5).astype(np.float32)         # scan order
    cells[..., 2 * K] -= 3.0

    def plant(b, key, c, det_logit):
        cells[b, key, 2 * K] = det_logit
        cells[b, key, 2 * K + 1:] = 0.0
        cells[b, key, 2 * K + 1 + c] = 12.0

    for key, c, dl in ((5, 1, 4.0), (130, 4, 3.0), (511, 4, 5.0), (640, 9, 2.5), (844, 12, 6.0)):
        plant(0, key, c, dl)
    plant(2, 17, 6, 3.0)
    plant(2, 301, 6, 4.5)
    cells[2, 700] = cells[2, 301]
    cells[3, :, 2 * K] = np.nan
    head = _head_from_cells(cells.reshape(B, H, W, nA, nCh))
    return Case('edge', head, np.zeros((B, MAX_GT, NL), dtype=np.float32), nA, nC, 0.5)


ALL_CASES = dict(CASES, tiny=tiny_case, edge=edge_case)


def meshes_for(classes):
    """({class id: (4, 400) mesh}, intrinsics): the chain case's mesh scaled by 5 % per class id, so that every class has
    object points of its own."""
    chain = CASES['chain']()
    return {c: chain.vertices * (1.0 + 0.05 * c) for c in classes}, chain.intrinsics

"""CPU side of the label-free multi-object detector: the C ABI table, the test inputs themselves (margins and coverage
are properties of the data, checked here without a GPU), the reference selection against a plain restatement, the
argument checks that must fire before any library call, and the drop-in names."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import detect_multi_cases as D
from detect_multi_cases import K
from helpers import ROOT


def test_abi_table_has_the_detect_entry():
    from singleshotpose_amd import _lib
    assert 'ssp_region_detect_multi' in _lib.exported_symbols()
    header = open(os.path.join(ROOT, 'include', 'ssp_hip.h')).read()
    decl = re.search(r'int ssp_region_detect_multi\(([^;]*)\);', header).group(1)
    assert len(_lib._SIGS['ssp_region_detect_multi']) == len(decl.split(',')) == 14
    assert _lib.query('ssp_abi_version') == 5


@pytest.mark.parametrize('name', sorted(D.ALL_CASES))
def test_case_preconditions_hold_for_every_class(name):
    case = D.ALL_CASES[name]()
    D.check_preconditions_all(case, range(case.nC))


def test_new_cases_hold_what_the_issue_asks_for():
    tiny, edge = D.tiny_case(), D.edge_case()
    assert (tiny.B, tiny.nA, tiny.nC, tiny.H, tiny.W, tiny.ncell) == (2, 2, 3, 3, 4, 24)
    assert (edge.B, edge.nA, edge.nC, edge.H, edge.W, edge.ncell) == (4, 5, 13, 13, 13, 845) and edge.ncell % 64 != 0
    det, prob, logit = D.decode_cpu(edge)
    conf = det * prob.max(axis=2)
    assert not np.any(conf[1] > edge.conf_thresh) and np.all(np.isnan(det[3])) and np.all(np.isfinite(det[:3]))
    nCh = 2 * K + 1 + edge.nC
    cells = edge.head.reshape(4, 5, nCh, 13, 13).transpose(0, 3, 4, 1, 2).reshape(4, 845, nCh)
    assert np.array_equal(cells[2, 301], cells[2, 700]) and logit[2, 301] > logit[2, 17] > 0


def test_reference_selection_covers_every_source():
    """From the reference selection alone, so that the GPU comparison cannot pass vacuously."""
    sources = set()
    for name in D.ALL_CASES:
        sources |= set(s for _, s, _ in D.table(name).values())
    assert sources == {0, 1, 2}
    edge = D.table('edge')
    assert all(edge[(1, c)][1] == 2 for c in range(13))
    assert sum(edge[(0, c)][1] == 1 for c in range(13)) >= 3
    assert all(edge[(3, c)] == (None, 0, -1) for c in range(13))
    assert edge[(2, 6)][1:] == (1, 301)                      # the tie: the first of the two cells in scan order
    tiny = D.table('tiny')
    assert all(tiny[(1, c)][1] == 2 for c in range(3))


@pytest.mark.parametrize('name', sorted(D.ALL_CASES))
def test_reference_row_agrees_with_the_plain_restatement(name):
    """reference_row (the oracle's get_multi_region_boxes_ref on the image alone + the validator's selection) against
    `restated` (decode_cpu + two plain loops) for EVERY class - most of them have no ground truth in the case: the same
    det_conf / class confidence / class and the coordinates of the cell `restated` names, to 1e-5 (two CPU evaluations of
    the same fp32 formulas)."""
    case = D.ALL_CASES[name]()
    labelled = set((b, c) for b, _, c in case.gts())
    unlabelled = 0
    for (b, c), (ref, source, key) in D.table(name).items():
        _, _, row = D.restated(case, b, c)
        assert (ref is None) == (row is None) == (source == 0) and (key == -1) == (source == 0)
        if ref is None:
            continue
        assert len(ref) == 2 * K + 3 and int(ref[2 * K + 2]) == c
        np.testing.assert_allclose(row, np.asarray(ref, dtype=np.float64), rtol=1e-5, atol=1e-7, err_msg=str((b, c)))
        unlabelled += (b, c) not in labelled
    assert unlabelled >= 3
    assert D.restated(case, 0, case.nC) == (0, -1, None) and D.restated(case, 0, -1) == (0, -1, None)


def test_argument_checks_raise_before_any_library_call(monkeypatch):
    from singleshotpose_amd import _lib
    from singleshotpose_amd.utils_multi import detect_multi_batched, detect_multi_region_boxes

    def no_call(name, *args):
        raise AssertionError("%s was called" % name)
    monkeypatch.setattr(_lib, 'call', no_call)
    case = D.tiny_case()
    head = torch.from_numpy(case.head)                  # a CPU tensor: nothing below may get as far as the GPU
    for classes in ([], [0, 3], [-1], [1, 2, 7]):
        with pytest.raises(ValueError):
            detect_multi_region_boxes(head, 0.5, case.nC, K, case.nA, classes=classes)
    for classes in (None, [2, 0], (1, 1), iter([0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            detect_multi_region_boxes(head, 0.5, case.nC, K, case.nA, classes=classes)
    meshes, Kc = D.meshes_for(range(3))
    args = (0.5, case.nC, K, D.ANCHORS[:4], case.nA)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detect_multi_batched(head, *args, meshes, Kc, 640, 480)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detect_multi_batched(head, *args, meshes, np.stack([Kc, Kc]), 640, 480, classes=[2])
    with pytest.raises(ValueError, match="no object model"):
        detect_multi_batched(head, *args, {0: meshes[0], 2: meshes[2]}, Kc, 640, 480, classes=[0, 1])
    with pytest.raises(ValueError):
        detect_multi_batched(head, *args, meshes, Kc, 640, 480, classes=[])
    with pytest.raises(ValueError, match="outside"):
        detect_multi_batched(head, *args, {0: meshes[0], 5: meshes[1]}, Kc, 640, 480)       # default list: the keys
    with pytest.raises(ValueError):
        detect_multi_batched(head, *args, {}, Kc, 640, 480)
    with pytest.raises(ValueError, match="per class"):
        detect_multi_batched(head, *args, meshes[0], Kc, 640, 480)                          # one mesh, no mapping
    with pytest.raises(ValueError, match="intrinsic_calibration"):
        detect_multi_batched(head, *args, meshes, np.stack([Kc, Kc, Kc]), 640, 480)         # 3 cameras, 2 images


def test_new_names_import_through_the_dropin_shim(monkeypatch):
    shims = [os.path.join(ROOT, 'dropin', 'multi_obj_pose_estimation'), os.path.join(ROOT, 'dropin')]
    for p in reversed(shims):
        monkeypatch.syspath_prepend(p)
    for m in ('utils', 'utils_multi'):
        monkeypatch.delitem(sys.modules, m, raising=False)
    try:
        import utils_multi
        from singleshotpose_amd import utils_multi as product
        assert os.path.dirname(utils_multi.__file__) == shims[0]
        for name in ('detect_multi_region_boxes', 'detect_multi_batched', 'MultiDetect', 'MultiPoses'):
            assert getattr(utils_multi, name) is getattr(product, name)
        scope = {}
        exec('from utils_multi import *', scope)           # what the reference's scripts do
        assert scope['detect_multi_batched'] is product.detect_multi_batched
        assert scope['detect_multi_region_boxes'] is product.detect_multi_region_boxes
    finally:
        for m in ('utils', 'utils_multi'):
            sys.modules.pop(m, None)

"""The label-free multi-object detector (utils_multi.detect_multi_region_boxes / detect_multi_batched) on the GPU against
the reference restated on the CPU, today's per-image path, the validator's match kernel (the same device code), and the
host-driven PnP chain.  Inputs and CPU expectations: detect_multi_cases.py."""
import numpy as np
import pytest
import torch

import detect_multi_cases as D
from detect_multi_cases import K

pytestmark = pytest.mark.gpu

RW = 2 * K + 3


def _detect(case, head, classes=None, only_objectness=0):
    from singleshotpose_amd.utils_multi import detect_multi_region_boxes
    d = detect_multi_region_boxes(head, case.conf_thresh, case.nC, K, case.nA, classes=classes,
                                  only_objectness=only_objectness)
    nQ = case.nC if classes is None else len(classes)
    assert d.boxes.is_cuda and d.boxes.shape == (head.size(0), nQ, RW) and d.boxes.dtype == torch.float32
    assert d.source.shape == d.key.shape == (head.size(0), nQ) and d.source.dtype == d.key.dtype == torch.int32
    assert d.classes.is_cuda and d.classes.dtype == torch.int32
    assert d.classes.tolist() == (list(range(case.nC)) if classes is None else list(classes))
    return d.boxes.cpu().numpy(), d.source.cpu().numpy(), d.key.cpu().numpy()


@pytest.fixture(scope='module')
def detected():
    """name -> (case, device head, boxes (B,nC,2K+3), source, key): one all-class launch per case, shared by the tests."""
    res = {}
    for name in sorted(D.ALL_CASES):
        case = D.ALL_CASES[name]()
        D.check_preconditions_all(case, range(case.nC))
        head = torch.from_numpy(case.head).cuda()
        res[name] = (case, head) + _detect(case, head)
    return res


@pytest.mark.parametrize('name', sorted(D.ALL_CASES))
def test_detect_equals_the_reference_for_every_image_and_class(detected, name):
    """Every (image, class) against reference_row (floats, rtol 1e-4 / atol 1e-6: the bar test_gpu_eval_multi.py holds the
    same comparison to) and the restated selection (source and key, exactly)."""
    case, _, boxes, source, key = detected[name]
    for (b, c), (ref, want_source, want_key) in D.table(name).items():
        assert (source[b, c], key[b, c]) == (want_source, want_key), (b, c)
        if ref is None:
            assert want_source == 0 and key[b, c] == -1 and np.all(boxes[b, c] == 0), (b, c)
            continue
        np.testing.assert_allclose(boxes[b, c], np.asarray(ref, dtype=np.float64), rtol=1e-4, atol=1e-6, err_msg=str((b, c)))
        assert boxes[b, c, 2 * K + 2] == c
    if name == 'edge':
        assert np.all(source[1] == 2) and np.all(source[3] == 0) and (source[2, 6], key[2, 6]) == (1, 301)
    if name == 'small':
        assert (source[0, 1], key[0, 1]) == (2, 2) and (source[5, 1], key[5, 1]) == (1, 3)


def _todays_path(case, head, b, c, only_objectness, rows):
    """(box, source, key) valid_multi.py:118-123 selects from today's get_multi_region_boxes on image b alone (the helper
    of test_gpu_eval_multi.py restated, with only_objectness)."""
    from singleshotpose_amd.utils_multi import get_multi_region_boxes
    conf = rows[:, 2 * K] if only_objectness else rows[:, 2 * K] * rows[:, 2 * K + 1]
    kept = np.nonzero(conf > case.conf_thresh)[0]
    boxes = get_multi_region_boxes(head[b:b + 1], case.conf_thresh, case.nC, K, D.ANCHORS, case.nA, c,
                                   only_objectness=only_objectness)[0]
    assert len(boxes) in (len(kept), len(kept) + 1)
    pick = D.select(boxes, c)
    if pick < len(kept):
        return boxes[pick], 1, int(kept[pick])
    hit = np.nonzero(np.all(rows[:, :2 * K] == np.asarray(boxes[pick][:2 * K], dtype=np.float32), axis=1))[0]
    assert len(hit) == 1
    return boxes[pick], 2, int(hit[0])


@pytest.mark.parametrize('only_objectness', [0, 1])
@pytest.mark.parametrize('name', sorted(D.ALL_CASES))
def test_detect_equals_todays_per_image_path(detected, name, only_objectness):
    """Same cell, source and class as get_multi_region_boxes(head[b:b+1], ..., correspondingclass=c) + the validator's
    selection, for every image and class; the 2K+2 floats to rtol 1e-6 (same formulas on the same device)."""
    from singleshotpose_amd.utils_multi import region_rows
    case, head = detected[name][:2]
    boxes, source, key = detected[name][2:] if only_objectness == 0 else _detect(case, head, None, 1)
    seen = set()
    for b in range(case.B):
        rows = region_rows(head[b:b + 1], case.nC, K, case.nA)[0]
        for c in range(case.nC):
            if np.all(np.isnan(rows[:, 2 * K])):         # today's path raises there, as the reference does
                assert source[b, c] == 0 and key[b, c] == -1 and np.all(boxes[b, c] == 0)
                continue
            box, want_source, want_key = _todays_path(case, head, b, c, only_objectness, rows)
            assert (source[b, c], key[b, c], int(boxes[b, c, 2 * K + 2])) == (want_source, want_key, c), (b, c)
            np.testing.assert_allclose(boxes[b, c, :2 * K + 2], np.asarray(box[:2 * K + 2], dtype=np.float32), rtol=1e-6,
                                       atol=0)
            seen.add(want_source)
    if only_objectness == 0:
        assert {1, 2} <= seen


@pytest.mark.parametrize('name', sorted(D.CASES))
def test_detect_rows_are_the_match_kernels_rows(detected, name):
    """On the labelled cases, for every ground truth (b, k, c): the validator's row is bit for bit the detector's row of
    (b, c) - both kernels call the same device functions."""
    from singleshotpose_amd.utils_multi import match_multi_region_boxes
    case, head, boxes, source, key = detected[name]
    m = match_multi_region_boxes(head, torch.from_numpy(case.target), case.conf_thresh, case.nC, K, case.nA,
                                 only_objectness=0, im_width=case.im_size[0], im_height=case.im_size[1])
    mb, ms, mk = m.boxes.cpu().numpy(), m.source.cpu().numpy(), m.key.cpu().numpy()
    checked = 0
    for b, k, c in case.gts():
        if not 0 <= c < case.nC:
            assert ms[b, k] == 0
            continue
        assert np.array_equal(mb[b, k, :RW], boxes[b, c]), (b, k, c)
        assert (ms[b, k], mk[b, k]) == (source[b, c], key[b, c]), (b, k, c)
        checked += 1
    assert checked >= 7


@pytest.mark.parametrize('name', ['edge', 'tiny'])
def test_class_lists(detected, name):
    case, head, boxes, source, key = detected[name]
    nC = case.nC
    lists = [list(range(nC)), [nC - 1], [2, 0], list(range(nC))[::-1], [1, 1, 0, 1], [nC - 1, 0] * 9]
    for classes in lists:
        got = _detect(case, head, classes)
        for want, have in zip((boxes, source, key), got):
            assert np.array_equal(have, want[:, classes]), classes


@pytest.mark.parametrize('name', ['edge', 'small'])
def test_images_are_independent(detected, name):
    case, head, boxes, source, key = detected[name]
    for b in range(case.B):
        got = _detect(case, head[b:b + 1])
        for want, have in zip((boxes, source, key), got):
            assert np.array_equal(have[0], want[b]), b


def _abi(head, classes, rows, meta, nA, nC, nQ, thresh, K_=K, shape=None):
    from singleshotpose_amd import _lib
    B, _, H, W = head.shape if shape is None else shape
    return _lib.call('ssp_region_detect_multi', head.data_ptr(), None if classes is None else classes.data_ptr(),
                     None if rows is None else rows.data_ptr(), meta.data_ptr(), B, nA, nC, H, W, K_, nQ, float(thresh), 0,
                     torch.cuda.current_stream().cuda_stream)


def test_every_output_element_is_written_and_foreign_class_ids_give_no_result(detected):
    case, head, boxes, source, key = detected['edge']
    sentinel = -777
    rows = torch.full((case.B, case.nC, RW), float('nan'), device='cuda')
    meta = torch.full((case.B, case.nC, 2), sentinel, dtype=torch.int32, device='cuda')
    _abi(head, None, rows, meta, case.nA, case.nC, case.nC, case.conf_thresh)
    r, m = rows.cpu().numpy(), meta.cpu().numpy()
    assert not np.any(np.isnan(r)) and not np.any(m == sentinel)
    assert np.array_equal(r, boxes) and np.array_equal(m[..., 0], source) and np.array_equal(m[..., 1], key)
    # class ids outside [0, nC) (the Python surface refuses them; the kernel answers `no result`), around a valid one
    ids = [-1, case.nC, 4, 65536, 4]
    classes = torch.tensor(ids, dtype=torch.int32).cuda()
    rows = torch.full((case.B, len(ids), RW), float('nan'), device='cuda')
    meta = torch.full((case.B, len(ids), 2), sentinel, dtype=torch.int32, device='cuda')
    _abi(head, classes, rows, meta, case.nA, case.nC, len(ids), case.conf_thresh)
    r, m = rows.cpu().numpy(), meta.cpu().numpy()
    for q, c in enumerate(ids):
        if c == 4:
            assert np.array_equal(r[:, q], boxes[:, 4]) and np.array_equal(m[:, q, 0], source[:, 4])
            assert np.array_equal(m[:, q, 1], key[:, 4])
        else:
            assert np.all(r[:, q] == 0) and np.all(m[:, q, 0] == 0) and np.all(m[:, q, 1] == -1)


def test_refusals_return_an_error_and_launch_nothing(detected):
    from singleshotpose_amd import _lib
    case, head = detected['edge'][:2]
    rows = torch.full((case.B, case.nC, RW), float('nan'), device='cuda')
    meta = torch.full((case.B, case.nC, 2), -777, dtype=torch.int32, device='cuda')
    classes = torch.arange(case.nC, dtype=torch.int32).cuda()
    a = (case.nA, case.nC)
    with pytest.raises(_lib.SspError, match="num_keypoints == 9"):
        _abi(head, classes, rows, meta, *a, case.nC, 0.5, K_=8)
    with pytest.raises(_lib.SspError, match="cells per image"):
        _abi(head, classes, rows, meta, 1, case.nC, case.nC, 0.5, shape=(1, 0, 1, 4097))
    with pytest.raises(_lib.SspError, match="queried class"):
        _abi(head, classes, rows, meta, *a, 0, 0.5)
    with pytest.raises(_lib.SspError, match="null buffer"):
        _abi(head, classes, None, meta, *a, case.nC, 0.5)
    with pytest.raises(_lib.SspError, match="classes == NULL"):
        _abi(head, None, rows, meta, *a, 3, 0.5)
    with pytest.raises(_lib.SspError, match="1..65535 classes"):
        _abi(head, classes, rows, meta, case.nA, 65536, case.nC, 0.5)
    torch.cuda.synchronize()
    assert np.all(np.isnan(rows.cpu().numpy())) and np.all(meta.cpu().numpy() == -777)


def _host_poses(meshes, Kc, corners, cls):
    """pnp_batched on the given pixel corners, each with the object points of its class and the float32-rounded K."""
    from singleshotpose_amd import utils as U
    objs = []
    for c in cls:
        corners3D = U.get_3D_corners(meshes[int(c)])
        objs.append(np.array(np.transpose(np.concatenate((np.zeros((3, 1)), corners3D[:3, :]), axis=1)), dtype='float32'))
    return U.pnp_batched(np.stack(objs), corners, np.array(Kc, dtype='float32'))


def test_pose_chain_equals_the_host_driven_chain(detected):
    from singleshotpose_amd.utils_multi import detect_multi_batched
    case, head, boxes, source, key = detected['edge']
    meshes, Kc = D.meshes_for(range(case.nC))
    p = detect_multi_batched(head, case.conf_thresh, case.nC, K, D.ANCHORS, case.nA, meshes, Kc, 640, 480)
    want = [(b, c) for b in range(case.B) for c in range(case.nC) if source[b, c] != 0]
    assert len(want) == 3 * 13 and list(zip(p.image.tolist(), p.cls.tolist())) == want
    assert np.array_equal(p.source, source[p.image, p.cls]) and np.array_equal(p.key, key[p.image, p.cls])
    assert np.array_equal(p.det_conf, boxes[p.image, p.cls, 2 * K]) and p.det_conf.dtype == np.float32
    assert np.array_equal(p.cls_conf, boxes[p.image, p.cls, 2 * K + 1])
    denorm = boxes[p.image, p.cls, :2 * K].reshape(-1, K, 2) * np.float32([640, 480])
    assert p.corners2D_pr.dtype == np.float32 and np.array_equal(p.corners2D_pr, denorm)
    R, t = _host_poses(meshes, Kc, p.corners2D_pr, p.cls)
    for got, ref in ((p.R_pr, R), (p.t_pr, t)):
        assert got.shape == ref.shape and got.dtype == np.float64
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    assert np.all(np.isfinite(p.R_pr[p.source == 1])) and np.all(np.isfinite(p.t_pr[p.source == 1]))
    # a subset in another order, with the meshes of those classes only: the same poses
    sub = [9, 1, 4]
    q = detect_multi_batched(head, case.conf_thresh, case.nC, K, D.ANCHORS, case.nA, {c: meshes[c] for c in sub}, Kc, 640,
                             480, classes=sub)
    assert q.cls.tolist() == sub * 3 and q.image.tolist() == [0] * 3 + [1] * 3 + [2] * 3
    for i, (b, c) in enumerate(zip(q.image, q.cls)):
        j = want.index((b, c))
        assert np.array_equal(q.R_pr[i], p.R_pr[j]) and np.array_equal(q.t_pr[i], p.t_pr[j])
        assert np.array_equal(q.corners2D_pr[i], p.corners2D_pr[j])


def test_pose_chain_equals_the_validators_on_a_labelled_case(detected):
    from singleshotpose_amd.utils_multi import detect_multi_batched, evaluate_multi_batched
    case, head = detected['chain'][:2]
    ev = evaluate_multi_batched(head, torch.from_numpy(case.target.reshape(case.B, -1)), case.conf_thresh, case.nC, K,
                                D.ANCHORS, case.nA, case.vertices, case.intrinsics, 640, 480)
    p = detect_multi_batched(head, case.conf_thresh, case.nC, K, D.ANCHORS, case.nA,
                             {c: case.vertices for c in range(case.nC)}, case.intrinsics, 640, 480)
    where = {(b, c): i for i, (b, c) in enumerate(zip(p.image.tolist(), p.cls.tolist()))}
    assert len(ev.image) == 7
    for i, (b, c) in enumerate(zip(ev.image.tolist(), ev.cls.tolist())):
        j = where[(b, c)]
        assert np.array_equal(ev.corners2D_pr[i], p.corners2D_pr[j]) and ev.source[i] == p.source[j]
        np.testing.assert_allclose(p.R_pr[j], ev.R_pr[i], rtol=1e-12, atol=0)
        np.testing.assert_allclose(p.t_pr[j], ev.t_pr[i], rtol=1e-12, atol=0)


def test_per_image_intrinsics_and_fallback_handling(detected):
    from singleshotpose_amd.utils_multi import detect_multi_batched
    case, head, boxes, source, key = detected['edge']
    meshes, K1 = D.meshes_for(range(case.nC))
    K2 = K1.copy()
    K2[0, 0] *= 1.25
    K2[1, 1] *= 1.2
    K2[0, 2] += 11.0
    args = (case.conf_thresh, case.nC, K, D.ANCHORS, case.nA, meshes)
    one, two = (detect_multi_batched(head, *args, Kc, 640, 480) for Kc in (K1, K2))
    mixed = detect_multi_batched(head, *args, np.stack([K1, K2, K2, K1]), 640, 480)
    assert np.array_equal(mixed.image, one.image) and np.array_equal(mixed.cls, one.cls)
    first = np.isin(mixed.image, [0, 3])
    assert first.any() and (~first).any()
    for name in ('R_pr', 't_pr'):
        got, a, b = getattr(mixed, name), getattr(one, name), getattr(two, name)
        assert np.array_equal(got[first], a[first], equal_nan=True) and np.array_equal(got[~first], b[~first], equal_nan=True)
    assert not np.array_equal(one.t_pr[one.source == 1], two.t_pr[two.source == 1])
    assert 3 not in one.image and set(one.image.tolist()) == {0, 1, 2}            # the NaN image never appears
    kept = detect_multi_batched(head, *args, K1, 640, 480, keep_fallback=False)
    sel = one.source != 2
    assert sel.sum() == (source == 1).sum() >= 5 and np.all(kept.source == 1) and 1 not in kept.image
    for name in one._fields:
        assert np.array_equal(getattr(kept, name), getattr(one, name)[sel]), name
    # only the NaN image: nothing survives, the shapes stay
    none = detect_multi_batched(head[3:4], *args, K1, 640, 480)
    assert len(none.image) == 0 and none.corners2D_pr.shape == (0, K, 2) and none.R_pr.shape == (0, 3, 3)
    assert none.t_pr.shape == (0, 3, 1)


@pytest.mark.parametrize('B,classes', [(1, [6]), (4, None)])
def test_one_detect_launch_and_one_pnp_launch(detected, monkeypatch, B, classes):
    from singleshotpose_amd import _lib
    from singleshotpose_amd.utils_multi import detect_multi_batched
    case, head = detected['edge'][:2]
    meshes, Kc = D.meshes_for(range(case.nC))
    calls, real = [], _lib.call

    def recording(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recording)
    p = detect_multi_batched(head[2:2 + B] if B == 1 else head, case.conf_thresh, case.nC, K, D.ANCHORS, case.nA, meshes,
                             Kc, 640, 480, classes=classes)
    assert calls == ['ssp_region_detect_multi', 'ssp_pnp_batched']
    assert len(p.image) == (1 if B == 1 else 39)

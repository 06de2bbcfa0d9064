"""The host half of the multi-object augmentation (singleshotpose_amd.image.draw_multi_augmentation and the drop-in
dataset_multi / image_multi modules) against tests/golden/multi_aug.json: what the reference's image_multi.py +
dataset_multi.py drew, decided and labelled over the same fixture (tools/gen_multi_aug_golden.py).  No GPU."""
import hashlib
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

from helpers import GOLD, ROOT

GOLDEN = json.load(open(os.path.join(GOLD, 'multi_aug.json')))
ARRAYS = np.load(os.path.join(GOLD, 'multi_aug.npz'))
JITTER, HUE, SAT, EXP = GOLDEN['_meta']['jitter_hue_saturation_exposure']
SHIMS = [os.path.join(ROOT, 'dropin', 'multi_obj_pose_estimation'), os.path.join(ROOT, 'dropin')]


@pytest.fixture(scope='module')
def fixture_cwd(tmp_path_factory):
    import fixture_occlusion as fo
    info = fo.make(str(tmp_path_factory.mktemp('occlusion') / 'fixture'))
    return info['cwd']


@pytest.fixture()
def dropin_modules(monkeypatch):
    for p in reversed(SHIMS):
        monkeypatch.syspath_prepend(p)
    for m in ('dataset', 'dataset_multi', 'image_multi', 'utils', 'utils_multi'):
        monkeypatch.delitem(sys.modules, m, raising=False)
    import dataset_multi
    import image_multi
    assert os.path.dirname(dataset_multi.__file__) == SHIMS[0] and os.path.dirname(image_multi.__file__) == SHIMS[0]
    yield dataset_multi, image_multi
    for m in ('dataset', 'dataset_multi', 'image_multi', 'utils', 'utils_multi'):
        sys.modules.pop(m, None)


def _label(rows):
    """The golden (8, 21) rows as the full max_num_gt * 21 vector (the generator asserted that the other rows are zero)."""
    full = np.zeros((50, 21))
    full[:8] = rows
    return full.reshape(-1)


@pytest.mark.parametrize('index', range(len(GOLDEN['direct'])), ids=lambda i: 'seed%d' % GOLDEN['direct'][i]['seed'])
def test_draws_decisions_labels_and_random_state_are_the_references(fixture_cwd, monkeypatch, index):
    case = GOLDEN['direct'][index]
    from singleshotpose_amd.image import draw_multi_augmentation
    monkeypatch.chdir(fixture_cwd)
    random.seed(case['seed'])
    rec = draw_multi_augmentation(case['image'], tuple(case['shape']), JITTER, HUE, SAT, EXP, 9, 50)
    assert [o['name'] for o in rec['objs']] == case['order']                 # shuffle(add_objs)
    assert rec['draws'] == case['draws']                                     # every drawn integer, in order
    assert rec['tries'] == case['tries']                                     # accept / reject decisions per object
    assert len(rec['draws']) == 7 + 6 * sum(case['tries'])
    assert rec['label'].dtype == np.float64
    assert rec['label'].tobytes() == _label(ARRAYS['label_%d' % index]).tobytes()      # the same double arithmetic: bit for bit
    assert hashlib.sha256(rec['total_mask'].tobytes()).hexdigest() == case['mask_sha256']
    assert random.random().hex() == case['next_random']                     # the stream is where the reference left it
    for o in rec['objs']:
        assert o['mask_sized'].shape == (case['shape'][1], case['shape'][0], 3) and o['mask'].dtype == np.uint8


def test_golden_covers_the_paths_that_matter():
    cov = GOLDEN['_meta']['coverage']
    assert cov['retry'] and cov['nonbinary'] and cov['over255']
    assert cov['scene_flip'] == [0, 1] and cov['obj_flip'] == [0, 1]
    assert cov['shift_x'] == [-1, 1] and cov['shift_y'] == [-1, 1]
    assert cov['outside'] == ['bottom', 'left', 'right', 'top']
    assert any(max(c['tries']) > 1 for c in GOLDEN['direct'])


def test_superimpose_masks_is_the_references_for_every_byte_pair():
    """ImageMath's int32 `mask + total * round(1 - mask / 255)` followed by convert('L'): the golden table holds the
    reference's result for all 256 x 256 (mask, total) pairs - sums above 255 come back as 255."""
    from singleshotpose_amd.image import superimpose_masks_u8
    z = np.load(os.path.join(GOLD, 'multi_aug.npz'))
    m, t = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    assert np.array_equal(superimpose_masks_u8(m, t), z['superimpose_masks'])
    assert z['superimpose_masks'][127, 200] == 255 and z['superimpose_masks'][100, 100] == 200
    # the three selects (superimpose_masked_imgs, mask_background, change_background; a = 200, b = 100): pos = mask >= 128
    ramp = np.arange(256)
    assert np.array_equal(z['select'][0], np.where(ramp >= 128, 200, 100))
    assert np.array_equal(z['select'][1], np.where(ramp >= 128, 200, 0))
    assert np.array_equal(z['select'][2], np.where(ramp >= 128, 200, 100))


def test_get_add_objs_for_all_13_objects_and_the_unknown_one():
    from singleshotpose_amd.image import get_add_objs
    want = {
        'ape': 'can cat duck glue holepuncher iron phone', 'benchvise': 'ape can cat driller duck glue holepuncher',
        'cam': 'ape benchvise can cat driller duck holepuncher', 'can': 'ape benchvise cat driller duck eggbox holepuncher',
        'cat': 'ape can duck glue holepuncher eggbox phone', 'driller': 'ape benchvise can cat duck glue holepuncher',
        'duck': 'ape can cat eggbox glue holepuncher phone', 'eggbox': 'ape benchvise cam can cat duck glue holepuncher',
        'glue': 'ape benchvise cam driller duck eggbox holepuncher', 'holepuncher': 'benchvise cam can cat driller duck eggbox',
        'iron': 'ape benchvise can cat driller duck glue', 'lamp': 'ape benchvise can driller eggbox holepuncher iron',
        'phone': 'ape benchvise cam can driller duck holepuncher'}
    assert len(want) == 13
    for k, v in want.items():
        got = get_add_objs(k)
        assert got == v.split()
        got.append('x')
        assert get_add_objs(k) == v.split()          # a fresh list every call: the caller shuffles it in place
    with pytest.raises(ValueError, match='bowl'):
        get_add_objs('bowl')


def test_dropin_modules_expose_the_references_names(dropin_modules):
    dataset_multi, image_multi = dropin_modules
    for n in ('get_add_objs', 'rand_scale', 'fill_truth_detection', 'load_data_detection', 'augment_objects',
              'mask_background', 'superimpose_masked_imgs', 'superimpose_masks'):
        assert callable(getattr(image_multi, n)), n
    with pytest.raises(ValueError, match='bowl'):
        image_multi.get_add_objs('bowl')
    random.seed(3)
    a = image_multi.rand_scale(1.5)
    random.seed(3)
    s = random.uniform(1, 1.5)
    assert a == (s if random.randint(1, 10000) % 2 else 1. / s)


def test_fill_truth_detection_recomputes_width_and_height(dropin_modules):
    _, image_multi = dropin_modules
    row = np.concatenate([[4.0], np.linspace(0.2, 0.8, 18), [9.0, 9.0]])
    lab = image_multi.fill_truth_detection(row[None], 640, 480, 1, 0.05, -0.02, 1.1, 0.9, 9, 50).reshape(50, 21)
    xs, ys = lab[0, 1:19:2], lab[0, 2:19:2]
    assert lab[0, 19] == xs.max() - xs.min() and lab[0, 20] == ys.max() - ys.min() and lab[0, 0] == 4.0
    assert not lab[1:].any()


def test_multiscale_widths_follow_the_references_schedule(dropin_modules):
    dataset_multi, _ = dropin_modules
    assert len(GOLDEN['widths']) == 5
    for w in GOLDEN['widths']:
        random.seed(w['seed'])
        got = [dataset_multi.multiscale_width(w['seen'], w['nbatches'], w['batch_size']) * 32 for _ in w['widths']]
        assert got == w['widths']
    assert set(GOLDEN['widths'][0]['widths']) == {416} and len(set(GOLDEN['widths'][4]['widths'])) > 3


def test_listdataset_keeps_the_references_constructor_and_refuses_other_transforms(dropin_modules, fixture_cwd, monkeypatch):
    dataset_multi, _ = dropin_modules
    monkeypatch.chdir(fixture_cwd)
    random.seed(2)
    ds = dataset_multi.listDataset('cfg/train_occlusion.txt', shape=(416, 416), shuffle=True, train=True, seen=8, batch_size=4,
                                   num_workers=2, bg_file_names=['../VOCdevkit/VOC2012/JPEGImages/bg0.png'])
    random.seed(2)
    lines = open('cfg/train_occlusion.txt').readlines()
    random.shuffle(lines)
    assert ds.lines == lines and (ds.nSamples, ds.nbatches, ds.objclass, ds.cell_size, ds.max_num_gt) == (8, 2, None, 32, 50)
    with pytest.raises(TypeError, match='ToTensor'):
        dataset_multi.listDataset('cfg/train_occlusion.txt', train=True, transform=lambda x: x)
    # the host half of __getitem__ needs no GPU: the sample carries the record, the label is the reference's
    ep = GOLDEN['epochs']['fixed_416']
    random.seed(ep['seed'])
    ds = dataset_multi.listDataset('cfg/train_occlusion.txt', shape=(416, 416), shuffle=True, train=True, seen=ep['seen'],
                                   batch_size=ep['batch'], num_workers=0, bg_file_names=['../VOCdevkit/VOC2012/JPEGImages/bg0.png'])
    sample, label = ds[0]
    assert type(sample).__name__ == 'RawMultiSample' and sample.shape == (416, 416)
    assert label.dtype == torch.float64 and label.numpy().tobytes() == _label(ARRAYS['epoch_fixed_416'][0, 0]).tobytes()
    assert ds.seen == ep['seen'] + 0
    # train=False: the objclass / labels_occlusion rule of dataset_multi.py:78
    test_list = '../LINEMOD/ape/test_occlusion.txt'
    dv = dataset_multi.listDataset(test_list, shape=(64, 64), shuffle=False, objclass='ape', train=False)
    img, lab = dv[0]
    first = open(test_list).readline().rstrip()
    want = np.loadtxt(first.replace('benchvise', 'ape').replace('JPEGImages', 'labels_occlusion').replace('.png', '.txt'))
    assert img.size == (64, 64) and np.allclose(lab.numpy()[:19], want[:19]) and not lab.numpy()[21:].any()

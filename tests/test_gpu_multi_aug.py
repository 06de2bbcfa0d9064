"""The multi-object training augmentation on the MI355X (csrc/image_aug.hip: masked-source and moved-destination resample
epilogues, the layer compositor; singleshotpose_amd.image.DeviceAugmenter.load_multi_data_detection_batch; the drop-in
dataset_multi / image_multi modules).  Every comparison is byte equality: against numpy / Pillow statements of the
semantics written here, and against tests/golden/multi_aug.{json,npz} - the reference's image_multi.py + dataset_multi.py
run over the same fixture (tools/gen_multi_aug_golden.py)."""
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GOLD, ROOT

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(GOLD, 'multi_aug.json')))
JITTER, HUE, SAT, EXP = GOLDEN['_meta']['jitter_hue_saturation_exposure']
SHIMS = [os.path.join(ROOT, 'dropin', 'multi_obj_pose_estimation'), ROOT, os.path.join(ROOT, 'dropin')]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope='module')
def fixture_cwd(tmp_path_factory):
    import fixture_occlusion as fo
    return fo.make(str(tmp_path_factory.mktemp('occlusion') / 'fixture'))['cwd']


# ------------------------------------------------------------------------------------------------ kernel pieces
def _resample_once(src, pass_, epi, out_hw, n_in, mask=None, x0=0, y0=0, flip=0):
    """One ssp_resample_u8 launch on one image with IDENTITY coefficients over `n_in` taps' axis (a pass whose size does not
    change): what is left is the epilogue under test."""
    from singleshotpose_amd import _lib
    from singleshotpose_amd.image import _DESC_DTYPE, resample_coeffs
    dev = torch.device('cuda')
    s = torch.from_numpy(src).to(dev)
    m = None if mask is None else torch.from_numpy(mask).to(dev)
    oh, ow = out_hw
    out = torch.full((oh, ow, 3), 7, dtype=torch.uint8, device=dev)
    ks, bnd, kk = resample_coeffs([n_in], n_in)
    tb, tk = torch.from_numpy(bnd[0].copy()).to(dev), torch.from_numpy(kk[0].copy()).to(dev)
    d = np.zeros(1, _DESC_DTYPE)
    d['src'], d['dst'], d['bounds'], d['kk'], d['ksize'] = s.data_ptr(), out.data_ptr(), tb.data_ptr(), tk.data_ptr(), ks
    d['mask'] = 0 if m is None else m.data_ptr()
    d['src_w'], d['src_h'], d['src_pitch'] = src.shape[1], src.shape[0], src.shape[1] * 3
    d['dst_w'], d['dst_h'], d['dst_pitch'] = ow, oh, ow * 3
    d['x0'], d['y0'], d['reserved'] = x0, y0, flip
    dd = torch.from_numpy(d.view(np.uint8).copy()).to(dev)
    _lib.call('ssp_resample_u8', dd.data_ptr(), 1, pass_, epi, oh * ow, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_masked_source_reads_img_times_rounded_mask_with_zero_fill_outside():
    """mask_background (image_multi.py:38-50) as the source side of the horizontal pass: a crop window reaching outside
    the image on every side, a mask with every byte value."""
    rs = np.random.RandomState(1)
    h, w = 37, 53
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    mask = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    mask[:3, :, :] = np.arange(w * 3).reshape(w, 3)[None] + 100          # 127 / 128 next to each other
    x0, y0, cw, ch = -5, -4, w + 11, h + 9
    want = np.zeros((ch, cw, 3), np.uint8)
    want[-y0:-y0 + h, -x0:-x0 + w] = img * np.round(mask / 255.0).astype(np.uint8)          # Image.crop fills with zeros
    assert np.array_equal(np.round(mask / 255.0), mask >= 128)
    got = _resample_once(img, 0, 3, (ch, cw), cw, mask=mask, x0=x0, y0=y0)
    assert np.array_equal(got, want)
    # without a mask the same launch reads the image plainly (the scene and the background layers)
    want[-y0:-y0 + h, -x0:-x0 + w] = img
    assert np.array_equal(_resample_once(img, 0, 3, (ch, cw), cw, x0=x0, y0=y0), want)


@pytest.mark.parametrize('sx,sy,flip', [(0, 0, 0), (5, -7, 0), (-80, 80, 1), (47, 29, 1), (-1, -1, 0), (-48, -30, 1)])
def test_vertical_pass_stores_at_the_offset_and_flip_position(sx, sy, flip):
    """ImageChops.offset(shift_x, shift_y) (wrap-around) then FLIP_LEFT_RIGHT, image_multi.py:218-223, as the store index."""
    from PIL import Image, ImageChops
    rs = np.random.RandomState(2)
    h, w = 30, 48
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    want = ImageChops.offset(Image.fromarray(img), sx, sy)
    if flip:
        want = want.transpose(Image.FLIP_LEFT_RIGHT)
    rolled = np.roll(img, (sy, sx), (0, 1))
    assert np.array_equal(np.asarray(want), rolled[:, ::-1] if flip else rolled)
    got = _resample_once(img, 1, 4, (h, w), h, x0=sx % w, y0=sy % h, flip=flip)
    assert np.array_equal(got, np.asarray(want))


@pytest.mark.parametrize('nobj', [0, 7, 8])
@pytest.mark.parametrize('shape', [(32, 32, 3), (17, 13, 3)])
def test_compositor_equals_the_layer_by_layer_statement(nobj, shape):
    """augment_objects + change_background per byte with non-binary masks (bicubic mask edges): sums above 255 clip
    (tests/golden/multi_aug.npz: superimpose_masks), every a * pos + b * neg is a select at mask >= 128."""
    from singleshotpose_amd.image import composite_u8
    rs = np.random.RandomState(10 + nobj)
    rnd = lambda: rs.randint(0, 256, shape).astype(np.uint8)
    soft = lambda: np.clip(rs.randint(-300, 556, shape), 0, 255).astype(np.uint8)          # many 0 / 255, every value between
    scene, sm, bg = rnd(), soft(), rnd()
    objs, masks = [rnd() for _ in range(nobj)], [soft() for _ in range(nobj)]
    table = np.load(os.path.join(GOLD, 'multi_aug.npz'))['superimpose_masks']
    total, tmask = scene * (sm >= 128), sm.copy()
    for o, m in zip(objs, masks):
        tmask = table[m, tmask]                                            # the reference's own result for this byte pair
        total = np.where(m >= 128, o, total)
    total = np.where(sm >= 128, scene, total)
    want = np.where(tmask >= 128, total, bg).astype(np.uint8)
    cu = lambda a: torch.from_numpy(a).cuda()
    got = composite_u8(cu(scene), cu(sm), cu(bg), [cu(o) for o in objs], [cu(m) for m in masks]).cpu().numpy()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the whole chain
def _record(case):
    from singleshotpose_amd.image import draw_multi_augmentation
    from PIL import Image
    rgb = lambda p: np.array(Image.open(p).convert('RGB'), dtype=np.uint8)
    random.seed(case['seed'])
    rec = draw_multi_augmentation(case['image'], tuple(case['shape']), JITTER, HUE, SAT, EXP, 9, 50)
    assert rec['draws'] == case['draws'] and rec['tries'] == case['tries']
    rec['img'], rec['bg'] = rgb(case['image']), rgb('../VOCdevkit/VOC2012/JPEGImages/bg0.png')
    for o in rec['objs']:
        o['img'] = rgb(o['path'])
    return rec


def test_whole_chain_gives_the_references_bytes(fixture_cwd, monkeypatch):
    """Every golden case (a retry, both flips, wrapping shifts in both directions, crop boxes outside the image on every
    side, non-binary masks, mask sums above 255; square and non-square network shapes): one batch per shape."""
    from singleshotpose_amd.image import DeviceAugmenter
    monkeypatch.chdir(fixture_cwd)
    aug = DeviceAugmenter()
    full = np.load(os.path.join(GOLD, 'multi_aug.npz'))
    by_shape = {}
    for i, c in enumerate(GOLDEN['direct']):
        by_shape.setdefault(tuple(c['shape']), []).append((i, c))
    assert len(by_shape) >= 4 and max(len(v) for v in by_shape.values()) >= 8
    for shape, cases in by_shape.items():
        recs = [_record(c) for _, c in cases]
        out, lab = aug.load_multi_data_detection_batch(recs, shape)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (len(cases), shape[1], shape[0], 3) and out.is_cuda
        out = out.cpu().numpy()
        for k, (i, c) in enumerate(cases):
            if 'u8_%d' % i in full.files:
                want = full['u8_%d' % i]
                assert np.array_equal(out[k], want), "case %d: %d bytes differ" % (i, int((out[k] != want).sum()))
                assert np.array_equal(recs[k]['total_mask'], full['mask_%d' % i])
            assert _sha(out[k]) == c['sha256'], "case %d (seed %d)" % (i, c['seed'])
            want = np.zeros((50, 21))
            want[:8] = full['label_%d' % i]
            assert lab[k].numpy().tobytes() == want.tobytes()
    assert sum('u8_%d' % i in full.files for i in range(len(GOLDEN['direct']))) >= 2


def _pillow_chain(rec):
    """The image half of image_multi.py:299-382 with Pillow, for records that did not come from files."""
    from PIL import Image, ImageChops
    from singleshotpose_amd.image import _crop_geometry, superimpose_masks_u8
    shape = rec['shape']

    def layer(img, mask, d, shift=None):
        a = img if mask is None else img * (mask >= 128)
        x = Image.fromarray(a.astype(np.uint8)).crop(_crop_geometry(d)[0]).resize(shape)
        if shift:
            x = ImageChops.offset(x, *shift)
        return np.asarray(x.transpose(Image.FLIP_LEFT_RIGHT) if d['flip'] else x)
    sc = layer(rec['img'], None, rec['scene'], (rec['scene']['shift_x'], rec['scene']['shift_y']))
    sm = rec['scene_mask']
    total, tmask = np.where(sm >= 128, sc, 0), sm
    for o in rec['objs']:
        tmask = superimpose_masks_u8(o['mask_sized'], tmask)
        total = np.where(o['mask_sized'] >= 128, layer(o['img'], o['mask'], o), total)
    total = np.where(sm >= 128, sc, total)
    bg = np.asarray(Image.fromarray(rec['bg']).resize(shape))
    return np.where(tmask >= 128, total, bg).astype(np.uint8)


def _synthetic_record(rs, shape, size, nobj, bg_size):
    from PIL import Image, ImageChops
    from singleshotpose_amd.image import _crop_geometry, _draw_crop
    rng = random.Random(int(rs.randint(1 << 30)))

    def blob_mask(w, h):
        yy, xx = np.mgrid[0:h, 0:w]
        cx, cy, r = rs.uniform(0.2, 0.8) * w, rs.uniform(0.2, 0.8) * h, rs.uniform(0.1, 0.3) * min(w, h)
        m = np.clip(255 * (1.5 - np.hypot(xx - cx, yy - cy) / r), 0, 255).astype(np.uint8)          # a soft edge: not 0 / 255
        return np.stack([m, m, np.roll(m, 2, 1)], -1)                                              # channels differ

    def sized(mask, d, shift=None):
        x = Image.fromarray(mask).crop(_crop_geometry(d)[0]).resize(shape)
        if shift:
            x = ImageChops.offset(x, *shift)
        return np.array(x.transpose(Image.FLIP_LEFT_RIGHT) if d['flip'] else x, dtype=np.uint8)
    w, h = size
    sc = _draw_crop(w, h, 0.1, rng)
    sc['shift_x'], sc['shift_y'] = rng.randint(-80, 80), rng.randint(-80, 80)
    rec = dict(shape=shape, scene=sc, img=rs.randint(0, 256, (h, w, 3)).astype(np.uint8),
               scene_mask=sized(blob_mask(w, h), sc, (sc['shift_x'], sc['shift_y'])),
               bg=rs.randint(0, 256, (bg_size[1], bg_size[0], 3)).astype(np.uint8), objs=[], label=np.zeros(50 * 21))
    for k in range(nobj):
        ow, oh = int(rs.randint(90, 400)), int(rs.randint(90, 300))
        d = _draw_crop(ow, oh, 0.1, rng)
        m = blob_mask(ow, oh)
        d.update(img=rs.randint(0, 256, (oh, ow, 3)).astype(np.uint8), mask=m, mask_sized=sized(m, d))
        rec['objs'].append(d)
    return rec


@pytest.mark.parametrize('shape', [(160, 160), (96, 136), (50, 34)])
def test_mixed_size_batch_equals_pillow_sample_by_sample(shape):
    """Scenes, objects and backgrounds of different sizes (up- and down-scaling in one launch), 7 and 8 objects and one
    sample without any in one batch, soft masks whose channels differ; (50, 34): a layer that is not a multiple of 16 bytes."""
    from singleshotpose_amd.image import DeviceAugmenter
    rs = np.random.RandomState(shape[0])
    recs = [_synthetic_record(rs, shape, (640, 480), 7, (500, 375)), _synthetic_record(rs, shape, (120, 90), 8, (64, 200)),
            _synthetic_record(rs, shape, (333, 517), 0, (700, 90)), _synthetic_record(rs, shape, (200, 200), 8, (160, 160))]
    out, _ = DeviceAugmenter().load_multi_data_detection_batch(recs, shape)
    out = out.cpu().numpy()
    for k, r in enumerate(recs):
        want = _pillow_chain(r)
        assert np.array_equal(out[k], want), "sample %d: %d bytes differ" % (k, int((out[k] != want).sum()))
    # resident CUDA tensors in place of host arrays give the same batch
    for r in recs:
        for d in [r] + r['objs']:
            for key in ('img', 'bg', 'mask', 'mask_sized', 'scene_mask'):
                if key in d:
                    d[key] = torch.from_numpy(d[key]).cuda()
    out2, _ = DeviceAugmenter().load_multi_data_detection_batch(recs, shape)
    assert np.array_equal(out2.cpu().numpy(), out)


# ------------------------------------------------------------------------------------------------ the drop-in surface
def _run(cmd, cwd, timeout=900):
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join(SHIMS)
    env['PYTHONUNBUFFERED'] = '1'
    env.pop('SSP_DATASET_FLOAT', None)
    p = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


@pytest.mark.parametrize('name', sorted(GOLDEN['epochs']))
def test_dropin_dataset_multi_epoch_is_the_reference_epoch_byte_for_byte(tmp_path, name):
    """dropin dataset_multi.listDataset inside a DataLoader with `data.cuda()`, as train_multi.py:49-74 has it
    (tools/dump_dataset_epoch.py --multi), over a seeded epoch: the SHA-256 of every batch and the labels are the
    reference pipeline's."""
    import fixture_occlusion as fo
    gold = GOLDEN['epochs'][name]
    root = str(tmp_path / 'fixture')
    fo.make(root)
    out = str(tmp_path / 'dropin.npz')
    _run([sys.executable, os.path.join(ROOT, 'tools', 'dump_dataset_epoch.py'), root, out, '--multi', '--seed', str(gold['seed']),
          '--seen', str(gold['seen']), '--batch', str(gold['batch'])], str(tmp_path))
    got = np.load(out)
    assert str(got['module']) == os.path.join(SHIMS[0], 'dataset_multi.py')
    assert len(gold['batches']) == 2
    for i, b in enumerate(gold['batches']):
        u8 = got['u8_%d' % i]
        assert list(u8.shape) == b['shape'] and u8.dtype == np.uint8
        assert _sha(u8) == b['sha256'], "batch %d" % i
        lab = got['lab_%d' % i]
        assert lab.dtype == np.float64 and lab.shape == (gold['batch'], 50 * 21)
        rows = lab.reshape(gold['batch'], 50, 21)
        assert rows[:, :8].tobytes() == np.load(os.path.join(GOLD, 'multi_aug.npz'))['epoch_' + name][i].tobytes()
        assert not rows[:, 8:].any()


_BATCH_PROBE = r'''
import os, random, sys
import numpy as np, torch
from torchvision import transforms
import dataset_multi, image_multi
random.seed(5); torch.manual_seed(5)
ds = dataset_multi.listDataset('cfg/train_occlusion.txt', shape=(416, 416), shuffle=False, transform=transforms.Compose([transforms.ToTensor()]),
                               train=True, seen=0, batch_size=4, num_workers=2, bg_file_names=['../VOCdevkit/VOC2012/JPEGImages/bg0.png'])
data, target = next(iter(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=2, pin_memory=True)))
assert type(data).__name__ == 'RawMultiBatch' and data.blob.is_pinned() and len(data) == 4
assert target.dtype == torch.float64 and tuple(target.shape) == (4, 50 * 21)
a = data.cuda()
b = data.to('cuda')
c = data.to(device=torch.device('cuda', 0))
assert a.dtype == torch.uint8 and tuple(a.shape) == (4, 416, 416, 3) == data.size() and torch.equal(a, b) and torch.equal(a, c)
os.environ['SSP_DATASET_FLOAT'] = '1'
f = data.cuda()
assert f.dtype == torch.float32 and tuple(f.shape) == (4, 3, 416, 416)
assert torch.equal(f, a.permute(0, 3, 1, 2).float().div(255))          # ToTensor's layout and arithmetic
del os.environ['SSP_DATASET_FLOAT']
try:
    data.to('cpu'); raise SystemExit('RawMultiBatch.to(cpu) must refuse')
except RuntimeError as e:
    assert 'no CPU fallback' in str(e)
try:
    data.mean(); raise SystemExit('RawMultiBatch must not behave like a tensor')
except AttributeError as e:
    assert 'no CPU fallback' in str(e)
# the per-sample names: load_data_detection = augment_objects + change_background, same stream
import hashlib, json
g = json.load(open(sys.argv[1]))['direct'][0]
random.seed(g['seed'])
img, label = image_multi.load_data_detection(g['image'], tuple(g['shape']), 0.1, 0.05, 1.5, 1.5, '../VOCdevkit/VOC2012/JPEGImages/bg0.png', 9, 50)
assert hashlib.sha256(np.asarray(img).tobytes()).hexdigest() == g['sha256'] and random.random().hex() == g['next_random']
want = np.zeros((50, 21)); want[:8] = np.load(sys.argv[1][:-5] + '.npz')['label_0']
assert np.asarray(label, dtype=np.float64).tobytes() == want.tobytes()
random.seed(g['seed'])
total, label2, tmask = image_multi.augment_objects(g['image'], 'benchvise', image_multi.get_add_objs('benchvise'), tuple(g['shape']), 0.1, 0.05, 1.5, 1.5, 9, 50)
assert hashlib.sha256(np.asarray(tmask).tobytes()).hexdigest() == g['mask_sha256'] and np.array_equal(label, label2)
from PIL import Image
black = np.asarray(image_multi.mask_background(img, tmask))
assert np.array_equal(black, np.asarray(img) * (np.asarray(tmask) >= 128))
assert np.array_equal(np.asarray(total), black)
back = image_multi.superimpose_masked_imgs(total, tmask, Image.open('../VOCdevkit/VOC2012/JPEGImages/bg0.png').convert('RGB').resize(img.size))
assert np.array_equal(np.asarray(back), np.asarray(img))
print('PROBE_OK', float(a.float().mean()))
'''


def test_rawmultibatch_device_entry_points_float_mode_and_per_sample_names(tmp_path):
    """Through a DataLoader with two workers and pin_memory: RawMultiBatch.cuda() / .to('cuda') / .to(device=...) give one
    uint8 batch; SSP_DATASET_FLOAT=1 returns ToTensor's float batch of the same bytes; .to('cpu') and tensor methods refuse;
    dropin image_multi's per-sample functions give the golden bytes."""
    import fixture_occlusion as fo
    info = fo.make(str(tmp_path / 'fixture'))
    out = _run([sys.executable, '-c', _BATCH_PROBE, os.path.join(GOLD, 'multi_aug.json')], info['cwd'])
    assert 'PROBE_OK' in out, out[-2000:]

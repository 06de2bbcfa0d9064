"""Writes tests/golden/multi_aug.json and multi_aug.npz: the reference's multi-object augmentation
(multi_obj_pose_estimation/image_multi.py + dataset_multi.py, imported unmodified and read-only) run over the synthetic
OCCLUSION-shaped dataset of tests/fixture_occlusion.make().

Build machine only (the reference is not on the GPU machines); only the results it writes are committed.  One environment
patch, as oracle/gen_image_golden.py has it: Pillow >= 12 renamed ImageMath.eval to ImageMath.unsafe_eval.  The draws are
recorded by wrapping random.randint / random.shuffle and two functions of the imported module while a sample runs; the
reference's files are not touched.

multi_aug.json
  direct   load_data_detection(imgpath, shape, 0.1, 0.05, 1.5, 1.5, bg, 9, 50) after random.seed(seed), per case: seed,
           image, shape, the shuffled object order, the drawn integers (flip draws reduced mod 2), candidates tried per
           object, SHA-256 of the output bytes and of the total mask, and the next
           random.random() of the stream
  epochs   dataset_multi.listDataset(train=True) inside a DataLoader, as train_multi.py:49-56 builds it, for a seeded
           epoch: per batch the shape and SHA-256 of the (B, H, W, 3) bytes
  widths   the multi-scale widths of a seeded walk over the five `seen` stages
multi_aug.npz
  u8_<i>, mask_<i>   full output and total-mask bytes of the first cases
  label_<i>          the 8 label rows (8, 21) float64 of direct case i (the other 42 rows are zero: asserted here)
  epoch_<name>       the label rows of a seeded epoch, (batches, B, 8, 21) float64
  superimpose_masks  the reference's superimpose_masks over all 256 x 256 (mask, total) byte pairs: what ImageMath's
                     int32 sum + convert('L') does with values above 255
  select             superimpose_masked_imgs / mask_background / change_background over all 256 mask bytes

    python tools/gen_multi_aug_golden.py [--time]
"""
import hashlib
import io
import json
import os
import random
import sys
import tempfile
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference/multi_obj_pose_estimation'
sys.path[:0] = [REF, os.path.join(ROOT, 'dropin', 'multi_obj_pose_estimation'), ROOT, os.path.join(ROOT, 'dropin'),
                os.path.join(ROOT, 'tests')]

JITTER, HUE, SAT, EXP = 0.1, 0.05, 1.5, 1.5
# (seed, train image index, shape); the first N_FULL keep their bytes
DIRECT = [(s, s % 8, (160, 160)) for s in range(10)] + [(20, 1, (224, 160)), (21, 5, (160, 192)), (22, 2, (416, 416))]
N_FULL = 3
EPOCHS = [dict(name='fixed_416', seed=0, seen=0, batch=4), dict(name='multiscale_last_stage', seed=1, seen=1000, batch=4)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def next_random():
    r = random.Random()
    r.setstate(random.getstate())
    return r.random().hex()


class Recorder(object):
    """Wraps random.randint / random.shuffle and the imported module's data_augmentation_with_mask / superimpose_masks
    while one sample runs."""

    def __init__(self, mod):
        self.mod = mod

    def __enter__(self):
        self.ints, self.order, self.cands, self.accepted_at, self.over255 = [], None, 0, [], False
        self.saved = (random.randint, random.shuffle, self.mod.data_augmentation_with_mask, self.mod.superimpose_masks)
        randint, shuffle, aug, sup = self.saved

        def rec_randint(a, b):
            v = randint(a, b)
            self.ints.append(v)
            return v

        def rec_shuffle(x):
            shuffle(x)
            if self.order is None:
                self.order = list(x)

        def rec_aug(*a, **k):
            self.cands += 1
            return aug(*a, **k)

        def rec_sup(mask, total):
            self.accepted_at.append(self.cands)
            m, t = np.array(mask).astype(int), np.array(total).astype(int)
            self.over255 |= bool(((m + np.where(m >= 128, 0, t)) > 255).any())
            return sup(mask, total)
        random.randint, random.shuffle = rec_randint, rec_shuffle
        self.mod.data_augmentation_with_mask, self.mod.superimpose_masks = rec_aug, rec_sup
        return self

    def __exit__(self, *exc):
        random.randint, random.shuffle, self.mod.data_augmentation_with_mask, self.mod.superimpose_masks = self.saved

    def draws(self):
        """The integers in draw order with the flip draws reduced mod 2: 7 for the scene, 6 per candidate."""
        v = list(self.ints)
        assert (len(v) - 7) % 6 == 0 and (len(v) - 7) // 6 == self.cands
        v[4] %= 2
        for c in range(self.cands):
            v[7 + 6 * c + 5] %= 2
        return v

    def tries(self):
        return [b - a for a, b in zip([0] + self.accepted_at[:-1], self.accepted_at)]


def main():
    from PIL import Image, ImageMath
    if not hasattr(ImageMath, 'eval'):
        ImageMath.eval = ImageMath.unsafe_eval
    import image_multi as ref
    import dataset_multi as refds
    assert os.path.dirname(os.path.abspath(ref.__file__)) == REF and os.path.dirname(os.path.abspath(refds.__file__)) == REF
    import torch
    import fixture_occlusion as fo
    import PIL
    torch.set_num_threads(1)
    out = {'_meta': {'generator': 'tools/gen_multi_aug_golden.py', 'fixture': 'tests/fixture_occlusion.py make()',
                     'source': 'multi_obj_pose_estimation/image_multi.py + dataset_multi.py (unmodified)',
                     'pillow': PIL.__version__, 'jitter_hue_saturation_exposure': [JITTER, HUE, SAT, EXP]}}
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        info = fo.make(os.path.join(tmp, 'fixture'))
        os.chdir(info['cwd'])
        lines = [l.rstrip() for l in open('cfg/train_occlusion.txt')]
        bg = '../VOCdevkit/VOC2012/JPEGImages/bg0.png'
        if '--time' in sys.argv:
            random.seed(0)
            t0 = time.perf_counter()
            n = 8
            for i in range(n):
                ref.load_data_detection(lines[i % len(lines)], (416, 416), JITTER, HUE, SAT, EXP, bg, 9, 50)
            print(json.dumps({'reference_load_data_detection_ms_per_sample': round((time.perf_counter() - t0) / n * 1e3, 1),
                              'shape': [416, 416], 'samples': n, 'machine': 'build container, one CPU core'}))
            return
        # ---- direct cases ----
        cov = dict(retry=False, scene_flip=set(), obj_flip=set(), shift_x=set(), shift_y=set(), outside=set(), nonbinary=False,
                   over255=False)
        cases = []
        for i, (seed, idx, shape) in enumerate(DIRECT):
            random.seed(seed)
            with Recorder(ref) as r:
                # augment_objects returns the total mask load_data_detection drops: same stream, same pixels
                objname = os.path.basename(os.path.dirname(os.path.dirname(lines[idx])))
                total, label, tmask = ref.augment_objects(lines[idx], objname, ref.get_add_objs(objname), shape, JITTER, HUE, SAT,
                                                          EXP, 9, 50)
                img = ref.change_background(total, tmask, Image.open(bg).convert('RGB'))
            nxt = next_random()
            random.seed(seed)
            img2, label2 = ref.load_data_detection(lines[idx], shape, JITTER, HUE, SAT, EXP, bg, 9, 50)
            assert np.array_equal(np.array(img), np.array(img2)) and np.array_equal(label, label2) and nxt == next_random()
            u8, mk, d = np.array(img), np.array(tmask), r.draws()
            assert u8.shape == (shape[1], shape[0], 3)
            cases.append(dict(seed=seed, image=lines[idx], shape=list(shape), order=r.order, draws=d, tries=r.tries(),
                              sha256=sha(u8), mask_sha256=sha(mk), next_random=nxt))
            rows = np.asarray(label, np.float64).reshape(50, 21)
            assert rows[:8].any(axis=1).all() and not rows[8:].any()
            arrays['label_%d' % i] = rows[:8].copy()
            if i < N_FULL:
                arrays['u8_%d' % i], arrays['mask_%d' % i] = u8, mk
            cov['retry'] |= max(r.tries()) > 1
            cov['scene_flip'].add(d[4])
            cov['obj_flip'] |= set(d[7 + 6 * c + 5] for c in range(r.cands))
            cov['shift_x'].add(np.sign(d[5]))
            cov['shift_y'].add(np.sign(d[6]))
            for blk in [d[0:4]] + [d[7 + 6 * c + 1:7 + 6 * c + 5] for c in range(r.cands)]:
                cov['outside'] |= set(k for k, v in zip(('left', 'right', 'top', 'bottom'), blk) if v < 0)
            cov['nonbinary'] |= bool(((mk != 0) & (mk != 255)).any())
            cov['over255'] |= r.over255
        assert cov['retry'], "no case rejects a candidate: pick other seeds"
        assert cov['scene_flip'] == {0, 1} and cov['obj_flip'] == {0, 1}, cov
        assert {-1, 1} <= cov['shift_x'] and {-1, 1} <= cov['shift_y'], cov
        assert cov['outside'] == {'left', 'right', 'top', 'bottom'}, cov
        assert cov['nonbinary'], "no mask byte other than 0 / 255"
        out['direct'] = cases
        out['_meta']['coverage'] = {k: (sorted(int(x) if not isinstance(x, str) else x for x in v) if isinstance(v, set) else v)
                                    for k, v in cov.items()}
        # ---- what ImageMath + convert('L') do, byte by byte ----
        m, t = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
        rgb = lambda a: Image.fromarray(np.stack([a, a, a], -1))
        arrays['superimpose_masks'] = np.array(ref.superimpose_masks(rgb(m), rgb(t)))[..., 0]
        assert arrays['superimpose_masks'][127, 255] == 255 and arrays['superimpose_masks'][128, 255] == 128
        ramp = np.arange(256, dtype=np.uint8)[None, :]
        a, b = np.full((1, 256), 200, np.uint8), np.full((1, 256), 100, np.uint8)
        arrays['select'] = np.stack([np.array(ref.superimpose_masked_imgs(rgb(a), rgb(ramp), rgb(b)))[0, :, 0],
                                     np.array(ref.mask_background(rgb(a), rgb(ramp)))[0, :, 0],
                                     np.array(ref.change_background(rgb(a), rgb(ramp), rgb(b)))[0, :, 0]])
        # ---- seeded epochs through the reference's dataset ----
        bgs = ['../VOCdevkit/VOC2012/JPEGImages/bg0.png']
        out['epochs'] = {}
        for ep in EPOCHS:
            random.seed(ep['seed'])
            ds = refds.listDataset('cfg/train_occlusion.txt', shape=(416, 416), shuffle=True, transform=None, train=True,
                                   seen=ep['seen'], batch_size=ep['batch'], num_workers=0, bg_file_names=bgs)
            batches, epoch_labels = [], []
            for b in range(len(ds) // ep['batch']):
                items = [ds[b * ep['batch'] + j] for j in range(ep['batch'])]
                u8 = np.stack([np.array(im) for im, _ in items])
                labs = np.stack([lab.numpy().astype(np.float64).reshape(50, 21) for _, lab in items])
                assert not labs[:, 8:].any()
                epoch_labels.append(labs[:, :8].copy())
                batches.append(dict(shape=list(u8.shape), sha256=sha(u8)))
            arrays['epoch_' + ep['name']] = np.stack(epoch_labels)
            out['epochs'][ep['name']] = dict(seed=ep['seed'], seen=ep['seen'], batch=ep['batch'], batches=batches,
                                             next_random=next_random())
        # ---- the multi-scale schedule ----
        walk = []
        for stage, seen in enumerate((0, 20 * 8, 40 * 8, 60 * 8, 80 * 8)):
            random.seed(100 + stage)
            ds = refds.listDataset('cfg/train_occlusion.txt', shape=(416, 416), shuffle=False, train=False, seen=seen,
                                   batch_size=4, num_workers=0, bg_file_names=bgs, objclass='ape')
            ds.train = True
            ws = []
            for _ in range(12):      # the shape draw of __getitem__ (dataset_multi.py:43-58) alone
                try:
                    ds.bg_file_names = []          # the next statement of the training branch raises: nothing else is drawn
                    ds[0]
                except ValueError:
                    pass
                ws.append(ds.shape[0])
            walk.append(dict(seed=100 + stage, seen=seen, nbatches=ds.nbatches, batch_size=4, widths=ws))
        out['widths'] = walk
    os.chdir(ROOT)
    with open(os.path.join(GOLD, 'multi_aug.json'), 'w') as f:
        one = lambda v: json.dumps(v, sort_keys=True)      # one record per line: the file stays a few dozen lines
        f.write('{"_meta": %s,\n"direct": [\n%s\n],\n"epochs": {\n%s\n},\n"widths": [\n%s\n]}\n' % (
            one(out['_meta']), ',\n'.join(one(c) for c in out['direct']),
            ',\n'.join('%s: %s' % (one(k), one(v)) for k, v in sorted(out['epochs'].items())),
            ',\n'.join(one(w) for w in out['widths'])))
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:      # fixed timestamps: a rerun writes identical bytes
        for k in sorted(arrays):
            b = io.BytesIO()
            np.save(b, arrays[k])
            z.writestr(zipfile.ZipInfo(k + '.npy', (1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)
    with open(os.path.join(GOLD, 'multi_aug.npz'), 'wb') as f:
        f.write(buf.getvalue())
    print('wrote multi_aug.json (%d direct cases, coverage %s) and multi_aug.npz' % (len(cases), out['_meta']['coverage']))


if __name__ == '__main__':
    main()

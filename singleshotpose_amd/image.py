"""Training-time image augmentation on the MI355X: the reference's image.py, batched and byte-exact with Pillow.

/root/reference/image.py runs, per sample and on the host, change_background (:111-128), data_augmentation (:46-76) and
distort_image (:14-31) through Pillow, then dataset.py:113-131 turns the PIL image into a float tensor.  Here the decoded
bytes of a whole batch go to the GPU once and four launches produce the augmented uint8 batch (csrc/image_aug.hip),
which Darknet.forward takes as it is (ssp_u8hwc_to_nhwc does ToTensor's /255): SURVEY.md section 8(f) row 3.

    aug = DeviceAugmenter(device)
    batch_u8, labels = aug.load_data_detection_batch(imgs, masks, bgs, label_rows, shape=(416, 416), jitter=0.2, hue=0.1,
                                                     saturation=1.5, exposure=1.5, num_keypoints=9, max_num_gt=50)
    out = model(batch_u8)                 # (B, H, W, 3) uint8 on the GPU; labels: (B, 50 * 21) float64 as dataset.py yields

What stays on the host: file decoding (PIL / libjpeg, out of scope), the random draws (Python's `random`, in the reference's
order, so a seeded run draws what the reference draws), the label arithmetic (fill_truth_detection, 21 numbers per
object) and the resampling coefficient tables - Pillow computes those in double per output column / row
(ImagingResample.precompute_coeffs); resample_coeffs() restates that with the same operation order, vectorised over the
batch (a few hundred KB per batch, one upload together with the launch descriptors).
No CPU fallback: without the HIP library this module raises.

The multi-object trainer's pipeline (multi_obj_pose_estimation/image_multi.py:299-382: a scene, 7 or 8 pasted objects, a
background) is split differently, because its retry loop decides on RESIZED MASKS while it draws:
draw_multi_augmentation() runs in the DataLoader worker and does the draws, the mask crops / resizes (Pillow, network
shape), the overlap test and the labels; DeviceAugmenter.load_multi_data_detection_batch() does everything that touches
an RGB image - three launches per batch.
"""
import ctypes
import random as _random

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 32 - 8 - 2      # Pillow: 8-bit pixels, 2 guard bits


class _Desc(ctypes.Structure):      # include/ssp_hip.h: SspResampleDesc
    _fields_ = [('src', ctypes.c_uint64), ('dst', ctypes.c_uint64), ('bounds', ctypes.c_uint64), ('kk', ctypes.c_uint64),
                ('img', ctypes.c_uint64), ('mask', ctypes.c_uint64), ('lut', ctypes.c_uint64),
                ('src_w', ctypes.c_int), ('src_h', ctypes.c_int), ('src_pitch', ctypes.c_int),
                ('x0', ctypes.c_int), ('y0', ctypes.c_int), ('row0', ctypes.c_int),
                ('dst_w', ctypes.c_int), ('dst_h', ctypes.c_int), ('dst_pitch', ctypes.c_int),
                ('ksize', ctypes.c_int), ('img_pitch', ctypes.c_int), ('reserved', ctypes.c_int)]


_DESC_DTYPE = np.dtype([(n, np.uint64 if t is ctypes.c_uint64 else np.int32) for n, t in _Desc._fields_])
assert _DESC_DTYPE.itemsize == ctypes.sizeof(_Desc) == 104

MAX_OBJS = 8      # include/ssp_hip.h: SSP_COMPOSITE_MAX_OBJS (get_add_objs gives 7 or 8)
_COMP_DTYPE = np.dtype([('scene', np.uint64), ('scene_mask', np.uint64), ('bg', np.uint64), ('out', np.uint64),
                        ('obj', np.uint64, (MAX_OBJS,)), ('obj_mask', np.uint64, (MAX_OBJS,)), ('nbytes', np.int64),
                        ('nobj', np.int32), ('reserved', np.int32)])      # include/ssp_hip.h: SspCompositeDesc
assert _COMP_DTYPE.itemsize == 176


def resample_coeffs(in_sizes, out_size):
    """Pillow's bicubic coefficient rows (precompute_coeffs + normalize_coeffs_8bpc over the whole input range) for a batch
    of input sizes and one output size.  Returns (ksize, bounds int32 (B, out, 2), kk int32 (B, out, ksize)); rows are
    padded with zeros to the largest ksize of the batch.  Every operation is an IEEE double operation in the order the C
    code performs it, so the integer coefficients are Pillow's."""
    in_sizes = np.asarray(in_sizes, dtype=np.int64).reshape(-1)
    scale = in_sizes.astype(np.float64) / float(out_size)
    filterscale = np.maximum(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int((np.ceil(support).astype(np.int64) * 2 + 1).max())
    ss = 1.0 / filterscale
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx[None, :] + 0.5) * scale[:, None]
    xmin = np.trunc(center - support[:, None] + 0.5).astype(np.int64)
    xmin = np.maximum(xmin, 0)
    xmax = np.trunc(center + support[:, None] + 0.5).astype(np.int64)
    xmax = np.minimum(xmax, in_sizes[:, None])
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, None, :]
    arg = ((x + xmin[..., None]).astype(np.float64) - center[..., None] + 0.5) * ss[:, None, None]
    arg = np.abs(arg)
    a = -0.5
    near = ((a + 2.0) * arg - (a + 3.0)) * arg * arg + 1
    far = (((arg - 5) * arg + 8) * arg - 4) * a
    w = np.where(arg < 1.0, near, np.where(arg < 2.0, far, 0.0))
    w = np.where(x < n[..., None], w, 0.0)
    ww = np.zeros(n.shape, np.float64)
    for j in range(ksize):                       # the C loop's summation order
        ww = ww + w[..., j]
    with np.errstate(divide='ignore', invalid='ignore'):
        k = np.where(ww[..., None] != 0.0, w / ww[..., None], w)
    fixed = np.where(k < 0, np.trunc(-0.5 + k * (1 << PRECISION_BITS)), np.trunc(0.5 + k * (1 << PRECISION_BITS)))
    kk = np.where(x < n[..., None], fixed, 0.0).astype(np.int32)
    bounds = np.stack([xmin, n], -1).astype(np.int32)
    return ksize, bounds, kk


def distort_tables(hue, sat, val):
    """The H, S and V tables of distort_image (image.py:14-31): 768 bytes per sample ((B, 768) for array arguments).
    Image.point(callable) on an 8-bit band evaluates the callable on 0..255 and rounds the Python floats half to even
    (np.rint), clipped to 0..255; the hue table wraps once in each direction, in the reference's order."""
    hue = np.atleast_1d(np.asarray(hue, np.float64))[:, None]
    sat = np.atleast_1d(np.asarray(sat, np.float64))[:, None]
    val = np.atleast_1d(np.asarray(val, np.float64))[:, None]
    i = np.arange(256, dtype=np.float64)[None, :]
    x = i + hue * 255
    x = np.where(x > 255, x - 255, x)
    x = np.where(x < 0, x + 255, x)
    t = np.concatenate([x, i * sat, i * val], 1)
    t = np.clip(np.rint(t), 0, 255).astype(np.uint8)
    return t[0] if t.shape[0] == 1 else t


def rand_scale(s, rng=_random):
    """image.py:33-37."""
    scale = rng.uniform(1, s)
    if rng.randint(1, 10000) % 2:
        return scale
    return 1. / scale


def draw_augmentation(ow, oh, jitter, hue, saturation, exposure, rng=_random):
    """The random draws of data_augmentation / random_distort_image (image.py:46-64, :39-44), in the reference's order."""
    dw, dh = int(ow * jitter), int(oh * jitter)
    pleft = rng.randint(-dw, dw)
    pright = rng.randint(-dw, dw)
    ptop = rng.randint(-dh, dh)
    pbot = rng.randint(-dh, dh)
    flip = rng.randint(1, 10000) % 2
    dhue = rng.uniform(-hue, hue)
    dsat = rand_scale(saturation, rng)
    dexp = rand_scale(exposure, rng)
    return dict(pleft=pleft, pright=pright, ptop=ptop, pbot=pbot, flip=flip, dhue=dhue, dsat=dsat, dexp=dexp)


def fill_truth_detection(labpath, w, h, flip, dx, dy, sx, sy, num_keypoints, max_num_gt):
    """image.py:78-109 (same signature): label rows of one image moved into the crop.  `labpath` may also be the parsed
    (n, 2K+3) array."""
    num_labels = 2 * num_keypoints + 3
    label = np.zeros((max_num_gt, num_labels))
    if isinstance(labpath, str):
        import os
        if not os.path.getsize(labpath):
            return np.reshape(label, (-1))
        bs = np.loadtxt(labpath)
    else:
        bs = np.array(labpath, dtype=np.float64)
    if bs is None or bs.size == 0:
        return np.reshape(label, (-1))
    bs = np.reshape(bs, (-1, num_labels))
    cc = 0
    for i in range(bs.shape[0]):
        row = bs[i]
        row[1] = min(0.999, max(0, row[1] * sx - dx))      # the centroid stays inside the image
        row[2] = min(0.999, max(0, row[2] * sy - dy))
        for j in range(1, num_keypoints):
            row[2 * j + 1] = row[2 * j + 1] * sx - dx
            row[2 * j + 2] = row[2 * j + 2] * sy - dy
        label[cc] = row
        cc += 1
        if cc >= 50:
            break
    return np.reshape(label, (-1))


# ------------------------------------------------------------------------------------------------ multi-object, host half
_ADD_OBJS = {      # image_multi.py:8-36
    'ape': ['can', 'cat', 'duck', 'glue', 'holepuncher', 'iron', 'phone'],
    'benchvise': ['ape', 'can', 'cat', 'driller', 'duck', 'glue', 'holepuncher'],
    'cam': ['ape', 'benchvise', 'can', 'cat', 'driller', 'duck', 'holepuncher'],
    'can': ['ape', 'benchvise', 'cat', 'driller', 'duck', 'eggbox', 'holepuncher'],
    'cat': ['ape', 'can', 'duck', 'glue', 'holepuncher', 'eggbox', 'phone'],
    'driller': ['ape', 'benchvise', 'can', 'cat', 'duck', 'glue', 'holepuncher'],
    'duck': ['ape', 'can', 'cat', 'eggbox', 'glue', 'holepuncher', 'phone'],
    'eggbox': ['ape', 'benchvise', 'cam', 'can', 'cat', 'duck', 'glue', 'holepuncher'],
    'glue': ['ape', 'benchvise', 'cam', 'driller', 'duck', 'eggbox', 'holepuncher'],
    'holepuncher': ['benchvise', 'cam', 'can', 'cat', 'driller', 'duck', 'eggbox'],
    'iron': ['ape', 'benchvise', 'can', 'cat', 'driller', 'duck', 'glue'],
    'lamp': ['ape', 'benchvise', 'can', 'driller', 'eggbox', 'holepuncher', 'iron'],
    'phone': ['ape', 'benchvise', 'cam', 'can', 'driller', 'duck', 'holepuncher'],
}
PIXEL_THRESHOLD = 200      # image_multi.py:301
MAX_OVERLAP = 0.2          # image_multi.py:353


def get_add_objs(objname):
    """image_multi.py:8-36: the objects pasted next to `objname` (a new list: augment_objects shuffles it in place).  An
    unknown name is a ValueError naming it (the reference ends in UnboundLocalError)."""
    if objname not in _ADD_OBJS:
        raise ValueError("get_add_objs: unknown object %r (known: %s)" % (objname, ', '.join(sorted(_ADD_OBJS))))
    return list(_ADD_OBJS[objname])


def fill_truth_detection_multi(labpath, w, h, flip, dx, dy, sx, sy, num_keypoints, max_num_gt):
    """image_multi.py:123-165 (same signature; `labpath` may also be the parsed rows).  Unlike the single-object version it
    recomputes the width / height columns from the moved keypoints; like it, it ignores `flip`, `w` and `h`."""
    num_labels = 2 * num_keypoints + 3
    label = np.zeros((max_num_gt, num_labels))
    if isinstance(labpath, str):
        import os
        if not os.path.getsize(labpath):
            return np.reshape(label, (-1))
        bs = np.loadtxt(labpath)
    else:
        bs = np.array(labpath, dtype=np.float64)
    if bs is None or bs.size == 0:
        return np.reshape(label, (-1))
    bs = np.reshape(bs, (-1, num_labels))
    cc = 0
    for i in range(bs.shape[0]):
        xs = [bs[i][2 * j + 1] for j in range(num_keypoints)]
        ys = [bs[i][2 * j + 2] for j in range(num_keypoints)]
        xs[0] = min(0.999, max(0, xs[0] * sx - dx))      # the centroid stays inside the image
        ys[0] = min(0.999, max(0, ys[0] * sy - dy))
        for j in range(1, num_keypoints):
            xs[j] = xs[j] * sx - dx
            ys[j] = ys[j] * sy - dy
        for j in range(num_keypoints):
            bs[i][2 * j + 1] = xs[j]
            bs[i][2 * j + 2] = ys[j]
        bs[i][2 * num_keypoints + 1] = max(xs) - min(xs)
        bs[i][2 * num_keypoints + 2] = max(ys) - min(ys)
        label[cc] = bs[i]
        cc += 1
        if cc >= max_num_gt:
            break
    return np.reshape(label, (-1))


def multi_label_path(imgpath):
    return imgpath.replace('images', 'labels').replace('JPEGImages', 'labels').replace('.jpg', '.txt').replace('.png', '.txt')


def multi_mask_path(imgpath):
    return imgpath.replace('JPEGImages', 'mask').replace('/00', '/').replace('.jpg', '.png')


def superimpose_masks_u8(mask, total_mask):
    """image_multi.py:282-297 on uint8 arrays: ImageMath's int32 `mask + total * round(1 - mask / 255)`, then
    convert('L'), which clips to 0..255 (values up to 127 + 255 occur where a bicubic mask edge meets a covered pixel)."""
    t = mask.astype(np.int32) + np.where(mask >= 128, 0, total_mask).astype(np.int32)
    return np.minimum(t, 255).astype(np.uint8)


def _open_rgb(path):
    from PIL import Image
    return Image.open(path).convert('RGB')


def _draw_crop(ow, oh, jitter, rng):
    dw, dh = int(ow * jitter), int(oh * jitter)
    pleft = rng.randint(-dw, dw)
    pright = rng.randint(-dw, dw)
    ptop = rng.randint(-dh, dh)
    pbot = rng.randint(-dh, dh)
    flip = rng.randint(1, 10000) % 2
    return dict(pleft=pleft, pright=pright, ptop=ptop, pbot=pbot, flip=flip, ow=ow, oh=oh)


def _crop_geometry(d):
    """(box, sx, sy, dx, dy) of data_augmentation_with_mask (image_multi.py:241-252)."""
    ow, oh = d['ow'], d['oh']
    swidth, sheight = ow - d['pleft'] - d['pright'], oh - d['ptop'] - d['pbot']
    sx, sy = float(swidth) / ow, float(sheight) / oh
    box = (d['pleft'], d['ptop'], d['pleft'] + swidth - 1, d['ptop'] + sheight - 1)
    return box, sx, sy, (float(d['pleft']) / ow) / sx, (float(d['ptop']) / oh) / sy


def draw_multi_augmentation(imgpath, shape, jitter, hue, saturation, exposure, num_keypoints=9, max_num_gt=50, rng=_random,
                            linemod_prefix='../LINEMOD/', path_prefix='../', open_rgb=_open_rgb):
    """The host half of augment_objects (image_multi.py:299-365) for one training sample: every random draw, from `rng` in
    the reference's order (shuffle(add_objs); the scene's pleft, pright, ptop, pbot, flip, shift_x, shift_y; per candidate
    randint(0, len(lines) - 1), pleft, pright, ptop, pbot, flip), the mask side of every candidate (crop, bicubic resize to
    the network shape, flip: Pillow on one 3-channel mask), the `> 200` overlap test against the running total mask with the
    reference's retries, superimpose_masks, and the label rows (fill_truth_detection_multi; row k + 1 = the first row of the
    k-th accepted object, :358).  No RGB image is opened here: a rejected candidate costs one mask decode and resize.
    hue / saturation / exposure are accepted and unused, as in the reference.

    Returns a dict: shape, imgpath, scene (the draws), scene_mask (H, W, 3) uint8, objs (accepted candidates in order:
    path, the draws, mask = the raw (h, w, 3) mask, mask_sized (H, W, 3)), tries (candidates drawn per object), draws (the
    flat sequence of drawn integers), label (max_num_gt * (2K + 3) float64), total_mask (the host's running mask)."""
    import os
    from PIL import Image, ImageChops
    shape = (int(shape[0]), int(shape[1]))
    objname = os.path.basename(os.path.dirname(os.path.dirname(imgpath)))
    add_objs = get_add_objs(objname)
    num_labels = 2 * num_keypoints + 3
    rng.shuffle(add_objs)
    mask = open_rgb(multi_mask_path(imgpath))
    iw, ih = mask.size
    sc = _draw_crop(iw, ih, jitter, rng)
    sc['shift_x'] = rng.randint(-80, 80)
    sc['shift_y'] = rng.randint(-80, 80)
    log = [sc[k] for k in ('pleft', 'pright', 'ptop', 'pbot', 'flip', 'shift_x', 'shift_y')]
    box, sx, sy, dx, dy = _crop_geometry(sc)
    dx -= float(sc['shift_x']) / shape[0]
    dy -= float(sc['shift_y']) / shape[1]
    m = ImageChops.offset(mask.crop(box).resize(shape), sc['shift_x'], sc['shift_y'])
    if sc['flip']:
        m = m.transpose(Image.FLIP_LEFT_RIGHT)
    scene_mask = np.array(m, dtype=np.uint8)
    label = fill_truth_detection_multi(multi_label_path(imgpath), iw, ih, sc['flip'], dx, dy, 1. / sx, 1. / sy, num_keypoints,
                                       max_num_gt)
    total_label = np.reshape(label, (-1, num_labels))
    total_mask = scene_mask
    yy = np.where(total_mask > PIXEL_THRESHOLD, 1, 0)
    objs, tries, count = [], [], 1
    for obj in add_objs:
        n = 0
        while True:
            n += 1
            with open(linemod_prefix + obj + '/train.txt', 'r') as f:
                lines = f.readlines()
            idx = rng.randint(0, len(lines) - 1)
            path = path_prefix + lines[idx].rstrip()
            omask = open_rgb(multi_mask_path(path))
            d = _draw_crop(omask.size[0], omask.size[1], jitter, rng)
            log += [idx] + [d[k] for k in ('pleft', 'pright', 'ptop', 'pbot', 'flip')]
            box, sx, sy, dx, dy = _crop_geometry(d)
            m = omask.crop(box).resize(shape)
            if d['flip']:
                m = m.transpose(Image.FLIP_LEFT_RIGHT)
            sized = np.array(m, dtype=np.uint8)
            xx = np.where(sized > PIXEL_THRESHOLD, 1, 0)
            area = int(np.sum(xx))
            if area == 0:                                   # nothing of the object left in the crop: draw again
                continue
            if float(np.sum(xx * yy)) / float(area) < MAX_OVERLAP:
                break
        tries.append(n)
        total_mask = superimpose_masks_u8(sized, total_mask)
        yy = np.where(total_mask > PIXEL_THRESHOLD, 1, 0)
        row = fill_truth_detection_multi(multi_label_path(path), iw, ih, d['flip'], dx, dy, 1. / sx, 1. / sy, num_keypoints,
                                         max_num_gt)
        total_label[count, :] = np.reshape(row, (-1, num_labels))[0, :]
        count += 1
        d.update(path=path, name=obj, mask=np.array(omask, dtype=np.uint8), mask_sized=sized)
        objs.append(d)
    return dict(shape=shape, imgpath=imgpath, scene=sc, scene_mask=scene_mask, objs=objs, tries=tries, draws=log,
                label=np.reshape(total_label, (-1)), total_mask=total_mask)


class DeviceAugmenter(object):
    """Batched image.py on one GPU.  Buffers (staging, intermediates) are cached and grow to the largest batch seen."""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("singleshotpose_amd.image runs on the MI355X HIP kernels only (no CPU fallback)")
        _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._bufs = {}
        self._events = {}
        self.time_kernels = False
        self.kernel_events = None

    # -------------------------------------------------------------------------------------------- buffers
    def _buf(self, name, nbytes, pinned=False):
        t = self._bufs.get(name)
        if pinned:      # the previous batch's asynchronous upload must have left this staging buffer
            ev = self._events.get(name)
            if ev is not None:
                ev.synchronize()
        if t is None or t.numel() < nbytes:
            n = int(nbytes * 1.25) + 256
            t = torch.empty(n, dtype=torch.uint8, pin_memory=True) if pinned else \
                torch.empty(n, dtype=torch.uint8, device=self.device)
            self._bufs[name] = t
        return t

    def _to_device_list(self, arrays, name):
        """list of (h, w, 3) uint8 numpy arrays / CUDA tensors -> list of (device pointer, h, w): host arrays travel in one
        pinned staging copy."""
        out, host, off = [None] * len(arrays), [], 0
        for i, a in enumerate(arrays):
            if isinstance(a, torch.Tensor):
                if not (a.is_cuda and a.dtype == torch.uint8 and a.dim() == 3 and a.size(2) == 3 and a.is_contiguous()):
                    raise ValueError("image tensors must be contiguous (h, w, 3) uint8 on the GPU")
                out[i] = (a.data_ptr(), a.size(0), a.size(1))
                self._keep.append(a)
            else:
                a = np.ascontiguousarray(a, dtype=np.uint8)
                if a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError("images are (h, w, 3) uint8 RGB arrays (Image.open(...).convert('RGB'))")
                host.append((i, a, off))
                off += (a.size + 15) // 16 * 16
        if host:
            stage = self._buf(name + '_pin', off, pinned=True)
            dev = self._buf(name + '_dev', off)
            sv = stage.numpy()
            for i, a, o in host:
                sv[o:o + a.size] = a.reshape(-1)
            dev[:off].copy_(stage[:off], non_blocking=True)
            self._events[name + '_pin'] = torch.cuda.current_stream(self.device).record_event()
            for i, a, o in host:
                out[i] = (dev.data_ptr() + o, a.shape[0], a.shape[1])
        return out

    # -------------------------------------------------------------------------------------------- the pipeline
    def load_data_detection_batch(self, imgs, masks, bgs, labels, shape, jitter, hue, saturation, exposure,
                                  num_keypoints=9, max_num_gt=50, rng=_random, draws=None):
        """load_data_detection (image.py:130-145) for a batch.

        imgs / masks / bgs: per sample an (h, w, 3) uint8 RGB array (numpy, or an already resident CUDA tensor); image and
        mask of a sample have the same size, backgrounds any size.  labels: per sample a label file path or the parsed
        (n, 2K+3) rows.  shape = (width, height) of the network input.  The random numbers come from `rng` (default: the
        global `random`, as in the reference) sample by sample in the reference's order; `draws` (list of
        draw_augmentation dicts) overrides them.
        Returns (uint8 CUDA tensor (B, height, width, 3), float64 CPU tensor (B, max_num_gt * (2K+3)))."""
        B = len(imgs)
        if not (B and len(masks) == B and len(bgs) == B and len(labels) == B):
            raise ValueError("imgs, masks, bgs and labels must be non-empty lists of one length")
        sw, sh = int(shape[0]), int(shape[1])
        st = torch.cuda.current_stream(self.device).cuda_stream
        self._keep = []
        with torch.cuda.device(self.device):
            im = self._to_device_list(imgs, 'img')
            mk = self._to_device_list(masks, 'mask')
            bg = self._to_device_list(bgs, 'bg')
            for i in range(B):
                if im[i][1:] != mk[i][1:]:
                    raise ValueError("image %d and its mask differ in size" % i)
            oh = np.array([t[1] for t in im], np.int64)
            ow = np.array([t[2] for t in im], np.int64)
            bh = np.array([t[1] for t in bg], np.int64)
            bw = np.array([t[2] for t in bg], np.int64)
            if draws is None:
                draws = [draw_augmentation(int(ow[i]), int(oh[i]), jitter, hue, saturation, exposure, rng) for i in range(B)]
            pleft = np.array([d['pleft'] for d in draws], np.int64)
            ptop = np.array([d['ptop'] for d in draws], np.int64)
            swidth = ow - pleft - np.array([d['pright'] for d in draws], np.int64)
            sheight = oh - ptop - np.array([d['pbot'] for d in draws], np.int64)
            cw, ch = swidth - 1, sheight - 1           # img.crop((l, t, l + swidth - 1, t + sheight - 1)), image.py:64
            if (cw <= 0).any() or (ch <= 0).any():
                raise ValueError("jitter leaves an empty crop")

            # ---- coefficient tables: background -> image size (per sample sizes), crop -> network shape ----
            def per_sample(in_sizes, out_sizes):
                """out sizes differ per sample (the background is resized to each image's size): group equal ones."""
                res = [None] * B
                for o in np.unique(out_sizes):
                    idx = np.nonzero(out_sizes == o)[0]
                    ks, bnd, kk = resample_coeffs(in_sizes[idx], int(o))
                    for j, i in enumerate(idx):
                        res[i] = (ks, bnd[j], kk[j])
                return res
            bg_h, bg_v = per_sample(bw, ow), per_sample(bh, oh)
            ks_ch, bnd_ch, kk_ch = resample_coeffs(cw, sw)
            ks_cv, bnd_cv, kk_cv = resample_coeffs(ch, sh)

            # rows of each horizontal pass = what its vertical pass reads (ImagingResample: ybox_first .. ybox_last)
            def rows(bnd):
                return int(bnd[0, 0]), int(bnd[-1, 0] + bnd[-1, 1])
            bg_rows = [rows(bg_v[i][1]) for i in range(B)]
            cr_rows = [rows(bnd_cv[i]) for i in range(B)]

            # ---- one blob: descriptors (4 launches x B), coefficient tables, distort tables ----
            parts, off = [], [0]

            def put(arr):
                arr = np.ascontiguousarray(arr)
                o = off[0]
                parts.append((o, arr))
                off[0] = (o + arr.nbytes + 15) // 16 * 16
                return o
            desc = np.zeros((4, B), _DESC_DTYPE)
            o_desc = put(desc)
            # tables shared by the whole batch go in as one array each, per-sample ones (background) one by one
            o_ch_b, o_ch_k, o_cv_b, o_cv_k = put(bnd_ch), put(kk_ch), put(bnd_cv), put(kk_cv)
            luts = distort_tables([d['dhue'] for d in draws], [d['dsat'] for d in draws], [d['dexp'] for d in draws])
            o_lut = put(luts.reshape(B, 768))
            o_bg = np.array([[put(bg_h[i][1]), put(bg_h[i][2]), put(bg_v[i][1]), put(bg_v[i][2])] for i in range(B)], np.int64)
            blob_n = off[0]
            # intermediates
            bg_r0 = np.array([r[0] for r in bg_rows], np.int64)
            bg_nr = np.array([r[1] - r[0] for r in bg_rows], np.int64)
            cr_r0 = np.array([r[0] for r in cr_rows], np.int64)
            cr_nr = np.array([r[1] - r[0] for r in cr_rows], np.int64)
            t1_off = np.concatenate([[0], np.cumsum(bg_nr * ow * 3)])
            cp_off = np.concatenate([[0], np.cumsum(oh * ow * 3)])
            t2_off = np.concatenate([[0], np.cumsum(cr_nr * sw * 3)])
            tmp1 = self._buf('tmp1', int(t1_off[-1]))
            comp = self._buf('comp', int(cp_off[-1]))
            tmp2 = self._buf('tmp2', int(t2_off[-1]))
            out = torch.empty(B, sh, sw, 3, dtype=torch.uint8, device=self.device)
            blob_dev = self._buf('blob_dev', blob_n)
            base = blob_dev.data_ptr()
            idx = np.arange(B, dtype=np.int64)
            p_im = np.array([t[0] for t in im], np.uint64)
            p_mk = np.array([t[0] for t in mk], np.uint64)
            p_bg = np.array([t[0] for t in bg], np.uint64)
            p_t1 = (tmp1.data_ptr() + t1_off[:-1]).astype(np.uint64)
            p_cp = (comp.data_ptr() + cp_off[:-1]).astype(np.uint64)
            p_t2 = (tmp2.data_ptr() + t2_off[:-1]).astype(np.uint64)

            def fill(d, **kw):
                for k, v in kw.items():
                    d[k] = v
            # background, horizontal pass: (bh x bw) -> rows [r0, r1) x ow
            fill(desc[0], src=p_bg, src_w=bw, src_h=bh, src_pitch=bw * 3, row0=bg_r0, dst=p_t1, dst_w=ow, dst_h=bg_nr,
                 dst_pitch=ow * 3, bounds=(base + o_bg[:, 0]).astype(np.uint64), kk=(base + o_bg[:, 1]).astype(np.uint64),
                 ksize=np.array([t[0] for t in bg_h]))
            # background, vertical pass + composite (image.py:111-128)
            fill(desc[1], src=p_t1, src_w=ow, src_h=bg_nr, src_pitch=ow * 3, row0=bg_r0, dst=p_cp, dst_w=ow, dst_h=oh,
                 dst_pitch=ow * 3, bounds=(base + o_bg[:, 2]).astype(np.uint64), kk=(base + o_bg[:, 3]).astype(np.uint64),
                 ksize=np.array([t[0] for t in bg_v]), img=p_im, mask=p_mk, img_pitch=ow * 3)
            # crop window of the composite, horizontal pass to the network width
            fill(desc[2], src=p_cp, src_w=ow, src_h=oh, src_pitch=ow * 3, x0=pleft, y0=ptop, row0=cr_r0, dst=p_t2, dst_w=sw,
                 dst_h=cr_nr, dst_pitch=sw * 3, bounds=(base + o_ch_b + idx * bnd_ch[0].nbytes).astype(np.uint64),
                 kk=(base + o_ch_k + idx * kk_ch[0].nbytes).astype(np.uint64), ksize=ks_ch)
            # vertical pass to the network height + distort_image (image.py:14-31)
            fill(desc[3], src=p_t2, src_w=sw, src_h=cr_nr, src_pitch=sw * 3, row0=cr_r0,
                 dst=(out.data_ptr() + idx * (sh * sw * 3)).astype(np.uint64), dst_w=sw, dst_h=sh, dst_pitch=sw * 3,
                 bounds=(base + o_cv_b + idx * bnd_cv[0].nbytes).astype(np.uint64),
                 kk=(base + o_cv_k + idx * kk_cv[0].nbytes).astype(np.uint64), ksize=ks_cv,
                 lut=(base + o_lut + idx * 768).astype(np.uint64))
            parts[0] = (o_desc, desc)
            blob = self._buf('blob_pin', blob_n, pinned=True)
            bv = blob.numpy()
            for o, arr in parts:
                bv[o:o + arr.nbytes] = arr.reshape(-1).view(np.uint8)
            blob_dev[:blob_n].copy_(blob[:blob_n], non_blocking=True)
            self._events['blob_pin'] = torch.cuda.current_stream(self.device).record_event()

            dsz = _DESC_DTYPE.itemsize
            mx = [int((bg_nr * ow).max()), int((oh * ow).max()), int(cr_nr.max()) * sw, sh * sw]
            ev = None
            if self.time_kernels:       # tools/aug_bench.py: device time of the four launches alone
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            _lib.call('ssp_resample_u8', base + o_desc + 0 * B * dsz, B, 0, 0, mx[0], st)
            _lib.call('ssp_resample_u8', base + o_desc + 1 * B * dsz, B, 1, 1, mx[1], st)
            _lib.call('ssp_resample_u8', base + o_desc + 2 * B * dsz, B, 0, 0, mx[2], st)
            _lib.call('ssp_resample_u8', base + o_desc + 3 * B * dsz, B, 1, 2, mx[3], st)
            if ev is not None:
                ev[1].record()
                self.kernel_events = ev

        # ---- labels (host): image.py:139-144 ----
        lab = np.zeros((B, max_num_gt * (2 * num_keypoints + 3)))
        for i in range(B):
            sx, sy = float(swidth[i]) / float(ow[i]), float(sheight[i]) / float(oh[i])
            dx = (float(pleft[i]) / float(ow[i])) / sx
            dy = (float(ptop[i]) / float(oh[i])) / sy
            lab[i] = fill_truth_detection(labels[i], sw, sh, draws[i]['flip'], dx, dy, 1. / sx, 1. / sy, num_keypoints,
                                          max_num_gt)
        self._keep = []
        return out, torch.from_numpy(lab)

    # -------------------------------------------------------------------------------------------- the multi-object pipeline
    def load_multi_data_detection_batch(self, samples, shape=None):
        """load_data_detection of image_multi.py (:367-382) for a batch, the image half: `samples` are
        draw_multi_augmentation() results with the decoded pixels added - sample['img'] (the scene), sample['bg'], and
        obj['img'] for every accepted object, each an (h, w, 3) uint8 RGB array (numpy, or a resident CUDA tensor; the
        same holds for the masks the draw step produced: scene_mask, obj['mask'], obj['mask_sized']).  All samples share
        one network shape (width, height).  Three launches for the whole batch:
          1. horizontal resample of every layer (scene, objects, background) over its crop window; the objects read
             img * round(mask / 255) (mask_background as the source side of the taps),
          2. vertical resample of every layer; the scene is stored at its ImageChops.offset + flip position, an object at
             its flip position,
          3. the compositor: superimpose_masks / superimpose_masked_imgs per accepted object in order, the scene object
             back on top, change_background.
        Returns (uint8 CUDA tensor (B, height, width, 3), float64 CPU tensor (B, max_num_gt * (2K+3)))."""
        B = len(samples)
        if not B:
            raise ValueError("samples must be a non-empty list")
        shapes = set(tuple(s['shape']) for s in samples) | (set() if shape is None else {(int(shape[0]), int(shape[1]))})
        if len(shapes) != 1:
            raise ValueError("the samples of one batch must share one network shape, got %s" % sorted(shapes))
        sw, sh = shapes.pop()
        nobj = [len(s['objs']) for s in samples]
        if max(nobj) > MAX_OBJS:
            raise ValueError("at most %d pasted objects per sample" % MAX_OBJS)
        st = torch.cuda.current_stream(self.device).cuda_stream
        self._keep = []
        nbytes = sh * sw * 3
        stride = (nbytes + 15) // 16 * 16
        with torch.cuda.device(self.device):
            # ---- every array of the batch in one staging copy: resample sources first, then the network-shape masks ----
            arrays, src, msk, geo, sized = [], [], [], [], []      # layer -> index into arrays (source, raw mask or -1)
            first = []                                              # per sample: index of its scene layer
            for s in samples:
                first.append(len(src))
                sc = s['scene']
                box, _, _, _, _ = _crop_geometry(sc)
                arrays.append(s['img']); src.append(len(arrays) - 1); msk.append(-1)
                geo.append((box[0], box[1], box[2] - box[0], box[3] - box[1], sc['shift_x'] % sw, sc['shift_y'] % sh, sc['flip']))
                for o in s['objs']:
                    box, _, _, _, _ = _crop_geometry(o)
                    arrays.append(o['img']); src.append(len(arrays) - 1)
                    arrays.append(o['mask']); msk.append(len(arrays) - 1)
                    geo.append((box[0], box[1], box[2] - box[0], box[3] - box[1], 0, 0, o['flip']))
                arrays.append(s['bg']); src.append(len(arrays) - 1); msk.append(-1)
                geo.append((0, 0, -1, -1, 0, 0, 0))
                arrays.append(s['scene_mask']); sized.append(len(arrays) - 1)
                for o in s['objs']:
                    arrays.append(o['mask_sized']); sized.append(len(arrays) - 1)
            dev = self._to_device_list(arrays, 'multi')
            L = len(src)
            geo = np.array(geo, np.int64)
            p_src = np.array([dev[i][0] for i in src], np.uint64)
            p_msk = np.array([dev[i][0] if i >= 0 else 0 for i in msk], np.uint64)
            oh = np.array([dev[i][1] for i in src], np.int64)
            ow = np.array([dev[i][2] for i in src], np.int64)
            for l in range(L):
                if msk[l] >= 0 and dev[msk[l]][1:] != dev[src[l]][1:]:
                    raise ValueError("a pasted object's image and mask differ in size")
            for i in sized:
                if dev[i][1:] != (sh, sw) or dev[i][0] % 16:
                    raise ValueError("resized masks are 16-byte aligned (height, width, 3) arrays of the network shape")
            x0, y0 = geo[:, 0], geo[:, 1]
            cw = np.where(geo[:, 2] < 0, ow, geo[:, 2])
            ch = np.where(geo[:, 3] < 0, oh, geo[:, 3])
            if (cw <= 0).any() or (ch <= 0).any():
                raise ValueError("jitter leaves an empty crop")
            ks_h, bnd_h, kk_h = resample_coeffs(cw, sw)
            ks_v, bnd_v, kk_v = resample_coeffs(ch, sh)
            r0 = bnd_v[:, 0, 0].astype(np.int64)                       # rows the vertical pass reads (ybox_first .. ybox_last)
            nr = (bnd_v[:, -1, 0] + bnd_v[:, -1, 1]).astype(np.int64) - r0

            parts, off = [], [0]

            def put(arr):
                arr = np.ascontiguousarray(arr)
                o = off[0]
                parts.append((o, arr))
                off[0] = (o + arr.nbytes + 15) // 16 * 16
                return o
            desc = np.zeros((2, L), _DESC_DTYPE)
            comp = np.zeros(B, _COMP_DTYPE)
            o_desc, o_comp = put(desc), put(comp)
            o_hb, o_hk, o_vb, o_vk = put(bnd_h), put(kk_h), put(bnd_v), put(kk_v)
            blob_n = off[0]
            t_off = np.concatenate([[0], np.cumsum((nr * sw * 3 + 15) // 16 * 16)])
            tmp = self._buf('multi_tmp', int(t_off[-1]))
            layers = self._buf('multi_layers', L * stride)
            out = torch.empty(B, sh, sw, 3, dtype=torch.uint8, device=self.device)
            if stride != nbytes:      # the compositor addresses every layer from a 16-byte aligned start
                outbuf = self._buf('multi_out', B * stride)
            else:
                outbuf = out
            blob_dev = self._buf('blob_dev', blob_n)
            base = blob_dev.data_ptr()
            idx = np.arange(L, dtype=np.int64)
            p_tmp = (tmp.data_ptr() + t_off[:-1]).astype(np.uint64)
            p_lay = (layers.data_ptr() + idx * stride).astype(np.uint64)

            def fill(d, **kw):
                for k, v in kw.items():
                    d[k] = v
            fill(desc[0], src=p_src, mask=p_msk, src_w=ow, src_h=oh, src_pitch=ow * 3, x0=x0, y0=y0, row0=r0, dst=p_tmp,
                 dst_w=sw, dst_h=nr, dst_pitch=sw * 3, bounds=(base + o_hb + idx * bnd_h[0].nbytes).astype(np.uint64),
                 kk=(base + o_hk + idx * kk_h[0].nbytes).astype(np.uint64), ksize=ks_h)
            fill(desc[1], src=p_tmp, src_w=sw, src_h=nr, src_pitch=sw * 3, row0=r0, dst=p_lay, dst_w=sw, dst_h=sh,
                 dst_pitch=sw * 3, x0=geo[:, 4], y0=geo[:, 5], reserved=geo[:, 6],
                 bounds=(base + o_vb + idx * bnd_v[0].nbytes).astype(np.uint64),
                 kk=(base + o_vk + idx * kk_v[0].nbytes).astype(np.uint64), ksize=ks_v)
            k = 0
            for i in range(B):
                f, n = first[i], nobj[i]
                c = comp[i]
                c['scene'], c['bg'] = p_lay[f], p_lay[f + n + 1]
                c['scene_mask'] = dev[sized[k]][0]
                c['out'] = outbuf.data_ptr() + i * stride
                c['obj'][:n] = p_lay[f + 1:f + 1 + n]
                c['obj_mask'][:n] = [dev[j][0] for j in sized[k + 1:k + 1 + n]]
                c['nbytes'], c['nobj'] = nbytes, n
                k += 1 + n
            blob = self._buf('blob_pin', blob_n, pinned=True)
            bv = blob.numpy()
            for o, arr in parts:
                bv[o:o + arr.nbytes] = arr.reshape(-1).view(np.uint8)
            blob_dev[:blob_n].copy_(blob[:blob_n], non_blocking=True)
            self._events['blob_pin'] = torch.cuda.current_stream(self.device).record_event()

            ev = None
            if self.time_kernels:       # tools/aug_bench.py: device time of the three launches alone
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            dsz = _DESC_DTYPE.itemsize
            _lib.call('ssp_resample_u8', base + o_desc, L, 0, 3, int(nr.max()) * sw, st)
            _lib.call('ssp_resample_u8', base + o_desc + L * dsz, L, 1, 4, sh * sw, st)
            _lib.call('ssp_composite_u8', base + o_comp, B, nbytes, st)
            if ev is not None:
                ev[1].record()
                self.kernel_events = ev
            if outbuf is not out:
                out.view(B, nbytes).copy_(outbuf[:B * stride].view(B, stride)[:, :nbytes])
        self._keep = []
        return out, torch.from_numpy(np.stack([np.asarray(s['label'], np.float64) for s in samples]))


def distort_image(rgb_u8, hue, sat, val):
    """distort_image (image.py:14-31) of a CUDA uint8 (..., 3) RGB tensor."""
    if not (rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.size(-1) == 3):
        raise RuntimeError("singleshotpose_amd.image.distort_image takes a CUDA uint8 (..., 3) tensor (no CPU fallback)")
    x = rgb_u8.contiguous()
    out = torch.empty_like(x)
    lut = torch.from_numpy(distort_tables(hue, sat, val).reshape(-1)).to(x.device)
    _lib.call('ssp_distort_u8', x.data_ptr(), out.data_ptr(), x.numel() // 3, lut.data_ptr(), 0,
              torch.cuda.current_stream(x.device).cuda_stream)
    return out


def composite_u8(scene, scene_mask, bg, objs=(), obj_masks=()):
    """The layer compositor alone (include/ssp_hip.h: ssp_composite_u8) on CUDA uint8 tensors of one shape: per byte
    total = pos(scene_mask) ? scene : 0, then every (obj, obj_mask) in order, the scene back on top, `bg` where the running
    mask stays below 128.  image_multi.py's mask_background is (img, mask, zeros), superimpose_masked_imgs is
    (img, mask, total) and change_background at equal sizes is (img, mask, bg)."""
    ts = [scene, scene_mask, bg] + list(objs) + list(obj_masks)
    if len(objs) != len(obj_masks) or len(objs) > MAX_OBJS:
        raise ValueError("as many object masks as objects, at most %d" % MAX_OBJS)
    for t in ts:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.shape == scene.shape):
            raise RuntimeError("singleshotpose_amd.image.composite_u8 takes CUDA uint8 tensors of one shape (no CPU fallback)")
    n = scene.numel()
    pad = (n + 15) // 16 * 16
    buf = torch.zeros(len(ts) + 1, pad, dtype=torch.uint8, device=scene.device)      # 16-byte aligned rows
    for i, t in enumerate(ts):
        buf[i, :n] = t.reshape(-1)
    c = np.zeros(1, _COMP_DTYPE)
    row = lambda i: buf.data_ptr() + i * pad
    c['scene'], c['scene_mask'], c['bg'], c['out'] = row(0), row(1), row(2), row(len(ts))
    k = len(objs)
    c['obj'][0, :k] = [row(3 + i) for i in range(k)]
    c['obj_mask'][0, :k] = [row(3 + k + i) for i in range(k)]
    c['nbytes'], c['nobj'] = n, k
    d = torch.from_numpy(c.view(np.uint8).copy()).to(scene.device)
    with torch.cuda.device(scene.device):
        _lib.call('ssp_composite_u8', d.data_ptr(), 1, n, torch.cuda.current_stream(scene.device).cuda_stream)
    return buf[len(ts), :n].reshape(scene.shape).clone()


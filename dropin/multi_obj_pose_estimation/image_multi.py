"""Drop-in for the names of the reference's multi_obj_pose_estimation/image_multi.py, on the GPU kernels of
singleshotpose_amd.image.  The batched form - what dataset_multi.py feeds, three launches per DataLoader batch - is the
product path; the functions here keep the reference's per-sample signatures (PIL images in and out).

    get_add_objs            image_multi.py:8-36     (host; an unknown object is a ValueError naming it)
    rand_scale              :78-82                  (host: two draws from `random`)
    fill_truth_detection    :123-165                (host: recomputes the width / height columns)
    load_data_detection     :367-382                draws + mask side on the host, the pixels in one batch-of-one GPU pass
    augment_objects         :299-365                the same pass before change_background
    mask_background         :38-50                  the compositor kernel with no objects and a black background
    superimpose_masked_imgs :265-280                the compositor kernel (images of one size)
    superimpose_masks       :282-297                (host: the worker keeps the running mask; same integer arithmetic)
change_background (:167-182) and the two data_augmentation_with_mask functions (:184-263) are stages INSIDE the fused pass
(the crop is a resample window, offset and flip are the vertical pass's store index, the background is one more layer)
and are not offered on their own.  No CPU fallback: without the HIP library the pixel functions raise.
"""
import numpy as np
import torch
from PIL import Image

from singleshotpose_amd import image as _image
from singleshotpose_amd.image import get_add_objs, rand_scale  # noqa: F401
from singleshotpose_amd.image import fill_truth_detection_multi as fill_truth_detection  # noqa: F401


def _augmenter():
    from dataset import _augmenter as per_device
    return per_device(torch.device('cuda', torch.cuda.current_device()))


def _rgb(pil_or_path):
    im = Image.open(pil_or_path) if isinstance(pil_or_path, str) else pil_or_path
    return np.array(im.convert('RGB'), dtype=np.uint8)


def _composite(scene, mask, bg):
    t = [torch.from_numpy(_rgb(x)).cuda() for x in (scene, mask, bg)]
    return Image.fromarray(_image.composite_u8(*t).cpu().numpy())


def mask_background(img, mask):
    return _composite(img, mask, Image.new('RGB', img.size))


def superimpose_masked_imgs(masked_img, mask, total_mask):
    return _composite(masked_img, mask, total_mask.resize(masked_img.size).convert('RGB'))


def superimpose_masks(mask, total_mask):
    total = _rgb(total_mask.resize(mask.size))
    return Image.fromarray(_image.superimpose_masks_u8(_rgb(mask), total))


def _run(imgpath, shape, jitter, hue, saturation, exposure, bg, num_keypoints, max_num_gt):
    rec = _image.draw_multi_augmentation(imgpath, shape, jitter, hue, saturation, exposure, num_keypoints, max_num_gt)
    rec['img'] = _rgb(imgpath)
    rec['bg'] = bg
    for o in rec['objs']:
        o['img'] = _rgb(o['path'])
    out, label = _augmenter().load_multi_data_detection_batch([rec], shape)
    return Image.fromarray(out[0].cpu().numpy()), label[0].numpy(), Image.fromarray(rec['total_mask'])


def augment_objects(imgpath, objname, add_objs, shape, jitter, hue, saturation, exposure, num_keypoints, max_num_gt):
    """`objname` / `add_objs` are derived from the path again, as load_data_detection derives them (the shuffle is the
    first draw either way); where the total mask is below 128 the reference's total image is black, which is what a
    black background gives."""
    return _run(imgpath, shape, jitter, hue, saturation, exposure, np.zeros((8, 8, 3), np.uint8), num_keypoints, max_num_gt)


def load_data_detection(imgpath, shape, jitter, hue, saturation, exposure, bgpath, num_keypoints, max_num_gt):
    img, label, _ = _run(imgpath, shape, jitter, hue, saturation, exposure, _rgb(bgpath), num_keypoints, max_num_gt)
    return img, label

"""Multi-object decode helpers - host-side mirror of multi_obj_pose_estimation/utils_multi.py.

Everything utils.py offers, plus get_multi_region_boxes (utils_multi.py:266-382), bbox_iou (:125-156) and `nms`
(:223-241: no caller on the pose path - valid_multi.py / train_multi.py never invoke it - kept as a small host helper
because the reference's scripts do `from utils_multi import *`).  The per-cell decode (sigmoid, grid offsets, softmax, arg-max) runs in ssp_region_decode_all; the
variable-length box lists are assembled on the host from that one device->host copy, with the reference's rules:
threshold on det_conf (only_objectness) or det_conf*cls_max_conf; a fallback box of `correspondingclass` when no kept
box has that class; `max_cls_conf` is NOT reset per image.

match_multi_region_boxes / evaluate_multi_batched are the batched validator (valid_multi.py:94-149 for every image and
every ground truth of a batch, all object classes in one pass): ssp_region_match_multi selects the box of each ground
truth on the device, one fused ssp_pnp_batched launch and one ssp_pose_errors launch follow, one copy returns the result.
Given one mesh per class ({class id: vertices}) every ground truth is scored against its own object model
(ssp_pose_errors_models), the symmetric classes with ADD-S as well (ssp_adds_errors); summarize_multi turns the result
into the per-class accuracies the reference's validators print.

detect_multi_region_boxes / detect_multi_batched are the same selection WITHOUT labels, for a trained network on new
images: ssp_region_detect_multi selects the box of every queried class of every image in one launch (the device code of
ssp_region_match_multi), one ssp_pnp_batched launch turns all of them into poses, one copy returns the result.
"""
import collections
import collections.abc
import sys

import numpy as np
import torch

from . import _lib
from .utils import *  # noqa: F401,F403
from .utils import (_pack_models, _to_dev_f64, adds_device, get_3D_corners, pnp_device, pose_errors_device,
                    pose_errors_models_device)

MAX_GT = 50      # label rows per image (dataset_multi.py pads every label file to 50 rows)


def _span(lo_a, hi_a, lo_b, hi_b):
    """Length of the overlap of two intervals (<= 0 when they are disjoint)."""
    return min(hi_a, hi_b) - max(lo_a, lo_b)


def bbox_iou(box1, box2, x1y1x2y2=False):
    """Intersection over union of two boxes given as corners (x1, y1, x2, y2) or as centre + size (x, y, w, h) - the
    helper region_loss_multi.py:74 calls on [0, 0, anchor_w, anchor_h] boxes (utils_multi.py:125-156); on the hot path
    the anchor pick runs inside ssp_region_loss, this host version serves callers and tests."""
    if x1y1x2y2:
        ax0, ay0, ax1, ay1 = box1[0], box1[1], box1[2], box1[3]
        bx0, by0, bx1, by1 = box2[0], box2[1], box2[2], box2[3]
    else:
        ax0, ax1 = box1[0] - box1[2] / 2.0, box1[0] + box1[2] / 2.0
        ay0, ay1 = box1[1] - box1[3] / 2.0, box1[1] + box1[3] / 2.0
        bx0, bx1 = box2[0] - box2[2] / 2.0, box2[0] + box2[2] / 2.0
        by0, by1 = box2[1] - box2[3] / 2.0, box2[1] + box2[3] / 2.0
    ow, oh = _span(ax0, ax1, bx0, bx1), _span(ay0, ay1, by0, by1)
    if ow <= 0 or oh <= 0:
        return 0.0
    inter = ow * oh
    return inter / ((ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0) - inter)


def nms(boxes, nms_thresh):
    """Greedy non-maximum suppression over (x, y, w, h, det_conf, ...) boxes (utils_multi.py:223-241): boxes are visited
    by descending det_conf; a visited box with det_conf > 0 is kept and zeroes the det_conf (IN PLACE, as the reference
    does) of every later box whose centre-size IoU with it exceeds `nms_thresh`."""
    if len(boxes) == 0:
        return boxes
    order = np.argsort(np.asarray([1.0 - float(b[4]) for b in boxes], dtype=np.float32), kind='stable')
    kept = []
    for pos, i in enumerate(order):
        cur = boxes[i]
        if not cur[4] > 0:
            continue
        kept.append(cur)
        for j in order[pos + 1:]:
            if bbox_iou(cur, boxes[j], x1y1x2y2=False) > nms_thresh:
                boxes[j][4] = 0
    return kept


def region_rows(output, num_classes, num_keypoints, num_anchors):
    """(B, nA*h*w, 2K+3+nC) float32 CPU array of decoded cells in the reference's (cy, cx, anchor) scan order."""
    if output.dim() == 3:
        output = output.unsqueeze(0)
    if not output.is_cuda:
        raise RuntimeError("get_multi_region_boxes runs on the MI355X HIP kernel only: got a %s tensor (no CPU fallback)" % output.device)
    assert output.size(1) == (2 * num_keypoints + 1 + num_classes) * num_anchors
    out = output.detach().to(torch.float32).contiguous()
    B, h, w = out.size(0), out.size(2), out.size(3)
    rows = torch.empty(B, num_anchors * h * w, 2 * num_keypoints + 3 + num_classes, dtype=torch.float32, device=out.device)
    _lib.call('ssp_region_decode_all', out.data_ptr(), rows.data_ptr(), B, num_anchors, num_classes, h, w,
              num_keypoints, torch.cuda.current_stream().cuda_stream)
    return rows.cpu().numpy()


def get_multi_region_boxes(output, conf_thresh, num_classes, num_keypoints, anchors, num_anchors, correspondingclass,
                           only_objectness=1, validation=False):
    K = num_keypoints
    rows = region_rows(output, num_classes, K, num_anchors)
    all_boxes = []
    max_cls_conf = -sys.maxsize          # persists across images, as in the reference
    max_ind = None                       # (image, cell) of the running fallback candidate - also persists
    for b in range(rows.shape[0]):
        r = rows[b]
        det, cmax, cid = r[:, 2 * K], r[:, 2 * K + 1], r[:, 2 * K + 2]
        ccorr = r[:, 2 * K + 3 + correspondingclass]
        conf = det if only_objectness else det * cmax
        # running arg-max used by the fallback box: strict improvements of BOTH det_conf and the class confidence
        max_conf = -1
        for ind in range(r.shape[0]):
            if det[ind] > max_conf and ccorr[ind] > max_cls_conf:
                max_conf, max_cls_conf, max_ind = det[ind], ccorr[ind], (b, ind)
        boxes = []
        for ind in np.nonzero(conf > conf_thresh)[0]:
            box = [float(v) for v in r[ind, :2 * K]] + [float(det[ind]), float(cmax[ind]), int(cid[ind])]
            if (not only_objectness) and validation:
                for c in range(num_classes):
                    tmp = r[ind, 2 * K + 3 + c]
                    if c != int(cid[ind]) and det[ind] * tmp > conf_thresh:
                        box += [float(tmp), c]
            boxes.append(box)
        if len(boxes) == 0 or correspondingclass not in [bx[2 * K + 2] for bx in boxes]:
            if max_ind is None:
                raise UnboundLocalError("max_ind")      # the reference fails the same way when no cell ever qualified
            boxes.append([float(v) for v in rows[max_ind[0]][max_ind[1], :2 * K]] +
                         [float(max_conf), float(max_cls_conf), correspondingclass])
        all_boxes.append(boxes)
    return all_boxes


MultiMatch = collections.namedtuple('MultiMatch', 'boxes source key match')
MultiEval = collections.namedtuple('MultiEval', 'image gt cls source corners2D_pr match R_gt t_gt R_pr t_pr errors')


def _head_f32(output, num_classes, num_keypoints, num_anchors, who):
    if output.dim() == 3:
        output = output.unsqueeze(0)
    if not output.is_cuda:
        raise RuntimeError("%s runs on the MI355X HIP kernel only: got a %s tensor (no CPU fallback)" % (who, output.device))
    assert output.size(1) == (2 * num_keypoints + 1 + num_classes) * num_anchors
    return output.detach().to(torch.float32).contiguous()


def _labels(target, B, num_keypoints):
    """The DataLoader's (B, 50*(2K+3)) label tensor (host or device, any float type) as (B, 50, 2K+3), not yet moved."""
    t = target if torch.is_tensor(target) else torch.as_tensor(np.asarray(target))
    return t.detach().reshape(B, MAX_GT, 2 * num_keypoints + 3)


def match_multi_region_boxes(output, target, conf_thresh, num_classes, num_keypoints, num_anchors, only_objectness=0,
                             im_width=640, im_height=480):
    """The box valid_multi.py:110-123 selects for every ground truth of every image, in one launch (no host loop).

    output: the raw head (B, nA*(2K+1+nC), H, W) on the device; target: the (B, 50*(2K+3)) labels, host or device.
    For ground truth k of image b, of class c, the result is what get_multi_region_boxes(output[b:b+1], ...,
    correspondingclass=c, only_objectness) followed by the validator's best-det_conf selection yields.  Returns device
    tensors, one fixed row per label slot:
      boxes  (B, 50, 2K+3) float32  2K normalised corner coordinates, det_conf, class confidence, class
      source (B, 50) int32          1 a kept cell of class c, 2 the fallback box, 0 no result: a row at or past the
                                    image's ground-truth count, a class outside [0, nC), or a head whose det_conf is NaN
                                    everywhere (the reference raises UnboundLocalError there); such rows are all zero
      key    (B, 50) int32          scan-order index (cy*W + cx)*nA + anchor of the selected cell, -1 when source is 0
      match  (B, 50) float32        corner_confidence(ground-truth corners, predicted corners) at im_width x im_height

    IMAGES ARE INDEPENDENT.  The reference carries max_cls_conf and max_ind from one image of a batched call over to the
    next (get_multi_region_boxes above reproduces that), but it only ever calls the function at batch 1; this function
    gives every image the batch-1 result.
    """
    K = num_keypoints
    out = _head_f32(output, num_classes, K, num_anchors, "match_multi_region_boxes")
    B, h, w = out.size(0), out.size(2), out.size(3)
    tgt = _labels(target, B, K).to(device=out.device, dtype=torch.float32).contiguous()
    rows = torch.empty(B, MAX_GT, 2 * K + 4, dtype=torch.float32, device=out.device)
    meta = torch.empty(B, MAX_GT, 2, dtype=torch.int32, device=out.device)
    _lib.call('ssp_region_match_multi', out.data_ptr(), tgt.data_ptr(), rows.data_ptr(), meta.data_ptr(), B, num_anchors,
              num_classes, h, w, K, float(conf_thresh), 1 if only_objectness else 0, int(im_width), int(im_height),
              torch.cuda.current_stream().cuda_stream)
    return MultiMatch(rows[..., :2 * K + 3], meta[..., 0], meta[..., 1], rows[..., 2 * K + 3])


def _object_points(vertices):
    """The nine PnP object points of a mesh, (9,3) float32: the centroid 0 and the 8 corners of get_3D_corners
    (valid_multi.py:135)."""
    corners3D = get_3D_corners(np.asarray(vertices.cpu() if torch.is_tensor(vertices) else vertices))
    return np.array(np.transpose(np.concatenate((np.zeros((3, 1)), corners3D[:3, :]), axis=1)), dtype='float32')


def _class_models(vertices, symmetric):
    """{class id: mesh} -> (sorted class ids, concatenated (sumN,3) float64 mesh, (nM+1,) int32 offsets, (nM,9,3) float64
    PnP object points, sorted symmetric model indices); ValueError before anything touches the GPU."""
    classes = sorted(int(c) for c in vertices.keys())
    v, off = _pack_models([vertices[c] for c in classes])          # raises on an empty mapping / a mesh of another shape
    obj = np.stack([_object_points(vertices[c]) for c in classes]).astype(np.float64)
    sym = sorted(set(int(c) for c in (symmetric if symmetric is not None else ())))
    missing = [c for c in sym if c not in classes]
    if missing:
        raise ValueError("symmetric names class %s, which has no object model" % missing)
    return classes, v, off, obj, [classes.index(c) for c in sym]


def evaluate_multi_batched(output, target, conf_thresh, num_classes, num_keypoints, anchors, num_anchors, vertices,
                           intrinsic_calibration, im_width, im_height, only_objectness=0, symmetric=None):
    """valid_multi.py:94-149 for all images and all ground truths of a batch, every object class in the same pass.

    match_multi_region_boxes, then on the device: both corner sets denormalised in float32, fix_corner_order on the
    ground-truth corners, ONE PnP launch over the 2n problems (ground truths first, predictions after) with the object
    points (centroid 0 + the 8 corners of get_3D_corners(vertices)) and K rounded to float32 as valid_multi.py:135-136
    does, one pose-error launch with the float64 K, one device->host copy.  Which label rows are ground truths (row
    index below the image's count, class inside [0, nC)) is read from the labels on the host - free for the host tensor
    a DataLoader yields; a device `target` costs one extra copy of its first two columns.  Rows the kernel reports as
    source 0 (NaN head) are dropped.  Images are independent (see match_multi_region_boxes).

    Returns numpy arrays over the n surviving ground truths, in (image, row) order: image, gt (label row), cls, source
    (n,) ints; corners2D_pr (n,9,2) float32 pixels; match (n,) float32; R_gt, R_pr (n,3,3), t_gt, t_pr (n,3,1) float64;
    errors (n,4) float64 in pose_errors_batched's column order.

    ONE MESH PER CLASS.  `vertices` may be a mapping {class id: (3|4, N) mesh} instead of one mesh for the whole batch -
    the reference's validator is run once per object and loads that object's mesh, corners and diameter each time
    (valid_multi.py:47-50).  Every ground truth and its prediction then use the object points of their own class in the
    same single PnP launch and the vertices of their own class in one ssp_pose_errors_models launch; ground truths of a
    class WITHOUT a model are left out of the result (the reference scores 6 of the 13 classes of yolo-pose-multi.cfg the
    same way).  symmetric: an iterable of class ids scored with ADD-S as well (adi(estimate, ground truth),
    utils_multi.py:66-69; only their rows go to ssp_adds_errors): `errors` is then (n,5), column 4 ADD-S for those
    classes and NaN for the others.  The meshes, offsets and object points are assembled once per call on the host and
    uploaded in one copy.  An empty mapping, a mesh that is not (3|4, N) and a symmetric id without a model raise
    ValueError before the GPU is touched; a single mesh with symmetric=None takes the single-mesh path unchanged."""
    K = num_keypoints
    models = None
    if isinstance(vertices, collections.abc.Mapping):
        models = _class_models(vertices, symmetric)
    elif symmetric is not None:
        raise ValueError("symmetric needs one object model per class: pass vertices as {class id: mesh}")
    ncol = 5 if symmetric is not None else 4
    out = _head_f32(output, num_classes, K, num_anchors, "evaluate_multi_batched")
    dev = out.device
    lab = _labels(target, out.size(0), K)
    m = match_multi_region_boxes(out, lab, conf_thresh, num_classes, K, num_anchors, only_objectness, im_width, im_height)
    head = lab[..., :2].to(torch.float32).cpu().numpy()
    image, gt = [], []
    for b in range(head.shape[0]):
        stop = np.nonzero(head[b, :, 1] == 0)[0]
        for k in range(int(stop[0]) if len(stop) else MAX_GT):
            if np.isfinite(head[b, k, 0]) and 0 <= int(head[b, k, 0]) < num_classes and (
                    models is None or int(head[b, k, 0]) in models[0]):
                image.append(b)
                gt.append(k)
    image, gt = np.asarray(image, dtype=np.int64), np.asarray(gt, dtype=np.int64)
    n = len(image)
    cls = head[image, gt, 0].astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    if n == 0:
        z = np.zeros
        return MultiEval(image, gt, cls, z(0, dtype=np.int64), z((0, K, 2), dtype=np.float32), z(0, dtype=np.float32),
                         z((0, 3, 3)), z((0, 3, 1)), z((0, 3, 3)), z((0, 3, 1)), z((0, ncol)))
    if models is None:
        bi, ki = torch.as_tensor(image).to(dev), torch.as_tensor(gt).to(dev)
    else:
        # one upload of the indices (image, label row, model of every ground truth, rows of the symmetric classes) and
        # one of the floats (meshes back to back, object points, offsets: integers below 2^53 are exact in float64)
        classes, mesh, off, objs, sym = models
        which = np.searchsorted(classes, cls)
        sym_rows = np.nonzero(np.isin(which, sym))[0]
        idx = torch.as_tensor(np.concatenate((image, gt, which, sym_rows)).astype(np.int64)).to(dev)
        bi, ki, pm, sel = idx[:n], idx[n:2 * n], idx[2 * n:3 * n], idx[3 * n:]
        blob = torch.as_tensor(np.concatenate((mesh.reshape(-1), objs.reshape(-1), off.astype(np.float64)))).to(dev)
        v = blob[:mesh.size].reshape(-1, 3)
        objd = blob[mesh.size:mesh.size + objs.size].reshape(-1, K, 3)
        offd = blob[mesh.size + objs.size:].to(torch.int32)
    scale = torch.tensor([float(im_width), float(im_height)], dtype=torch.float32, device=dev)
    order = torch.tensor([0, 1, 3, 5, 7, 2, 4, 6, 8], device=dev)                      # fix_corner_order
    tgt = lab.to(device=dev, dtype=torch.float32)
    c_gt = (tgt[bi, ki, 1:2 * K + 1].reshape(n, K, 2) * scale)[:, order]
    c_pr = m.boxes[bi, ki, :2 * K].reshape(n, K, 2) * scale
    K32 = np.array(np.asarray(intrinsic_calibration.cpu() if torch.is_tensor(intrinsic_calibration)
                              else intrinsic_calibration), dtype='float32')
    if models is None:
        p3 = torch.as_tensor(_object_points(vertices).astype(np.float64)).to(dev).expand(2 * n, K, 3).contiguous()
    else:
        p3 = objd[pm].repeat(2, 1, 1).contiguous()           # ground truths first, predictions after: the same points twice
    Kt = torch.as_tensor(K32.astype(np.float64)).to(dev).expand(2 * n, 3, 3).contiguous()
    Rt = pnp_device(p3, torch.cat((c_gt, c_pr), dim=0).to(torch.float64).contiguous(), Kt)
    Kd = _to_dev_f64(intrinsic_calibration).reshape(1, 9)
    if models is None:
        v = _to_dev_f64(vertices)
        if v.dim() != 2 or v.size(0) not in (3, 4):
            raise ValueError("vertices must be (3,N) or (4,N)")
        err = pose_errors_device(v[:3].t().contiguous(), Rt[:n], Rt[n:], Kd)
    else:
        pm32 = pm.to(torch.int32)
        err = pose_errors_models_device(v, offd, pm32, Rt[:n].contiguous(), Rt[n:].contiguous(), Kd)
        if symmetric is not None:
            err = torch.cat((err, torch.full((n, 1), float('nan'), dtype=torch.float64, device=dev)), dim=1)
            if len(sym_rows):
                err[sel, 4] = adds_device(v, offd, pm32[sel].contiguous(), Rt[n:][sel].contiguous(), Rt[:n][sel].contiguous(),
                                          int(np.diff(off)[sym].max()))
    packed = torch.cat((m.source[bi, ki].to(torch.float64).unsqueeze(1), m.match[bi, ki].to(torch.float64).unsqueeze(1),
                        c_pr.reshape(n, 2 * K).to(torch.float64), Rt[:n], Rt[n:], err), dim=1).cpu().numpy()
    keep = packed[:, 0] != 0
    packed = packed[keep]
    o = 2 + 2 * K
    return MultiEval(image[keep], gt[keep], cls[keep], packed[:, 0].astype(np.int64),
                     packed[:, 2:o].astype(np.float32).reshape(-1, K, 2), packed[:, 1].astype(np.float32),
                     packed[:, o:o + 9].reshape(-1, 3, 3).copy(), packed[:, o + 9:o + 12].reshape(-1, 3, 1).copy(),
                     packed[:, o + 12:o + 21].reshape(-1, 3, 3).copy(), packed[:, o + 21:o + 24].reshape(-1, 3, 1).copy(),
                     packed[:, o + 24:o + 24 + ncol].copy())


MultiDetect = collections.namedtuple('MultiDetect', 'boxes source key classes')
MultiPoses = collections.namedtuple('MultiPoses', 'image cls source key det_conf cls_conf corners2D_pr R_pr t_pr')


def _class_list(classes, num_classes, who):
    """A host iterable of class ids (None: every class) as a list of ints; ValueError on an empty list or an id outside
    [0, num_classes) - nothing here touches the GPU."""
    if classes is None:
        return list(range(int(num_classes)))
    cl = [int(c) for c in classes]
    if len(cl) == 0:
        raise ValueError("%s: the list of classes is empty" % who)
    bad = [c for c in cl if not 0 <= c < num_classes]
    if bad:
        raise ValueError("%s: class %s is outside [0, %d)" % (who, bad, num_classes))
    return cl


def detect_multi_region_boxes(output, conf_thresh, num_classes, num_keypoints, num_anchors, classes=None,
                              only_objectness=0):
    """The box of every queried class on every image, WITHOUT labels, in one launch and with no copy to the host.

    output: the raw head (B, nA*(2K+1+nC), H, W) on the device; classes: a host iterable of class ids (an id may repeat,
    any order), or None for all num_classes of them.  For image b and class c the result is what
    get_multi_region_boxes(output[b:b+1], ..., correspondingclass=c, only_objectness) followed by the validator's
    best-det_conf selection (valid_multi.py:118-123) yields - the rows match_multi_region_boxes returns for a ground truth
    of class c, from the same device code.  Returns device tensors, nQ = len(classes):
      boxes   (B, nQ, 2K+3) float32  2K normalised corner coordinates, det_conf, class confidence, class
      source  (B, nQ) int32          1 a kept cell of class c (conf > conf_thresh and c is its arg-max class); 2 the
                                     reference's fallback box: NOTHING of class c passed the threshold, the object is
                                     probably not in the image; 0 no result (det_conf NaN everywhere), the row is all zero
      key     (B, nQ) int32          scan-order index (cy*W + cx)*nA + anchor of the selected cell, -1 when source is 0
      classes (nQ,) int32            the queried class of every column
    Images are independent (see match_multi_region_boxes).  An empty list and an id outside [0, num_classes) raise
    ValueError before the GPU is touched; a CPU `output` raises RuntimeError (no CPU fallback)."""
    K = num_keypoints
    cl = _class_list(classes, num_classes, "detect_multi_region_boxes")
    out = _head_f32(output, num_classes, K, num_anchors, "detect_multi_region_boxes")
    B, h, w = out.size(0), out.size(2), out.size(3)
    nQ = len(cl)
    if classes is None:
        cls_dev, cls_ptr = torch.arange(nQ, dtype=torch.int32, device=out.device), None      # NULL: slot q is class q
    else:
        cls_dev = torch.tensor(cl, dtype=torch.int32).to(out.device)
        cls_ptr = cls_dev.data_ptr()
    rows = torch.empty(B, nQ, 2 * K + 3, dtype=torch.float32, device=out.device)
    meta = torch.empty(B, nQ, 2, dtype=torch.int32, device=out.device)
    _lib.call('ssp_region_detect_multi', out.data_ptr(), cls_ptr, rows.data_ptr(), meta.data_ptr(), B, num_anchors,
              num_classes, h, w, K, nQ, float(conf_thresh), 1 if only_objectness else 0,
              torch.cuda.current_stream().cuda_stream)
    return MultiDetect(rows, meta[..., 0], meta[..., 1], cls_dev)


def detect_multi_batched(output, conf_thresh, num_classes, num_keypoints, anchors, num_anchors, vertices,
                         intrinsic_calibration, im_width, im_height, classes=None, only_objectness=0, keep_fallback=True):
    """From the raw head of a batch of NEW images (no labels) to one 6D pose per image and object class.

    detect_multi_region_boxes, then on the device: the corners denormalised in float32 (x * im_width, y * im_height),
    ONE PnP launch over all B * nQ (image, class) problems - each with the object points of its own class (centroid 0 +
    the 8 corners of get_3D_corners(vertices[c])) and K rounded to float32, as evaluate_multi_batched does - and one
    device->host copy.  Rows without a result (source 0) still occupy a problem slot, fed with fixed finite corners,
    and are dropped afterwards: the launch shape depends on B and nQ only.

    vertices: {class id: (3|4, N) mesh}; classes: a host iterable of class ids, default the mapping's sorted keys;
    intrinsic_calibration: (3,3), or (B,3,3) with one camera per image.  keep_fallback=False also drops the source 2
    rows (nothing of that class passed the threshold - see detect_multi_region_boxes).  Returns numpy arrays over the
    n surviving (image, class) pairs, in (image, class-list) order: image, cls, source, key (n,) ints; det_conf,
    cls_conf (n,) float32; corners2D_pr (n,9,2) float32 pixels; R_pr (n,3,3), t_pr (n,3,1) float64.
    A `vertices` that is no mapping, an empty mapping, a mesh that is not (3|4, N), a queried class without a mesh or
    outside [0, num_classes), an empty class list and intrinsics of another shape raise ValueError before the GPU is
    touched; a CPU `output` raises RuntimeError."""
    K = num_keypoints
    if not isinstance(vertices, collections.abc.Mapping):
        raise ValueError("detect_multi_batched needs one object model per class: pass vertices as {class id: mesh}")
    mclasses, _, _, objs, _ = _class_models(vertices, None)
    cl = _class_list(mclasses if classes is None else classes, num_classes, "detect_multi_batched")
    missing = [c for c in cl if c not in mclasses]
    if missing:
        raise ValueError("detect_multi_batched: class %s has no object model" % missing)
    B = 1 if output.dim() == 3 else output.size(0)
    K32 = np.array(np.asarray(intrinsic_calibration.cpu() if torch.is_tensor(intrinsic_calibration)
                              else intrinsic_calibration), dtype='float32')
    if K32.shape not in ((3, 3), (B, 3, 3)):
        raise ValueError("intrinsic_calibration must be (3,3) or (B,3,3) = (%d,3,3), got %s" % (B, K32.shape))
    d = detect_multi_region_boxes(output, conf_thresh, num_classes, K, num_anchors, cl, only_objectness)
    dev = d.boxes.device
    nQ = len(cl)
    n = B * nQ
    # one upload of the floats: the object points of the queried classes, the camera(s), the pixel scale and the
    # stand-in corners of the rows without a result (a 3 x 3 grid inside the image: finite and not degenerate)
    which = [mclasses.index(c) for c in cl]
    grid = np.array([[im_width * (1 + i) / 4.0, im_height * (1 + j) / 4.0] for j in range(3) for i in range(3)])
    blob = torch.as_tensor(np.concatenate((objs[which].reshape(-1), K32.astype(np.float64).reshape(-1), grid.reshape(-1),
                                           [float(im_width), float(im_height)]))).to(dev)
    o1 = nQ * K * 3
    o2 = o1 + K32.size
    p3 = blob[:o1].reshape(nQ, K, 3).repeat(B, 1, 1).contiguous()                # problem b * nQ + q: class cl[q]
    Kt = blob[o1:o2].reshape(-1, 1, 3, 3).expand(-1, nQ, 3, 3) if K32.ndim == 3 else blob[o1:o2].reshape(1, 3, 3)
    Kt = Kt.reshape(-1, 3, 3).expand(n, 3, 3).contiguous()
    standin = blob[o2:o2 + 2 * K].reshape(1, K, 2)
    scale = blob[o2 + 2 * K:].to(torch.float32)
    src = d.source.reshape(n)
    c_pr = d.boxes[..., :2 * K].reshape(n, K, 2) * scale
    p2 = torch.where((src != 0).reshape(n, 1, 1), c_pr.to(torch.float64), standin).contiguous()
    Rt = pnp_device(p3, p2, Kt)
    packed = torch.cat((src.to(torch.float64).unsqueeze(1), d.key.reshape(n, 1).to(torch.float64),
                        d.boxes[..., 2 * K:2 * K + 2].reshape(n, 2).to(torch.float64),
                        c_pr.reshape(n, 2 * K).to(torch.float64), Rt), dim=1).cpu().numpy()
    keep = packed[:, 0] != 0
    if not keep_fallback:
        keep &= packed[:, 0] != 2
    image = np.repeat(np.arange(B, dtype=np.int64), nQ)[keep]
    cls = np.tile(np.asarray(cl, dtype=np.int64), B)[keep]
    packed = packed[keep]
    o = 4 + 2 * K
    return MultiPoses(image, cls, packed[:, 0].astype(np.int64), packed[:, 1].astype(np.int64),
                      packed[:, 2].astype(np.float32), packed[:, 3].astype(np.float32),
                      packed[:, 4:o].astype(np.float32).reshape(-1, K, 2), packed[:, o:o + 9].reshape(-1, 3, 3).copy(),
                      packed[:, o + 9:o + 12].reshape(-1, 3, 1).copy())


def summarize_multi(ev, diameters, px=5.0, add_frac=0.1, cm=0.05, deg=5.0):
    """Per-class accuracies of an evaluate_multi_batched result, host numpy: {class id: dict(count, acc_px, acc_add,
    acc_cm_deg)} for every class of `diameters` ({class id: model diameter}), in percent with the reference's
    eps = 1e-5 in the denominator (valid_multi.py:154-156, valid.py's acc / acc3d10 / acc5cm5deg):
      acc_px      pixel_dist <= px
      acc_add     ADD(-S) <= add_frac * diameter: ADD-S (column 4) where it is finite, vertex_dist (column 1) otherwise
      acc_cm_deg  trans_dist <= cm and angle_dist <= deg
    A class without rows has count 0 and accuracies 0."""
    eps = 1e-5
    errors, cls = np.asarray(ev.errors, dtype=np.float64), np.asarray(ev.cls)
    add = errors[:, 1].copy()
    if errors.shape[1] > 4:
        adds = np.isfinite(errors[:, 4])
        add[adds] = errors[adds, 4]
    res = {}
    for c in sorted(diameters):
        rows = cls == c
        count = int(rows.sum())
        pct = lambda hit: int(np.count_nonzero(hit[rows])) * 100. / (count + eps)
        res[c] = dict(count=count, acc_px=pct(errors[:, 0] <= px), acc_add=pct(add <= add_frac * float(diameters[c])),
                      acc_cm_deg=pct((errors[:, 2] <= cm) & (errors[:, 3] <= deg)))
    return res

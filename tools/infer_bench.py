#!/usr/bin/env python
"""Latency-bound pieces of the path (SURVEY.md section 8(d) config 4 and the 'report us per call' rows): eval-mode
forward at 672x672 (valid.py's test size), decode, batched PnP, batched pose errors, RegionLoss, fused SGD, and the
multi-object validator (eval_multi: evaluate_multi_batched against today's per-ground-truth host route).
Prints one JSON object; numbers go to DESIGN.md section 3.  `infer_bench.py eval_multi` runs that line alone;
`infer_bench.py pnp` the batched PnP line alone;
`infer_bench.py detect_multi` times the label-free multi-object detector (detect_multi_batched, all 13 classes) against
the per-image, per-class host route;
`infer_bench.py adds` times ADD-S and the per-class validator."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def eval_multi(res):
    """B=64, 5x13x13 head, 13 classes, 2 ground truths per image.  `batched`: one evaluate_multi_batched call (match
    kernel, one fused PnP launch, one pose-error launch, one copy).  `per_gt_host_route`: what a validator can do without
    it - per ground truth a batch-1 get_multi_region_boxes for its class, the selection loop of valid_multi.py:118-123 and
    two pnp calls (its pose errors are NOT included, the batched call's are)."""
    from singleshotpose_amd import utils_multi as UM
    B, nA, nC, K, grid, thresh = 64, 5, 13, 9, 13, 0.05
    anchors = [1.4820, 2.2412, 2.0501, 3.1265, 2.3946, 4.6891, 3.1018, 3.9910, 3.4879, 5.8851]
    g = torch.Generator().manual_seed(0)
    head = torch.randn(B, nA, 2 * K + 1 + nC, grid, grid, generator=g)
    head[:, :, 2 * K] -= 3.0                              # a few dozen cells per image above the threshold
    head = head.view(B, -1, grid, grid).cuda()
    rs = np.random.RandomState(0)
    tgt = np.zeros((B, 50, 2 * K + 3), dtype=np.float32)
    for b in range(B):
        for k in range(2):
            c = rs.uniform(0.3, 0.7, 2)
            tgt[b, k, 0] = rs.randint(0, nC)
            tgt[b, k, 1:2 * K + 1] = (c[None, :] + rs.uniform(-0.1, 0.1, (K, 2))).reshape(-1)
    target = torch.from_numpy(tgt.reshape(B, -1))
    half = np.array([0.038, 0.039, 0.046])
    verts = np.concatenate(((rs.uniform(-1, 1, (5841, 3)) * half).T, np.ones((1, 5841))), axis=0)
    Kc = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.5704, 242.0489], [0.0, 0.0, 1.0]])
    obj = np.array(np.concatenate((np.zeros((3, 1)), UM.get_3D_corners(verts)[:3, :]), axis=1).T, dtype='float32')
    K32 = np.array(Kc, dtype='float32')

    def batched():
        return UM.evaluate_multi_batched(head, target, thresh, nC, K, anchors, nA, verts, Kc, 640, 480)

    def per_gt():
        poses = 0
        for b in range(B):
            for k in range(2):
                c = int(tgt[b, k, 0])
                boxes = UM.get_multi_region_boxes(head[b:b + 1], thresh, nC, K, anchors, nA, c, only_objectness=0)[0]
                best = -sys.maxsize
                for bx in boxes:
                    if bx[2 * K] > best and bx[2 * K + 2] == c:
                        best, box_pr = bx[2 * K], bx
                gt = np.array(np.reshape(tgt[b, k, 1:2 * K + 1], [-1, 2]), dtype='float32') * np.float32([640, 480])
                pr = np.array(np.reshape(box_pr[:2 * K], [-1, 2]), dtype='float32') * np.float32([640, 480])
                UM.pnp(obj, UM.fix_corner_order(gt), K32)
                UM.pnp(obj, pr, K32)
                poses += 1
        return poses

    n = len(batched().image)
    res['eval_multi_b64_13x13_2gt_batched'] = {'us': round(timed(batched, 20) * 1e6, 1), 'ground_truths': n}
    res['eval_multi_b64_13x13_2gt_per_gt_host_route'] = {'us': round(timed(per_gt, 2, warm=1) * 1e6, 1), 'ground_truths': per_gt()}


def detect_multi(res):
    """B=64, 5x13x13 head, all 13 classes, one mesh per class, no labels.  `batched`: one detect_multi_batched call
    (detect kernel, one PnP launch over the 832 problems, one copy); `select_only`: detect_multi_region_boxes alone,
    synchronised.  `per_class_host_route`: the label-free route without them - per image and class a batch-1
    get_multi_region_boxes, the selection loop of valid_multi.py:118-123 and one pnp call."""
    from singleshotpose_amd import utils_multi as UM
    B, nA, nC, K, grid, thresh = 64, 5, 13, 9, 13, 0.05
    anchors = [1.4820, 2.2412, 2.0501, 3.1265, 2.3946, 4.6891, 3.1018, 3.9910, 3.4879, 5.8851]
    g = torch.Generator().manual_seed(0)
    head = torch.randn(B, nA, 2 * K + 1 + nC, grid, grid, generator=g)
    head[:, :, 2 * K] -= 3.0                              # a few dozen cells per image above the threshold
    head = head.view(B, -1, grid, grid).cuda()
    rs = np.random.RandomState(0)
    half = np.array([0.038, 0.039, 0.046])
    verts = np.concatenate(((rs.uniform(-1, 1, (5841, 3)) * half).T, np.ones((1, 5841))), axis=0)
    meshes = {c: np.concatenate((verts[:3] * (1.0 + 0.1 * c), verts[3:]), axis=0) for c in range(nC)}
    Kc = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.5704, 242.0489], [0.0, 0.0, 1.0]])
    objs = {c: np.array(np.concatenate((np.zeros((3, 1)), UM.get_3D_corners(meshes[c])[:3, :]), axis=1).T, dtype='float32')
            for c in range(nC)}
    K32 = np.array(Kc, dtype='float32')

    def batched():
        return UM.detect_multi_batched(head, thresh, nC, K, anchors, nA, meshes, Kc, 640, 480)

    def select_only(th=thresh):
        d = UM.detect_multi_region_boxes(head, th, nC, K, nA)
        torch.cuda.synchronize()
        return d

    def per_class():
        poses = 0
        for b in range(B):
            for c in range(nC):
                boxes = UM.get_multi_region_boxes(head[b:b + 1], thresh, nC, K, anchors, nA, c, only_objectness=0)[0]
                best = -sys.maxsize
                for bx in boxes:
                    if bx[2 * K] > best and bx[2 * K + 2] == c:
                        best, box_pr = bx[2 * K], bx
                pr = np.array(np.reshape(box_pr[:2 * K], [-1, 2]), dtype='float32') * np.float32([640, 480])
                UM.pnp(objs[c], pr, K32)
                poses += 1
        return poses

    p = batched()
    res['detect_multi_b64_13x13_13cls_batched'] = {'us': round(timed(batched, 20) * 1e6, 1), 'poses': len(p.image),
                                                   'fallback_rows': int((p.source == 2).sum())}
    res['detect_multi_b64_13x13_13cls_select_only'] = {'us': round(timed(select_only, 50) * 1e6, 1)}
    # the same launch at a threshold nothing passes: every one of the 832 rows walks the fallback chain
    res['detect_multi_b64_13x13_13cls_select_only_all_fallback'] = {
        'us': round(timed(lambda: select_only(0.9), 50) * 1e6, 1), 'fallback_rows': int((select_only(0.9).source == 2).sum())}
    res['detect_multi_b64_13x13_13cls_per_class_host_route'] = {'us': round(timed(per_class, 1, warm=1) * 1e6, 1),
                                                                'poses': B * nC}


def adds(res):
    """N = 5841 vertices (the ape mesh), n = 128 poses.  One adds_device call (ssp_adds_errors: n * N^2 = 4.4 G fp64 pair
    evaluations) on device tensors; ssp_pose_errors_models against ssp_pose_errors on the same poses; the host route,
    utils.adi (scipy KD-tree) once per pose, where scipy imports; and the whole validator call of eval_multi() with one
    mesh for six of the 13 classes and one of them symmetric, beside the single-mesh call in the same run."""
    from singleshotpose_amd import _lib
    from singleshotpose_amd import utils as U
    from singleshotpose_amd import utils_multi as UM
    rs = np.random.RandomState(0)
    N, n = 5841, 128
    half = np.array([0.038, 0.039, 0.046])
    verts = rs.uniform(-1, 1, (N, 3)) * half
    R = np.stack([np.linalg.qr(rs.standard_normal((3, 3)))[0] for _ in range(n)])
    R *= np.sign(np.linalg.det(R))[:, None, None]
    t = np.stack([np.array([rs.uniform(-.1, .1), rs.uniform(-.1, .1), rs.uniform(.6, 1.2)]) for _ in range(n)])
    def turn(angle):
        a = rs.standard_normal(3)
        a /= np.linalg.norm(a)
        X = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        return np.eye(3) + np.sin(angle) * X + (1 - np.cos(angle)) * X.dot(X)
    small = np.stack([turn(0.05) for _ in range(n)])          # the estimate: 3 degrees and up to 1 cm off
    R2, t2 = np.einsum('nij,njk->nik', small, R), t + rs.uniform(-0.01, 0.01, (n, 3))
    dev = torch.device('cuda', 0)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    v, off, pm = up(verts), up(np.array([0, N], dtype=np.int32)), up(np.zeros(n, dtype=np.int32))
    Rt_gt, Rt_pr = up(np.concatenate((R.reshape(n, 9), t), axis=1)), up(np.concatenate((R2.reshape(n, 9), t2), axis=1))
    Kc = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.5704, 242.0489], [0.0, 0.0, 1.0]])
    Kd = up(Kc.reshape(1, 9))
    q = lambda count: _lib.query('ssp_adds_workspace_doubles', 1, count)
    res['adds_chunk_vertices'] = next(c for c in (256, 512, 1024, 2048) if q(c) == 1 and q(c + 1) == 2)
    dt = timed(lambda: U.adds_device(v, off, pm, Rt_pr, Rt_gt, N), 10)
    res['adds_device_128x5841'] = {'us': round(dt * 1e6, 1), 'pairs_per_s': round(n * N * N / dt, -6)}
    dt = timed(lambda: U.pose_errors_models_device(v, off, pm, Rt_gt, Rt_pr, Kd), 20)
    res['pose_errors_models_128x5841'] = {'us': round(dt * 1e6, 1)}
    dt = timed(lambda: U.pose_errors_device(v, Rt_gt, Rt_pr, Kd), 20)
    res['pose_errors_128x5841'] = {'us': round(dt * 1e6, 1)}
    dt = timed(lambda: U.adi_batched(verts.T, R2, t2, R, t), 10)
    res['adi_batched_128x5841_incl_h2d_d2h'] = {'us': round(dt * 1e6, 1)}
    gpu = U.adi_batched(verts.T, R2, t2, R, t)
    try:
        import scipy  # noqa: F401
        t0 = time.perf_counter()
        host = np.array([U.adi(verts.dot(R2[i].T) + t2[i], verts.dot(R[i].T) + t[i]) for i in range(n)])
        res['adi_host_scipy_128x5841'] = {'us': round((time.perf_counter() - t0) * 1e6, 1),
                                          'max_abs_diff_to_gpu': float(np.abs(host - gpu).max())}
    except ImportError:
        res['adi_host_scipy_128x5841'] = 'scipy is not installed'
    # the whole validator call: eval_multi()'s inputs, one 5841-vertex mesh for six classes, one of them symmetric
    B, nA, nC, K, grid, thresh = 64, 5, 13, 9, 13, 0.05
    anchors = [1.4820, 2.2412, 2.0501, 3.1265, 2.3946, 4.6891, 3.1018, 3.9910, 3.4879, 5.8851]
    g = torch.Generator().manual_seed(0)
    head = torch.randn(B, nA, 2 * K + 1 + nC, grid, grid, generator=g)
    head[:, :, 2 * K] -= 3.0
    head = head.view(B, -1, grid, grid).cuda()
    tgt = np.zeros((B, 50, 2 * K + 3), dtype=np.float32)
    for b in range(B):
        for k in range(2):
            c = rs.uniform(0.3, 0.7, 2)
            tgt[b, k, 0] = rs.randint(0, 6)
            tgt[b, k, 1:2 * K + 1] = (c[None, :] + rs.uniform(-0.1, 0.1, (K, 2))).reshape(-1)
    target = torch.from_numpy(tgt.reshape(B, -1))
    meshes = {c: (verts * (1.0 + 0.1 * c)).T for c in range(6)}
    call = lambda vertices, **kw: UM.evaluate_multi_batched(head, target, thresh, nC, K, anchors, nA, vertices, Kc, 640, 480, **kw)
    rows = len(call(meshes).image)
    nsym = int((call(meshes).cls == 3).sum())
    res['eval_multi_b64_13x13_2gt_single_mesh'] = {'us': round(timed(lambda: call(meshes[0]), 20) * 1e6, 1), 'ground_truths': rows}
    res['eval_multi_b64_13x13_2gt_6_meshes'] = {'us': round(timed(lambda: call(meshes), 20) * 1e6, 1), 'ground_truths': rows}
    res['eval_multi_b64_13x13_2gt_6_meshes_1_symmetric'] = {'us': round(timed(lambda: call(meshes, symmetric=[3]), 20) * 1e6, 1),
                                                            'ground_truths': rows, 'adds_rows': nsym}


def pnp(res):
    """64 noise-free synthetic poses (ape-sized box, LINEMOD intrinsics) through pnp_batched, host copies included;
    returns what the pose-error rows of main() go on with."""
    from singleshotpose_amd import utils as U
    rs = np.random.RandomState(0)
    n = 64
    half = np.array([0.038, 0.039, 0.046])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    obj = np.concatenate((np.zeros((1, 3)), corners), axis=0)
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.5704, 242.0489], [0.0, 0.0, 1.0]])
    R = np.stack([np.linalg.qr(rs.standard_normal((3, 3)))[0] for _ in range(n)])
    R *= np.sign(np.linalg.det(R))[:, None, None]
    t = np.stack([np.array([[rs.uniform(-.1, .1)], [rs.uniform(-.1, .1)], [rs.uniform(.6, 1.2)]]) for _ in range(n)])
    cam = np.einsum('ij,njk->nik', K, np.einsum('nij,kj->nik', R, obj) + t)
    uv = (cam[:, :2] / cam[:, 2:3]).transpose(0, 2, 1)
    objs = np.broadcast_to(obj, (n, 9, 3))
    dt = timed(lambda: U.pnp_batched(objs, uv, K), 20)
    res['pnp_batched_64_incl_h2d_d2h'] = {'us': round(dt * 1e6, 1)}
    return rs, half, objs, uv, K, R, t


def main():
    if sys.argv[1:] in (['eval_multi'], ['detect_multi'], ['adds'], ['pnp']):
        res = {}
        {'eval_multi': eval_multi, 'detect_multi': detect_multi, 'adds': adds, 'pnp': pnp}[sys.argv[1]](res)
        print(json.dumps(res))
        return
    from singleshotpose_amd import utils as U
    from singleshotpose_amd.darknet import Darknet
    from singleshotpose_amd.region_loss import RegionLoss
    torch.manual_seed(0)
    dev = torch.device('cuda', 0)
    model = Darknet(os.path.join(ROOT, 'cfg', 'yolo-pose.cfg')).to(dev).eval()
    res = {}
    with torch.no_grad():
        for B, iters in ((1, 50), (8, 20), (64, 5)):
            x = torch.rand(B, 3, 672, 672, device=dev)
            model(x)
            dt = timed(lambda: model(x), iters)
            res['eval_forward_672_b%d' % B] = {'ms': round(dt * 1e3, 3), 'images_per_s': round(B / dt, 1)}
        x = torch.rand(64, 3, 672, 672, device=dev)
        out = model(x)
        dt = timed(lambda: U.region_boxes_batched(out, 1, 9), 50)
        res['decode_argmax_b64_21x21'] = {'us': round(dt * 1e6, 1)}
        dt = timed(lambda: U.get_region_boxes(out, 1, 9), 10)
        res['get_region_boxes_b64_21x21_incl_host_list'] = {'us': round(dt * 1e6, 1)}
    rs, half, objs, uv, K, R, t = pnp(res)
    verts = rs.uniform(-1, 1, (5841, 3)) * half          # the ape mesh has 5841 vertices
    Rg, tg = U.pnp_batched(objs, uv, K)
    dt = timed(lambda: U.pose_errors_batched(verts.T, Rg, tg, R, t, K), 20)
    res['pose_errors_batched_64x5841_incl_h2d_d2h'] = {'us': round(dt * 1e6, 1)}
    dt = timed(lambda: U.calc_pts_diameter_gpu(verts), 10)
    res['pts_diameter_5841_incl_h2d_d2h'] = {'us': round(dt * 1e6, 1)}
    # RegionLoss alone (B=64, 13x13), labels already on the device
    crit = RegionLoss()
    crit.verbose = False
    head = torch.randn(64, 20, 13, 13, device=dev, requires_grad=True)
    tgt = torch.zeros(64, 50 * 21, dtype=torch.float64)
    tgt[:, 1:19] = torch.rand(64, 18, dtype=torch.float64) * 0.5 + 0.25
    tgt[:, 19:21] = 0.2
    tgt_dev = tgt.to(dev)
    dt = timed(lambda: crit(head, tgt_dev, 20), 50)
    res['region_loss_fwd_b64_device_labels'] = {'us': round(dt * 1e6, 1)}
    dt = timed(lambda: crit(head, tgt, 20), 50)
    res['region_loss_fwd_b64_host_f64_labels'] = {'us': round(dt * 1e6, 1)}
    eval_multi(res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

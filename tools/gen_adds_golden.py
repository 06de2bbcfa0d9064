"""Writes tests/golden/adds.npz: the reference's ADD-S, adi(pts_est, pts_gt) of utils.py:60-63 (scipy cKDTree built on the
estimated points, queried with the ground-truth points), and its plain ADD (compute_transformation + the norm of
valid.py:168-172) over synthetic meshes and poses.  The reference's utils.py is imported unmodified and read-only, with
cv2 stubbed as oracle/gen_golden.py does (utils.py imports it and never calls it here).

Build machine only (the reference and scipy are not needed by the tests); only the data this writes is committed.

adds.npz
  base                 (1500, 3) float64 point cloud, denser towards the centre; every mesh is a slice of it
  sym_mesh             (400, 3)  a mesh that maps onto itself under a half turn about z: P and diag(-1,-1,1) P
  launches             number of launches L; launch k is what ONE call of the kernel gets:
  models_<k>           (nM, 2) int32  (start, N): model m is base[start : start + N]   (sym_mesh for the symmetric launch)
  pose_model_<k>       (n,) int32     the model of every pose
  Rt_gt_<k>, Rt_pr_<k> (n, 12)        R (9, row-major) | t (3) of the ground truth and of the estimate
  adds_<k>             (n,)           adi(estimate-posed points, ground-truth-posed points)
  add_<k>              (n,)           mean || ground-truth-posed - estimate-posed ||
  sizes                the N of the single-mesh launches 0 .. len(sizes)-1 (n = 1 each): the tile and chunk edges
  multi_launch         index of the n = 5 launch with three meshes of different sizes in shuffled pose_model order
  direction_launch     index of the launch whose two directions differ; direction_swapped: adi(gt-posed, estimate-posed)
  symmetric_launch     index of the launch on sym_mesh whose estimate is the ground truth turned by 180 degrees about z

    python tools/gen_adds_golden.py
"""
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference'

SIZES = [1, 2, 63, 255, 256, 257, 511, 512, 513, 600, 1023, 1024, 1025]      # 256-wide tile; 256 / 512 / 1024-wide chunks
MULTI = [(700, 63), (40, 257), (900, 600)]                                     # (start, N) slices of base
MULTI_ORDER = [2, 0, 1, 2, 0]


def rotation(rs, max_angle=np.pi):
    axis = rs.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rs.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx.dot(Kx)


def pose_pair(rs, rot=0.15, shift=0.02):
    """A ground-truth pose in front of the camera and an estimate a few degrees and centimetres off."""
    R_gt = rotation(rs)
    t_gt = np.array([rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2), rs.uniform(0.6, 1.2)])
    R_pr = rotation(rs, rot).dot(R_gt)
    t_pr = t_gt + rs.uniform(-shift, shift, 3)
    return R_gt, t_gt, R_pr, t_pr


def main():
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))      # utils.py:10 imports cv2; never called here
    sys.path.insert(0, REF)
    import utils as ref
    assert os.path.dirname(os.path.abspath(ref.__file__)) == REF

    def score(mesh, R_gt, t_gt, R_pr, t_pr):
        """(adi(est, gt), adi(gt, est), ADD) through the reference's own functions."""
        vertices = np.c_[mesh, np.ones((len(mesh), 1))].transpose()
        gt = ref.compute_transformation(vertices, np.concatenate((R_gt, t_gt.reshape(3, 1)), axis=1))
        pr = ref.compute_transformation(vertices, np.concatenate((R_pr, t_pr.reshape(3, 1)), axis=1))
        add = np.mean(np.linalg.norm(gt - pr, axis=0))
        return ref.adi(pr.T, gt.T), ref.adi(gt.T, pr.T), add

    rs = np.random.RandomState(2024)
    base = rs.uniform(-1, 1, (1500, 3)) * np.array([0.1, 0.1, 0.05]) * rs.uniform(0, 1, (1500, 1)) ** 2
    half = rs.uniform(-1, 1, (200, 3)) * np.array([0.1, 0.1, 0.05])
    sym_mesh = np.concatenate((half, half * np.array([-1.0, -1.0, 1.0])), axis=0)
    arrays = {'base': base, 'sym_mesh': sym_mesh, 'sizes': np.array(SIZES, dtype=np.int32)}
    launches = []          # (mesh source, models, pose_model, poses)

    def add_launch(source, models, pose_model, poses):
        k = len(launches)
        launches.append(k)
        Rt = lambda R, t: np.concatenate((R.reshape(9), t.reshape(3)))
        arrays['models_%d' % k] = np.array(models, dtype=np.int32).reshape(-1, 2)
        arrays['pose_model_%d' % k] = np.array(pose_model, dtype=np.int32)
        arrays['Rt_gt_%d' % k] = np.stack([Rt(p[0], p[1]) for p in poses])
        arrays['Rt_pr_%d' % k] = np.stack([Rt(p[2], p[3]) for p in poses])
        res = [score(source[models[m][0]:models[m][0] + models[m][1]], *p) for m, p in zip(pose_model, poses)]
        arrays['adds_%d' % k] = np.array([r[0] for r in res])
        arrays['add_%d' % k] = np.array([r[2] for r in res])
        return k, res

    for i, N in enumerate(SIZES):                       # n = 1, one mesh, every tile / chunk edge
        add_launch(base, [((37 * i) % (len(base) - N), N)], [0], [pose_pair(rs)])
    arrays['multi_launch'] = np.array(add_launch(base, MULTI, MULTI_ORDER, [pose_pair(rs) for _ in MULTI_ORDER])[0])

    # the direction case: a coarse estimate of a cloud with a dense core - the two directions must differ clearly
    k, res = add_launch(base, [(0, 600)], [0], [pose_pair(rs, rot=0.5, shift=0.04)])
    fwd, swapped = res[0][0], res[0][1]
    assert abs(fwd - swapped) >= 1e-3 * max(fwd, swapped), (fwd, swapped)
    arrays['direction_launch'], arrays['direction_swapped'] = np.array(k), np.array([swapped])

    # the symmetric case: the estimate is the ground truth turned by half a turn about the object's z axis
    R_gt, t_gt, _, _ = pose_pair(rs)
    k, res = add_launch(sym_mesh, [(0, len(sym_mesh))], [0], [(R_gt, t_gt, R_gt.dot(np.diag([-1.0, -1.0, 1.0])), t_gt)])
    assert res[0][0] < 1e-12 and res[0][2] > 0.05, res
    arrays['symmetric_launch'] = np.array(k)
    arrays['launches'] = np.array(len(launches))

    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:      # fixed timestamps: a rerun writes identical bytes
        for name in sorted(arrays):
            b = io.BytesIO()
            np.save(b, arrays[name])
            z.writestr(zipfile.ZipInfo(name + '.npy', (1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)
    with open(os.path.join(GOLD, 'adds.npz'), 'wb') as f:
        f.write(buf.getvalue())
    print('wrote adds.npz: %d launches, %d bytes; direction %.6g vs %.6g; symmetric ADD-S %.3g, ADD %.4f'
          % (len(launches), len(buf.getvalue()), fwd, swapped, res[0][0], res[0][2]))


if __name__ == '__main__':
    main()

"""Inputs shared by the ADD-S tests (test_adds_cpu.py, test_gpu_adds.py): the launches of tests/golden/adds.npz
(tools/gen_adds_golden.py: the reference's adi through its KD-tree) and the brute-force numpy restatement of ADD-S.
Everything here runs on the CPU; the fixture is loaded once per process and never modified."""
import functools

import numpy as np

from helpers import gold


def posed(mesh, Rt):
    """(N,3) mesh under Rt = R (9, row-major) | t (3): R v + t, as compute_transformation does with [R|t] and (v, 1)."""
    return mesh.dot(Rt[:9].reshape(3, 3).T) + Rt[9:]


def brute_adds(pts_est, pts_gt):
    """adi(pts_est, pts_gt) without a tree: for every ground-truth point the distance to the nearest estimated point."""
    diff = pts_gt[:, None, :] - pts_est[None, :, :]
    d2 = (diff * diff).sum(axis=2)
    return np.sqrt(d2.min(axis=1)).mean()


class Launch(object):
    """What one kernel call gets: meshes (list of (N,3)), pose_model (n,), Rt_gt / Rt_pr (n,12), and the reference's
    adds / add (n,)."""

    def __init__(self, g, k):
        source = g['sym_mesh'] if k == int(g['symmetric_launch']) else g['base']
        self.meshes = [np.ascontiguousarray(source[s:s + N]) for s, N in g['models_%d' % k]]
        self.pose_model = g['pose_model_%d' % k]
        self.Rt_gt, self.Rt_pr = g['Rt_gt_%d' % k], g['Rt_pr_%d' % k]
        self.adds, self.add = g['adds_%d' % k], g['add_%d' % k]
        self.n = len(self.pose_model)

    def pose(self, i):
        """(mesh, Rt_gt, Rt_pr) of pose i."""
        return self.meshes[self.pose_model[i]], self.Rt_gt[i], self.Rt_pr[i]

    def R_t(self, Rt):
        return Rt[:, :9].reshape(-1, 3, 3), Rt[:, 9:].reshape(-1, 3, 1)


@functools.lru_cache(maxsize=None)
def fixture():
    g = gold('adds.npz')
    g = {k: g[k] for k in g.files}
    return g, [Launch(g, k) for k in range(int(g['launches']))]


def exact_case(N, seed):
    """Data on which every transformed coordinate and every squared distance is exact in fp64 under ANY contraction:
    vertices and translations are multiples of 2^-10 below 1/4 and 1 in magnitude, rotations are signed permutation
    matrices.  -> (mesh (N,3), Rt_gt (12,), Rt_pr (12,))."""
    rs = np.random.RandomState(seed)
    mesh = rs.randint(-255, 256, (N, 3)) / 1024.0

    def signed_permutation():
        R = np.zeros((3, 3))
        R[np.arange(3), rs.permutation(3)] = rs.choice([-1.0, 1.0], 3)
        return R
    Rt = lambda: np.concatenate((signed_permutation().reshape(9), rs.randint(-64, 65, 3) / 1024.0))
    return mesh, Rt(), Rt()


def rounding_case(n=64, seed=7):
    """One single-vertex mesh under n pose pairs whose rotations are signed permutation matrices, with arbitrary fp64
    vertex and translations: every transformed coordinate is one vertex coordinate plus one translation, rounded once
    under any contraction, so the only place where fusing a product into a sum can show is the squared distance
    (dx*dx + dy*dy) + dz*dz.  With N = 1 the mean is the one distance: the result is fixed to the last bit.
    -> (mesh (1,3), Rt_gt (n,12), Rt_pr (n,12))."""
    rs = np.random.RandomState(seed)
    mesh = rs.uniform(-0.1, 0.1, (1, 3))

    def Rt():
        R = np.zeros((3, 3))
        R[np.arange(3), rs.permutation(3)] = rs.choice([-1.0, 1.0], 3)
        return np.concatenate((R.reshape(9), rs.uniform(-0.3, 0.3, 3)))
    return mesh, np.stack([Rt() for _ in range(n)]), np.stack([Rt() for _ in range(n)])

"""CPU side of ADD-S and the per-class validator: the fixture tests/golden/adds.npz against the brute-force numpy
restatement the GPU tests use, the input conditions its generator asserted, the C ABI table, summarize_multi on a
hand-computed table, and the argument errors, which are raised before anything touches the GPU."""
import os
import re

import numpy as np
import pytest
import torch

import adds_cases as A
import eval_multi_cases as E
from helpers import ROOT


def test_brute_force_reproduces_every_golden_adds():
    """The reference's adi goes through scipy's KD-tree; all pairs in numpy - difference, square, sum over x, y, z, min,
    one root per query, mean - give the same number.  The bar is the GPU tests' bar (1e-13 + 1e-12 * golden)."""
    g, launches = A.fixture()
    sizes = [len(l.meshes[0]) for l in launches[:len(g['sizes'])]]
    assert sizes == g['sizes'].tolist() and {1, 2, 63, 255, 256, 257, 511, 512, 513, 600} <= set(sizes)
    for l in launches:
        for i in range(l.n):
            mesh, Rt_gt, Rt_pr = l.pose(i)
            got = A.brute_adds(A.posed(mesh, Rt_pr), A.posed(mesh, Rt_gt))
            assert abs(got - l.adds[i]) <= 1e-13 + 1e-12 * l.adds[i], (len(mesh), got, l.adds[i])
            add = np.linalg.norm(A.posed(mesh, Rt_gt) - A.posed(mesh, Rt_pr), axis=1).mean()
            assert abs(add - l.add[i]) <= 1e-13 + 1e-12 * l.add[i]
    multi = launches[int(g['multi_launch'])]
    assert multi.n == 5 and len(set(len(m) for m in multi.meshes)) == 3
    assert multi.pose_model.tolist() != sorted(multi.pose_model.tolist())          # shuffled model order


def test_fixture_input_conditions():
    """What the generator asserted, re-checked on the stored data: the two directions of the direction case differ by
    at least 1e-3 relative (a kernel with the point sets swapped cannot pass), and the symmetric case has ADD-S < 1e-12
    while its ADD is above 0.05."""
    g, launches = A.fixture()
    d = launches[int(g['direction_launch'])]
    mesh, Rt_gt, Rt_pr = d.pose(0)
    fwd = A.brute_adds(A.posed(mesh, Rt_pr), A.posed(mesh, Rt_gt))
    swapped = A.brute_adds(A.posed(mesh, Rt_gt), A.posed(mesh, Rt_pr))
    assert abs(fwd - d.adds[0]) <= 1e-12 * fwd and abs(swapped - g['direction_swapped'][0]) <= 1e-12 * swapped
    assert abs(fwd - swapped) >= 1e-3 * max(fwd, swapped)
    s = launches[int(g['symmetric_launch'])]
    assert s.adds[0] < 1e-12 and s.add[0] > 0.05
    mesh, Rt_gt, Rt_pr = s.pose(0)
    assert A.brute_adds(A.posed(mesh, Rt_pr), A.posed(mesh, Rt_gt)) < 1e-12


def test_exact_case_is_exact():
    """The data of the exact-arithmetic GPU test: every coordinate after the transform is a multiple of 2^-10 and every
    squared distance a multiple of 2^-20 below 2, so no operation before the square root rounds."""
    for N in (1, 2, 257, 600):
        mesh, Rt_gt, Rt_pr = A.exact_case(N, N)
        for Rt in (Rt_gt, Rt_pr):
            R = Rt[:9].reshape(3, 3)
            assert np.array_equal(np.abs(R).sum(axis=0), np.ones(3)) and np.array_equal(np.abs(R).sum(axis=1), np.ones(3))
            p = A.posed(mesh, Rt) * 1024.0
            assert np.array_equal(p, np.round(p)) and np.abs(p).max() < 512
        diff = (A.posed(mesh, Rt_gt)[:, None] - A.posed(mesh, Rt_pr)[None]) * 1024.0
        d2 = (diff * diff).sum(axis=2)
        assert np.array_equal(d2, np.round(d2)) and d2.max() < 2 ** 21


def test_rounding_case_tells_fused_from_unfused_arithmetic():
    """The data of the GPU test that pins `(dx*dx + dy*dy) + dz*dz` with every operation rounded on its own: on several
    of its poses each of the two ways a compiler can fuse the sum into FMAs give another distance (exact rational
    arithmetic, rounded where an FMA rounds), so a contracted kernel cannot return the restatement's bits."""
    from fractions import Fraction as Fr
    mesh, Rt_gt, Rt_pr = A.rounding_case()
    differ = [0, 0]
    for g, p in zip(Rt_gt, Rt_pr):
        dx, dy, dz = (A.posed(mesh, g) - A.posed(mesh, p))[0]
        plain = (dx * dx + dy * dy) + dz * dz
        assert np.sqrt(plain) == A.brute_adds(A.posed(mesh, p), A.posed(mesh, g))
        fused_a = float(Fr(dz) * Fr(dz) + Fr(float(Fr(dy) * Fr(dy) + Fr(dx * dx))))        # fma(dz,dz, fma(dy,dy, dx*dx))
        fused_b = float(Fr(dz) * Fr(dz) + Fr(float(Fr(dx) * Fr(dx) + Fr(dy * dy))))        # fma(dz,dz, fma(dx,dx, dy*dy))
        differ[0] += np.sqrt(fused_a) != np.sqrt(plain)
        differ[1] += np.sqrt(fused_b) != np.sqrt(plain)
    assert min(differ) >= 4, differ          # one would do; 7 and more of the 64 do


def test_abi_table_has_the_new_entries():
    from singleshotpose_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ssp_hip.h')).read()
    for name, nargs in (('ssp_pose_errors_models', 11), ('ssp_adds_workspace_doubles', 2), ('ssp_adds_errors', 12)):
        assert name in _lib.exported_symbols()
        decl = re.search(r'(?:int|int64_t) %s\(([^;]*)\);' % name, header).group(1)
        assert len(_lib._SIGS[name]) == len(decl.split(',')) == nargs
    assert _lib.query('ssp_abi_version') == 5
    # the workspace: one double per (pose, chunk of query vertices); nothing for an empty launch
    q = lambda n, N: _lib.query('ssp_adds_workspace_doubles', n, N)
    chunk = next(c for c in (256, 512, 1024) if q(1, c) == 1 and q(1, c + 1) == 2)
    assert q(5, 600) == 5 * -(-600 // chunk) and q(128, 5841) == 128 * -(-5841 // chunk)
    assert q(0, 600) == 0 and q(3, 0) == 0 and q(1, 1) == 1
    # the fixture has a mesh at chunk - 1, chunk and chunk + 1
    assert {chunk - 1, chunk, chunk + 1} <= set(A.fixture()[0]['sizes'].tolist())


def test_summarize_multi_on_a_hand_computed_table():
    """Six rows: class 1 (diameter 0.1) rows 0-2, class 4 (diameter 0.2, symmetric: column 4 filled) rows 3-5 of which row
    5 has NaN in column 4 and falls back to vertex_dist; class 9 has a diameter and no rows."""
    from singleshotpose_amd.utils_multi import MultiEval, summarize_multi
    nan = float('nan')
    errors = np.array([
        # pixel  ADD     trans  angle  ADD-S
        [3.0,    0.009,  0.04,  4.0,   nan],      # class 1: px yes, add yes (<= 0.01), 5cm5deg yes
        [5.0,    0.011,  0.05,  5.0,   nan],      # class 1: px yes (<=), add no, 5cm5deg yes (<= on both)
        [7.0,    0.010,  0.06,  1.0,   nan],      # class 1: px no, add yes (<=), 5cm5deg no (translation)
        [1.0,    0.150,  0.01,  9.0,   0.015],    # class 4: px yes, ADD-S 0.015 <= 0.02 yes (ADD would say no), no (angle)
        [6.0,    0.010,  0.01,  1.0,   0.025],    # class 4: px no, ADD-S 0.025 no (ADD would say yes), 5cm5deg yes
        [2.0,    0.019,  0.02,  2.0,   nan],      # class 4: px yes, column 4 NaN -> ADD 0.019 yes, 5cm5deg yes
    ])
    z = np.zeros
    ev = MultiEval(z(6, dtype=np.int64), np.arange(6), np.array([1, 1, 1, 4, 4, 4]), np.ones(6, dtype=np.int64),
                   z((6, 9, 2), dtype=np.float32), z(6, dtype=np.float32), z((6, 3, 3)), z((6, 3, 1)), z((6, 3, 3)),
                   z((6, 3, 1)), errors)
    res = summarize_multi(ev, {1: 0.1, 4: 0.2, 9: 0.3})
    assert sorted(res) == [1, 4, 9]
    pct = lambda k: k * 100. / (3 + 1e-5)
    assert res[1] == dict(count=3, acc_px=pct(2), acc_add=pct(2), acc_cm_deg=pct(2))
    assert res[4] == dict(count=3, acc_px=pct(2), acc_add=pct(2), acc_cm_deg=pct(2))
    assert res[9] == dict(count=0, acc_px=0.0, acc_add=0.0, acc_cm_deg=0.0)
    # other thresholds; a four-column result (no symmetric classes) uses vertex_dist everywhere
    res = summarize_multi(ev, {4: 0.2}, px=1.0, add_frac=0.05, cm=0.015, deg=10.0)
    assert res == {4: dict(count=3, acc_px=pct(1), acc_add=pct(0), acc_cm_deg=pct(2))}
    res = summarize_multi(ev._replace(errors=errors[:, :4]), {4: 0.2})
    assert res[4]['acc_add'] == pct(2) and res[4]['count'] == 3          # rows 4 and 5 by ADD; row 3 (0.15) fails


def test_argument_errors_are_raised_before_the_gpu():
    """Every ValueError case, on this machine's CPU: raised before a tensor is moved or a kernel is looked up (the head
    passed to evaluate_multi_batched is a CPU tensor, which the function would refuse with a RuntimeError next)."""
    from singleshotpose_amd import utils as U
    from singleshotpose_amd.utils_multi import evaluate_multi_batched
    rs = np.random.RandomState(0)
    mesh3, mesh4 = rs.uniform(-1, 1, (3, 20)), np.concatenate((rs.uniform(-1, 1, (3, 30)), np.ones((1, 30))))
    R, t = np.stack([np.eye(3)] * 4), np.zeros((4, 3, 1))
    Kc = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.5704, 242.0489], [0.0, 0.0, 1.0]])
    # adi_batched: a mesh that is not (3|4, N); mismatched pose counts
    for bad in (np.zeros((5, 20)), np.zeros(20), np.zeros((3, 0)), np.zeros((2, 3, 20))):
        with pytest.raises(ValueError, match=r"\(3,N\) or \(4,N\)"):
            U.adi_batched(bad, R, t, R, t)
    for args in ((R[:3], t, R, t), (R, t[:3], R, t), (R, t, R[:2], t), (R, t, R, t[:1])):
        with pytest.raises(ValueError, match="same number of poses"):
            U.adi_batched(mesh3, *args)
    # pose_errors_models_batched: no model, a bad mesh, counts, model_index out of range, a symmetric id without a model
    pem = U.pose_errors_models_batched
    with pytest.raises(ValueError, match="no object model"):
        pem([], [], R[:0], t[:0], R[:0], t[:0], Kc)
    with pytest.raises(ValueError, match=r"\(3,N\) or \(4,N\)"):
        pem([mesh3, np.zeros((2, 9))], [0, 1, 0, 1], R, t, R, t, Kc)
    with pytest.raises(ValueError, match="same number of poses"):
        pem([mesh3, mesh4], [0, 1, 0, 1], R, t, R[:3], t, Kc)
    with pytest.raises(ValueError, match="one entry per pose"):
        pem([mesh3, mesh4], [0, 1, 0], R, t, R, t, Kc)
    for idx in ([0, 1, 2, 0], [0, -1, 0, 0]):
        with pytest.raises(ValueError, match=r"in \[0, 2\)"):
            pem([mesh3, mesh4], idx, R, t, R, t, Kc)
    with pytest.raises(ValueError, match="symmetric"):
        pem([mesh3, mesh4], [0, 1, 0, 1], R, t, R, t, Kc, symmetric=[2])
    with pytest.raises(ValueError, match=r"\(3,3\) or \(n,3,3\)"):
        pem([mesh3, mesh4], [0, 1, 0, 1], R, t, R, t, np.stack([Kc] * 3))
    # evaluate_multi_batched: an empty mapping, a bad mesh, a symmetric id without a model (also with a single mesh)
    case = E.small_case()
    head, target = torch.from_numpy(case.head), torch.from_numpy(case.target)
    ev = lambda vertices, **kw: evaluate_multi_batched(head, target, case.conf_thresh, case.nC, E.K, E.ANCHORS[:4], case.nA,
                                                       vertices, Kc, *case.im_size, **kw)
    with pytest.raises(ValueError, match="no object model"):
        ev({})
    with pytest.raises(ValueError, match=r"\(3,N\) or \(4,N\)"):
        ev({0: mesh3, 1: np.zeros((20, 3))})
    with pytest.raises(ValueError, match="symmetric"):
        ev({0: mesh3, 1: mesh4}, symmetric=[2])
    with pytest.raises(ValueError, match="symmetric"):
        ev(mesh4, symmetric=[0])
    # ... and with valid arguments the same call gets as far as the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev({0: mesh3, 1: mesh4}, symmetric=[1])


def test_new_names_resolve_through_the_dropin_shims(tmp_path):
    """`PYTHONPATH=repo:repo/dropin` as the reference's scripts are run: the new names sit next to their neighbours."""
    import subprocess
    import sys
    code = r'''
import os, sys
import utils
for n in "adi adi_batched adds_device pose_errors_batched pose_errors_models_batched".split():
    assert callable(getattr(utils, n)), n
sys.path.insert(0, os.path.join(r"%s", "dropin", "multi_obj_pose_estimation"))
import utils_multi
for n in "evaluate_multi_batched summarize_multi adi_batched pose_errors_models_batched".split():
    assert callable(getattr(utils_multi, n)), n
print("ok")
''' % ROOT
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'dropin')]))
    out = subprocess.run([sys.executable, '-c', code], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('ok'), out.stderr[-2000:]

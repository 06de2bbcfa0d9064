"""ADD-S (ssp_adds_errors) and the per-mesh pose errors (ssp_pose_errors_models) on the GPU against the reference's own
adi numbers (tests/golden/adds.npz, through scipy's KD-tree), the brute-force numpy restatement on exact data, and the
single-mesh kernel.  Inputs: adds_cases.py."""
import numpy as np
import pytest
import torch

import adds_cases as A

pytestmark = pytest.mark.gpu

KC = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.5704, 242.0489], [0.0, 0.0, 1.0]])


def _device_launch(meshes, pose_model, Rt_gt, Rt_pr):
    """adds_device on one launch of the fixture: (n,) float64 device tensor."""
    from singleshotpose_amd import utils as U
    dev = torch.device('cuda', torch.cuda.current_device())
    v = torch.as_tensor(np.ascontiguousarray(np.concatenate(meshes, axis=0))).to(dev)
    off = torch.as_tensor(np.concatenate(([0], np.cumsum([len(m) for m in meshes]))).astype(np.int32)).to(dev)
    return U.adds_device(v, off, torch.as_tensor(np.asarray(pose_model, dtype=np.int32)).to(dev),
                         torch.as_tensor(np.ascontiguousarray(Rt_pr)).to(dev), torch.as_tensor(np.ascontiguousarray(Rt_gt)).to(dev))


@pytest.fixture(scope='module')
def device_results():
    """adds_device once per launch of the fixture, shared by the tests: list of (n,) float64 ndarrays."""
    _, launches = A.fixture()
    return [_device_launch(l.meshes, l.pose_model, l.Rt_gt, l.Rt_pr).cpu().numpy() for l in launches]


def test_golden_adds_device_and_adi_batched(device_results):
    """Every launch of the fixture - N = 1, 2, 63, 255, 256, 257, 511, 512, 513, 600, 1023, 1024, 1025 at n = 1 (the edges
    of the 256-wide tile and of a 256-, 512- or 1024-wide chunk), and n = 5 over three meshes in shuffled model order -
    against the reference's adi.  Bar |gpu - golden| <= 1e-13 + 1e-12 * golden: coordinates are below 2 m, a four-term fp64
    transform errs by about 1e-15 m in any contraction order, a distance by a few times that and the mean by no more; the
    bar is some 25 times above, and a nearest-neighbour flip at a near-tie moves the minimum continuously."""
    from singleshotpose_amd import utils as U
    g, launches = A.fixture()
    assert len(launches) == len(device_results) >= 16
    for l, got in zip(launches, device_results):
        assert got.shape == (l.n,) and got.dtype == np.float64
        print('N %s  gpu - golden %s' % ([len(m) for m in l.meshes], (got - l.adds).tolist()))
        assert np.all(np.abs(got - l.adds) <= 1e-13 + 1e-12 * l.adds), (got, l.adds)
    # adi_batched: the host form, estimate first as the reference's adi; one mesh per call
    for k in list(range(len(g['sizes']))) + [int(g['direction_launch'])]:
        l = launches[k]
        R_gt, t_gt = l.R_t(l.Rt_gt)
        R_pr, t_pr = l.R_t(l.Rt_pr)
        for vertices in (l.meshes[0].T, np.concatenate((l.meshes[0].T, np.ones((1, len(l.meshes[0])))))):      # (3,N), (4,N)
            got = U.adi_batched(vertices, R_pr, t_pr, R_gt, t_gt)
            assert got.shape == (1,) and got.dtype == np.float64
            assert np.array_equal(got, device_results[k])                 # the same launch: the same bits
    multi = launches[int(g['multi_launch'])]
    mesh = multi.meshes[2]
    rows = np.nonzero(multi.pose_model == 2)[0]
    got = U.adi_batched(mesh.T, *(multi.R_t(multi.Rt_pr[rows]) + multi.R_t(multi.Rt_gt[rows])))
    assert len(rows) == 2 and np.array_equal(got, device_results[int(g['multi_launch'])][rows])
    assert U.adi_batched(mesh.T, np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3))).shape == (0,)


@pytest.mark.parametrize('N', [1, 2, 255, 256, 257, 511, 512, 513, 600, 1025])
def test_exact_data_equals_the_numpy_restatement(N):
    """Vertices and translations multiples of 2^-10, rotations signed permutation matrices: every transformed coordinate
    and every squared distance is exact under any contraction, the square root is correctly rounded, so only the
    summation order of the mean is left: <= N * 2^-52 (exactly equal at N = 1)."""
    mesh, Rt_gt, Rt_pr = A.exact_case(N, N)
    want = A.brute_adds(A.posed(mesh, Rt_pr), A.posed(mesh, Rt_gt))
    got = float(_device_launch([mesh], [0], Rt_gt[None], Rt_pr[None]).cpu().numpy()[0])
    print('N %d  gpu %r  numpy %r  diff %.3g' % (N, got, want, got - want))
    assert want > 0 and abs(got - want) <= N * 2.0 ** -52
    if N == 1:
        assert got == want


def test_squared_distance_is_not_contracted():
    """(dx*dx + dy*dy) + dz*dz with every product and sum rounded on its own, the arithmetic of the numpy restatement:
    on single-vertex data whose transforms round once under any contraction (adds_cases.rounding_case; its CPU test
    shows that a fused sum changes the result on many of the poses) the kernel returns the restatement's bits."""
    mesh, Rt_gt, Rt_pr = A.rounding_case()
    got = _device_launch([mesh], np.zeros(len(Rt_gt), dtype=np.int32), Rt_gt, Rt_pr).cpu().numpy()
    want = np.array([A.brute_adds(A.posed(mesh, p), A.posed(mesh, g)) for g, p in zip(Rt_gt, Rt_pr)])
    print('poses with other bits: %d of %d' % (int((got != want).sum()), len(want)))
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_direction_is_the_references(device_results):
    """adi(est, gt): the tree on the estimate, the queries from the ground truth.  The stored case differs by more than
    1e-3 relative between the two directions; the kernel matches the first and, with the poses swapped, the second."""
    g, launches = A.fixture()
    k = int(g['direction_launch'])
    l, got = launches[k], device_results[k][0]
    swapped = float(g['direction_swapped'][0])
    assert abs(got - l.adds[0]) <= 1e-13 + 1e-12 * l.adds[0]
    assert abs(got - swapped) >= 0.5e-3 * swapped
    back = _device_launch(l.meshes, l.pose_model, l.Rt_pr, l.Rt_gt).cpu().numpy()[0]       # estimate and ground truth swapped
    assert abs(back - swapped) <= 1e-13 + 1e-12 * swapped


def test_half_turn_of_a_symmetric_mesh(device_results):
    """The estimate is the ground truth turned by 180 degrees about the axis the mesh is symmetric under: ADD-S < 1e-12
    while ADD (column 1 of the same row) is above 0.05."""
    from singleshotpose_amd import utils as U
    g, launches = A.fixture()
    k = int(g['symmetric_launch'])
    l = launches[k]
    assert device_results[k][0] < 1e-12
    R_gt, t_gt = l.R_t(l.Rt_gt)
    R_pr, t_pr = l.R_t(l.Rt_pr)
    row = U.pose_errors_models_batched([l.meshes[0].T], [0], R_gt, t_gt, R_pr, t_pr, KC, symmetric=[0])[0]
    assert row[4] < 1e-12 and row[1] > 0.05
    assert abs(row[1] - l.add[0]) <= 1e-13 + 1e-12 * l.add[0]


def test_two_launches_give_equal_bits(device_results):
    g, launches = A.fixture()
    for k in (int(g['multi_launch']), len(g['sizes']) - 1):
        l = launches[k]
        again = _device_launch(l.meshes, l.pose_model, l.Rt_gt, l.Rt_pr).cpu().numpy()
        assert np.array_equal(again.view(np.int64), device_results[k].view(np.int64))


def test_short_workspace_is_refused_and_nothing_is_launched():
    from singleshotpose_amd import _lib
    g, launches = A.fixture()
    l = launches[int(g['multi_launch'])]
    dev = torch.device('cuda', torch.cuda.current_device())
    v = torch.as_tensor(np.concatenate(l.meshes, axis=0)).to(dev)
    off = torch.as_tensor(np.concatenate(([0], np.cumsum([len(m) for m in l.meshes]))).astype(np.int32)).to(dev)
    pm = torch.as_tensor(l.pose_model.astype(np.int32)).to(dev)
    Rt_gt, Rt_pr = torch.as_tensor(l.Rt_gt).to(dev), torch.as_tensor(l.Rt_pr).to(dev)
    maxN = max(len(m) for m in l.meshes)
    words = _lib.query('ssp_adds_workspace_doubles', l.n, maxN)
    assert words >= l.n
    work = torch.full((words,), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((l.n,), -7.0, dtype=torch.float64, device=dev)
    args = lambda count: (v.data_ptr(), off.data_ptr(), pm.data_ptr(), len(l.meshes), maxN, Rt_gt.data_ptr(), Rt_pr.data_ptr(),
                          l.n, out.data_ptr(), work.data_ptr(), count, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.SspError, match="workspace"):
        _lib.call('ssp_adds_errors', *args(words - 1))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((work == -7.0).all())          # nothing ran
    with pytest.raises(_lib.SspError, match="nM > 0"):
        _lib.call('ssp_adds_errors', *(args(words)[:3] + (0,) + args(words)[4:]))
    _lib.call('ssp_adds_errors', *args(words))                                # the exact size is enough
    assert np.all(np.abs(out.cpu().numpy() - l.adds) <= 1e-13 + 1e-12 * l.adds)


def test_pose_errors_models_against_the_single_mesh_kernel():
    """One model: the bits of ssp_pose_errors on the same poses.  Three models: every row has the bits of a single-mesh
    call on that row's mesh.  Column 4 is NaN exactly on the rows of a non-symmetric mesh, ADD-S on the others."""
    from singleshotpose_amd import _lib
    from singleshotpose_amd import utils as U
    g, launches = A.fixture()
    l = launches[int(g['multi_launch'])]
    R_gt, t_gt = l.R_t(l.Rt_gt)
    R_pr, t_pr = l.R_t(l.Rt_pr)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    one = U.pose_errors_models_batched([l.meshes[1].T], np.zeros(l.n, dtype=np.int64), R_gt, t_gt, R_pr, t_pr, KC)
    single = U.pose_errors_batched(l.meshes[1].T, R_gt, t_gt, R_pr, t_pr, KC)
    assert one.shape == (l.n, 5) and single.shape == (l.n, 4)
    assert np.array_equal(bits(one[:, :4]), bits(single)) and np.all(np.isnan(one[:, 4]))
    three = U.pose_errors_models_batched([m.T for m in l.meshes], l.pose_model, R_gt, t_gt, R_pr, t_pr, KC, symmetric=(2, 0))
    for m, mesh in enumerate(l.meshes):
        rows = np.nonzero(l.pose_model == m)[0]
        assert len(rows) >= 1
        per_mesh = U.pose_errors_batched(mesh.T, R_gt[rows], t_gt[rows], R_pr[rows], t_pr[rows], KC)
        assert np.array_equal(bits(three[rows, :4]), bits(per_mesh)), m
    assert np.array_equal(np.isnan(three[:, 4]), l.pose_model == 1)
    sym = l.pose_model != 1
    assert np.all(np.abs(three[sym, 4] - l.adds[sym]) <= 1e-13 + 1e-12 * l.adds[sym])
    assert np.all(np.abs(three[:, 1] - l.add) <= 1e-13 + 1e-12 * l.add)
    per_pose_K = U.pose_errors_models_batched([m.T for m in l.meshes], l.pose_model, R_gt, t_gt, R_pr, t_pr,
                                              np.broadcast_to(KC, (l.n, 3, 3)))
    assert np.array_equal(bits(per_pose_K[:, :4]), bits(three[:, :4])) and np.all(np.isnan(per_pose_K[:, 4]))
    # nM <= 0 is refused on the host side of the launch
    dev = torch.device('cuda', torch.cuda.current_device())
    z = torch.zeros(16, dtype=torch.float64, device=dev)
    zi = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.SspError, match="nM > 0"):
        _lib.call('ssp_pose_errors_models', z.data_ptr(), zi.data_ptr(), zi.data_ptr(), 0, z.data_ptr(), z.data_ptr(),
                  z.data_ptr(), 0, 1, z.data_ptr(), torch.cuda.current_stream().cuda_stream)

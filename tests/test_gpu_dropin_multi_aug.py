"""The reference's UNMODIFIED train_multi.py on the MI355X with the multi-object data path on the GPU as well: only
train_multi.py and MeshPly.py are staged next to the driver, so `import dataset_multi` (train_multi.py:24) and its
`from image_multi import *` resolve to dropin/multi_obj_pose_estimation/ - every batch is augmented inside the script's own
`data = data.cuda()` (train_multi.py:74).  Same run, same golden numbers and same bars as
tests/test_gpu_dropin.py::test_unmodified_train_multi_py_runs_and_matches_the_cpu_reference, which keeps the reference's
host pipeline: the first-batch bar is reachable only if pixels, labels and the random stream are the reference's."""
import json
import os
import subprocess
import sys
import zipfile

import pytest

from helpers import GOLD, ROOT

pytestmark = pytest.mark.gpu
MULTI_SHIMS = os.path.join(ROOT, 'dropin', 'multi_obj_pose_estimation')


def _callers_dir(tmp_path):
    dst = str(tmp_path / 'multi_callers_without_dataset')
    os.makedirs(dst, exist_ok=True)
    z = os.path.join(ROOT, 'oracle', '_ref', 'callers.zip')
    if not os.path.isfile(z) or 'multi_obj_pose_estimation/train_multi.py' not in zipfile.ZipFile(z).namelist():
        pytest.skip("the reference's multi-object driver scripts are not staged (oracle/_ref/callers.zip: run "
                    "__graft_entry__.build() in the build container, where /root/reference exists)")
    with zipfile.ZipFile(z) as f:
        with open(os.path.join(dst, 'train_multi.py'), 'wb') as o:
            o.write(f.read('multi_obj_pose_estimation/train_multi.py'))
        f.extract('MeshPly.py', dst)
    return dst


def _close(a, b, rel, abs_=0.0):
    return abs(a - b) <= abs_ + rel * abs(b)


def test_unmodified_train_multi_py_with_the_gpu_data_path_matches_the_cpu_reference(tmp_path):
    import fixture_occlusion as fo
    gold = json.load(open(os.path.join(GOLD, 'dropin_multi.json')))['train']
    ref = _callers_dir(tmp_path)
    assert sorted(os.listdir(ref)) == ['MeshPly.py', 'train_multi.py']
    info = fo.make(str(tmp_path / 'fixture'))
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([MULTI_SHIMS, ROOT, os.path.join(ROOT, 'dropin')])
    env['PYTHONUNBUFFERED'] = '1'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_pinned.py'), os.path.join(ref, 'train_multi.py'),
                        '--datacfg', 'cfg/occlusion.data', '--modelcfg', 'cfg/yolo-pose-multi.cfg', '--initweightfile',
                        'init.weights'], cwd=info['cwd'], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    got = fo.parse_train_output(p.stdout)
    print(json.dumps(got['steps']))
    assert got['epochs'] == gold['epochs']
    assert len(got['steps']) == len(gold['steps']) == 2
    for i, (a, b, b1) in enumerate(zip(got['steps'], gold['steps'], gold['steps_one_thread'])):
        assert (a['seen'], a['nGT']) == (b['seen'], b['nGT']) == (4 * (i + 1), 32)
        for k in ('loss_x', 'loss_y', 'loss_conf', 'loss_cls', 'total'):
            if i == 0:
                assert _close(a[k], b[k], 1e-4, 1e-5), (i, k, a[k], b[k])
            else:      # 3x the reference's own run-to-run spread + 0.5 %: the bar of the existing test, for its reasons
                spread = abs(b1[k] - b[k])
                assert abs(a[k] - b[k]) <= 3.0 * spread + 5e-3 * abs(b[k]), (i, k, a[k], b[k], spread)
        if i == 0:
            assert a['recall'] == b['recall'] and abs(a['proposals'] - b['proposals']) <= 2, (a, b)

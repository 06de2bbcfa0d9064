"""Writes tests/golden/generic_{pose,cls,strided}.npz: the reference Darknet (imported read-only, as oracle/gen_golden.py
does) run on the cfgs that exercise the blocks outside the yolo-pose path - shortcut, stride-1 max-pool, non-BN relu / leaky
convolutions (generic-pose.cfg); avgpool, connected, softmax, cost (generic-cls.cfg); stride-2 convolutions, 3x3 and 1x1, on
even and odd maps (generic-strided.cfg).

Build machine only (the reference is not on the GPU machines); only the data it writes is committed.  Each file holds:
  weights           the seeded .weights byte stream (uint8), loaded by both sides
  x                 the input (B, 3, H, W)
  y_eval, y_train   eval / training-mode forward outputs
  buf/<name>        BatchNorm running statistics after the training forward
  probe             the tensor the training output is contracted with: loss = (y * probe).sum()
  grad/ | gslice/   every parameter gradient of that loss in fp32 (whole, or an even slice of big ones), gnorm/ its norm
  g64/ | g64slice/  the same step in float64 (model.double()), g64norm/ its norm
  keys, shapes      the reference's state_dict keys and shapes

Deterministic: fixed seeds, one CPU thread, and zip entries with a fixed timestamp - a rerun writes byte-identical files.

    python tools/gen_generic_blocks_golden.py
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)

CASES = (        # tag, cfg, B, H, W, weight seed, input seed
    ('pose', 'generic-pose.cfg', 2, 80, 80, 31, 131),
    ('cls', 'generic-cls.cfg', 4, 64, 64, 32, 132),
    ('strided', 'generic-strided.cfg', 2, 40, 44, 33, 133),
)
NSLICE = 512


def seeded_weights(blocks, models, seed):
    """A .weights stream (header + per conv / connected block, in the order cfg.py's loaders read) of deterministic values:
    filters / Linear weights ~ N(0, 1) * 1.5 / sqrt(fan_in), biases and BN shifts ~ N(0, 0.1), BN scales and running
    variances ~ U(0.5, 1.5), running means ~ N(0, 0.1)."""
    rs = np.random.RandomState(seed)
    parts = [np.array([0, 0, 0, 0], dtype=np.int32).tobytes()]
    f32 = lambda a: a.astype(np.float32).tobytes()
    for ind, b in enumerate(blocks[1:]):
        t = b['type']
        if t == 'convolutional':
            conv = models[ind][0]
            cout, fan_in = conv.weight.shape[0], conv.weight[0].numel()
            if int(b['batch_normalize']):
                parts.append(f32(rs.standard_normal(cout) * 0.1))          # bn.bias
                parts.append(f32(rs.uniform(0.5, 1.5, cout)))               # bn.weight
                parts.append(f32(rs.standard_normal(cout) * 0.1))          # running_mean
                parts.append(f32(rs.uniform(0.5, 1.5, cout)))               # running_var
            else:
                parts.append(f32(rs.standard_normal(cout) * 0.1))          # conv.bias
            parts.append(f32(rs.standard_normal(tuple(conv.weight.shape)) * (1.5 / np.sqrt(fan_in))))
        elif t == 'connected':
            m = models[ind]
            lin = m if isinstance(m, torch.nn.Linear) else m[0]
            cout, cin = lin.weight.shape
            parts.append(f32(rs.standard_normal(cout) * 0.1))
            parts.append(f32(rs.standard_normal((cout, cin)) * (1.5 / np.sqrt(cin))))
    return b''.join(parts)


def grads_of(model, whole, part, norm):
    """Gradient of every parameter under key `whole` (<= 4096 elements) or an even slice of it under `part`, its norm
    under `norm` (the key names oracle/gen_golden.py's files use)."""
    rec = {}
    for n, p in model.named_parameters():
        g = p.grad.numpy()
        rec[norm + n] = np.array([np.sqrt((g.astype(np.float64) ** 2).sum())])
        if g.size <= 4096:
            rec[whole + n] = g
        else:
            rec[part + n] = g.reshape(-1)[:: max(1, g.size // NSLICE)][:NSLICE].copy()
    return rec


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps (byte-identical reruns)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def run_case(ref_darknet, tag, cfg, B, H, W, wseed, xseed):
    cfgfile = os.path.join(GOLD, cfg)
    with contextlib.redirect_stdout(io.StringIO()):
        model = ref_darknet.Darknet(cfgfile)
    stream = seeded_weights(model.blocks, model.models, wseed)
    with tempfile.TemporaryDirectory() as td:
        wpath = os.path.join(td, 'w.weights')
        with open(wpath, 'wb') as f:
            f.write(stream)
        model.load_weights(wpath)
        with contextlib.redirect_stdout(io.StringIO()):
            m64 = ref_darknet.Darknet(cfgfile)
        m64.load_weights(wpath)
    sd = model.state_dict()
    rec = dict(weights=np.frombuffer(stream, dtype=np.uint8).copy(),
               keys=np.array(list(sd.keys())),
               shapes=np.array(json.dumps([list(v.shape) for v in sd.values()])))
    rs = np.random.RandomState(xseed)
    x = rs.uniform(0, 1, (B, 3, H, W)).astype(np.float32)
    rec['x'] = x
    model.eval()
    with torch.no_grad():
        rec['y_eval'] = model(torch.from_numpy(x)).numpy()
    model.train()
    y = model(torch.from_numpy(x))
    probe = rs.standard_normal(tuple(y.shape)).astype(np.float32)
    (y * torch.from_numpy(probe)).sum().backward()
    rec['y_train'] = y.detach().numpy()
    rec['probe'] = probe
    rec.update(grads_of(model, 'grad/', 'gslice/', 'gnorm/'))
    for n, b in model.named_buffers():
        if 'running' in n:
            rec['buf/' + n] = b.numpy().copy()
    m64 = m64.double().train()
    y64 = m64(torch.from_numpy(x).double())
    (y64 * torch.from_numpy(probe).double()).sum().backward()
    rec['y_train64'] = y64.detach().numpy()
    rec.update(grads_of(m64, 'g64/', 'g64slice/', 'g64norm/'))
    out = os.path.join(GOLD, 'generic_%s.npz' % tag)
    save_npz(out, rec)
    print('generic', tag, tuple(rec['y_eval'].shape), 'max|y_eval| %.4g' % float(np.abs(rec['y_eval']).max()), out)


def main():
    from oracle.gen_golden import import_reference
    torch.set_num_threads(1)
    _, _, ref_darknet = import_reference()
    for case in CASES:
        run_case(ref_darknet, *case)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Generate tests/golden/smplx_rot.npz FROM THE REFERENCE'S OWN rotation conversion and L1div.

Run where the reference tree is available (default /root/reference, or MOTIONCRAFT_REFERENCE):

    python tests/golden/make_golden_smplx.py

The SMPL-X package and its model file are not available, and the reference only calls them; two neighbouring pieces of the
reference itself pin what can be pinned:

  * ``rot.axis_angle`` [N,3] / ``rot.matrix`` [N,3,3]: ``mogen/datasets/EMAGE_2024/utils/rotation_conversions.py``'s
    ``axis_angle_to_matrix`` (pure torch, loaded by file path) in float64, on random directions at angles from 1e-6 to
    pi - 1e-6 (log-spaced below 1e-2, uniform above) and on exact zeros.  ``rot.angle`` holds the angles.
  * ``l1div.joints<i>`` [frames,165] float32 / ``l1div.avg_after<i>``: the reference's ``L1div`` (``utils/metric.py:12-27``)
    run over three small joint sequences, its ``avg()`` after each; ``librosa`` / ``matplotlib`` are stubbed in ``sys.modules`` (the module imports them at the
    top and L1div uses neither).  ``run`` overwrites its argument, so it is fed copies.

The fixture holds data only and is written with fixed zip timestamps: a re-run reproduces it byte for byte.
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('MOTIONCRAFT_REFERENCE', '/root/reference')
UTILS = os.path.join(REF, 'mogen', 'datasets', 'EMAGE_2024', 'utils')


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_metric():
    stubs = {}
    for name in ('librosa', 'librosa.display', 'matplotlib', 'matplotlib.pyplot'):
        stubs[name] = types.ModuleType(name)
    stubs['librosa'].display = stubs['librosa.display']
    stubs['matplotlib'].pyplot = stubs['matplotlib.pyplot']
    stubs['matplotlib.pyplot'].figure = lambda *a, **k: None
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        return load_by_path('ref_emage_metric', os.path.join(UTILS, 'metric.py'))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def write_npz(path, arrays):
    """np.savez_compressed with fixed entry timestamps (byte-reproducible)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    rc = load_by_path('ref_rotation_conversions', os.path.join(UTILS, 'rotation_conversions.py'))
    rs = np.random.RandomState(2024)
    angle = np.concatenate([np.logspace(-6, -2, 96), rs.uniform(1e-2, np.pi - 1e-3, 128),
                            np.pi - np.logspace(-6, -3, 24), [1e-6, 1e-4, np.pi - 1e-6]])
    d = rs.randn(angle.size, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    aa = np.concatenate([d * angle[:, None], np.zeros((4, 3))])
    angle = np.concatenate([angle, np.zeros(4)])
    mat = rc.axis_angle_to_matrix(torch.from_numpy(aa)).numpy()
    assert mat.dtype == np.float64 and mat.shape == (aa.shape[0], 3, 3)
    out = {'rot.axis_angle': aa, 'rot.angle': angle, 'rot.matrix': mat}

    metric = load_metric()
    calc = metric.L1div()
    seqs = []
    for i, frames in enumerate((34, 60, 7)):
        j = (0.5 * np.random.RandomState(300 + i).randn(frames, 165) + np.linspace(-1, 1, 165)).astype(np.float32)
        seqs.append(j)
        calc.run(j.copy())
        out[f'l1div.joints{i}'] = j
        out[f'l1div.avg_after{i}'] = np.float64(calc.avg())
    out['l1div.count'] = np.int64(len(seqs))
    write_npz(os.path.join(OUT, 'smplx_rot.npz'), out)
    print(f'rotations: {aa.shape[0]} (angles {angle[angle > 0].min():.1e} .. pi - {np.pi - angle.max():.1e}, 4 zeros); '
          f'L1div after each sequence: {[float(out[f"l1div.avg_after{i}"]) for i in range(len(seqs))]}')


if __name__ == '__main__':
    main()

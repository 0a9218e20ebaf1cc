"""``tools/sample.py --anim_dir`` and ``tools/skeleton_npy.py``: the argument errors on the host, and on the MI355X the frames both
write for one sample, which must be the same pictures."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_ref
from helpers import HML_SMALL
from motioncraft_amd import postprocess as P
from motioncraft_amd import skeleton as sk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAMPLE = [sys.executable, os.path.join(ROOT, 'tools', 'sample.py')]
NPY = [sys.executable, os.path.join(ROOT, 'tools', 'skeleton_npy.py')]


def test_tools_list_and_check_the_animation_arguments(tmp_path):
    r = subprocess.run(SAMPLE + ['--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and all(f in r.stdout for f in ('--anim_dir', '--anim_size', '--anim_fps'))
    bad = str(tmp_path / 'bad.npy')
    np.save(bad, np.zeros((4, 23, 3), np.float32))
    r = subprocess.run(NPY + [bad, '--out', str(tmp_path / 'o')], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '23 joints' in r.stderr
    r = subprocess.run(NPY + [bad, '--out', str(tmp_path / 'o'), '--anim_size', '5000x10'], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '--anim_size' in r.stderr
    assert not os.path.exists(str(tmp_path / 'o'))


@pytest.mark.gpu
def test_sample_tool_draws_the_animation_and_the_npy_tool_draws_it_again(tmp_path):
    from motioncraft_amd import synthetic
    schedule = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
    model = dict(type='MotionDiffusion', model=synthetic.reference_model_cfg(HML_SMALL),
                 loss_recon=dict(type='MSELoss', loss_weight=1, reduction='none'), diffusion_train=schedule,
                 diffusion_test=dict(schedule, respace='15,15,8,6,6'), inference_type='ddim', loss_reduction='batch')
    cfg = tmp_path / 'hml_small.py'
    cfg.write_text(f'model = {model!r}\n')
    pose, anim, again = str(tmp_path / 'joints.npy'), str(tmp_path / 'anim'), str(tmp_path / 'again')
    args = ['synthetic:3', '--random-condition', '5', '--out', str(tmp_path), '--text', 'a person walks', 'a dancer spins',
            '--motion_length', '10', '7', '--pose_npy', pose, '--anim_dir', anim, '--anim_size', '64x48']
    r = subprocess.run(SAMPLE + [str(cfg)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'drew 17 frames' in r.stdout, r.stderr[-2000:]
    frames = np.stack([raster_ref.read_bmp(os.path.join(anim, f'frame_{i}.bmp')) for i in range(17)])
    assert frames.shape == (17, 48, 64, 3) and not os.path.exists(os.path.join(anim, 'frame_17.bmp'))
    renderer = sk.SkeletonRenderer(sk.T2M_CHAINS, width=64, height=48)
    want = renderer.render(torch.from_numpy(np.load(pose)).cuda()).cpu().numpy()          # one animation over both intervals
    assert np.array_equal(frames, want) and len(np.unique(frames.reshape(-1, 3), axis=0)) >= 4
    r = subprocess.run(NPY + [pose, '--out', again, '--anim_size', '64x48'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and '17 frames of 64x48' in r.stdout, r.stderr[-2000:]
    assert np.array_equal(np.stack([raster_ref.read_bmp(os.path.join(again, f'frame_{i}.bmp')) for i in range(17)]), frames)

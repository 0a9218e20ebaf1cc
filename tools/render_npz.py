#!/usr/bin/env python
"""Render a saved SMPL-X motion on the device: the counterpart of the reference's ``render_one_sequence_wo_gt``
(mogen/datasets/EMAGE_2024/utils/other_tools.py:695-765) and, with ``--gt``, of the side-by-side pair ``generate_silent_videos`` stacks
horizontally (fast_render.py:83-95).  ``res_*.npz`` / ``gt_*.npz`` hold poses [n,165], expressions [n,100], trans [n,3], betas [300], as
``tools/sample.py`` and the reference write them.  The body model and the rasteriser run on the MI355X; the frames are written as
``frame_%d.bmp`` (kept), and joined into an mp4 when an ffmpeg is on PATH.  The scene is the reference's (fast_render.py:35-81); the
colours are this project's shading model, not pyrender's.

    python tools/render_npz.py res_x.npz --smplx_model SMPLX_NEUTRAL_2020.npz --out frames/ [--gt gt_x.npz] [--render_size 960x720]
        [--render_fps 30] [--num_betas 300]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from motioncraft_amd import postprocess, render                 # noqa: E402

KEYS = ('poses', 'expressions', 'trans')


def parse_args():
    p = argparse.ArgumentParser(description='render res_*.npz / gt_*.npz SMPL-X motions to frames')
    p.add_argument('npz', help='poses / expressions / trans / betas of the motion to draw')
    p.add_argument('--smplx_model', default=None, metavar='PATH', help='the published SMPL-X model file (.npz)')
    p.add_argument('--out', required=True, metavar='DIR', help='where frame_%%d.bmp (and the mp4) go')
    p.add_argument('--gt', default=None, metavar='NPZ', help='a second motion drawn to the right of the first, frame by frame')
    p.add_argument('--render_size', default='960x720', metavar='WxH', help='size of ONE view (the reference: 960x720)')
    p.add_argument('--render_fps', type=float, default=30.0)
    p.add_argument('--num_betas', type=int, default=300), p.add_argument('--num_expression_coeffs', type=int, default=100)
    return p.parse_args()


def load_motion(path):
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in KEYS if k not in z.files]
        if missing:
            raise ValueError(f'{path}: not a saved SMPL-X motion, missing {missing}')
        d = {k: np.asarray(z[k], np.float64) for k in KEYS}
        betas = np.asarray(z['betas'], np.float64).reshape(-1) if 'betas' in z.files else None
    n = d['poses'].shape[0]
    if d['poses'].ndim != 2 or d['poses'].shape[1] != 165 or any(d[k].shape[0] != n for k in KEYS):
        raise ValueError(f'{path}: poses must be [n,165] with expressions and trans of the same length, got '
                         + ', '.join(f'{k} {d[k].shape}' for k in KEYS))
    return d, betas


def main():
    a = parse_args()
    if not a.smplx_model:
        raise ValueError('the mesh comes from the body model: --smplx_model PATH is required')
    W, H = render.parse_size(a.render_size)
    if not a.render_fps > 0:
        raise ValueError(f'--render_fps must be positive, got {a.render_fps}')
    motions = [load_motion(p) for p in ([a.npz, a.gt] if a.gt else [a.npz])]
    if a.gt and motions[0][0]['poses'].shape[0] != motions[1][0]['poses'].shape[0]:
        raise ValueError(f'--gt holds {motions[1][0]["poses"].shape[0]} frames, the motion {motions[0][0]["poses"].shape[0]}')
    from motioncraft_amd.body_model import SMPLXBodyModel
    body = SMPLXBodyModel.from_npz(a.smplx_model, num_betas=a.num_betas, num_expression_coeffs=a.num_expression_coeffs)
    if body.faces.shape[0] == 0:
        raise ValueError(f'{a.smplx_model} holds no faces (key f): nothing to draw')
    renderer = render.MeshRenderer(body.faces, body.num_vertices, width=W, height=H)
    views = []
    for d, betas in motions:
        post = {k: torch.from_numpy(d[k]).cuda() for k in KEYS}
        if betas is not None and betas.size < body.num_betas:
            betas = np.concatenate([betas, np.zeros(body.num_betas - betas.size)])
        views.append(postprocess.smplx_render(post, body, renderer, betas=betas))
    frames = views[0] if len(views) == 1 else torch.cat(views, dim=2)        # np.hstack of the two figures
    name = os.path.splitext(os.path.basename(a.npz))[0]
    paths, mp4 = render.save_frames(frames, a.out, a.render_fps, name[4:] if name.startswith('res_') else name)
    print(f'{len(paths)} frames of {frames.shape[2]}x{frames.shape[1]} -> {a.out}' + (f', {mp4}' if mp4 else ' (no ffmpeg on PATH: frames only)'))
    renderer.close(), body.close()


if __name__ == '__main__':
    main()

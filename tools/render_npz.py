#!/usr/bin/env python
"""Render a saved SMPL-X motion on the device: the counterpart of the reference's ``render_one_sequence_wo_gt``
(mogen/datasets/EMAGE_2024/utils/other_tools.py:695-765) and, with ``--gt``, of the side-by-side pair ``generate_silent_videos`` stacks
horizontally (fast_render.py:83-95).  ``res_*.npz`` / ``gt_*.npz`` hold poses [n,165], expressions [n,100], trans [n,3], betas [300], as
``tools/sample.py`` and the reference write them.  The body model and the rasteriser run on the MI355X; with ``--out`` the frames are
written as ``frame_%d.bmp`` (kept), and joined into an mp4 when an ffmpeg is on PATH; with ``--avi`` they are encoded on the device into
one Motion-JPEG AVI, and ``--audio`` puts the speech beside them: the counterpart of ``add_audio_to_video``
(mogen/datasets/EMAGE_2024/utils/media.py:4-21), which turns ``res_<id>.npz`` + the wav into a clip with sound.  The wav is decoded at
its own rate and mixed to mono, not resampled.  The scene is the reference's (fast_render.py:35-81); the colours are this project's
shading model, not pyrender's.

    python tools/render_npz.py res_x.npz --smplx_model SMPLX_NEUTRAL_2020.npz [--out frames/] [--avi clip.avi [--audio x.wav]
        [--avi_quality 90]] [--gt gt_x.npz] [--render_size 960x720] [--render_fps 30] [--num_betas 300]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from motioncraft_amd import audio, postprocess, render, video   # noqa: E402

KEYS = ('poses', 'expressions', 'trans')


def parse_args():
    p = argparse.ArgumentParser(description='render res_*.npz / gt_*.npz SMPL-X motions to frames')
    p.add_argument('npz', help='poses / expressions / trans / betas of the motion to draw')
    p.add_argument('--smplx_model', default=None, metavar='PATH', help='the published SMPL-X model file (.npz)')
    p.add_argument('--out', default=None, metavar='DIR', help='where frame_%%d.bmp (and the mp4) go')
    p.add_argument('--avi', default=None, metavar='FILE', help='one Motion-JPEG AVI, encoded on the device; --out is then optional')
    p.add_argument('--avi_quality', type=int, default=90, metavar='N', help='JPEG quality of --avi, 1..100')
    p.add_argument('--audio', default=None, metavar='WAV', help='with --avi: the speech, as the PCM track of the file (cut or padded to the video)')
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


def speech_track(path):
    """(int16 [samples], rate): the wav decoded on the device at the file's own rate, its channels averaged, back at 16 bits."""
    y, rate = audio.load_wav(path)
    return torch.clamp(torch.round(y * 32768.0), -32768, 32767).to(torch.int16).cpu().numpy(), rate


def main():
    a = parse_args()
    if not a.smplx_model:
        raise ValueError('the mesh comes from the body model: --smplx_model PATH is required')
    if not (a.out or a.avi):
        raise ValueError('name an output: --out DIR for frames, --avi FILE for one video file, or both')
    if a.audio and not a.avi:
        raise ValueError('--audio goes into the file --avi FILE names; frames alone carry no sound')
    if not 1 <= a.avi_quality <= 100:
        raise ValueError(f'--avi_quality must be in 1..100, got {a.avi_quality}')
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
    if a.out:
        paths, mp4 = render.save_frames(frames, a.out, a.render_fps, name[4:] if name.startswith('res_') else name)
        print(f'{len(paths)} frames of {frames.shape[2]}x{frames.shape[1]} -> {a.out}' + (f', {mp4}' if mp4 else ' (no ffmpeg on PATH: frames only)'))
    if a.avi:
        pcm, rate = speech_track(a.audio) if a.audio else (None, None)
        size = video.save_avi(frames, a.avi, a.render_fps, audio=pcm, audio_rate=rate, quality=a.avi_quality)
        print(f'{frames.shape[0]} frames of {frames.shape[2]}x{frames.shape[1]}' + (f' + {a.audio} at {rate} Hz' if a.audio else '') + f' -> {a.avi} ({size} bytes)')
    renderer.close(), body.close()


if __name__ == '__main__':
    main()

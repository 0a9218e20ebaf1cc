#!/usr/bin/env python
"""Draw a saved joint file on the device: the ``--pose_npy`` file of ``tools/sample.py`` and of the reference's tool
(tools/visualize.py:55-56), fp32 [frames, J, 3], as the skeleton animation ``plot_3d_motion`` makes of it
(mogen/utils/plot_utils.py:107-204).  J = 22 draws the HumanML3D chains, J = 21 the KIT chains, J = 52 the body with both hands.  The
rasteriser runs on the MI355X; with ``--out`` the frames are written as ``frame_%d.bmp`` (kept) and joined into an mp4 when an ffmpeg is
on PATH; with ``--avi`` they are encoded on the device into one Motion-JPEG AVI and never leave it uncompressed.
Not drawn: the title, anti-aliasing, mplot3d's projecting caps.

    python tools/skeleton_npy.py joints.npy [--out frames/] [--avi clip.avi [--avi_quality 90]] [--anim_size 1000x1000] [--anim_fps 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

from motioncraft_amd import lib, render, skeleton, video        # noqa: E402

# the fingers of the 52-joint layout: three joints each, in the order of the file, hanging off the wrists 20 and 21
HAND_CHAINS = [[20 + side] + [22 + 15 * side + 3 * f + k for k in range(3)] for side in (0, 1) for f in range(5)]


def chains_for(J):
    if J == 22:
        return skeleton.T2M_CHAINS
    if J == 21:
        return skeleton.KIT_CHAINS
    if J == 52:
        return skeleton.T2M_CHAINS + HAND_CHAINS
    raise ValueError(f'{J} joints: expected 22 (human_ml3d), 21 (kit_ml) or 52 (body and hands)')


def parse_anim_size(text):
    W, H = render.parse_size(text, '--anim_size')
    if max(W, H) > skeleton.MAX_SIZE:
        raise ValueError(f'--anim_size: at most {skeleton.MAX_SIZE} pixels a side, got {text!r}')
    return W, H


def main():
    p = argparse.ArgumentParser(description='draw a saved [frames, J, 3] joint file as a skeleton animation')
    p.add_argument('npy', help='joint positions [frames, J, 3], as --pose_npy saves them')
    p.add_argument('--out', default=None, metavar='DIR', help='where frame_%%d.bmp (and the mp4) go')
    p.add_argument('--avi', default=None, metavar='FILE', help='one Motion-JPEG AVI, encoded on the device; --out is then optional')
    p.add_argument('--avi_quality', type=int, default=90, metavar='N', help='JPEG quality of --avi, 1..100')
    p.add_argument('--anim_size', default='1000x1000', metavar='WxH', help='frame size (the reference: 1000x1000)')
    p.add_argument('--anim_fps', type=float, default=20.0)
    a = p.parse_args()
    if not (a.out or a.avi):
        raise ValueError('name an output: --out DIR for frames, --avi FILE for one video file, or both')
    if not 1 <= a.avi_quality <= 100:
        raise ValueError(f'--avi_quality must be in 1..100, got {a.avi_quality}')
    W, H = parse_anim_size(a.anim_size)
    if not a.anim_fps > 0:
        raise ValueError(f'--anim_fps must be positive, got {a.anim_fps}')
    joints = np.load(a.npy, allow_pickle=False)
    if joints.ndim != 3 or joints.shape[2] != 3 or joints.shape[0] < 1:
        raise ValueError(f'{a.npy}: expected joint positions [frames, J, 3], got {joints.shape}')
    if a.avi:
        lib.load(require_gpu=True)                               # no device: the library's message, before anything is drawn
    r = skeleton.SkeletonRenderer(chains_for(joints.shape[1]), width=W, height=H, num_joints=joints.shape[1])
    frames = r.render(torch.from_numpy(np.ascontiguousarray(joints, np.float32)).cuda())
    name = os.path.splitext(os.path.basename(a.npy))[0]
    if a.out:
        paths, mp4 = render.save_frames(frames, a.out, a.anim_fps, name)
        print(f'{len(paths)} frames of {W}x{H} -> {a.out}' + (f', {mp4}' if mp4 else ' (no ffmpeg on PATH: frames only)'))
    if a.avi:
        size = video.save_avi(frames, a.avi, a.anim_fps, quality=a.avi_quality)
        print(f'{frames.shape[0]} frames of {W}x{H} -> {a.avi} ({size} bytes)')
    r.close()


if __name__ == '__main__':
    main()

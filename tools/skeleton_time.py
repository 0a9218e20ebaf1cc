#!/usr/bin/env python
"""Time the skeleton renderer on a clip of the text-to-motion size (the figures in DESIGN.md section 4h): 196 frames of the 22-joint
HumanML3D skeleton at 1000 x 1000, ``skeleton.SkeletonRenderer.render`` end to end.  Device times are hipEvents around ``--batch``
back-to-back calls divided by their number, warm-up excluded, median of ``--reps``.  The byte floor it is held against is the 3 bytes
of colour per pixel, written once, at the 8 TB/s HBM peak of the MI355X; the design reads next to nothing.

Where matplotlib imports, the same scene is also drawn the reference's way -- an ``Axes3D`` at elev 120 / azim -90 / dist 7.5 with the
ground quad, the trail and the five chains, one ``canvas.draw()`` on the Agg backend per frame -- and timed on the host
(``--host_frames`` frames, 0 = skip).  Writing the video comes on top of that there and is not counted on either side.

    python tools/skeleton_time.py [--frames 196] [--size 1000x1000] [--reps 9] [--batch 3] [--host_frames 196]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motioncraft_amd import render, skeleton                    # noqa: E402
from resample_time import timed                                 # noqa: E402

HBM_PEAK = 8.0e12                                               # bytes / s
# bone vectors (child - parent) of a standing 22-joint body, metres, y up
BONES = {1: (0.07, -0.09, 0), 2: (-0.07, -0.09, 0), 3: (0, 0.11, 0), 4: (0.03, -0.38, 0), 5: (-0.03, -0.38, 0), 6: (0, 0.13, 0),
         7: (0, -0.4, -0.03), 8: (0, -0.4, -0.03), 9: (0, 0.06, 0), 10: (0, -0.06, 0.12), 11: (0, -0.06, 0.12), 12: (0, 0.21, 0),
         13: (0.08, 0.12, 0), 14: (-0.08, 0.12, 0), 15: (0, 0.09, 0.02), 16: (0.1, 0.03, 0), 17: (-0.1, 0.03, 0), 18: (0.26, 0, 0),
         19: (-0.26, 0, 0), 20: (0.25, 0, 0), 21: (-0.25, 0, 0)}


def clip(frames):
    """joints [frames, 22, 3]: the body walks along +z on a slow curve, legs and arms swinging about x."""
    t = np.arange(frames) / 20.0
    out = np.zeros((frames, 22, 3))
    out[:, 0] = np.stack([0.4 * np.sin(0.5 * t), 0.93 + 0.02 * np.sin(8 * t), 0.12 * np.arange(frames) / 2], axis=1)
    swing = {1: 1, 4: 1, 2: -1, 5: -1, 16: -1, 18: -1, 17: 1, 19: 1}            # hips, knees, shoulders, elbows
    for j in range(1, 22):
        b = np.broadcast_to(np.asarray(BONES[j], np.float64), (frames, 3)).copy()
        if j in swing:
            a = 0.5 * swing[j] * np.sin(4 * t)
            b[:, 1], b[:, 2] = np.cos(a) * b[:, 1] - np.sin(a) * b[:, 2] - (np.sin(a) * 0.3 if j > 15 else 0), np.sin(a) * b[:, 1] + np.cos(a) * b[:, 2]
        out[:, j] = out[:, skeleton.T2M_PARENTS[j]] + b
    return out.astype(np.float32)


def host_draw(joints, size, count):
    """seconds per frame of the host drawing, or None without matplotlib"""
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        from mpl_toolkits.mplot3d.art3d import Poly3DCollection
    except Exception:
        return None
    data = joints.astype(np.float64).copy()
    lo, hi = data.min(axis=(0, 1)), data.max(axis=(0, 1))
    data[:, :, 1] -= lo[1]
    path = data[:, 0, [0, 2]].copy()
    data[:, :, [0, 2]] -= path[:, None]
    fig = plt.figure(figsize=(size[0] / 100, size[1] / 100), dpi=100)
    ax = fig.add_axes([0, 0, 1, 1], projection='3d')
    names = skeleton.CHAIN_COLORS
    t0 = time.perf_counter()
    for i in range(count):
        ax.clear()
        ax.set_xlim3d(-1, 1), ax.set_ylim3d(0, 2), ax.set_zlim3d(0, 2)
        ax.view_init(elev=120, azim=-90)
        ax._dist = 7.5
        x0, x1, z0, z1 = lo[0] - path[i, 0], hi[0] - path[i, 0], lo[2] - path[i, 1], hi[2] - path[i, 1]
        quad = Poly3DCollection([[(x0, 0, z0), (x0, 0, z1), (x1, 0, z1), (x1, 0, z0)]])
        quad.set_facecolor((0.5, 0.5, 0.5, 0.5))
        ax.add_collection3d(quad)
        if i > 1:
            ax.plot3D(path[:i, 0] - path[i, 0], np.zeros(i), path[:i, 1] - path[i, 1], linewidth=1.0, color='blue')
        for c, chain in enumerate(skeleton.T2M_CHAINS):
            ax.plot3D(data[i, chain, 0], data[i, chain, 1], data[i, chain, 2], linewidth=4.0 if c < 5 else 2.0, color=names[c])
        ax.set_axis_off()
        fig.canvas.draw()
    dt = (time.perf_counter() - t0) / max(count, 1)
    plt.close(fig)
    return dt


def main():
    p = argparse.ArgumentParser(description='time the skeleton renderer on a clip of the text-to-motion size')
    p.add_argument('--frames', type=int, default=196), p.add_argument('--size', default='1000x1000')
    p.add_argument('--reps', type=int, default=9), p.add_argument('--batch', type=int, default=3)
    p.add_argument('--host_frames', type=int, default=196, help='frames drawn with matplotlib for the comparison (0 = skip)')
    a = p.parse_args()
    W, H = render.parse_size(a.size, '--size')
    if max(W, H) > skeleton.MAX_SIZE:
        raise ValueError(f'--size: at most {skeleton.MAX_SIZE} pixels a side, got {a.size}')
    joints = clip(a.frames)
    dev = torch.from_numpy(joints).cuda()
    r = skeleton.SkeletonRenderer(skeleton.T2M_CHAINS, width=W, height=H)
    out = r.render(dev, return_buffers=True)
    shares = [float((out['layer'] == l).float().mean()) for l in (1, 2)] + [float((out['layer'] >= 3).float().mean())]
    r.render(dev)
    torch.cuda.synchronize()
    med, low = timed(lambda: r.render(dev), a.reps, a.batch)
    floor_us = a.frames * 3 * W * H / HBM_PEAK * 1e6
    print(f'{a.frames} frames of 22 joints at {W}x{H}: plane {100 * shares[0]:.1f} %, trail {100 * shares[1]:.2f} %, chains {100 * shares[2]:.2f} % of the pixels')
    print(f'render: median {med:.0f} us (min {low:.0f}) = {med / a.frames:.2f} us per frame = {a.frames / med * 1e6:.0f} frames/s')
    print(f'byte floor: {3 * W * H / 1e6:.2f} MB per frame = {floor_us:.0f} us for the clip at {HBM_PEAK / 1e12:.0f} TB/s; the run is '
          f'{floor_us / med:.3f} of the floor rate')
    r.close()
    if a.host_frames > 0:
        count = min(a.host_frames, a.frames)
        dt = host_draw(joints, (W, H), count)
        if dt is None:
            print('host comparison: matplotlib does not import here')
        else:
            print(f'host, matplotlib mplot3d + Agg: {dt * 1e3:.1f} ms per frame over {count} frames = {1 / dt:.1f} frames/s, '
                  f'{dt * a.frames:.1f} s for the clip; the device is {dt * a.frames * 1e6 / med:.0f} times faster')


if __name__ == '__main__':
    main()

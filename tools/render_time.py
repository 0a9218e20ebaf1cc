#!/usr/bin/env python
"""Time the device renderer on a clip of the published model's size (the figures in DESIGN.md): 196 frames of a 10 475-vertex /
20 908-face body-sized mesh at 960 x 720 under the reference's camera, ``render.MeshRenderer.render`` end to end.
Device times are hipEvents around ``--batch`` back-to-back calls divided by their number, warm-up excluded, median of ``--reps``.
The byte floor it is held against is what the design cannot avoid per frame: the 8-byte visibility key of every pixel read once and
reset once by the shade kernel, the 3 bytes of colour, and the vertex streams (12 B read; screen, zcam and normal written once and
read once: 2 x 24 B) -- about 19 B per pixel -- at the 8 TB/s HBM peak of the MI355X.  The atomics of the raster kernel come on top.
``--sweep`` times the clip, and a scene with a floor quad that fills the viewport behind the mesh, at several values of the
large-triangle threshold (bounding-box pixels above which waves walk a triangle instead of one thread), then the floor scene at
several numbers of waves per large triangle.
Per-kernel times come from a kernel trace of one call:  tools/prof_cmd.sh render tools/render_time.py --reps 1 --batch 1

    python tools/render_time.py [--frames 196] [--size 960x720] [--reps 9] [--batch 3] [--sweep]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motioncraft_amd import render                              # noqa: E402
from resample_time import timed                                 # noqa: E402

HBM_PEAK = 8.0e12                                               # bytes / s
V, F = 10475, 20908


def body_mesh():
    """A closed ellipsoid of 85 rings x 123 columns + 2 poles = 10 457 vertices and 20 910 faces, outward oriented, cut to the
    published counts: two faces dropped, 18 unused vertices appended."""
    R, C = 85, 123
    th = np.pi * (np.arange(R) + 1) / (R + 1)
    ph = 2 * np.pi * np.arange(C) / C
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(C)), np.outer(np.sin(th), np.sin(ph))], axis=2).reshape(-1, 3)
    v = np.concatenate([ring, [[0, 1, 0], [0, -1, 0]], np.zeros((V - R * C - 2, 3))])
    top, bottom = R * C, R * C + 1
    idx = lambda r, c: r * C + c % C
    f = [[top, idx(0, c + 1), idx(0, c)] for c in range(C)] + [[bottom, idx(R - 1, c), idx(R - 1, c + 1)] for c in range(C)]
    for r in range(R - 1):
        for c in range(C):
            f += [[idx(r, c), idx(r, c + 1), idx(r + 1, c)], [idx(r + 1, c), idx(r, c + 1), idx(r + 1, c + 1)]]
    return v * [0.28, 0.85, 0.16], np.asarray(f[:F], np.int64)


def clip(frames, floor=False):
    """vertices [frames, V(+4), 3]: the ellipsoid at (0, 1, 0) swaying about the vertical axis; with ``floor`` a quad that fills the
    viewport stands behind it (two more triangles)."""
    v, f = body_mesh()
    t = np.linspace(0, 2 * np.pi, frames, endpoint=False)
    c, s = np.cos(0.6 * np.sin(t)), np.sin(0.6 * np.sin(t))
    out = np.stack([np.stack([c[i] * v[:, 0] + s[i] * v[:, 2], v[:, 1], -s[i] * v[:, 0] + c[i] * v[:, 2]], axis=1) for i in range(frames)])
    out += [0.0, 1.0, 0.0]
    out[:, :, 0] += 0.1 * np.sin(t)[:, None]
    if floor:
        quad = np.array([[-1.5, -0.5, -1.0], [1.5, -0.5, -1.0], [1.5, 2.5, -1.0], [-1.5, 2.5, -1.0]])
        out = np.concatenate([out, np.broadcast_to(quad, (frames, 4, 3))], axis=1)
        f = np.concatenate([f, [[V, V + 1, V + 2], [V, V + 2, V + 3]]])
    return torch.from_numpy(out.astype(np.float32)).cuda(), f


def main():
    p = argparse.ArgumentParser(description='time the device renderer on a clip of the published size')
    p.add_argument('--frames', type=int, default=196), p.add_argument('--size', default='960x720')
    p.add_argument('--reps', type=int, default=9), p.add_argument('--batch', type=int, default=3)
    p.add_argument('--sweep', action='store_true', help='sweep the large-triangle threshold, with and without a floor quad')
    a = p.parse_args()
    W, H = render.parse_size(a.size, '--size')
    verts, faces = clip(a.frames)
    r = render.MeshRenderer(faces, verts.shape[1], width=W, height=H)
    rgb, face, *_ = r.render(verts, return_buffers=True)
    covered = float((face >= 0).float().mean())
    r.render(verts)
    torch.cuda.synchronize()
    med, low = timed(lambda: r.render(verts), a.reps, a.batch)
    per_frame = 19 * W * H + (12 + 2 * 24) * V
    floor_us = a.frames * per_frame / HBM_PEAK * 1e6
    print(f'{a.frames} frames of {verts.shape[1]} vertices / {faces.shape[0]} faces at {W}x{H}, {100 * covered:.1f} % of the pixels covered, '
          f'{a.frames * faces.shape[0] / 1e6:.2f} M triangles')
    print(f'render: median {med:.0f} us (min {low:.0f}) = {med / a.frames:.2f} us per frame')
    print(f'byte floor: {per_frame / 1e6:.2f} MB per frame = {floor_us:.0f} us for the clip at {HBM_PEAK / 1e12:.0f} TB/s; '
          f'the run is {floor_us / med:.3f} of the floor rate ({a.frames * per_frame / med / 1e6:.2f} TB/s of unavoidable bytes)')
    r.close()
    if a.sweep:
        for floor in (False, True):
            verts, faces = clip(a.frames, floor)
            line = []
            for threshold in (16, 64, 256, 1024, 4096, 65536, 2 ** 31 - 1):
                if floor and threshold > 65536:
                    line.append('all-thread: not run (one thread would walk the viewport)')
                    continue
                r = render.MeshRenderer(faces, verts.shape[1], width=W, height=H, large_threshold=threshold)
                r.render(verts)
                torch.cuda.synchronize()
                line.append(f'{threshold}: {timed(lambda: r.render(verts), max(3, a.reps // 3), 1)[0]:.0f} us')
                r.close()
            print(('clip + floor quad' if floor else 'clip') + ', large_threshold -> median: ' + ', '.join(line))
        line = []
        for slices in (1, 2, 4, 8, 16, 32, 64, 256):                         # the floor scene is still loaded
            r = render.MeshRenderer(faces, verts.shape[1], width=W, height=H, large_slices=slices)
            r.render(verts)
            torch.cuda.synchronize()
            line.append(f'{slices}: {timed(lambda: r.render(verts), max(3, a.reps // 3), 1)[0]:.0f} us')
            r.close()
        print('clip + floor quad, large_slices (waves per large triangle, default threshold) -> median: ' + ', '.join(line))


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Time the device JPEG encoder on clips of the two renderers' sizes (the figures in DESIGN.md): 196 frames at 960 x 720 (the mesh
renderer's default) and at 1000 x 1000 (the skeleton renderer's), ``video.JpegEncoder.encode`` end to end -- the kernels, and the copy of
the encoded bytes to the host -- and the bytes that come out.  Beside it the path frames took before: the device-to-host copy of the raw
frames and ``render.write_frames`` (one 24-bit BMP per frame) into a temporary directory.  Both are wall-clock times around a
synchronised call, warm-up excluded, the median of ``--reps``.  The frames are a white background with a shaded, hard-edged body in
the middle: what the renderers draw.

    python tools/video_time.py [--frames 196] [--sizes 960x720 1000x1000] [--quality 90] [--subsampling 4:2:0] [--reps 5]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motioncraft_amd import lib, render, video                  # noqa: E402


def clip(frames, W, H):
    """uint8 [frames, H, W, 3] on the device: a grey ellipse with a soft gradient across it and a hard outline, swaying over white."""
    y, x = torch.meshgrid(torch.arange(H, device='cuda', dtype=torch.float32), torch.arange(W, device='cuda', dtype=torch.float32), indexing='ij')
    out = torch.full((frames, H, W, 3), 255, dtype=torch.uint8, device='cuda')
    for i in range(frames):
        cx = W / 2 + 0.1 * W * torch.sin(torch.tensor(2 * torch.pi * i / frames))
        d = ((x - cx) / (0.15 * W)) ** 2 + ((y - H / 2) / (0.4 * H)) ** 2
        shade = (60 + 160 * (1 - d).clamp(0, 1) ** 0.5 + 20 * (x - cx) / W).clamp(0, 255).to(torch.uint8)
        out[i][d <= 1] = shade[d <= 1][:, None]
    return out


def median_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def main():
    p = argparse.ArgumentParser(description='time the device JPEG encoder beside the BMP path')
    p.add_argument('--frames', type=int, default=196), p.add_argument('--sizes', nargs='+', default=['960x720', '1000x1000'])
    p.add_argument('--quality', type=int, default=90), p.add_argument('--subsampling', default='4:2:0', choices=sorted(video.SUBSAMPLINGS))
    p.add_argument('--reps', type=int, default=5)
    a = p.parse_args()
    lib.load(require_gpu=True)
    for size in a.sizes:
        W, H = render.parse_size(size, '--sizes')
        frames = clip(a.frames, W, H)
        enc = video.JpegEncoder(W, H, a.quality, a.subsampling)
        files = enc.encode(frames)
        encoded = sum(len(f) for f in files)
        t_enc = median_ms(lambda: enc.encode(frames), a.reps)
        enc.close()
        with tempfile.TemporaryDirectory() as tmp:
            t_bmp = median_ms(lambda: render.write_frames(frames, tmp), max(1, a.reps // 2))
        raw = frames.numel()
        print(f'{a.frames} frames of {W}x{H}, quality {a.quality}, {a.subsampling}: encode + copy {t_enc:.1f} ms ({t_enc / a.frames:.3f} ms per frame), '
              f'{encoded} bytes = {encoded / a.frames / 1e3:.1f} kB per frame, 1 / {raw / encoded:.1f} of the raw {raw} bytes')
        print(f'    the BMP path: copy of the raw frames + write_frames {t_bmp:.1f} ms ({t_bmp / a.frames:.3f} ms per frame); ratio {t_bmp / t_enc:.1f}')


if __name__ == '__main__':
    main()

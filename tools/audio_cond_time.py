#!/usr/bin/env python
"""Time the S2G audio condition on a synthetic clip (the figures in DESIGN.md and profiles/audio_cond_time.txt):
  (a) ``mc_audio_condition`` alone, window 1024;  (b) ``AudioCondition.__call__`` (onset strength + pick + the kernel) on a clip
  already on the device;  (c) the numpy restatement ``tests/audio_cond_ref.py`` on this host;  (d) the kernel at window 64.
Device times are hipEvents around ``--batch`` back-to-back launches divided by their number (one launch of a clip this short is
over before the next is enqueued, so a single bracketed launch times the enqueue), warm-up excluded, median of ``--reps``.
(a) is set against the traffic floor of 12 B per sample (4 read, 8 written) at the 6.3 TB/s a copy reaches on this part; a clip
whose 12 B per sample fit the 256 MiB Infinity Cache stays there between the launches of a batch, so only a longer one (an hour:
--seconds 3600) is held against HBM like for like.

    python tools/audio_cond_time.py [--seconds 60] [--sr 16000] [--reps 15] [--batch 200] [--no-host]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import audio_cond_ref                                           # noqa: E402
from motioncraft_amd import lib as L, speech                    # noqa: E402
from onset_time import clip                                     # noqa: E402

INFINITY_CACHE = 256 << 20
HBM_COPY_RATE = 6.3e12                                          # B/s: what a float4 copy reaches on the MI355X


def timed(fn, reps, batch):
    """median and minimum device time of one ``fn()`` in us, from ``batch`` calls between two events"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / batch)
    return statistics.median(out), min(out)


def main():
    p = argparse.ArgumentParser(description='time the S2G audio condition on a synthetic clip')
    p.add_argument('--seconds', type=int, default=60), p.add_argument('--sr', type=int, default=16000)
    p.add_argument('--reps', type=int, default=15), p.add_argument('--batch', type=int, default=200)
    p.add_argument('--no-host', action='store_true', help='skip the numpy restatement (its time grows with the clip: 1023 passes over it)')
    a = p.parse_args()
    lib = L.load(require_gpu=True)
    y_host = clip(a.sr, a.seconds)
    y = torch.from_numpy(y_host).cuda()
    n = y.numel()
    out = torch.empty(n, 2, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel(window):
        L.check(lib.mc_audio_condition(ctypes.c_void_p(y.data_ptr()), n, window, None, 0, ctypes.c_void_p(out.data_ptr()), stream), 'mc_audio_condition')
    ac = speech.AudioCondition(sr=a.sr)
    for _ in range(3):
        kernel(1024), kernel(64), ac(y)
    torch.cuda.synchronize()
    k1024, k64 = timed(lambda: kernel(1024), a.reps, a.batch), timed(lambda: kernel(64), a.reps, a.batch)
    whole = timed(lambda: ac(y), a.reps, max(1, a.batch // 20))
    floor_us = 12.0 * n / HBM_COPY_RATE * 1e6
    print(f'{a.seconds} s at {a.sr} Hz: {n} samples, {(n + speech.AUDIO_COND_TILE - 1) // speech.AUDIO_COND_TILE} workgroups, {12 * n / 1e6:.1f} MB of traffic')
    if 12 * n < INFINITY_CACHE:
        print(f'    the same {12 * n / 1e6:.1f} MB are read and written by every launch of a batch and fit the {INFINITY_CACHE >> 20} MiB Infinity Cache: '
              'the times below are cache-resident, and the HBM floor is a lower bound they are not held against like for like')
    print(f'(a) mc_audio_condition, window 1024: median {k1024[0]:.2f} us (min {k1024[1]:.2f}) = {12.0 * n / (k1024[0] * 1e-6) / 1e12:.2f} TB/s; '
          f'floor at 6.3 TB/s {floor_us:.2f} us = {100 * floor_us / k1024[0]:.0f} % of the measured time')
    print(f'(b) AudioCondition.__call__ on a device clip: median {whole[0]:.0f} us (min {whole[1]:.0f})')
    if not a.no_host:
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = audio_cond_ref.envelope(y_host)
            runs.append(time.perf_counter() - t0)
        host = statistics.median(runs)
        kernel(1024)
        same = np.array_equal(out[:, 0].cpu().numpy().view(np.uint32), want.view(np.uint32))
        print(f'(c) numpy restatement of the envelope on this host, median of 3: {host:.3f} s (min {min(runs):.3f}, max {max(runs):.3f}) = {host * 1e6 / k1024[0]:.0f} x (a); the same bits: {same}')
    print(f'(d) window 64: median {k64[0]:.2f} us (min {k64[1]:.2f}); window 1024 takes {k1024[0] / k64[0]:.2f} x that for 16 x the window '
          f'(10 table levels against 6)')


if __name__ == '__main__':
    main()

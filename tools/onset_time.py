#!/usr/bin/env python
"""Time ``OnsetDetector.strength`` + ``pick`` on a synthetic clip (the figure in DESIGN.md): hipEvents around the two calls,
warm-up excluded, median of ``--reps`` runs.

    python tools/onset_time.py [--seconds 120] [--sr 16000] [--reps 15]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motioncraft_amd import scoring                             # noqa: E402


def clip(sr, seconds, seed=1):
    """float32 [seconds * sr]: white noise of 0.02 rms plus three decaying tone bursts per second"""
    rs = np.random.RandomState(seed)
    n = seconds * sr
    y = 0.02 * rs.standard_normal(n)
    for _ in range(3 * seconds):
        i0, f, a, tau = rs.randint(0, n - sr // 2), rs.uniform(150, 3500), rs.uniform(0.05, 0.8), rs.uniform(0.03, 0.12)
        t = np.arange(min(n - i0, sr // 2)) / sr
        y[i0:i0 + t.size] += a * np.exp(-t / tau) * np.sin(2 * np.pi * f * t)
    return y.astype(np.float32)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out)


def main():
    p = argparse.ArgumentParser(description='time onset detection on a synthetic clip')
    p.add_argument('--seconds', type=int, default=120), p.add_argument('--sr', type=int, default=16000), p.add_argument('--reps', type=int, default=15)
    a = p.parse_args()
    det = scoring.OnsetDetector(sr=a.sr)
    y = torch.from_numpy(clip(a.sr, a.seconds)).cuda()
    for _ in range(3):
        env = det.strength(y)
        det.pick(env)
    torch.cuda.synchronize()
    both, st, pk = timed(lambda: det.pick(det.strength(y)), a.reps), timed(lambda: det.strength(y), a.reps), timed(lambda: det.pick(env), a.reps)
    F = env.numel()
    flop = 2.0 * F * 2050 * 2048
    print(f'{a.seconds} s at {a.sr} Hz: {F} frames, {det.detect(y).size} onsets; strength + pick median {both[0]:.0f} us (min {both[1]:.0f}); '
          f'strength alone {st[0]:.0f} us; pick alone {pk[0]:.0f} us')
    print(f'DFT product {flop / 1e9:.1f} GFLOP: {flop / (st[0] * 1e-6) / 1e12:.1f} TFLOP/s over the whole strength call')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Time decode + resampling of a synthetic clip on the device (the figures in DESIGN.md): 60 s of 16-bit stereo at 44.1 kHz through
  (a) 44 100 -> 16 000 and  (b) 44 100 -> 22 050 -> 16 000, the reference's ``librosa.load`` + ``librosa.resample`` detour,
against  (c) the host-to-device copy of the same bytes (pageable memory, as ``audio.load_wav`` uploads them, and pinned) and
(d) ``scipy.signal.resample_poly`` on this host (the mono float32 mix, which scipy filters in float32, and its fp64 form).
Device times are hipEvents around ``--batch`` back-to-back runs divided by their number, warm-up excluded, median of ``--reps``;
the copy is timed one at a time (it is synchronous), the host with ``time.perf_counter``.  If a chain took longer than the copy of
the clip it processes, staging the taps in LDS would be the next step (``csrc/mc_resample.hip`` reads them through L2).

    python tools/resample_time.py [--seconds 60] [--sr 44100] [--target 16000] [--load_sr 22050] [--reps 15] [--batch 20] [--no-host]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from motioncraft_amd import audio                               # noqa: E402
from onset_time import clip                                     # noqa: E402


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


def host_timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out), min(out)


def main():
    p = argparse.ArgumentParser(description='time decode + resampling of a synthetic clip')
    p.add_argument('--seconds', type=int, default=60), p.add_argument('--sr', type=int, default=44100)
    p.add_argument('--target', type=int, default=16000), p.add_argument('--load_sr', type=int, default=22050)
    p.add_argument('--reps', type=int, default=15), p.add_argument('--batch', type=int, default=20)
    p.add_argument('--no-host', action='store_true', help='skip scipy on the host')
    a = p.parse_args()
    left = clip(a.sr, a.seconds)
    pcm = np.round(np.stack([left, 0.5 * np.roll(left, 7)], axis=1) * 32767).astype('<i2')
    host_bytes = torch.frombuffer(bytearray(pcm.tobytes()), dtype=torch.uint8)
    raw = host_bytes.cuda()
    direct, first, second = audio.Resampler(a.sr, a.target), audio.Resampler(a.sr, a.load_sr), audio.Resampler(a.load_sr, a.target)
    chain_a = lambda: direct(audio.decode_pcm(raw, 2, 2))
    chain_b = lambda: second(first(audio.decode_pcm(raw, 2, 2)))
    mono = audio.decode_pcm(raw, 2, 2)
    for _ in range(3):
        chain_a(), chain_b()
    torch.cuda.synchronize()
    dec = timed(lambda: audio.decode_pcm(raw, 2, 2), a.reps, a.batch)
    res = timed(lambda: direct(mono), a.reps, a.batch)
    ta, tb = timed(chain_a, a.reps, a.batch), timed(chain_b, a.reps, a.batch)
    n_a, n_b = chain_a().numel(), chain_b().numel()

    def upload(src):
        src.cuda()
        torch.cuda.synchronize()
    pinned = host_bytes.pin_memory()
    upload(host_bytes), upload(pinned)
    up_page, up_pin = host_timed(lambda: upload(host_bytes), a.reps), host_timed(lambda: upload(pinned), a.reps)
    mb = raw.numel() / 1e6
    print(f'{a.seconds} s of 16-bit stereo at {a.sr} Hz: {pcm.shape[0]} frames, {mb:.1f} MB')
    print(f'    mc_pcm_decode alone: median {dec[0]:.1f} us (min {dec[1]:.1f}); mc_resample_poly {direct.up}/{direct.down} alone, '
          f'{direct.taps.size} taps, {8 * direct.taps.size / 1e3:.0f} KB of them read through L2: median {res[0]:.1f} us (min {res[1]:.1f})')
    print(f'(a) decode + {a.sr} -> {a.target}: {n_a} samples, median {ta[0]:.1f} us (min {ta[1]:.1f})')
    print(f'(b) decode + {a.sr} -> {a.load_sr} -> {a.target}: {n_b} samples, median {tb[0]:.1f} us (min {tb[1]:.1f})')
    print(f'(c) host-to-device copy of the {mb:.1f} MB: pageable median {up_page[0]:.0f} us (min {up_page[1]:.0f}) = {mb / up_page[0] * 1e3:.1f} GB/s; '
          f'pinned median {up_pin[0]:.0f} us (min {up_pin[1]:.0f}) = {mb / up_pin[0] * 1e3:.1f} GB/s')
    worst = max(ta[0], tb[0])
    print(f'    (a) is {ta[0] / up_page[0]:.2f} x and (b) {tb[0] / up_page[0]:.2f} x the pageable copy (what load_wav does), '
          f'{ta[0] / up_pin[0]:.2f} x and {tb[0] / up_pin[0]:.2f} x the pinned one: the slower chain is '
          + ('under both copies, so the taps stay in global memory' if worst <= min(up_page[0], up_pin[0]) else
             'under the pageable copy but over the pinned one: staging the taps in LDS would pay only for a pinned upload' if worst <= up_page[0] else
             'over the copy load_wav makes: the taps should be staged in LDS'))
    if not a.no_host:
        from scipy.signal import resample_poly
        y32 = mono.cpu().numpy()
        y64 = y32.astype(np.float64)
        h32 = host_timed(lambda: resample_poly(y32, direct.up, direct.down), 3)
        h64 = host_timed(lambda: resample_poly(y64, direct.up, direct.down), 3)
        d64 = host_timed(lambda: resample_poly(resample_poly(y64, first.up, first.down), second.up, second.down), 3)
        print(f'(d) scipy.signal.resample_poly on this host, {a.sr} -> {a.target}, median of 3: float32 {h32[0] / 1e3:.1f} ms, fp64 {h64[0] / 1e3:.1f} ms '
              f'= {h64[0] / res[0]:.0f} x the kernel; the detour in fp64 {d64[0] / 1e3:.1f} ms')


if __name__ == '__main__':
    main()

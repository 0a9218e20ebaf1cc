#!/usr/bin/env python
"""Time the device Frechet distance (``embmetrics.frechet_distance``: centre both tables, three one-sided Jacobi decompositions) beside
the host route on the same box (the figures in DESIGN.md): the copy of the two fp32 tables to the host,
``calculate_activation_statistics`` and ``calculate_frechet_distance`` (``scipy.linalg.sqrtm``) of ``evaluation``, as the evaluators
run it.  Sizes: two tables of n rows at the evaluator widths, and the few-sequence case of the S2G / M2D tests.  Both are wall-clock
times around a synchronised call, warm-up excluded, the median of ``--reps``.  Also the sweeps and the round launches of each
decomposition (ground truth, sample, product), and both values against the exact nuclear-norm value in fp64 LAPACK.

    python tools/metrics_time.py [--sizes 4096x256 1024x512 24x256] [--reps 5]
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

from motioncraft_amd import embmetrics, evaluation, lib         # noqa: E402


def tables(n, d, seed):
    """two fp32 tables [n, d]: random rows mixed by a dense d x d matrix, the second one shifted"""
    rs = np.random.RandomState(seed)
    make = lambda shift: (rs.randn(n, d) @ (rs.randn(d, d) / np.sqrt(d)) + shift * rs.randn(d)).astype(np.float32)
    return make(0.0), make(0.3)


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


def host_fid(gt_dev, pred_dev):
    """nan where calculate_frechet_distance refuses the root's imaginary part"""
    gt, pred = gt_dev.cpu().numpy(), pred_dev.cpu().numpy()
    try:
        return _host_fid(gt, pred)
    except ValueError as e:
        print(f'    host: {e}')
        return float('nan')


def _host_fid(gt, pred):
    return evaluation.calculate_frechet_distance(*evaluation.calculate_activation_statistics(gt, 1.0), *evaluation.calculate_activation_statistics(pred, 1.0))


def exact_fid(gt, pred):
    """the nuclear-norm form with LAPACK singular values of the product of the two triangular factors (at most d x d)"""
    a, b = (np.asarray(t, dtype=np.float64) for t in (gt, pred))
    mu1, mu2 = a.mean(axis=0), b.mean(axis=0)
    a, b = a - mu1, b - mu2
    nuc = np.linalg.svd(np.linalg.qr(a, mode='r') @ np.linalg.qr(b, mode='r').T, compute_uv=False).sum()
    s = (mu1 - mu2) @ (mu1 - mu2) + (a * a).sum() / (len(a) - 1) + (b * b).sum() / (len(b) - 1)
    return s - 2 * nuc / np.sqrt((len(a) - 1) * (len(b) - 1)), s


def main():
    p = argparse.ArgumentParser(description='time the device Frechet distance beside the host sqrtm route')
    p.add_argument('--sizes', nargs='+', default=['4096x256', '1024x512', '24x256'], metavar='NxD')
    p.add_argument('--reps', type=int, default=5)
    a = p.parse_args()
    lib.load(require_gpu=True)
    for size in a.sizes:
        n, d = (int(v) for v in size.split('x'))
        gt, pred = tables(n, d, seed=n + d)
        gt_dev, pred_dev = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
        out, info = embmetrics.frechet_distance(gt_dev, pred_dev, return_info=True)
        t_dev = median_ms(lambda: embmetrics.frechet_distance(gt_dev, pred_dev), a.reps)
        t_host = median_ms(lambda: host_fid(gt_dev, pred_dev), max(1, a.reps // 2))
        exact, s = exact_fid(gt, pred)
        dev_fid, h_fid = float(out.item()), float(host_fid(gt_dev, pred_dev))
        launches = sum(info['launches'])
        print(f'two tables [{n}, {d}]: device {t_dev:.1f} ms, host (copy + statistics + sqrtm, fp32 tables) {t_host:.1f} ms; ratio host / device {t_host / t_dev:.2f}')
        print(f'    sweeps {info["sweeps"]}  round launches {info["launches"]} = {launches} ({1e3 * t_dev / max(launches, 1):.1f} us of the device time per launch)')
        print(f'    FID device {dev_fid!r}  host {h_fid!r}  exact {float(exact)!r}; |device - exact| / s {abs(dev_fid - exact) / s:.1e}  |host - exact| / s {abs(h_fid - exact) / s:.1e}')


if __name__ == '__main__':
    main()

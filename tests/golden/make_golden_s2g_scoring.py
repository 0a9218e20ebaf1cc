#!/usr/bin/env python
"""Generate tests/golden/s2g_scoring.npz FROM THE REFERENCE'S OWN beat alignment.

Run where the reference tree is available (MOTIONCRAFT_REFERENCE, as for make_golden_smplx.py):

    python tests/golden/make_golden_s2g_scoring.py

``mogen/datasets/EMAGE_2024/utils/metric.py`` is loaded by file path with ``librosa`` / ``matplotlib`` stubbed in
``sys.modules`` (the module imports them at the top; ``load_pose`` and ``calculate_align`` use neither), and its
``alignment(0.3, 7, mean_vel)`` -- the constructor call of ``tools/s2g_test.py:87`` -- runs on synthetic fp32 joints: sums of four
sinusoids per coordinate at 0.3 .. 2.5 Hz.  Cases: (frames, mask) = (200, 60) [the reference's mask], (40, 8), (33, 0), (17, 0),
each with ``mean_vel`` in float32 and in float64 and with 1, 9 and 300 onset times.  Stored per case: the inputs, the beat frames
per joint (``beats_idx`` cut by ``beats_ptr``) and the align scores.

Every beat decision is a strict comparison of two rounded numbers, so the inputs are searched (seeds in order) until every
decision keeps a relative margin >= 1e-4 in both precisions of ``mean_vel`` and the all-float64 re-evaluation of the rules gives
the same sets; the restatement ``tests/test_scoring_host.py`` holds (the one the device is also checked against) must reproduce
the reference's sets and scores here, or nothing is written.  The achieved margins are recorded in the file.

The fixture holds data only and is written with fixed zip timestamps: a re-run reproduces it byte for byte.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                              # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))             # the repository root

from make_golden_smplx import load_metric, write_npz  # noqa: E402
import test_scoring_host as H  # noqa: E402

CASES = ((200, 60), (40, 8), (33, 0), (17, 0))
N_ONSETS = (1, 9, 300)
SIGMA, ORDER, FPS = 0.3, 7, 30
MAX_SEEDS = 400


def main():
    metric = load_metric()
    out = {'cases.T': np.array([c[0] for c in CASES], np.int64), 'cases.mask': np.array([c[1] for c in CASES], np.int64),
           'cases.n_onsets': np.array(N_ONSETS, np.int64), 'sigma': np.float64(SIGMA), 'order': np.int64(ORDER), 'pose_fps': np.float64(FPS),
           'margin.required': np.float64(H.MARGIN)}
    for T, mask in CASES:
        t0, t1 = mask, T - mask
        for seed in range(1000 * T, 1000 * T + MAX_SEEDS):
            joints, mv64 = H.synthetic_joints(T, seed, FPS)
            found = {}
            for tag, mv in (('f32', mv64.astype(np.float32)), ('f64', mv64)):
                beats, margin = H.beat_sets(H.speeds(joints, FPS, mv), t0, t1, ORDER)
                again, _ = H.beat_sets(H.speeds(joints, FPS, mv, np.float64), t0, t1, ORDER)
                if margin < H.MARGIN or any(not np.array_equal(a, b) for a, b in zip(beats, again)):
                    break
                found[tag] = (mv, beats, margin)
            if len(found) == 2:
                break
        else:
            raise SystemExit(f'T={T}: no seed in {MAX_SEEDS} keeps the margin')
        rs = np.random.RandomState(seed + 7)
        onsets = {n: np.sort(rs.uniform(0.0, (t1 - t0) / FPS, n)) for n in N_ONSETS}
        out[f'T{T}.joints'], out[f'T{T}.seed'] = joints, np.int64(seed)
        for n in N_ONSETS:
            out[f'T{T}.onsets{n}'] = onsets[n]
        for tag, (mv, beats, margin) in found.items():
            ref = metric.alignment(SIGMA, ORDER, mv)
            got = ref.load_pose(joints.reshape(T, 165).copy(), t0, t1, FPS, True)
            assert len(got) == 55
            got = [np.asarray(b, np.int64).reshape(-1) for b in got]
            for j in range(55):
                assert np.array_equal(got[j], beats[j]), (T, tag, j, got[j], beats[j])
            pre = f'T{T}.{tag}.'
            out[pre + 'mean_vel'] = mv
            out[pre + 'beats_ptr'] = np.concatenate([[0], np.cumsum([len(b) for b in got])]).astype(np.int64)
            out[pre + 'beats_idx'] = np.concatenate(got).astype(np.int64)
            out[pre + 'margin'] = np.float64(margin)
            for n in N_ONSETS:
                want = float(ref.calculate_align(onsets[n], ref.load_pose(joints.reshape(T, 165).copy(), t0, t1, FPS, True), FPS))
                assert abs(H.align_score(beats, onsets[n], FPS, SIGMA) - want) <= 1e-12
                out[pre + f'score{n}'] = np.float64(want)
            print(f'T={T} mask={mask} mean_vel {tag}: seed {seed}, {sum(len(b) for b in got)} beats, margin {margin:.2e}, '
                  f'scores {[float(out[pre + f"score{n}"]) for n in N_ONSETS]}')
    path = os.path.join(HERE, 's2g_scoring.npz')
    write_npz(path, out)
    print(f'{path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()

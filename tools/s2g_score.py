#!/usr/bin/env python
"""Score a speech-to-gesture run from its saved files: the six numbers the reference logs at the end of
``tools/s2g_test.py`` (``CustomTrainer.test``, lines 451-483), computed on the device by ``motioncraft_amd.scoring``.

    python tools/s2g_score.py RESULTS_DIR (--wav WAV_DIR [--resample [--load_sr 22050]] | --onsets ONSETS_DIR) --smplx_model SMPLX_NEUTRAL_2020.npz \
        --evaluator CHECKPOINT.pth --mean_vel mean_vel.npy [--device_metrics]

RESULTS_DIR holds the ``res_<id>.npz`` / ``gt_<id>.npz`` pairs the test writes (s2g_test.py:431-448: poses [T,165],
expressions [T,100], trans [T,3], betas [300]).  WAV_DIR holds one ``<id>.wav`` per pair.  Without --resample it is 16-bit PCM,
mono or the first channel, ALREADY at ``--audio_sr``.  With --resample it is integer PCM of any rate, width and channel count,
decoded, mixed to mono and resampled to ``--audio_sr`` on the device (``motioncraft_amd.audio.load_wav``), through ``--load_sr``
first if given: ``--load_sr 22050`` is the ``librosa.load`` + ``librosa.resample`` of s2g_test.py:416-417.  The resampler is
librosa's ``polyphase`` mode, pinned to ``scipy.signal.resample_poly``; it is not the reference's ``soxr_hq``, whose parity stays
unpinned, so the audio differs from the reference's above roughly 0.9 of the Nyquist rate.  The onsets are detected on the device
from the audio cut like s2g_test.py:418-419.  Or ONSETS_DIR holds one ``<id>.npy`` per pair with the onset times in seconds, i.e.
``alignment.load_audio`` of the audio cut by the align mask on both sides.  The sample is re-packed from its saved arrays, so the 322-d channels the ``.npz`` does not
carry (159:209, 312:322) enter the whole-body embedding as zeros.  With --device_metrics the embeddings never leave the device and
the two FIDs are the nuclear-norm form of ``motioncraft_amd.embmetrics``: exact for the singular covariances of a few sequences,
where ``scipy.linalg.sqrtm`` carries a rounding band of its own (about 1e-7 relative).
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import motioncraft_amd as mc                                    # noqa: E402
from motioncraft_amd import audio, scoring, speech              # noqa: E402
from motioncraft_amd.body_model import SMPLXBodyModel           # noqa: E402


def parse_args():
    p = argparse.ArgumentParser(description='score res_*.npz / gt_*.npz pairs of a speech-to-gesture run')
    p.add_argument('results', help='directory with the res_<id>.npz / gt_<id>.npz pairs')
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--wav', metavar='DIR', help='directory with one <id>.wav per pair: 16-bit PCM at --audio_sr; onsets are detected on the device')
    src.add_argument('--onsets', metavar='DIR', help='directory with one <id>.npy of onset times (seconds) per pair')
    p.add_argument('--audio_sr', type=int, default=16000, help='the rate the detector runs at (the reference\'s audio_sr); without --resample the wav files must already have it')
    p.add_argument('--resample', action='store_true', help='decode, mix to mono and resample the wav files to --audio_sr on the device (librosa\'s polyphase mode, not soxr_hq)')
    p.add_argument('--load_sr', type=int, default=None, metavar='N', help='with --resample: go through N Hz first (22050: the reference\'s librosa.load)')
    p.add_argument('--smplx_model', required=True, metavar='PATH', help='the published SMPL-X model file (.npz)')
    p.add_argument('--evaluator', required=True, metavar='PATH', help='checkpoint of the T2MContrastiveModel_SMPLX embedding model')
    p.add_argument('--mean_vel', required=True, metavar='PATH', help='.npy [55]: the mean joint speeds the alignment divides by')
    p.add_argument('--device_metrics', action='store_true', help='keep the embeddings on the device and reduce the two FIDs there (embmetrics.frechet_distance)')
    p.add_argument('--align_mask', type=int, default=60), p.add_argument('--pose_fps', type=float, default=30)
    p.add_argument('--latent_dim', type=int, default=256), p.add_argument('--ff_size', type=int, default=1024)
    p.add_argument('--num_layers', type=int, default=4), p.add_argument('--num_heads', type=int, default=4)
    a = p.parse_args()
    if (a.resample or a.load_sr is not None) and not a.wav:
        p.error('--resample and --load_sr go with --wav')
    if a.load_sr is not None and not a.resample:
        p.error('--load_sr needs --resample')
    return a


def read_wav(path, sr, resample=False, load_sr=None):
    try:
        if resample:
            print(audio.describe(path, sr, load_sr))
            return audio.load_wav(path, sr=sr, load_sr=load_sr)[0]
        return speech.read_wav(path, sr)
    except ValueError as e:
        raise SystemExit(str(e))


def main():
    a = parse_args()
    ids = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(a.results, 'res_*.npz')))
    if not ids:
        raise SystemExit(f'{a.results}: no res_*.npz')
    body = SMPLXBodyModel.from_npz(a.smplx_model)
    enc = dict(latent_dim=a.latent_dim, ff_size=a.ff_size, num_layers=a.num_layers, num_heads=a.num_heads)
    evaluator = mc.build_submodule(dict(type='T2MContrastiveModel_SMPLX', motion_encoder=dict(nfeats=322, vae=True, **enc),
                                        init_cfg=dict(type='Pretrained', checkpoint=a.evaluator)))
    scorer = scoring.S2GScorer(body, evaluator, np.load(a.mean_vel), align_mask=a.align_mask, pose_fps=a.pose_fps, on_device=a.device_metrics)
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))
    for i in ids:
        with np.load(os.path.join(a.results, f'res_{i}.npz')) as res, np.load(os.path.join(a.results, f'gt_{i}.npz')) as gt:
            rec_motion = scoring.pack_motion(t(res['poses']), t(res['expressions']), t(res['trans']))
            source = (dict(audio=read_wav(os.path.join(a.wav, f'{i}.wav'), a.audio_sr, a.resample, a.load_sr), audio_sr=a.audio_sr) if a.wav else
                      dict(onset_times=np.load(os.path.join(a.onsets, f'{i}.npy'))))
            per_seq = scorer.add_sequence(rec_motion, t(gt['poses']), t(gt['expressions']), t(gt['trans']), t(gt['betas']).reshape(-1)[:300],
                                          **source)
        print(f'{i}: {rec_motion.shape[0]} frames  l2 {per_seq["l2"]:.6e}  lvel {per_seq["lvel"]:.6e}  align {per_seq["align"]:.6f}', file=sys.stderr)
    for name, value in scorer.summary().items():
        print(f'{name}: {value}')


if __name__ == '__main__':
    main()

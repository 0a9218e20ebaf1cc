#!/usr/bin/env python
"""Sample a gesture sequence for one speech clip: the front half of the reference's ``tools/s2g_test.py`` (``_g_test``, lines
120-260, and the ``res_<id>.npz`` of lines 440-448) on the device.

    python tools/s2g_sample.py CONFIG CHECKPOINT --wav CLIP.wav [--resample [--load_sr 22050]] [--words w1 w2 ... | --text "w1 w2 ..."] --out DIR \\
        [--mean mean.npy --std std.npy] [--repaint --overlap_len N | --coupled] [--seed S] [--fp16 split|plain] [--graph] [--betas GT.npz] \\
        [--clip_feat feats.npy | --xf_out xf.npy | --random-condition SEED]

CONFIG is an S2G config (``configs/stmogen/S2G_Beats2_*.py``: ``copy_blocks_num``, ``control_cond_feats``,
``condition_encode_cfg`` with ``condition_pre_encode_type='wav'``); CHECKPOINT may be "synthetic[:SEED]".  Without --resample
CLIP.wav is 16-bit PCM, mono or the first channel, ALREADY at 16 kHz, and the waveform goes to the device once.  With --resample
it is integer PCM of any rate, 8 to 32 bits and any channel count: its bytes go to the device once and are decoded, mixed to mono
and resampled to 16 kHz there (``motioncraft_amd.audio.load_wav``); --load_sr 22050 goes through 22 050 Hz first, as the
reference's ``librosa.load`` + ``librosa.resample`` do.  The resampler is librosa's ``polyphase`` mode, pinned to
``scipy.signal.resample_poly``; it is not ``soxr_hq``, the reference's, so the condition differs from the reference's above
roughly 0.9 of the Nyquist rate.  Compressed and float files stay with the caller.  The ``onset+amplitude`` condition
(``motioncraft_amd.speech.AudioCondition``) and the window walk over it stay on the device.  The prompt is 'A person is doing a speech, and the speech content is <words>' for every window; the reference takes each
window's words from a TextGrid, which this tool does not read.  As in ``tools/sample.py``, the prompt reaches the model through
the CLIP tower only when the ``clip`` package is importable: otherwise give --clip_feat / --xf_out / --random-condition.
Writes DIR/res_<id>.npz (<id> = the wav's base name) with the keys ``tools/s2g_score.py`` reads.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

import motioncraft_amd as mc                                    # noqa: E402
from motioncraft_amd import audio, scoring, speech, synthetic   # noqa: E402
from motioncraft_amd.checkpoint import load_checkpoint          # noqa: E402

AUDIO_SR = 16000                                                # the S2G configs' audio_sr; speech.SAMPLES_PER_FRAME = AUDIO_SR // 30


def parse_args():
    p = argparse.ArgumentParser(description='speech-to-gesture sampling from a wav file')
    p.add_argument('config')
    p.add_argument('checkpoint')
    p.add_argument('--wav', required=True, metavar='FILE', help='16-bit PCM at 16 kHz; with --resample integer PCM of any rate, width and channel count')
    p.add_argument('--resample', action='store_true', help='decode, mix to mono and resample to 16 kHz on the device (librosa\'s polyphase mode, not soxr_hq)')
    p.add_argument('--load_sr', type=int, default=None, metavar='N', help='with --resample: go through N Hz first (22050: the reference\'s librosa.load)')
    words = p.add_mutually_exclusive_group()
    words.add_argument('--words', nargs='+', default=None, help='the words of the speech, in order')
    words.add_argument('--text', default=None, help='the same as one string, split at white space')
    p.add_argument('--out', required=True, metavar='DIR')
    p.add_argument('--motion_length', type=int, default=64, help='frames per window (the reference\'s pose_length)')
    p.add_argument('--pre_frames', type=int, default=4, help='frames two neighbouring windows share')
    p.add_argument('--samples_per_frame', type=int, default=speech.SAMPLES_PER_FRAME,
                   help='audio samples per motion frame; the reference fixes 16000 // 30, which a checkpoint of its configs expects')
    p.add_argument('--mean'), p.add_argument('--std')
    p.add_argument('--betas', metavar='NPZ', help='file whose `betas` go into the result (the ground-truth .npz); default zeros')
    p.add_argument('--clip_feat', help='.npy [1,77,512] CLIP text features (ln_final output)')
    p.add_argument('--xf_out', help='.npy [1,77,text_latent_dim] frozen condition embedding')
    p.add_argument('--random-condition', type=int, default=None, metavar='SEED')
    p.add_argument('--seed', type=int, default=0)
    # long-sequence / RePaint options read by the sampler through cfg.model['opt'] (tools/s2g_test.py:551-560)
    p.add_argument('--repaint', action='store_true'), p.add_argument('--overlap_len', type=int, default=0)
    p.add_argument('--same_overlap_noisy', action='store_true'), p.add_argument('--no_resample', action='store_true')
    p.add_argument('--timestep_respacing', default='ddim50'), p.add_argument('--jump_n_sample', type=int, default=5)
    p.add_argument('--jump_length', type=int, default=3), p.add_argument('--addBlend', type=bool, default=True)
    p.add_argument('--no_repaint', action='store_true')
    p.add_argument('--coupled', action='store_true',
                   help='all windows of the clip in ONE batch, the --pre_frames shared frames of neighbours blended at every step (no seam, no '
                        'sequential windows; 0 < 2 pre_frames <= motion_length)')
    p.add_argument('--fp16', choices=['split', 'plain'], default=None, help='fp16-MFMA mode: split = fp32-class hi/lo form')
    p.add_argument('--graph', action='store_true', help='hipGraph replay of the sampler step')
    a = p.parse_args()
    if a.load_sr is not None and not a.resample:
        p.error('--load_sr needs --resample')
    if a.coupled and (a.repaint or a.graph):
        p.error('--coupled is a window mode of its own: it goes with neither --repaint nor --graph')
    return a


def main():
    a = parse_args()
    cfg = mc.Config.fromfile(a.config)
    cfg.model['opt'] = a
    model = mc.build_architecture(cfg.model)
    model.model = mc.ControlT2MHalf(model.model, copy_blocks_num=cfg.copy_blocks_num, control_cond_feats=cfg.control_cond_feats, cfg=cfg)
    if a.checkpoint.startswith('synthetic'):
        seed = int(a.checkpoint.split(':')[1]) if ':' in a.checkpoint else 0
        sd = synthetic.make_control_wav_state(model.model.dims, cfg.copy_blocks_num, cfg.control_cond_feats, seed)
        model.load_state_dict({'model.' + k: v for k, v in sd.items()})
    else:
        load_checkpoint(model, a.checkpoint, map_location='cpu')
    model.eval()
    if a.fp16 or cfg.get('fp16', None) is not None:
        mc.wrap_fp16_model(model, split=(a.fp16 != 'plain'))
    dims = model.model.dims
    try:
        if a.resample:
            print(audio.describe(a.wav, AUDIO_SR, a.load_sr))
            wav, _ = audio.load_wav(a.wav, sr=AUDIO_SR, load_sr=a.load_sr)
        else:
            wav = speech.read_wav(a.wav, AUDIO_SR)
    except ValueError as e:
        raise SystemExit(str(e))
    dev = torch.device('cuda', torch.cuda.current_device())
    cond_kw = {}
    if a.xf_out:
        cond_kw['xf_out'] = torch.from_numpy(np.load(a.xf_out)).float().to(dev)
    elif a.clip_feat:
        cond_kw['clip_feat'] = torch.from_numpy(np.load(a.clip_feat)).float().to(dev)
    elif a.random_condition is not None:
        g = torch.Generator().manual_seed(a.random_condition)
        cond_kw['xf_out'] = torch.nn.functional.layer_norm(torch.randn(1, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    words = a.words if a.words is not None else (a.text or '').split()
    stats = dict(mean=np.load(a.mean) if a.mean else None, std=np.load(a.std) if a.std else None)
    if a.coupled:
        recs, wins = speech.sample_speech(model, wav, words=words, motion_length=a.motion_length, pre_frames=a.pre_frames,
                                          samples_per_frame=a.samples_per_frame, coupled=True, input_dim=dims['input_feats'],
                                          condition_kwargs=cond_kw, inference_kwargs=dict(generator=gen), shard=False, **stats)
        rec, windows = recs[0], [wins[(0, w)] for w in range(len(wins))]
    else:
        rec, windows = speech.sample_speech(
            model, wav, words=words, motion_length=a.motion_length, pre_frames=a.pre_frames,
            samples_per_frame=a.samples_per_frame, repaint=a.repaint, overlap_len=a.overlap_len, fix_very_first=False,
            input_dim=dims['input_feats'], condition_kwargs=cond_kw,
            inference_kwargs=dict(generator=gen, **({'graph': True} if a.graph else {})), **stats)
    pose, exps, trans = scoring.unpack_rec_motion(torch.from_numpy(rec))           # s2g_test.py:289-297
    if a.betas:
        with np.load(a.betas) as f:
            betas = f['betas']
    else:
        betas = np.zeros(300)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, 'res_' + os.path.splitext(os.path.basename(a.wav))[0] + '.npz')
    np.savez(path, betas=betas, poses=pose.numpy(), expressions=exps.numpy(), trans=trans.numpy(), model='smplx2020', gender='neutral',
             mocap_frame_rate=30)                                                   # s2g_test.py:440-448
    print(f'{len(wav)} samples -> {len(windows)} windows of {a.motion_length} frames -> {rec.shape[0]} frames -> {path}')


if __name__ == '__main__':
    main()

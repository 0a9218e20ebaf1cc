"""The front half of the speech-to-gesture (S2G) test, ``tools/s2g_test.py``: from a waveform to the sampled gesture sequence.

  * ``AudioCondition``: the ``onset+amplitude`` audio representation the S2G configs feed the WavEncoder (``audio_rep`` of
    ``mogen/datasets/EMAGE_2024/configs/st_mogen_emage.yaml``), built as in ``dataloaders/beat_motionx.py:398-412``: a 1024-sample
    rolling maximum of ``|y|`` next to a one-hot column of librosa onsets, float32 [samples, 2].  It is built on the device
    (``mc_audio_condition``, ``csrc/mc_audiocond.hip``, fed the onset mask of ``scoring.OnsetDetector``) from one upload of the
    waveform and stays there.  Parity is pinned to the numpy restatement ``tests/audio_cond_ref.py``, bit for bit.
  * ``speech_frames`` / ``speech_prompt`` / ``sample_speech``: the frame count, the text prompt and the window walk of
    ``CustomTrainer._g_test`` (s2g_test.py:120-260) on ``longform.sample_long`` with 533 audio samples per frame.
  * ``read_wav``: the 16-bit PCM reader of the two S2G tools, for a file already at the model's rate.

Other integer PCM files -- any rate, width and channel count -- are decoded, mixed to mono and resampled on the device by
``motioncraft_amd.audio.load_wav`` (the two tools' ``--resample``): the reference's ``librosa.load`` + ``librosa.resample`` in
librosa's ``polyphase`` mode, pinned to scipy; it is not ``soxr_hq``, so a condition built this way differs from the reference's
above roughly 0.9 of the Nyquist rate.  Compressed and float files stay with the caller, and so does the source of the prompt's
words (the reference reads them per frame from a TextGrid through its vocabulary).  Nothing here falls back to the host: a missing library or GPU is an error.
"""
import wave

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _p, stream as _stream
from . import longform
from .scoring import OnsetDetector

AUDIO_COND_TILE = _lib.MC_AUDIO_COND_TILE                                # output samples per workgroup
MAX_WINDOW = _lib.MC_AUDIO_COND_MAX_WINDOW
SAMPLES_PER_FRAME = 16000 // 30                                          # s2g_test.py:155: audio rows per motion frame
PROMPT = 'A person is doing a speech, and the speech content is '        # s2g_test.py:175


def read_wav(path, sr):
    """16-bit PCM wav at ``sr`` -> float32 [N] in [-1, 1): the first channel, scaled by 1 / 32768.  Anything else is a ValueError."""
    with wave.open(path, 'rb') as f:
        if f.getsampwidth() != 2 or f.getcomptype() != 'NONE':
            raise ValueError(f'{path}: {8 * f.getsampwidth()}-bit {f.getcomptype()} samples; this tool reads 16-bit PCM only (decode it first)')
        if f.getframerate() != sr:
            raise ValueError(f'{path}: {f.getframerate()} Hz, but the detector runs at {sr} Hz.  Resampling stays with the caller: the '
                             f'reference resamples with librosa.resample (soxr), which is not restated here; resample the file to {sr} Hz first')
        data = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2').reshape(-1, f.getnchannels())
    return data[:, 0].astype(np.float32) / 32768.0


class AudioCondition:
    """``onset+amplitude`` of beat_motionx.py:398-412 on the device.  Column 0: ``max |y[s : s + frame_length]|`` with
    ``s = min(i, N - frame_length)`` -- the last full window's value is repeated over the final ``frame_length - 1`` samples.
    Column 1: ones at the onset FRAME indices of ``librosa.onset.onset_detect(y, sr, units='frames')`` (hop ``hop_length``),
    written into the sample-indexed column as they are -- the reference does that, and the checkpoints are trained on it."""

    def __init__(self, sr=16000, frame_length=1024, hop_length=512):
        self.frame_length = int(frame_length)
        if not 1 <= self.frame_length <= MAX_WINDOW:
            raise ValueError(f'frame_length={frame_length}: 1..{MAX_WINDOW}')
        self.detector = OnsetDetector(sr=sr, hop_length=hop_length)

    def _wave(self, y, window):
        t = OnsetDetector._check_wave(y)
        if t.numel() < window:
            raise ValueError(f'{t.numel()} samples hold no full window of {window}')
        return t.to(device=t.device if t.is_cuda else 'cuda', dtype=torch.float32).contiguous()

    @staticmethod
    def _run(t, window, mask):
        lib = _lib.load(require_gpu=True)
        out = torch.empty(t.numel(), 2, device=t.device, dtype=torch.float32)
        _lib.check(lib.mc_audio_condition(_p(t), t.numel(), window, _p(mask) if mask is not None else None, 0 if mask is None else mask.numel(),
                                          _p(out), _stream()), 'mc_audio_condition')
        return out

    def __call__(self, y):
        """y [N] (device tensor, or anything ``torch.as_tensor`` takes) -> the condition, device fp32 [N, 2]."""
        t = self._wave(y, self.frame_length)
        if self.detector.num_frames(t.numel()) > t.numel():
            raise ValueError(f'{t.numel()} samples at hop {self.detector.hop_length}: more onset frames than samples to mark them in')
        # _strength, not strength: t has passed _check_wave above and is on the device; strength would run the finiteness pass (a
        # device synchronisation) a second time
        mask, _ = self.detector.pick(self.detector._strength(t))
        return self._run(t, self.frame_length, mask)

    def amplitude_envelope(self, y, window=None):
        """column 0 alone, device fp32 [N]; ``window`` defaults to ``frame_length``."""
        window = self.frame_length if window is None else int(window)
        if not 1 <= window <= MAX_WINDOW:
            raise ValueError(f'window={window}: 1..{MAX_WINDOW}')
        return self._run(self._wave(y, window), window, None)[:, 0]


def speech_frames(n_samples, samples_per_frame=SAMPLES_PER_FRAME, multiple=8):
    """The motion frames a clip of ``n_samples`` gives: whole frames of audio, trimmed down to a multiple of 8 (s2g_test.py:130-137)."""
    n = int(n_samples) // int(samples_per_frame)
    return n - n % int(multiple)


def speech_prompt(words):
    """s2g_test.py:170-176: the prompt of a window from its words, each non-empty word once, in first-seen order."""
    return PROMPT + ' '.join(w for w in dict.fromkeys(words) if w != '')


def sample_speech(model, wave, words=(), motion_length=64, pre_frames=4, samples_per_frame=SAMPLES_PER_FRAME, condition=None,
                  batched=False, coupled=False, **driver_kwargs):
    """wave [N] at the condition's rate -> the gesture sequence of ``speech_frames(N)`` frames: the condition is built on the device,
    and window i of ``motion_length`` frames reads its rows ``[i * stride * spf, (i * stride + motion_length) * spf)``,
    stride = ``motion_length - pre_frames`` (s2g_test.py:144-155).  ``words``: the words of the prompt (one prompt for the clip;
    the reference forms it per window from a TextGrid, which is not read here).  ``condition``: an ``AudioCondition`` (default: a new
    one).  ``driver_kwargs`` go to the window driver: repaint, overlap_len, fix_very_first, first_gt, mean, std, gt_space,
    condition_kwargs, inference_kwargs, ...  Returns what ``longform.sample_long`` returns, or with ``batched=True`` what
    ``longform.sample_long_batched`` returns for this one sequence.  ``coupled=True``: all windows of the clip in one batch with their
    shared frames coupled at every step (``longform.sample_long_coupled``; ``pre_frames`` is the overlap, ``driver_kwargs`` are that
    driver's: weights, noise, mean, std, condition_kwargs, inference_kwargs, max_batch, ...); returns what that driver returns."""
    if coupled and batched:
        raise ValueError('coupled and batched name two different window drivers: pick one')
    cond = (condition if condition is not None else AudioCondition())(wave)
    total = speech_frames(cond.shape[0], samples_per_frame)
    text = speech_prompt(words)
    if coupled:
        return longform.sample_long_coupled(model, [total], motion_length, pre_frames, c=[cond], text=[text],
                                            c_rows_per_frame=samples_per_frame, **driver_kwargs)
    if batched:
        return longform.sample_long_batched(model, [total], motion_length, pre_frames, c=[cond], text=[text],
                                            c_rows_per_frame=samples_per_frame, **driver_kwargs)
    return longform.sample_long(model, total, motion_length, pre_frames, c=cond, text=text, c_rows_per_frame=samples_per_frame, **driver_kwargs)

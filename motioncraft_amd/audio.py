"""From a PCM wav file to the waveform the S2G front reads, on the device: decode, mono mix and rational resampling.

The reference reads its audio with ``librosa.load(path)`` -- libsndfile decode, ``librosa.to_mono``, resampling to librosa's default
22 050 Hz -- followed by ``librosa.resample(..., target_sr=16000)`` (``dataloaders/beat_sep_lower.py:392-393``,
``tools/s2g_test.py:416-417``): even a 16 kHz file goes 16 000 -> 22 050 -> 16 000 before the model or the scorer sees it.

  * ``load_wav``: header and raw bytes through ``wave``, ONE upload of the bytes, ``mc_pcm_decode`` and ``mc_resample_poly``
    (``csrc/mc_resample.hip``) on the device.  ``load_sr=22050`` walks the reference's detour.
  * ``Resampler``: one rational ratio with its filter kept on the device.
  * ``resample_filter``: scipy's own default design for ``resample_poly``.

The resampler is librosa's ``res_type='polyphase'`` mode, which is exactly ``scipy.signal.resample_poly(y, target // gcd,
orig // gcd)``; it is pinned to scipy itself (``tests/test_resample_host.py``, ``tests/test_resample_gpu.py``).  It is NOT
``soxr_hq``, librosa's default and what the reference's checkpoints were trained behind: parity with ``soxr_hq`` stays unpinned,
and a condition built this way differs from the reference's above roughly 0.9 of the Nyquist rate, where the two filters' transition
bands differ.  Nothing here falls back to the host: a missing library or GPU is an error.
"""
import functools
import math
import wave

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _p, stream as _stream

RESAMPLE_TILE = _lib.MC_RESAMPLE_TILE                                    # outputs per workgroup
LIBROSA_LOAD_SR = 22050                                                  # librosa.load's default rate, the reference's detour


def resample_filter(up, down, window=('kaiser', 5.0)):
    """The fp64 taps ``scipy.signal.resample_poly(x, up, down, window=window)`` designs for itself, already multiplied by ``up``:
    ``firwin(2 * 10 * max(up, down) + 1, 1 / max(up, down), window=window) * up``.  Odd length, centred."""
    from scipy.signal import firwin
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f'up={up}, down={down}: both >= 1')
    m = max(up, down)
    return firwin(2 * 10 * m + 1, 1.0 / m, window=window) * up


def out_len(n_in, up, down):
    """``ceil(n_in * up / down)``: the length scipy's ``resample_poly`` and librosa's ``resample`` give."""
    return -(-int(n_in) * int(up) // int(down))


def phase_major(taps, up):
    """taps fp64 [n_taps] -> fp64 [up, L], L = ceil(n_taps / up): row p holds the taps of phase p in the order an output walks them
    with ascending input index, ``table[p, i] = taps[p + (L - 1 - i) * up]``, zero past the filter's end (``mc_resample_poly``)."""
    taps = np.asarray(taps, dtype=np.float64)
    L = -(-taps.size // up)
    padded = np.zeros(up * L)
    padded[:taps.size] = taps
    return padded.reshape(L, up).T[:, ::-1].copy()                       # a copy, not ascontiguousarray: L = 1 would keep the negative stride


class Resampler:
    """``orig_sr`` -> ``target_sr`` on the device with the semantics of ``scipy.signal.resample_poly`` (zero padding), i.e. of
    ``librosa.resample(..., res_type='polyphase')``.  The rates are reduced by their gcd; the phase-major taps go to the device once.
    ``taps``: an odd-length fp64 filter of the caller's, already multiplied by ``up`` (default: ``resample_filter``)."""

    def __init__(self, orig_sr, target_sr, taps=None):
        orig_sr, target_sr = int(orig_sr), int(target_sr)
        if orig_sr < 1 or target_sr < 1:
            raise ValueError(f'rates {orig_sr} -> {target_sr}: both >= 1')
        g = math.gcd(orig_sr, target_sr)
        self.orig_sr, self.target_sr, self.up, self.down = orig_sr, target_sr, target_sr // g, orig_sr // g
        self.identity = self.up == self.down == 1                         # as in scipy: the input itself, whatever the taps
        self.taps, self._tables = None, {}                                # the phase-major taps, one copy per device
        if self.identity:
            return
        taps = resample_filter(self.up, self.down) if taps is None else np.array(taps, dtype=np.float64)
        if taps.ndim != 1 or taps.size % 2 != 1:
            raise ValueError(f'taps of shape {taps.shape}: one odd-length filter centred on a sample')
        if not np.isfinite(taps).all():
            raise ValueError('taps are not finite')
        self.taps = taps
        _lib.load(require_gpu=True)
        self._host_table = torch.from_numpy(phase_major(taps, self.up))
        self._table(torch.device('cuda', torch.cuda.current_device()))

    def _table(self, device):
        if device not in self._tables:
            self._tables[device] = self._host_table.to(device)
        return self._tables[device]

    def out_len(self, n_in):
        return out_len(n_in, self.up, self.down)

    def __call__(self, y):
        """y: device fp32 [N] -> device fp32 [ceil(N * up / down)]; the identity ratio returns ``y`` itself."""
        if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 1 and y.numel() >= 1):
            raise ValueError('the resampler takes a non-empty device float32 tensor [N]')
        if self.identity:
            return y
        y = y.contiguous()
        table = self._table(y.device)
        lib = _lib.load(require_gpu=True)
        out = torch.empty(self.out_len(y.numel()), device=y.device, dtype=torch.float32)
        with torch.cuda.device(y.device):                                 # the launch goes to the clip's device, on its current stream
            _lib.check(lib.mc_resample_poly(_p(y), y.numel(), self.up, self.down, _p(table), self.taps.size, _p(out), out.numel(),
                                            _stream(y.device)), 'mc_resample_poly')
        return out


@functools.lru_cache(maxsize=16)
def _resampler(orig_sr, target_sr):
    return Resampler(orig_sr, target_sr)


def wav_header(path):
    """(rate, channels, sample_bytes, n_frames) of a PCM wav file; a compressed or non-PCM one is a ValueError."""
    try:
        with wave.open(path, 'rb') as f:
            if f.getcomptype() != 'NONE':
                raise ValueError(f'{path}: {f.getcomptype()} compression; only uncompressed integer PCM is decoded')
            return f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
    except (wave.Error, EOFError) as e:
        raise ValueError(f'{path}: not an integer PCM wav file ({e})') from None


def rate_chain(file_sr, sr=None, load_sr=None):
    """The rates a file at ``file_sr`` goes through: ``[file_sr, load_sr, sr]`` without the stages that are absent."""
    chain = [int(file_sr)]
    for r in (load_sr, sr):
        if r is not None:
            chain.append(int(r))
    return chain


def describe(path, sr=None, load_sr=None):
    """One line for a tool's output: the file's rate, channels and width, and the rates ``load_wav`` takes it through."""
    rate, channels, width, n_frames = wav_header(path)
    return (f'{path}: {rate} Hz, {channels} channel{"s" if channels != 1 else ""}, {8 * width}-bit PCM, {n_frames} frames; '
            + ' -> '.join(str(r) for r in rate_chain(rate, sr, load_sr)) + ' Hz on the device (polyphase, not soxr_hq)')


def decode_pcm(raw, channels, sample_bytes, mono=True):
    """raw: device uint8 [n_frames * channels * sample_bytes], a wav file's data chunk -> device fp32 [n_frames] in [-1, 1):
    the mean of the channels (``mono``) or channel 0 alone, scaled by ``2 ** -(8 * sample_bytes - 1)`` (``mc_pcm_decode``)."""
    frame = int(channels) * int(sample_bytes)
    if not (torch.is_tensor(raw) and raw.is_cuda and raw.dtype == torch.uint8 and raw.dim() == 1 and raw.is_contiguous()):
        raise ValueError('decode_pcm takes a contiguous device uint8 tensor [bytes]')
    if frame < 1 or raw.numel() < frame or raw.numel() % frame:
        raise ValueError(f'{raw.numel()} bytes are no whole number (>= 1) of frames of {channels} x {sample_bytes} bytes')
    lib = _lib.load(require_gpu=True)
    out = torch.empty(raw.numel() // frame, device=raw.device, dtype=torch.float32)
    with torch.cuda.device(raw.device):
        _lib.check(lib.mc_pcm_decode(_p(raw), out.numel(), int(channels), int(sample_bytes), int(bool(mono)), _p(out), _stream(raw.device)),
                   'mc_pcm_decode')
    return out


def load_wav(path, sr=None, mono=True, load_sr=None):
    """An integer PCM wav of any rate, 8 to 32 bits, any channel count -> ``(device fp32 [N], rate)``.  The file's bytes are uploaded
    once and decoded on the device: the mean of the channels (``mono=True``: ``librosa.to_mono``) or the first channel.  With
    ``sr`` the waveform is resampled to it; with ``load_sr`` it first goes to ``load_sr`` -- ``load_sr=22050, sr=16000`` is the
    reference's ``librosa.load`` + ``librosa.resample`` detour, in librosa's ``polyphase`` mode (not ``soxr_hq``).  The length
    follows ``ceil(n * target / orig)`` at each stage, as librosa's does.  Without ``sr`` and ``load_sr`` the rate is the file's."""
    rate, channels, width, n_frames = wav_header(path)
    if n_frames < 1:
        raise ValueError(f'{path}: no samples')
    _lib.load(require_gpu=True)
    with wave.open(path, 'rb') as f:
        raw = f.readframes(n_frames)
    y = decode_pcm(torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda(), channels, width, mono)
    chain = rate_chain(rate, sr, load_sr)
    for a, b in zip(chain, chain[1:]):
        y = _resampler(a, b)(y)
    return y, chain[-1]

"""Rendered frames -> one playable file, encoded on the device: Motion-JPEG in an AVI container, with the speech as a PCM track.

The reference ends its tools with two ffmpeg child processes, ``convert_img_to_mp4`` and ``add_audio_to_video``
(mogen/datasets/EMAGE_2024/utils/media.py:4-33).  Here ``JpegEncoder`` turns the uint8 frames ``render.MeshRenderer`` and
``skeleton.SkeletonRenderer`` leave in HBM into baseline JPEG files with the HIP encoder ``mc_mjpeg_*`` (``csrc/mc_mjpeg.hip``: integer
arithmetic only, its byte stream is restated in ``tests/jpeg_ref.py``), so only compressed bytes cross to the host, and ``AviWriter``
wraps them with the standard library alone.  Every player reads the result, and ffmpeg remuxes it to mp4 without re-encoding
(``ffmpeg -i clip.avi -c copy clip.mp4`` for the video; PCM audio wants ``-c:a aac``).  No inter-frame codec, no OpenDML: a file ends
below 2^31 bytes.
"""
import fractions
import os
import struct

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _p, stream as _stream

DEFAULT_WORK_BYTES = 256 << 20
OUT_BYTES = 256 << 20                              # device bytes of encoded output per call: frames go through in groups whose BOUND fits
MAX_SIZE = _lib.MC_MJPEG_MAX_SIZE
SUBSAMPLINGS = {'4:2:0': _lib.MC_MJPEG_420, '4:4:4': _lib.MC_MJPEG_444}
RIFF_LIMIT = 2 ** 31 - 1


def _size(width, height):
    for name, v in (('width', width), ('height', height)):
        if not (isinstance(v, (int, np.integer)) and 1 <= v <= MAX_SIZE):
            raise ValueError(f'{name} must be an integer in 1..{MAX_SIZE}, got {v!r}')
    return int(width), int(height)


class JpegEncoder:
    """``JpegEncoder(width, height)``; ``.encode(frames)`` takes uint8 [n, H, W, 3] on the device and returns ``n`` ``bytes``, one
    complete JPEG file each.  ``quality`` 1..100 scales the Annex K tables by the IJG rule; ``subsampling`` '4:2:0' or '4:4:4'.  The
    native object is created at the first ``encode``; ``close()`` frees it."""

    def __init__(self, width, height, quality=90, subsampling='4:2:0'):
        self.width, self.height = _size(width, height)
        if not (isinstance(quality, (int, np.integer)) and 1 <= quality <= 100):
            raise ValueError(f'quality must be an integer in 1..100, got {quality!r}')
        if subsampling not in SUBSAMPLINGS:
            raise ValueError(f'subsampling must be one of {sorted(SUBSAMPLINGS)}, got {subsampling!r}')
        self.quality, self.subsampling = int(quality), subsampling
        self._native, self._work = None, None

    def native(self):
        if self._native is None:
            self._native = _lib.NativeObject('mjpeg', self.width, self.height, self.quality, SUBSAMPLINGS[self.subsampling])
        return self._native

    def close(self):
        self._work = None
        if self._native is not None:
            self._native.close()
            self._native = None

    def max_bytes(self, frames=1):
        """The bound of ``mc_mjpeg_max_bytes``: what ``frames`` frames can encode to at most, whatever they show."""
        obj = self.native()
        return int(obj.lib.mc_mjpeg_max_bytes(obj.handle, frames))

    def encode(self, frames, work_bytes=DEFAULT_WORK_BYTES):
        """Frames run in chunks that fit ``work_bytes`` of scratch (raised to one frame's need); the result does not depend on it.
        Only the encoded bytes and their offsets are copied to the host."""
        return [data for files in self.encode_groups(frames, work_bytes) for data in files]

    def encode_groups(self, frames, work_bytes=DEFAULT_WORK_BYTES):
        """``encode`` by turns: yields the files of one group of frames after the other -- as many frames as ``OUT_BYTES`` of output
        buffer hold under the bound -- so that a long clip is never on the host as a whole."""
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
            raise ValueError(f'frames must be a uint8 tensor, got {getattr(frames, "dtype", type(frames).__name__)}')
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.height, self.width, 3):
            raise ValueError(f'frames must be [n, {self.height}, {self.width}, 3], got {tuple(frames.shape)}')
        if not frames.is_cuda:
            raise ValueError('frames must be in device (HBM) memory: there is no host encoder')
        if not (isinstance(work_bytes, (int, np.integer)) and work_bytes >= 0):
            raise ValueError(f'work_bytes must be a non-negative integer, got {work_bytes!r}')
        obj = self.native()
        x, dev = frames.contiguous(), frames.device
        n = x.shape[0]
        group = max(1, min(n, OUT_BYTES // self.max_bytes(1)))
        need = lambda k: int(obj.lib.mc_mjpeg_work_bytes(obj.handle, k))
        wb = max(min(int(work_bytes), need(group)), need(1))
        if self._work is None or self._work[0] != (dev, wb):                      # the scratch is kept between calls; its contents are not
            self._work = None                                                       # (the old one goes before the new one comes)
            self._work = ((dev, wb), torch.empty(wb, device=dev, dtype=torch.uint8))
        work = self._work[1]
        for f0 in range(0, n, group):
            with torch.cuda.device(dev):
                stream = _stream(dev)
                k = min(group, n - f0)
                cap = self.max_bytes(k)
                out = torch.empty(cap, device=dev, dtype=torch.uint8)
                offsets = torch.empty(k + 1, device=dev, dtype=torch.int64)
                _lib.check(obj.lib.mc_mjpeg_encode(obj.handle, _p(x[f0:]), k, _p(work), wb, _p(out), cap, _p(offsets), stream), 'mc_mjpeg_encode')
                at = offsets.cpu().tolist()                 # waits for the stream
                data = out[:at[k]].cpu().numpy().tobytes()
            yield [data[at[i]:at[i + 1]] for i in range(k)]


def _chunk(tag, payload):
    return tag + struct.pack('<I', len(payload)) + payload + b'\0' * (len(payload) & 1)


class AviWriter:
    """RIFF ``AVI `` with one ``vids`` / ``MJPG`` stream and, when ``audio_rate`` is given, one ``auds`` stream of 16-bit PCM.

    ``hdrl`` holds ``avih`` and a ``strl`` (``strh`` + ``strf``) per stream; ``movi`` holds one ``00dc`` chunk per frame, each followed by
    that frame's share of the audio as ``01wb``; ``idx1`` follows.  Chunks are word-aligned.  ``fps`` is written as the exact fraction
    ``Fraction(fps).limit_denominator(1001)`` in ``dwRate / dwScale`` (30000 / 1001 stays 30000 / 1001), and frame ``i`` carries
    ``round((i + 1) rate / fps) - round(i rate / fps)`` samples with that fraction as ``fps``.

    Audio is taken from what ``add_audio`` has queued when a frame is written, so add it BEFORE the frames it belongs to; a frame that
    finds the queue short gets silence, and what is still queued at ``close`` is dropped: audio longer than the video is cut, shorter
    audio is padded, the reference's ``-shortest`` in the one direction that matters.  No OpenDML: a frame that would take the file past
    ``limit`` (2^31 - 1 bytes, index included) raises ``ValueError`` before anything of it is written, and ``close`` still leaves a
    complete file of the frames before it.  Takes any JPEG bytes."""

    def __init__(self, path, width, height, fps, audio_rate=None, audio_channels=1, limit=RIFF_LIMIT):
        self.width, self.height = _size(width, height)
        if not (isinstance(fps, (int, float, fractions.Fraction, np.integer, np.floating)) and fps > 0 and fps < 1e6):
            raise ValueError(f'fps must be a positive number, got {fps!r}')
        self.fps = fractions.Fraction(float(fps) if isinstance(fps, (np.integer, np.floating)) else fps).limit_denominator(1001)
        if not self.fps > 0:
            raise ValueError(f'fps={fps!r} is no fraction with a denominator up to 1001')
        if audio_rate is not None and not (isinstance(audio_rate, (int, np.integer)) and 1 <= audio_rate <= 2 ** 31 - 1):
            raise ValueError(f'audio_rate must be None or a positive integer, got {audio_rate!r}')
        if not (isinstance(audio_channels, (int, np.integer)) and 1 <= audio_channels <= 64):
            raise ValueError(f'audio_channels must be an integer in 1..64, got {audio_channels!r}')
        if not (isinstance(limit, (int, np.integer)) and 0 < limit <= RIFF_LIMIT):
            raise ValueError(f'limit must be an integer in 1..{RIFF_LIMIT}, got {limit!r}')
        if audio_rate is not None and audio_rate * 2 * audio_channels >= 2 ** 32:
            raise ValueError(f'audio_rate={audio_rate} x {audio_channels} channels: the bytes per second do not fit the header')
        self.audio_rate = None if audio_rate is None else int(audio_rate)
        self.channels, self.limit = int(audio_channels), int(limit)
        self.frames, self.samples = 0, 0                    # written so far
        self._queue = np.zeros((0, self.channels), np.int16)
        self._index, self._largest = [], [0, 0]             # (tag, offset from 'movi', length); the largest chunk of each stream
        self._movi, self._end = 0, 4                        # the header's length does not depend on what it counts
        head = len(self._header())
        self._movi, self._end = head - 4, head              # idx1 counts from the 'movi' tag; the chunks start behind it
        self._fh = open(path, 'wb')
        self._fh.write(self._header())

    def _header(self):
        """RIFF .. the 'movi' tag, with the counts and sizes as they stand now (written first, written again by ``close``)."""
        rate, scale = self.fps.numerator, self.fps.denominator
        W, H, n = self.width, self.height, self.frames
        movi_bytes = self._end - self._movi                 # the 'movi' tag and the chunks
        index_bytes = 8 + 16 * len(self._index)
        per_sec = min(int(movi_bytes * rate / (n * scale)), 2 ** 32 - 1) if n else 0
        streams = _chunk(b'LIST', b'strl' + _chunk(b'strh', struct.pack(
            '<4s4sIHHIIIIIIIIhhhh', b'vids', b'MJPG', 0, 0, 0, 0, scale, rate, 0, n, self._largest[0], 0xFFFFFFFF, 0, 0, 0, W, H)) + _chunk(
            b'strf', struct.pack('<IiiHH4sIiiII', 40, W, H, 1, 24, b'MJPG', 3 * W * H, 0, 0, 0, 0)))
        if self.audio_rate is not None:
            align = 2 * self.channels
            streams += _chunk(b'LIST', b'strl' + _chunk(b'strh', struct.pack(
                '<4s4sIHHIIIIIIIIhhhh', b'auds', b'\0\0\0\0', 0, 0, 0, 0, 1, self.audio_rate, 0, self.samples, self._largest[1], 0xFFFFFFFF, align,
                0, 0, 0, 0)) + _chunk(b'strf', struct.pack('<HHIIHHH', 1, self.channels, self.audio_rate, self.audio_rate * align, align, 16, 0)))
        avih = _chunk(b'avih', struct.pack('<14I', int(round(1e6 * scale / rate)), per_sec, 0, 0x110, n, 0, 1 + (self.audio_rate is not None),
                                           max(self._largest), W, H, 0, 0, 0, 0))        # AVIF_HASINDEX | AVIF_ISINTERLEAVED
        hdrl = _chunk(b'LIST', b'hdrl' + avih + streams)
        riff = 4 + len(hdrl) + 8 + movi_bytes + index_bytes
        return b'RIFF' + struct.pack('<I', riff) + b'AVI ' + hdrl + b'LIST' + struct.pack('<I', movi_bytes) + b'movi'

    def add_audio(self, samples):
        """int16 [samples] (one channel) or [samples, channels]: queued for the frames written after it."""
        if self.audio_rate is None:
            raise ValueError('this file has no audio stream: give audio_rate')
        a = samples.cpu().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
        if a.dtype != np.int16 or a.ndim not in (1, 2) or a.reshape(a.shape[0], -1).shape[1] != self.channels:
            raise ValueError(f'audio must be int16 [samples] or [samples, {self.channels}], got {a.dtype} {a.shape}')
        self._queue = np.concatenate([self._queue, a.reshape(a.shape[0], self.channels)])

    def add_frames(self, jpegs):
        """A list of ``bytes``, one JPEG file per frame (one ``bytes`` is one frame)."""
        if self._fh is None:
            raise ValueError('the file is closed')
        if isinstance(jpegs, (bytes, bytearray, memoryview)):
            jpegs = [jpegs]
        for data in jpegs:
            data = bytes(data)
            if data[:2] != b'\xff\xd8':
                raise ValueError('a frame must be the bytes of a JPEG file (SOI first)')
            chunks = [(b'00dc', data)]
            if self.audio_rate is not None:
                count = round((self.frames + 1) * self.audio_rate / self.fps) - round(self.frames * self.audio_rate / self.fps)
                pcm = self._queue[:count]
                if pcm.shape[0] < count:
                    pcm = np.concatenate([pcm, np.zeros((count - pcm.shape[0], self.channels), np.int16)])
                chunks.append((b'01wb', pcm.astype('<i2').tobytes()))
            body = b''.join(_chunk(tag, payload) for tag, payload in chunks)
            if self._end + len(body) + 8 + 16 * (len(self._index) + len(chunks)) > self.limit:
                raise ValueError(f'frame {self.frames} would take the file past {self.limit} bytes, the RIFF limit without OpenDML: '
                                 'write a shorter clip, a smaller frame or a lower quality')
            at = self._end - self._movi
            for s, (tag, payload) in enumerate(chunks):
                self._index.append((tag, at, len(payload)))
                self._largest[s] = max(self._largest[s], len(payload))
                at += 8 + len(payload) + (len(payload) & 1)
            self._fh.write(body)
            self._end += len(body)
            self.frames += 1
            if self.audio_rate is not None:
                self.samples += count
                self._queue = self._queue[count:]

    def close(self):
        if self._fh is None:
            return
        fh, self._fh = self._fh, None
        try:
            fh.write(_chunk(b'idx1', b''.join(struct.pack('<4sIII', tag, 0x10, at, size) for tag, at, size in self._index)))   # AVIIF_KEYFRAME
            fh.seek(0)
            fh.write(self._header())
        finally:
            fh.close()

    def abandon(self):
        """Close the file as it is, without index or final header: for a caller that is about to remove it."""
        fh, self._fh = self._fh, None
        if fh is not None:
            fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def save_avi(frames, path, fps, audio=None, audio_rate=None, quality=90, subsampling='4:2:0'):
    """uint8 [n, H, W, 3] frames on the device -> the file ``path``; ``audio`` int16 [samples] or [samples, channels] at ``audio_rate``
    becomes its PCM track, cut or padded with silence to the video's length.  Returns the number of bytes written.  All or nothing:
    when the encoder cannot be created or the clip passes the RIFF limit, the error is raised and no file is left at ``path``."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
        raise ValueError(f'frames must be a uint8 tensor [n, H, W, 3] with n >= 1, got {getattr(frames, "dtype", type(frames).__name__)} '
                         f'{tuple(getattr(frames, "shape", ()))}')
    if (audio is None) != (audio_rate is None):
        raise ValueError('audio and audio_rate go together: give both or neither')
    channels = 1
    if audio is not None:
        audio = audio.cpu().numpy() if isinstance(audio, torch.Tensor) else np.asarray(audio)
        if audio.dtype != np.int16 or audio.ndim not in (1, 2):
            raise ValueError(f'audio must be int16 [samples] or [samples, channels], got {audio.dtype} {audio.shape}')
        channels = 1 if audio.ndim == 1 else audio.shape[1]
    if not frames.is_cuda:
        raise ValueError('frames must be in device (HBM) memory: there is no host encoder')
    H, W = int(frames.shape[1]), int(frames.shape[2])
    enc = JpegEncoder(W, H, quality, subsampling)
    avi = None
    try:
        enc.native()                                        # the library and the native object first: a refusal leaves no file
        avi = AviWriter(path, W, H, fps, audio_rate, channels)
        if audio is not None:
            avi.add_audio(audio)
        for files in enc.encode_groups(frames):             # encode and write by turns
            avi.add_frames(files)
        avi.close()
        return avi._end + 8 + 16 * len(avi._index)
    except BaseException:
        if avi is not None:                                 # all or nothing: no header-only or partial clip stays behind
            avi.abandon()
            os.remove(path)
        raise
    finally:
        enc.close()

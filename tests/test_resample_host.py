"""CPU: the numpy restatement of rational resampling (``resample_ref.py``) against ``scipy.signal.resample_poly`` itself, the filter
design and the phase-major table of ``motioncraft_amd.audio``, and the arguments ``mc_resample_out_len`` / ``mc_resample_poly`` and
the wav header reader refuse.

Bound, restatement against scipy: both are fp64 sums of the same products, so per output
``|ref - scipy| <= (n_terms + 2) * 2^-52 * sum |x_k h_k|`` (``resample_ref.fp64_bound``)."""
import ctypes
import struct
import wave

import numpy as np
import pytest
import torch
from scipy.signal import firwin, resample_poly

import resample_ref as R
from motioncraft_amd import audio
from motioncraft_amd import lib as L

RATIOS = ((441, 320), (320, 441), (160, 441), (1, 3), (2, 1), (640, 441), (3, 2))


def pcm16(n, seed):
    """random 16-bit-valued samples in [-1, 1), fp64"""
    return np.random.RandomState(seed).randint(-32768, 32768, n).astype(np.float64) / 32768.0


@pytest.mark.parametrize('up,down', RATIOS)
def test_restatement_against_scipy(up, down):
    taps = audio.resample_filter(up, down)
    for n in (37, 700, 701):
        x = pcm16(n, n + up)
        want = resample_poly(x, up, down)
        got = R.resample(x, up, down, taps)
        assert got.shape == want.shape == (R.out_len(n, up, down),)
        err, bound = np.abs(got - want), R.fp64_bound(x, up, down, taps)
        print(f'{up}/{down} n={n}: max |ref - scipy| = {err.max():.3e}, smallest bound {bound.min():.3e}')
        assert (err <= bound).all(), (n, err.max())


@pytest.mark.parametrize('up,down', RATIOS)
def test_filter_is_the_one_scipy_designs_for_itself(up, down):
    taps = audio.resample_filter(up, down)
    m = max(up, down)
    assert taps.dtype == np.float64 and taps.shape == (20 * m + 1,) and np.array_equal(taps, taps[::-1])
    assert np.array_equal(taps, firwin(20 * m + 1, 1.0 / m, window=('kaiser', 5.0)) * up)
    x = pcm16(500, 3)
    assert np.array_equal(resample_poly(x, up, down, window=taps / up), resample_poly(x, up, down))
    other = audio.resample_filter(up, down, window='hamming')            # the window reaches the design
    assert other.shape == taps.shape and not np.array_equal(other, taps)
    assert np.array_equal(resample_poly(x, up, down, window=other / up), resample_poly(x, up, down, window='hamming'))


@pytest.mark.parametrize('up,n_taps', ((1, 7), (3, 7), (4, 9), (7, 7), (9, 5), (160, 8821)))
def test_phase_major_table(up, n_taps):
    taps = np.arange(1.0, n_taps + 1)
    table = audio.phase_major(taps, up)
    rows = -(-n_taps // up)
    assert table.shape == (up, rows) and table.dtype == np.float64 and table.flags.c_contiguous
    assert tuple(torch.from_numpy(table).shape) == (up, rows)           # no negative stride left by the reversal, also when rows == 1
    for p in range(up):
        for i in range(rows):
            t = p + (rows - 1 - i) * up
            assert table[p, i] == (taps[t] if t < n_taps else 0.0)


def test_restatement_with_a_short_filter_and_one_sample():
    """filters shorter than ``up`` (phases without a tap), a single tap, and a clip of one sample"""
    for up, down, taps in ((5, 3, [1.0, 2.0, 3.0]), (4, 1, [2.5]), (3, 7, np.arange(1.0, 12.0)), (1, 2, [0.25, 0.5, 0.25])):
        for n in (1, 2, 9):
            x = pcm16(n, n)
            want = resample_poly(x, up, down, window=np.asarray(taps) / up)
            got = R.resample(x, up, down, taps)
            assert got.shape == want.shape and (np.abs(got - want) <= R.fp64_bound(x, up, down, taps)).all(), (up, down, n)


def test_lengths():
    lib = L.load(require_gpu=False)
    for up, down in RATIOS + ((1, 1), (7, 1), (1, 7)):
        for n in list(range(0, 50)) + [44100, 2 ** 31 - 1, 2 ** 31, 2 ** 33, 2 ** 33 + 1]:
            want = -(-n * up // down)                                    # python integers: exact
            assert lib.mc_resample_out_len(n, up, down) == want == audio.out_len(n, up, down), (n, up, down)
    assert lib.mc_resample_out_len(2 ** 33, 441, 320) == 11838003610                # 2^33 * 441 / 320 = 11838003609.6
    for n, up, down in ((-1, 1, 1), (10, 0, 1), (10, 1, 0), (10, -3, 2), (2 ** 62, 640, 1)):
        assert lib.mc_resample_out_len(n, up, down) == -1
    assert audio.rate_chain(44100) == [44100] and audio.rate_chain(44100, 16000) == [44100, 16000]
    assert audio.rate_chain(16000, 16000, 22050) == [16000, 22050, 16000] and audio.rate_chain(48000, None, 22050) == [48000, 22050]
    r = audio.Resampler(16000, 16000)
    assert r.identity and (r.up, r.down) == (1, 1)


def test_bad_arguments_are_refused_before_any_launch():
    lib = L.load(require_gpu=False)
    x, y, taps = np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros(64)
    px, py, pt = (ctypes.c_void_p(a.ctypes.data) for a in (x, y, taps))
    ok = dict(n_in=10, up=3, down=2, n_taps=7, n_out=15)
    for change, text in ((dict(up=4, n_out=20), 'share a factor'), (dict(up=6, down=4), 'share a factor'), (dict(n_taps=8), 'odd'),
                         (dict(n_taps=0), 'odd'), (dict(n_out=14), 'n_out'), (dict(n_out=16), 'n_out'), (dict(n_in=0, n_out=0), 'n_in'),
                         (dict(up=0), 'up='), (dict(down=-1), 'down='), (dict(up=1, down=40, n_out=1, n_taps=801), 'two steps')):
        a = dict(ok, **change)
        rc = lib.mc_resample_poly(px, a['n_in'], a['up'], a['down'], pt, a['n_taps'], py, a['n_out'], None)
        assert rc == 1 and 'resample' in L.last_error() and text in L.last_error(), (change, L.last_error())
    assert lib.mc_resample_poly(None, 10, 3, 2, pt, 7, py, 15, None) == 1
    assert lib.mc_resample_poly(ctypes.c_void_p(x.ctypes.data + 2), 10, 3, 2, pt, 7, py, 15, None) == 1 and 'aligned' in L.last_error()
    for channels, width, out, text in ((0, 2, py, 'channels'), (2, 0, py, 'byte samples'), (2, 5, py, 'byte samples'),
                                       (2, 2, ctypes.c_void_p(y.ctypes.data + 1), 'aligned')):
        assert lib.mc_pcm_decode(px, 4, channels, width, 1, out, None) == 1 and text in L.last_error(), (channels, width, L.last_error())
    assert lib.mc_pcm_decode(px, 0, 2, 2, 1, py, None) == 1
    for taps in (np.ones(8), np.ones(0), np.ones((3, 3)), [1.0, float('nan'), 1.0]):
        with pytest.raises(ValueError):
            audio.Resampler(44100, 16000, taps=taps)
    for rates in ((0, 16000), (16000, 0), (-1, 2)):
        with pytest.raises(ValueError):
            audio.Resampler(*rates)
    with pytest.raises(ValueError):
        audio.resample_filter(0, 3)


def test_header_reader(tmp_path):
    path = str(tmp_path / 'a.wav')
    with wave.open(path, 'wb') as f:
        f.setnchannels(3), f.setsampwidth(3), f.setframerate(48000)
        f.writeframes(bytes(9 * 5))
    assert audio.wav_header(path) == (48000, 3, 3, 5)
    floats = str(tmp_path / 'float.wav')                                 # WAVE_FORMAT_IEEE_FLOAT: not integer PCM
    data = np.zeros(8, '<f4').tobytes()
    with open(floats, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(data)) + b'WAVEfmt ' + struct.pack('<IHHIIHH', 16, 3, 1, 16000, 64000, 4, 32)
                + b'data' + struct.pack('<I', len(data)) + data)
    noise = str(tmp_path / 'noise.wav')
    with open(noise, 'wb') as f:
        f.write(b'not a wav file at all')
    for bad in (floats, noise):
        with pytest.raises(ValueError):
            audio.wav_header(bad)
        with pytest.raises(ValueError):
            audio.load_wav(bad, sr=16000)


def test_library_exports_the_entries():
    lib = L.load(require_gpu=False)
    for name in ('mc_pcm_decode', 'mc_resample_out_len', 'mc_resample_poly'):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert audio.RESAMPLE_TILE == 512

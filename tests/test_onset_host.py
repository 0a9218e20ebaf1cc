"""Without a GPU: the float64 restatement of librosa 0.10.1's onset detection (``onset_ref.py``) against itself -- the peak
pick as truncated windows and as librosa's running filters -- the mel filter bank's structure, the library's new symbols, and
every argument check of ``OnsetDetector`` / ``BeatAlignment.load_audio`` / ``S2GScorer.add_sequence``, which raise before any
device call.

The short arrays of the peak-pick comparison hold multiples of 1/8 and use dyadic deltas, so every window sum is exact in both
forms and a tie is a tie in both.
"""
import itertools

import numpy as np
import pytest
import torch

import onset_ref as R
from motioncraft_amd import lib as L
from motioncraft_amd import scoring as S

NEW_SYMBOLS = ('mc_onset_work_bytes', 'mc_onset_strength', 'mc_onset_pick')
RATES = (16000, 22050)
N20 = {sr: 20 * sr + 137 for sr in RATES}


@pytest.fixture(scope='module')
def envelopes():
    return {sr: R.onset_strength(R.base_signal(sr, N20[sr], seed=sr), sr) for sr in RATES}


def test_pick_sizes_at_both_rates():
    assert R.pick_sizes(16000) == (0, 1, 3, 4, 0) and R.pick_sizes(22050) == (1, 1, 4, 5, 1)
    for sr in RATES:
        d = S.OnsetDetector(sr=sr)
        assert (d.pre_max, d.post_max, d.pre_avg, d.post_avg, d.wait) == R.pick_sizes(sr) and d.DELTA == R.DELTA


@pytest.mark.parametrize('sr', RATES)
def test_window_and_filter_forms_pick_the_same_frames_on_the_seeded_signal(envelopes, sr):
    env = envelopes[sr]
    assert env.shape == (R.num_frames(N20[sr]),) and (env[:3] == 0).all() and (env >= 0).all()
    a, b = R.onset_frames(env, sr), R.onset_frames(env, sr, pick=R.peak_pick_filters)
    x = R.normalise(env)
    mx, av = R.pick_terms(x, *R.pick_sizes(sr)[:4])
    near = np.abs(x - av - R.DELTA) < 1e-3
    print(f'sr {sr}: {env.size} frames, {a.size} onsets, {100 * near.mean():.2f} % of frames within 1e-3 of the threshold')
    assert a.size >= 40 and np.array_equal(a, b)
    assert x.min() == 0 and abs(x.max() - 1) < 1e-15
    assert np.array_equal(R.onset_detect(R.base_signal(sr, N20[sr], seed=sr), sr), a * 512 / sr)


def short_arrays():
    rs = np.random.RandomState(7)
    for n in range(1, 13):
        yield np.full(n, 0.5)                                          # all equal
        yield np.zeros(n)
        yield np.arange(n) / 8.0
        yield np.arange(n)[::-1] / 8.0
        yield (np.arange(n) % 2) * 1.0                                 # ties between every other frame
        for _ in range(6):
            yield rs.randint(0, 4, n) / 8.0                            # few levels: many ties


def test_window_and_filter_forms_agree_on_short_arrays_with_ties():
    sizes = [R.pick_sizes(16000), R.pick_sizes(22050), (2, 1, 1, 2, 3), (3, 3, 0, 1, 2), (1, 2, 5, 1, 0)]
    picked = compared = 0
    for x, (pre_max, post_max, pre_avg, post_avg, wait), delta in itertools.product(short_arrays(), sizes, (0.0, 0.0625, 0.25)):
        a = R.peak_pick_windows(x, pre_max, post_max, pre_avg, post_avg, delta, wait)
        b = R.peak_pick_filters(x, pre_max, post_max, pre_avg, post_avg, delta, wait)
        assert np.array_equal(a, b), (x, pre_max, post_max, pre_avg, post_avg, delta, wait, a, b)
        picked += a.size
        compared += 1
    assert compared > 1000 and picked > 1000
    # an all-equal array: every frame equals its window maximum and its window mean, so delta decides; wait thins the rest
    assert R.peak_pick_windows(np.full(6, 0.5), 1, 1, 4, 5, 0.0, 1).tolist() == [0, 2, 4]
    assert R.peak_pick_windows(np.full(6, 0.5), 1, 1, 4, 5, 0.0625, 1).size == 0
    assert R.onset_frames(np.zeros(9), 16000).size == 0 and R.onset_frames(np.full(9, 2.0), 16000).size == 0


@pytest.mark.parametrize('sr', RATES)
def test_mel_basis_structure(sr):
    pts = R.mel_points(sr)
    freqs = np.arange(1025) * (sr / 2048)
    assert pts.shape == (130,) and pts[0] == 0 and abs(pts[-1] - sr / 2) < 1e-9 and (np.diff(pts) > 0).all()
    for W in (R.mel_basis(sr), S.mel_filter_bank(sr, 2048, 128)):
        assert W.shape == (128, 1025) and W.dtype == np.float32 and (W >= 0).all()
        for i in range(128):
            nz = np.flatnonzero(W[i])
            assert nz.size > 0, f'row {i} is empty'
            assert freqs[nz[0]] > pts[i] and freqs[nz[-1]] < pts[i + 2]
            assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))
    assert np.array_equal(R.mel_basis(sr), S.mel_filter_bank(sr, 2048, 128))
    # Slaney normalisation: a row's weights integrate to about 1 over frequency (exactly, for a finely sampled triangle)
    area = R.mel_basis(sr)[-1].astype(np.float64).sum() * (sr / 2048)
    assert abs(area - 1) < 0.05


def test_dft_table_is_the_windowed_transform():
    T = S.dft_table(2048)
    assert T.shape == (2048, 2050) and T.dtype == np.float32
    y = np.random.RandomState(3).standard_normal(2048)
    spec = np.fft.rfft(y * R.hann())
    got = y @ T.astype(np.float64)
    assert np.abs(got[0::2] - spec.real).max() < 1e-4 and np.abs(got[1::2] - spec.imag).max() < 1e-4
    assert (T[:, 1] == 0).all() and np.abs(T[:, 2049]).max() < 1e-15     # the imaginary parts of bins 0 and 1024


def test_library_exports_the_onset_symbols_and_sizes_the_workspace():
    lib = L.load(require_gpu=False)
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    import motioncraft_amd
    assert 'OnsetDetector' in motioncraft_amd.__all__ and motioncraft_amd.OnsetDetector is S.OnsetDetector
    wb = lib.mc_onset_work_bytes
    assert wb(16000, 2048, 512, 128) > 4 * (1025 + 128) * 32 and wb(16000, 2048, 512, 128) % 16 == 0
    assert wb(1, 2048, 512, 128) > 0
    for bad in ((0, 2048, 512, 128), (-5, 2048, 512, 128), (16000, 0, 512, 128), (16000, -2048, 512, 128), (16000, 1024, 512, 128),
                (16000, 2048, 0, 128), (16000, 2048, -512, 128), (16000, 2048, 510, 128), (16000, 2048, 1024, 128), (16000, 2048, 512, 0),
                (16000, 2048, 512, -1), (16000, 2048, 512, 129), (1 << 40, 2048, 512, 128)):
        assert wb(*bad) == -1, bad


def test_argument_checks_raise_before_any_device_call(monkeypatch):
    monkeypatch.setattr(L, 'load', lambda *a, **k: pytest.fail('an argument error reached the library'))
    for kw, msg in ((dict(sr=0), 'sr=0'), (dict(sr=-1.0), 'sr=-1.0'), (dict(hop_length=0), 'hop_length=0'), (dict(hop_length=-512), 'hop_length=-512'),
                    (dict(hop_length=1024), 'hop_length=1024'), (dict(hop_length=510), 'hop_length=510'), (dict(n_fft=1024), 'n_fft=1024'),
                    (dict(n_fft=0), 'n_fft=0'), (dict(n_mels=0), 'n_mels=0'), (dict(n_mels=-3), 'n_mels=-3'), (dict(n_mels=129), 'n_mels=129')):
        with pytest.raises(ValueError, match=msg):
            S.OnsetDetector(**kw)
    det = S.OnsetDetector()
    assert (det.sr, det.hop_length, det.n_fft, det.n_mels) == (16000.0, 512, 2048, 128) and det.num_frames(511) == 1 and det.num_frames(512) == 2
    good = np.zeros(4000, np.float32)
    for call in (det.strength, det.detect):
        with pytest.raises(ValueError, match='must be 1-D'):
            call(np.zeros((2, 4000), np.float32))
        with pytest.raises(ValueError, match='must be 1-D'):
            call(np.float32(0.5))
        with pytest.raises(ValueError, match='holds no sample'):
            call(np.zeros(0, np.float32))
        with pytest.raises(ValueError, match='floating point'):
            call(np.zeros(4000, np.int16))
        for bad in (np.nan, np.inf, -np.inf):
            y = good.copy()
            y[1234] = bad
            with pytest.raises(ValueError, match='not finite'):
                call(y)
    with pytest.raises(ValueError, match='units='):
        det.detect(good, units='samples')
    for bad in (np.zeros(8, np.float32), torch.zeros(8), torch.zeros(8, dtype=torch.float64), [0.0, 1.0]):
        with pytest.raises(ValueError, match='float32 device tensor'):
            det.pick(bad)
    al = S.BeatAlignment(0.3, 7, np.ones(55, np.float32))
    with pytest.raises(ValueError, match='must be 1-D'):
        al.load_audio(np.zeros((2, 4000), np.float32))
    with pytest.raises(ValueError, match='holds no sample'):
        al.load_audio(good, 3000, 2000)
    with pytest.raises(ValueError, match='not finite'):
        al.load_audio(np.full(4000, np.nan, np.float32), 100, 3000)
    with pytest.raises(ValueError, match='sr=0'):
        al.load_audio(good, sr_audio=0)


def test_add_sequence_takes_exactly_one_of_onset_times_and_audio(monkeypatch):
    monkeypatch.setattr(L, 'load', lambda *a, **k: pytest.fail('an argument error reached the library'))
    sc = S.S2GScorer(None, None, np.ones(55, np.float32), align_mask=60)
    T = 150
    seq = (torch.zeros(T, 322), torch.zeros(T, 165), torch.zeros(T, 100), torch.zeros(T, 3), torch.zeros(300))
    audio = np.zeros(16000 * 5, np.float32)
    with pytest.raises(ValueError, match='exactly one of onset_times and audio'):
        sc.add_sequence(*seq)
    with pytest.raises(ValueError, match='exactly one of onset_times and audio'):
        sc.add_sequence(*seq, onset_times=[0.1], audio=audio)
    with pytest.raises(ValueError, match='exactly one of onset_times and audio'):
        sc.add_sequence(*seq, [0.1], audio)
    with pytest.raises(ValueError, match='must be 1-D'):
        sc.add_sequence(*seq, audio=audio.reshape(2, -1))
    with pytest.raises(ValueError, match='not finite'):
        sc.add_sequence(*seq, audio=np.full(100, np.inf, np.float32))
    with pytest.raises(ValueError, match='audio_sr=0'):
        sc.add_sequence(*seq, audio=audio, audio_sr=0)
    with pytest.raises(ValueError, match='no onset times'):
        sc.add_sequence(*seq, onset_times=[])
    with pytest.raises(ValueError, match='leave nothing between the two masks'):
        sc.add_sequence(torch.zeros(120, 322), torch.zeros(120, 165), torch.zeros(120, 100), torch.zeros(120, 3), torch.zeros(300), audio=audio)
    assert sc.num_sequences == 0

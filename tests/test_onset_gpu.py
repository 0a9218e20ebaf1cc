"""On the MI355X: audio onset detection (``mc_onset_strength`` / ``mc_onset_pick``, ``scoring.OnsetDetector``) against the
float64 restatement of librosa 0.10.1's ``onset_detect`` in ``onset_ref.py``.

Bounds.
  * envelope, compared after min/max normalisation: within ``8 x band``, where ``band`` is measured in the test on the same
    input: the largest normalised-envelope difference between the float64 restatement and its float32 CPU evaluation
    (``onset_ref.onset_strength_fp32``: ``torch.stft`` float32, float32 mel projection, dB and flux).  The device sums the
    2048 products of a DFT bin directly, which rounds like sqrt(K) where an FFT rounds like log K: about 4x, doubled.
  * onset frames: EQUAL to the restatement's except at frames whose decision lies inside the noise.  A frame is uncertain only
    if the restatement's |env[n] - mean - delta| <= ``16 x band`` (or, where pre_max > 0, its margin over a neighbour in the max
    window is that small); at most 1 % of the frames may be, and the restatement must find at least 40 onsets.  Because of the
    ``wait`` rule a flipped frame moves later decisions, so the device mask must equal the greedy pass over the certain
    candidates plus exactly those uncertain frames the device reported.
  * repeated runs, another stream: bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

import onset_ref as R
from motioncraft_amd import scoring as S
from test_scoring_gpu import evaluator, s2g_sequence, small           # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FT = 32                                      # frames per workgroup of onset_melpow_k (csrc/mc_onset.hip)
ENV_FACTOR, EDGE_FACTOR, MAX_UNCERTAIN = 8, 16, 0.01


@functools.lru_cache(maxsize=None)
def detector(sr, hop=512, n_mels=128):
    return S.OnsetDetector(sr=sr, hop_length=hop, n_mels=n_mels)


@functools.lru_cache(maxsize=None)
def signal(kind, sr, n):
    if kind == 'base':
        y = R.base_signal(sr, n, seed=sr + n)
    elif kind == 'silence_then_base':
        y = np.concatenate([np.zeros(2 * sr, np.float32), R.base_signal(sr, n - 2 * sr, seed=sr + n)])
    elif kind == 'last_click_in_noise':                                # noise some 80 dB below the click, which alone sets the clamp floor
        y = (4e-6 * np.random.RandomState(n).standard_normal(n)).astype(np.float32)
        y[-1] = 1.0
    elif kind in ('clicks', 'clicks_in_noise'):
        y = (1e-3 * np.random.RandomState(n).standard_normal(n)).astype(np.float32) if kind == 'clicks_in_noise' else np.zeros(n, np.float32)
        y[0] = y[-1] = 1.0
    return y


@functools.lru_cache(maxsize=None)
def reference(kind, sr, n, hop=512, n_mels=128):
    """(float64 envelope, band) of one input, computed once"""
    y = signal(kind, sr, n)
    env = R.onset_strength(y, sr, hop=hop, n_mels=n_mels)
    env32 = R.onset_strength_fp32(y, sr, hop=hop, n_mels=n_mels)
    assert env32.dtype == np.float32 and env.shape == env32.shape == (R.num_frames(n, hop),)
    env.setflags(write=False)
    return env, float(np.abs(R.normalise(env32) - R.normalise(env)).max())


def check_envelope(kind, sr, n, hop=512, n_mels=128):
    want, band = reference(kind, sr, n, hop, n_mels)
    got = detector(sr, hop, n_mels).strength(signal(kind, sr, n))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    diff = float(np.abs(R.normalise(got) - R.normalise(want)).max())
    print(f'{kind} sr {sr} N {n} hop {hop}: {want.size} frames, band {band:.2e}, device {diff:.2e} = {diff / band if band else 0:.2f} x band')
    assert np.isfinite(got).all() and (got >= 0).all() and (got[:1 + 1024 // hop] == 0).all()
    assert diff <= ENV_FACTOR * band
    return got


def check_frames(kind, sr, n, min_onsets=40):
    want_env, band = reference(kind, sr, n)
    pre_max, post_max, pre_avg, post_avg, wait = R.pick_sizes(sr)
    x = R.normalise(want_env)
    F = x.size
    _, av = R.pick_terms(x, pre_max, post_max, pre_avg, post_avg)
    eps = EDGE_FACTOR * band
    gap = np.full(F, np.inf)                                           # margin of x[n] over the other frames of its max window
    for i in range(F):
        others = [x[k] for k in range(max(0, i - pre_max), min(F, i + post_max)) if k != i]
        if others:
            gap[i] = x[i] - max(others)
    margin = x - av - R.DELTA
    sure = (gap > eps) & (margin > eps) & (x > eps)
    no = (gap < -eps) | (margin < -eps) | (x <= 0)
    unsure = ~sure & ~no
    want = R.onset_frames(want_env, sr)
    det = detector(sr)
    y = signal(kind, sr, n)
    got = det.detect(y, units='frames')
    times = det.detect(y)
    print(f'{kind} sr {sr}: {F} frames, {want.size} onsets in the restatement, {got.size} on the device, {int(unsure.sum())} uncertain frames '
          f'({100 * unsure.mean():.2f} %), band {band:.2e}')
    assert want.size >= min_onsets and unsure.mean() <= MAX_UNCERTAIN
    assert got.dtype == np.int64 and times.dtype == np.float64 and np.array_equal(times, got * 512 / sr)
    dev = np.zeros(F, bool)
    dev[got] = True
    assert np.array_equal(got, R.greedy_wait(sure | (unsure & dev), wait))
    if not unsure.any():
        assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize('sr', (16000, 22050))
def test_envelope_and_onsets_of_the_20_s_signal(sr):
    n = 20 * sr + 137
    check_envelope('base', sr, n)
    check_frames('base', sr, n)


@pytest.mark.parametrize('frames', (FT - 1, FT, FT + 1))
def test_envelope_around_the_row_tile(frames):
    n = (frames - 1) * 512 + (0, 17, 511)[frames % 3]
    assert R.num_frames(n) == frames
    check_envelope('base', 16000, n)


@pytest.mark.parametrize('n,frames', ((511, 1), (512, 2), (1535, 3), (2048, 5)))
def test_envelope_of_the_shortest_clips(n, frames):
    assert R.num_frames(n) == frames
    got = check_envelope('base', 16000, n)
    if frames <= 3:
        assert not got.any() and detector(16000).detect(signal('base', 16000, n)).size == 0


def test_envelope_at_another_hop_and_mel_count():
    check_envelope('base', 16000, 3 * 16000 + 41, hop=256, n_mels=40)


def test_silence_has_no_onsets():
    det = detector(16000)
    y = np.zeros(3 * 16000 + 5, np.float32)
    assert not det.strength(y).cpu().numpy().any()
    assert det.detect(y).size == 0 and det.detect(y, units='frames').dtype == np.int64


@pytest.mark.parametrize('sr', (16000, 22050))
def test_silence_then_signal_runs_the_80_db_clamp(sr):
    n = 22 * sr + 137
    want, _ = reference('silence_then_base', sr, n)
    assert not want[:2 * sr // 512 - 2].any() and want[2 * sr // 512 + 4:].any()       # -100 dB everywhere before the signal: clamped, no flux
    check_envelope('silence_then_base', sr, n)
    got = check_frames('silence_then_base', sr, n)
    assert got.min() >= 2 * sr // 512 - 2


def test_clicks_at_the_first_and_last_sample_see_the_zero_padding():
    """The frames around both clicks reach past the clip.  Alone, the clicks leave the envelope at zero: the power only falls
    after frame 0, and the envelope's lag of 3 frames ends before the last click's frames -- so anything the device made of
    the padding would show as a non-zero value.  Over a noise floor the clicks set the spectrogram's maximum."""
    n = 16000 + 77
    want, band = reference('clicks', 16000, n)
    assert not want.any() and band == 0
    assert not check_envelope('clicks', 16000, n).any() and detector(16000).detect(signal('clicks', 16000, n)).size == 0
    want, _ = reference('clicks_in_noise', 16000, n)
    assert want.any()
    check_envelope('clicks_in_noise', 16000, n)


def test_a_last_sample_click_sets_the_clamp_floor():
    """Only the last two frames reach past the end of the clip, and the envelope's lag keeps their flux out of it: the right-hand
    padding shows through the spectrogram's maximum alone.  Here the click at the last sample is that maximum and the noise lies
    around 80 dB below it, so the floor max - 80 cuts through the noise and a wrong last frame would move the whole envelope."""
    n = 16000 + 77
    y = signal('last_click_in_noise', 16000, n)
    want, _ = reference('last_click_in_noise', 16000, n)
    quiet = y.copy()
    quiet[-1] = 0
    assert want.any() and np.abs(R.normalise(R.onset_strength(quiet, 16000)) - R.normalise(want)).max() > 1e-2      # the click matters
    check_envelope('last_click_in_noise', 16000, n)


def test_two_runs_and_another_stream_give_the_same_bits():
    det = detector(22050)
    y = torch.from_numpy(signal('base', 22050, 20 * 22050 + 137).copy()).cuda()
    env = det.strength(y)
    mask, count = det.pick(env)
    env2 = det.strength(y)
    mask2, count2 = det.pick(env2)
    assert torch.equal(env, env2) and torch.equal(mask, mask2) and torch.equal(count, count2)
    assert int(count) == int(mask.sum()) > 0 and mask.dtype == torch.uint8 and int(mask.max()) == 1
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env3 = det.strength(y)
        mask3, count3 = det.pick(env3)
    side.synchronize()
    assert torch.equal(env, env3) and torch.equal(mask, mask3) and torch.equal(count, count3)


def test_load_audio_slices_then_detects():
    al = S.BeatAlignment(0.3, 7, np.ones(55, np.float32))
    for sr in (16000, 22050):
        y = signal('base', sr, 20 * sr + 137)
        a, b = 3 * sr + 11, 15 * sr + 5
        got = al.load_audio(y, a, b, sr_audio=sr)
        assert got.dtype == np.float64 and got.size > 10 and np.array_equal(got, detector(sr).detect(y[a:b]))
        assert got.max() < (b - a) / sr                                # relative to the slice
        assert np.array_equal(al.load_audio(y, sr_audio=sr), detector(sr).detect(y))
        assert np.array_equal(al.load_audio(torch.from_numpy(y.copy()).cuda(), a, b, sr_audio=sr), got)


def scorer_state(sc):
    return (sc.align, sc.l2_all, sc.lvel, sc.total_length, sc.num_sequences, sc.l1_calculator.avg(),
            {k: [e.tobytes() for e in v] for k, v in sc.emb.items()})


@pytest.mark.parametrize('extra', (0, 10000))
def test_s2g_scorer_from_audio_equals_the_scorer_from_its_onsets(small, evaluator, extra):
    """``extra`` samples of audio beyond the motion: s2g_test.py:419 measures the right-hand cut from the UNCUT length."""
    _, body = small
    mean_vel = np.full(55, 0.5, np.float32)
    T, sr = 150, 16000
    q = s2g_sequence(T, 90)
    del q['onset_times']
    audio = R.base_signal(sr, int(sr / 30 * T) + extra, seed=5)
    a = int(60 * (sr / 30))
    cut = audio[:int(sr / 30 * T)]
    onsets = S.BeatAlignment(0.3, 7, mean_vel).load_audio(cut, a, len(audio) - a)
    assert onsets.size >= 3 and np.array_equal(onsets, detector(sr).detect(cut[a:len(audio) - a]))
    from_audio, from_onsets = (S.S2GScorer(body, evaluator, mean_vel, align_mask=60) for _ in range(2))
    per_a = from_audio.add_sequence(**q, audio=audio)
    per_o = from_onsets.add_sequence(**q, onset_times=onsets)
    assert per_a == per_o and scorer_state(from_audio) == scorer_state(from_onsets)
    assert 0 < per_a['align'] <= 1 and from_audio.num_sequences == 1 and from_audio.total_length == T

"""CPU: the numpy restatement of the S2G audio condition (``audio_cond_ref.py``) against a brute-force loop, the frame count and
prompt of ``motioncraft_amd.speech``, and the window walk of ``longform`` over a condition with several rows per frame against the
index expression of the S2G test loop (``tools/s2g_test.py:144-155``)."""
import ctypes

import numpy as np
import pytest
import torch

import audio_cond_ref as R
from motioncraft_amd import lib as L
from motioncraft_amd import longform, speech

WALKS = ((200, 64, 4, 533), (29, 8, 2, 3), (16, 8, 7, 1))               # (frames, window, shared frames, rows per frame)


@pytest.mark.parametrize('window', (1, 2, 3, 7))
def test_restated_envelope_equals_the_double_loop(window):
    rs = np.random.RandomState(window)
    for n in range(window, 3 * window + 2):
        y = rs.standard_normal(n).astype(np.float32)
        got = R.envelope(y, window)
        assert got.dtype == np.float32 and got.shape == (n,)
        assert np.array_equal(got, R.envelope_loops(y, window)), (n, window)


def test_tail_repeats_the_last_full_window_and_does_not_shrink():
    n, window = 40, 7
    y = (0.1 * np.random.RandomState(0).standard_normal(n)).astype(np.float32)
    y[n - window - 1] = 5.0                                              # the largest sample: in the second-to-last full window, in no later one
    y[n - window] = -2.0                                                 # the largest magnitude of the last full window, at its first sample
    got = R.envelope(y, window)
    assert np.array_equal(got, R.envelope_loops(y, window))
    assert got[n - window - 1] == 5.0 and (got[n - window:] == 2.0).all()
    shrinking = R.envelope_shrinking(y, window)                          # a window cut at the end of the clip loses that sample
    assert np.array_equal(shrinking[:n - window + 1], got[:n - window + 1]) and (shrinking[n - window + 1:] < 1.0).all()


def test_condition_puts_onset_frames_at_sample_indices():
    y = np.random.RandomState(1).standard_normal(3000).astype(np.float32)
    c = R.condition(y, [0, 3, 5], window=16)
    assert c.dtype == np.float32 and c.shape == (3000, 2)
    assert np.array_equal(np.flatnonzero(c[:, 1]), [0, 3, 5]) and np.array_equal(c[:, 0], R.envelope(y, 16))


def test_frame_count_and_prompt():
    assert speech.SAMPLES_PER_FRAME == 533 == R.SAMPLES_PER_FRAME
    assert speech.speech_frames(533 * 64) == 64                          # remainder 0
    assert speech.speech_frames(533 * 71) == 64 and speech.speech_frames(533 * 71 + 532) == 64       # remainder 7
    assert speech.speech_frames(533 * 72 - 1) == 64 and speech.speech_frames(533 * 72) == 72
    assert speech.speech_frames(532) == 0 and speech.speech_frames(100, samples_per_frame=10, multiple=4) == 8
    head = 'A person is doing a speech, and the speech content is '
    assert speech.speech_prompt(['so', 'we', '', 'so', 'go', 'we', '']) == head + 'so we go'
    assert speech.speech_prompt([]) == head and speech.speech_prompt(['', '']) == head
    assert speech.speech_prompt(('b', 'a', 'b')) == head + 'b a'


class Recorder:
    """a ``model`` that keeps the ``c`` of every call and returns zeros"""

    def __init__(self):
        self.c = []

    def __call__(self, **kw):
        self.c.append(kw['c'].clone())
        return [dict(pred_motion=torch.zeros(kw['motion'].shape[1:])) for _ in range(kw['motion'].shape[0])]


def rows(n_rows, seed=0):
    """[n_rows, 2]: column 0 counts the rows, so a slice names the rows it was cut from"""
    c = torch.randn(n_rows, 2, generator=torch.Generator().manual_seed(seed))
    c[:, 0] = torch.arange(n_rows)
    return c


@pytest.mark.parametrize('n,L,pre,r', WALKS)
def test_sample_long_cuts_the_rows_of_the_reference_loop(n, L, pre, r):
    c = rows(n * r + 5)
    model = Recorder()
    rec, wins = longform.sample_long(model, n, L, pre, c=c, c_rows_per_frame=r, device='cpu', input_dim=4)
    want = R.window_rows(n, L, pre, r)
    assert len(model.c) == len(wins) == len(want) >= 2
    for got, (lo, hi) in zip(model.c, want):
        assert hi - lo == L * r and tuple(got.shape) == (1, L * r, 2)
        assert torch.equal(got[0], c[lo:hi])
    if r == 1:                                                           # today's slices: window i starts at frame i * stride
        plain = Recorder()
        longform.sample_long(plain, n, L, pre, c=c, device='cpu', input_dim=4)
        assert all(torch.equal(a, b) for a, b in zip(plain.c, model.c))
        assert all(torch.equal(g[0], c[i * (L - pre):i * (L - pre) + L]) for i, g in enumerate(plain.c))


@pytest.mark.parametrize('n,L,pre,r', WALKS)
def test_sample_long_batched_cuts_the_same_rows_for_two_lengths(n, L, pre, r):
    totals = [n, n + 2 * (L - pre) + 1]
    cs = [rows(t * r, seed=s) for s, t in enumerate(totals)]
    model = Recorder()
    recs, wins = longform.sample_long_batched(model, totals, L, pre, c=cs, text=['a', 'b'], c_rows_per_frame=r, device='cpu', input_dim=4,
                                              shard=False, max_batch=3)
    got = torch.cat(model.c)
    want = [(s, lo, hi) for s, t in enumerate(totals) for lo, hi in R.window_rows(t, L, pre, r)]
    assert len(want) == got.shape[0] == len(wins) and len(R.window_rows(totals[1], L, pre, r)) >= len(R.window_rows(n, L, pre, r)) + 2
    for g, (s, lo, hi) in zip(got, want):
        assert torch.equal(g, cs[s][lo:hi])
    if r == 1:
        plain = Recorder()
        longform.sample_long_batched(plain, totals, L, pre, c=cs, text=['a', 'b'], device='cpu', input_dim=4, shard=False, max_batch=3)
        assert torch.equal(torch.cat(plain.c), got)


def test_drivers_reject_a_short_condition_and_a_bad_row_count():
    with pytest.raises(ValueError, match='rows'):
        longform.sample_long(Recorder(), 16, 8, 2, c=rows(16 * 3 - 1), c_rows_per_frame=3, device='cpu', input_dim=4)
    with pytest.raises(ValueError, match='rows'):
        longform.sample_long_batched(Recorder(), [16, 16], 8, 2, c=[rows(48), rows(47)], c_rows_per_frame=3, device='cpu', input_dim=4, shard=False)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='c_rows_per_frame'):
            longform.sample_long(Recorder(), 16, 8, 2, c=rows(64), c_rows_per_frame=bad, device='cpu', input_dim=4)


def test_sample_speech_hands_the_condition_to_the_driver(monkeypatch):
    """with a stand-in condition: the frame count, the prompt and the rows per frame reach ``sample_long`` / ``sample_long_batched``"""
    seen = {}

    def driver(name):
        def run(model, total, L, pre, **kw):
            seen[name] = dict(total=total, L=L, pre=pre, **kw)
            return name
        return run
    monkeypatch.setattr(longform, 'sample_long', driver('one'))
    monkeypatch.setattr(longform, 'sample_long_batched', driver('batched'))
    cond = rows(533 * 21 + 9)
    kw = dict(words=['hi', '', 'hi', 'all'], motion_length=8, pre_frames=2, condition=lambda y: cond, repaint=True, mean=1.0)
    assert speech.sample_speech('m', None, **kw) == 'one' and speech.sample_speech('m', None, batched=True, **kw) == 'batched'
    one, many = seen['one'], seen['batched']
    assert one['total'] == 16 and many['total'] == [16] and one['c'] is cond and many['c'][0] is cond
    assert one['text'] == many['text'][0] == 'A person is doing a speech, and the speech content is hi all'
    for d in (one, many):
        assert (d['L'], d['pre'], d['c_rows_per_frame'], d['repaint'], d['mean']) == (8, 2, 533, True, 1.0)


def test_library_exports_the_symbol_with_its_signature():
    lib = L.load(require_gpu=False)
    assert 'mc_audio_condition' in L.EXPORTED_SYMBOLS and hasattr(lib, 'mc_audio_condition')
    fn = lib.mc_audio_condition
    vp = ctypes.c_void_p
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [vp, ctypes.c_int64, ctypes.c_int32, vp, ctypes.c_int32, vp, vp]
    import motioncraft_amd
    for name in ('AudioCondition', 'sample_speech', 'speech_frames', 'speech_prompt', 'speech'):
        assert name in motioncraft_amd.__all__ and hasattr(motioncraft_amd, name)
    assert speech.AUDIO_COND_TILE == 4096 and speech.MAX_WINDOW == 1024


def test_bad_arguments_return_before_any_launch():
    """the argument checks of the C entry point run on the host: no device is needed to see them refuse"""
    lib = L.load(require_gpu=False)
    fake = ctypes.c_void_p(4096)                                         # never dereferenced: every case below fails a check first
    for n, window, frames in ((0, 1, 0), (-3, 1, 0), (1023, 1024, 0), (4096, 0, 0), (4096, 1025, 0), (4096, -1, 0), (16, 8, 17), (16, 8, -1)):
        assert lib.mc_audio_condition(fake, n, window, fake, frames, fake, None) == 1, (n, window, frames)      # MC_ERR_ARG
        assert 'audio condition' in L.last_error()
    assert lib.mc_audio_condition(None, 16, 8, None, 0, fake, None) == 1 and lib.mc_audio_condition(fake, 16, 8, None, 0, None, None) == 1


def test_argument_checks_raise_before_any_device_call(monkeypatch):
    monkeypatch.setattr(L, 'load', lambda *a, **k: pytest.fail('an argument error reached the library'))
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match='frame_length'):
            speech.AudioCondition(frame_length=bad)
    ac = speech.AudioCondition()
    for y, msg in ((np.zeros(1023, np.float32), 'no full window'), (np.zeros((2, 2048), np.float32), '1-D'),
                   (np.full(2048, np.nan, np.float32), 'finite'), (np.array([np.inf] + [0.0] * 2047, np.float32), 'finite'),
                   (np.zeros(2048, np.int16), 'floating'), (np.zeros(0, np.float32), 'no sample')):
        with pytest.raises(ValueError, match=msg):
            ac(y)
        with pytest.raises(ValueError, match=msg):
            ac.amplitude_envelope(y)
    with pytest.raises(ValueError, match='window=2000'):
        ac.amplitude_envelope(np.zeros(4096, np.float32), window=2000)
    with pytest.raises(ValueError, match='no full window'):
        ac.amplitude_envelope(np.zeros(5, np.float32), window=6)

"""On the MI355X: the S2G audio condition (``mc_audio_condition``, ``speech.AudioCondition``) against the numpy restatement
``audio_cond_ref.py``, the window walk over it, and ``tools/s2g_sample.py``.

Bounds.
  * envelope and onset column: EQUAL to the restatement, compared as bits.  A maximum of float32 magnitudes has no rounding, so
    any difference is a wrong window, not arithmetic.
  * repeated runs, another stream: bit for bit.
  * ``sample_long`` over the device condition: bit-equal to direct model calls on the slices the S2G test loop would cut, with
    the same noise -- the driver adds nothing but the slicing.
"""
import ctypes
import functools
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import audio_cond_ref as R
from motioncraft_amd import lib as L
from motioncraft_amd import longform, scoring, speech

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = speech.AUDIO_COND_TILE
S2G_CONFIG = os.path.join(HERE, 'configs', 'stmogen_s2g_small.py')
S2G_SEED, S2G_WINDOW, S2G_PRE, S2G_ROWS = 2, 16, 4, 523                 # the small S2G model: 16-frame windows of 523 audio rows per frame


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def raw_condition(y, window, mask=None):
    """``mc_audio_condition`` itself: y float32 (numpy or device tensor), mask uint8 device tensor or None -> device [N, 2]"""
    lib = L.load(require_gpu=True)
    t = (y if torch.is_tensor(y) else torch.from_numpy(np.array(y, dtype=np.float32))).cuda()
    assert t.dtype == torch.float32 and t.is_contiguous()
    out = torch.full((t.numel(), 2), float('nan'), device='cuda')
    L.check(lib.mc_audio_condition(ctypes.c_void_p(t.data_ptr()), t.numel(), window, None if mask is None else ctypes.c_void_p(mask.data_ptr()),
                                   0 if mask is None else mask.numel(), ctypes.c_void_p(out.data_ptr()),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mc_audio_condition')
    return out


@functools.lru_cache(maxsize=None)
def noise(n):
    y = np.random.RandomState(n).standard_normal(n).astype(np.float32)
    y.setflags(write=False)
    return y


def check_envelope(y, window):
    want = R.envelope(y, window)
    out = raw_condition(y, window).cpu().numpy()
    got = out[:, 0]
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (y.size, window, bad[:8], got[bad[:8]], want[bad[:8]])
    assert not out[:, 1].any() and not np.signbit(out[:, 1]).any()       # no mask: a column of +0
    return got


@pytest.mark.parametrize('n', (1024, 1025, 2047, 2048, 2049, T - 1, T, T + 1, T + 1023, T + 1024, 2 * T + 1, 3 * T + 517))
def test_envelope_at_the_tile_edges_with_the_reference_window(n):
    check_envelope(noise(n), 1024)


@pytest.mark.parametrize('window', (1, 2, 3, 63, 64, 65, 1000))
def test_envelope_at_other_windows(window):
    check_envelope(noise(T + 130), window)


@pytest.mark.parametrize('n', (1, 5, 777, 1024))
def test_one_window_gives_one_value(n):
    y = noise(n)
    got = check_envelope(y, n)
    assert (got == np.abs(y).max()).all()


def test_a_clip_that_does_not_start_on_16_bytes():
    y = torch.from_numpy(noise(2 * T + 300).copy()).cuda()
    for start in (1, 2, 3):
        cut = y[start:]
        assert cut.data_ptr() % 16 == 4 * start
        got = raw_condition(cut, 1024)[:, 0].cpu().numpy()
        assert np.array_equal(bits(got), bits(R.envelope(noise(2 * T + 300)[start:], 1024)))


SPIKE_N, SPIKE_W = 2 * T + 300, 1024
SPIKES = {'first': 0, 'last': SPIKE_N - 1, 'start_of_last_window': SPIKE_N - SPIKE_W, 'before_last_window': SPIKE_N - SPIKE_W - 1,
          'end_of_tile': T - 1, 'start_of_tile': T, 'last_of_halo': T + SPIKE_W - 2, 'first_past_halo': T + SPIKE_W - 1}


@pytest.mark.parametrize('sign', (1.0, -1.0))
@pytest.mark.parametrize('where', tuple(SPIKES))
def test_a_single_spike_is_seen_by_exactly_its_windows(where, sign):
    at = SPIKES[where]
    y = noise(SPIKE_N).copy()
    y[at] = 10.0 * sign
    got = check_envelope(y, SPIKE_W)
    lo = max(0, at - SPIKE_W + 1)
    seen = np.flatnonzero(got == 10.0)
    if at >= SPIKE_N - SPIKE_W:                                          # in the last full window: repeated to the end of the clip
        assert seen[0] == lo and seen[-1] == SPIKE_N - 1 and seen.size == SPIKE_N - lo
    else:
        assert seen[0] == lo and seen[-1] == at and seen.size == at - lo + 1


@pytest.mark.parametrize('window', (1024, 65))
def test_ramps_show_a_window_one_sample_short_or_long(window):
    n = T + 1024 + 77
    up = np.arange(1, n + 1, dtype=np.float32)
    got = check_envelope(up, window)
    assert np.array_equal(got[:n - window + 1], up[window - 1:]) and (got[n - window:] == n).all()
    down = up[::-1].copy()
    got = check_envelope(down, window)
    assert np.array_equal(got[:n - window + 1], down[:n - window + 1]) and (got[n - window:] == window).all()
    check_envelope(-up, window)


def test_negative_zeros_give_positive_zeros():
    y = np.full(T + 1024 + 5, -0.0, np.float32)
    assert np.signbit(y).all()
    out = raw_condition(y, 1024).cpu().numpy()
    assert not bits(out).any()


def test_onset_mask_marks_sample_indices():
    n, window = T + 2000, 64
    y = noise(n)
    env = R.envelope(y, window)
    n_frames = 1 + n // 512
    for frames in ([0, n_frames - 1], [0, 1, 5, n_frames - 2, n_frames - 1], [3], []):
        mask = torch.zeros(n_frames, dtype=torch.uint8)
        if frames:
            mask[frames] = 1
            mask[frames[0]] = 255                                        # any non-zero byte is set
        out = raw_condition(y, window, mask.cuda()).cpu().numpy()
        assert np.array_equal(bits(out), bits(R.condition(y, frames, window))) and np.array_equal(np.flatnonzero(out[:, 1]), frames)
        assert np.array_equal(bits(out[:, 0]), bits(env))
    full = torch.ones(n, dtype=torch.uint8).cuda()                       # a mask as long as the clip: n_frames == n_samples is allowed
    assert (raw_condition(y, window, full)[:, 1] == 1).all()


@functools.lru_cache(maxsize=None)
def click_train(seconds=4, sr=16000):
    """a click every 0.37 s over faint noise"""
    y = (1e-3 * np.random.RandomState(7).standard_normal(seconds * sr)).astype(np.float32)
    y[np.arange(int(0.2 * sr), y.size, int(0.37 * sr))] = 0.9
    y.setflags(write=False)
    return y


def test_condition_of_a_click_train_equals_the_restatement_fed_the_detected_frames():
    y = click_train()
    ac = speech.AudioCondition()
    frames = ac.detector.detect(y, units='frames')
    assert frames.size >= 3
    out = ac(y)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (y.size, 2) and out.is_contiguous()
    assert np.array_equal(bits(out.cpu().numpy()), bits(R.condition(y, frames)))
    env = ac.amplitude_envelope(y)
    assert env.is_cuda and tuple(env.shape) == (y.size,) and torch.equal(env, out[:, 0])
    assert torch.equal(ac(torch.from_numpy(y.copy()).cuda()), out)       # a device tensor stays where it is
    assert np.array_equal(bits(ac.amplitude_envelope(y, window=100).cpu().numpy()), bits(R.envelope(y, 100)))


def test_bad_input_raises():
    ac = speech.AudioCondition()
    for y in (np.zeros(1023, np.float32), np.zeros((2, 4096), np.float32), np.array([0.0] * 2047 + [np.nan], np.float32),
              torch.full((4096,), float('inf')).cuda()):
        with pytest.raises(ValueError):
            ac(y)
        with pytest.raises(ValueError):
            ac.amplitude_envelope(y)
    lib = L.load(require_gpu=True)
    y = torch.zeros(2048, device='cuda')
    out = torch.zeros(2048, 2, device='cuda')
    for n, window, n_frames in ((2048, 0, 0), (2048, 1025, 0), (1000, 1024, 0), (0, 1, 0), (2048, 1024, 2049)):
        rc = lib.mc_audio_condition(ctypes.c_void_p(y.data_ptr()), n, window, ctypes.c_void_p(y.data_ptr()), n_frames, ctypes.c_void_p(out.data_ptr()), None)
        assert rc == 1 and 'audio condition' in L.last_error()            # MC_ERR_ARG, nothing launched


def test_two_runs_and_another_stream_give_the_same_bits():
    y = torch.from_numpy(noise(3 * T + 517).copy()).cuda()
    mask = (torch.arange(1 + y.numel() // 512) % 3 == 0).to(torch.uint8).cuda()
    a, b = raw_condition(y, 1024, mask), raw_condition(y, 1024, mask)
    assert torch.equal(a, b) and not torch.isnan(a).any()
    ac = speech.AudioCondition()
    wave_dev = torch.from_numpy(click_train().copy()).cuda()
    c1, c2 = ac(wave_dev), ac(wave_dev)
    assert torch.equal(c1, c2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = raw_condition(y, 1024, mask)
        c3 = ac(wave_dev)
    side.synchronize()
    assert torch.equal(a, c) and torch.equal(c1, c3)


# ---- the window walk over the device condition ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def s2g_model():
    import motioncraft_amd as mc
    from motioncraft_amd import synthetic
    cfg = mc.Config.fromfile(S2G_CONFIG)
    arch = mc.build_architecture(cfg.model)
    arch.model = mc.ControlT2MHalf(arch.model, copy_blocks_num=cfg.copy_blocks_num, control_cond_feats=cfg.control_cond_feats, cfg=cfg)
    sd = synthetic.make_control_wav_state(arch.model.dims, cfg.copy_blocks_num, cfg.control_cond_feats, S2G_SEED)
    arch.load_state_dict({'model.' + k: v for k, v in sd.items()})
    yield arch
    arch.model.release()


def speech_like(n, seed=3):
    """noise under a slow envelope with a few clicks, float32 [n] in (-1, 1)"""
    rs = np.random.RandomState(seed)
    y = 0.05 * rs.standard_normal(n) * (1.0 + np.sin(np.arange(n) * (2 * np.pi / 3000.0)))
    y[rs.randint(0, n, 12)] = 0.8
    return y.astype(np.float32)


def test_sample_long_over_the_device_condition_equals_direct_calls(s2g_model):
    arch = s2g_model
    Lw, pre, r = S2G_WINDOW, S2G_PRE, S2G_ROWS
    assert arch.model.base_model.wav_encoder.out_len(r * Lw) == Lw         # the encoder turns a window's rows into the window's frames
    total = pre + 3 * (Lw - pre)
    cond = speech.AudioCondition()(speech_like(total * r + 80))
    assert cond.is_cuda and tuple(cond.shape) == (total * r + 80, 2)
    rows = R.window_rows(total, Lw, pre, r)
    assert len(rows) == 3 == longform.window_starts(total, Lw, pre)[0]
    g = torch.Generator().manual_seed(31)
    dims = arch.model.dims
    xf = torch.nn.functional.layer_norm(torch.randn(1, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda()
    x_Ts = [torch.randn(1, Lw, 322, generator=g) for _ in range(3)]

    def draws(seed):
        gen = torch.Generator().manual_seed(seed)
        return (torch.randn(1, Lw, 322, generator=gen) for _ in range(10 ** 6))
    fixed = lambda i: dict(noise=x_Ts[i], step_noise=draws(70 + i))
    seen = []

    def spy(**kw):
        seen.append(kw['c'])
        return arch(**kw)
    rec, wins = longform.sample_long(spy, total, Lw, pre, c=cond, c_rows_per_frame=r, text='a speech', condition_kwargs=dict(xf_out=xf),
                                     inference_kwargs=fixed)
    assert rec.shape == (total, 322) and len(wins) == 3 and np.isfinite(rec).all()
    dev = cond.device
    for i, (lo, hi) in enumerate(rows):
        # the slice the model saw is a view of the condition: nothing went through the host or was uploaded again
        assert seen[i].is_cuda and tuple(seen[i].shape) == (1, Lw * r, 2) and seen[i].data_ptr() == cond.data_ptr() + lo * 2 * 4
        kw = dict(motion=torch.zeros(1, Lw, 322, device=dev), motion_mask=torch.ones(1, Lw, device=dev),
                  motion_length=torch.tensor([Lw], device=dev).long(), num_intervals=1, motion_metas=[{'text': 'a speech'}],
                  c=cond[lo:hi].unsqueeze(0), xf_out=xf, inference_kwargs=fixed(i))
        direct = arch(**kw)[0]['pred_motion'][:Lw].numpy()
        assert np.array_equal(bits(direct), bits(wins[i])), (i, np.abs(direct - wins[i]).max())
    assert np.abs(wins[0] - wins[1]).max() > 1e-3                        # the windows differ: their audio and noise do
    other, _ = longform.sample_long(arch, total, Lw, pre, c=torch.roll(cond, 5000, 0), c_rows_per_frame=r, text='a speech',
                                    condition_kwargs=dict(xf_out=xf), inference_kwargs=fixed)
    assert not np.array_equal(other, rec)                                # and the condition reaches the sample


def test_s2g_sample_tool_writes_what_the_scorer_reads(tmp_path):
    n = 40 * S2G_ROWS + 80
    pcm = np.round(speech_like(n) * 32767).astype('<i2')
    path = tmp_path / 'clip_7.wav'
    with wave.open(str(path), 'wb') as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    assert np.array_equal(speech.read_wav(str(path), 16000), pcm.astype(np.float32) / 32768.0)
    out = tmp_path / 'res'
    cmd = [sys.executable, os.path.join(HERE, '..', 'tools', 's2g_sample.py'), S2G_CONFIG, f'synthetic:{S2G_SEED}', '--wav', str(path),
           '--words', 'hello', 'there', 'hello', '--out', str(out), '--motion_length', str(S2G_WINDOW), '--pre_frames', str(S2G_PRE),
           '--samples_per_frame', str(S2G_ROWS), '--random-condition', '1', '--seed', '4']
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    with np.load(out / 'res_clip_7.npz') as z:
        assert set(z.files) == {'betas', 'poses', 'expressions', 'trans', 'model', 'gender', 'mocap_frame_rate'}
        poses, exps, trans = z['poses'], z['expressions'], z['trans']
        assert poses.shape == (40, 165) and exps.shape == (40, 100) and trans.shape == (40, 3) and z['betas'].shape == (300,)
        assert str(z['model']) == 'smplx2020' and str(z['gender']) == 'neutral' and int(z['mocap_frame_rate']) == 30
    assert np.isfinite(poses).all() and poses[:, :66].any() and not poses[:, 69:75].any()
    # what tools/s2g_score.py makes of the file: the 322-d motion whose unpacking is the file again
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))
    back = scoring.unpack_rec_motion(scoring.pack_motion(t(poses), t(exps), t(trans)))
    assert all(torch.equal(a, t(b)) for a, b in zip(back, (poses, exps, trans)))

"""On the MI355X: ``mc_resample_poly`` / ``mc_pcm_decode`` (``csrc/mc_resample.hip``) and ``motioncraft_amd.audio`` against the numpy
restatement ``resample_ref.py`` and ``scipy.signal.resample_poly`` itself, then ``load_wav`` into the S2G front and the tool.

Bounds.
  * resampling: the kernel sums the restatement's products in fp64 and rounds once to float32, so for every sample
    ``|y_gpu - ref64| <= ulp32(ref64) / 2 + (n_terms + 2) * 2^-52 * sum |x_k h_k|`` (``bound``): the rounding to float32 plus the
    distance of two fp64 sums of the same n_terms products.  The same bound holds against scipy's fp64 output, which is such a sum
    too.  Against ``float32(scipy)`` both sides carry a rounding to float32: one ulp32 instead of half of one.
  * an all-ones clip: an interior output is the sum of its phase's taps.  That sum is NOT 1: scipy's design normalises the whole
    filter, and a single phase of the Kaiser(5.0) design is off by up to 6.8e-4 (``phase_sums``; scipy's own output shows the same
    ripple).  So the interior is held to its phase's sum within the bound, which is what catches a wrong phase table, and to 1
    within the filter's own ripple.
  * decode: EQUAL to the numpy statement of the formula, compared as bits -- the channel sum is exact in fp64, the division by the
    channel count and the conversion to float32 are IEEE operations numpy performs identically, the power of two is exact.
  * envelope of the resampled waveform: EQUAL to ``audio_cond_ref.envelope`` of the downloaded samples, as bits.
  * repeated runs, another stream: bit for bit.
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
from scipy.signal import resample_poly

import audio_cond_ref
import resample_ref as R
from motioncraft_amd import audio, speech
from motioncraft_amd import lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = audio.RESAMPLE_TILE
RATIOS = ((441, 320), (320, 441), (160, 441), (1, 3), (2, 1), (640, 441), (3, 2))
S2G_CONFIG = os.path.join(HERE, 'configs', 'stmogen_s2g_small.py')
S2G_SEED, S2G_WINDOW, S2G_PRE, S2G_ROWS = 2, 16, 4, 523                 # the small S2G model: 16-frame windows of 523 audio rows per frame


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def filt(up, down):
    taps = audio.resample_filter(up, down)
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def table(up, down):
    return torch.from_numpy(audio.phase_major(filt(up, down), up)).cuda()


def raw_resample(x, up, down, taps=None):
    """``mc_resample_poly`` itself: x float32 (numpy or a device tensor, taken where it lies) -> device [n_out], NaN before the launch"""
    lib = L.load(require_gpu=True)
    t = x if torch.is_tensor(x) else torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    tab = table(up, down) if taps is None else torch.from_numpy(audio.phase_major(taps, up)).cuda()
    n_taps = filt(up, down).size if taps is None else len(taps)
    out = torch.full((R.out_len(t.numel(), up, down),), float('nan'), device='cuda')
    L.check(lib.mc_resample_poly(ctypes.c_void_p(t.data_ptr()), t.numel(), up, down, ctypes.c_void_p(tab.data_ptr()), n_taps,
                                 ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
            'mc_resample_poly')
    return out


def bound(x64, up, down, taps, ref64):
    return R.ulp32(ref64) / 2 + R.fp64_bound(x64, up, down, taps)


def check(x, up, down, taps=None, got=None):
    """x float32 [n] -> the kernel's output, held to the restatement and to scipy"""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    h = filt(up, down) if taps is None else np.asarray(taps, np.float64)
    ref = R.resample(x64, up, down, h)
    sci = resample_poly(x64, up, down) if taps is None else resample_poly(x64, up, down, window=h / up)
    got = (raw_resample(x, up, down, taps) if got is None else got).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape == sci.shape
    b = bound(x64, up, down, h, ref)
    err, err_sci, err_sci32 = np.abs(got - ref), np.abs(got - sci), np.abs(got.astype(np.float64) - sci.astype(np.float32))
    print(f'{up}/{down} n={x.size}: max |gpu - ref64| / bound = {np.max(err / np.maximum(b, 1e-300)):.3f}, '
          f'{int((bits(got) != bits(sci.astype(np.float32))).sum())} of {got.size} differ from float32(scipy) in a bit')
    bad = np.flatnonzero(~(err <= b))
    assert bad.size == 0, (up, down, x.size, bad[:8], got[bad[:8]], ref[bad[:8]], b[bad[:8]])
    assert (err_sci <= b).all(), np.flatnonzero(~(err_sci <= b))[:8]
    assert (err_sci32 <= b + R.ulp32(sci) / 2).all()
    return got, ref, b


def pcm16(n, seed):
    """random 16-bit-valued samples in [-1, 1), float32"""
    return (np.random.RandomState(seed).randint(-32768, 32768, n).astype(np.float32) / 32768.0)


def tile_n(up, down):
    """the longest clip whose outputs fit one tile: ``tile_n + 1`` starts a second workgroup"""
    n = T * down // up
    assert R.out_len(n, up, down) <= T < R.out_len(n + 1, up, down)
    return n


def whole_n(up, down):
    """a clip of more than one tile with n * up % down == 0"""
    return down * -(-(T + T // 5) // up)


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('up,down', RATIOS)
def test_kernel_at_the_tile_edges(up, down):
    check(pcm16(37, 1), up, down)                                        # shorter than one filter span
    n = tile_n(up, down)
    for m in (n - 1, n, n + 1):
        check(pcm16(m, m), up, down)
    if R.out_len(n, up, down) != T:                                      # no clip gives exactly T outputs at this ratio: the last full one
        assert up > down


@pytest.mark.parametrize('up,down', RATIOS)
def test_kernel_over_several_tiles_with_and_without_a_remainder(up, down):
    n = whole_n(up, down)
    assert n * up % down == 0 and R.out_len(n, up, down) > T
    check(pcm16(n, 5), up, down)
    if down > 1:
        assert (n + 1) * up % down != 0
        check(pcm16(n + 1, 6), up, down)
    check(pcm16(3 * tile_n(up, down) + 17, 7), up, down)                  # four workgroups, the last one short


def phase_sums(up, down):
    """fp64 [up]: the sum of each phase's taps, what an interior output of an all-ones clip is"""
    return audio.phase_major(filt(up, down), up).sum(axis=1)


@pytest.mark.parametrize('up,down', RATIOS)
def test_all_ones_give_each_phase_its_taps_sum(up, down):
    n = whole_n(up, down) + 1
    taps = filt(up, down)
    half = (taps.size - 1) // 2
    got, ref, b = check(np.ones(n, np.float32), up, down)
    m = np.arange(got.size)
    q = half + m * down
    interior = (q - (taps.size - 1) >= 0) & (q // up <= n - 1)            # every tap of the phase meets a sample of the clip
    assert interior.sum() > T // 2
    sums = phase_sums(up, down)
    want = sums[q % up]
    assert (np.abs(got - want)[interior] <= (R.ulp32(want) / 2 + b)[interior]).all()
    ripple = np.abs(sums - 1.0).max()
    assert ripple < 1e-3                                                 # the filter's own: 6.8e-4 at 441/320, 2e-16 at 1/3
    assert (np.abs(got - 1.0)[interior] <= ripple + (R.ulp32(1.0) / 2 + b)[interior]).all()
    assert np.abs(got - 1.0)[~interior].max() > 0.01                     # and the edges of the clip are not: zero padding


@pytest.mark.parametrize('up,down', RATIOS)
def test_impulses_at_both_ends_and_zeros(up, down):
    n = whole_n(up, down) + 1
    taps = filt(up, down)
    for at in (0, n - 1):
        x = np.zeros(n, np.float32)
        x[at] = 1.0
        got, ref, _ = check(x, up, down)
        assert np.count_nonzero(got) > 0
        m = np.arange(got.size)
        t = (taps.size - 1) // 2 + m * down - at * up                    # the one tap each output sees
        seen = (t >= 0) & (t < taps.size)
        assert np.array_equal(bits(got[seen]), bits(taps[t[seen]].astype(np.float32))) and not bits(got[~seen]).any()
    for zero in (0.0, -0.0):
        out = raw_resample(np.full(n, zero, np.float32), up, down).cpu().numpy()
        assert out.shape == (R.out_len(n, up, down),) and not bits(out).any()    # exact zeros, +0


def test_a_clip_that_does_not_start_on_16_bytes():
    up, down = 160, 441
    n = 2 * tile_n(up, down) + 300
    host = pcm16(n + 3, 11)
    dev = torch.from_numpy(host).cuda()
    for start in (1, 2, 3):
        cut = dev[start:]
        assert cut.data_ptr() % 16 == 4 * start
        check(host[start:], up, down, got=raw_resample(cut, up, down))


def test_filters_of_the_callers():
    """a filter shorter than ``up`` (phases without a tap), one tap, an asymmetric one, and ``Resampler(taps=)``"""
    for up, down, taps in ((5, 3, [1.0, 2.0, 3.0]), (4, 1, [2.5]), (3, 7, np.arange(1.0, 12.0)), (1, 2, [0.25, 0.5, 0.25])):
        for n in (1, 2, 700):
            check(pcm16(n, n + up), up, down, taps=np.asarray(taps))
    x = pcm16(3000, 4)
    taps = audio.resample_filter(160, 441, window='hamming')
    r = audio.Resampler(44100, 16000, taps=taps)
    assert (r.up, r.down) == (160, 441)
    check(x, 160, 441, taps=taps, got=r(torch.from_numpy(x).cuda()))
    same = audio.Resampler(48000, 48000)
    t = torch.from_numpy(x).cuda()
    assert same(t) is t
    for bad in (x, torch.from_numpy(x), t.double(), t.reshape(2, -1), t[:0]):
        with pytest.raises(ValueError):
            r(bad)


def test_an_index_past_2_to_the_31():
    """m * down passes 2^31 at output 4 869 481 for down = 441: five minutes of audio at 16 kHz.  The references here are scipy's
    fp64 output and, for the bound's ``sum |x_k h_k|``, scipy again on the magnitudes (inflated by 1e-9 for its own rounding)."""
    up, down = 160, 441
    n_out = 2 ** 31 // down + 3 * T + 5
    n = n_out * down // up
    x = pcm16(n, 12)
    x64 = x.astype(np.float64)
    taps = filt(up, down)
    got = raw_resample(x, up, down).cpu().numpy()
    sci = resample_poly(x64, up, down)
    assert got.shape == sci.shape and (got.size - 1) * down > 2 ** 31
    mag = resample_poly(np.abs(x64), up, down, window=np.abs(taps) / up) * (1 + 1e-9)
    b = R.ulp32(sci) / 2 + (-(-taps.size // up) + 2) * 2.0 ** -52 * mag
    bad = np.flatnonzero(~(np.abs(got - sci) <= b))
    assert bad.size == 0, (bad[:8], got[bad[:8]], sci[bad[:8]])


def test_two_runs_and_another_stream_give_the_same_bits():
    up, down = 160, 441
    x = torch.from_numpy(pcm16(3 * tile_n(up, down) + 17, 9)).cuda()
    a, b = raw_resample(x, up, down), raw_resample(x, up, down)
    assert torch.equal(a, b) and not torch.isnan(a).any()
    r = audio.Resampler(44100, 16000)
    c1, c2 = r(x), r(x)
    assert torch.equal(c1, c2) and torch.equal(c1, a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = raw_resample(x, up, down)
        c3 = r(x)
    side.synchronize()
    assert torch.equal(a, c) and torch.equal(a, c3)


# ---- decode --------------------------------------------------------------------------------------------------------------
def pack(ints, width):
    """int64 [frames, channels] -> the bytes a wav file of that width holds"""
    if width == 1:
        return (ints + 128).astype(np.uint8).tobytes()
    if width == 3:
        return np.ascontiguousarray(ints.astype('<i4').view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    return ints.astype({2: '<i2', 4: '<i4'}[width]).tobytes()


def frames_of(width, channels, n, seed):
    lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
    ints = np.random.RandomState(seed).randint(lo, hi + 1, (n, channels), dtype=np.int64)
    ends = np.array([[lo] * 3, [hi] * 3, [lo, hi, lo], [hi, lo, hi], [hi, hi, hi - 1], [0, -1, 1]], np.int64)[:, :channels]
    ints[:min(n, len(ends))] = ends[:n]
    return ints


@pytest.mark.parametrize('width', (1, 2, 3, 4))
def test_decode_equals_the_formula(width):
    scale = 2.0 ** (8 * width - 1)
    for channels in (1, 2, 3):
        for n in (1, 1000):
            ints = frames_of(width, channels, n, 10 * width + channels)
            raw = torch.frombuffer(bytearray(pack(ints, width)), dtype=torch.uint8).cuda()
            assert raw.numel() == n * channels * width
            mean = np.float32(ints.sum(axis=1, dtype=np.float64) / channels / scale)
            first = np.float32(ints[:, 0].astype(np.float64) / scale)
            got_mean, got_first = audio.decode_pcm(raw, channels, width, mono=True), audio.decode_pcm(raw, channels, width, mono=False)
            assert got_mean.is_cuda and got_mean.dtype == torch.float32 and tuple(got_mean.shape) == (n,)
            assert np.array_equal(bits(got_mean.cpu().numpy()), bits(mean)), (width, channels, n)
            assert np.array_equal(bits(got_first.cpu().numpy()), bits(first)), (width, channels, n)
            assert np.abs(mean).max() <= 1.0 and (channels > 1 or np.array_equal(bits(mean), bits(first)))
    raw = torch.zeros(12, dtype=torch.uint8).cuda()
    for bad in (dict(raw=raw, channels=5, sample_bytes=1), dict(raw=raw[:0], channels=1, sample_bytes=2), dict(raw=raw.cpu(), channels=1, sample_bytes=2),
                dict(raw=raw.float(), channels=1, sample_bytes=2)):
        with pytest.raises(ValueError):
            audio.decode_pcm(**bad)


def write_wav(path, ints, rate, width=2):
    with wave.open(str(path), 'wb') as f:
        f.setnchannels(ints.shape[1]), f.setsampwidth(width), f.setframerate(rate)
        f.writeframes(pack(ints, width))


def test_first_channel_form_equals_read_wav(tmp_path):
    ints = frames_of(2, 2, 3000, 5)
    write_wav(tmp_path / 'a.wav', ints, 16000)
    y, rate = audio.load_wav(str(tmp_path / 'a.wav'), mono=False)
    assert rate == 16000 and y.is_cuda and y.dtype == torch.float32
    assert np.array_equal(bits(y.cpu().numpy()), bits(speech.read_wav(str(tmp_path / 'a.wav'), 16000)))
    z, _ = audio.load_wav(str(tmp_path / 'a.wav'), sr=16000, mono=False)  # the file's own rate: nothing is resampled
    assert torch.equal(y, z)


# ---- load_wav ------------------------------------------------------------------------------------------------------------
FILE_SR, FILE_FRAMES = 44100, 23300                                      # 0.53 s: one 16-frame window of the small S2G model at 16 kHz


def speech_like(n, sr, seed=3):
    """noise under a slow envelope with a few clicks, in (-1, 1); the envelope's period is 3000 samples at 16 kHz"""
    rs = np.random.RandomState(seed)
    y = 0.05 * rs.standard_normal(n) * (1.0 + np.sin(np.arange(n) * (2 * np.pi * 16000 / (3000.0 * sr))))
    y[rs.randint(0, n, 12)] = 0.8
    return y


def stereo16(n, sr, seed=3):
    """int64 [n, 2]: two channels that differ"""
    left, right = speech_like(n, sr, seed), 0.5 * np.roll(speech_like(n, sr, seed), 7)
    return np.round(np.stack([left, right], axis=1) * 32767).astype(np.int64)


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    ints = stereo16(FILE_FRAMES, FILE_SR)
    path = tmp_path_factory.mktemp('wav') / 'stereo_44k.wav'
    write_wav(path, ints, FILE_SR)
    mono = np.float32(ints.sum(axis=1, dtype=np.float64) / 2 / 32768.0)
    mono.setflags(write=False)
    return str(path), mono


def test_load_wav_to_16k_matches_the_scipy_chain(clip):
    path, mono = clip
    y, rate = audio.load_wav(path)
    assert rate == FILE_SR and np.array_equal(bits(y.cpu().numpy()), bits(mono))
    y16, rate = audio.load_wav(path, sr=16000)
    assert rate == 16000 and y16.is_cuda and y16.dtype == torch.float32 and y16.is_contiguous()
    assert tuple(y16.shape) == (-(-FILE_FRAMES * 16000 // FILE_SR),) == (8454,)
    check(mono, 160, 441, got=y16)
    assert torch.equal(audio.load_wav(path, sr=16000)[0], y16)
    assert audio.describe(path, 16000).count('44100 -> 16000') == 1 and '2 channels, 16-bit' in audio.describe(path, 16000)
    assert '44100 -> 22050 -> 16000' in audio.describe(path, 16000, 22050)


def test_load_wav_through_22050_matches_the_two_stage_scipy_chain(clip):
    path, mono = clip
    mid, rate = audio.load_wav(path, load_sr=22050)
    assert rate == 22050 and tuple(mid.shape) == (-(-FILE_FRAMES // 2),)
    check(mono, 1, 2, got=mid)
    y16, rate = audio.load_wav(path, sr=16000, load_sr=22050)
    n_mid = -(-FILE_FRAMES * 22050 // FILE_SR)
    assert rate == 16000 and tuple(y16.shape) == (-(-n_mid * 16000 // 22050),)       # the nested ceils, as librosa's lengths
    check(mid.cpu().numpy(), 320, 441, got=y16)                           # the second stage on the downloaded intermediate
    assert torch.equal(audio.Resampler(22050, 16000)(mid), y16)
    direct = audio.load_wav(path, sr=16000)[0]
    assert direct.shape != y16.shape or not torch.equal(direct, y16)     # the detour is not the direct route


# ---- into the S2G front --------------------------------------------------------------------------------------------------
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


def test_resampled_waveform_feeds_the_audio_condition_and_the_sampler(clip, s2g_model):
    path, _ = clip
    y16, _ = audio.load_wav(path, sr=16000)
    cond = speech.AudioCondition()(y16)
    assert cond.is_cuda and tuple(cond.shape) == (y16.numel(), 2)
    assert np.array_equal(bits(cond[:, 0].cpu().numpy()), bits(audio_cond_ref.envelope(y16.cpu().numpy())))
    frames = speech.speech_frames(y16.numel(), S2G_ROWS)
    assert frames == S2G_WINDOW
    dims = s2g_model.model.dims
    g = torch.Generator().manual_seed(31)
    xf = torch.nn.functional.layer_norm(torch.randn(1, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda()
    gen = torch.Generator(device=y16.device).manual_seed(4)
    rec, windows = speech.sample_speech(s2g_model, y16, words=['hello', 'there'], motion_length=S2G_WINDOW, pre_frames=S2G_PRE,
                                        samples_per_frame=S2G_ROWS, fix_very_first=False, input_dim=dims['input_feats'],
                                        condition_kwargs=dict(xf_out=xf), inference_kwargs=dict(generator=gen))
    assert rec.shape == (frames, 322) and len(windows) == 1 and np.isfinite(rec).all()


# ---- the tool ------------------------------------------------------------------------------------------------------------
def test_s2g_sample_tool_resamples_only_when_asked(tmp_path):
    """the clip of the existing tool test (40 frames of 523 rows + 80 samples at 16 kHz), re-rendered at 44.1 kHz stereo"""
    n_file = -(-(40 * S2G_ROWS + 80) * 441 // 160)
    n_out = -(-n_file * 160 // 441)
    assert speech.speech_frames(n_out, S2G_ROWS) == 40
    path = tmp_path / 'clip_7.wav'
    write_wav(path, stereo16(n_file, FILE_SR), FILE_SR)
    out = tmp_path / 'res'
    cmd = [sys.executable, os.path.join(HERE, '..', 'tools', 's2g_sample.py'), S2G_CONFIG, f'synthetic:{S2G_SEED}', '--wav', str(path),
           '--words', 'hello', 'there', 'hello', '--out', str(out), '--motion_length', str(S2G_WINDOW), '--pre_frames', str(S2G_PRE),
           '--samples_per_frame', str(S2G_ROWS), '--random-condition', '1', '--seed', '4']
    done = subprocess.run(cmd + ['--resample'], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert '44100 -> 16000' in done.stdout and '44100 Hz, 2 channels, 16-bit' in done.stdout and f'{n_out} samples' in done.stdout
    with np.load(out / 'res_clip_7.npz') as z:
        poses, exps, trans = z['poses'], z['expressions'], z['trans']
    frames = speech.speech_frames(n_out, S2G_ROWS)
    assert poses.shape == (frames, 165) and exps.shape == (frames, 100) and trans.shape == (frames, 3)
    assert np.isfinite(poses).all() and np.isfinite(exps).all() and np.isfinite(trans).all() and poses[:, :66].any()
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert plain.returncode != 0 and '44100 Hz, but the detector runs at 16000 Hz.  Resampling stays with the caller' in plain.stderr
    bad = subprocess.run(cmd + ['--load_sr', '22050'], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2 and '--load_sr needs --resample' in bad.stderr

"""Audio onset detection restated in float64 numpy: what ``librosa.onset.onset_detect(y, sr, hop_length=512, units='time')`` of
librosa 0.10.1 computes with its defaults (the call of the reference's ``alignment.load_audio``).  librosa is not a dependency,
so this restatement is what ``csrc/mc_onset.hip`` and ``motioncraft_amd.scoring.OnsetDetector`` are pinned to.

  frames    y padded with n_fft/2 zeros on both sides; F = 1 + N // hop frames of n_fft samples, times the periodic Hann window
  power     |rfft(frame)|^2, n_fft/2 + 1 bins
  mel       W [n_mels, bins] (Slaney scale, Slaney norm, fmin 0, fmax sr/2; computed in float64, stored as float32) times power
  dB        10 log10(max(1e-10, M)), then max(S, max(S) - 80) over the whole spectrogram
  envelope  d[i] = mean over mel rows of max(0, S[:, i+1] - S[:, i]);  env = concat(zeros(1 + n_fft // (2 hop)), d)[:F]
  normalise env -= min; env /= max + tiny; an all-zero envelope has no onsets
  pick      n is an onset iff env[n] == max(env[n-pre_max : n+post_max]) and env[n] >= mean(env[n-pre_avg : n+post_avg]) + delta
            and env[n] > 0 and n > last onset + wait; windows truncated at both ends of the array

``peak_pick_windows`` states the last step as written above; ``peak_pick_filters`` states it the way librosa does, with scipy's
running filters and the two edge corrections.  ``test_onset_host.py`` holds them against each other.
"""
import numpy as np

N_FFT, HOP, N_MELS = 2048, 512, 128
DELTA = 0.07


def num_frames(n, hop=HOP):
    return 1 + n // hop


def hann(n_fft=N_FFT):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)


def power_spectrum(y, n_fft=N_FFT, hop=HOP):
    """y [N] -> float64 [F, n_fft/2 + 1]"""
    y = np.asarray(y, np.float64)
    pad = np.concatenate([np.zeros(n_fft // 2), y, np.zeros(n_fft // 2)])
    F = num_frames(y.size, hop)
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(pad[idx] * hann(n_fft)[None, :], axis=1)
    return spec.real ** 2 + spec.imag ** 2


def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    step = np.log(6.4) / 27
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / step, f / (200.0 / 3))


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    step = np.log(6.4) / 27
    return np.where(m >= 15.0, 1000.0 * np.exp(step * (m - 15.0)), (200.0 / 3) * m)


def mel_points(sr, n_mels=N_MELS):
    """the n_mels + 2 band edges in Hz"""
    return mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2), n_mels + 2))


def mel_basis(sr, n_fft=N_FFT, n_mels=N_MELS):
    """float32 [n_mels, n_fft/2 + 1]"""
    pts = mel_points(sr, n_mels)
    freqs = np.arange(n_fft // 2 + 1) * (sr / n_fft)
    ramps = pts[:, None] - freqs[None, :]
    width = np.diff(pts)
    W = np.zeros((n_mels, freqs.size))
    for i in range(n_mels):
        W[i] = np.maximum(0.0, np.minimum(-ramps[i] / width[i], ramps[i + 2] / width[i + 1]))
    W *= (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return W.astype(np.float32)


def envelope_from_power(P, W, n_fft=N_FFT, hop=HOP):
    """power [F, bins] (any float dtype; the arithmetic stays in it) + mel basis -> the un-normalised envelope [F]"""
    M = P @ W.astype(P.dtype).T
    S = 10.0 * np.log10(np.maximum(P.dtype.type(1e-10), M))
    S = np.maximum(S, S.max() - 80.0)
    d = np.maximum(0.0, S[1:] - S[:-1]).mean(axis=1)
    lag = 1 + n_fft // (2 * hop)
    return np.concatenate([np.zeros(lag, P.dtype), d.astype(P.dtype)])[:P.shape[0]]


def onset_strength(y, sr, n_fft=N_FFT, hop=HOP, n_mels=N_MELS):
    return envelope_from_power(power_spectrum(y, n_fft, hop), mel_basis(sr, n_fft, n_mels), n_fft, hop)


def onset_strength_fp32(y, sr, n_fft=N_FFT, hop=HOP, n_mels=N_MELS):
    """The same in float32 on the CPU: ``torch.stft`` float32 (center, constant padding, periodic Hann), then a float32 mel
    projection, dB and flux.  Its distance from ``onset_strength`` is the rounding band a float32 implementation may claim."""
    import torch
    yt = torch.from_numpy(np.array(y, np.float32))
    F = num_frames(yt.numel(), hop)
    if yt.numel() <= n_fft // 2:                      # torch refuses a constant pad wider than the input; pad by hand
        yt = torch.cat([torch.zeros(n_fft // 2), yt, torch.zeros(n_fft // 2)])
        spec = torch.stft(yt, n_fft, hop_length=hop, window=torch.hann_window(n_fft, periodic=True), center=False, return_complex=True)
    else:
        spec = torch.stft(yt, n_fft, hop_length=hop, window=torch.hann_window(n_fft, periodic=True), center=True, pad_mode='constant',
                          return_complex=True)
    P = (spec.real ** 2 + spec.imag ** 2).T.contiguous().numpy()
    assert P.dtype == np.float32 and P.shape == (F, n_fft // 2 + 1)
    return envelope_from_power(P, mel_basis(sr, n_fft, n_mels), n_fft, hop)


def normalise(env):
    """float64; an all-zero envelope stays all zero"""
    env = np.asarray(env, np.float64)
    env = env - env.min()
    return env / (env.max() + np.finfo(np.float64).tiny)


def pick_sizes(sr, hop=HOP):
    """(pre_max, post_max, pre_avg, post_avg, wait) of onset_detect's defaults"""
    return (int(0.03 * sr // hop), int(0.00 * sr // hop + 1), int(0.10 * sr // hop), int(0.10 * sr // hop + 1), int(0.03 * sr // hop))


def pick_terms(x, pre_max, post_max, pre_avg, post_avg):
    """(window maximum, window mean) per frame, windows truncated at the ends"""
    x = np.asarray(x, np.float64)
    n = x.size
    mx = np.array([x[max(0, i - pre_max):min(n, i + post_max)].max() for i in range(n)])
    av = np.array([x[max(0, i - pre_avg):min(n, i + post_avg)].mean() for i in range(n)])
    return mx, av


def greedy_wait(candidates, wait):
    out, last = [], -np.inf
    for i in np.flatnonzero(candidates):
        if i > last + wait:
            out.append(i)
            last = i
    return np.asarray(out, np.int64)


def peak_pick_windows(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    x = np.asarray(x, np.float64)
    mx, av = pick_terms(x, pre_max, post_max, pre_avg, post_avg)
    return greedy_wait((x == mx) & (x >= av + delta) & (x > 0), wait)


def peak_pick_filters(x, pre_max, post_max, pre_avg, post_avg, delta, wait):
    """librosa 0.10.1's ``util.peak_pick``: running filters, the truncated means written over both edges, the greedy loop"""
    import scipy.ndimage
    x = np.asarray(x, np.float64)
    mov_max = scipy.ndimage.maximum_filter1d(x, int(pre_max + post_max), mode='constant', origin=int(np.ceil(0.5 * (pre_max - post_max))),
                                             cval=x.min())
    mov_avg = scipy.ndimage.uniform_filter1d(x, int(pre_avg + post_avg), mode='nearest', origin=int(np.ceil(0.5 * (pre_avg - post_avg))))
    n = 0
    while n - pre_avg < 0 and n < x.shape[0]:
        mov_avg[n] = np.mean(x[max(n - pre_avg, 0):n + post_avg])
        n += 1
    n = max(x.shape[0] - post_avg, 0)
    while n < x.shape[0]:
        mov_avg[n] = np.mean(x[max(n - pre_avg, 0):n + post_avg])
        n += 1
    detections = x * (x == mov_max)
    detections = detections * (detections >= mov_avg + delta)
    return greedy_wait(detections != 0, wait)


def onset_frames(env, sr, hop=HOP, pick=peak_pick_windows):
    """un-normalised envelope -> int64 onset frames"""
    env = np.asarray(env, np.float64)
    if not env.any():
        return np.zeros(0, np.int64)
    return pick(normalise(env), *pick_sizes(sr, hop)[:4], DELTA, pick_sizes(sr, hop)[4])


def onset_detect(y, sr, hop=HOP, units='time'):
    frames = onset_frames(onset_strength(y, sr, hop=hop), sr, hop)
    return frames * hop / sr if units == 'time' else frames


def base_signal(sr, n_samples, seed, bursts=60):
    """float32 [n_samples]: white noise of 0.02 rms plus `bursts` exponentially decaying tone bursts with random onset, frequency
    150 .. 3500 Hz, amplitude 0.05 .. 0.8 and a decay time of 30 .. 120 ms"""
    rs = np.random.RandomState(seed)
    y = 0.02 * rs.standard_normal(n_samples)
    t = np.arange(n_samples) / sr
    for _ in range(bursts):
        t0, f, a, tau = rs.uniform(0, 0.97 * n_samples / sr), rs.uniform(150, 3500), rs.uniform(0.05, 0.8), rs.uniform(0.03, 0.12)
        on = t >= t0
        y[on] += a * np.exp(-(t[on] - t0) / tau) * np.sin(2 * np.pi * f * (t[on] - t0))
    return y.astype(np.float32)

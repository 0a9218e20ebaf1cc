"""Rational resampling restated in numpy, fp64: ``scipy.signal.resample_poly(x, up, down)`` with zero padding, which is librosa's
``res_type='polyphase'`` mode, as one closed form.  ``csrc/mc_resample.hip`` and ``motioncraft_amd.audio.Resampler`` are pinned to
this file and, through ``tests/test_resample_host.py``, to scipy itself.

    y[m] = sum over k of x[k] * taps[half + m*down - k*up],   0 <= k < n_in,   0 <= half + m*down - k*up < n_taps

for m in 0 .. ceil(n_in * up / down) - 1, with ``taps`` the odd-length filter already multiplied by ``up`` and
``half = (n_taps - 1) / 2``: the input with ``up - 1`` zeros between its samples, convolved with the filter centred on output
position ``m * down``, zeros outside the clip.  ``resample`` is a plain loop over the outputs.  ``terms`` gives, per output, the
number of products and the sum of their magnitudes: an fp64 sum of n terms in any order is within ``n * 2^-53 * sum |x_k h_k|``
(to first order) of the exact one, so two such sums differ by at most ``(n + 2) * 2^-52 * sum |x_k h_k|`` -- ``fp64_bound`` -- with
the + 2 covering the products' own roundings and the second-order terms; a result rounded to float32 adds half its ulp
(``ulp32``)."""
import numpy as np


def out_len(n_in, up, down):
    return -(-n_in * up // down)


def _window(m, n_in, up, down, n_taps):
    """the inputs k and taps t = half + m*down - k*up of output m, k ascending"""
    q = (n_taps - 1) // 2 + m * down
    k_lo = max(0, -(-(q - (n_taps - 1)) // up))
    k_hi = min(n_in - 1, q // up)
    k = np.arange(k_lo, k_hi + 1)
    return k, q - k * up


def resample(x, up, down, taps):
    """x [n_in], taps fp64 [n_taps] (odd, times ``up``) -> fp64 [ceil(n_in * up / down)]"""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    if taps.ndim != 1 or taps.size % 2 != 1:
        raise ValueError('an odd-length filter')
    y = np.zeros(out_len(x.size, up, down))
    for m in range(y.size):
        k, t = _window(m, x.size, up, down, taps.size)
        acc = 0.0
        for a, b in zip(x[k].tolist(), taps[t].tolist()):              # ascending k, one product and one add at a time
            acc += a * b
        y[m] = acc
    return y


def terms(x, up, down, taps):
    """per output: (the number of products, the sum of their magnitudes), int64 [n_out] and fp64 [n_out]"""
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    n_out = out_len(x.size, up, down)
    count, mag = np.zeros(n_out, np.int64), np.zeros(n_out)
    for m in range(n_out):
        k, t = _window(m, x.size, up, down, taps.size)
        count[m], mag[m] = k.size, np.abs(x[k] * taps[t]).sum()
    return count, mag


def fp64_bound(x, up, down, taps):
    count, mag = terms(x, up, down, taps)
    return (count + 2) * 2.0 ** -52 * mag


def ulp32(v):
    """the spacing of float32 at |v| (fp64 in, fp64 out); the subnormal spacing below 2^-126"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 23)

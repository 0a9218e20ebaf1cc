"""fp64 numpy restatement of the multistep sampler (DPM-Solver++ 2M on the data prediction) and the closed-form problem that
decided its design.  Nothing here imports the package: the tests compare the package against this file.

Schedule: ``ab[i]`` / ``ab_prev[i]`` are alpha-bar at spaced index i and at the level below it (``ab_prev[0] == 1``).  With
alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha / sigma), s = index i, t = the level below it, h = lambda_t - lambda_s:

    order 1:  x <- (sigma_t / sigma_s) x - alpha_t expm1(-h) x0                                       (DDIM, eta = 0)
    order 2:  r = h_prev / h,  D = (1 + 1 / (2 r)) x0 - (1 / (2 r)) x0_prev,  then order 1 with D in place of x0

i.e. x_prev = kx x + k0 x0 + k1 x0_prev.  First-order updates: the first of a walk, the one at i == 1 (the last with a finite h; the
lower-order final step, ``final_first_order``), and the one at i == 0, which is exactly (0, 1, 0).
"""
import math

import numpy as np


def linear_alphas_cumprod(T=1000):
    k = 1000 / T
    return np.cumprod(1.0 - np.linspace(k * 0.0001, k * 0.02, T, dtype=np.float64))


def spaced(ac, timesteps):
    """(ab, ab_prev, timestep_map) of the base alpha-bars ``ac`` restricted to ``timesteps``"""
    tmap = sorted(int(t) for t in set(timesteps))
    ab = np.asarray([ac[t] for t in tmap], dtype=np.float64)
    return ab, np.append(1.0, ab[:-1]), tmap


def time_timesteps(T, S):
    """the 'ddimS' spacing: a constant integer stride from 0"""
    for stride in range(1, T):
        if len(range(0, T, stride)) == S:
            return set(range(0, T, stride))
    raise ValueError((T, S))


def logsnr_timesteps(ac, S):
    """S points uniform in lambda between lambda(T-1) and lambda(0), each snapped to the timestep of nearest lambda, plus both ends"""
    T = len(ac)
    lam = 0.5 * (np.log(ac) - np.log1p(-ac))
    kept = {0, T - 1}
    for v in np.linspace(lam[T - 1], lam[0], S):
        kept.add(int(np.argmin(np.abs(lam - v))))
    return kept


def coef_table(ab, ab_prev, indices, order=2, final_first_order=True):
    """[(kx, k0, k1)] of a walk through ``indices`` (fp64)"""
    out, h_prev = [], None
    for i in indices:
        if ab_prev[i] >= 1.0:
            out.append((0.0, 1.0, 0.0))
            h_prev = None
            continue
        a_s, s_s = math.sqrt(ab[i]), math.sqrt(1 - ab[i])
        a_t, s_t = math.sqrt(ab_prev[i]), math.sqrt(1 - ab_prev[i])
        h = math.log(a_t / s_t) - math.log(a_s / s_s)
        kx, k0, k1 = s_t / s_s, -a_t * math.expm1(-h), 0.0
        if order == 2 and h_prev is not None and not (final_first_order and i == 1):
            r = h_prev / h
            k0, k1 = k0 * (1 + 1 / (2 * r)), -k0 / (2 * r)
        out.append((kx, k0, k1))
        h_prev = h
    return out


def update(k, x, x0, x0_prev):
    """one update in fp64; x0_prev is not touched when k1 == 0 (it may be None or hold NaN)"""
    kx, k0, k1 = k
    out = kx * np.asarray(x, dtype=np.float64) + k0 * np.asarray(x0, dtype=np.float64)
    if k1 != 0.0:
        out = out + k1 * np.asarray(x0_prev, dtype=np.float64)
    return out


def loop(denoise_fn, x_T, ab, ab_prev, indices, order=2, final_first_order=True):
    """``denoise_fn(x, i) -> x0``; returns the sample after the last index"""
    x, x0_prev = np.asarray(x_T, dtype=np.float64), None
    for k, i in zip(coef_table(ab, ab_prev, indices, order, final_first_order), indices):
        x0 = denoise_fn(x, i)
        x = update(k, x, x0, x0_prev)
        x0_prev = x0
    return x


# ---- the Gaussian toy problem: per-element data N(0, s2) -------------------------------------------------------------------------
def toy_predictor(s2, ab):
    """the optimal x0 prediction  E[x0 | x] = s2 sqrt(ab) / (s2 ab + 1 - ab) x"""
    return lambda x, i: s2 * math.sqrt(ab[i]) / (s2 * ab[i] + 1 - ab[i]) * x


def toy_exact(s2, ab_T, x_T=1.0):
    """the probability-flow solution at ab = 1 started from x_T at ab_T:  x_T s / sqrt(s2 ab_T + 1 - ab_T)"""
    return x_T * math.sqrt(s2) / math.sqrt(s2 * ab_T + 1 - ab_T)


def toy_error(spacing, s2, S, order=2, final_first_order=True, T=1000):
    """|solver - exact| at ab = 1 for x_T = 1 on the linear T-step schedule spaced to S ('time' or 'logsnr')"""
    ac = linear_alphas_cumprod(T)
    ts = time_timesteps(T, S) if spacing == 'time' else logsnr_timesteps(ac, S)
    ab, ab_prev, _ = spaced(ac, ts)
    idx = list(range(len(ab)))[::-1]
    got = loop(toy_predictor(s2, ab), 1.0, ab, ab_prev, idx, order, final_first_order)
    return abs(float(got) - toy_exact(s2, ab[-1]))


def toy_table(Ss=(10, 20, 50), s2s=(0.25, 1.0, 4.0), spacings=('time', 'logsnr')):
    """rows (spacing, s2, S, order-1 error, plain 2M error, 2M with the first-order last update)"""
    return [(sp, s2, S, toy_error(sp, s2, S, 1), toy_error(sp, s2, S, 2, False), toy_error(sp, s2, S, 2, True))
            for sp in spacings for s2 in s2s for S in Ss]


if __name__ == '__main__':
    print('| spacing | s² | S | DDIM | plain 2M | 2M + first-order last update |')
    print('|---|---|---|---|---|---|')
    for sp, s2, S, e1, e2p, e2 in toy_table():
        print(f'| {sp} | {s2:g} | {S} | {e1:.3f} | {e2p:.3f} | {e2:.3f} |')

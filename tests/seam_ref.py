"""fp64 numpy restatement of the coupled-window sampler update (``mc_ctx_set_seams`` / ``sampler_seam_k``): the plan rules, the seam
blend and the step.  Nothing here imports the package: the tests compare the package against this file.

Windows of ``T`` frames, overlap ``ov`` with ``0 < 2 ov <= T``, ``stride = T - ov``; row ``b`` starts at global frame
``first_frame[b]``.  Rows b, b + 1 are neighbours when ``first_frame[b + 1] == first_frame[b] + stride`` -- then frames
``[stride, T)`` of b (its tail) and ``[0, ov)`` of b + 1 (its head) are the same frames -- and must otherwise be disjoint
(``first_frame[b + 1] >= first_frame[b] + T``).  On a shared frame f with right-window weight ``w[f]``:

    x0 = w[f] x0_right + (1 - w[f]) x0_left;    both rows take  x_prev = update(x_left, x0, noise_left / hist_left)

The update itself is ``dpm_solver_ref.update`` (mode 2) or the closed forms of p_sample / ddim_sample (modes 0 / 1):

    p_sample     x_prev = c1 x0 + c2 x + nonzero exp(0.5 log_var) noise
    ddim_sample  eps = (sqrt_recip x - x0) / sqrt_recipm1;  sigma = eta sqrt((1 - ab_prev) / (1 - ab)) sqrt(1 - ab / ab_prev)
                 x_prev = sqrt(ab_prev) x0 + sqrt(1 - ab_prev - sigma^2) eps + nonzero sigma noise
"""
import math

import numpy as np

import dpm_solver_ref as R


# ---- plan -------------------------------------------------------------------------------------------------------------------------
def plan_flags(first_frame, T, ov):
    """[(has a left neighbour, has a right neighbour)] per row; ValueError for a plan the rules refuse"""
    if not (isinstance(ov, (int, np.integer)) and 0 < 2 * ov <= T):
        raise ValueError(f'overlap {ov!r} outside 0 < 2 ov <= {T}')
    ff = [int(v) for v in first_frame]
    if not ff or any(v < 0 for v in ff):
        raise ValueError('first_frame: at least one entry, none negative')
    left, right = [False] * len(ff), [False] * len(ff)
    for b in range(len(ff) - 1):
        gap = ff[b + 1] - ff[b]
        if gap == T - ov:
            right[b], left[b + 1] = True, True
        elif gap < T:
            raise ValueError(f'rows {b}, {b + 1}: first frames {ff[b]}, {ff[b + 1]} neither neighbours nor disjoint')
    return list(zip(left, right))


def default_weights(ov):
    """w[f] = (f + 1) / (ov + 1), computed in fp64 and cast to fp32 (returned as the fp32 values in fp64)"""
    return ((np.arange(ov, dtype=np.float64) + 1.0) / (ov + 1.0)).astype(np.float32).astype(np.float64)


def seam_plan(total_frames, T, ov):
    """(windows, first frames, stitched length) of one sequence"""
    if not 0 < 2 * ov <= T:
        raise ValueError((T, ov))
    n = (total_frames - ov) // (T - ov)
    if n < 1:
        raise ValueError('shorter than one window')
    return n, [i * (T - ov) for i in range(n)], (n - 1) * (T - ov) + T


def gather_windows(z, first_frame, T):
    """z [frames, C] over the global frames -> [B, T, C]: equal on shared frames by construction"""
    return np.stack([np.asarray(z)[f:f + T] for f in first_frame])


def seams_equal(x, flags, ov):
    x = np.asarray(x)
    T = x.shape[1]
    return all(np.array_equal(x[b, T - ov:], x[b + 1, :ov]) for b, (_, r) in enumerate(flags) if r)


def seam_mask(flags, T, ov):
    """bool [B, T]: the frames that lie in two windows"""
    m = np.zeros((len(flags), T), dtype=bool)
    for b, (l, r) in enumerate(flags):
        m[b, :ov] |= l
        m[b, T - ov:] |= r
    return m


# ---- blend and step ---------------------------------------------------------------------------------------------------------------
def blend(x0, flags, ov, w=None):
    """per-window x0 [B, T, C] -> the shared x0: on a seam (1 - w) left + w right in both rows, elsewhere unchanged"""
    x0 = np.asarray(x0, dtype=np.float64)
    T = x0.shape[1]
    w = default_weights(ov) if w is None else np.asarray(w, dtype=np.float64)
    out = x0.copy()
    for b, (_, r) in enumerate(flags):
        if r:
            v = (1.0 - w)[:, None] * x0[b, T - ov:] + w[:, None] * x0[b + 1, :ov]
            out[b, T - ov:] = v
            out[b + 1, :ov] = v
    return out


def share_left(a, flags, ov):
    """the left row's values on every seam, in both rows (the noise / the history a seam element reads)"""
    a = np.array(a, dtype=np.float64)
    T = a.shape[1]
    for b, (_, r) in enumerate(flags):          # ascending: a middle row's head is overwritten before its tail is read -- they are disjoint
        if r:
            a[b + 1, :ov] = a[b, T - ov:]
    return a


def update(c, x, x0, noise=None, x0_prev=None):
    """one sampler update in fp64 from the fp32 fields of a StepCoefs-like ``c`` (mode 0 ddpm, 1 ddim, 2 multistep)"""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    if c.mode == 2:
        return R.update((float(c.c2), float(c.c1), float(c.eta)), x, x0, x0_prev)
    nz = np.asarray(noise, dtype=np.float64)
    if c.mode == 0:
        return float(c.c1) * x0 + float(c.c2) * x + float(c.nonzero) * math.exp(0.5 * float(c.log_var)) * nz
    ab, abp, eta = float(c.ab), float(c.ab_prev), float(c.eta)
    sigma = eta * math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)
    eps = (float(c.sqrt_recip) * x - x0) / float(c.sqrt_recipm1)
    return math.sqrt(abp) * x0 + math.sqrt(1 - abp - sigma * sigma) * eps + float(c.nonzero) * sigma * nz


def step(c, x, x0_windows, flags, ov, w=None, noise=None, x0_prev=None):
    """one coupled step: (x_prev, shared x0).  ``x`` is taken as it is (seam-consistent by precondition); the noise and the history are
    the left row's on a seam."""
    x0 = blend(x0_windows, flags, ov, w)
    nz = share_left(noise, flags, ov) if noise is not None else None
    hp = share_left(x0_prev, flags, ov) if (x0_prev is not None and c.mode == 2 and float(c.eta) != 0.0) else x0_prev
    return update(c, x, x0, nz, hp), x0

"""Edited rows (``mc_ctx_set_edit_rows``) per element in fp64: the kept region of every row on top of
``rowstep_ref.sampler_rows`` (imported, not restated).

Element e of row b with ``keep[e] != 0`` is given: ``x0 = gt`` (a select: whatever ``gt`` holds elsewhere, a NaN included, reaches no
output), then the row's own update of ``(x, x0)``; mode 1 replaces the new sample there by ``sqrt(ab_prev) gt + sqrt(1 - ab_prev) z2``
(``gaussian_diffusion.py:492-501`` and ``:855-877`` without the cross-fade); mode 2 stores the edited x0 as its history."""
import numpy as np

import rowstep_ref

DRAW_FLIP = 1 << 63          # the kept region's noise of a row is draw number (step draw ^ 2^63) of the row's seed


def edit_rows(x, a, b, noise, hist, gt, keep, gt_noise, coefs, TC):
    """flat arrays [B * TC]; element e takes ``coefs[e // TC]`` -> (x_prev, x0) in fp64.  ``gt_noise`` is read in mode 1 only, ``hist``
    in mode 2 where the row's eta != 0 (the caller stores x0 as the new history)."""
    x, a, b = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (x, a, b))
    keep = np.asarray(keep).reshape(-1) != 0
    gt = np.asarray(gt, dtype=np.float64).reshape(-1)
    x0 = np.where(keep, gt, a + b)
    assert np.isfinite(x0).all()
    out, _ = rowstep_ref.sampler_rows(x, x0, np.zeros_like(x0), noise, hist, coefs, TC)
    for r, c in enumerate(coefs):
        k = rowstep_ref.coefs_dict(c) if not isinstance(c, dict) else c
        if k['mode'] != 1:
            continue
        s = slice(r * TC, (r + 1) * TC)
        z2 = np.asarray(gt_noise, dtype=np.float64).reshape(-1)[s]
        with np.errstate(invalid='ignore'):
            kept = np.sqrt(k['ab_prev']) * gt[s] + np.sqrt(1 - k['ab_prev']) * z2
        out[s] = np.where(keep[s], kept, out[s])
    return out, x0

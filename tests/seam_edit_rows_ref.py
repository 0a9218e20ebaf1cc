"""fp64 restatement of the combined update (``mc_ctx_set_long_edits`` / ``sampler_seam_edit_rows_k``): kept regions
on seam-coupled rows, composed from ``seam_rows_ref`` (the blend, the owner's operands) and ``edit_ref`` (the select and the kept
region's update).  No arithmetic of its own: the order alone is stated here --

    x0m = blend(a + b)                      (section 4q: on a shared frame (1 - w) left + w right, in both rows)
    x0  = keep ? gt : x0m                   (section 4p: a select, after the blend)
    x_prev = the row's update of (x, x0);   mode 1, kept: sqrt(ab_prev) gt + sqrt(1 - ab_prev) z2;   mode 2: history <- x0

with the OWNER's (the left row's) keep / gt / noise / gt_noise / history entry on a shared element, in both rows."""
import numpy as np

import edit_ref
import seam_rows_ref as SR

DRAW_FLIP = edit_ref.DRAW_FLIP


def owner_tables(gt, keep, rows, ov):
    """the entries an output is computed from: the left row's on every shared frame, in both rows (``keep`` as bool)"""
    return SR.share_left(gt, rows, ov), SR.share_left(np.asarray(keep) != 0, rows, ov) != 0


def step(coefs, x, a, b, rows, ov, gt, keep, w=None, noise=None, hist=None, gt_noise=None):
    """one combined rows step in fp64 -> (x_prev [B, T, C], x0 [B, T, C]); ``coefs[b]`` the entry of row b (equal on both rows of a seam)"""
    x = np.asarray(x, dtype=np.float64)
    B, T, C = x.shape
    x0m = SR.blend(np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64), rows, ov, w)
    g, k = owner_tables(gt, keep, rows, ov)
    nz = SR.share_left(noise, rows, ov) if noise is not None else np.zeros_like(x)
    hp = SR.share_left(hist, rows, ov) if hist is not None else np.zeros_like(x)
    z2 = SR.share_left(gt_noise, rows, ov) if gt_noise is not None else np.zeros_like(x)
    out, x0 = edit_ref.edit_rows(x, x0m, np.zeros_like(x0m), nz, hp, g, k, z2, coefs, T * C)
    return out.reshape(B, T, C), x0.reshape(B, T, C)


def window_tables(gt, keep, first_frames, T):
    """a request-global edit (gt [n, C], keep [n, C]) cut into window rows: row j shows frames [first_frames[j], + T); frames past n free"""
    gt, keep = np.asarray(gt), np.asarray(keep) != 0
    n, C = gt.shape
    G = np.zeros((len(first_frames), T, C), dtype=gt.dtype)
    K = np.zeros((len(first_frames), T, C), dtype=bool)
    for j, f in enumerate(first_frames):
        m = max(0, min(n - f, T))
        G[j, :m], K[j, :m] = gt[f:f + m], keep[f:f + m]
    return G, K

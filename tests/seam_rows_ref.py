"""fp64 numpy restatement of the seam-coupled rows update (``mc_ctx_set_seam_rows`` / ``sampler_seam_rows_k``),
built on ``rowstep_ref`` (the per-row updates) and ``seam_ref`` (the blend weights, the closed forms).  Nothing here imports the package.

Row b of [B, T, C] shows global frames ``[first_frame[b], first_frame[b] + T)`` of its request; ``right[b]`` is the row holding the
request's next window -- ANY row -- or -1.  With ``stride = T - ov``: ``first_frame[right[b]] == first_frame[b] + stride``, so frames
``[stride, T)`` of b (its tail) are frames ``[0, ov)`` of right[b] (its head).  On a shared frame f

    x0 = w[f] x0_right + (1 - w[f]) x0_left;    both rows take  x_prev = update_{row b}(x_left, x0, noise_left / hist_left)

under the LEFT row's coefficients (the two rows of a seam carry equal ones).  Device noise: element r of row b in draw d is element
``first_frame[b] * C + r`` of the request's field ``philox_normal(n, seed[b], d)``."""
import numpy as np

import rowstep_ref
import seam_ref


def plan_rows(right, first_frame, T, ov):
    """[(right, has_left, first_frame)] per row; ValueError for a table the rules refuse"""
    if not (isinstance(ov, (int, np.integer)) and 0 < 2 * ov <= T):
        raise ValueError(f'overlap {ov!r} outside 0 < 2 ov <= {T}')
    right, ff = [int(v) for v in right], [int(v) for v in first_frame]
    B = len(right)
    if B < 1 or len(ff) != B:
        raise ValueError('right / first_frame: one entry per row')
    if any(v < 0 for v in ff):
        raise ValueError('first_frame: none negative')
    left = [False] * B
    for b, r in enumerate(right):
        if not -1 <= r < B or r == b:
            raise ValueError(f'right[{b}] = {r}')
        if r < 0:
            continue
        if left[r]:
            raise ValueError(f'row {r} is the right neighbour of two rows')
        left[r] = True
        if ff[r] != ff[b] + T - ov:
            raise ValueError(f'rows {b} -> {r}: first frames {ff[b]}, {ff[r]} not one stride apart')
    for b in range(B):
        n, v = 0, right[b]
        while v >= 0:
            n += 1
            if n >= B:
                raise ValueError(f'the chain from row {b} does not end')
            v = right[v]
    return [(right[b], left[b], ff[b]) for b in range(B)]


def pairs(rows):
    """[(left row, right row)] of every seam"""
    return [(b, r) for b, (r, _, _) in enumerate(rows) if r >= 0]


def seam_mask(rows, T, ov):
    """bool [B, T]: the frames that lie in two windows"""
    m = np.zeros((len(rows), T), dtype=bool)
    for b, (r, l, _) in enumerate(rows):
        m[b, :ov] |= l
        m[b, T - ov:] |= r >= 0
    return m


def blend(x0, rows, ov, w=None):
    """per-window x0 [B, T, C] -> the shared x0: on a seam (1 - w) left + w right in both rows, elsewhere unchanged"""
    x0 = np.asarray(x0, dtype=np.float64)
    T = x0.shape[1]
    w = seam_ref.default_weights(ov) if w is None else np.asarray(w, dtype=np.float64)
    if w.shape != (ov,) or (w < 0).any() or (w > 1).any():
        raise ValueError('weights: ov numbers in [0, 1]')
    out = x0.copy()
    for b, r in pairs(rows):
        v = (1.0 - w)[:, None] * x0[b, T - ov:] + w[:, None] * x0[r, :ov]
        out[b, T - ov:] = v
        out[r, :ov] = v
    return out


def share_left(a, rows, ov):
    """the left row's values on every seam, in both rows (a head is never a tail: the order of the copies does not matter)"""
    src = np.asarray(a, dtype=np.float64)
    out = src.copy()
    T = src.shape[1]
    for b, r in pairs(rows):
        out[r, :ov] = src[b, T - ov:]
    return out


def seams_equal(x, rows, ov):
    x = np.asarray(x)
    T = x.shape[1]
    return all(np.array_equal(x[b, T - ov:], x[r, :ov]) for b, r in pairs(rows))


def global_index(rows, T, C):
    """int64 [B, T C]: the index of every element in its request's field"""
    return np.stack([np.int64(ff) * np.int64(C) + np.arange(T * C, dtype=np.int64) for _, _, ff in rows])


def gather_field(field_of_row, rows, T, C):
    """field_of_row[b]: the request's field (flat, at least (first_frame[b] + T) C long) -> [B, T, C]"""
    return np.stack([np.asarray(field_of_row[b]).reshape(-1)[ff * C:(ff + T) * C].reshape(T, C) for b, (_, _, ff) in enumerate(rows)])


def step(coefs, x, a, b, rows, ov, w=None, noise=None, hist=None):
    """one coupled rows step in fp64: element e under ``coefs[e // (T C)]`` with x0 = a + b blended on the seams -> (x_prev, x0).  The
    noise and the history are the left row's on a seam; x is taken as it is (seam-consistent by precondition)."""
    x = np.asarray(x, dtype=np.float64)
    B, T, C = x.shape
    x0 = blend(np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64), rows, ov, w)
    nz = share_left(noise, rows, ov) if noise is not None else np.zeros_like(x)
    hp = share_left(hist, rows, ov) if hist is not None else np.zeros_like(x)
    out, _ = rowstep_ref.sampler_rows(x, x0, np.zeros_like(x0), nz, hp, coefs, T * C)
    return out.reshape(B, T, C), x0

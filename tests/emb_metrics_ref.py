"""Float64 references of the embedding-table metrics (``csrc/mc_embmetrics.hip`` / ``motioncraft_amd.embmetrics``).

(a) ``fid_nuclear``: the Frechet distance in its nuclear-norm form with ``np.linalg.svd`` (LAPACK) -- the oracle:
        |mu1 - mu2|^2 + |A_c|_F^2 / (n - 1) + |B_c|_F^2 / (m - 1) - 2 |A_c B_c^T|_* / sqrt((n - 1)(m - 1)).
(b) ``fid_jacobi``: the kernel's algorithm restated in numpy: the same factors, the same one-sided Jacobi (round-robin pair order,
    skip rule, floor, sweep logic), the pairs of a round at once.  It differs from the device in summation order and in fused
    multiply-adds only.
(c) direct-difference restatements of the rank rule, the matching sum, the z-score and the pair distances.
"""
import numpy as np

MAX_SWEEPS = 30
EPS = np.finfo(np.float64).eps


class NoConvergence(RuntimeError):
    pass


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def centred(table, emb_scale=1.0):
    a = np.asarray(table, dtype=np.float64)
    mu = a.mean(axis=0)
    return mu * emb_scale, (a - mu) * emb_scale


def fid_terms(gt, pred, emb_scale=1.0):
    """(|dmu|^2, Tr C1, Tr C2, Tr sqrt(C1 C2)) with LAPACK singular values"""
    mu1, a = centred(gt, emb_scale)
    mu2, b = centred(pred, emb_scale)
    n, m = a.shape[0], b.shape[0]
    nuc = np.linalg.svd(a @ b.T, compute_uv=False).sum()
    return float((mu1 - mu2) @ (mu1 - mu2)), float((a * a).sum() / (n - 1)), float((b * b).sum() / (m - 1)), float(nuc / np.sqrt((n - 1) * (m - 1)))


def fid_nuclear(gt, pred, emb_scale=1.0):
    dm, t1, t2, root = fid_terms(gt, pred, emb_scale)
    return dm + t1 + t2 - 2 * root


def fid_scale(gt, pred, emb_scale=1.0):
    """s = |dmu|^2 + Tr C1 + Tr C2: what the bands are relative to"""
    dm, t1, t2, _ = fid_terms(gt, pred, emb_scale)
    return dm + t1 + t2


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def rr_pairs(c):
    """the rounds of the kernel's round-robin over c columns: a list of (p, q) index arrays, p < q, the bye's pair left out"""
    m = c + (c & 1)
    rounds = []
    for k in range(m - 1):
        i = np.arange(m // 2)
        a = np.where(i == 0, m - 1, (k + i) % (m - 1))
        b = np.where(i == 0, k, (k - i + (m - 1)) % (m - 1))
        p, q = np.minimum(a, b), np.maximum(a, b)
        keep = q < c
        rounds.append((p[keep], q[keep]))
    return rounds


def jacobi(W, r, max_sweeps=MAX_SWEEPS):
    """One-sided Jacobi in place on the columns of W [rtot, c] (the first r rows are the data, the rest rides along).
    Returns the number of sweeps; raises NoConvergence at the cap."""
    c = W.shape[1]
    T = np.ascontiguousarray(W.T)                       # one column per row: the pairs of a round are gathered as rows
    norm2 = np.einsum('ij,ij->i', T[:, :r], T[:, :r])
    floor2 = np.ldexp(norm2.max(), -1000) if c else 0.0
    if c < 2:
        return 0
    tol = EPS * np.sqrt(r)
    rounds = rr_pairs(c)
    for sweep in range(max_sweeps):
        rotated = 0
        for p, q in rounds:
            x, y = T[p], T[q]
            xr, yr = x[:, :r], y[:, :r]
            al, be, ga = np.einsum('ij,ij->i', xr, xr), np.einsum('ij,ij->i', yr, yr), np.einsum('ij,ij->i', xr, yr)
            go = ~((al <= floor2) | (be <= floor2) | ~(np.abs(ga) > tol * (np.sqrt(al) * np.sqrt(be))))
            if not go.any():
                continue
            rotated += int(go.sum())
            with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
                z = (be - al) / (2.0 * ga)
                t = np.where(z >= 0, 1.0, -1.0) / (np.abs(z) + np.sqrt(1.0 + z * z))
                cs = 1.0 / np.sqrt(1.0 + t * t)
                sn = cs * t
            cs, sn = np.where(go, cs, 1.0)[:, None], np.where(go, sn, 0.0)[:, None]
            T[p], T[q] = cs * x - sn * y, sn * x + cs * y
        if rotated == 0:
            W[:] = T.T
            return sweep + 1
    raise NoConvergence(f'{c} columns of {r} rows still rotated pairs in sweep {max_sweeps}')


def factor(table, emb_scale=1.0, max_sweeps=MAX_SWEEPS):
    """(mean, Tr C * (n - 1), F [d, min(n, d)]) with F^T F' carrying the singular values of A_c A'_c^T"""
    mu, a = centred(table, emb_scale)
    n, d = a.shape
    if n >= d:
        W = np.concatenate([a, np.eye(d)], axis=0)
        trace = (a * a).sum(axis=0).sum()
        jacobi(W, n, max_sweeps)
        return mu, trace, W[n:] * np.sqrt((W[:n] * W[:n]).sum(axis=0))
    W = np.ascontiguousarray(a.T)
    trace = (W * W).sum(axis=0).sum()
    jacobi(W, d, max_sweeps)
    return mu, trace, W


def fid_jacobi(gt, pred, emb_scale=1.0, max_sweeps=MAX_SWEEPS):
    n, m = np.shape(gt)[0], np.shape(pred)[0]
    mu1, tr1, f1 = factor(gt, emb_scale, max_sweeps)
    mu2, tr2, f2 = factor(pred, emb_scale, max_sweeps)
    rows, cols = (f1, f2) if f1.shape[1] >= f2.shape[1] else (f2, f1)
    K = rows.T @ cols
    jacobi(K, K.shape[0], max_sweeps)
    nuc = 0.0
    for s in np.sqrt((K * K).sum(axis=0)):
        nuc += s
    dmu = mu1 - mu2
    return float(dmu @ dmu + tr1 / (n - 1) + tr2 / (m - 1) - 2.0 * nuc / np.sqrt(float(n - 1) * float(m - 1)))


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def distances(text, motion):
    t, m = np.asarray(text, dtype=np.float64), np.asarray(motion, dtype=np.float64)
    return np.sqrt(((t[:, None, :] - m[None, :, :]) ** 2).sum(axis=2))


def ranks(text, motion):
    """rank_i = #{j : dist(t_i, m_j) < dist(t_i, m_i)} + #{j < i : dist(t_i, m_j) = dist(t_i, m_i)}"""
    dist = distances(text, motion)
    own = np.diagonal(dist)[:, None]
    before = np.arange(dist.shape[0])[None, :] < np.arange(dist.shape[0])[:, None]
    return (dist < own).sum(axis=1) + ((dist == own) & before).sum(axis=1)


def batches(n, batch):
    return [slice(b, min(b + batch, n)) for b in range(0, n, batch)]


def r_precision_counts(text, motion, batch, top_k):
    """int [batches, top_k]: per batch the rows whose rank is below k, k = 1..top_k"""
    return np.array([[(ranks(text[s], motion[s]) < k).sum() for k in range(1, top_k + 1)] for s in batches(len(text), batch)])


def matching_sums(text, motion, batch):
    return np.array([np.diagonal(distances(text[s], motion[s])).sum() for s in batches(len(text), batch)])


def zscore(table):
    e = np.asarray(table, dtype=np.float64)
    sd = np.std(e, axis=0)
    sd[sd == 0] = 1e-8
    return (e - e.mean(axis=0)) / sd


def pair_distance(table, first, second, emb_scale=1.0, norm_scale=1.0):
    """table [groups, rows, d] (or [rows, d]): the mean over groups and pairs of |(a[g, f] - a[g, s]) * norm_scale|, a = table * emb_scale"""
    a = np.asarray(table, dtype=np.float64)
    a = (a if a.ndim == 3 else a[None]) * emb_scale
    return float(np.sqrt((((a[:, first] - a[:, second]) * norm_scale) ** 2).sum(axis=2)).mean())


# ---- the three families of tables --------------------------------------------------------------------------------------------
def dense_mixed(n, d, seed, shift=0.0):
    """random rows mixed by a dense d x d matrix: full rank when n - 1 >= d, rank n - 1 otherwise"""
    rs = np.random.RandomState(seed)
    return (rs.randn(n, d) @ (rs.randn(d, d) / np.sqrt(d)) + shift * rs.randn(d)).astype(np.float32)


def decaying(n, d, seed, ratio=0.7):
    """singular spectrum ratio^i in a random orthogonal basis"""
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.randn(d, d))
    return ((rs.randn(n, d) * ratio ** np.arange(d)) @ q.T + 0.1 * rs.randn(d)).astype(np.float32)

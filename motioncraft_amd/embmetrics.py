"""The metric functions of ``mogen/core/evaluation/utils.py`` over embedding tables that stay on the device
(``mc_emb_*``, ``csrc/mc_embmetrics.hip``): the Frechet distance in its nuclear-norm form (three one-sided Jacobi decompositions, no
covariance and no matrix root), mean / covariance, the z-score, R precision counts and the matching-score sum from direct
differences, and the gathered pair distances of diversity and multimodality.

Tables are float32 or float64 device tensors [rows, d]; every result is float64, computed in a fixed order: two runs give the same
bits.  ``diversity`` and ``multimodality`` take the arguments of the host functions of ``evaluation`` and draw their indices with the
same ``np.random.choice`` calls in the same order, so the global generator advances exactly as it does there.

Nothing here falls back to the host: a missing library or GPU is an error.
"""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _p, stream as _stream

MAX_DIM, MAX_ROWS, MAX_BATCH, MAX_TOPK, MAX_SWEEPS = (_lib.CONSTANTS[f'MC_EMB_MAX_{n}'] for n in ('DIM', 'ROWS', 'BATCH', 'TOPK', 'SWEEPS'))


class NoConvergence(RuntimeError):
    """a Jacobi decomposition still rotated column pairs in its last allowed sweep (``MC_ERR_NOCONV``)"""


def _table(t, name, ndim=2):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f'{name} must be a device tensor')
    if t.dim() != ndim:
        raise ValueError(f'{name} must have {ndim} dimensions, got {tuple(t.shape)}')
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float32)
    if not 1 <= t.shape[-1] <= MAX_DIM:
        raise ValueError(f'{name}: {t.shape[-1]} columns (1..{MAX_DIM})')
    return t.detach().contiguous()


def _both(a, b, names):
    a = _table(a, names[0])
    b = _table(b, names[1])
    if a.dtype != b.dtype:                       # one of each: the wider one decides (the conversion is exact)
        a, b = a.to(torch.float64), b.to(torch.float64)
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError(f'{names[0]} {tuple(a.shape)} and {names[1]} {tuple(b.shape)} must share their width and device')
    return a, b


def _f64(t):
    return int(t.dtype == torch.float64)


def _work(nbytes, device):
    return torch.empty(max(1, (nbytes + 7) // 8), device=device, dtype=torch.float64)


def frechet_distance(gt_emb, pred_emb, emb_scale=1.0, max_sweeps=0, return_info=False):
    """``calculate_frechet_distance`` of the statistics of ``gt_emb * emb_scale`` [n, d] and ``pred_emb * emb_scale`` [m, d], as a
    float64 device tensor [1].  The value is the exact one for positive semi-definite covariances, also for n - 1 < d, where
    ``scipy.linalg.sqrtm`` is off by its own rounding band.  The call waits for the stream once per Jacobi sweep.
    ``max_sweeps``: the cap per decomposition (0: ``MAX_SWEEPS``); ``NoConvergence`` when it is reached.  ``return_info``: also
    ``dict(sweeps=(gt, pred, product), launches=(...))``."""
    gt, pred = _both(gt_emb, pred_emb, ('gt_emb', 'pred_emb'))
    lib = _lib.load(require_gpu=True)
    n, m, d = gt.shape[0], pred.shape[0], gt.shape[1]
    wb = int(lib.mc_emb_frechet_work_bytes(n, m, d))
    if wb < 0:
        raise ValueError(f'tables [{n}, {d}] and [{m}, {d}]: 2..{MAX_ROWS} rows of 1..{MAX_DIM} columns each')
    if not 0 <= int(max_sweeps) <= MAX_SWEEPS:
        raise ValueError(f'max_sweeps={max_sweeps}: 0 (the cap) or 1..{MAX_SWEEPS}')
    with torch.cuda.device(gt.device):
        work, out = _work(wb, gt.device), torch.empty(1, device=gt.device, dtype=torch.float64)
        info = (ctypes.c_int32 * 6)()
        rc = lib.mc_emb_frechet(_p(gt), n, _p(pred), m, d, _f64(gt), float(emb_scale), int(max_sweeps), _p(work), work.numel() * 8, _p(out), info, _stream())
    if rc == _lib.MC_ERR_NOCONV:
        raise NoConvergence(_lib.last_error())
    _lib.check(rc, 'mc_emb_frechet')
    return (out, dict(sweeps=tuple(info[0::2]), launches=tuple(info[1::2]))) if return_info else out


def activation_statistics(emb, emb_scale=1.0):
    """``calculate_activation_statistics``: (mean [d], covariance [d, d]) of ``emb * emb_scale``, float64 device tensors."""
    a = _table(emb, 'emb')
    lib = _lib.load(require_gpu=True)
    n, d = a.shape
    wb = int(lib.mc_emb_statistics_work_bytes(n, d))
    if wb < 0:
        raise ValueError(f'table [{n}, {d}]: 2..{MAX_ROWS} rows of 1..{MAX_DIM} columns')
    with torch.cuda.device(a.device):
        work = _work(wb, a.device)
        mean, cov = torch.empty(d, device=a.device, dtype=torch.float64), torch.empty(d, d, device=a.device, dtype=torch.float64)
        _lib.check(lib.mc_emb_statistics(_p(a), n, d, _f64(a), float(emb_scale), _p(work), work.numel() * 8, _p(mean), _p(cov), _stream()), 'mc_emb_statistics')
    return mean, cov


def zscore(emb):
    """``evaluation._zscore``: (x - column mean) / population deviation, a zero deviation replaced by 1e-8; float64 [n, d]."""
    a = _table(emb, 'emb')
    lib = _lib.load(require_gpu=True)
    if not 1 <= a.shape[0] <= MAX_ROWS:
        raise ValueError(f'table {tuple(a.shape)}: 1..{MAX_ROWS} rows')
    with torch.cuda.device(a.device):
        out = torch.empty(a.shape, device=a.device, dtype=torch.float64)
        _lib.check(lib.mc_emb_zscore(_p(a), a.shape[0], a.shape[1], _f64(a), _p(out), _stream()), 'mc_emb_zscore')
    return out


def _retrieval(text_emb, motion_emb, batch_size, top_k, with_sum):
    t, m = _both(text_emb, motion_emb, ('text_emb', 'motion_emb'))
    if t.shape != m.shape or not 1 <= t.shape[0] <= MAX_ROWS:
        raise ValueError(f'text_emb {tuple(t.shape)} and motion_emb {tuple(m.shape)} must pair row by row (1..{MAX_ROWS} rows)')
    n = t.shape[0]
    batch = n if batch_size is None else int(batch_size)
    if not 1 <= batch <= MAX_BATCH:
        raise ValueError(f'batch_size={batch}: 1..{MAX_BATCH}')
    if not 1 <= int(top_k) <= MAX_TOPK:
        raise ValueError(f'top_k={top_k}: 1..{MAX_TOPK}')
    lib = _lib.load(require_gpu=True)
    nb = -(-n // batch)
    with torch.cuda.device(t.device):
        counts = torch.empty(nb, int(top_k), device=t.device, dtype=torch.int32)
        sums = torch.empty(nb, device=t.device, dtype=torch.float64) if with_sum else None
        _lib.check(lib.mc_emb_retrieval(_p(t), _p(m), n, t.shape[1], _f64(t), batch, int(top_k), _p(counts), _p(sums), _stream()), 'mc_emb_retrieval')
    return counts, sums


def r_precision_counts(text_emb, motion_emb, top_k=3, batch_size=None):
    """Rows [n, d] paired one to one, cut into batches of ``batch_size`` (None: one batch; at most ``MAX_BATCH``; the last one may be
    short) -> int32 device tensor [batches, top_k]: per batch the rows whose own motion is among the k nearest, k = 1..top_k, under
    rank_i = #{j : dist(t_i, m_j) < dist(t_i, m_i)} + #{j < i : equal}.  Distances come from direct differences in float64."""
    return _retrieval(text_emb, motion_emb, batch_size, top_k, False)[0]


def matching_score_sum(text_emb, motion_emb, batch_size=None):
    """float64 device tensor [batches]: per batch the sum over its rows of dist(t_i, m_i).  The tables are taken as they are:
    the matching score of the reference is this sum over ``zscore``d batches."""
    return _retrieval(text_emb, motion_emb, batch_size, 1, True)[1]


def _pair_distance(table, first, second, emb_scale, norm_scale):
    lib = _lib.load(require_gpu=True)
    groups, rows, d = table.shape
    with torch.cuda.device(table.device):
        idx = torch.from_numpy(np.stack([first, second]).astype(np.int32)).to(table.device)
        out = torch.empty(1, device=table.device, dtype=torch.float64)
        _lib.check(lib.mc_emb_pair_distance(_p(table), groups, rows, d, _f64(table), _p(idx[0]), _p(idx[1]), idx.shape[1], float(emb_scale), float(norm_scale),
                                            _p(out), _stream()), 'mc_emb_pair_distance')
    return out


def diversity(activation, diversity_times, emb_scale=1.0, norm_scale=1.0):
    """``calculate_diversity``: two ``np.random.choice(n, diversity_times, replace=False)`` draws from the global generator, then
    the mean of |(a[first] - a[second]) * norm_scale| with a = activation * emb_scale; float64 device tensor [1]."""
    a = _table(activation, 'activation')
    if not a.shape[0] > diversity_times >= 1:
        raise ValueError(f'{a.shape[0]} rows must exceed diversity_times={diversity_times} (>= 1)')
    first = np.random.choice(a.shape[0], diversity_times, replace=False)
    second = np.random.choice(a.shape[0], diversity_times, replace=False)
    return _pair_distance(a[None], first, second, emb_scale, norm_scale)


def multimodality(activation, multimodality_times):
    """``calculate_multimodality``: activation [num_sentences, num_repeats, d]; the two draws over the repeats, then the mean over
    sentences and pairs of |a[:, first] - a[:, second]|; float64 device tensor [1]."""
    a = _table(activation, 'activation', ndim=3)
    if not a.shape[1] > multimodality_times >= 1:
        raise ValueError(f'{a.shape[1]} repeats must exceed multimodality_times={multimodality_times} (>= 1)')
    first = np.random.choice(a.shape[1], multimodality_times, replace=False)
    second = np.random.choice(a.shape[1], multimodality_times, replace=False)
    return _pair_distance(a, first, second, 1.0, 1.0)

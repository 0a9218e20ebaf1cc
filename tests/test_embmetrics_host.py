"""CPU: the references of the embedding-table metrics (``emb_metrics_ref.py``) against each other and against the host functions
of ``evaluation``, the exports, and that the host path of the evaluators is the path of before.

Nothing here can fail because of a kernel.  The two bands are printed and asserted only loosely; with
s = |dmu|^2 + Tr C1 + Tr C2,
    band_alg = |fid_jacobi - fid_nuclear| / s      the one-sided Jacobi algorithm's own error (restatement (b) against oracle (a))
    band_ref = |sqrtm route - fid_nuclear| / s     the reference method's own error (``calculate_frechet_distance`` on fp64 inputs)
``bands(tag)`` is what the GPU tests take their tolerance from.
"""
import functools

import numpy as np
import pytest
import torch

import emb_metrics_ref as R
from motioncraft_amd import evaluation as E, lib as L

EPS = np.finfo(np.float64).eps
NEW_SYMBOLS = ('mc_emb_frechet_work_bytes', 'mc_emb_frechet', 'mc_emb_statistics_work_bytes', 'mc_emb_statistics', 'mc_emb_zscore', 'mc_emb_retrieval',
               'mc_emb_pair_distance')
# tag: (family, n, m, d); the second table is shifted so that |dmu|^2 takes part
FID_CASES = {
    'n2_m2_d1': ('dense', 2, 2, 1), 'n3_m5_d2': ('dense', 3, 5, 2), 'n5_m4_d3': ('dense', 5, 4, 3), 'n40_m43_d33': ('dense', 40, 43, 33),
    'n200_m203_d64': ('dense', 200, 203, 64), 'n24_m27_d256': ('dense', 24, 27, 256), 'n300_m303_d256': ('dense', 300, 303, 256),
    'n64_m67_d512': ('dense', 64, 67, 512), 'identical_n40_d33': ('identical', 40, 40, 33), 'repeated_row_n20_m43_d33': ('repeated', 20, 43, 33),
    'decaying_n600_m603_d64': ('decaying', 600, 603, 64),
}
FAMILIES = ('n200_m203_d64', 'n24_m27_d256', 'decaying_n600_m603_d64')           # full rank, n - 1 < d, decaying spectrum


@functools.lru_cache(maxsize=None)
def fid_tables(tag):
    """(gt, pred) float32 tables of a case"""
    family, n, m, d = FID_CASES[tag]
    seed = 100 + 2 * list(FID_CASES).index(tag)
    if family == 'decaying':
        return R.decaying(n, d, seed), R.decaying(m, d, seed + 1)
    gt, pred = R.dense_mixed(n, d, seed), R.dense_mixed(m, d, seed + 1, shift=0.3)
    if family == 'identical':
        pred = gt.copy()
    if family == 'repeated':
        gt = np.repeat(gt[:1], n, axis=0)
    return gt, pred


def host_fid(gt, pred, emb_scale=1.0):
    """the reference's method on fp64 inputs"""
    g, p = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    return float(E.calculate_frechet_distance(*E.calculate_activation_statistics(g, emb_scale), *E.calculate_activation_statistics(p, emb_scale)))


def bands_of(gt, pred, emb_scale=1.0):
    a, s = R.fid_nuclear(gt, pred, emb_scale), R.fid_scale(gt, pred, emb_scale)
    return dict(oracle=a, scale=s, band_alg=abs(R.fid_jacobi(gt, pred, emb_scale) - a) / s, band_ref=abs(host_fid(gt, pred, emb_scale) - a) / s)


@functools.lru_cache(maxsize=None)
def bands(tag):
    return bands_of(*fid_tables(tag))


def fid_tolerance(b):
    """|device - oracle| may reach 4 band_alg s.  A band below one spacing of the doubles near s is no measurement of the algorithm
    (it is 0 where (b) and (a) happen to round alike, and the last subtraction of the distance alone rounds by up to eps s / 2), so
    the band counts as at least eps."""
    return 4 * max(b['band_alg'], EPS) * b['scale']


def test_exports_and_work_bytes():
    lib = L.load(require_gpu=False)
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    import motioncraft_amd
    from motioncraft_amd import embmetrics
    assert motioncraft_amd.embmetrics is embmetrics and 'embmetrics' in motioncraft_amd.__all__
    for name in ('frechet_distance', 'activation_statistics', 'zscore', 'r_precision_counts', 'matching_score_sum', 'diversity', 'multimodality'):
        assert callable(getattr(embmetrics, name)), name
    assert L.MC_EMB_MAX_DIM >= 512 and L.MC_EMB_MAX_SWEEPS == embmetrics.MAX_SWEEPS == R.MAX_SWEEPS and L.MC_ERR_NOCONV not in (L.MC_OK, L.MC_ERR_ARG, L.MC_ERR_HIP)
    # tall table: (n + d) d + d + 2 d + 1 doubles; short: d n + d + 2 n + 1; the product, its norms, the floor and the counter
    assert lib.mc_emb_frechet_work_bytes(300, 24, 256) == 8 * ((556 * 256 + 3 * 256 + 1) + (256 * 24 + 256 + 48 + 1) + 256 * 24 + 24 + 2)
    assert lib.mc_emb_statistics_work_bytes(40, 33) == 8 * 40 * 33
    for bad in ((1, 3, 2), (3, 1, 2), (3, 3, 0), (3, 3, L.MC_EMB_MAX_DIM + 1), (L.MC_EMB_MAX_ROWS + 1, 3, 2)):
        assert lib.mc_emb_frechet_work_bytes(*bad) == -1, bad
    assert lib.mc_emb_statistics_work_bytes(1, 4) == -1 and lib.mc_emb_statistics_work_bytes(4, L.MC_EMB_MAX_DIM + 1) == -1


def test_null_arguments_are_refused_before_anything_runs():
    lib = L.load(require_gpu=False)
    assert lib.mc_emb_frechet(None, 3, None, 3, 2, 0, 1.0, 0, None, 0, None, None, None) == L.MC_ERR_ARG and 'null' in L.last_error()
    assert lib.mc_emb_statistics(None, 3, 2, 0, 1.0, None, 0, None, None, None) == L.MC_ERR_ARG
    assert lib.mc_emb_zscore(None, 3, 2, 0, None, None) == L.MC_ERR_ARG
    assert lib.mc_emb_retrieval(None, None, 3, 2, 0, 3, 1, None, None, None) == L.MC_ERR_ARG
    assert lib.mc_emb_pair_distance(None, 1, 3, 2, 0, None, None, 2, 1.0, 1.0, None, None) == L.MC_ERR_ARG


def test_round_robin_meets_every_pair_once_per_sweep():
    for c in (2, 3, 4, 5, 24, 33, 64):
        rounds = R.rr_pairs(c)
        assert len(rounds) == c + (c & 1) - 1
        seen = []
        for p, q in rounds:
            both = np.concatenate([p, q])
            assert len(set(both.tolist())) == both.size and (p < q).all() and q.max(initial=0) < c        # disjoint within a round
            seen += list(zip(p.tolist(), q.tolist()))
        assert sorted(seen) == [(i, j) for i in range(c) for j in range(i + 1, c)]


def test_jacobi_singular_values_and_zero_columns():
    rs = np.random.RandomState(3)
    W = rs.randn(40, 7)
    W[:, 2] = 0.0                                                         # a zero column is skipped, not divided by
    W[:, 5] = W[:, 1]                                                     # a repeated one rotates to zero
    want = np.linalg.svd(W, compute_uv=False)
    full = np.concatenate([W, np.eye(7)])
    sweeps = R.jacobi(full, 40)
    got = np.sort(np.sqrt((full[:40] ** 2).sum(axis=0)))[::-1]
    assert np.isfinite(full).all() and 1 <= sweeps < R.MAX_SWEEPS
    assert np.abs(got - want).max() <= 64 * EPS * want[0]
    assert np.abs(W @ full[40:] - full[:40]).max() <= 64 * EPS * want[0]             # the identity block became V
    with pytest.raises(R.NoConvergence):
        R.jacobi(rs.randn(40, 7), 40, max_sweeps=1)


@pytest.mark.parametrize('tag', FAMILIES)
def test_bands_of_the_algorithm_and_of_the_reference_method(tag):
    gt, pred = fid_tables(tag)
    b = bands(tag)
    print(f'{tag}: oracle {b["oracle"]!r} s {b["scale"]:.6g} band_alg {b["band_alg"]:.2e} band_ref {b["band_ref"]:.2e}')
    # the scipy route stays finite and inside calculate_frechet_distance's own imaginary check: it returned a number
    assert np.isfinite(host_fid(gt, pred))
    from scipy import linalg
    c1, c2 = (np.cov(np.asarray(t, dtype=np.float64), rowvar=False) for t in (gt, pred))
    root, _ = linalg.sqrtm(c1.dot(c2), disp=False)
    imag = float(np.abs(np.diagonal(root).imag).max()) if np.iscomplexobj(root) else 0.0
    print(f'    sqrtm: {"complex" if np.iscomplexobj(root) else "real"} root, largest diagonal imaginary part {imag:.1e}')
    assert np.isfinite(root).all() and imag <= 1e-3
    assert b['band_alg'] <= 1e-11 and b['band_ref'] <= 1e-5                # loose: the measured values are in DESIGN.md


def test_emb_scale_enters_both_forms_alike():
    gt, pred = fid_tables('n40_m43_d33')
    a = R.fid_nuclear(gt, pred, 0.5)
    assert abs(a - 0.25 * R.fid_nuclear(gt, pred)) <= 1e-12 * abs(a) and abs(R.fid_jacobi(gt, pred, 0.5) - a) <= 1e-11 * R.fid_scale(gt, pred, 0.5)
    assert abs(host_fid(gt, pred, 0.5) - a) <= 1e-9 * R.fid_scale(gt, pred, 0.5)


def test_direct_difference_restatements_vs_the_host_functions():
    rs = np.random.RandomState(5)
    text = rs.randn(39, 33)
    motion = text + 0.9 * rs.randn(39, 33)
    dist = E.euclidean_distance_matrix(text, motion)
    assert np.abs(R.distances(text, motion) - dist).max() <= 1e-12 * dist.max()
    for s in R.batches(39, 32):
        want = E.calculate_top_k(np.argsort(E.euclidean_distance_matrix(text[s], motion[s]), axis=1), 3).sum(axis=0)
        assert np.array_equal(R.r_precision_counts(text[s], motion[s], 32, 3)[0], want)
    assert [(s.start, s.stop) for s in R.batches(39, 32)] == [(0, 32), (32, 39)]
    z = R.zscore(np.concatenate([text, np.full((39, 1), 2.5)], axis=1))
    assert np.array_equal(z, E._zscore(np.concatenate([text, np.full((39, 1), 2.5)], axis=1))) and (z[:, -1] == 0).all()
    want = E.euclidean_distance_matrix(E._zscore(text), E._zscore(motion)).trace()
    assert abs(R.matching_sums(R.zscore(text), R.zscore(motion), 64)[0] - want) <= 1e-12 * want
    np.random.seed(11)
    want = E.calculate_diversity(text, 10, 0.5, 2.0)
    np.random.seed(11)
    first, second = np.random.choice(39, 10, replace=False), np.random.choice(39, 10, replace=False)
    assert abs(R.pair_distance(text, first, second, 0.5, 2.0) - want) <= 1e-14 * want
    act = rs.randn(3, 7, 33)
    np.random.seed(12)
    want = E.calculate_multimodality(act, 4)
    np.random.seed(12)
    first, second = np.random.choice(7, 4, replace=False), np.random.choice(7, 4, replace=False)
    assert abs(R.pair_distance(act, first, second) - want) <= 1e-14 * want


# ---- the evaluators: a stub embedding model, shared with the GPU tests -----------------------------------------------------------------
class Tracked(torch.Tensor):
    """an embedding that counts its copies to the host"""
    transfers = 0

    def cpu(self, *args, **kwargs):
        Tracked.transfers += 1
        return super().cpu(*args, **kwargs).as_subclass(torch.Tensor)


class StubModel:
    """Fixed embeddings: a motion's is tanh(its time mean, projected), a text's the row of a table its string names.  float64, so
    that the host path's arithmetic is float64 throughout and its error is the band measured above."""

    def __init__(self, device, width, channels, n_text, seed=21):
        g = torch.Generator().manual_seed(seed)
        self.device = device
        self.proj = torch.randn(channels, width, generator=g, dtype=torch.float64).to(device)
        self.text = torch.randn(n_text, width, generator=g, dtype=torch.float64).to(device)

    def encode_motion(self, motion, motion_length=None, motion_mask=None, device=None):
        return torch.tanh(motion.to(self.device, torch.float64).mean(dim=1) @ self.proj).as_subclass(Tracked)

    def encode_text(self, text, token=None, device=None):
        return self.text[[int(t) for t in text]].as_subclass(Tracked)


def stub_results(n, extra, frames=4, channels=6, seed=22):
    """n paired results and `extra` more (the repeats MultiModality appends); the sample follows its text's row loosely"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n + extra):
        gt = torch.randn(frames, channels, generator=g)
        out.append(dict(motion=gt, pred_motion=gt + 0.7 * torch.randn(frames, channels, generator=g), motion_mask=torch.ones(frames),
                        pred_motion_mask=torch.ones(frames), motion_length=torch.tensor(frames), pred_motion_length=torch.tensor(frames),
                        text=str(i % n)))
    return out


EVALUATOR_CFGS = (dict(type='R Precision', batch_size=32, top_k=3), dict(type='Matching Score', batch_size=32), dict(type='FID', emb_scale=0.5),
                  dict(type='Diversity', num_samples=10, emb_scale=0.5, norm_scale=2.0),
                  dict(type='MultiModality', num_samples=3, num_repeats=5, num_picks=2))


def run_evaluators(model, results, n, on_device, seed=31):
    """the five evaluators in turn from one seed -> (their numbers, the state of the global generator afterwards)"""
    np.random.seed(seed)
    out = {}
    for metric in EVALUATOR_CFGS:
        cfg = dict(evaluator_model=model, replication_times=1, on_device=on_device)
        ev, _ = E.build_evaluator(metric, cfg, n, [np.arange(n)])
        assert ev.on_device is on_device
        out.update(ev.evaluate(results if metric['type'] == 'MultiModality' else results[:n]))
    return out, np.random.get_state()


def test_host_evaluators_are_the_path_of_before():
    """on_device=False (the default) from the same inputs and seed: the numbers of the metric functions applied by hand, exactly"""
    n = 39
    model, results = StubModel('cpu', 12, 6, n), stub_results(n, 15)
    Tracked.transfers = 0
    got, _ = run_evaluators(model, results, n, False)
    assert Tracked.transfers > 0
    assert E.BaseEvaluator().on_device is False and E.FIDEvaluator(data_len=n).on_device is False
    stack = lambda key, part: torch.stack([r[key] for r in part])
    pred, gt = (model.encode_motion(stack(k, results[:n])).as_subclass(torch.Tensor).numpy() for k in ('pred_motion', 'motion'))
    text = model.text.numpy()
    counts, match = np.zeros(3), 0.0
    for s in R.batches(n, 32):
        counts += E.calculate_top_k(np.argsort(E.euclidean_distance_matrix(text[s], pred[s]), axis=1), 3).sum(axis=0)
        match += E.euclidean_distance_matrix(E._zscore(text[s]), E._zscore(pred[s])).trace()
    fid = E.calculate_frechet_distance(*E.calculate_activation_statistics(E._zscore(gt), 0.5), *E.calculate_activation_statistics(E._zscore(pred), 0.5))
    np.random.seed(31)                                                    # the draws in the order of the metrics: diversity, then
    div = E.calculate_diversity(pred, 10, 0.5, 2.0)                       # MultiModalityEvaluator's sentences, then its picks
    assert np.random.choice(n, 3).shape == (3,)
    mm_emb = model.encode_motion(stack('pred_motion', results[n:])).as_subclass(torch.Tensor).numpy().reshape(3, 5, -1)
    mm = E.calculate_multimodality(mm_emb, 2)
    for k in range(3):
        assert got['R_precision Top %d (mean)' % (k + 1)] == counts[k] / n
    assert got['Matching Score (mean)'] == match / n and got['FID (mean)'] == fid and got['Diversity (mean)'] == div and got['MultiModality (mean)'] == mm

"""On the MI355X: ``motioncraft_amd.embmetrics`` (``mc_emb_*``, ``csrc/mc_embmetrics.hip``) and the ``on_device`` paths built on it.

Bounds.
  * Frechet distance vs oracle (a) of ``emb_metrics_ref.py``: ``4 * band_alg * s`` for the same case, band_alg = |(b) - (a)| / s
    computed here from the numpy restatement (b) of the kernel's algorithm, s = |dmu|^2 + Tr C1 + Tr C2; the device differs from
    (b) in fused multiply-adds and the shape of the reduction trees only, which change the rounding and not its scale.  A band
    below eps counts as eps (``test_embmetrics_host.fid_tolerance``).  And no further from (a) than ``(band_ref + 4 band_alg) s``:
    at least as good as the ``sqrtm`` route.
  * mean / covariance / z-score vs fp64 numpy: 4 x the band of fp64 numpy against itself with the rows in another order (at least
    eps), relative to the largest magnitude of the result.
  * R precision counts: EQUAL to (c) and to the host ``calculate_top_k`` on inputs whose every decision keeps a relative gap above
    1e-6 (asserted on the oracle alone); a tie pinned against (c).
  * matching score, diversity, multimodality: 1e-12 relative (sums of at most 512 squares of fp64 differences carry a few hundred
    eps; the host's expanded square loses a few digits more on these inputs); the numpy generator ends in the host call's state.
  * repeated runs: bit for bit.
  * evaluators with ``on_device=True`` vs ``False`` from one seed on a stub model with float64 tables: counts equal, FID within
    ``(band_ref + 4 band_alg) s`` of its own z-scored tables, the others 1e-12; no embedding is copied to the host.
  * scorers and ``tools/s2g_score.py --device_metrics``: the host path there reduces fp32 embeddings in fp32, so the device FIDs are
    compared with the same route on the same embeddings in fp64, within the bands of those embeddings; the lines that do not
    depend on the flag are the same text.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import emb_metrics_ref as R
import test_embmetrics_host as H
from motioncraft_amd import embmetrics as M, evaluation as E, lib as L

pytestmark = pytest.mark.gpu
EPS = H.EPS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_fid(gt, pred, **kw):
    return float(M.frechet_distance(dev(gt), dev(pred), **kw).item())


@pytest.mark.parametrize('tag', tuple(H.FID_CASES))
def test_frechet_distance_vs_the_nuclear_norm_oracle(tag):
    gt, pred = H.fid_tables(tag)
    b = H.bands(tag)
    out, info = M.frechet_distance(dev(gt), dev(pred), return_info=True)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (1,)
    got = float(out.item())
    err, tol = abs(got - b['oracle']), H.fid_tolerance(b)
    print(f'{tag}: device {got!r} oracle {b["oracle"]!r} s {b["scale"]:.6g}  |device - oracle| / s {err / b["scale"]:.2e}  band_alg {b["band_alg"]:.2e}  '
          f'band_ref {b["band_ref"]:.2e}  sweeps {info["sweeps"]} launches {info["launches"]}')
    assert np.isfinite(got)
    assert err <= tol, (err / b['scale'], b['band_alg'])
    assert err <= b['band_ref'] * b['scale'] + tol
    assert all(s <= M.MAX_SWEEPS for s in info['sweeps'])
    if tag.startswith('identical'):
        assert abs(got) <= tol                                             # pure cancellation
    if tag.startswith('repeated'):
        _, c = R.centred(pred)
        dmu = gt[0].astype(np.float64) - pred.astype(np.float64).mean(axis=0)
        assert abs(got - (dmu @ dmu + (c * c).sum() / (len(pred) - 1))) <= tol        # zero covariance: |dmu|^2 + Tr C2


def test_frechet_distance_emb_scale_and_float64_tables():
    gt, pred = H.fid_tables('n40_m43_d33')
    b = H.bands_of(gt, pred, 0.5)
    for g, p in ((gt, pred), (gt.astype(np.float64), pred.astype(np.float64)), (gt, pred.astype(np.float64))):
        assert abs(device_fid(g, p, emb_scale=0.5) - b['oracle']) <= H.fid_tolerance(b)


def order_band(fn, table, seed=0):
    """fp64 numpy against itself with the rows in another order, relative to the result's largest magnitude; at least eps"""
    a = np.asarray(table, dtype=np.float64)
    one, other = fn(a), fn(a[np.random.RandomState(seed).permutation(len(a))])
    return one, max(float(np.abs(one - other).max()) / max(float(np.abs(one).max()), np.finfo(np.float64).tiny), EPS)


@pytest.mark.parametrize('tag', tuple(t for t in H.FID_CASES if not t.startswith('identical')))
def test_activation_statistics_vs_numpy(tag):
    for table in H.fid_tables(tag):
        mean, cov = M.activation_statistics(dev(table), 0.5)
        want_mu, band_mu = order_band(lambda a: E.calculate_activation_statistics(a, 0.5)[0], table)
        want_cov, band_cov = order_band(lambda a: np.atleast_2d(E.calculate_activation_statistics(a, 0.5)[1]), table)
        d = table.shape[1]
        assert mean.dtype == cov.dtype == torch.float64 and tuple(mean.shape) == (d,) and tuple(cov.shape) == (d, d)
        e_mu, e_cov = np.abs(mean.cpu().numpy() - want_mu).max(), np.abs(cov.cpu().numpy() - want_cov).max()
        s_mu, s_cov = np.abs(want_mu).max(), max(np.abs(want_cov).max(), np.finfo(np.float64).tiny)
        print(f'{tag} [{table.shape[0]}, {d}]: mean {e_mu / s_mu:.2e} (band {band_mu:.2e})  covariance {e_cov / s_cov:.2e} (band {band_cov:.2e})')
        assert e_mu <= 4 * band_mu * s_mu and e_cov <= 4 * band_cov * s_cov
        assert torch.equal(cov, cov.T)


@pytest.mark.parametrize('n, d', [(1, 3), (7, 1), (39, 33), (130, 65), (32, 256), (64, 512)])
def test_zscore_with_a_constant_column(n, d):
    rs = np.random.RandomState(n + d)
    table = (rs.randn(n, d) * rs.uniform(0.1, 3, d) + rs.randn(d)).astype(np.float32)
    table[:, d // 2] = np.float32(1.7)                                     # deviation exactly 0 -> 1e-8, and (x - mean) = 0 exactly
    got = M.zscore(dev(table))
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, d)
    got = got.cpu().numpy()
    want, perm = R.zscore(table), np.random.RandomState(0).permutation(n)
    band = max(np.abs(R.zscore(table[perm]) - want[perm]).max() / max(np.abs(want).max(), 1.0), EPS)       # the rows in another order
    assert (got[:, d // 2] == 0).all() and (want[:, d // 2] == 0).all() and np.isfinite(got).all()
    err = np.abs(got - want).max()
    print(f'z-score [{n}, {d}]: {err:.2e} (band {band:.2e}, largest |z| {np.abs(want).max():.3g})')
    assert err <= 4 * band * max(np.abs(want).max(), 1.0)
    assert np.array_equal(M.zscore(dev(table.astype(np.float64))).cpu().numpy(), got)       # fp32 values widen exactly


def retrieval_inputs(n, d, seed, tie=False):
    """text and motion [n, d] float32 living in a 4-dimensional subspace, each motion pulled toward its text: the ranks vary, and
    (checked by the caller) no decision is closer than 1e-6"""
    rs = np.random.RandomState(seed)
    basis = rs.randn(4, d)
    latent = rs.randn(n, 4)
    text = (latent @ basis).astype(np.float32)
    motion = ((latent + 0.8 * rs.randn(n, 4)) @ basis).astype(np.float32)
    if tie:
        motion[5] = motion[2]
        motion[20] = motion[9]
    return text, motion


def decision_gap(text, motion, batch):
    """the smallest relative distance of a dist(t_i, m_j) from dist(t_i, m_i) that is not an exact tie, and the exact ties (i, j)"""
    gap, ties = np.inf, []
    for s in R.batches(len(text), batch):
        dist = R.distances(text[s], motion[s])
        own = np.diagonal(dist)[:, None]
        rel = np.abs(dist - own) / own
        rel[dist == own] = np.inf
        ties += [(s.start + i, s.start + j) for i, j in np.argwhere(dist == own) if i != j]
        gap = min(gap, rel.min())
    return gap, ties


@pytest.mark.parametrize('d', [33, 256])
def test_r_precision_counts_equal_the_oracle_and_the_host(d):
    text, motion = retrieval_inputs(39, d, 40 + d)
    gap, ties = decision_gap(text, motion, 32)
    assert gap > 1e-6 and not ties                                        # a condition on the oracle alone
    want = R.r_precision_counts(text, motion, 32, 3)
    t64, m64 = text.astype(np.float64), motion.astype(np.float64)
    host = np.array([E.calculate_top_k(np.argsort(E.euclidean_distance_matrix(t64[s], m64[s]), axis=1), 3).sum(axis=0) for s in R.batches(39, 32)])
    assert np.array_equal(want, host) and want.shape == (2, 3) and 0 < want[0, 0] < 32 and want[0, 0] < want[0, 2]      # the ranks vary
    got = M.r_precision_counts(dev(text), dev(motion), top_k=3, batch_size=32)
    assert got.dtype == torch.int32 and got.is_cuda
    print(f'd={d}: counts {got.cpu().numpy().tolist()}')
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(M.r_precision_counts(dev(t64), dev(m64), top_k=3, batch_size=32).cpu().numpy(), want)
    one = M.r_precision_counts(dev(text[:32]), dev(motion[:32]), top_k=3)                   # batch_size None: one batch
    assert np.array_equal(one.cpu().numpy(), want[:1])


def test_r_precision_tie_rule():
    text, motion = retrieval_inputs(32, 33, 77, tie=True)
    ranks = R.ranks(text, motion)
    dist = R.distances(text, motion)
    gap, ties = decision_gap(text, motion, 32)
    assert gap > 1e-6 and sorted(ties) == [(2, 5), (5, 2), (9, 20), (20, 9)]
    # the later row of a tied pair counts the earlier one, the earlier row does not count the later one
    assert ranks[5] == (dist[5] < dist[5, 5]).sum() + 1 and ranks[2] == (dist[2] < dist[2, 2]).sum()
    want = R.r_precision_counts(text, motion, 32, 8)
    got = M.r_precision_counts(dev(text), dev(motion), top_k=8)
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)


@pytest.mark.parametrize('d', [33, 256])
def test_matching_score_sum(d):
    text, motion = retrieval_inputs(39, d, 50 + d)
    t64, m64 = text.astype(np.float64), motion.astype(np.float64)
    zt, zm = M.zscore(dev(text[:32])), M.zscore(dev(motion[:32]))
    got = M.matching_score_sum(zt, zm)
    want = R.matching_sums(R.zscore(text[:32]), R.zscore(motion[:32]), 32)[0]
    host = E.euclidean_distance_matrix(E._zscore(t64[:32]), E._zscore(m64[:32])).trace()
    assert got.dtype == torch.float64 and tuple(got.shape) == (1,)
    print(f'd={d}: matching sum {got.item()!r}  vs (c) {abs(got.item() - want) / want:.1e}  vs host {abs(got.item() - host) / host:.1e}')
    assert abs(got.item() - want) <= 1e-12 * want and abs(got.item() - host) <= 1e-12 * host
    # raw tables, two batches (32 and a ragged 7) in one launch
    got = M.matching_score_sum(dev(text), dev(motion), batch_size=32).cpu().numpy()
    want = R.matching_sums(text, motion, 32)
    assert got.shape == (2,) and np.abs(got - want).max() <= 1e-12 * want.max()


@pytest.mark.parametrize('n, d, times', [(39, 33, 10), (301, 256, 300), (64, 512, 63)])
def test_diversity(n, d, times):
    table = R.dense_mixed(n, d, 60 + n)
    np.random.seed(17)
    host = E.calculate_diversity(table.astype(np.float64), times, 0.5, 2.0)
    state = np.random.get_state()
    np.random.seed(17)
    first, second = np.random.choice(n, times, replace=False), np.random.choice(n, times, replace=False)
    want = R.pair_distance(table, first, second, 0.5, 2.0)
    np.random.seed(17)
    got = M.diversity(dev(table), times, 0.5, 2.0)
    after = np.random.get_state()
    assert got.dtype == torch.float64 and tuple(got.shape) == (1,)
    print(f'diversity [{n}, {d}] x {times}: {got.item()!r}  vs (c) {abs(got.item() - want) / want:.1e}  vs host {abs(got.item() - host) / host:.1e}')
    assert abs(got.item() - want) <= 1e-12 * want and abs(got.item() - host) <= 1e-12 * host
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]


@pytest.mark.parametrize('sentences, repeats, d, picks', [(3, 5, 33, 2), (100, 30, 256, 10)])
def test_multimodality(sentences, repeats, d, picks):
    act = R.dense_mixed(sentences * repeats, d, 70 + d).reshape(sentences, repeats, d)
    np.random.seed(18)
    host = E.calculate_multimodality(act.astype(np.float64), picks)
    state = np.random.get_state()
    np.random.seed(18)
    first, second = np.random.choice(repeats, picks, replace=False), np.random.choice(repeats, picks, replace=False)
    want = R.pair_distance(act, first, second)
    np.random.seed(18)
    got = M.multimodality(dev(act), picks)
    after = np.random.get_state()
    print(f'multimodality [{sentences}, {repeats}, {d}] x {picks}: {got.item()!r}  vs (c) {abs(got.item() - want) / want:.1e}  vs host {abs(got.item() - host) / host:.1e}')
    assert abs(got.item() - want) <= 1e-12 * want and abs(got.item() - host) <= 1e-12 * host
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_two_runs_give_the_same_bits():
    gt, pred = (dev(t) for t in H.fid_tables('n300_m303_d256'))
    one = M.frechet_distance(gt, pred)
    M.zscore(gt)                                                           # an unrelated launch in between
    torch.randn(1 << 16, device='cuda').sum()
    two = M.frechet_distance(gt, pred)
    assert torch.equal(one, two) and one.cpu().numpy().tobytes() == two.cpu().numpy().tobytes()
    a, b = M.activation_statistics(gt), M.activation_statistics(gt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refusals():
    lib = L.load(require_gpu=True)
    gt, pred = (dev(t) for t in H.fid_tables('n40_m43_d33'))
    out = torch.zeros(1, device='cuda', dtype=torch.float64)
    work = torch.empty(1 << 16, device='cuda', dtype=torch.float64)

    def call(g, n, p, m, d, sweeps=0, w=work):
        return lib.mc_emb_frechet(g, n, p, m, d, 0, 1.0, sweeps, L.ptr(w), w.numel() * 8, L.ptr(out), None, L.stream())
    assert call(L.ptr(gt), 40, L.ptr(pred), 43, 33) == L.MC_OK
    assert call(L.ptr(gt), 40, L.ptr(pred), 43, L.MC_EMB_MAX_DIM + 1) == L.MC_ERR_ARG and str(L.MC_EMB_MAX_DIM) in L.last_error()
    assert call(L.ptr(gt), 1, L.ptr(pred), 43, 33) == L.MC_ERR_ARG and call(L.ptr(gt), 40, L.ptr(pred), 1, 33) == L.MC_ERR_ARG
    assert call(L.ptr(gt), 40, L.ptr(pred), 43, 33, w=work[:64]) == L.MC_ERR_ARG and 'workspace' in L.last_error()
    assert call(L.ptr(gt), 40, L.ptr(pred), 43, 33, sweeps=L.MC_EMB_MAX_SWEEPS + 1) == L.MC_ERR_ARG
    host = np.ascontiguousarray(H.fid_tables('n40_m43_d33')[0])
    assert call(host.ctypes.data, 40, L.ptr(pred), 43, 33) == L.MC_ERR_ARG and 'device pointer' in L.last_error()
    assert lib.mc_emb_zscore(host.ctypes.data, 40, 33, 0, L.ptr(work), L.stream()) == L.MC_ERR_ARG and 'device pointer' in L.last_error()
    assert lib.mc_emb_statistics(L.ptr(gt), 1, 33, 0, 1.0, L.ptr(work), work.numel() * 8, L.ptr(work), L.ptr(work), L.stream()) == L.MC_ERR_ARG
    assert lib.mc_emb_retrieval(L.ptr(gt), L.ptr(gt), 40, 33, 0, L.MC_EMB_MAX_BATCH + 1, 3, L.ptr(work), None, L.stream()) == L.MC_ERR_ARG
    for bad in (lambda: M.frechet_distance(gt.cpu(), pred), lambda: M.frechet_distance(gt, pred[:, :32]), lambda: M.frechet_distance(gt[:1], pred),
                lambda: M.r_precision_counts(gt, gt, batch_size=65), lambda: M.r_precision_counts(gt, pred), lambda: M.diversity(gt, 40),
                lambda: M.zscore(torch.zeros(3, L.MC_EMB_MAX_DIM + 1, device='cuda'))):
        with pytest.raises(ValueError):
            bad()
    # one sweep where more are needed: the error code comes back, nothing loops, and the next call is unaffected
    assert call(L.ptr(gt), 40, L.ptr(pred), 43, 33, sweeps=1) == L.MC_ERR_NOCONV and 'sweep 1' in L.last_error()
    with pytest.raises(M.NoConvergence):
        M.frechet_distance(gt, pred, max_sweeps=1)
    b = H.bands('n40_m43_d33')
    assert abs(float(M.frechet_distance(gt, pred).item()) - b['oracle']) <= H.fid_tolerance(b)


def test_evaluators_on_the_device_agree_with_the_host_path():
    n = 39
    model, results = H.StubModel('cuda', 48, 6, n), H.stub_results(n, 15)
    H.Tracked.transfers = 0
    host, host_state = H.run_evaluators(model, results, n, False)
    assert H.Tracked.transfers > 0
    H.Tracked.transfers = 0
    got, state = H.run_evaluators(model, results, n, True)
    assert H.Tracked.transfers == 0                                        # no embedding was copied to the host
    print(host, got, sep='\n')
    assert list(got) == list(host)
    assert state[0] == host_state[0] and np.array_equal(state[1], host_state[1]) and state[2:] == host_state[2:]
    for k in range(1, 4):
        assert got[f'R_precision Top {k} (mean)'] == host[f'R_precision Top {k} (mean)']
    for key in ('Matching Score (mean)', 'Diversity (mean)', 'MultiModality (mean)'):
        assert abs(got[key] - host[key]) <= 1e-12 * abs(host[key]) and host[key] > 0, key
    # the FID evaluator's own tables (39 rows of 48 columns: n - 1 < d), z-scored on the host in fp64
    ev = E.FIDEvaluator(data_len=n, evaluator_model=model, emb_scale=0.5)
    res = ev.prepare_results(results[:n])
    pred, gt = E._zscore(ev._motion_emb(res)), E._zscore(ev._motion_emb(res, prefix=''))
    assert pred.dtype == np.float64 and pred.shape == (n, 48)
    b = H.bands_of(gt, pred, 0.5)
    print(f'FID: device {got["FID (mean)"]!r} host {host["FID (mean)"]!r} oracle {b["oracle"]!r} band_alg {b["band_alg"]:.2e} band_ref {b["band_ref"]:.2e}')
    assert abs(got['FID (mean)'] - host['FID (mean)']) <= b['band_ref'] * b['scale'] + H.fid_tolerance(b)
    assert all(v == 0 for k, v in got.items() if k.endswith('(conf)'))


def test_evaluator_embeddings_reach_the_reduction_as_device_tensors(monkeypatch):
    n = 39
    model, results = H.StubModel('cuda', 16, 6, n), H.stub_results(n, 0)
    seen = []
    real = M.frechet_distance
    monkeypatch.setattr(M, 'frechet_distance', lambda gt, pred, *a, **k: (seen.append((gt, pred)), real(gt, pred, *a, **k))[1])
    ev = E.FIDEvaluator(data_len=n, evaluator_model=model, on_device=True)
    assert np.isfinite(ev.evaluate(results)['FID (mean)'])
    assert len(seen) == 1 and all(t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (n, 16) for t in seen[0])


# ---- the scorers and the tool ----------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_FLAGS = ('--latent_dim', '128', '--ff_size', '256', '--num_layers', '2', '--num_heads', '2')       # helpers.EVAL_DIMS


@pytest.fixture(scope='module')
def eval_state():
    from helpers import EVAL_DIMS
    from oracle import weights as W
    return {k: torch.as_tensor(v) for k, v in W.make_eval_encoder_state(W.eval_encoder_param_shapes(**EVAL_DIMS), seed=8).items()}


@pytest.fixture(scope='module')
def evaluator(eval_state):
    import motioncraft_amd as mc
    from helpers import EVAL_DIMS
    enc_cfg = {k: v for k, v in EVAL_DIMS.items() if k != 'nfeats'}
    model = mc.build_submodule(dict(type='T2MContrastiveModel_SMPLX', motion_encoder=dict(nfeats=EVAL_DIMS['nfeats'], vae=True, **enc_cfg),
                                    state_dict=eval_state))
    yield model
    model.encoder.close()


def fid_agrees(got, gt_emb, pred_emb):
    """the device's FID vs the host route on the same embeddings in fp64: within the host route's band + 4 x the algorithm's"""
    from motioncraft_amd import scoring as S
    host, b = S._fid(gt_emb, pred_emb), H.bands_of(gt_emb, pred_emb)
    print(f'    FID device {got!r} host {host!r} oracle {b["oracle"]!r} band_alg {b["band_alg"]:.2e} band_ref {b["band_ref"]:.2e}')
    return abs(got - host) <= b['band_ref'] * b['scale'] + H.fid_tolerance(b)


def test_m2d_scorer_on_the_device(evaluator):
    from motioncraft_amd import scoring as S
    host, devs = S.M2DScorer(evaluator), S.M2DScorer(evaluator, on_device=True)
    g = torch.Generator().manual_seed(96)
    for T in (40, 33, 57, 24, 31):
        rec, gt = torch.randn(T, 322, generator=g), torch.randn(T, 322, generator=g)
        host.add_sequence(rec, gt)
        devs.add_sequence(rec, gt)
    assert all(e.is_cuda for v in devs.emb.values() for e in v)
    np.random.seed(6)
    want = host.summary()
    state = np.random.get_state()
    np.random.seed(6)
    got = devs.summary()
    after = np.random.get_state()
    print(want, got, sep='\n')
    assert list(got) == list(want) and after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    cat = {k: np.concatenate(v).astype(np.float64) for k, v in host.emb.items()}
    # the scorer's host path reduces the fp32 embeddings in fp32; the comparison is with the same route in fp64
    assert fid_agrees(got['FID(Whole Body) score'], cat['gt'], cat['pred'])
    assert fid_agrees(got['FID (Hands) score'], cat['hand_gt'], cat['hand_pred'])
    # the host diversity runs on the fp32 table in fp32; the device widens the same values and reduces in fp64
    assert abs(got['Diversity score'] - want['Diversity score']) <= 64 * np.finfo(np.float32).eps * want['Diversity score']
    np.random.seed(6)
    assert abs(got['Diversity score'] - E.calculate_diversity(cat['pred'], 4, 1.0, 1.0)) <= 1e-12 * got['Diversity score']


def test_s2g_score_tool_with_device_metrics(tmp_path, eval_state):
    """tools/s2g_score.py with and without --device_metrics on two saved sequences (mean_vel and onsets of the reference fixture):
    the four lines that do not depend on the flag are the same text; the host path reduces the fp32 embeddings in fp32, so the two
    FIDs of the device path are compared with the same route on the same embeddings in fp64, within the bands of those embeddings"""
    import smplx_lbs_ref as ref
    import test_scoring_host as SH
    from motioncraft_amd import scoring as S
    g, _ = SH.golden_cases()
    np.savez(tmp_path / 'model.npz', **ref.synthetic_model(V=1031, shape_space=300, seed=13))
    torch.save(eval_state, tmp_path / 'evaluator.pth')
    np.save(tmp_path / 'mean_vel.npy', g['T200.f32.mean_vel'])
    os.makedirs(tmp_path / 'onsets')
    rs = np.random.RandomState(3)
    for i, name in enumerate(('a', 'b', 'c')):
        T = 200 - 7 * i
        np.save(tmp_path / 'onsets' / f'{name}.npy', g['T200.onsets9'][g['T200.onsets9'] < (T - 120) / 30])
        for kind in ('res', 'gt'):
            np.savez(tmp_path / f'{kind}_{name}.npz', poses=ref.random_poses(T, 50 + 2 * i + (kind == 'gt')).astype(np.float32),
                     expressions=rs.randn(T, 100).astype(np.float32), trans=(0.1 * rs.randn(T, 3)).astype(np.float32), betas=rs.randn(300).astype(np.float32))
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 's2g_score.py'), str(tmp_path), '--onsets', str(tmp_path / 'onsets'), '--smplx_model',
           str(tmp_path / 'model.npz'), '--evaluator', str(tmp_path / 'evaluator.pth'), '--mean_vel', str(tmp_path / 'mean_vel.npy'), *EVAL_FLAGS]
    lines = []
    for flags in ((), ('--device_metrics',)):
        r = subprocess.run(['timeout', '-k', '10', '120'] + cmd + list(flags), capture_output=True, text=True, timeout=150)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(r.stdout.splitlines())
        print(r.stdout)
    host, got = lines
    names = ['l2 loss', 'lvel loss', 'align score', 'l1div score', 'FID(Whole Body) score', 'FID (Hands) score']
    assert [l.split(': ')[0] for l in host] == names == [l.split(': ')[0] for l in got]
    assert host[:4] == got[:4]
    # the embeddings the tool reduced: the same packings through the same evaluator weights, in this process
    import motioncraft_amd as mc
    from helpers import EVAL_DIMS
    model = mc.build_submodule(dict(type='T2MContrastiveModel_SMPLX', motion_encoder=dict(vae=True, **EVAL_DIMS), state_dict=eval_state))
    emb = dict(pred=[], gt=[], hand_pred=[], hand_gt=[])
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))
    for name in ('a', 'b', 'c'):
        with np.load(tmp_path / f'res_{name}.npz') as res, np.load(tmp_path / f'gt_{name}.npz') as gt:
            rec_motion = S.pack_motion(t(res['poses']), t(res['expressions']), t(res['trans']))
            rec_pose, _, rec_trans = S.unpack_rec_motion(rec_motion)
            emb['pred'].append(S._embed(model, rec_motion))
            emb['gt'].append(S._embed(model, S.pack_motion(t(gt['poses']), t(gt['expressions']), t(gt['trans']))))
            emb['hand_pred'].append(S._embed(model, S.hand_only_motion(rec_pose, rec_trans)))
            emb['hand_gt'].append(S._embed(model, S.hand_only_motion(t(gt['poses']), t(gt['trans']))))
    model.encoder.close()
    cat = {k: np.concatenate(v).astype(np.float64) for k, v in emb.items()}
    value = lambda line: float(line.split(': ')[1])
    assert value(host[4]) == S._fid(np.concatenate(emb['gt']), np.concatenate(emb['pred']))          # the tool's host FID: fp32 throughout
    assert fid_agrees(value(got[4]), cat['gt'], cat['pred'])
    assert fid_agrees(value(got[5]), cat['hand_gt'], cat['hand_pred'])

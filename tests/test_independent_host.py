"""Host: the statements behind independent requests -- the row-keyed noise definition, the oracle's "no drops, no coupling", and the
request batcher's packing against a stub model call (no GPU)."""
import numpy as np
import pytest
import torch

import rowseed_ref
from helpers import HML_SMALL, SMALL, SMALL_SEED, skew_gates, synth_inputs
from oracle import philox_oracle as P

SEEDS = [7, 2 ** 63 + 5, 7 + 2 ** 32]          # (two keys that differ in the high word only)


@pytest.mark.parametrize('dims,T', [(SMALL, 24), (HML_SMALL, 23)], ids=['C322_T24', 'C263_T23'])
def test_rowseed_ref_rows_are_the_b1_streams(dims, T):
    """Row b of the flat-group walk equals draw_normal(T C, seeds[b], d).  C = 263, T = 23: T C is odd, so flat groups straddle rows and
    every later row sits askew of its own Philox blocks."""
    C = dims['input_feats']
    if C == 263:
        assert (T * C) % 4 != 0 and rowseed_ref.straddling_groups(len(SEEDS), T, C) >= 1
    else:
        assert (T * C) % 4 == 0 and rowseed_ref.straddling_groups(len(SEEDS), T, C) == 0
    for d in (0, 3):
        got = rowseed_ref.draw_rows(SEEDS, T, C, d)
        for b, s in enumerate(SEEDS):
            assert np.array_equal(got[b].reshape(-1), P.draw_normal(T * C, s, d)), (b, d)
    assert not np.array_equal(rowseed_ref.draw_rows(SEEDS, T, C, 0), rowseed_ref.draw_rows(SEEDS, T, C, 1))


@pytest.fixture(scope='module')
def oracle_case():
    from oracle import weights as W
    sd = skew_gates(W.make_state_dict(SMALL, SMALL_SEED), SMALL, 'hot_pair')
    B, T = 3, 24
    lengths = (24, 17, 20)
    x, xf, mask = synth_inputs(SMALL, B, T, seed=91, lengths=lengths)
    x2, xf2, mask2 = synth_inputs(SMALL, B, T, seed=92, lengths=(24, 9, 24))
    # the same request in row 0, other requests (content, lengths) in rows 1-2
    xr, xfr, maskr = x.clone(), xf.clone(), mask.clone()
    xr[1:], xfr[1:], maskr[1:] = x2[1:], xf2[1:], mask2[1:]
    return sd, (x, xf, mask), (xr, xfr, maskr)


def test_oracle_row_is_a_function_of_its_request_without_drops(oracle_case):
    """One denoiser call at t = 640 on the oracle.  capacity_factor = E drops nothing (2 int(E ceil(N / E)) >= 2 N): row 0 does not move
    when rows 1-2 are replaced (<= 1e-6) and equals the same request alone up to summation order (<= 1e-4).  At 1.5 the replacement moves
    row 0 by more than 1e-2: the inputs can show the coupling."""
    from oracle import stmogen_oracle as O
    sd, (x, xf, mask), (xr, xfr, maskr) = oracle_case
    E = float(SMALL['E'])
    full = O.denoise(sd, SMALL, x, 640, xf, mask, capacity_factor=E)
    repl = O.denoise(sd, SMALL, xr, 640, xfr, maskr, capacity_factor=E)
    alone = O.denoise(sd, SMALL, x[:1], 640, xf[:1], mask[:1], capacity_factor=E)
    d_repl, d_alone = float((full[0] - repl[0]).abs().max()), float((full[0] - alone[0]).abs().max())
    full15 = O.denoise(sd, SMALL, x, 640, xf, mask)
    repl15 = O.denoise(sd, SMALL, xr, 640, xfr, maskr)
    d15 = float((full15[0] - repl15[0]).abs().max())
    print(f'row 0: replaced mates {d_repl:.2e} (cf = E), alone {d_alone:.2e} (cf = E), replaced mates {d15:.2e} (cf = 1.5); |out| {float(full.abs().max()):.2f}')
    assert d_repl <= 1e-6
    assert d_alone <= 1e-4
    assert d15 > 1e-2


# ---- the batcher against a stub model call ------------------------------------------------------
def _stub_runner(calls, frames=6, C=3):
    def run(xf, lengths, seeds, c):
        calls.append(dict(xf=xf.clone(), lengths=list(lengths), seeds=list(seeds), c=None if c is None else c.clone()))
        rows = []
        for b in range(xf.shape[0]):               # a row-wise function of (condition, length, seed, control)
            base = float(xf[b].sum()) + 1000.0 * lengths[b] + float(seeds[b] % 997) + (0.0 if c is None else float(c[b].sum()))
            rows.append(base + torch.arange(frames * C, dtype=torch.float64).reshape(frames, C))
        return torch.stack(rows)
    return run


def _requests(n, with_c=()):
    from motioncraft_amd.serve import Request
    g = torch.Generator().manual_seed(3)
    out = []
    for i in range(n):
        c = torch.randn(4, 2, generator=g) if i in with_c else None
        out.append(Request(length=1 + i % 6, seed=100 + i, xf_out=torch.randn(2, 5, generator=g), c=c))
    return out


def test_batcher_packs_pads_and_does_not_depend_on_the_order():
    from motioncraft_amd.serve import DUMMY_SEED, RequestBatcher
    reqs = _requests(5)
    results = []
    for order in ([0, 1, 2, 3, 4], [3, 0, 4, 2, 1]):
        calls = []
        bt = RequestBatcher(None, batch=3, frames=6, sampler='ddim', steps=4, runner=_stub_runner(calls))
        handles = {i: bt.submit(reqs[i]) for i in order}
        plan = bt.plan()
        assert [len(rows) for rows in plan] == [3, 3]
        assert sorted(h for rows in plan for h in rows if h is not None) == sorted(handles.values())
        assert sum(h is None for rows in plan for h in rows) == 1
        out = bt.run()
        assert len(calls) == 2 and all(c['xf'].shape[0] == 3 for c in calls)
        # the open row is the fixed dummy request: zero condition, full length, the dummy seed
        assert calls[1]['lengths'][2] == 6 and calls[1]['seeds'][2] == DUMMY_SEED and float(calls[1]['xf'][2].abs().max()) == 0.0
        assert bt.plan() == [] and bt.run() == {}
        results.append({i: out[handles[i]] for i in order})
        for i in order:
            assert tuple(out[handles[i]].shape) == (reqs[i].length, 3)
    for i in range(5):
        assert torch.equal(results[0][i], results[1][i]), i


def test_batcher_keeps_controlled_and_plain_requests_apart():
    from motioncraft_amd.serve import RequestBatcher
    reqs = _requests(4, with_c=(1, 3))
    calls = []
    bt = RequestBatcher(None, batch=3, frames=6, runner=_stub_runner(calls))
    for r in reqs:
        bt.submit(r)
    out = bt.run()
    assert len(out) == 4 and len(calls) == 2
    assert sorted(c['c'] is None for c in calls) == [False, True]
    ctrl = next(c for c in calls if c['c'] is not None)
    assert tuple(ctrl['c'].shape) == (3, 4, 2) and float(ctrl['c'][2].abs().max()) == 0.0      # the dummy row's control is zero


def test_batcher_and_request_argument_errors():
    from motioncraft_amd.serve import Request, RequestBatcher
    xf = torch.zeros(2, 5)
    for kw in (dict(length=0, seed=1, xf_out=xf), dict(length=2, seed=-1, xf_out=xf), dict(length=2, seed=2 ** 64, xf_out=xf),
               dict(length=2, seed=1), dict(length=2, seed=1, xf_out=xf, text='a'), dict(length=2.5, seed=1, xf_out=xf),
               dict(length=2, seed=1, xf_out=torch.zeros(1, 2, 5)), dict(length=2, seed=1, xf_out=xf, c=torch.zeros(3))):
        with pytest.raises(ValueError):
            Request(**kw)
    for kw in (dict(batch=0, frames=6), dict(batch=3, frames=0), dict(batch=3, frames=6, sampler='euler'),
               dict(batch=3, frames=6, steps=0), dict(batch=3, frames=6, capacity_factor=-1)):
        with pytest.raises(ValueError):
            RequestBatcher(None, **kw)
    bt = RequestBatcher(None, batch=3, frames=6, runner=_stub_runner([]))
    with pytest.raises(ValueError):
        bt.submit(Request(length=7, seed=1, xf_out=xf))
    with pytest.raises(ValueError):
        bt.submit('a person walks')


def test_seed_lists_are_checked_before_anything_runs():
    from motioncraft_amd.diffusion import GaussianDiffusion
    from motioncraft_amd.engine import check_seeds
    assert check_seeds((1, 2 ** 64 - 1, 0), 3) == [1, 2 ** 64 - 1, 0]
    for bad, rows in (((1, 2), 3), ((1, 2, -1), 3), ((1, 2, 2 ** 64), 3), (5, 1), (('a',), 1)):
        with pytest.raises(ValueError):
            check_seeds(bad, rows)
    g = torch.Generator()
    for kw in (dict(noise=torch.zeros(1)), dict(step_noise=[1]), dict(generator=g)):
        args = dict(noise=None, step_noise=None, generator=None)
        args.update(kw)
        with pytest.raises(ValueError, match='exclusive'):
            GaussianDiffusion._seeds_of([1, 2, 3], (3, 24, 322), **args)
    assert GaussianDiffusion._seeds_of(None, (3, 24, 322), None, None, g) is None

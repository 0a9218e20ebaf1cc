"""Host: the per-row-timestep restatement of the oracle (``rowstep_ref``) and the scheduling of ``serve.ContinuousBatcher`` through a
fake runner -- admission order, the clipping of ``n``, per-row walk positions (draw 1 + position), retirement, dummy fill, fresh flags
and argument errors."""
import pytest
import torch

import rowstep_ref
from helpers import SMALL, SMALL_SEED, synth_inputs

B, T = 3, 24
LENGTHS = (24, 17, 20)


@pytest.fixture(scope='module')
def small():
    from oracle import weights as W
    threads = torch.get_num_threads()
    torch.set_num_threads(4)
    yield W.make_state_dict(SMALL, SMALL_SEED)
    torch.set_num_threads(threads)


def test_restatement_equals_the_oracle_when_all_rows_share_a_timestep(small):
    from oracle import stmogen_oracle as O
    x, xf, mask = synth_inputs(SMALL, B, T, seed=81, lengths=LENGTHS)
    for cf in (None, float(SMALL['E'])):
        want = O.denoise(small, SMALL, x, 640, xf, mask, capacity_factor=cf)
        got = rowstep_ref.denoise_rows(small, SMALL, x, [640] * B, xf, mask, capacity_factor=cf)
        assert torch.equal(got, want)


def test_without_drops_a_row_of_a_mixed_call_is_its_b1_call(small):
    """no capacity cut: nothing couples the rows, so row b at ts[b] equals the B = 1 call at ts[b] (fp32 reduction order of a batched
    matmul aside: 1e-5)"""
    from oracle import stmogen_oracle as O
    x, xf, mask = synth_inputs(SMALL, B, T, seed=82, lengths=LENGTHS)
    ts = [999, 250, 400]
    cf = float(SMALL['E'])
    got = rowstep_ref.denoise_rows(small, SMALL, x, ts, xf, mask, capacity_factor=cf)
    same = rowstep_ref.denoise_rows(small, SMALL, x, [400] * B, xf, mask, capacity_factor=cf)
    assert float((got[0] - same[0]).abs().max()) > 1e-3                  # the timestep matters
    for b, t in enumerate(ts):
        alone = O.denoise(small, SMALL, x[b:b + 1], t, xf[b:b + 1], mask[b:b + 1], capacity_factor=cf)
        assert float((got[b] - alone[0]).abs().max()) <= 1e-5, b
    # a per-row guidance scale is the row's own weight
    scaled = rowstep_ref.denoise_rows(small, SMALL, x, ts, xf, mask, capacity_factor=cf, scales=[SMALL['scale'], 1.0, SMALL['scale']])
    assert torch.equal(scaled[0], got[0]) and torch.equal(scaled[2], got[2]) and not torch.equal(scaled[1], got[1])
    out2 = rowstep_ref.denoise_rows(small, SMALL, x, ts, xf, mask, capacity_factor=cf, out2=True)
    w = rowstep_ref.guidance_weight(400, 1.0)
    assert float((out2[2] * w + out2[B + 2] * (1 - w)
                  - rowstep_ref.denoise_rows(small, SMALL, x, ts, xf, mask, capacity_factor=cf, scales=[1.0] * B)[2]).abs().max()) <= 1e-6


# ---- ContinuousBatcher through a fake runner ----------------------------------------------------------
class FakeRunner:
    """records every call; a row's "motion" is seed + the sum over its steps of (1 + position) * scale -- a function of the request alone"""

    def __init__(self, steps, batch, frames, C=2):
        self.steps, self.batch, self.frames, self.C = steps, batch, frames, C
        self.calls = []
        self.x = torch.zeros(batch, frames, C)

    def condition(self, xf_out, lengths, seeds, fresh, c):
        assert tuple(xf_out.shape)[0] == self.batch and len(lengths) == len(seeds) == len(fresh) == self.batch
        self.calls.append(('condition', [float(v) for v in xf_out[:, 0, 0]], list(lengths), list(seeds), list(fresh), None if c is None else tuple(c.shape)))
        self.controls = getattr(self, 'controls', []) + [None if c is None else c.clone()]
        for b, f in enumerate(fresh):
            if f:
                self.x[b] = float(seeds[b])

    def advance(self, pos, scales):
        assert all(len(r) == self.batch for r in pos) and len(scales) == self.batch
        self.calls.append(('advance', [list(r) for r in pos], list(scales)))
        for row in pos:
            for b, p in enumerate(row):
                assert 0 <= p < self.steps
                self.x[b] += (1 + p) * (2.5 if scales[b] is None else scales[b])

    def result(self):
        return self.x.clone()


def _req(i, length=3, scale=None, c=None):
    from motioncraft_amd.serve import Request
    return Request(length=length, seed=100 + i, xf_out=torch.full((4, 3), float(i + 1)), guidance_scale=scale, c=c)


def _expected(i, steps, scale=None):
    return 100 + i + sum(1 + p for p in range(steps)) * (2.5 if scale is None else scale)


def _advances(r):
    return [c for c in r.calls if c[0] == 'advance']


def test_admission_order_dummy_fill_and_fresh_flags():
    from motioncraft_amd.serve import DUMMY_SEED, ContinuousBatcher
    r = FakeRunner(4, 3, 6)
    bt = ContinuousBatcher(None, batch=3, frames=6, steps=4, runner=r)
    assert bt.tick() == 0 and r.calls == []                              # nothing to run: no call at all
    h = [bt.submit(_req(i, length=3 + i)) for i in range(2)]
    assert bt.tick() == 1
    kind, xf0, lengths, seeds, fresh, c = r.calls[0]
    assert kind == 'condition' and xf0 == [1.0, 2.0, 0.0] and lengths == [3, 4, 6] and seeds == [100, 101, DUMMY_SEED] and c is None
    assert fresh == [True, True, True]                                   # the first call starts the dummy row too
    assert r.calls[1] == ('advance', [[0, 0, 0]], [None, None, None])
    assert bt.occupied == [h[0], h[1], None]
    h.append(bt.submit(_req(2)))                                         # joins at tick 1 in the open row
    assert bt.tick() == 1
    assert r.calls[2][0] == 'condition' and r.calls[2][4] == [False, False, True] and r.calls[2][3] == [100, 101, 102]
    assert r.calls[3] == ('advance', [[1, 1, 0]], [None, None, None])
    assert bt.tick(2) == 2                                               # rows 0, 1 end: clipped to their remaining 2
    assert r.calls[4] == ('advance', [[2, 2, 1], [3, 3, 2]], [None, None, None])
    done = bt.poll()
    assert sorted(done) == h[:2] and bt.occupied == [None, None, h[2]] and bt.poll() == {}
    assert tuple(done[h[0]].shape) == (3, 2) and tuple(done[h[1]].shape) == (4, 2)
    assert float(done[h[0]][0, 0]) == _expected(0, 4) and float(done[h[1]][0, 0]) == _expected(1, 4)
    assert bt.finished_at[h[0]] == 4 and bt.submitted_at[h[2]] == 1
    # open rows run the dummy at walk position 0; no condition call without an admission
    n_cond = sum(c[0] == 'condition' for c in r.calls)
    assert bt.tick(5) == 1                                               # row 2 has one step left
    assert r.calls[-1] == ('advance', [[0, 0, 3]], [None, None, None]) and sum(c[0] == 'condition' for c in r.calls) == n_cond
    assert float(bt.poll()[h[2]][0, 0]) == _expected(2, 4)
    assert bt.tick() == 0
    # the next admission replaces the retired rows' conditions by the dummy: every stale row is fresh
    h3 = bt.submit(_req(3))
    bt.tick()
    assert r.calls[-2][0] == 'condition' and r.calls[-2][4] == [True, True, True] and r.calls[-2][1] == [4.0, 0.0, 0.0]
    assert bt.occupied == [h3, None, None]


def test_n_is_clipped_to_the_smallest_remaining_walk_and_run_drains_the_queue():
    from motioncraft_amd.serve import ContinuousBatcher
    r = FakeRunner(6, 2, 4)
    bt = ContinuousBatcher(None, batch=2, frames=4, steps=6, runner=r)
    hs = [bt.submit(_req(i, scale=[None, 1.0, 4.0, None, 0.5][i])) for i in range(5)]
    assert bt.tick(4) == 4                                               # both rows fresh: nothing clips 4 <= 6
    assert bt.tick(4) == 2                                               # ... now 2 steps are left
    out = bt.poll()
    assert sorted(out) == hs[:2]
    out.update(bt.run())
    assert sorted(out) == hs
    for i, h in enumerate(hs):
        assert float(out[h][0, 0]) == _expected(i, 6, [None, 1.0, 4.0, None, 0.5][i]), i
    # no advance is longer than a walk
    for _, pos, scales in _advances(r):
        assert 1 <= len(pos) <= 6
    assert bt.ticks == sum(len(c[1]) for c in _advances(r))
    assert all(bt.finished_at[h] - bt.submitted_at[h] >= 6 for h in hs)
    # requests 2 and 3 took the two rows as soon as they were free, request 4 the first row free after that
    assert bt.finished_at[hs[2]] == 12 and bt.finished_at[hs[3]] == 12 and bt.finished_at[hs[4]] == 18


def test_control_requests_never_share_a_call_with_plain_ones():
    from motioncraft_amd.serve import ContinuousBatcher
    r = FakeRunner(2, 2, 4)
    bt = ContinuousBatcher(None, batch=2, frames=4, steps=2, runner=r)
    ctrl = torch.zeros(3, 5)
    h0 = bt.submit(_req(0))
    h1 = bt.submit(_req(1, c=ctrl))
    h2 = bt.submit(_req(2))
    bt.tick()
    assert bt.occupied == [h0, h2]                                       # the control request waits: the running rows have none
    out = bt.run()
    assert sorted(out) == [h0, h1, h2]
    conds = [c for c in r.calls if c[0] == 'condition']
    assert [c[5] for c in conds] == [None, (2, 3, 5)]


def test_successive_control_batches_of_one_shape_hand_over_their_own_contents():
    """two control batches of the same [Tc, Fc] one after the other: every condition call carries the control rows of the requests it
    admits (the dummy row's are zero) with every row fresh -- the runner must set the control condition on each of them"""
    from motioncraft_amd.serve import ContinuousBatcher
    r = FakeRunner(2, 2, 4)
    bt = ContinuousBatcher(None, batch=2, frames=4, steps=2, runner=r)
    cs = [torch.full((3, 5), float(v)) for v in (1, 2, 3)]
    hs = [bt.submit(_req(i, c=c)) for i, c in enumerate(cs)]
    out = bt.run()
    assert sorted(out) == hs
    conds = [c for c in r.calls if c[0] == 'condition']
    assert [c[5] for c in conds] == [(2, 3, 5), (2, 3, 5)] and [c[4] for c in conds] == [[True, True], [True, True]]
    assert [float(v) for v in r.controls[0][:, 0, 0]] == [1.0, 2.0] and [float(v) for v in r.controls[1][:, 0, 0]] == [3.0, 0.0]
    assert bt.finished_at[hs[2]] == 4                                    # the third request waited for the batch to drain


def test_argument_errors():
    from motioncraft_amd.serve import ContinuousBatcher, Request
    r = FakeRunner(4, 2, 4)
    for kw in (dict(sampler='euler'), dict(batch=0), dict(frames=0), dict(steps=0), dict(capacity_factor=-1)):
        with pytest.raises(ValueError):
            ContinuousBatcher(None, **{**dict(batch=2, frames=4, steps=4, runner=r), **kw})
    bt = ContinuousBatcher(None, batch=2, frames=4, steps=4, runner=r)
    with pytest.raises(ValueError):
        bt.submit('a prompt')
    with pytest.raises(ValueError):
        bt.submit(_req(0, length=5))                                     # longer than the batcher's frames
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            bt.tick(bad)
    with pytest.raises(ValueError):
        Request(length=3, seed=1, xf_out=torch.zeros(4, 3), guidance_scale='high')
    with pytest.raises(ValueError):
        Request(length=3, seed=1, xf_out=torch.zeros(4, 3), guidance_scale=float('nan'))
    assert Request(length=3, seed=1, xf_out=torch.zeros(4, 3)).guidance_scale is None

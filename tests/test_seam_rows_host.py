"""Host: long requests in ``serve.ContinuousBatcher`` (``overlap=``) through a fake runner -- window planning on
and off the grid, ``W > batch``, strict FIFO admission into non-contiguous open rows, the row seam table re-sent on every admission and
retirement of a long request, rows of a request advancing and retiring together, the stitch, and ``overlap=None`` behaving as ever --
plus the fp64 restatement ``seam_rows_ref`` against ``seam_ref`` where the two describe the same thing."""
import numpy as np
import pytest
import torch

import seam_ref
import seam_rows_ref as SR

T, OV = 6, 2
STRIDE = T - OV


class FakeRunner:
    """records every call; after a walk frame t of a row holds 1000 seed + (the row's first frame + t) + 0.001 * the steps it took: a
    function of the request and the GLOBAL frame alone, so the stitch of a long request is checkable frame by frame"""

    def __init__(self, steps, batch, frames, C=2):
        self.steps, self.batch, self.frames, self.C = steps, batch, frames, C
        self.calls = []
        self.x = torch.zeros(batch, frames, C, dtype=torch.float64)

    def condition(self, xf_out, lengths, seeds, fresh, c, first_frames=None):
        assert tuple(xf_out.shape)[0] == self.batch and len(lengths) == len(seeds) == len(fresh) == self.batch
        self.calls.append(('condition', [float(v) for v in xf_out[:, 0, 0]], list(lengths), list(seeds), list(fresh),
                           None if first_frames is None else list(first_frames), None if c is None else c.clone()))
        for b, f in enumerate(fresh):
            if f:
                first = 0 if first_frames is None else first_frames[b]
                self.x[b] = (1000.0 * seeds[b] + first + torch.arange(self.frames, dtype=torch.float64))[:, None]

    def seams(self, right, first_frame):
        self.calls.append(('seams', list(right), list(first_frame)))

    def clear_seams(self):
        self.calls.append(('clear_seams',))

    def advance(self, pos, scales):
        self.calls.append(('advance', [list(r) for r in pos], list(scales)))
        self.x += 0.001 * len(pos)

    def result(self):
        return self.x.clone()


def _req(i, length, c=None, edit=None):
    from motioncraft_amd.serve import Request
    return Request(length=length, seed=1 + i, xf_out=torch.full((4, 3), float(i + 1)), c=c, edit=edit)


def _kinds(r, kind):
    return [c for c in r.calls if c[0] == kind]


def _batcher(batch, steps=3, **kw):
    from motioncraft_amd.serve import ContinuousBatcher
    r = FakeRunner(steps, batch, T)
    return ContinuousBatcher(None, batch=batch, frames=T, steps=steps, runner=r, **kw), r


# ---- planning ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F, want', [
    (1, [(0, 1)]), (T, [(0, T)]),
    (T + 1, [(0, 6), (4, 3)]),                         # one frame over: a second, ragged window of ov + 1 frames
    (T + STRIDE, [(0, 6), (4, 6)]),                    # on the grid: F = T + (W - 1) stride
    (T + STRIDE + 1, [(0, 6), (4, 6), (8, 3)]),
    (T + 2 * STRIDE - 1, [(0, 6), (4, 6), (8, 5)]),
    (T + 2 * STRIDE, [(0, 6), (4, 6), (8, 6)]),
])
def test_plan_windows(F, want):
    from motioncraft_amd.serve import plan_windows
    got = plan_windows(F, T, OV)
    assert got == want
    if F > T:
        assert len(got) == -((OV - F) // STRIDE) and OV < got[-1][1] <= T and got[-1][0] + got[-1][1] == F
        assert all(f == j * STRIDE for j, (f, _) in enumerate(got))
    if F > T and (F - T) % STRIDE == 0:                # on the grid the plan is 4m's
        n, ff, frames = seam_ref.seam_plan(F, T, OV)
        assert (n, ff, frames) == (len(got), [f for f, _ in got], F)


def test_plan_windows_refuses_a_bad_overlap():
    from motioncraft_amd.serve import plan_windows
    for ov in (0, -1, T // 2 + 1):
        with pytest.raises(ValueError, match='overlap'):
            plan_windows(20, T, ov)


def test_constructor_and_submit_errors():
    from motioncraft_amd.serve import ContinuousBatcher, Edit
    for ov in (0, 4, -2, 1.5, True):
        with pytest.raises(ValueError, match='overlap'):
            ContinuousBatcher(None, batch=3, frames=T, steps=3, runner=FakeRunner(3, 3, T), overlap=ov)
    with pytest.raises(ValueError, match='seam_weights'):
        ContinuousBatcher(None, batch=3, frames=T, steps=3, runner=FakeRunner(3, 3, T), seam_weights=[0.5, 0.5])
    with pytest.raises(ValueError, match='seam_weights'):
        ContinuousBatcher(None, batch=3, frames=T, steps=3, runner=FakeRunner(3, 3, T), overlap=OV, seam_weights=[0.5, 1.5])
    bt, r = _batcher(3, overlap=OV)
    with pytest.raises(ValueError, match='4 windows'):                   # W > batch
        bt.submit(_req(0, T + 3 * STRIDE))
    assert bt.submit(_req(0, T + 2 * STRIDE)) == 0                        # W == batch is served
    e = Edit.keyframes(torch.zeros(3, 2), [0])
    with pytest.raises(ValueError, match='edit'):
        bt.submit(_req(1, T + 1, edit=e))
    with pytest.raises(ValueError, match='rows per frame'):
        bt.submit(_req(1, 10, c=torch.zeros(25, 3)))


def test_without_overlap_everything_is_as_before():
    bt, r = _batcher(3)
    with pytest.raises(ValueError, match=f'request of {T + 1} frames in a batcher of {T}'):
        bt.submit(_req(0, T + 1))
    h = [bt.submit(_req(i, 3 + i)) for i in range(2)]
    out = bt.run()
    assert sorted(out) == h and [tuple(out[k].shape) for k in h] == [(3, 2), (4, 2)]
    assert not _kinds(r, 'seams') and not _kinds(r, 'clear_seams')
    assert all(c[5] is None for c in _kinds(r, 'condition'))              # no first_frames argument was ever passed
    # ... and with overlap set, short requests alone see the same calls
    bt2, r2 = _batcher(3, overlap=OV)
    for i in range(2):
        bt2.submit(_req(i, 3 + i))
    out2 = bt2.run()
    assert all(torch.equal(out[k], out2[k]) for k in h) and [c[:6] for c in r.calls] == [c[:6] for c in r2.calls]


# ---- admission, the table, retirement, the stitch ---------------------------------------------------------------------------------
def test_fifo_admission_into_non_contiguous_rows_table_resent_and_stitch():
    """batch 4, walk 4, one step per round.  Three short requests are admitted one round apart, so their rows open one round apart.
    Behind them wait w2 (W = 2), w3 (W = 3) and a short request s, in this order:
      round 3: one row open (3): w2 waits, and with it everyone behind; row 0 retires at the end
      round 4: rows 0 and 3 open: w2 takes exactly those -- not contiguous, right[0] = 3 -- and the table is sent; row 1 retires
      rounds 5, 6: one, then two rows open: w3 waits for three, and s does NOT overtake it; row 2 retires in round 5
      round 7: w2 retires: the table is re-sent -- no long request runs, so it is cleared
      round 8: w3 takes rows 0, 1, 2 and s row 3; the table is sent again; both retire in round 11, and it is cleared again"""
    bt, r = _batcher(4, steps=4, overlap=OV)
    h0 = bt.submit(_req(0, 3))
    assert bt.tick() == 1
    h1 = bt.submit(_req(1, 3))
    assert bt.tick() == 1
    h2 = bt.submit(_req(2, 3))
    assert bt.tick() == 1 and bt.occupied == [h0, h1, h2, None]          # at walk positions 3, 2, 1
    F2, F3 = T + STRIDE, T + 2 * STRIDE - 1                               # 10 frames on the grid; 13 frames: windows of 6, 6, 5
    w2, w3, s = bt.submit(_req(5, F2)), bt.submit(_req(6, F3)), bt.submit(_req(7, 2))
    n_cond = len(_kinds(r, 'condition'))
    assert bt.tick() == 1 and bt.occupied == [None, h1, h2, None]        # round 3
    assert len(_kinds(r, 'condition')) == n_cond and not _kinds(r, 'seams')
    assert bt.tick() == 1 and bt.occupied == [w2, None, h2, w2]          # round 4
    cond = _kinds(r, 'condition')[-1]
    assert cond[1] == [6.0, 2.0, 3.0, 6.0]                                # xf_out repeated per window
    assert cond[2] == [T, 3, 3, T] and cond[3] == [6, 2, 3, 6] and cond[4] == [True, False, False, True] and cond[5] == [0, 0, 0, STRIDE]
    assert [c for c in r.calls if c[0] in ('seams', 'clear_seams')] == [('seams', [3, -1, -1, -1], [0, 0, 0, STRIDE])]
    assert r.calls[-2][0] == 'seams' and r.calls[-1] == ('advance', [[0, 3, 2, 0]], [None] * 4)      # the table is up before the step
    assert bt.tick() == 1 and bt.occupied == [w2, None, None, w2]        # round 5
    assert bt.tick() == 1 and bt.occupied == [w2, None, None, w2]        # round 6: two rows open, w3 needs three, s stays behind it
    assert r.calls[-1] == ('advance', [[2, 0, 0, 2]], [None] * 4)        # the rows of w2 walk together
    assert bt.tick() == 1 and bt.occupied == [None] * 4                   # round 7
    assert r.calls[-1] == ('clear_seams',)
    out = bt.poll()
    assert tuple(out[w2].shape) == (F2, 2)
    assert torch.allclose(out[w2][:, 0], 6000.0 + torch.arange(F2, dtype=torch.float64) + 0.004, rtol=0, atol=1e-9)
    assert bt.tick() == 1 and bt.occupied == [w3, w3, w3, s]             # round 8
    cond = _kinds(r, 'condition')[-1]
    assert cond[2] == [T, T, 5, 2] and cond[3] == [7, 7, 7, 8] and cond[5] == [0, STRIDE, 2 * STRIDE, 0]
    assert r.calls[-2] == ('seams', [1, 2, -1, -1], [0, STRIDE, 2 * STRIDE, 0])
    out = bt.run()
    assert bt.finished_at[w2] == 8 and bt.finished_at[w3] == bt.finished_at[s] == 12
    assert tuple(out[w3].shape) == (F3, 2) and tuple(out[s].shape) == (2, 2)
    assert torch.allclose(out[w3][:, 0], 7000.0 + torch.arange(F3, dtype=torch.float64) + 0.004, rtol=0, atol=1e-9)
    assert [c[0] for c in r.calls if c[0] in ('seams', 'clear_seams')] == ['seams', 'clear_seams', 'seams', 'clear_seams']


def test_a_second_long_request_joins_a_running_one_and_the_table_holds_both():
    bt, r = _batcher(4, steps=3, overlap=OV)
    a = bt.submit(_req(0, T + 1))                                         # W = 2, ragged: 6 + 3 frames
    assert bt.tick() == 1 and bt.occupied == [a, a, None, None]
    b = bt.submit(_req(1, T + STRIDE))
    assert bt.tick() == 1 and bt.occupied == [a, a, b, b]
    assert _kinds(r, 'seams') == [('seams', [1, -1, -1, -1], [0, STRIDE, 0, 0]), ('seams', [1, -1, 3, -1], [0, STRIDE, 0, STRIDE])]
    assert bt.tick() == 1 and bt.occupied == [None, None, b, b]          # a retires: the table goes on with b alone
    assert r.calls[-1] == ('seams', [-1, -1, 3, -1], [0, 0, 0, STRIDE])
    out = bt.run()
    assert tuple(out[a].shape) == (T + 1, 2) and tuple(out[b].shape) == (T + STRIDE, 2) and r.calls[-1] == ('clear_seams',)


def test_rows_of_a_request_advance_and_retire_together_and_control_is_sliced():
    bt, r = _batcher(3, steps=2, overlap=OV)
    F = T + STRIDE + 1                                                    # 11 frames, W = 3, last window 3 frames
    per = 2                                                               # control rows per frame
    c = torch.arange(F * per * 3, dtype=torch.float32).view(F * per, 3)
    h = bt.submit(_req(0, F, c=c))
    assert bt.tick(5) == 2                                                # clipped to the walk
    cond = _kinds(r, 'condition')[0]
    cc = cond[6]
    assert tuple(cc.shape) == (3, T * per, 3)
    assert torch.equal(cc[0], c[:T * per]) and torch.equal(cc[1], c[STRIDE * per:(STRIDE + T) * per])
    assert torch.equal(cc[2][:3 * per], c[2 * STRIDE * per:]) and not bool(cc[2][3 * per:].any())     # the ragged window: zero rows behind it
    assert _kinds(r, 'advance')[0][1] == [[0, 0, 0], [1, 1, 1]]
    out = bt.poll()
    assert tuple(out[h].shape) == (F, 2) and bt.occupied == [None] * 3
    assert [c_[0] for c_ in r.calls if c_[0] in ('seams', 'clear_seams')] == ['seams', 'clear_seams']
    assert _kinds(r, 'seams')[0] == ('seams', [1, 2, -1], [0, STRIDE, 2 * STRIDE])


def test_stitch_takes_stride_frames_of_every_window_but_the_last():
    bt, _ = _batcher(3, overlap=OV)
    wins = [torch.full((T, 1), float(j)) for j in range(3)]
    got = bt._stitch(wins, 2 * STRIDE + 3)[:, 0].tolist()
    assert got == [0.0] * STRIDE + [1.0] * STRIDE + [2.0] * 3


# ---- the fp64 restatement ---------------------------------------------------------------------------------------------------------
# The three test_reference_* tests below check tests/seam_rows_ref.py against tests/seam_ref.py and against itself: sanity of the
# restatement the GPU tests lean on.  They pin nothing in the package (and pass without it); the test right below ties the two together.
def test_every_table_the_batcher_sends_passes_the_reference_plan_rules():
    """the tables ``_send_seams`` builds for staggered long requests on scattered rows are tables ``seam_rows_ref.plan_rows`` (= the
    library's rules) accepts, and their chains are the requests' ``plan_windows``"""
    from motioncraft_amd.serve import plan_windows
    bt, r = _batcher(6, steps=5, overlap=OV)
    lengths = {}
    for i, (F, at) in enumerate([(3, 0), (T + 2 * STRIDE - 1, 0), (2, 1), (T + STRIDE, 2), (T + 1, 3), (T + 3 * STRIDE, 4)]):
        while bt.ticks < at:
            bt.tick()
        lengths[bt.submit(_req(i, F))] = F
    done = bt.run()
    sent = _kinds(r, 'seams')
    for _, right, first in sent:
        rows = SR.plan_rows(right, first, T, OV)                           # raises for a table the rules refuse
        heads = [b for b, (rt, left, _) in enumerate(rows) if rt >= 0 and not left]
        assert heads and all(rt >= 0 or left or f == 0 for rt, left, f in rows)
        for b in heads:                                                   # walk every chain: its first frames are one request's windows
            chain, v = [], b
            while v >= 0:
                chain.append(rows[v][2])
                v = rows[v][0]
            assert any([f for f, _ in plan_windows(F, T, OV)] == chain for F in lengths.values() if F > T), chain
    # req1 alone; req3 + req4 admitted in one round (one table holding two chains); req5 alone -- each batch retires together
    assert [c[0] for c in r.calls if c[0] in ('seams', 'clear_seams')] == ['seams', 'clear_seams'] * 3
    assert sum(1 for rt in sent[1][1] if rt >= 0) == 2                     # two chains of two windows in one table
    assert sorted(done) == sorted(lengths) and all(done[h].shape[0] == F for h, F in lengths.items())


def test_reference_plan_and_blend_agree_with_the_adjacent_form():
    """adjacent neighbours in row order: seam_rows_ref is seam_ref"""
    rs = np.random.RandomState(0)
    B, C = 4, 5
    ff = [0, 4, 12, 16]
    flags = seam_ref.plan_flags(ff, T, OV)
    right = [b + 1 if flags[b][1] else -1 for b in range(B)]
    rows = SR.plan_rows(right, ff, T, OV)
    assert [(l, r >= 0) for r, l, _ in rows] == flags
    x0 = rs.standard_normal((B, T, C))
    assert np.array_equal(SR.blend(x0, rows, OV), seam_ref.blend(x0, flags, OV))
    z = rs.standard_normal((B, T, C))
    assert np.array_equal(SR.share_left(z, rows, OV), seam_ref.share_left(z, flags, OV))


def test_reference_refuses_what_the_library_refuses():
    good = ([2, -1, 1], [0, 8, 4])
    assert [r for r, _, _ in SR.plan_rows(*good, T, OV)] == [2, -1, 1]
    bad = [([0, -1, -1], [0, 0, 0]),            # right[b] == b
           ([2, 2, -1], [0, 0, 4]),             # row 2 named twice
           ([1, -1, -1], [0, 5, 0]),            # not one stride apart
           ([1, 0, -1], [0, 4, 0]),             # a cycle (also breaks the stride rule)
           ([3, -1, -1], [0, 4, 0]),            # out of range
           ([1, -1, -1], [-4, 0, 0])]           # negative first frame
    for right, ff in bad:
        with pytest.raises(ValueError):
            SR.plan_rows(right, ff, T, OV)
    with pytest.raises(ValueError):
        SR.plan_rows(*good, T, 4)
    with pytest.raises(ValueError):
        SR.blend(np.zeros((3, T, 1)), SR.plan_rows(*good, T, OV), OV, w=[0.5, 1.5])


def test_reference_global_counters():
    """element r of a row at first frame f is element f C + r of the request's field; shared frames coincide"""
    C = 263
    rows = SR.plan_rows([2, -1, 1], [0, 8, 4], T, OV)
    g = SR.global_index(rows, T, C)
    assert g.shape == (3, T * C) and g.dtype == np.int64
    assert np.array_equal(g[0, STRIDE * C:], g[2, :OV * C]) and np.array_equal(g[2, STRIDE * C:], g[1, :OV * C])
    big = SR.global_index(SR.plan_rows([-1], [8_170_000], T, OV), T, C)
    assert int(big[0, 0]) == 8_170_000 * 263 > 2 ** 31

"""Host: edits on long requests in ``serve.ContinuousBatcher(overlap=, long_edits=True)`` through a fake runner
whose uploads go through the real ``serve._RowsRunner._upload_edits`` -- the window slices of an edit, equal entries on both copies of a
shared frame, no exclusion wait, the table cleared with the last edited row -- and ``long_edits=False`` behaving exactly as before."""
import types

import numpy as np
import pytest
import torch

import seam_edit_rows_ref as SE
import seam_rows_ref as SR
from test_edit_host import FlagOnlyContext
from test_seam_rows_host import FakeRunner, OV, STRIDE, T

C = 2


class LongEditRunner(FakeRunner):
    """the fake runner of the long-request tests plus an edit table kept by the real upload code in a FlagOnlyContext"""

    def __init__(self, steps, batch, frames):
        from motioncraft_amd import serve
        super().__init__(steps, batch, frames, C)
        net = types.SimpleNamespace(dims=dict(input_feats=C), pre_process=lambda m: 2.0 * m)      # (a visible normalisation)
        self.rows = object.__new__(serve._RowsRunner)
        self.rows.o = types.SimpleNamespace(batch=batch, frames=frames, model=types.SimpleNamespace(model=net))
        self.rows.ctx = FlagOnlyContext(batch, frames, C)
        self.table_right = None

    def condition(self, xf_out, lengths, seeds, fresh, c, edits=None, first_frames=None):
        super().condition(xf_out, lengths, seeds, fresh, c, first_frames=first_frames)
        if edits is not None:
            self.calls.append(('edits', list(fresh), [e is not None for e in edits], None if first_frames is None else list(first_frames)))
            self.rows._upload_edits(edits, fresh, 'cpu', first_frames)

    def clear_edits(self):
        self.calls.append(('clear_edits',))
        self.rows.clear_edits()

    def seams(self, right, first_frame):
        super().seams(right, first_frame)
        self.table_right = list(right)

    def clear_seams(self):
        super().clear_seams()
        self.table_right = None


def _req(i, length, edit=None):
    from motioncraft_amd.serve import Request
    return Request(length=length, seed=1 + i, xf_out=torch.full((4, 3), float(i + 1)), edit=edit)


def _edit(n, frames, seed=0, channels=None):
    """keyframes ``frames`` of an n-frame motion on all channels (or ``channels``); motion seeded, distinct per element"""
    from motioncraft_amd.serve import Edit
    motion = torch.randn(n, C, generator=torch.Generator().manual_seed(seed))
    keep = torch.zeros(n, C, dtype=torch.bool)
    for f in frames:
        keep[f, slice(None) if channels is None else channels] = True
    return Edit(motion, keep)


def _batcher(batch, steps=3, **kw):
    from motioncraft_amd.serve import ContinuousBatcher
    r = LongEditRunner(steps, batch, T)
    return ContinuousBatcher(None, batch=batch, frames=T, steps=steps, runner=r, **kw), r


def _kinds(r, kind):
    return [c for c in r.calls if c[0] == kind]


# ---- Edit.tables: the window form -------------------------------------------------------------------------------------------------
def test_window_slices_of_an_edit_offsets_ragged_end_and_frames_past_n_free():
    from motioncraft_amd.serve import plan_windows
    n = 11                                                                # the edit holds 11 frames of a 13-frame request
    e = _edit(n, [0, 4, 5, 9, 10], seed=3)
    pre = lambda m: 2.0 * m + 1.0
    whole_gt, whole_kp = e.tables(13, pre)
    assert torch.equal(e.tables(T, pre)[0], e.tables(T, pre, 0)[0]) and torch.equal(e.tables(T, pre)[1], whole_kp[:T])     # first_frame 0 = the old form
    wins = plan_windows(13, T, OV)
    assert wins == [(0, 6), (4, 6), (8, 5)]
    ref_gt, ref_kp = SE.window_tables(whole_gt[:n].numpy(), whole_kp[:n].numpy(), [f for f, _ in wins], T)
    for j, (f, _) in enumerate(wins):
        gt, kp = e.tables(T, pre, f)
        assert tuple(gt.shape) == (T, C) and kp.dtype == torch.uint8
        assert np.array_equal(kp.numpy() != 0, ref_kp[j])
        assert np.array_equal(gt.numpy()[ref_kp[j]], ref_gt[j][ref_kp[j]])          # model space, where kept
        assert not bool(kp[max(0, n - f):].any())                           # frames past the edit's n: free
    assert bool(e.tables(T, pre, 8)[1][:3].any()) and not bool(e.tables(T, pre, 8)[1][3:].any())
    assert not bool(e.tables(T, pre, n)[1].any()) and not bool(e.tables(T, pre, 40)[1].any())      # a window wholly past the edit
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match='first_frame'):
            e.tables(T, pre, bad)


# ---- the constructor and submit ---------------------------------------------------------------------------------------------------
def test_long_edits_needs_overlap_and_false_keeps_the_value_error():
    from motioncraft_amd.serve import ContinuousBatcher
    with pytest.raises(ValueError, match='long_edits'):
        ContinuousBatcher(None, batch=3, frames=T, steps=3, runner=LongEditRunner(3, 3, T), long_edits=True)
    bt, _ = _batcher(3, overlap=OV)
    assert bt.long_edits is False
    with pytest.raises(ValueError, match='edits on long requests are not served'):
        bt.submit(_req(0, T + 1, edit=_edit(3, [0])))
    bt, _ = _batcher(3, overlap=OV, long_edits=True)
    assert bt.submit(_req(0, T + 1, edit=_edit(3, [0]))) == 0
    with pytest.raises(ValueError, match='4 windows'):                   # the other submit checks stand
        bt.submit(_req(1, T + 3 * STRIDE, edit=_edit(3, [0])))


# ---- uploads: every window its slice, both copies of a shared frame equal -----------------------------------------------------------
def test_window_rows_are_uploaded_with_their_slices_and_shared_frames_agree():
    """batch 4: a short request runs in row 0; the long edited request (13 frames: windows 6, 6, 5; the edit holds 11) takes rows
    1, 2, 3 one round later.  Keyframes on shared frames (4, 5 and 9) and off them, plus one channel of frame 7."""
    bt, r = _batcher(4, steps=3, overlap=OV, long_edits=True)
    s = bt.submit(_req(0, 3))
    assert bt.tick() == 1
    e = _edit(11, [0, 4, 5, 9, 10], seed=5)
    e.keep[7, 1] = True
    h = bt.submit(_req(1, 13, edit=e))
    assert bt.tick() == 1 and bt.occupied == [s, h, h, h]
    up = _kinds(r, 'edits')
    assert up == [('edits', [False, True, True, True], [False, True, True, True], [0, 0, STRIDE, 2 * STRIDE])]
    ctx = r.rows.ctx
    assert ctx.uploads == [None]                                          # no table was set: every row is sent, the short one with nothing kept
    assert not bool(ctx.keep[0].any())
    gt, kp = ctx.gt, ctx.keep != 0
    for j, b in enumerate((1, 2, 3)):
        want_gt, want_kp = e.tables(T, lambda m: 2.0 * m, j * STRIDE)
        assert torch.equal(kp[b], want_kp != 0) and torch.equal(gt[b], want_gt)
    rows = SR.plan_rows(r.table_right, [0, 0, STRIDE, 2 * STRIDE], T, OV)
    assert SR.pairs(rows) == [(1, 2), (2, 3)]
    for l, rr in SR.pairs(rows):                                          # the two copies of every shared frame: equal keep / gt
        assert torch.equal(kp[l, T - OV:], kp[rr, :OV]) and torch.equal(gt[l, T - OV:], gt[rr, :OV])
    assert bool(kp[1, T - OV:].all()) and bool(kp[2, T - OV + 1].all()) and not bool(kp[2, T - OV].any())     # frames 4, 5 | 9 kept, 8 free
    assert kp[2, 3].tolist() == [False, True]                             # frame 7, channel 1
    assert not bool(kp[3, 3:].any())                                      # frames 11, 12 (past the edit) and the ragged rest: free
    # the order of the calls of the admission round: condition (with the upload), then the seam table, then the step
    names = [c[0] for c in r.calls]
    k = len(names) - 1 - names[::-1].index('edits')
    assert names[k - 1] == 'condition' and names[k + 1:k + 3] == ['seams', 'advance']
    out = bt.run()
    assert tuple(out[h].shape) == (13, C) and tuple(out[s].shape) == (3, C)
    assert r.calls[-2:] == [('clear_seams',), ('clear_edits',)] or r.calls[-2:] == [('clear_edits',), ('clear_seams',)]
    assert not ctx.edit_rows and r.table_right is None


# ---- admission --------------------------------------------------------------------------------------------------------------------
def _admission(long_edits):
    """batch 4, walk 4.  A short edited request E runs; a long request L (W = 2) is submitted one round later, then a short
    edited request E2 while L runs.  -> (rounds at which L and E2 were admitted, the batcher, the runner)"""
    bt, r = _batcher(4, steps=4, overlap=OV, long_edits=long_edits)
    e = bt.submit(_req(0, 3, edit=_edit(2, [0])))
    assert bt.tick() == 1
    l = bt.submit(_req(1, T + STRIDE))
    started = {}
    e2 = None
    for rnd in range(1, 16):
        if l in bt.occupied and e2 is None:
            e2 = bt.submit(_req(2, 3, edit=_edit(2, [1])))
        if bt.tick() == 0:
            break
        for h in (l, e2):
            if h is not None and h in bt.occupied and h not in started:
                started[h] = rnd
        if e2 is not None and not bt._pending and not any(o is not None for o in bt.occupied):
            break
    bt.run()
    return started[l], started[e2], bt, r


def test_no_exclusion_wait_with_long_edits_and_exactly_the_old_waits_without():
    l_at, e2_at, bt, r = _admission(True)
    assert (l_at, e2_at) == (1, 2)                                        # L joins beside the edited row at once; E2 joins beside L at once
    assert bt.finished_at[1] == 1 + 4 and bt.finished_at[2] == 2 + 4
    l_at, e2_at, bt, r = _admission(False)
    assert (l_at, e2_at) == (4, 8)                                        # L waits for E (rounds 0-3) to retire, E2 for L (rounds 4-7)
    ups = _kinds(r, 'edits')
    assert all(c[3] is None for c in ups)                                 # and no upload ever carried first frames


def test_a_long_request_without_an_edit_beside_a_short_edited_one_keeps_its_calls():
    """co-residency: the long request's rows get nothing kept, the seam table stands, the edit table is cleared when the short
    edited request retires while the long one walks on"""
    bt, r = _batcher(4, steps=4, overlap=OV, long_edits=True)
    e = bt.submit(_req(0, 3, edit=_edit(2, [0])))
    assert bt.tick() == 1 and bt.tick() == 1
    l = bt.submit(_req(1, T + STRIDE))
    assert bt.tick() == 1 and bt.occupied == [e, l, l, None]
    assert _kinds(r, 'edits')[-1] == ('edits', [False, True, True, False], [True, False, False, False], [0, 0, STRIDE, 0])
    ctx = r.rows.ctx
    assert ctx.edit_rows and bool(ctx.keep[0].any()) and not bool(ctx.keep[1:].any())
    assert bt.tick() == 1 and bt.occupied == [None, l, l, None]          # E retires: the last edited row
    assert r.calls[-1] == ('clear_edits',) and not ctx.edit_rows and r.table_right == [-1, 2, -1, -1]
    bt.run()
    assert r.calls[-1] == ('clear_seams',) and r.calls.count(('clear_edits',)) == 1


def test_tables_are_cleared_after_the_last_edited_row_retires_and_set_again_later():
    bt, r = _batcher(3, steps=2, overlap=OV, long_edits=True)
    a = bt.submit(_req(0, T + 1, edit=_edit(T + 1, [0, T])))
    out = bt.run()
    assert tuple(out[a].shape) == (T + 1, C) and not r.rows.ctx.edit_rows and r.calls.count(('clear_edits',)) == 1
    b = bt.submit(_req(1, 3))                                             # no edit anywhere: no edits= call at all
    n = len(_kinds(r, 'edits'))
    bt.run()
    assert len(_kinds(r, 'edits')) == n
    c = bt.submit(_req(2, T + STRIDE, edit=_edit(3, [2])))
    bt.tick()
    assert r.rows.ctx.edit_rows and r.rows.ctx.uploads[-1] is None        # a table set again: every row is sent
    bt.run()
    assert not r.rows.ctx.edit_rows and r.calls.count(('clear_edits',)) == 2

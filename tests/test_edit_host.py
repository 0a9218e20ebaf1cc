"""Host: edited rows -- the fp64 restatement ``edit_ref`` against the oracle's pinned steps, the end-of-walk
coefficient facts the exactness argument rests on, ``serve.Edit`` / ``Request`` validation, the ``pre_process`` / ``post_process`` round
trip, both batchers through stub runners, and the argument handling of ``tools/sample.py --edit_npz``."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import edit_ref
from test_rowsteps_host import FakeRunner

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
RESPACINGS = ('ddim6', 'ddim10', 'ddim50', '6', '50', None)


def _diffusion(respace):
    from motioncraft_amd.diffusion import build_diffusion
    return build_diffusion(dict(BASE, respace=respace))


# ---- the restatement against the oracle ----------------------------------------------------------------
@pytest.mark.parametrize('i', [9, 4, 0])
def test_edit_ref_equals_the_oracles_repaint_step_without_blend(i):
    """mode 1 == O.ddim_step_repaint(add_blend=False) (pinned to the reference by tests/test_oracle.py), mode 0 == O.ddpm_step on
    x0 = where(keep, gt, x0_model): <= 1e-5"""
    from oracle import stmogen_oracle as O
    d = _diffusion('ddim10')
    sched = O.Schedule(1000, 'ddim10')
    g = torch.Generator().manual_seed(5 + i)
    Bn, Tn, C = 2, 6, 7
    x, x0m, nz, gt, z2 = (torch.randn(Bn, Tn, C, generator=g) for _ in range(5))
    keep = torch.rand(Bn, Tn, C, generator=g) < 0.4
    TC = Tn * C
    want, want0 = O.ddim_step_repaint(sched, i, x, x0m, nz, keep, gt, z2, overlap_len=3, add_blend=False, eta=0.0)
    c = d.step_coefs(i, 'ddim', 2.5, 0.0)
    gtn = gt.clone()
    gtn[~keep] = float('nan')
    got, got0 = edit_ref.edit_rows(x, x0m, torch.zeros_like(x), nz, None, gtn, keep, z2, [c] * Bn, TC)
    assert np.abs(got - want.double().numpy().reshape(-1)).max() <= 1e-5 and np.abs(got0 - want0.double().numpy().reshape(-1)).max() <= 1e-6
    sched_p = O.Schedule(1000, '10')
    dp = _diffusion('10')
    c = dp.step_coefs(i, 'ddpm', 2.5)
    want = O.ddpm_step(sched_p, i, x, torch.where(keep, gt, x0m), nz)
    got, _ = edit_ref.edit_rows(x, x0m, torch.zeros_like(x), nz, None, gtn, keep, None, [c] * Bn, TC)
    assert np.abs(got - want.double().numpy().reshape(-1)).max() <= 1e-5


def test_edit_ref_mode_2_stores_the_edited_x0():
    d = _diffusion('ddim6')
    walk = d.multistep_coefs([5, 4, 3, 2, 1, 0], 2.5, 2)
    g = torch.Generator().manual_seed(8)
    x, a, hist, gt = (torch.randn(12, generator=g).double().numpy() for _ in range(4))
    keep = np.arange(12) % 3 == 0
    c = walk[2]
    got, x0 = edit_ref.edit_rows(x, a, np.zeros(12), None, hist, gt, keep, None, [c], 12)
    assert np.array_equal(x0[keep], gt[keep]) and np.array_equal(x0[~keep], a[~keep])
    assert np.allclose(got, float(c.eta) * hist + float(c.c2) * x + float(c.c1) * x0, rtol=0, atol=1e-12)


# ---- exactness at the end of a walk ---------------------------------------------------------------------------
@pytest.mark.parametrize('respace', RESPACINGS, ids=[str(r) for r in RESPACINGS])
def test_final_step_coefficients_make_the_kept_region_exact(respace):
    """schedule index 0 in fp32: c1 = 1, c2 = 0, nonzero = 0, ab_prev = 1; the multistep entry is (kx, k0, k1) = (0, 1, 0).  Hence
    DDPM: x_prev = fma(0, z, fma(0, x, 1 g)) = g;  DDIM kept: fma(sqrt(1), g, sqrt(0) z2) = g;  2M: fma(0, hist, fma(0, x, 1 g)) = g --
    bit for bit wherever z2, x and hist are finite."""
    d = _diffusion(respace)
    one, zero = np.float32(1.0), np.float32(0.0)
    for mode in ('ddpm', 'ddim'):
        c = d.step_coefs(0, mode, 2.5, 0.5 if mode == 'ddim' else 0.0)
        assert np.float32(c.nonzero) == zero and np.float32(c.ab_prev) == one
        if mode == 'ddpm':
            assert np.float32(c.c1) == one and np.float32(c.c2) == zero and np.isfinite(c.log_var)
    idx = list(range(d.num_timesteps))[::-1]
    if d.num_timesteps <= 50:                                  # (the multistep walk is a 10-50 step sampler)
        last = d.multistep_coefs(idx, 2.5, 2)[-1]
        assert (np.float32(last.c2), np.float32(last.c1), np.float32(last.eta)) == (zero, one, zero)


# ---- Edit / Request ----------------------------------------------------------------------------------------
def test_edit_validation_and_constructors():
    from motioncraft_amd.serve import Edit, Request
    from motioncraft_amd.synthetic import part_layout
    m = torch.randn(6, 322, generator=torch.Generator().manual_seed(1))
    k = torch.zeros(6, 322, dtype=torch.bool)
    with pytest.raises(ValueError, match='all False'):
        Edit(m, k)
    k[2, 5] = True
    bad = m.clone()
    bad[2, 5] = float('nan')
    with pytest.raises(ValueError, match='finite'):
        Edit(bad, k)
    bad = m.clone()
    bad[0, 0] = float('inf')                                  # not kept: allowed, and never uploaded
    gt, kp = Edit(bad, k).tables(8)
    assert bool(torch.isfinite(gt).all()) and tuple(gt.shape) == (8, 322) and kp.dtype == torch.uint8 and int(kp.sum()) == 1 and kp[2, 5] == 1
    for args in ((m, k.to(torch.uint8)), (m, k[:5]), (m[0], k[0]), (m.long(), k)):
        with pytest.raises(ValueError):
            Edit(*args)
    e = Edit.keyframes(m, [0, 5])
    assert e.keep[[0, 5]].all() and not e.keep[1:5].any() and e.frames == 6 and e.feats == 322
    for frames in ([6], [-1], [], [True]):
        with pytest.raises(ValueError):
            Edit.keyframes(m, frames)
    e = Edit.inbetween(m, 2, 1)
    assert e.keep[:, 0].tolist() == [True, True, False, False, False, True]
    for head, tail in ((0, 0), (4, 3), (-1, 2)):
        with pytest.raises(ValueError):
            Edit.inbetween(m, head, tail)
    names, channels, _ = part_layout('motionx')
    e = Edit.parts(m, ['lleg', 'root'], 'motionx', frames=[1, 2])
    cols = sorted(set(channels['lleg']) | set(channels['root']))
    assert e.keep[1].nonzero().view(-1).tolist() == cols and torch.equal(e.keep[1], e.keep[2]) and int(e.keep.sum()) == 2 * len(cols)
    assert bool(Edit.parts(m, 'lleg', 'motionx').keep[:, channels['lleg']].all())
    with pytest.raises(ValueError, match='parts'):
        Edit.parts(m, ['tail'], 'motionx')
    with pytest.raises(ValueError, match='channels'):
        Edit.parts(m[:, :100], ['lleg'], 'motionx')
    xf = torch.zeros(4, 3)
    assert Request(6, 1, xf_out=xf, edit=e).edit is e and Request(6, 1, xf_out=xf).edit is None
    with pytest.raises(ValueError, match='frames'):
        Request(5, 1, xf_out=xf, edit=e)
    with pytest.raises(ValueError, match='Edit'):
        Request(6, 1, xf_out=xf, edit=(m, k))
    # a wrong channel count is refused at submit, where the model is known
    from motioncraft_amd.serve import RequestBatcher
    model = types.SimpleNamespace(model=types.SimpleNamespace(dims=dict(input_feats=263)))
    with pytest.raises(ValueError, match='322 channels'):
        RequestBatcher(model, batch=1, frames=6, runner=lambda *a, **k: None).submit(Request(6, 1, xf_out=xf, edit=e))


def test_pre_process_inverts_post_process(tmp_path):
    """fp32: pre = fl(fl(m - mean) / fl(std + 1e-9)), post = fl(fl(q std) + mean) -- five roundings of relative size u = 2^-24, four of them
    on quantities of size |m - mean| and the last on the result, plus the 1e-9 in the divisor:
        |post(pre(m)) - m| <= |m - mean| (4 u + 1e-9 / std) + u |m|      (first order; x 1.01 for the products of two roundings)"""
    from motioncraft_amd.models import ControlT2MHalf, STMoGenTransformer
    g = torch.Generator().manual_seed(3)
    mean, std = torch.randn(322, generator=g) * 3, torch.rand(322, generator=g) * 1.9 + 0.1
    np.save(tmp_path / 'mean.npy', mean.numpy()), np.save(tmp_path / 'std.npy', std.numpy())
    net = types.SimpleNamespace(post_process_cfg=dict(mean_path=str(tmp_path / 'mean.npy'), std_path=str(tmp_path / 'std.npy')))
    m = torch.randn(40, 322, generator=g) * 5 + mean
    q = STMoGenTransformer.pre_process(net, m)
    want = ((m.double() - mean.double()) / (std.double() + 1e-9))
    assert float((q.double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())
    back = STMoGenTransformer.post_process(net, q)
    u = 2.0 ** -24
    bound = 1.01 * ((m - mean).abs().double() * (4 * u + 1e-9 / std.double()) + u * m.abs().double())
    assert bool(((back.double() - m.double()).abs() <= bound).all())
    plain = types.SimpleNamespace(post_process_cfg=None)
    assert STMoGenTransformer.pre_process(plain, m) is m
    wrapped = types.SimpleNamespace(base_model=types.SimpleNamespace(pre_process=lambda v: v + 1))
    assert torch.equal(ControlT2MHalf.pre_process(wrapped, m), m + 1)


# ---- the batchers through stub runners ------------------------------------------------------------------------
class EditRunner(FakeRunner):
    """FakeRunner that also keeps an edit table: rows -> the Edit uploaded for them (None: nothing kept)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.table = None

    def condition(self, xf_out, lengths, seeds, fresh, c, edits=None):
        super().condition(xf_out, lengths, seeds, fresh, c)
        if edits is not None:
            assert len(edits) == self.batch
            self.table = self.table or [None] * self.batch
            for b, f in enumerate(fresh):
                if f:
                    self.table[b] = edits[b]
            self.calls.append(('edits', list(fresh), [e is not None for e in edits]))

    def clear_edits(self):
        assert self.table is not None
        self.table = None
        self.calls.append(('clear_edits',))


def _req(i, length=3, edit=None):
    from motioncraft_amd.serve import Request
    return Request(length=length, seed=100 + i, xf_out=torch.full((4, 3), float(i + 1)), edit=edit)


def _edit(frames=2, C=2):
    from motioncraft_amd.serve import Edit
    return Edit.keyframes(torch.ones(frames, C), [0])


def test_continuous_batcher_uploads_edits_with_admissions_and_clears_the_table():
    from motioncraft_amd.serve import ContinuousBatcher
    r = EditRunner(4, 3, 6)
    bt = ContinuousBatcher(None, batch=3, frames=6, steps=4, runner=r)
    e0, e2 = _edit(), _edit(3)
    h0 = bt.submit(_req(0, edit=e0))
    h1 = bt.submit(_req(1))
    bt.tick()
    # first call: every row fresh -- row 0 its edit, row 1 (no edit) and row 2 (dummy) nothing kept
    assert r.calls[1] == ('edits', [True, True, True], [True, False, False]) and r.table == [e0, None, None]
    bt.tick()
    h2 = bt.submit(_req(2, edit=e2))
    bt.tick()                                                 # joins row 2 at tick 2: only that row is uploaded
    up = [c for c in r.calls if c[0] == 'edits']
    assert up[-1] == ('edits', [False, False, True], [True, False, True]) and r.table == [e0, None, e2]
    bt.tick()                                                 # rows 0, 1 end; row 2 (edited) still runs: the table stays
    assert sorted(bt.poll()) == [h0, h1] and r.table == [e0, None, e2] and ('clear_edits',) not in r.calls
    h3 = bt.submit(_req(3))                                   # admitted into row 0; stale row 1 becomes the dummy: both fresh, nothing kept
    bt.tick()
    up = [c for c in r.calls if c[0] == 'edits']
    assert up[-1] == ('edits', [True, True, False], [False, False, True]) and r.table == [None, None, e2]
    bt.tick()                                                 # row 2 ends: the last edited row retired
    assert h2 in bt.poll() and r.calls[-1] == ('clear_edits',) and r.table is None
    n_edits = len(up)
    rest = bt.run()                                           # the rest runs without an edits= argument
    assert h3 in rest and len([c for c in r.calls if c[0] == 'edits']) == n_edits and r.calls.count(('clear_edits',)) == 1
    # a later edit sets a table again
    bt.submit(_req(4, edit=e0))
    bt.run()
    assert r.calls.count(('clear_edits',)) == 2 and r.table is None


class FlagOnlyContext:
    """the edit tables of a context, in the WORST form a clear may take: mc_ctx_set_edit_rows(NULL, NULL) drops the flag and leaves
    the bytes (the library also zeroes the keep bytes; the runner must not depend on it).  ``kept()``: what the sampler would see."""

    def __init__(self, B, T, C):
        self.gt, self.keep, self.edit_rows, self.uploads = torch.zeros(B, T, C), torch.zeros(B, T, C, dtype=torch.uint8), False, []

    def set_edit_rows(self, gt, keep, fresh=None):
        for b in range(self.gt.shape[0]):
            if fresh is None or fresh[b]:
                self.gt[b], self.keep[b] = gt[b], keep[b]
        self.edit_rows = True
        self.uploads.append(None if fresh is None else list(fresh))

    def clear_edit_rows(self):
        self.edit_rows = False

    def kept(self):
        """per row: the value the kept region would force (None: nothing kept)"""
        out = []
        for b in range(self.gt.shape[0]):
            on = self.edit_rows and bool(self.keep[b].any())
            out.append(float(self.gt[b][self.keep[b] != 0][0]) if on else None)
        return out


class RowsEditRunner(FakeRunner):
    """FakeRunner whose edits go through the real serve._RowsRunner upload code into a FlagOnlyContext"""

    def __init__(self, steps, batch, frames, C=2):
        from motioncraft_amd import serve
        super().__init__(steps, batch, frames, C)
        net = types.SimpleNamespace(dims=dict(input_feats=C), pre_process=lambda m: m)
        self.rows = object.__new__(serve._RowsRunner)
        self.rows.o = types.SimpleNamespace(batch=batch, frames=frames, model=types.SimpleNamespace(model=net))
        self.rows.ctx = FlagOnlyContext(batch, frames, C)

    def condition(self, xf_out, lengths, seeds, fresh, c, edits=None):
        super().condition(xf_out, lengths, seeds, fresh, c)
        if edits is not None:
            self.rows._upload_edits(edits, fresh, 'cpu')

    def clear_edits(self):
        self.rows.clear_edits()


def test_a_retired_rows_kept_region_never_comes_back_on_a_request_without_an_edit():
    """batch 2, walk 4: A (edit) in row 0; P (none) joins row 1 two ticks later; A retires, the table is cleared; Q (none) takes row 0
    with no upload; P retires and R (edit) takes row 1, which sets a table again while Q is mid-walk.  After every round the sampler
    sees, per row, exactly the running request's own edit -- also when a clear only drops the flag."""
    from motioncraft_amd.serve import ContinuousBatcher, Edit
    r = RowsEditRunner(4, 2, 6)
    bt = ContinuousBatcher(None, batch=2, frames=6, steps=4, runner=r)
    ctx = r.rows.ctx
    ed = lambda v: Edit.keyframes(torch.full((2, 2), float(v)), [0])
    reqs = {}

    def submit(i, edit=None):
        reqs[bt.submit(_req(i, edit=edit))] = None if edit is None else float(edit.motion[0, 0])

    def check():
        want = [None if h is None else reqs[h] for h in bt.occupied]
        assert ctx.kept() == want, (bt.ticks, ctx.kept(), want)
    submit(0, ed(7))
    for k in range(8):
        if k == 2:
            submit(1)
        if k == 4:
            submit(2)
        if k == 6:
            submit(3, ed(9))
        assert bt.tick() == 1
        if k == 0:
            assert ctx.kept() == [7.0, None]
        if k == 3:
            assert ctx.kept() == [None, None] and not ctx.edit_rows      # A retired in this round: cleared
        if k in (4, 5):
            assert not ctx.edit_rows and bool(ctx.keep[0].any())         # Q walks in row 0 over A's stale bytes, the flag down
        if k == 6:
            assert bt.occupied[0] is not None and ctx.kept() == [None, 9.0]   # R's table is up; Q (row 0) sees nothing kept
            assert ctx.uploads[-1] is None                               # ... because every row was uploaded
        if k not in (3, 7):                                              # (rounds that retire the last edited row end with no table)
            check()
    # a second edit into a context that HOLDS a table uploads the fresh rows only
    r2 = RowsEditRunner(4, 2, 6)
    bt2 = ContinuousBatcher(None, batch=2, frames=6, steps=4, runner=r2)
    bt2.submit(_req(0, edit=ed(3)))
    bt2.tick()
    bt2.submit(_req(1, edit=ed(5)))
    bt2.tick()
    assert r2.rows.ctx.uploads == [None, [False, True]] and r2.rows.ctx.kept() == [3.0, 5.0]


def test_existing_stub_signatures_are_still_accepted():
    """no request with an edit: neither batcher passes edits= (the runners of the earlier host tests take none)"""
    from motioncraft_amd.serve import ContinuousBatcher, RequestBatcher
    r = FakeRunner(2, 2, 4)
    bt = ContinuousBatcher(None, batch=2, frames=4, steps=2, runner=r)
    hs = [bt.submit(_req(i)) for i in range(3)]
    assert sorted(bt.run()) == hs
    calls = []

    def runner(xf_out, lengths, seeds, c):
        calls.append(list(seeds))
        return torch.zeros(2, 4, 2)
    rb = RequestBatcher(None, batch=2, frames=4, runner=runner)
    hs = [rb.submit(_req(i)) for i in range(3)]
    assert sorted(rb.run()) == hs and len(calls) == 2


def test_request_batcher_passes_edits_only_for_batches_that_hold_one():
    from motioncraft_amd.serve import RequestBatcher
    calls = []

    def runner(xf_out, lengths, seeds, c, **kw):
        calls.append((list(seeds), kw))
        return torch.zeros(2, 4, 2)
    rb = RequestBatcher(None, batch=2, frames=4, runner=runner)
    e = _edit()
    for i, ed in enumerate([None, None, e]):
        rb.submit(_req(i, edit=ed))
    rb.run()
    assert calls[0] == ([100, 101], {}) and calls[1][0] == [102, 0] and calls[1][1] == dict(edits=[e, None])


# ---- tools/sample.py --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sample_tool():
    spec = importlib.util.spec_from_file_location('sample_tool', os.path.join(os.path.dirname(HERE), 'tools', 'sample.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sample_tool_edit_arguments(sample_tool, tmp_path):
    base = ['cfg.py', 'synthetic', '--text', 'a walk', '--motion_length', '8']
    a = sample_tool.parse_args(base + ['--edit_npz', 'e.npz', '--no_drop', '--keep_frames', '0-1,6', '--keep_parts', 'lleg,root'])
    sample_tool.check_edit_args(a)
    assert (a.edit_npz, a.keep_frames, a.keep_parts) == ('e.npz', '0-1,6', 'lleg,root')
    assert sample_tool.parse_frames('0-2, 5,7-7', 8) == [0, 1, 2, 5, 7]
    for spec in ('0-8', '3-1', 'a', '-1'):
        with pytest.raises(SystemExit):
            sample_tool.parse_frames(spec, 8)
    for extra in (['--repaint'], ['--overlap_len', '4'], ['--same_overlap_noisy'], ['--graph'], ['--clip_feat', 'f.npy']):
        with pytest.raises(SystemExit):
            sample_tool.check_edit_args(sample_tool.parse_args(base + ['--edit_npz', 'e.npz', '--no_drop'] + extra))
    with pytest.raises(SystemExit, match='no_drop'):
        sample_tool.check_edit_args(sample_tool.parse_args(base + ['--edit_npz', 'e.npz']))
    with pytest.raises(SystemExit, match='one sample'):
        sample_tool.check_edit_args(sample_tool.parse_args(['cfg.py', 'synthetic', '--text', 'a', 'b', '--motion_length', '8', '8',
                                                            '--edit_npz', 'e.npz', '--no_drop']))
    with pytest.raises(SystemExit, match='edit_npz'):
        sample_tool.check_edit_args(sample_tool.parse_args(base + ['--keep_frames', '0-1']))
    sample_tool.check_edit_args(sample_tool.parse_args(base))            # no edit: nothing to refuse
    # the file forms
    m = np.random.default_rng(0).standard_normal((6, 322)).astype(np.float32)
    keep = np.zeros((6, 322), dtype=bool)
    keep[0] = True
    np.savez(tmp_path / 'a.npz', motion=m, keep=keep)
    np.savez(tmp_path / 'b.npz', motion=m, keep_frames=np.array([0, 5]), keep_channels=np.array([3, 4]))
    np.savez(tmp_path / 'c.npz', motion=m)
    args = lambda f, *more: sample_tool.parse_args(base + ['--edit_npz', str(tmp_path / f), '--no_drop'] + list(more))
    e = sample_tool.load_edit(args('a.npz'), 'motionx', 322)
    assert torch.equal(e.keep, torch.from_numpy(keep)) and torch.equal(e.motion, torch.from_numpy(m))
    e = sample_tool.load_edit(args('b.npz'), 'motionx', 322)
    assert int(e.keep.sum()) == 4 and bool(e.keep[5, 4])
    e = sample_tool.load_edit(args('c.npz', '--keep_frames', '1-2', '--keep_parts', 'root'), 'motionx', 322)
    assert e.keep[1].any() and e.keep[2].any() and not e.keep[0].any()
    mean, std = np.full(322, 2.0, dtype=np.float32), np.full(322, 4.0, dtype=np.float32)
    e = sample_tool.load_edit(args('a.npz'), 'motionx', 322, mean, std)
    assert float((e.motion - torch.from_numpy((m - 2.0) / 4.0)).abs().max()) <= 1e-6
    for f, more in (('c.npz', ()), ('a.npz', ('--keep_parts', 'tail'))):
        with pytest.raises(SystemExit):
            sample_tool.load_edit(args(f, *more), 'motionx', 322)
    with pytest.raises(SystemExit, match='expected'):
        sample_tool.load_edit(args('a.npz'), 'human_ml3d', 263)

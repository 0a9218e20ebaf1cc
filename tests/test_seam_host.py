"""CPU: coupled windows of a long sequence -- the plan arithmetic (``longform.seam_plan`` / ``check_seams``), the fp64 restatement
``seam_ref.py`` on a toy denoiser, and the window driver ``longform.sample_long_coupled`` with the model replaced by a function of
the call's own inputs.  Nothing here touches the GPU; the device side is ``test_seam_gpu.py``."""
import numpy as np
import pytest
import torch

import seam_ref as S
from motioncraft_amd import longform
from motioncraft_amd.diffusion import build_diffusion

BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')

# (first_frame, T, ov): every rule of the plan broken once
BAD_PLANS = [([0, 3], 8, 2),              # partial overlap: 3 is neither +6 nor >= +8
             ([0, 7], 8, 2),              # partial overlap by one frame
             ([6, 0], 8, 2),              # decreasing
             ([0, 0], 8, 2),              # the same window twice
             ([-1, 5], 8, 2),             # negative entry
             ([0, 6, 11], 8, 2),          # the second pair is wrong
             ([0, 3], 8, 5),              # 2 ov > T: a frame would lie in three windows
             ([0, 8], 8, 0),              # no overlap is "clear", not a plan
             ([0, 9], 8, -1)]
GOOD_PLANS = [([0, 6, 12], 8, 2), ([0, 4, 8], 8, 4), ([0, 6, 14, 20], 8, 2), ([5], 8, 3), ([0, 8, 16], 8, 2), ([3, 9, 100], 8, 2)]


def _coefs(mode, n=5):
    """(schedule indices, StepCoefs) of the first n steps of a 10-step walk"""
    d = build_diffusion(dict(BASE, respace='ddim10'))
    idx = list(range(d.num_timesteps))[::-1]
    if mode == 'dpmpp':
        return idx[:n], d.multistep_coefs(idx, 6.5)[:n]
    return idx[:n], [d.step_coefs(i, mode, 6.5, eta=0.5 if mode == 'ddim' else 0.0) for i in idx[:n]]


def _toy_denoiser(x, b_of_row):
    """per-window x0 that depends on the window's own index and on the frame's position IN the window: neighbours disagree on their
    shared frames unless something couples them"""
    B, T, C = x.shape
    pos = np.arange(T, dtype=np.float64)[None, :, None] / T
    return np.tanh(0.7 * x + 0.3 * pos) + 0.05 * np.asarray(b_of_row, dtype=np.float64)[:, None, None]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('total,T,ov', [(60, 24, 6), (196 * 4, 196, 30), (24, 24, 6), (41, 24, 6), (42, 24, 6), (36, 24, 12), (100, 8, 1)])
def test_seam_plan_against_window_starts_and_stitch_lengths(total, T, ov):
    n, first, frames = longform.seam_plan(total, T, ov)
    n_ref, stride = longform.window_starts(total, T, ov)
    assert (n, first, frames) == S.seam_plan(total, T, ov)
    assert n == n_ref and first == [i * stride for i in range(n)] and stride == T - ov
    rec = longform.stitch_windows([np.zeros((T, 3), np.float32)] * n, ov, True)
    assert rec.shape[0] == frames == (n - 1) * stride + T <= total
    ff, w = longform.check_seams(first, T, ov, rows=n)
    assert ff == first and w is None
    flags = S.plan_flags(first, T, ov)
    assert [l for l, _ in flags] == [i > 0 for i in range(n)] and [r for _, r in flags] == [i < n - 1 for i in range(n)]


def test_seam_plan_refuses_what_it_cannot_cover():
    for total, T, ov in [(23, 24, 6), (60, 24, 13), (60, 24, 0)]:
        with pytest.raises(ValueError):
            longform.seam_plan(total, T, ov)


@pytest.mark.parametrize('ff,T,ov', BAD_PLANS)
def test_invalid_plans_are_rejected_before_the_library(ff, T, ov):
    """check_seams and the restatement refuse the same plans, and NativeContext.set_seams raises without a call into the library"""
    from motioncraft_amd.engine import NativeContext
    with pytest.raises(ValueError):
        S.plan_flags(ff, T, ov)
    with pytest.raises(ValueError):
        longform.check_seams(ff, T, ov)

    class Lib:
        calls = []

        def __getattr__(self, name):
            def f(*a):
                Lib.calls.append(name)
                return 0
            return f

    ctx = object.__new__(NativeContext)
    ctx.lib, ctx.B, ctx.T, ctx.handle, ctx._graph_state = Lib(), len(ff), T, None, None
    if ov == 0:          # overlap 0 is the "clear" call by definition: that one reaches the library, with no plan in it
        return
    with pytest.raises(ValueError):
        ctx.set_seams(ff, ov)
    assert Lib.calls == []
    ctx.handle = None


def test_other_argument_checks():
    for bad_w in ([0.5], [0.5, 1.5], [0.5, -0.1], [0.5, float('nan')]):
        with pytest.raises(ValueError):
            longform.check_seams([0, 6], 8, 2, weights=bad_w)
    with pytest.raises(ValueError):
        longform.check_seams([0, 6], 8, 2, rows=3)
    with pytest.raises(ValueError):
        longform.check_seams([], 8, 2)
    with pytest.raises(ValueError):
        longform.check_seams([0, 6.5], 8, 2)
    assert longform.check_seams([0, 6], 8, 2, weights=[0, 1], rows=2) == ([0, 6], [0.0, 1.0])


@pytest.mark.parametrize('ff,T,ov', GOOD_PLANS)
def test_valid_plans_agree_with_the_restatement(ff, T, ov):
    assert longform.check_seams(ff, T, ov)[0] == ff
    flags = S.plan_flags(ff, T, ov)
    for b in range(len(ff) - 1):
        assert flags[b][1] == flags[b + 1][0] == (ff[b + 1] - ff[b] == T - ov)
    assert not flags[0][0] and not flags[-1][1]


def test_default_weights():
    w = S.default_weights(6)
    assert w.shape == (6,) and np.all(np.diff(w) > 0) and 0 < w[0] and w[-1] < 1
    assert np.array_equal(w, np.asarray([(f + 1) / 7 for f in range(6)], dtype=np.float32).astype(np.float64))


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['ddpm', 'ddim', 'dpmpp'])
@pytest.mark.parametrize('ff,T,ov', [([0, 5, 10], 8, 3), ([0, 3, 6], 6, 3), ([0, 6, 14, 20], 8, 2)])
def test_restatement_keeps_seams_equal_over_a_walk(mode, ff, T, ov):
    """5 steps with a denoiser whose windows disagree on shared frames: x stays equal there after every step, in all three modes,
    with a middle row that has no interior (2 ov == T) and with two sequences in the batch -- and without the blend it does not"""
    C = 5
    flags = S.plan_flags(ff, T, ov)
    rng = np.random.default_rng(7)
    z = rng.standard_normal((max(ff) + T, C))
    x = S.gather_windows(z, ff, T)
    assert S.seams_equal(x, flags, ov)
    idx, coefs = _coefs(mode)
    x0_prev, x0_prev_plain, rows = None, None, np.arange(len(ff))
    x_plain = x.copy()
    for c in coefs:
        noise = rng.standard_normal(x.shape)             # NOT seam-consistent: the step takes the left row's
        x, x0 = S.step(c, x, _toy_denoiser(x, rows), flags, ov, noise=noise, x0_prev=x0_prev)
        assert S.seams_equal(x, flags, ov) and S.seams_equal(x0, flags, ov)
        x0_plain = _toy_denoiser(x_plain, rows)
        x_plain = S.update(c, x_plain, x0_plain, noise, x0_prev_plain)
        x0_prev, x0_prev_plain = x0, x0_plain
    assert not S.seams_equal(x_plain, flags, ov)


@pytest.mark.parametrize('mode', ['ddpm', 'ddim', 'dpmpp'])
def test_one_window_per_sequence_is_the_plain_update(mode):
    """rows that are all disjoint: no seam, the step is the plain update exactly"""
    T, ov, C = 8, 3, 4
    ff = [0, 8, 30]
    flags = S.plan_flags(ff, T, ov)
    assert flags == [(False, False)] * 3 and not S.seam_mask(flags, T, ov).any()
    rng = np.random.default_rng(1)
    x, x0w, noise, hp = (rng.standard_normal((3, T, C)) for _ in range(4))
    for c in _coefs(mode, 3)[1]:
        got, x0 = S.step(c, x, x0w, flags, ov, noise=noise, x0_prev=hp)
        assert np.array_equal(x0, x0w) and np.array_equal(got, S.update(c, x, x0w, noise, hp))


def test_blend_weights_and_mask():
    T, ov = 8, 3
    flags = S.plan_flags([0, 5, 10], T, ov)
    m = S.seam_mask(flags, T, ov)
    assert m.sum() == 4 * ov and m[1].tolist() == [True] * 3 + [False] * 2 + [True] * 3
    x0 = np.random.default_rng(2).standard_normal((3, T, 2))
    left, right = S.blend(x0, flags, ov, np.zeros(ov)), S.blend(x0, flags, ov, np.ones(ov))
    assert np.array_equal(left[1, :ov], x0[0, T - ov:]) and np.array_equal(right[0, T - ov:], x0[1, :ov])
    assert np.array_equal(left[~m], x0[~m]) and np.array_equal(right[~m], x0[~m])
    mid = S.blend(x0, flags, ov)
    lo, hi = np.minimum(x0[0, T - ov:], x0[1, :ov]), np.maximum(x0[0, T - ov:], x0[1, :ov])
    assert np.all(mid[0, T - ov:] >= lo) and np.all(mid[0, T - ov:] <= hi)          # convex


# ---- the driver -------------------------------------------------------------------------------------------------------------------
class CoupledFn:
    """stands in for the architecture: returns the x_T it was handed (seam-consistent by the driver's construction) plus a term of the
    window's own condition rows ON FRAMES NO OTHER WINDOW SHARES, and records how it was called"""

    def __init__(self, ov):
        self.calls, self.ov = [], ov

    def __call__(self, motion, motion_mask, motion_length, num_intervals, motion_metas, inference_kwargs, seams, c=None, xf_out=None, **kw):
        b, L, C = motion.shape
        x = inference_kwargs['noise']
        assert tuple(x.shape) == (b, L, C)
        self.calls.append(dict(b=b, seams=seams, text=[m['text'] for m in motion_metas], c=c, xf=xf_out, x=x.clone()))
        pred = x.clone()
        if c is not None:
            r = c.shape[1] // L
            pred[:, self.ov:L - self.ov] += c.view(b, L, r, -1).mean(dim=(2, 3))[:, self.ov:L - self.ov, None]
        return [{'pred_motion': pred[j]} for j in range(b)]


@pytest.mark.parametrize('r', [1, 3])
def test_driver_rows_chunks_noise_and_stitching(r):
    L, ov, C, F = 24, 6, 5, 4
    totals = [60, 24, 100, 45]                    # 3, 1, 5, 2 windows
    plans = [longform.seam_plan(t, L, ov) for t in totals]
    assert [p[0] for p in plans] == [3, 1, 5, 2]
    g = torch.Generator().manual_seed(5)
    cs = [torch.randn(t * r, F, generator=g) for t in totals]
    xf = torch.randn(4, 3, 2, generator=g)
    mean, std = torch.randn(C, generator=g).numpy(), (torch.rand(C, generator=g) + 0.5).numpy()
    fn = CoupledFn(ov)
    gen = torch.Generator().manual_seed(9)
    recs, wins = longform.sample_long_coupled(fn, totals, L, ov, c=cs, text=['a', 'b', 'c', 'd'], mean=mean, std=std, input_dim=C,
                                              device=torch.device('cpu'), condition_kwargs=dict(xf_out=xf),
                                              inference_kwargs=dict(generator=gen), max_batch=6, shard=False, c_rows_per_frame=r)
    # whole sequences per call, up to 6 windows: (3 + 1), (5), (2)
    assert [k['b'] for k in fn.calls] == [4, 5, 2]
    assert fn.calls[0]['text'] == ['a', 'a', 'a', 'b'] and fn.calls[1]['text'] == ['c'] * 5
    assert torch.equal(fn.calls[0]['xf'], xf[[0, 0, 0, 1]])
    stride = L - ov
    first0 = fn.calls[0]['seams']['first_frame']
    assert first0 == [0, stride, 2 * stride, plans[0][2]] and fn.calls[0]['seams']['overlap'] == ov
    for k in fn.calls:
        ff = k['seams']['first_frame']
        flags = S.plan_flags(ff, L, ov)                                      # the plan is one the rules accept ...
        assert S.seams_equal(k['x'].numpy(), flags, ov)                      # ... and x_T agrees on every shared frame
        assert longform.check_seams(ff, L, ov, rows=k['b'])[0] == ff
    # windows of one sequence: neighbours; the first window of the next sequence: disjoint
    assert S.plan_flags(first0, L, ov) == [(False, True), (True, True), (True, False), (False, False)]
    # the condition rows of window w are those of its frames
    w2 = fn.calls[1]['c'][2]
    assert torch.equal(w2, cs[2][2 * stride * r:(2 * stride + L) * r])
    for s, t in enumerate(totals):
        n, ff, frames = plans[s]
        assert recs[s].shape == (frames, C) and recs[s].dtype == np.float32
        ref = longform.stitch_windows([wins[(s, w)] for w in range(n)], ov, True, mean, std)
        assert np.array_equal(recs[s], ref)
        for w in range(n - 1):
            assert np.array_equal(wins[(s, w)][stride:], wins[(s, w + 1)][:ov])
    assert len(wins) == 11
    # the same generator seed: the same bits; explicit per-sequence noise: used as given
    fn2 = CoupledFn(ov)
    recs2, _ = longform.sample_long_coupled(fn2, totals, L, ov, c=cs, text=['a', 'b', 'c', 'd'], mean=mean, std=std, input_dim=C,
                                            device=torch.device('cpu'), condition_kwargs=dict(xf_out=xf),
                                            inference_kwargs=dict(generator=torch.Generator().manual_seed(9)), max_batch=6, shard=False,
                                            c_rows_per_frame=r)
    assert all(np.array_equal(a, b) for a, b in zip(recs, recs2))
    z = [torch.randn(p[2], C, generator=g) for p in plans]
    fn3 = CoupledFn(ov)
    longform.sample_long_coupled(fn3, totals, L, ov, text='t', noise=z, input_dim=C, device=torch.device('cpu'), max_batch=11, shard=False)
    assert [k['b'] for k in fn3.calls] == [11]
    assert torch.equal(fn3.calls[0]['x'][4 + 2], z[2][2 * stride:2 * stride + L])


def test_driver_errors():
    fn, dev = CoupledFn(6), torch.device('cpu')
    with pytest.raises(ValueError, match='max_batch'):
        longform.sample_long_coupled(fn, [100], 24, 6, input_dim=3, device=dev, max_batch=4, shard=False)
    with pytest.raises(ValueError, match='overlap'):
        longform.sample_long_coupled(fn, [100], 24, 13, input_dim=3, device=dev, shard=False)
    with pytest.raises(ValueError, match='shorter'):
        longform.sample_long_coupled(fn, [20], 24, 6, input_dim=3, device=dev, shard=False)
    with pytest.raises(ValueError, match='graph'):
        longform.sample_long_coupled(fn, [60], 24, 6, input_dim=3, device=dev, shard=False, inference_kwargs=dict(graph=True))
    with pytest.raises(ValueError, match='noise'):
        longform.sample_long_coupled(fn, [60], 24, 6, input_dim=3, device=dev, shard=False, noise=[torch.zeros(59, 3)])
    assert fn.calls == []

    class Uncoupled(CoupledFn):
        def __call__(self, **kw):
            out = super().__call__(**kw)
            out[1]['pred_motion'] = out[1]['pred_motion'] + 1.0
            return out

    with pytest.raises(RuntimeError, match='shared frames'):
        longform.sample_long_coupled(Uncoupled(6), [60], 24, 6, input_dim=3, device=dev, shard=False)


def test_loops_refuse_what_does_not_go_with_seams():
    """graph replay, outpainting and seeding are refused before any context is asked for"""
    d = build_diffusion(dict(BASE, respace='ddim10'))
    seams = dict(first_frame=[0, 18], overlap=6)
    kw = dict(seams=seams, y={})

    class NoModel:
        cfg_scale = 6.5

        def sampling_context(self, *a, **k):
            raise AssertionError('reached the context')

    for loop in (d.ddim_sample_loop, d.p_sample_loop, d.dpm_solver_sample_loop):
        with pytest.raises(ValueError, match='graph'):
            loop(NoModel(), (2, 24, 5), clip_denoised=False, model_kwargs=kw, graph=True)
        with pytest.raises(NotImplementedError):
            loop(NoModel(), (2, 24, 5), clip_denoised=False, model_kwargs=kw, pre_seq=torch.zeros(2, 2, 5))
        mask = torch.zeros(2, 24, 5, dtype=torch.bool)
        mask[:, :6] = True
        with pytest.raises(NotImplementedError):
            loop(NoModel(), (2, 24, 5), clip_denoised=False, model_kwargs=dict(seams=seams, y=dict(gt=torch.zeros(2, 24, 5), outpainting_mask=mask)))
    with pytest.raises(NotImplementedError):
        d.p_sample_loop(NoModel(), (2, 24, 5), clip_denoised=False, model_kwargs=kw, transl_req=[[0, 1.0, 2.0]])
    with pytest.raises(ValueError, match='seams'):
        d.ddim_sample_loop(NoModel(), (2, 24, 5), clip_denoised=False, model_kwargs=dict(seams=dict(first=[0]), y={}))


def test_speech_front_selects_the_driver(monkeypatch):
    from motioncraft_amd import speech
    seen = {}

    def driver(model, total, L, ov, **kw):
        seen.update(total=total, L=L, ov=ov, **kw)
        return 'coupled'

    monkeypatch.setattr(longform, 'sample_long_coupled', driver)
    cond = lambda wave: torch.zeros(40 * 3 + 2, 2)          # noqa: E731
    assert speech.sample_speech('m', None, words=['hi'], motion_length=16, pre_frames=4, samples_per_frame=3, condition=cond,
                                coupled=True, max_batch=8) == 'coupled'
    assert seen['total'] == [40] and (seen['L'], seen['ov']) == (16, 4) and seen['c_rows_per_frame'] == 3 and seen['max_batch'] == 8
    assert seen['text'] == [speech.speech_prompt(['hi'])] and len(seen['c']) == 1
    with pytest.raises(ValueError):
        speech.sample_speech('m', None, condition=cond, coupled=True, batched=True)

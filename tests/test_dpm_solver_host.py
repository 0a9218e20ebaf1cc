"""Host side of the multistep sampler (DPM-Solver++ 2M): coefficient tables, log-SNR spacing, accuracy on the closed-form problem and
the refusals of the loop -- against tests/dpm_solver_ref.py (fp64) and the DDIM tables that are pinned to the reference.  No GPU."""
import math

import numpy as np
import pytest
import torch

import dpm_solver_ref as R
from motioncraft_amd import lib as L_
from motioncraft_amd.diffusion import build_diffusion, logsnr_timesteps, space_timesteps

BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
SCALE = 6.5


def k64(d, indices, order):
    """the fp64 (kx, k0, k1) the package's fp32 tables are cast from: the restatement on the package's own alpha-bars"""
    return R.coef_table(d.alphas_cumprod, d.alphas_cumprod_prev, indices, order)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize('respace', ['ddim50', 'ddim20'])
def test_order1_is_ddim_eta0(respace):
    """order-1 (kx, k0) == DDIM eta = 0 rewritten as kx x + k0 x0 from the tables behind step_coefs(i, 'ddim'): to 1e-12 in fp64 at every
    index, and the fp32 struct fields are the casts of those."""
    d = build_diffusion(dict(BASE, respace=respace))
    idx = list(range(d.num_timesteps))[::-1]
    ks = k64(d, idx, 1)
    cs = d.multistep_coefs(idx, SCALE, order=1)
    for (kx, k0, k1), c, i in zip(ks, cs, idx):
        dd = d.step_coefs(i, 'ddim', SCALE, 0.0)
        # ddim_sample, eta = 0:  eps = (sr x - x0) / srm1;  x_prev = sqrt(abp) x0 + sqrt(1 - abp) eps
        sr, srm1 = d.sqrt_recip_alphas_cumprod[i], d.sqrt_recipm1_alphas_cumprod[i]
        abp = d.alphas_cumprod_prev[i]
        assert np.float32(abp) == np.float32(dd.ab_prev) and np.float32(sr) == np.float32(dd.sqrt_recip)      # (the tables step_coefs casts)
        dir_ = math.sqrt(1 - abp)
        kx_ddim, k0_ddim = dir_ * sr / srm1, math.sqrt(abp) - dir_ / srm1
        assert k1 == 0.0 and c.eta == 0.0
        if i == 0:
            assert (kx, k0) == (0.0, 1.0) and abs(kx_ddim) <= 1e-12 and rel(k0_ddim, 1.0) <= 1e-12
        else:
            assert rel(kx, kx_ddim) <= 1e-12 and rel(k0, k0_ddim) <= 1e-12, (i, kx, kx_ddim, k0, k0_ddim)
        assert c.mode == L_.MC_SAMPLER_MULTISTEP == 2
        assert (c.c2, c.c1) == (np.float32(kx), np.float32(k0))
        assert (c.text_coef, c.none_coef) == (dd.text_coef, dd.none_coef)


@pytest.mark.parametrize('respace', ['ddim50', 'ddim20', 'logsnr20', '15,15,8,6,6'])
def test_fixed_coefficients(respace):
    d = build_diffusion(dict(BASE, respace=respace))
    idx = list(range(d.num_timesteps))[::-1]
    cs = d.multistep_coefs(idx, SCALE, order=2)
    ks = k64(d, idx, 2)
    by_i = dict(zip(idx, cs))
    assert (by_i[0].c2, by_i[0].c1, by_i[0].eta) == (0.0, 1.0, 0.0)            # exactly x_prev = x0, no inf arithmetic
    assert cs[0].eta == 0.0 and by_i[1].eta == 0.0                            # no history / the lower-order final step
    assert all(c.eta != 0.0 for c in cs[1:-2])                                # every other step is second order
    for c, (kx, k0, k1) in zip(cs, ks):
        assert (c.c2, c.c1, c.eta) == (np.float32(kx), np.float32(k0), np.float32(k1))
        assert all(math.isfinite(v) for v in (c.c2, c.c1, c.eta))
    # truncated walks and walks that start elsewhere: k1 belongs to the sequence
    part = d.multistep_coefs(idx[3:8], SCALE)
    assert part[0].eta == 0.0 and part[1].eta == cs[4].eta
    with pytest.raises(ValueError):
        d.multistep_coefs(idx, SCALE, order=3)


def test_constant_h_coefficients_sum_to_order1():
    """for a constant step in lambda, k0 + k1 == -alpha_t expm1(-h) (the second-order correction redistributes, r = 1): 1e-12"""
    S, h = 12, 0.6
    lam = -4.0 + h * np.arange(S + 1)[::-1]                 # lam[j]: level j, decreasing with j; level 0 is the data end (dropped below)
    ab_full = 1.0 / (1.0 + np.exp(-2.0 * lam))              # alpha^2 = sigmoid(2 lambda)
    ab = ab_full[1:]
    ab_prev = ab_full[:-1].copy()
    idx = list(range(S))[::-1]
    ks = R.coef_table(ab, ab_prev, idx, 2, final_first_order=False)
    for (kx, k0, k1), i in zip(ks[1:], idx[1:]):
        a_t = math.sqrt(ab_prev[i])
        assert k1 != 0.0 and rel(k0 + k1, -a_t * math.expm1(-h)) <= 1e-12
        assert rel(k1, 0.5 * a_t * math.expm1(-h)) <= 1e-9
    # the package on the same levels (all S + 1 of them as a schedule: index 1 is first order there, index 0 is the (0, 1, 0) step)
    from motioncraft_amd.diffusion import GaussianDiffusion, ModelMeanType, ModelVarType
    d = GaussianDiffusion(betas=1.0 - ab_full / np.append(1.0, ab_full[:-1]), model_mean_type=ModelMeanType.START_X,
                          model_var_type=ModelVarType.FIXED_LARGE)
    walk = list(range(S + 1))[::-1]
    cs = d.multistep_coefs(walk, SCALE)
    for c, i in zip(cs[1:-2], walk[1:-2]):
        want = -math.sqrt(d.alphas_cumprod_prev[i]) * math.expm1(-h)
        assert c.eta != 0.0 and abs((float(c.c1) + float(c.eta)) - want) <= 3 * 2.0 ** -24 * 1.5 * abs(want)      # (three fp32 casts of values <= 1.5 |want|)


def test_logsnr_timesteps():
    ac = R.linear_alphas_cumprod(1000)
    lam = 0.5 * (np.log(ac) - np.log1p(-ac))
    for S in (2, 5, 10, 20, 50, 200):
        ts = logsnr_timesteps(1000, S)
        assert isinstance(ts, set) and 0 in ts and 999 in ts and len(ts) <= max(S, 2)
        srt = sorted(ts)
        assert srt == sorted(set(srt)) and all(0 <= t < 1000 for t in srt)
        assert all(lam[a] > lam[b] for a, b in zip(srt[:-1], srt[1:]))         # lambda monotone along the set
        assert ts == R.logsnr_timesteps(ac, S)
        if S >= 5:       # uniform in lambda up to the snapping: no gap above 1.5 x the ideal step (+ the coarsest local grid step)
            gaps = -np.diff(lam[srt])
            ideal = (lam[0] - lam[999]) / (S - 1)
            assert gaps.max() <= 1.5 * ideal + np.abs(np.diff(lam)).max()
    from motioncraft_amd.diffusion import get_named_beta_schedule
    assert logsnr_timesteps(get_named_beta_schedule('linear', 1000), 20) == logsnr_timesteps(1000, 20)
    assert len(logsnr_timesteps(1000, 2000)) <= 1000                 # fewer than S: several points snap to one timestep
    d = build_diffusion(dict(BASE, respace='logsnr20'))
    assert d.timestep_map == sorted(logsnr_timesteps(1000, 20)) and d.num_timesteps <= 20
    assert space_timesteps(1000, 'logsnr20') == logsnr_timesteps(1000, 20)
    # the existing strings are untouched
    assert space_timesteps(1000, 'ddim50') == set(range(0, 1000, 20))
    assert build_diffusion(dict(BASE, respace='15,15,8,6,6')).num_timesteps == 50


def test_restatement_loop_uses_the_package_tables():
    """the package's fp32 coefficients drive the same walk as the restatement's fp64 ones (a loop-level check of multistep_coefs)"""
    d = build_diffusion(dict(BASE, respace='ddim20'))
    idx = list(range(d.num_timesteps))[::-1]
    f = R.toy_predictor(1.0, d.alphas_cumprod)
    ref = R.loop(f, 1.0, d.alphas_cumprod, d.alphas_cumprod_prev, idx, 2)
    x, prev = 1.0, 0.0
    for c, i in zip(d.multistep_coefs(idx, SCALE, 2), idx):
        x0 = f(x, i)
        x, prev = c.c2 * x + c.c1 * x0 + c.eta * prev, x0
    assert abs(x - float(ref)) <= 1e-5


@pytest.mark.parametrize('spacing', ['time', 'logsnr'])
@pytest.mark.parametrize('s2', [0.25, 1.0, 4.0])
@pytest.mark.parametrize('S', [10, 20, 50])
def test_order2_beats_order1_on_the_closed_form_problem(spacing, s2, S):
    """Gaussian data N(0, s2), optimal predictor, exact probability-flow solution at alpha-bar = 1; linear 1000-step schedule.  A
    condition, not a tuned number: the second-order error is strictly below the first-order one in all 18 cases, on the PACKAGE's
    schedule and coefficients (and the restatement agrees with them)."""
    d = build_diffusion(dict(BASE, respace=f'ddim{S}' if spacing == 'time' else f'logsnr{S}'))
    idx = list(range(d.num_timesteps))[::-1]
    f = R.toy_predictor(s2, d.alphas_cumprod)
    exact = R.toy_exact(s2, d.alphas_cumprod[-1])
    err = {}
    for order in (1, 2):
        x, prev = 1.0, 0.0
        for c, i in zip(d.multistep_coefs(idx, SCALE, order), idx):
            x0 = f(x, i)
            x, prev = float(c.c2) * x + float(c.c1) * x0 + (float(c.eta) * prev if c.eta != 0.0 else 0.0), x0
        err[order] = abs(x - exact)
        assert abs(err[order] - R.toy_error(spacing, s2, S, order)) <= 1e-5
    print(f'{spacing} s2={s2} S={S}: order 1 {err[1]:.4f}  order 2 {err[2]:.4f}  ({err[1] / err[2]:.2f}x)')
    assert err[2] < err[1]


def test_plain_2m_without_the_final_rule_loses_at_few_steps():
    """why the lower-order final step is not optional: plain 2M is worse than first order somewhere at S <= 20 on the time spacing"""
    assert any(R.toy_error('time', s2, S, 2, final_first_order=False) > R.toy_error('time', s2, S, 1) for s2 in (0.25, 1.0) for S in (10, 20))


def test_sample_tool_sampler_options():
    """tools/sample.py: --sampler / --steps / --spacing -> cfg.model; the default keeps the config's choice; --repaint with dpmpp exits"""
    import argparse
    import importlib.util
    import os
    import motioncraft_amd as mc
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location('sample_tool', os.path.join(here, '..', 'tools', 'sample.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    def run(**kw):
        cfg = mc.Config.fromfile(os.path.join(here, 'configs', 'stmogen_small.py'))
        tool.apply_sampler(cfg, argparse.Namespace(**dict(dict(sampler=None, steps=None, spacing=None, repaint=False), **kw)))
        return cfg.model['inference_type'], cfg.model['diffusion_test']['respace']
    assert run() == ('ddim', '15,15,8,6,6')
    assert run(sampler='ddpm') == ('ddpm', '15,15,8,6,6')
    assert run(sampler='dpmpp') == ('dpmpp', '15,15,8,6,6')
    assert run(sampler='dpmpp', steps=20) == ('dpmpp', 'ddim20')
    assert run(sampler='dpmpp', steps=10, spacing='logsnr') == ('dpmpp', 'logsnr10')
    for bad in (dict(sampler='dpmpp', repaint=True), dict(sampler='ddim', steps=20), dict(steps=20), dict(sampler='dpmpp', spacing='logsnr'),
                dict(sampler='dpmpp', steps=1)):
        with pytest.raises(SystemExit):
            run(**bad)


def test_loop_refuses_outpainting_and_seeding():
    d = build_diffusion(dict(BASE, respace='ddim10'))
    shape = (1, 8, 322)

    class M:
        cfg_scale = SCALE

        def sampling_context(self, *a, **k):
            raise AssertionError('the refusal comes before any device work')
    keep = torch.zeros(shape, dtype=torch.bool)
    keep[:, :2] = True
    kw = dict(clip_denoised=False, device=torch.device('cpu'))
    with pytest.raises(NotImplementedError, match='outpainting'):
        d.dpm_solver_sample_loop(M(), shape, model_kwargs=dict(y=dict(outpainting_mask=keep, gt=torch.zeros(shape))), **kw)
    with pytest.raises(NotImplementedError, match='pre_seq'):
        d.dpm_solver_sample_loop(M(), shape, model_kwargs={}, pre_seq=torch.zeros(1, 2, 322), **kw)
    with pytest.raises(NotImplementedError, match='transl_req'):
        d.dpm_solver_sample_loop(M(), shape, model_kwargs={}, transl_req=[[0, 0.0, 0.0]], **kw)
    with pytest.raises(NotImplementedError):                     # the guard shared with the other two loops
        d.dpm_solver_sample_loop(M(), shape, model_kwargs={}, device=torch.device('cpu'))
    with pytest.raises(ValueError):
        d.dpm_solver_sample_loop(M(), shape, model_kwargs={}, order=3, **kw)

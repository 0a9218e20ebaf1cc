"""GPU (MI355X): the multistep sampler (DPM-Solver++ 2M, mode 2) -- sampler_multistep_k through the context-free op, the per-step loop,
the fused loop, graph replay and MotionDiffusion -- against tests/dpm_solver_ref.py (fp64) and the CPU oracle denoiser.

The reference has no such sampler, so nothing here is a golden of it: the update is pinned to the fp64 restatement applied to the
device's own operands (lockstep), the denoiser call to the oracle at the same x with the bound the fp32 path already carries.

Bound of one update per element (three fused operations on top of the two of the CFG combine, each rounding at most 2^-24 of the sum
of magnitudes it rounds, one spare):  4 * 2^-24 * (|kx x| + |k0 x0| + |k1 x0_prev| + |a w| + |b (1 - w)|)."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest
import torch

import dpm_solver_ref as R
from helpers import SMALL, SMALL_SEED, synth_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
EPS = 2.0 ** -24
TOL_STEP = 2e-4             # one denoiser call of the fp32 path against the oracle (tests/test_gpu_parity.py)
C = 322
CASES = {2: None, 3: [24, 19, 11]}          # batch -> valid lengths (None: full)


@pytest.fixture(autouse=True)
def time_limit():
    """every test here under its own time limit: a hung launch ends the process instead of the session waiting on it"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def ks(c):
    """(kx, k0, k1) the device was given: the fp32 fields as exact doubles"""
    return float(c.c2), float(c.c1), float(c.eta)


def bound(c, x, x0, x0_prev, cfg_mag):
    kx, k0, k1 = ks(c)
    b = np.abs(kx * x) + np.abs(k0 * x0) + cfg_mag
    if k1 != 0.0:
        b = b + np.abs(k1 * x0_prev)
    return 4 * EPS * b


def f64(t):
    return t.detach().cpu().double().numpy()


@pytest.fixture(scope='module')
def small():
    import motioncraft_amd as mc
    from oracle import weights as W
    sd = W.make_state_dict(SMALL, SMALL_SEED)
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_small.py'))
    arch = mc.build_architecture(cfg.model)
    arch.load_state_dict({'model.' + k: v for k, v in sd.items()})
    yield sd, arch
    arch.model.release()


def _inputs(B):
    x_T, xf, mask = synth_inputs(SMALL, B, 24, seed=11 + B, lengths=CASES[B])
    return x_T, dict(xf_out=xf, motion_mask=mask, y={})


@pytest.fixture(scope='module')
def per_step(small):
    """the per-step loop (fused=False, trajectory) on 10 steps for both batches, run once: {B: (diffusion, x_T, kwargs, trajectory, final)}"""
    from motioncraft_amd.diffusion import build_diffusion
    sd, arch = small
    out = {}
    for B in CASES:
        d = build_diffusion(dict(BASE, respace='ddim10'))
        x_T, kw = _inputs(B)
        traj = []
        final = d.dpm_solver_sample_loop(arch.model, (B, 24, C), noise=x_T, clip_denoised=False, model_kwargs=kw, fused=False,
                                         trajectory=traj)
        torch.cuda.synchronize()
        hist = arch.model._ctx[(B, 24)].buffer('x0_hist')
        out[B] = (d, x_T, kw, traj, final.clone(), hist)
    return out


# ---- the context-free op ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,offset', [(3 * 7 * 263, 1), (2 * 24 * 322, 0), (3 * 7 * 263, 0)])
def test_multistep_op_vs_fp64(n, offset):
    """first step (k1 = 0, history full of NaN), second step (reads what the first wrote), final step (0, 1, 0): x_prev == x0 bit for
    bit; out of place and in place give the same bits; n odd with every pointer off 16-byte alignment (element path) and aligned
    (f32x4 path, no tail), and aligned with the odd n (f32x4 path + element tail); nothing is stored past n."""
    from motioncraft_amd import lib as L_
    from motioncraft_amd.diffusion import build_diffusion
    from motioncraft_amd.engine import _ptr, _stream
    lib = L_.load(require_gpu=True)
    d = build_diffusion(dict(BASE, respace='ddim10'))
    idx = list(range(d.num_timesteps))[::-1]
    coefs = d.multistep_coefs(idx, 6.5)
    seq = [coefs[0], coefs[1], coefs[-1]]
    assert seq[0].eta == 0.0 and seq[1].eta != 0.0 and ks(seq[2]) == (0.0, 1.0, 0.0)
    g = torch.Generator().manual_seed(n)
    GUARD = 8

    def dev(fill=None):
        """a device operand of n floats `offset` floats into its allocation, GUARD sentinels behind it"""
        t = torch.full((offset + n + GUARD,), 777.0, device='cuda')
        if fill is not None:
            t[offset:offset + n] = fill.cuda()
        return t, t[offset:offset + n]

    x = torch.randn(n, generator=g)
    hist_full, hist = dev(torch.full((n,), float('nan')))
    assert (hist.data_ptr() % 16 != 0) == bool(offset)
    x0_prev = None
    for step, c in enumerate(seq):
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        w, u = float(c.text_coef), float(c.none_coef)
        x0_ref = f64(a) * w + f64(b) * u
        cfg_mag = np.abs(f64(a) * w) + np.abs(f64(b) * u)
        ref = R.update(ks(c), f64(x), x0_ref, x0_prev)
        bnd = bound(c, f64(x), x0_ref, x0_prev, cfg_mag)
        (_, xd), (_, ad), (_, bd) = dev(x), dev(a), dev(b)
        xp_full, xp = dev()
        x0_full, x0 = dev()
        hist_before = hist.clone()
        L_.check(lib.mc_op_sampler_multistep(_ptr(xd), _ptr(ad), _ptr(bd), _ptr(hist), _ptr(xp), _ptr(x0), n, ctypes.byref(c),
                                             _stream()), 'mc_op_sampler_multistep')
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xp).all()) and bool(torch.isfinite(x0).all()), step
        e0, e1 = np.abs(f64(x0) - x0_ref), np.abs(f64(xp) - ref)
        print(f'n={n} step {step}: x0 err/bound {float((e0 / (4 * EPS * cfg_mag)).max()):.3f}  x_prev err/bound {float((e1 / bnd).max()):.3f}')
        assert bool((e0 <= 4 * EPS * cfg_mag).all()), step
        assert bool((e1 <= bnd).all()), step
        assert torch.equal(hist, x0), step                                       # the history now holds this step's x0
        for full in (xp_full, x0_full, hist_full):
            assert bool((full[:offset] == 777.0).all()) and bool((full[offset + n:] == 777.0).all()), ('stored outside [0, n)', step)
        if step == 2:
            assert torch.equal(xp, x0)                                           # (0, 1, 0): x_prev = x0 bit for bit
        # in place (x_prev aliasing x_t), from the same history: the same bits
        h2_full, h2 = dev(hist_before)
        xin_full, xin = dev(x)
        L_.check(lib.mc_op_sampler_multistep(_ptr(xin), _ptr(ad), _ptr(bd), _ptr(h2), _ptr(xin), None, n, ctypes.byref(c), _stream()),
                 'mc_op_sampler_multistep')
        torch.cuda.synchronize()
        assert torch.equal(xin, xp) and torch.equal(h2, x0), step
        assert bool((xin_full[offset + n:] == 777.0).all()) and bool((h2_full[offset + n:] == 777.0).all())
        x, x0_prev = xp.cpu(), f64(x0)
    # the op is for mode 2 only
    ddim = d.step_coefs(5, 'ddim', 6.5)
    rc = lib.mc_op_sampler_multistep(_ptr(xd), _ptr(ad), _ptr(bd), _ptr(hist), _ptr(xp), None, n, ctypes.byref(ddim), _stream())
    assert rc == L_.MC_ERR_ARG


# ---- the per-step loop, in lockstep ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', sorted(CASES))
def test_per_step_loop_lockstep_vs_restatement_and_oracle(small, per_step, B):
    """at every one of the 10 steps: device x_prev against the restatement's update of the device's own x, x0 and previous x0 (the
    bound above; x0 is an operand here, so its own magnitude stands for the CFG terms), and device x0 against the CPU oracle denoiser
    at the same x (2e-4)."""
    from oracle import stmogen_oracle as O
    sd, arch = small
    d, x_T, kw, traj, final, hist = per_step[B]
    idx = list(range(d.num_timesteps))[::-1]
    coefs = d.multistep_coefs(idx, SMALL['scale'])
    assert [t[0] for t in traj] == idx and len(idx) == 10
    assert sum(c.eta != 0.0 for c in coefs) == 7                                 # second order but for the first step and indices 1, 0
    x, x0_prev, worst_u, worst_d = x_T, None, 0.0, 0.0
    for (i, x_prev, x0), c in zip(traj, coefs):
        ref = R.update(ks(c), f64(x), f64(x0), x0_prev)
        bnd = bound(c, f64(x), f64(x0), x0_prev, np.abs(f64(x0)))
        e = np.abs(f64(x_prev) - ref)
        worst_u = max(worst_u, float((e / bnd).max()))
        assert bool((e <= bnd).all()), (B, i)
        x0_o = O.denoise(sd, SMALL, x.cpu(), d.timestep_map[i], kw['xf_out'], kw['motion_mask'])
        err = float((x0.cpu().double() - x0_o.double()).abs().max())
        worst_d = max(worst_d, err)
        assert err <= TOL_STEP, (B, i, err)
        x, x0_prev = x_prev, f64(x0)
    print(f'B={B}: worst update err/bound {worst_u:.3f}, worst |x0 - oracle| {worst_d:.2e}')
    assert torch.equal(traj[-1][1], traj[-1][2]) and torch.equal(final, traj[-1][1])          # index 0: x = x0
    assert torch.equal(hist.view(B, 24, C), traj[-1][2])                                       # "x0_hist" = the last step's x0
    assert bool(torch.isfinite(final).all())


@pytest.mark.parametrize('B', sorted(CASES))
def test_fused_loop_and_graph_replay_give_the_per_step_bits(small, per_step, B):
    sd, arch = small
    d, x_T, kw, traj, final, _ = per_step[B]
    fused = d.dpm_solver_sample_loop(arch.model, (B, 24, C), noise=x_T, clip_denoised=False, model_kwargs=kw)
    torch.cuda.synchronize()
    assert torch.equal(fused, final)
    for _ in range(2):          # the second call reuses the captured graph
        replay = d.dpm_solver_sample_loop(arch.model, (B, 24, C), noise=x_T, clip_denoised=False, model_kwargs=kw, graph=True)
        torch.cuda.synchronize()
        assert torch.equal(replay, final)
    # a truncated walk is a prefix of the whole one
    part = d.dpm_solver_sample_loop(arch.model, (B, 24, C), noise=x_T, clip_denoised=False, model_kwargs=kw, num_steps=4)
    torch.cuda.synchronize()
    assert torch.equal(part, traj[3][1])
    arch.model._ctx[(B, 24)].graph_release()


def test_no_per_step_draw(small, per_step):
    """two runs from the same noise under different generator seeds: bit-identical (order 1 too)"""
    sd, arch = small
    d, x_T, kw, traj, final, _ = per_step[2]
    outs = []
    for seed in (1, 2):
        g = torch.Generator(device='cuda').manual_seed(seed)
        outs.append(d.dpm_solver_sample_loop(arch.model, (2, 24, C), noise=x_T, clip_denoised=False, model_kwargs=kw, generator=g))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], final)
    o1 = [d.dpm_solver_sample_loop(arch.model, (2, 24, C), noise=x_T, clip_denoised=False, model_kwargs=kw, order=1,
                                   generator=torch.Generator(device='cuda').manual_seed(s), fused=f) for s, f in ((3, True), (4, False))]
    torch.cuda.synchronize()
    assert torch.equal(o1[0], o1[1]) and not torch.equal(o1[0], final)


# ---- history state, refusals, workspace ------------------------------------------------------------------------------------------
def test_history_state_and_refusals(small):
    from motioncraft_amd import lib as L_
    from motioncraft_amd.diffusion import build_diffusion
    sd, arch = small
    nm = arch.model.native
    B, T = 2, 24
    d = build_diffusion(dict(BASE, respace='ddim10'))
    idx = list(range(d.num_timesteps))[::-1]
    ms = d.multistep_coefs(idx, SMALL['scale'])
    ddim = [d.step_coefs(i, 'ddim', SMALL['scale']) for i in idx]
    x_T, kw = _inputs(B)
    ctx = nm.context(B, T, max_steps=10)
    ctx.set_timesteps(d.timestep_map)
    xf, mask = kw['xf_out'].cuda(), kw['motion_mask'].cuda()
    ctx.set_condition(xf, mask)

    def code(rc):
        return pytest.raises(RuntimeError, match=rf'\(code {rc}\)')

    # a context that never used mode 2 keeps its workspace: the same bytes before and after a DDIM (mode 1) loop
    bytes0 = ctx.workspace_bytes
    x = x_T.cuda().clone()
    ctx.sample_loop(x, idx, ddim, noise=None, seed=5)
    torch.cuda.synchronize()
    assert ctx.workspace_bytes == bytes0
    with code(L_.MC_ERR_STATE):
        ctx.buffer('x0_hist')
    # k1 != 0 with no history: MC_ERR_STATE, and nothing was allocated for it
    x = x_T.cuda().clone()
    with code(L_.MC_ERR_STATE):
        ctx.sample_step(x, idx[1], ms[1], None)
    assert 'previous x0' in L_.last_error() and ctx.workspace_bytes == bytes0
    # first step of a walk, then the second: fine; the history buffer is the only growth
    x1 = ctx.sample_step(x, idx[0], ms[0], None)
    assert ctx.workspace_bytes == bytes0 + (B * T * C * 4 + 255) // 256 * 256
    x2 = ctx.sample_step(x1, idx[1], ms[1], None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x2).all())
    # each of the three setters clears the flag
    for reset in (lambda: ctx.set_condition(xf, mask), lambda: ctx.set_timesteps(d.timestep_map), lambda: ctx.set_control(None)):
        reset()
        with code(L_.MC_ERR_STATE):
            ctx.sample_step(x1, idx[1], ms[1], None)
        with code(L_.MC_ERR_STATE):
            ctx.sample_loop(x1.clone(), idx[1:3], ms[1:3])
        ctx.sample_step(x, idx[0], ms[0], None)
        ctx.sample_step(x1, idx[1], ms[1], None)
    # modes 0 / 1 still need their noise
    with code(L_.MC_ERR_ARG):
        ctx.sample_step(x, idx[0], ddim[0], None)
    # no outpainting / seeding form of mode 2
    keep = torch.zeros(B, T, C, dtype=torch.bool, device='cuda')
    with code(L_.MC_ERR_ARG):
        ctx.sample_step_inpaint(x, idx[0], ms[0], torch.zeros_like(x), torch.zeros_like(x), keep, gt_noise=torch.zeros_like(x))
    assert 'mode 2' in L_.last_error()
    with code(L_.MC_ERR_ARG):
        ctx.sample_step_seeded(x, idx[0], ms[0], torch.zeros_like(x), 1.0, 0.0)
    # one graph per table: a table that mixes mode 2 with another mode is refused; so is a replay that would read a history that is not there
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gx, gn = torch.empty_like(x), torch.zeros_like(x)
        with code(L_.MC_ERR_ARG):
            ctx.graph_capture(gx, gn, ms[::-1][:5] + ddim[::-1][5:])
        assert 'mixes' in L_.last_error()
        ctx.graph_capture(gx, None, ms[::-1])
        ctx.set_condition(xf, mask)          # (the library copies the condition: the graph stays valid, the history does not)
        with code(L_.MC_ERR_STATE):
            ctx.graph_step(idx[1])
        gx.copy_(x_T.cuda())
        ctx.graph_step(idx[0])
        ctx.graph_step(idx[1])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(gx, x2)               # replay = eager, step for step
    ctx.graph_release()
    ctx.close()


# ---- through the architecture API -----------------------------------------------------------------------------------------------
def test_motion_diffusion_dpmpp(small):
    import motioncraft_amd as mc
    sd, arch = small
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_small.py'))
    cfg.model.inference_type = 'dpmpp'
    cfg.model.diffusion_test = dict(BASE, respace='logsnr10')
    arch2 = mc.build_architecture(cfg.model)
    arch2.load_state_dict({'model.' + k: v for k, v in sd.items()})
    B, T = 2, 24
    x_T, kw = _inputs(B)
    mask = kw['motion_mask']

    def call(a, **ik):
        return a(motion=torch.zeros(B, T, C), motion_mask=mask, motion_length=mask.sum(1, keepdim=True).long(),
                 motion_metas=[{'text': 'a'}, {'text': 'b'}], xf_out=kw['xf_out'], inference_kwargs=dict(noise=x_T, **ik))
    res = call(arch2)
    ref = call(arch)                          # the config's own 'ddim'
    assert isinstance(res, list) and len(res) == B and set(res[0]) == set(ref[0])
    final = torch.stack([r['pred_motion'] for r in res])
    assert bool(torch.isfinite(final).all()) and not final.is_cuda
    first = torch.stack([r['pred_motion'] for r in call(arch2, order=1)])
    assert bool(torch.isfinite(first).all()) and not torch.equal(first, final)
    with pytest.raises(NotImplementedError, match='pre_seq'):
        call(arch2, pre_seq=torch.zeros(B, 2, C))
    arch2.model.release()

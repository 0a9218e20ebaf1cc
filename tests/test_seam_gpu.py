"""GPU (MI355X): coupled windows of a long sequence -- sampler_seam_k through the context-free op, the context (per-step walk, fused
loop, all three modes), the refusals, and the window driver -- against tests/seam_ref.py (fp64), the plain sampler ops and the CPU
oracle denoiser.

The reference has no such sampler, so nothing here is a golden of it.  Off the seams the coupled update must give the BITS of the plain
kernels; on the seams the update arithmetic is pinned without a tolerance by feeding the plain op the coupled op's own x0; only the blend
itself meets fp64, under a bound derived from its roundings (each rounds at most 2^-24 of the magnitude it rounds):

  one CFG combination  x0 = a w + b u:  4 * 2^-24 * (|a w| + |b u|) =: 4 eps M          (tests/test_dpm_solver_gpu.py's bound: 2 + spare)
  the blend  fma(w, x0_r, rn(rn(1 - w) x0_l)):  the two CFG errors pass through with weights w and 1 - w, then 1 - w, the product and
  the fma round once each; with |x0| <= M and one spare:  4 eps (w M_r + (1 - w) M_l)
  together:  8 * 2^-24 * (w M_r + (1 - w) M_l)
"""
import ctypes
import faulthandler
import os

import numpy as np
import pytest
import torch

import seam_ref as S
from helpers import CTRL, CTRL_COPY, CTRL_FEATS, SMALL, SMALL_SEED, synth_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
EPS = 2.0 ** -24
TOL_STEP = 2e-4             # one denoiser call of the fp32 path against the oracle (tests/test_dpm_solver_gpu.py, tests/test_gpu_parity.py)
C = 322
T, OV = 24, 6               # the context-level windows
PLANS = {3: [0, 18, 36], 4: [0, 18, 42, 60]}          # batch -> first frames: one chain of three; two sequences of two
GUARD = 8

# name -> (B, T, C, ov, first_frame, offset in floats of every operand from 16-byte alignment)
OP_SHAPES = {
    'chain_unaligned': (3, 7, 263, 3, [0, 4, 8], 1),         # middle row: head, ONE interior frame, tail; groups straddle seam boundaries
    'chain_no_interior': (3, 6, 251, 3, [0, 3, 6], 0),       # 2 ov == T: the middle row is all seam; n % 4 != 0 (element tail)
    'two_sequences_aligned': (4, 8, 322, 2, [0, 6, 14, 20], 0),   # f32x4 path off the seams
    'pair_and_single': (3, 8, 263, 3, [0, 5, 40], 0),        # rows 0-1 neighbours, row 2 alone
}


@pytest.fixture(autouse=True)
def time_limit():
    """every test here under its own time limit: a hung launch ends the process instead of the session waiting on it"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def f64(t):
    return t.detach().cpu().double().numpy()


def _lib():
    from motioncraft_amd import lib as L_
    from motioncraft_amd.engine import _ptr, _stream
    return L_, L_.load(require_gpu=True), _ptr, _stream


def _mode_coefs():
    """one StepCoefs per mode with every term live: DDPM mid-schedule, DDIM with eta = 0.5 (the noise counts), a second-order multistep step"""
    from motioncraft_amd.diffusion import build_diffusion
    d = build_diffusion(dict(BASE, respace='ddim10'))
    ms = d.multistep_coefs(list(range(d.num_timesteps))[::-1], 6.5)[1]
    assert ms.eta != 0.0
    return {0: d.step_coefs(5, 'ddpm', 6.5), 1: d.step_coefs(5, 'ddim', 6.5, eta=0.5), 2: ms}


class Ops:
    """operands of one op case on the device, each `offset` floats into its allocation with GUARD sentinels behind (and `offset` before)"""

    def __init__(self, B, T, Cc, ov, ff, offset, seed):
        self.shape, self.n, self.ov, self.ff, self.offset = (B, T, Cc), B * T * Cc, ov, ff, offset
        self.flags = S.plan_flags(ff, T, ov)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, T, Cc, generator=g)
        self.x = torch.from_numpy(S.share_left(x.numpy(), self.flags, ov)).float()          # the precondition: x agrees on shared frames
        self.a, self.b, self.noise, self.hist = (torch.randn(B, T, Cc, generator=g) for _ in range(4))     # (noise, history: NOT shared)
        self.fulls = []

    def dev(self, fill=None, guard=True):
        t = torch.full((self.offset + self.n + GUARD,), 777.0, device='cuda')
        if fill is not None:
            t[self.offset:self.offset + self.n] = fill.reshape(-1).cuda()
        v = t[self.offset:self.offset + self.n]
        assert (v.data_ptr() % 16 != 0) == bool(self.offset)
        if guard:
            self.fulls.append(t)
        return v

    def guards_intact(self):
        o, n = self.offset, self.n
        return all(bool((t[:o] == 777.0).all()) and bool((t[o + n:] == 777.0).all()) for t in self.fulls)


def _seam_op(o, c, x, a, b, noise, hist, xp, x0, weights=None, seed=0, draw=0):
    L_, lib, _ptr, _stream = _lib()
    B, T_, Cc = o.shape
    ff = (ctypes.c_int32 * B)(*o.ff)
    w = (ctypes.c_float * o.ov)(*weights) if weights is not None else None
    L_.check(lib.mc_op_sampler_seam(_ptr(x), _ptr(a), _ptr(b), _ptr(noise), seed, draw, _ptr(hist), _ptr(xp), _ptr(x0), B, T_, Cc, o.ov, ff, w,
                                    ctypes.byref(c), _stream()), 'mc_op_sampler_seam')
    torch.cuda.synchronize()


def _plain_op(o, c, x, a, b, noise, hist, xp, x0):
    L_, lib, _ptr, _stream = _lib()
    if c.mode == 2:
        L_.check(lib.mc_op_sampler_multistep(_ptr(x), _ptr(a), _ptr(b), _ptr(hist), _ptr(xp), _ptr(x0), o.n, ctypes.byref(c), _stream()),
                 'mc_op_sampler_multistep')
    else:
        L_.check(lib.mc_op_sampler_update(_ptr(x), _ptr(a), _ptr(b), _ptr(noise), _ptr(xp), _ptr(x0), o.n, ctypes.byref(c), _stream()),
                 'mc_op_sampler_update')
    torch.cuda.synchronize()


# ---- 1. the context-free op -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', sorted(OP_SHAPES))
def test_seam_op(name, mode):
    L_, lib, _ptr, _stream = _lib()
    B, T_, Cc, ov, ff, offset = OP_SHAPES[name]
    o = Ops(B, T_, Cc, ov, ff, offset, seed=100 + 10 * sorted(OP_SHAPES).index(name) + mode)
    c = _mode_coefs()[mode]
    ms = mode == 2
    sh = o.shape
    seam = torch.from_numpy(S.seam_mask(o.flags, T_, ov))[:, :, None].expand(*sh)          # bool [B, T, C]
    pairs = [b for b, (_, r) in enumerate(o.flags) if r]
    assert pairs and bool(seam.any()) and not bool(seam.all())
    xd, ad, bd, nd = o.dev(o.x), o.dev(o.a), o.dev(o.b), o.dev(o.noise)
    hist = o.dev(o.hist) if ms else None
    xp, x0 = o.dev(), o.dev()
    _seam_op(o, c, xd, ad, bd, None if ms else nd, hist, xp, x0)
    XP, X0 = xp.view(sh).cpu(), x0.view(sh).cpu()
    assert bool(torch.isfinite(XP).all()) and bool(torch.isfinite(X0).all())
    # (a) one value per shared element, in both rows
    for b in pairs:
        assert torch.equal(XP[b, T_ - ov:], XP[b + 1, :ov]) and torch.equal(X0[b, T_ - ov:], X0[b + 1, :ov]), b
        if ms:
            H = hist.view(sh).cpu()
            assert torch.equal(H[b, T_ - ov:], H[b + 1, :ov]), b
    if ms:
        assert torch.equal(hist.view(sh).cpu(), X0)                                         # the history holds this step's x0
    # (b) off the seams: the bits of the plain kernels on the same operands
    hist_p = o.dev(o.hist) if ms else None
    xp_p, x0_p = o.dev(), o.dev()
    _plain_op(o, c, xd, ad, bd, nd, hist_p, xp_p, x0_p)
    XP_p, X0_p = xp_p.view(sh).cpu(), x0_p.view(sh).cpu()
    assert torch.equal(XP[~seam], XP_p[~seam]) and torch.equal(X0[~seam], X0_p[~seam])
    assert not torch.equal(X0[seam], X0_p[seam])                                            # ... and on them the blend did something
    # (c) the update arithmetic, without a tolerance: the plain op on the coupled op's own x0 (text_coef 1, none_coef 0 pass it through
    # exactly), the same x, and the noise / history a seam element takes -- the LEFT row's
    c1 = type(c).from_buffer_copy(c)
    c1.text_coef, c1.none_coef = 1.0, 0.0
    zeros = o.dev(torch.zeros(sh))
    n_left = o.dev(torch.from_numpy(S.share_left(o.noise.numpy(), o.flags, ov)).float())
    h_left = o.dev(torch.from_numpy(S.share_left(o.hist.numpy(), o.flags, ov)).float()) if ms else None
    xp_c = o.dev()
    _plain_op(o, c1, xd, x0, zeros, n_left, h_left, xp_c, None)
    assert torch.equal(xp_c.view(sh).cpu(), XP)
    # (d) the blended x0 against fp64, under the bound of the module docstring
    w, u = float(c.text_coef), float(c.none_coef)
    A, Bn = f64(o.a), f64(o.b)
    x0_win, mag = A * w + Bn * u, np.abs(A * w) + np.abs(Bn * u)
    wt = S.default_weights(ov)
    ref = S.blend(x0_win, o.flags, ov, wt)
    bound = 4 * EPS * mag                                                                   # off the seams: one CFG combination
    for b in pairs:
        bl = 8 * EPS * (wt[:, None] * mag[b + 1, :ov] + (1 - wt)[:, None] * mag[b, T_ - ov:])
        bound[b, T_ - ov:], bound[b + 1, :ov] = bl, bl
    err = np.abs(f64(X0) - ref)
    sm = seam.numpy()
    print(f'{name} mode {mode}: x0 err/bound on seams {float((err[sm] / bound[sm]).max()):.3f}, off seams {float((err[~sm] / bound[~sm]).max()):.3f}')
    assert bool((err <= bound).all())
    # ... and the update against the restatement's coupled step on the device's own x0 (sanity of the restatement, loose: 1e-5 relative)
    ref_step, _ = S.step(c, f64(o.x), x0_win, o.flags, ov, wt, noise=None if ms else f64(o.noise), x0_prev=f64(o.hist) if ms else None)
    assert np.allclose(f64(XP), ref_step, rtol=0, atol=1e-5 * (1 + np.abs(ref_step).max()))
    # (e) in place = out of place
    x_in = o.dev(o.x)
    hist_in = o.dev(o.hist) if ms else None
    _seam_op(o, c, x_in, ad, bd, None if ms else nd, hist_in, x_in, None)
    assert torch.equal(x_in.view(sh).cpu(), XP)
    if ms:
        assert torch.equal(hist_in.view(sh).cpu(), X0)
    # (g) the device Philox form = the host-noise form fed the same draws
    if not ms:
        seed, draw = 77, 5
        pz = o.dev()
        L_.check(lib.mc_op_philox_normal(_ptr(pz), None, o.n, seed, draw, _stream()), 'mc_op_philox_normal')
        xp_h, xp_d, x0_d = o.dev(), o.dev(), o.dev()
        _seam_op(o, c, xd, ad, bd, pz, None, xp_h, None)
        _seam_op(o, c, xd, ad, bd, None, None, xp_d, x0_d, seed=seed, draw=draw)
        assert torch.equal(xp_h, xp_d) and torch.equal(x0_d.view(sh).cpu(), X0)
        assert not torch.equal(xp_d.view(sh).cpu(), XP)                                    # (other noise than the first run's)
        for b in pairs:
            assert torch.equal(xp_d.view(sh)[b, T_ - ov:], xp_d.view(sh)[b + 1, :ov])
    # (h) weights 0 / 1: the left / the right window's x0, bit for bit
    for wv, side in ((0.0, 'left'), (1.0, 'right')):
        x0_w, xp_w = o.dev(), o.dev()
        hist_w = o.dev(o.hist) if ms else None
        _seam_op(o, c, xd, ad, bd, None if ms else nd, hist_w, xp_w, x0_w, weights=[wv] * ov)
        X0w = x0_w.view(sh).cpu()
        for b in pairs:
            want = X0_p[b, T_ - ov:] if side == 'left' else X0_p[b + 1, :ov]
            assert torch.equal(X0w[b, T_ - ov:], want) and torch.equal(X0w[b + 1, :ov], want), (side, b)
        assert torch.equal(X0w[~seam], X0_p[~seam])
    # (f) nothing was stored before or behind any operand or output
    assert o.guards_intact()


# ---- 2. the context ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    import motioncraft_amd as mc
    from oracle import weights as W
    sd = W.make_state_dict(SMALL, SMALL_SEED)
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_small.py'))
    cfg.model.diffusion_test = dict(BASE, respace='ddim10')
    arch = mc.build_architecture(cfg.model)
    arch.load_state_dict({'model.' + k: v for k, v in sd.items()})
    yield sd, arch
    arch.model.release()


def _inputs(B):
    """x_T gathered from one draw per global frame (agrees on shared frames), per-row text condition, full masks; the coupled kwargs"""
    ff = PLANS[B]
    _, xf, mask = synth_inputs(SMALL, B, T, seed=40 + B)
    z = torch.randn(max(ff) + T, C, generator=torch.Generator().manual_seed(50 + B))
    x_T = torch.stack([z[f:f + T] for f in ff])
    plain = dict(xf_out=xf, motion_mask=mask, y={})
    return x_T, plain, dict(plain, seams=dict(first_frame=ff, overlap=OV))


def _walk(d, sampler, model, B, x_T, kw, **extra):
    loop = d.ddim_sample_loop if sampler == 'ddim' else d.dpm_solver_sample_loop
    out = loop(model, (B, T, C), noise=x_T, clip_denoised=False, model_kwargs=kw, **extra)
    torch.cuda.synchronize()
    return out.clone()


@pytest.fixture(scope='module')
def walks(small):
    """every walk of the context-level tests, run once: {(sampler, B): dict(plain before any table, per-step trajectory + final)}"""
    from motioncraft_amd.diffusion import build_diffusion
    sd, arch = small
    d = build_diffusion(dict(BASE, respace='ddim10'))
    out = {}
    for B in PLANS:
        x_T, plain, coupled = _inputs(B)
        for sampler in ('ddim', 'dpmpp'):
            before = _walk(d, sampler, arch.model, B, x_T, plain)          # the context has never seen a seam table
            traj = []
            final = _walk(d, sampler, arch.model, B, x_T, coupled, fused=False, trajectory=traj)
            out[(sampler, B)] = dict(d=d, before=before, traj=traj, final=final)
    return out


@pytest.mark.parametrize('B', sorted(PLANS))
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp'])
def test_per_step_walk_keeps_seams_and_meets_the_oracle(small, walks, sampler, B):
    """10 steps: the shared frames of x and of x0 are bit-equal in both rows after EVERY step; the device x0 is the oracle's per-window
    x0 at the same x, blended in fp64 (the blend is convex: it adds nothing to the denoiser's bound)"""
    from oracle import stmogen_oracle as O
    sd, arch = small
    w = walks[(sampler, B)]
    d, traj = w['d'], w['traj']
    x_T, plain, _ = _inputs(B)
    flags = S.plan_flags(PLANS[B], T, OV)
    assert len(traj) == 10 and S.seams_equal(x_T.numpy(), flags, OV)
    x, worst = x_T, 0.0
    for i, x_prev, x0 in traj:
        assert S.seams_equal(x_prev.cpu().numpy(), flags, OV) and S.seams_equal(x0.cpu().numpy(), flags, OV), (sampler, B, i)
        x0_o = O.denoise(sd, SMALL, x.cpu(), d.timestep_map[i], plain['xf_out'], plain['motion_mask'])
        err = float(np.abs(f64(x0) - S.blend(x0_o.double().numpy(), flags, OV)).max())
        worst = max(worst, err)
        assert err <= TOL_STEP, (sampler, B, i, err)
        x = x_prev
    print(f'{sampler} B={B}: worst |x0 - blended oracle| {worst:.2e}')
    assert torch.equal(w['final'], traj[-1][1]) and bool(torch.isfinite(w['final']).all())
    assert not torch.equal(w['final'], w['before'])                        # the table changed the walk
    sm = torch.from_numpy(S.seam_mask(flags, T, OV))
    assert not torch.equal(w['before'][:, :, 0][sm], w['final'][:, :, 0][sm])


@pytest.mark.parametrize('B', sorted(PLANS))
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp'])
def test_fused_loop_gives_the_per_step_bits_and_clearing_restores_the_plain_walk(small, walks, sampler, B):
    sd, arch = small
    w = walks[(sampler, B)]
    x_T, plain, coupled = _inputs(B)
    ctx = arch.model._ctx[(B, T)]
    assert ctx.seams is None                                               # the loops cleared the table behind them
    fused = _walk(w['d'], sampler, arch.model, B, x_T, coupled)            # mc_sample_loop
    assert torch.equal(fused, w['final'])
    part = _walk(w['d'], sampler, arch.model, B, x_T, coupled, num_steps=4)
    assert torch.equal(part, w['traj'][3][1])
    assert ctx.seams is None
    after = _walk(w['d'], sampler, arch.model, B, x_T, plain)              # the same context, table cleared: the plain walk's bits
    assert torch.equal(after, w['before'])


def test_device_noise_ddpm_walk_keeps_seams(small):
    """the fused loop drawing its noise in the kernel (Philox): a seam element takes the left row's counter, so the rows stay equal"""
    from motioncraft_amd.diffusion import build_diffusion
    sd, arch = small
    d = build_diffusion(dict(BASE, respace='ddim10'))
    for B in sorted(PLANS):
        x_T, plain, coupled = _inputs(B)
        flags = S.plan_flags(PLANS[B], T, OV)
        outs = [d.p_sample_loop(arch.model, (B, T, C), noise=x_T, clip_denoised=False, model_kwargs=kw,
                                generator=torch.Generator(device='cuda').manual_seed(3)).clone() for kw in (coupled, coupled, plain)]
        torch.cuda.synchronize()
        assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
        assert S.seams_equal(outs[0].cpu().numpy(), flags, OV) and not S.seams_equal(outs[2].cpu().numpy(), flags, OV)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(small):
    L_, lib, _ptr, _stream = _lib()
    from motioncraft_amd.diffusion import build_diffusion
    sd, arch = small
    nm = arch.model.native
    B = 3
    d = build_diffusion(dict(BASE, respace='ddim10'))
    idx = list(range(d.num_timesteps))[::-1]
    ddim = [d.step_coefs(i, 'ddim', SMALL['scale']) for i in idx]
    x_T, plain, _ = _inputs(B)
    ctx = nm.context(B, T, max_steps=10)
    ctx.set_timesteps(d.timestep_map)
    ctx.set_condition(plain['xf_out'].cuda(), plain['motion_mask'].cuda())
    x = x_T.cuda().clone()

    def code(rc):
        return pytest.raises(RuntimeError, match=rf'\(code {rc}\)')

    def raw_set(ff, ov, w=None):
        arr = (ctypes.c_int32 * len(ff))(*ff)
        warr = (ctypes.c_float * len(w))(*w) if w is not None else None
        return lib.mc_ctx_set_seams(ctx.handle, ov, arr, warr, _stream())

    ctx.set_seams(PLANS[B], OV)
    # every plan the rules refuse: MC_ERR_ARG from the library itself (the Python check bypassed), the table that was set stays set
    bad = [([0, 3, 36], OV), ([0, 18, 17], OV), ([-1, 17, 35], OV), ([0, 18, 40], OV), ([36, 18, 0], OV), ([0, 18, 36], 13), ([0, 18, 36], -2)]
    for ff, ov in bad:
        assert raw_set(ff, ov) == L_.MC_ERR_ARG, (ff, ov)
        assert 'mc_ctx_set_seams' in L_.last_error()
    assert raw_set(PLANS[B], OV, [0.5] * 5 + [1.5]) == L_.MC_ERR_ARG and 'weight' in L_.last_error()
    assert lib.mc_ctx_set_seams(ctx.handle, OV, None, None, _stream()) == L_.MC_ERR_ARG
    # with a table set: no graph capture, no outpainting step, no seeded step
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gx, gn = torch.empty_like(x), torch.zeros_like(x)
        with code(L_.MC_ERR_STATE):
            ctx.graph_capture(gx, gn, ddim[::-1])
        assert 'seam table' in L_.last_error()
    torch.cuda.current_stream().wait_stream(side)
    keep = torch.zeros(B, T, C, dtype=torch.bool, device='cuda')
    with code(L_.MC_ERR_STATE):
        ctx.sample_step_inpaint(x, idx[0], ddim[0], torch.zeros_like(x), torch.zeros_like(x), keep, gt_noise=torch.zeros_like(x))
    assert 'seam table' in L_.last_error()
    with code(L_.MC_ERR_STATE):
        ctx.sample_step_seeded(x, idx[0], ddim[0], torch.zeros_like(x), 1.0, 0.0)
    assert 'seam table' in L_.last_error()
    # the coupled step itself runs; once the table is cleared the refused entry points are back ...
    x1 = ctx.sample_step(x, idx[0], ddim[0], torch.zeros_like(x))
    torch.cuda.synchronize()
    assert S.seams_equal(x1.cpu().numpy(), S.plan_flags(PLANS[B], T, OV), OV)
    ctx.clear_seams()
    # ... capture among them; a captured graph replays the uncoupled step: no table beside it
    with torch.cuda.stream(side):
        ctx.graph_capture(gx, gn, ddim[::-1])
        assert raw_set(PLANS[B], OV) == L_.MC_ERR_STATE and 'graph' in L_.last_error()
        ctx.graph_release()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ctx.close()
    # the op: an invalid plan, or a noise tensor beside a Philox draw, is MC_ERR_ARG and nothing is launched (the output keeps its fill)
    o = Ops(3, 8, 263, 3, [0, 5, 10], 0, seed=1)
    xd, ad, bd, nd, xp = o.dev(o.x), o.dev(o.a), o.dev(o.b), o.dev(o.noise), o.dev()
    c = _mode_coefs()[1]
    for ff, ov, seed in (([0, 4, 10], 3, 0), ([0, 5, 10], 5, 0), ([0, 5, 10], 0, 0), ([0, 5, 10], 3, 9)):
        rc = lib.mc_op_sampler_seam(_ptr(xd), _ptr(ad), _ptr(bd), _ptr(nd), seed, 0, None, _ptr(xp), None, 3, 8, 263, ov, (ctypes.c_int32 * 3)(*ff),
                                    None, ctypes.byref(c), _stream())
        assert rc == L_.MC_ERR_ARG, (ff, ov, seed)
    torch.cuda.synchronize()
    assert bool((xp == 777.0).all())


# ---- 4. the window driver ---------------------------------------------------------------------------------------------------------
def _xf(S_, dims, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.layer_norm(torch.randn(S_, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda()


def test_driver_two_sequences_and_the_one_window_case(small):
    from motioncraft_amd import longform
    sd, arch = small
    totals = [60, 42]                                   # 3 and 2 windows
    xf = _xf(2, SMALL, 5)

    def run():
        gen = torch.Generator(device='cuda').manual_seed(11)
        return longform.sample_long_coupled(arch, totals, T, OV, text=['a', 'b'], condition_kwargs=dict(xf_out=xf), input_dim=C,
                                            inference_kwargs=dict(generator=gen), shard=False)
    recs, wins = run()
    assert sorted(wins) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    for s, t in enumerate(totals):
        n, _, frames = longform.seam_plan(t, T, OV)
        assert recs[s].shape == (frames, C) and np.isfinite(recs[s]).all()
        for w in range(n - 1):
            assert np.array_equal(wins[(s, w)][T - OV:], wins[(s, w + 1)][:OV])
    assert not np.array_equal(wins[(0, 2)][T - OV:], wins[(1, 0)][:OV])          # the next sequence is not coupled to this one
    recs2, _ = run()
    assert all(np.array_equal(a, b) for a, b in zip(recs, recs2))                # the same generator seed: the same bits
    assert arch.model._ctx[(5, T)].seams is None
    # a sequence of exactly one window, alone in its call: the plain model call, bit for bit
    z = torch.randn(T, C, generator=torch.Generator().manual_seed(12))
    one, w1 = longform.sample_long_coupled(arch, [T], T, OV, text=['a'], noise=[z], condition_kwargs=dict(xf_out=xf[:1]), input_dim=C,
                                           inference_kwargs=dict(generator=torch.Generator(device='cuda').manual_seed(13)), shard=False)
    dev = torch.device('cuda')
    direct = arch(motion=torch.zeros(1, T, C, device=dev), motion_mask=torch.ones(1, T, device=dev),
                  motion_length=torch.full((1, 1), T, device=dev).long(), num_intervals=1, motion_metas=[{'text': 'a'}], xf_out=xf[:1],
                  inference_kwargs=dict(noise=z[None], generator=torch.Generator(device='cuda').manual_seed(13)))
    assert np.array_equal(w1[(0, 0)], direct[0]['pred_motion'][:T].numpy()) and np.array_equal(one[0], w1[(0, 0)])


def test_driver_with_a_per_frame_condition():
    """the control branch with one condition row per frame (the music-to-dance form): window w reads the rows of its frames"""
    import motioncraft_amd as mc
    from motioncraft_amd import longform
    from oracle import weights as W
    sd = W.make_state_dict(CTRL, SMALL_SEED, shapes=W.control_param_shapes(CTRL, CTRL_COPY, CTRL_FEATS))
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_small.py'))
    cfg.model.model.num_layers = 3
    cfg.model.diffusion_test = dict(BASE, respace='ddim10')
    cfg.merge_from_dict({'condition_encode_cfg': dict(dataset_name='nothing', condition_pre_encode=False, condition_pre_encode_type='nothing',
                                                      control_cond_feats=CTRL_FEATS, condition_latent_dim=CTRL['L'] * CTRL['H'],
                                                      condition_cfg=True)})
    arch = mc.build_architecture(cfg.model)
    arch.model = mc.ControlT2MHalf(arch.model, copy_blocks_num=CTRL_COPY, control_cond_feats=CTRL_FEATS, cfg=cfg)
    arch.load_state_dict({'model.' + k: v for k, v in sd.items()})
    totals = [42, 60]
    g = torch.Generator().manual_seed(21)
    cs = [torch.randn(t, CTRL_FEATS, generator=g) for t in totals]
    xf = _xf(2, CTRL, 6)

    def run(c):
        return longform.sample_long_coupled(arch, totals, T, OV, c=c, text=['a', 'b'], condition_kwargs=dict(xf_out=xf), input_dim=C,
                                            inference_kwargs=dict(generator=torch.Generator(device='cuda').manual_seed(4)), shard=False)
    recs, wins = run(cs)
    assert [r.shape for r in recs] == [(longform.seam_plan(t, T, OV)[2], C) for t in totals] and all(np.isfinite(r).all() for r in recs)
    other, _ = run([cs[0], torch.roll(cs[1], 7, 0)])
    assert not np.array_equal(other[1], recs[1])                                 # the condition reaches the sample
    arch.model.release()


def test_driver_on_the_s2g_config_with_many_rows_per_frame():
    """the speech front: 523 audio rows per frame through the wav encoder, three coupled 16-frame windows sharing 4 frames"""
    import motioncraft_amd as mc
    from motioncraft_amd import longform, speech, synthetic
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_s2g_small.py'))
    cfg.model.diffusion_test = dict(BASE, respace='ddim10')
    arch = mc.build_architecture(cfg.model)
    arch.model = mc.ControlT2MHalf(arch.model, copy_blocks_num=cfg.copy_blocks_num, control_cond_feats=cfg.control_cond_feats, cfg=cfg)
    sd = synthetic.make_control_wav_state(arch.model.dims, cfg.copy_blocks_num, cfg.control_cond_feats, 2)
    arch.load_state_dict({'model.' + k: v for k, v in sd.items()})
    Lw, ov, r = 16, 4, 523
    rs = np.random.RandomState(3)
    n = 40 * r + 80
    y = (0.05 * rs.standard_normal(n) * (1.0 + np.sin(np.arange(n) * (2 * np.pi / 3000.0)))).astype(np.float32)
    xf = _xf(1, arch.model.dims, 7)
    seen = []

    def spy(**kw):
        seen.append((kw['c'].shape, kw['seams']))
        return arch(**kw)
    recs, wins = speech.sample_speech(spy, y, words=['hello', 'there'], motion_length=Lw, pre_frames=ov, samples_per_frame=r, coupled=True,
                                      input_dim=C, condition_kwargs=dict(xf_out=xf), shard=False,
                                      inference_kwargs=dict(generator=torch.Generator(device='cuda').manual_seed(8)))
    n_win, first, frames = longform.seam_plan(speech.speech_frames(n, r), Lw, ov)
    assert n_win == 3 and len(wins) == 3 and recs[0].shape == (frames, C) and np.isfinite(recs[0]).all()
    assert seen == [((3, Lw * r, 2), dict(first_frame=first, overlap=ov, weights=None))]
    for w in range(2):
        assert np.array_equal(wins[(0, w)][Lw - ov:], wins[(0, w + 1)][:ov])
    arch.model.release()

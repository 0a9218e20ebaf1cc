"""GPU (MI355X): long requests among the rows -- ``sampler_seam_rows_k`` through ``mc_op_sampler_seam_rows``, the context
(``mc_ctx_set_seam_rows`` + ``mc_sample_rows``), the refusals, and ``serve.ContinuousBatcher(overlap=)`` -- against
tests/seam_rows_ref.py (fp64), the row op, the whole-batch seam op and ``longform.sample_long_coupled``.

Device against device is exact (torch.equal).  The blend meets fp64 under section 4m's own bound (tests/test_seam_gpu.py):
``8 * 2^-24 * (w M_r + (1 - w) M_l)`` on a seam, ``4 * 2^-24 * M`` off it, with ``M = |a| + |b|`` of ``x0 = a + b``.  The device x0 of a
context step meets the oracle's per-window x0, blended in fp64, within the project's per-call 2e-4."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest
import torch

import rowstep_ref
import seam_ref as S
import seam_rows_ref as SR
from helpers import SMALL, SMALL_SEED

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
EPS = 2.0 ** -24
TOL_STEP = 2e-4
GUARD = 8
U64 = 2 ** 64 - 1

# ---- the kernel: B = 5, T = 7, C = 263 (T C = 1841 is odd: groups straddle rows), ov = 3 ----
KB, KT, KC, KOV = 5, 7, 263, 3
KSTRIDE = KT - KOV
K_RIGHT = [4, -1, -1, 0, -1]                      # one chain on rows (3, 0, 4): a right neighbour at a LOWER and at a higher index
K_FIRST = [KSTRIDE, 0, 5, 0, 2 * KSTRIDE]         # row 1 alone; row 2 alone at an odd first frame: 5 * 263 % 4 == 3 (two Philox calls a group)
K_REQ = [0, 1, 2, 0, 0]                           # the request of every row
K_SEEDS = [77, 2 ** 63 + 5, 11 + 2 ** 32]         # per request
BIG = 8_170_000                                   # BIG * 263 > 2^31


@pytest.fixture(autouse=True)
def time_limit():
    """every test here under its own time limit: a hung launch ends the process instead of the session waiting on it"""
    faulthandler.dump_traceback_later(180, exit=True)
    threads = torch.get_num_threads()
    yield
    torch.set_num_threads(threads)
    faulthandler.cancel_dump_traceback_later()


def f64(t):
    return t.detach().cpu().double().numpy()


def _lib():
    from motioncraft_amd import lib as L_
    from motioncraft_amd.engine import _ptr, _stream
    return L_, L_.load(require_gpu=True), _ptr, _stream


def _diffusion(respace='ddim10'):
    from motioncraft_amd.diffusion import build_diffusion
    return build_diffusion(dict(BASE, respace=respace))


def _request_coefs(mode):
    """three different entries, one per request, every term live; mode 2: request 2 takes a FIRST step (eta == 0: no history read)"""
    d = _diffusion()
    if mode == 2:
        ms = d.multistep_coefs(list(range(d.num_timesteps))[::-1], 6.5)
        assert ms[0].eta == 0.0 and ms[1].eta != 0.0 and ms[3].eta != 0.0
        return [ms[1], ms[3], ms[0]]
    name = 'ddpm' if mode == 0 else 'ddim'
    return [d.step_coefs(i, name, s, **({} if mode == 0 else dict(eta=0.5))) for i, s in ((5, 6.5), (3, 2.0), (8, 4.0))]


def _unit(c):
    c = type(c).from_buffer_copy(c)
    c.text_coef, c.none_coef = 1.0, 1.0
    return c


class Ops:
    """operands of one op case on the device, each `offset` floats into its allocation with GUARD sentinels behind (and `offset` before)"""

    def __init__(self, rows, offset, seed, shape=(KB, KT, KC), ov=KOV):
        B, T, C = shape
        self.shape, self.n, self.ov, self.rows, self.offset = shape, B * T * C, ov, rows, offset
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, T, C, generator=g)
        self.x = torch.from_numpy(SR.share_left(x.numpy(), rows, ov)).float()             # the precondition: x agrees on shared frames
        self.a, self.b, self.noise, self.hist = (torch.randn(B, T, C, generator=g) for _ in range(4))     # (noise, history: NOT shared)
        self.fulls = []

    def dev(self, fill=None):
        t = torch.full((self.offset + self.n + GUARD,), 777.0, device='cuda')
        if fill is not None:
            t[self.offset:self.offset + self.n] = fill.reshape(-1).cuda()
        v = t[self.offset:self.offset + self.n]
        assert (v.data_ptr() % 16 != 0) == bool(self.offset)
        self.fulls.append(t)
        return v

    def guards_intact(self):
        o, n = self.offset, self.n
        return all(bool((t[:o] == 777.0).all()) and bool((t[o + n:] == 777.0).all()) for t in self.fulls)


def _rows_op(o, coefs, x, a, b, noise, hist, xp, x0, weights=None, seeds=None, draws=None, raw=False):
    L_, lib, _ptr, _stream = _lib()
    B, T, C = o.shape
    right = (ctypes.c_int32 * B)(*[r for r, _, _ in o.rows])
    ff = (ctypes.c_int32 * B)(*[f for _, _, f in o.rows])
    w = (ctypes.c_float * o.ov)(*weights) if weights is not None else None
    sd = (ctypes.c_uint64 * B)(*[s & U64 for s in seeds]) if seeds is not None else None
    dr = (ctypes.c_uint64 * B)(*draws) if draws is not None else None
    rc = lib.mc_op_sampler_seam_rows(_ptr(x), _ptr(a), _ptr(b), _ptr(noise), sd, dr, _ptr(hist), _ptr(xp), _ptr(x0), B, T, C, o.ov, right, ff, w,
                                     (L_.StepCoefs * B)(*coefs), _stream())
    torch.cuda.synchronize()
    if raw:
        return rc
    L_.check(rc, 'mc_op_sampler_seam_rows')


def _plain_rows_op(o, coefs, x, a, b, noise, hist, xp, x0):
    L_, lib, _ptr, _stream = _lib()
    B, T, C = o.shape
    L_.check(lib.mc_op_sampler_rows(_ptr(x), _ptr(a), _ptr(b), _ptr(noise), _ptr(hist), _ptr(xp), _ptr(x0), B, T * C, (L_.StepCoefs * B)(*coefs),
                                    _stream()), 'mc_op_sampler_rows')
    torch.cuda.synchronize()


def _field(seed, draw, n):
    L_, lib, _ptr, _stream = _lib()
    z = torch.empty(n, device='cuda')
    L_.check(lib.mc_op_philox_normal(_ptr(z), None, n, seed & U64, draw, _stream()), 'mc_op_philox_normal')
    return z


# ---- 1. the context-free op -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'element_form'])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_seam_rows_op(mode, offset):
    rows = SR.plan_rows(K_RIGHT, K_FIRST, KT, KOV)
    o = Ops(rows, offset, seed=300 + 10 * mode + offset)
    req_coefs = _request_coefs(mode)
    coefs = [req_coefs[q] for q in K_REQ]
    ms = mode == 2
    sh, T, ov = o.shape, KT, KOV
    seam = torch.from_numpy(SR.seam_mask(rows, T, ov))[:, :, None].expand(*sh)
    pairs = SR.pairs(rows)
    assert sorted(pairs) == [(0, 4), (3, 0)] and bool(seam.any()) and not bool(seam.all())
    hist0 = o.hist.clone()
    if ms:
        hist0[2] = float('nan')                                                             # row 2 takes a first step: its history is not read
    xd, ad, bd, nd = o.dev(o.x), o.dev(o.a), o.dev(o.b), o.dev(o.noise)
    hist = o.dev(hist0) if ms else None
    xp, x0 = o.dev(), o.dev()
    _rows_op(o, coefs, xd, ad, bd, None if ms else nd, hist, xp, x0)
    XP, X0 = xp.view(sh).cpu(), x0.view(sh).cpu()
    assert bool(torch.isfinite(XP).all()) and bool(torch.isfinite(X0).all())
    # (a) one value per shared element, in both rows: x_prev, x0, history
    for l, r in pairs:
        assert torch.equal(XP[l, T - ov:], XP[r, :ov]) and torch.equal(X0[l, T - ov:], X0[r, :ov]), (l, r)
    if ms:
        assert torch.equal(hist.view(sh).cpu(), X0)                                         # the history holds this step's x0, seams included
    # (b) off the seams: the bits of the row kernels on the same operands (every row, those at first frame 0 among them)
    hist_p = o.dev(hist0) if ms else None
    xp_p, x0_p = o.dev(), o.dev()
    _plain_rows_op(o, coefs, xd, ad, bd, None if ms else nd, hist_p, xp_p, x0_p)
    XP_p, X0_p = xp_p.view(sh).cpu(), x0_p.view(sh).cpu()
    assert torch.equal(XP[~seam], XP_p[~seam]) and torch.equal(X0[~seam], X0_p[~seam])
    assert not torch.equal(X0[seam], X0_p[seam])                                            # ... and on them the blend did something
    # (c) the update arithmetic, without a tolerance: the row op on the coupled op's own x0 (a = x0, b = 0 passes it through exactly:
    # x0 + 0 is x0) with the noise / history a seam element takes -- the LEFT row's
    zeros = o.dev(torch.zeros(sh))
    n_left = o.dev(torch.from_numpy(SR.share_left(o.noise.numpy(), rows, ov)).float())
    h_left = o.dev(torch.from_numpy(SR.share_left(hist0.numpy(), rows, ov)).float()) if ms else None
    xp_c = o.dev()
    _plain_rows_op(o, coefs, xd, x0, zeros, None if ms else n_left, h_left, xp_c, None)
    assert torch.equal(xp_c.view(sh).cpu(), XP)
    # (d) the blended x0 against fp64 under 4m's bound
    A, Bn = f64(o.a), f64(o.b)
    mag = np.abs(A) + np.abs(Bn)
    wt = S.default_weights(ov)
    ref = SR.blend(A + Bn, rows, ov, wt)
    bound = 4 * EPS * mag
    for l, r in pairs:
        bl = 8 * EPS * (wt[:, None] * mag[r, :ov] + (1 - wt)[:, None] * mag[l, T - ov:])
        bound[l, T - ov:], bound[r, :ov] = bl, bl
    err = np.abs(f64(X0) - ref)
    sm = seam.numpy()
    print(f'mode {mode} offset {offset}: x0 err/bound on seams {float((err[sm] / bound[sm]).max()):.3f}, off seams {float((err[~sm] / bound[~sm]).max()):.3f}')
    assert bool((err <= bound).all())
    # ... and the whole step against the restatement (sanity of the restatement, loose: 1e-5 relative)
    hist_ref = np.nan_to_num(f64(hist0)) if ms else None
    ref_step, _ = SR.step(coefs, f64(o.x), A, Bn, rows, ov, wt, noise=None if ms else f64(o.noise), hist=hist_ref)
    assert np.allclose(f64(XP), ref_step, rtol=0, atol=1e-5 * (1 + np.abs(ref_step).max()))
    # (e) in place = out of place (a right neighbour at a lower row index included)
    x_in = o.dev(o.x)
    hist_in = o.dev(hist0) if ms else None
    _rows_op(o, coefs, x_in, ad, bd, None if ms else nd, hist_in, x_in, None)
    assert torch.equal(x_in.view(sh).cpu(), XP)
    if ms:
        assert torch.equal(hist_in.view(sh).cpu(), X0)
    # (g) device noise = host noise fed the requests' global fields, gathered per row: draw 0 and draw 1 + k
    if not ms:
        seeds = [K_SEEDS[q] for q in K_REQ]
        for draw in (0, 1 + 3):
            fields = [_field(K_SEEDS[q], draw, (f + T) * KC).cpu().numpy() for q, (_, _, f) in zip(K_REQ, rows)]
            gathered = torch.from_numpy(SR.gather_field(fields, rows, T, KC)).float()
            for l, r in pairs:
                assert torch.equal(gathered[l, T - ov:], gathered[r, :ov])                  # the same global index: the same normal
            pz = o.dev(gathered)
            xp_h, xp_d, x0_d = o.dev(), o.dev(), o.dev()
            _rows_op(o, coefs, xd, ad, bd, pz, None, xp_h, None)
            _rows_op(o, coefs, xd, ad, bd, None, None, xp_d, x0_d, seeds=seeds, draws=[draw] * KB)
            assert torch.equal(xp_h, xp_d) and torch.equal(x0_d.view(sh).cpu(), X0), draw
            assert not torch.equal(xp_d.view(sh).cpu(), XP)                                # (other noise than the first run's)
    # (h) weights 0 / 1: the left / the right window's x0, bit for bit
    for wv, side in ((0.0, 'left'), (1.0, 'right')):
        x0_w, xp_w = o.dev(), o.dev()
        hist_w = o.dev(hist0) if ms else None
        _rows_op(o, coefs, xd, ad, bd, None if ms else nd, hist_w, xp_w, x0_w, weights=[wv] * ov)
        X0w = x0_w.view(sh).cpu()
        for l, r in pairs:
            want = X0_p[l, T - ov:] if side == 'left' else X0_p[r, :ov]
            assert torch.equal(X0w[l, T - ov:], want) and torch.equal(X0w[r, :ov], want), (side, l, r)
        assert torch.equal(X0w[~seam], X0_p[~seam])
    # (f) nothing was stored before or behind any operand or output
    assert o.guards_intact()


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'element_form'])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_uniform_adjacent_rows_give_the_whole_batch_seam_kernels_bits(mode, offset):
    """one entry for every row, neighbours b -> b + 1, host noise: sampler_seam_rows_k == sampler_seam_k, bit for bit"""
    L_, lib, _ptr, _stream = _lib()
    ff = [0, KSTRIDE, 2 * KSTRIDE, 40, 40 + KSTRIDE]
    flags = S.plan_flags(ff, KT, KOV)
    rows = SR.plan_rows([b + 1 if fl[1] else -1 for b, fl in enumerate(flags)], ff, KT, KOV)
    assert SR.pairs(rows) == [(0, 1), (1, 2), (3, 4)]
    o = Ops(rows, offset, seed=400 + 10 * mode + offset)
    c = _unit(_request_coefs(mode)[0])
    ms = mode == 2
    xd, ad, bd, nd = o.dev(o.x), o.dev(o.a), o.dev(o.b), o.dev(o.noise)
    h1, h2 = (o.dev(o.hist), o.dev(o.hist)) if ms else (None, None)
    xp1, x01, xp2, x02 = o.dev(), o.dev(), o.dev(), o.dev()
    _rows_op(o, [c] * KB, xd, ad, bd, None if ms else nd, h1, xp1, x01)
    L_.check(lib.mc_op_sampler_seam(_ptr(xd), _ptr(ad), _ptr(bd), None if ms else _ptr(nd), 0, 0, _ptr(h2), _ptr(xp2), _ptr(x02), KB, KT, KC, KOV,
                                    (ctypes.c_int32 * KB)(*ff), None, ctypes.byref(c), _stream()), 'mc_op_sampler_seam')
    torch.cuda.synchronize()
    assert torch.equal(xp1, xp2) and torch.equal(x01, x02)
    if ms:
        assert torch.equal(h1, h2)
    assert o.guards_intact()


def test_first_frames_past_two_to_the_31_elements():
    """a chain whose first_frame * C exceeds 2^31: the counters are 64-bit -- device noise equals the request's field at those indices"""
    first = [BIG + KSTRIDE, 0, 5, BIG, BIG + 2 * KSTRIDE]
    rows = SR.plan_rows(K_RIGHT, first, KT, KOV)
    assert BIG * KC > 2 ** 31
    o = Ops(rows, 0, seed=500)
    coefs = [_request_coefs(0)[q] for q in K_REQ]
    seeds = [K_SEEDS[q] for q in K_REQ]
    draw = 2
    big = _field(K_SEEDS[0], draw, (BIG + 2 * KSTRIDE + KT) * KC)                           # the long request's field, 8.6 GB, on the device
    gathered = torch.empty(o.shape, device='cuda')
    for b, (_, _, f) in enumerate(rows):
        src = big if K_REQ[b] == 0 else _field(seeds[b], draw, (f + KT) * KC)
        gathered[b] = src[f * KC:(f + KT) * KC].view(KT, KC)
    del big
    torch.cuda.empty_cache()
    xd, ad, bd = o.dev(o.x), o.dev(o.a), o.dev(o.b)
    pz = o.dev(gathered.cpu())
    xp_h, xp_d = o.dev(), o.dev()
    _rows_op(o, coefs, xd, ad, bd, pz, None, xp_h, None)
    _rows_op(o, coefs, xd, ad, bd, None, None, xp_d, None, seeds=seeds, draws=[draw] * KB)
    assert torch.equal(xp_h, xp_d)
    low = _field(K_SEEDS[0], draw, KT * KC).view(KT, KC)
    assert not torch.equal(low, gathered[3])                                                # (not the counters of first frame 0)
    XP = xp_d.view(o.shape)
    for l, r in SR.pairs(rows):
        assert torch.equal(XP[l, KT - KOV:], XP[r, :KOV])
    assert o.guards_intact()


def test_op_refusals_launch_nothing():
    L_, lib, _ptr, _stream = _lib()
    rows = SR.plan_rows(K_RIGHT, K_FIRST, KT, KOV)
    o = Ops(rows, 0, seed=1)
    xd, ad, bd, nd, xp = o.dev(o.x), o.dev(o.a), o.dev(o.b), o.dev(o.noise), o.dev()
    req = _request_coefs(1)
    good = [req[q] for q in K_REQ]

    def call(right=K_RIGHT, first=K_FIRST, ov=KOV, coefs=good, weights=None, seeds=None, draws=None, noise=nd):
        bad = Ops.__new__(Ops)
        bad.shape, bad.ov, bad.rows = o.shape, ov, list(zip(right, [False] * KB, first))
        return _rows_op(bad, coefs, xd, ad, bd, noise, None, xp, None, weights=weights, seeds=seeds, draws=draws, raw=True)
    cases = dict(
        self_right=dict(right=[4, 1, -1, 0, -1]), out_of_range=dict(right=[5, -1, -1, 0, -1]), named_twice=dict(right=[4, -1, 4, 0, -1]),
        not_a_stride=dict(first=[KSTRIDE + 1, 0, 5, 0, 2 * KSTRIDE]), negative=dict(first=[KSTRIDE, -1, 5, 0, 2 * KSTRIDE]),
        cycle=dict(right=[3, -1, -1, 0, -1], first=[KSTRIDE, 0, 5, 0, 0]), overlap_0=dict(ov=0), overlap_wide=dict(ov=4),
        weight=dict(weights=[0.5, 0.5, 1.5]), seam_coefs_differ=dict(coefs=[req[1]] + good[1:]),
        seam_seeds_differ=dict(seeds=[1, 2, 3, 4, 1], draws=[1] * KB, noise=None), seam_draws_differ=dict(seeds=[1, 2, 3, 1, 1], draws=[1, 1, 1, 2, 1], noise=None),
        two_noise_sources=dict(seeds=[1, 2, 3, 1, 1], draws=[1] * KB), mixed_modes=dict(coefs=good[:1] + [_request_coefs(0)[1]] + good[2:]))
    for name, kw in cases.items():
        assert call(**kw) == L_.MC_ERR_ARG, name
        assert 'mc_op_sampler_seam_rows' in L_.last_error() or name == 'mixed_modes', name
    assert bool((xp == 777.0).all())
    assert call() == L_.MC_OK and not bool((xp == 777.0).any())


# ---- 2. the context ---------------------------------------------------------------------------------------------------------------
C = 322
T, OV = 24, 6
STRIDE = T - OV
CB = 4
SEED_L, SEED_S = 901, 2 ** 63 + 17
LAYOUTS = {'scattered': ([2, 0, 3], 1), 'packed': ([0, 1, 2], 3)}      # the rows of the long request's windows 0, 1, 2; the short request's row
LEAD = 2                                                              # the short request starts this many ticks before the long one
TICKS = 4                                                             # ticks with the long request in the batch


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


def _xf(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.layer_norm(torch.randn(n, SMALL['Nt'], SMALL['Dt'], generator=g), (SMALL['Dt'],))


def _table(long_rows):
    right, first = [-1] * CB, [0] * CB
    for j, b in enumerate(long_rows):
        right[b] = long_rows[j + 1] if j + 1 < len(long_rows) else -1
        first[b] = j * STRIDE
    return right, first


def _walk_coefs(d, mode, scale):
    idx = list(range(d.num_timesteps))[::-1]
    if mode == 'dpmpp':
        return d.multistep_coefs(idx, scale, 2)
    return [d.step_coefs(i, mode, scale, 0.5 if mode == 'ddim' else 0.0) for i in idx]


def _ctx_walk(nm, mode, layout, table=True, clear_after=None, inject=None):
    """the short request (scale 2.0) walks from tick 0; the long one (W = 3, the model's scale) joins at tick LEAD, the way the batcher
    admits it: its rows' condition fresh, x_T gathered from draw 0 of its field, the table set.  Until then its rows run the dummy at walk
    position 0.  -> per tick with the long request: (x before, schedule index per row, x after, x0)"""
    L_, lib, _ptr, _stream = _lib()
    d = _diffusion()
    long_rows, short_row = LAYOUTS[layout]
    right, first = _table(long_rows)
    xfs = _xf(2, 60)
    xf = torch.stack([xfs[1] if b == short_row else xfs[0] for b in range(CB)]).cuda()
    mask = torch.ones(CB, T, device='cuda')
    seeds = [SEED_S if b == short_row else SEED_L for b in range(CB)]
    walks = {False: _walk_coefs(d, mode, 2.0), True: _walk_coefs(d, mode, SMALL['scale'])}
    ctx = nm.context(CB, T, max_steps=d.num_timesteps)
    out = []
    try:
        ctx.set_capacity_factor(0)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf, mask)
        ctx.set_row_seeds(seeds)
        x = torch.zeros(CB, T, C, device='cuda')
        x[short_row] = _field(SEED_S, 0, T * C).view(T, C)
        x0 = torch.empty_like(x)
        for k in range(LEAD + TICKS):
            if k == LEAD:
                ctx.set_condition_rows(xf, mask, [b != short_row for b in range(CB)])
                z = _field(SEED_L, 0, (2 * STRIDE + T) * C).view(-1, C)
                for b in long_rows:
                    x[b] = z[first[b]:first[b] + T]
                if table:
                    ctx.set_seam_rows(right, first, OV)
            if clear_after is not None and k == LEAD + clear_after:
                ctx.clear_seam_rows()
            if inject is not None and k in inject:
                x.copy_(inject[k])
            pos = [k if b == short_row else max(k - LEAD, 0) for b in range(CB)]
            idx = [d.num_timesteps - 1 - p for p in pos]
            coefs = [walks[b != short_row][p] for b, p in enumerate(pos)]
            before = x.clone()
            ctx.sample_rows(x, [idx], [coefs], draws=None if mode == 'dpmpp' else [[1 + p for p in pos]], x0=x0)
            torch.cuda.synchronize()
            if k >= LEAD:
                out.append((before.cpu(), idx, x.clone().cpu(), x0.clone().cpu()))
    finally:
        ctx.close()
    return out


@pytest.fixture(scope='module')
def ctx_walks(small):
    sd, arch = small
    nm = arch.model.native
    return {(mode, layout, table): _ctx_walk(nm, mode, layout, table)
            for mode in ('ddim', 'dpmpp') for layout, table in (('scattered', True), ('packed', True), ('scattered', False))}


def _stitched(x, long_rows):
    return torch.cat([x[b, :STRIDE] for b in long_rows[:-1]] + [x[long_rows[-1]]])


@pytest.mark.parametrize('mode', ['ddim', 'dpmpp'])
def test_context_rows_2_0_3_beside_a_short_request_at_another_step(ctx_walks, mode):
    sc, pk, plain = (ctx_walks[(mode, l, t)] for l, t in (('scattered', True), ('packed', True), ('scattered', False)))
    (rows_s, short_s), (rows_p, short_p) = LAYOUTS['scattered'], LAYOUTS['packed']
    table = SR.plan_rows(*_table(rows_s), T, OV)
    assert SR.pairs(table) == [(0, 3), (2, 0)]
    for k in range(TICKS):
        before, idx, x, x0 = sc[k]
        assert idx[short_s] != idx[rows_s[0]] and bool(torch.isfinite(x).all())
        assert SR.seams_equal(before.numpy(), table, OV)
        assert SR.seams_equal(x.numpy(), table, OV) and SR.seams_equal(x0.numpy(), table, OV), (mode, k)      # after every tick
        assert not SR.seams_equal(plain[k][2].numpy(), table, OV)                           # (without a table the windows drift apart)
        assert torch.equal(x[short_s], plain[k][2][short_s]) and torch.equal(x0[short_s], plain[k][3][short_s])   # the short row never notices
        assert torch.equal(x[short_s], pk[k][2][short_p])
        assert torch.equal(_stitched(x, rows_s), _stitched(pk[k][2], rows_p)), (mode, k)   # the rows a request lands in do not matter
        assert torch.equal(_stitched(x0, rows_s), _stitched(pk[k][3], rows_p))


@pytest.mark.parametrize('mode', ['ddim', 'dpmpp'])
def test_context_x0_meets_the_oracle_per_window_blended(small, ctx_walks, mode):
    """teacher-forced: at the device's own x of every tick, the oracle's per-row x0 (each row at its own timestep and scale, nothing
    dropped), blended in fp64 (the blend is convex: it adds nothing to the denoiser's bound)"""
    sd, _ = small
    d = _diffusion()
    rows_s, short_s = LAYOUTS['scattered']
    table = SR.plan_rows(*_table(rows_s), T, OV)
    xfs = _xf(2, 60)
    xf = torch.stack([xfs[1] if b == short_s else xfs[0] for b in range(CB)])
    torch.set_num_threads(4)
    worst = 0.0
    for before, idx, _, x0 in ctx_walks[(mode, 'scattered', True)]:
        ts = [int(d.timestep_map[i]) for i in idx]
        scales = [2.0 if b == short_s else SMALL['scale'] for b in range(CB)]
        ref = rowstep_ref.denoise_rows(sd, SMALL, before, ts, xf, torch.ones(CB, T), capacity_factor=float(SMALL['E']), scales=scales)
        err = float(np.abs(f64(x0) - SR.blend(ref.double().numpy(), table, OV)).max())
        worst = max(worst, err)
    print(f'{mode}: worst |x0 - blended oracle| over {TICKS} ticks {worst:.2e}')
    assert worst <= TOL_STEP


def test_after_clear_seam_rows_the_context_gives_the_plain_rows_walk(small, ctx_walks):
    """one tick WITH the table, then clear_seam_rows: the next tick is the plain row kernels' -- bit-equal to the same tick of a context
    that never held a table, started from the same x (DDIM: no history to carry); and set-then-clear before any tick leaves no trace"""
    sd, arch = small
    nm = arch.model.native
    plain = ctx_walks[('ddim', 'scattered', False)]
    coupled = ctx_walks[('ddim', 'scattered', True)]
    got = _ctx_walk(nm, 'ddim', 'scattered', table=True, clear_after=1)
    assert torch.equal(got[0][2], coupled[0][2]) and not torch.equal(got[0][2], plain[0][2])      # tick 0 ran coupled
    assert not torch.equal(got[1][2], coupled[1][2])                                               # tick 1 did not
    ref = _ctx_walk(nm, 'ddim', 'scattered', table=False, inject={LEAD + 1: got[1][0].cuda()})
    assert torch.equal(ref[1][0], got[1][0]) and torch.equal(ref[1][2], got[1][2]) and torch.equal(ref[1][3], got[1][3])
    none = _ctx_walk(nm, 'ddim', 'scattered', table=True, clear_after=0)
    assert all(torch.equal(g[2], p[2]) and torch.equal(g[3], p[3]) for g, p in zip(none, plain))


def test_context_refusals_leave_the_context_as_it_was(small):
    L_, lib, _ptr, _stream = _lib()
    sd, arch = small
    nm = arch.model.native
    d = _diffusion()
    idx = list(range(d.num_timesteps))[::-1]
    ddim = [d.step_coefs(i, 'ddim', SMALL['scale']) for i in idx]
    rows_s, short_s = LAYOUTS['scattered']
    right, first = _table(rows_s)
    ctx = nm.context(CB, T, max_steps=10)
    ctx.set_capacity_factor(0)
    ctx.set_timesteps(d.timestep_map)
    ctx.set_condition(_xf(CB, 61).cuda(), torch.ones(CB, T, device='cuda'))
    ctx.set_row_seeds([SEED_S if b == short_s else SEED_L for b in range(CB)])
    x = torch.randn(CB, T, C, generator=torch.Generator().manual_seed(5)).cuda()

    def code(rc):
        return pytest.raises(RuntimeError, match=rf'\(code {rc}\)')

    def raw_set(right_, first_, ov, w=None):
        warr = (ctypes.c_float * len(w))(*w) if w is not None else None
        return lib.mc_ctx_set_seam_rows(ctx.handle, ov, (ctypes.c_int32 * CB)(*right_), (ctypes.c_int32 * CB)(*first_), warr, _stream())

    def tick(rows_idx=None, coefs=None, draws=None, xx=None):
        xx = x.clone() if xx is None else xx
        ctx.sample_rows(xx, [rows_idx or [9] * CB], [coefs or [ddim[0]] * CB], draws=[draws or [1] * CB])
        torch.cuda.synchronize()
        return xx
    ctx.set_seam_rows(right, first, OV)
    want = tick()
    # every table the rules refuse: MC_ERR_ARG, and the table that was set stays set (the next tick gives the same bits)
    bad = [([0, -1, 0, -1], first, OV), ([3, -1, 0, 4], first, OV), ([3, -1, 3, -1], first, OV), (right, [STRIDE + 1, 0, 0, 2 * STRIDE], OV),
           (right, [STRIDE, -2, 0, 2 * STRIDE], OV), ([3, -1, 0, 2], [STRIDE, 0, 0, 2 * STRIDE], OV), (right, first, 13), (right, first, -2)]
    for r_, f_, ov in bad:
        assert raw_set(r_, f_, ov) == L_.MC_ERR_ARG, (r_, f_, ov)
        assert 'mc_ctx_set_seam_rows' in L_.last_error()
    assert raw_set(right, first, OV, [0.5] * 5 + [1.5]) == L_.MC_ERR_ARG and 'weight' in L_.last_error()
    assert lib.mc_ctx_set_seam_rows(ctx.handle, OV, None, None, None, _stream()) == L_.MC_ERR_ARG
    assert torch.equal(tick(), want)
    # the rows of a seam must walk together: step index, coefficients, draw number, seed
    other = d.step_coefs(9, 'ddim', 2.0)
    for kw in (dict(rows_idx=[9, 9, 8, 9]), dict(coefs=[ddim[0], ddim[0], other, ddim[0]]), dict(draws=[1, 1, 1, 2])):
        xx = x.clone()
        with code(L_.MC_ERR_ARG):
            tick(xx=xx, **kw)
        assert 'share a seam' in L_.last_error() and torch.equal(xx, x)
    ctx.set_row_seeds([SEED_L, SEED_S, SEED_L + 1, SEED_L])
    with code(L_.MC_ERR_ARG):
        tick()
    assert 'seed' in L_.last_error()
    ctx.set_row_seeds([SEED_S if b == short_s else SEED_L for b in range(CB)])
    # with a table set: every entry without a rows form, the whole-batch seam table, an edit table, graph capture
    nz = torch.zeros_like(x)
    for call in (lambda: ctx.sample_step(x, idx[0], ddim[0], nz), lambda: ctx.sample_loop(x.clone(), idx[:2], ddim[:2], noise=torch.zeros(2, CB, T, C, device='cuda')),
                 lambda: ctx.sample_step_inpaint(x, idx[0], ddim[0], nz, nz, torch.zeros(CB, T, C, dtype=torch.bool, device='cuda'), gt_noise=nz),
                 lambda: ctx.sample_step_seeded(x, idx[0], ddim[0], nz, 1.0, 0.0),
                 lambda: ctx.set_seams([0, STRIDE, 2 * STRIDE, 100], OV),
                 lambda: ctx.set_edit_rows(nz, torch.zeros(CB, T, C, dtype=torch.uint8, device='cuda'))):
        with code(L_.MC_ERR_STATE):
            call()
        assert 'row seam table' in L_.last_error()
    assert lib.mc_ctx_graph_step(ctx.handle, 0, _stream()) == L_.MC_ERR_STATE and 'row seam table' in L_.last_error()
    # mode 2: the rows of a seam share their history flag.  One dpmpp tick gives every row a history; a condition call that makes
    # only ONE row of the seam (2, 0) fresh clears that row's flag alone: refused, x untouched; both rows fresh: served
    ms = d.multistep_coefs(idx, SMALL['scale'], 2)
    xf_c, mask_c = _xf(CB, 61).cuda(), torch.ones(CB, T, device='cuda')
    xm = x.clone()
    ctx.sample_rows(xm, [[idx[0]] * CB], [[ms[0]] * CB])
    ctx.set_condition_rows(xf_c, mask_c, [False, False, True, False])
    kept = xm.clone()
    with code(L_.MC_ERR_ARG):
        ctx.sample_rows(xm, [[idx[0]] * CB], [[ms[0]] * CB])
    assert 'history flag' in L_.last_error() and torch.equal(xm, kept)
    ctx.set_condition_rows(xf_c, mask_c, [True, False, True, True])
    ctx.sample_rows(xm, [[idx[0]] * CB], [[ms[0]] * CB])
    torch.cuda.synchronize()
    assert not torch.equal(xm, kept)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gx, gn = torch.empty_like(x), torch.zeros_like(x)
        with code(L_.MC_ERR_STATE):
            ctx.graph_capture(gx, gn, ddim[::-1])
        assert 'row seam table' in L_.last_error()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(tick(), want)                                       # the table is still the one that was set
    # the other way round: a whole-batch seam table, an edit table or a captured graph in the context refuse the row table
    ctx.clear_seam_rows()
    plain = tick()
    assert not torch.equal(plain, want)
    ctx.set_seams([0, STRIDE, 2 * STRIDE, 100], OV)
    assert raw_set(right, first, OV) == L_.MC_ERR_STATE and 'mc_ctx_set_seams' in L_.last_error()
    ctx.clear_seams()
    ctx.set_edit_rows(nz, torch.zeros(CB, T, C, dtype=torch.uint8, device='cuda'))
    assert raw_set(right, first, OV) == L_.MC_ERR_STATE and 'edit table' in L_.last_error()
    ctx.clear_edit_rows()
    with torch.cuda.stream(side):
        ctx.graph_capture(gx, gn, ddim[::-1])
        assert raw_set(right, first, OV) == L_.MC_ERR_STATE and 'graph' in L_.last_error()
        ctx.graph_release()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(tick(), plain)
    ctx.close()


# ---- 3. the batcher ---------------------------------------------------------------------------------------------------------------
def _long_request(F, seed=SEED_L, scale=None):
    from motioncraft_amd.serve import Request
    return Request(length=F, seed=seed, xf_out=_xf(1, 70)[0], guidance_scale=scale)


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp'])
def test_a_batcher_of_w_rows_is_sample_long_coupled(small, sampler):
    """one long request on the grid, F = T + (W - 1) stride, alone in a batcher of exactly W rows, against the whole-batch path of
    section 4m at capacity factor 0, fed the same x_T (draw 0 of the request's field): bit-equal"""
    from motioncraft_amd import longform
    from motioncraft_amd.serve import ContinuousBatcher
    sd, arch = small
    W = 3
    F = T + (W - 1) * STRIDE
    R = _long_request(F)
    bt = ContinuousBatcher(arch, batch=W, frames=T, sampler=sampler, overlap=OV)
    h = bt.submit(R)
    got = bt.run()[h]
    torch.cuda.synchronize()
    assert tuple(got.shape) == (F, C) and bool(torch.isfinite(got).all())
    z = _field(R.seed, 0, F * C).view(F, C).cpu()
    old = arch.inference_type
    arch.inference_type = sampler
    try:
        recs, _ = longform.sample_long_coupled(arch, [F], T, OV, text=['a'], noise=[z], condition_kwargs=dict(xf_out=R.xf_out[None].cuda()),
                                               input_dim=C, inference_kwargs=dict(capacity_factor=0), shard=False)
    finally:
        arch.inference_type = old
    assert recs[0].shape == (F, C)
    assert np.array_equal(got.cpu().numpy(), recs[0]), float(np.abs(got.cpu().numpy() - recs[0]).max())


def _serve(arch, arrivals, sampler='ddim', batch=CB, steps=6, eta=0.5):
    """arrivals: [(tick, Request)] -> (result of the LAST request, its rows, submitted_at, finished_at, the batcher)"""
    from motioncraft_amd.serve import ContinuousBatcher
    bt = ContinuousBatcher(arch, batch=batch, frames=T, sampler=sampler, steps=steps, eta=eta, overlap=OV)
    rows, out, k, h = {}, {}, 0, None
    for _ in range(60):
        while k < len(arrivals) and arrivals[k][0] <= bt.ticks:
            h = bt.submit(arrivals[k][1])
            k += 1
        bt.tick()
        for b, h_ in enumerate(bt.occupied):
            if h_ is not None:
                rows.setdefault(h_, set()).add(b)
        out.update(bt.poll())
        if k == len(arrivals) and not any(h_ is not None for h_ in bt.occupied):
            break
    torch.cuda.synchronize()
    return out[h].clone(), sorted(rows[h]), bt.submitted_at[h], bt.finished_at[h], bt


def test_a_long_request_joining_at_tick_3_gets_the_bits_it_gets_alone(small):
    """ddim6 with eta 0.5 (noise is drawn every step): W = 3 in rows (0, 1, 2) from tick 0 of an empty batch; the same request admitted
    at tick 3 into rows (1, 2, 3) beside a short request mid-walk with another prompt, seed and guidance scale"""
    from motioncraft_amd.serve import Request
    sd, arch = small
    F = T + 2 * STRIDE
    R = _long_request(F)
    other = Request(length=17, seed=5, xf_out=_xf(1, 71)[0], guidance_scale=1.25)
    alone, rows_a, t0_a, t1_a, _ = _serve(arch, [(0, R)])
    joined, rows_j, t0_j, t1_j, _ = _serve(arch, [(0, other), (3, R)])
    assert (rows_a, t0_a, t1_a) == ([0, 1, 2], 0, 6) and (rows_j, t0_j, t1_j) == ([1, 2, 3], 3, 9)
    assert tuple(alone.shape) == (F, C) and bool(torch.isfinite(alone).all())
    assert torch.equal(alone, joined), float((alone - joined).abs().max())


def test_a_ddpm_walk_on_device_noise_keeps_its_seams(small):
    sd, arch = small
    F = T + 2 * STRIDE
    _, rows, _, _, bt = _serve(arch, [(0, _long_request(F, seed=SEED_S))], sampler='ddpm', batch=3, steps=5, eta=0.0)
    x = bt.runner.x.cpu()                                                  # the windows as the walk left them
    table = SR.plan_rows([1, 2, -1], [0, STRIDE, 2 * STRIDE], T, OV)
    assert rows == [0, 1, 2] and bool(torch.isfinite(x).all()) and SR.seams_equal(x.numpy(), table, OV)
    assert bt.runner.ctx.seam_rows is None                                 # the last long request left: the table is cleared


def test_a_ragged_last_window(small):
    """F off the grid: the result has F frames, and its first (W - 1) stride frames are those of the same walk driven by hand -- three
    rows, the last one's motion_mask cut to the ragged length"""
    from motioncraft_amd.serve import ContinuousBatcher
    sd, arch = small
    F = T + 2 * STRIDE - 7                                                 # windows of 24, 24, 17 frames
    R = _long_request(F)
    bt = ContinuousBatcher(arch, batch=3, frames=T, sampler='ddim', steps=6, eta=0.5, overlap=OV)
    h = bt.submit(R)
    got = bt.run()[h]
    assert tuple(got.shape) == (F, C) and bool(torch.isfinite(got).all())
    by_hand = ContinuousBatcher(arch, batch=3, frames=T, sampler='ddim', steps=6, eta=0.5, overlap=OV).runner
    by_hand.condition(R.xf_out[None].repeat(3, 1, 1), [T, T, T - 7], [R.seed] * 3, [True] * 3, None, first_frames=[0, STRIDE, 2 * STRIDE])
    by_hand.seams([1, 2, -1], [0, STRIDE, 2 * STRIDE])
    by_hand.advance([[k] * 3 for k in range(6)], [None] * 3)
    out = by_hand.result()
    by_hand.clear_seams()
    torch.cuda.synchronize()
    assert torch.equal(got[:2 * STRIDE].cpu(), torch.cat([out[0, :STRIDE], out[1, :STRIDE]]).cpu())
    assert torch.equal(got[2 * STRIDE:].cpu(), out[2, :T - 7].cpu())

"""GPU (MI355X): rows of one batch at their own schedule index and guidance scale -- ``mc_sample_rows`` / ``mc_denoise_rows`` /
``mc_ctx_set_condition_rows``, the per-row kernel forms behind them and ``serve.ContinuousBatcher``.

Shapes are those of tests/test_independent_gpu.py: the reduced config (``helpers.SMALL``: L = 32, NL = 2, C = 322) at B = 3, T = 24, lengths
(24, 17, 20), and C = 263 at T = 23 (``HML_SMALL``), where a flat group of four straddles two rows.  Device against device is exact
(torch.equal); oracle comparisons use the project's bounds (2e-4 per call, 1e-3 per trajectory)."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest
import torch

import rowstep_ref
from helpers import CTRL, CTRL_COPY, CTRL_FEATS, CTRL_TC, HML_SMALL, SMALL, SMALL_SEED, skew_gates, synth_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B, T = 3, 24
LENGTHS = (24, 17, 20)
SEEDS = [11, 2 ** 63 + 5, 11 + 2 ** 32]
BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
TOL_CALL, TOL_TRAJ = 2e-4, 1e-3
SHAPES = {'C322_T24': (SMALL, 24), 'C263_T23': (HML_SMALL, 23)}


@pytest.fixture(autouse=True)
def time_limit():
    """every test here under its own time limit: a hung launch ends the process instead of the session waiting on it"""
    faulthandler.dump_traceback_later(180, exit=True)
    threads = torch.get_num_threads()
    yield
    torch.set_num_threads(threads)
    faulthandler.cancel_dump_traceback_later()


def _lib():
    from motioncraft_amd import lib as L_
    from motioncraft_amd.engine import _ptr, _stream
    return L_.load(require_gpu=True), _ptr, _stream


def _diffusion(respace):
    from motioncraft_amd.diffusion import build_diffusion
    return build_diffusion(dict(BASE, respace=respace))


@pytest.fixture(scope='module')
def natives():
    """shape id -> (dims, state dict, NativeModel); SMALL with hot_pair gates (the default capacity factor really drops tokens)"""
    from motioncraft_amd.engine import NativeModel
    from oracle import weights as W
    made = {}

    def get(name):
        if name not in made:
            dims, _ = SHAPES[name]
            sd = W.make_state_dict(dims, SMALL_SEED)
            if dims is SMALL:
                sd = skew_gates(sd, dims, 'hot_pair')
            made[name] = (dims, sd, NativeModel(dims, sd, cfg_scale=dims['scale']))
        return made[name]
    yield get
    for _, _, nm in made.values():
        nm.close()


@pytest.fixture(scope='module')
def arch():
    import motioncraft_amd as mc
    from oracle import weights as W
    sd = skew_gates(W.make_state_dict(SMALL, SMALL_SEED), SMALL, 'hot_pair')
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_small.py'))
    cfg.model.diffusion_test = dict(BASE, respace='ddim10')
    a = mc.build_architecture(cfg.model)
    a.load_state_dict({'model.' + k: v for k, v in sd.items()})
    yield sd, a
    a.model.release()


# schedule / precision variants of a context: name -> (MC_ROUTE_SMALL_CTX or None, options, precision)
VARIANTS = {
    'default': (None, {}, 'f32'),
    'two_groups': ('0', {'big_tokens': 0, 'route_early': 1}, 'f32'),          # the forced large-batch schedule (FiLM launches with row0 != 0)
    'f16x3': (None, {'half_min_rows': 0}, 'f16x3'),                           # fp16 hi / lo planes out of film_rows_k
    'tail2': (None, {'small_gemm_rows': 0}, 'f32'),                           # the one-pass decoder tail, block-range form (gemm_tail2_k)
    'tail1': (None, {'small_gemm_rows': 0, 'gemm_tune': 817}, 'f32'),         # ... and the column-tile form (gemm_tail_k)
}


def _context(nm, monkeypatch, variant, Tn, d, xf, mask, cf=None):
    env, options, prec = VARIANTS[variant]
    if env is not None:
        monkeypatch.setenv('MC_ROUTE_SMALL_CTX', env)
    ctx = nm.context(B, Tn, max_steps=d.num_timesteps)
    for k, v in options.items():
        ctx.set_option(k, v)
    if prec != 'f32':
        ctx.set_precision(prec)
        assert ctx.effective_precision == prec
    if cf is not None:
        ctx.set_capacity_factor(cf)
    ctx.set_timesteps(d.timestep_map)
    ctx.set_condition(xf.cuda(), mask.cuda())
    return ctx


def _walk_coefs(d, dims, mode, scale=None):
    idx = list(range(d.num_timesteps))[::-1]
    scale = dims['scale'] if scale is None else scale
    if mode == 'dpmpp':
        return idx, d.multistep_coefs(idx, scale, 2)
    return idx, [d.step_coefs(i, mode, scale, 0.5 if mode == 'ddim' else 0.0) for i in idx]


# ---- 1. uniform tables ----------------------------------------------------------------------------------
CASES_1 = [(v, m, 'C322_T24') for v in ('default', 'two_groups', 'f16x3') for m in ('ddpm', 'ddim', 'dpmpp')] + \
          [('tail2', 'ddim', 'C322_T24'), ('tail1', 'dpmpp', 'C322_T24'), ('default', 'ddpm', 'C263_T23'), ('default', 'dpmpp', 'C263_T23')]


@pytest.mark.parametrize('variant,mode,shape', CASES_1, ids=['-'.join(c) for c in CASES_1])
def test_uniform_tables_give_the_uniform_entries_bits(natives, monkeypatch, variant, mode, shape):
    """every row at the same index and coefficients: two single ticks of mc_sample_rows == two mc_sample_step calls on a noise tensor,
    and six ticks in one call == mc_sample_loop under a seed table (draw 1 + k), bit for bit -- x and the last x0"""
    dims, _, nm = natives(shape)
    Tn, C = SHAPES[shape][1], dims['input_feats']
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, Tn, seed=91, lengths=[Tn, Tn - 7, Tn - 4])
    idx, coefs = _walk_coefs(d, dims, mode)
    noise = torch.randn(2, B, Tn, C, generator=torch.Generator().manual_seed(92)).cuda()
    ctx = _context(nm, monkeypatch, variant, Tn, d, xf, mask)
    try:
        def fresh():
            ctx.set_condition(xf.cuda(), mask.cuda())       # (clears the multistep history: every walk starts without one)
            return x_T.cuda().clone(), torch.empty(B, Tn, C, device='cuda')
        xa, x0a = fresh()
        for k in range(2):
            ctx.sample_step(xa, idx[k], coefs[k], None if mode == 'dpmpp' else noise[k], x_prev=xa, x0=x0a)
        xb, x0b = fresh()
        for k in range(2):
            ctx.sample_rows(xb, [[idx[k]] * B], [[coefs[k]] * B], noise=None if mode == 'dpmpp' else noise[k:k + 1], x0=x0b)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xa).all())
        assert torch.equal(xa, xb), float((xa - xb).abs().max())
        assert torch.equal(x0a, x0b)
        ctx.set_row_seeds(SEEDS)
        xc, x0c = fresh()
        ctx.sample_loop(xc, idx, coefs, noise=None, draw0=1, x0=x0c)
        xd, x0d = fresh()
        ctx.sample_rows(xd, [[i] * B for i in idx], [[c] * B for c in coefs], draws=[[1 + k] * B for k in range(6)], x0=x0d)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(xc).all()) and not torch.equal(xc, x_T.cuda())
        assert torch.equal(xc, xd), float((xc - xd).abs().max())
        assert torch.equal(x0c, x0d)
        ctx.check()
    finally:
        ctx.close()


@pytest.mark.parametrize('mode', ['ddpm', 'ddim'])
def test_every_row_draws_at_its_own_draw_number_where_groups_straddle_rows(natives, mode):
    """C = 263, T = 23 (T C % 4 = 1: flat groups of four straddle both row boundaries), rows at steps (5, 3, 2) with draw numbers
    (1, 4, 2): the in-kernel draw equals the same tick fed a noise tensor whose row b is row b of mc_ctx_draw_rows(draw[b]), bit for bit
    -- an element in the next row of a straddling group takes that row's key AND that row's draw number"""
    dims, _, nm = natives('C263_T23')
    Tn, C = 23, dims['input_feats']
    assert (Tn * C) % 4 != 0
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, Tn, seed=98, lengths=[Tn, Tn - 7, Tn - 4])
    steps, draws = [5, 3, 2], [1, 4, 2]
    coefs = [d.step_coefs(i, mode, dims['scale'], 0.5 if mode == 'ddim' else 0.0) for i in steps]
    ctx = nm.context(B, Tn, max_steps=6)
    try:
        ctx.set_capacity_factor(0)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        ctx.set_row_seeds(SEEDS)
        fed = torch.stack([ctx.draw_rows(k)[b] for b, k in enumerate(draws)])[None].contiguous()
        same = torch.stack([ctx.draw_rows(1)[b] for b in range(B)])[None].contiguous()
        got = ctx.sample_rows(x_T.cuda().clone(), [steps], [coefs], draws=[draws]).clone()
        want = ctx.sample_rows(x_T.cuda().clone(), [steps], [coefs], noise=fed).clone()
        other = ctx.sample_rows(x_T.cuda().clone(), [steps], [coefs], noise=same).clone()
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(got[0], other[0]) and not torch.equal(got[1], other[1]) and not torch.equal(got[2], other[2])      # rows 1, 2 read draws 4, 2


# ---- 2. mixed steps against the reference model -----------------------------------------------------------
@pytest.mark.parametrize('cf', [1.5, 0], ids=['cf1.5_forced', 'cf0'])
def test_mixed_steps_meet_the_per_row_restatement(natives, monkeypatch, cf):
    """mc_denoise_rows at step_index (5, 0, 2) of ddim6 against rowstep_ref (the oracle's functions with ts as a vector): both decoded
    halves within the per-call bound.  At 1.5 the routing is teacher-forced to the device's expert ids and keep flags (a top-2 choice or
    a capacity cut may flip at a near tie), at 0 to its expert ids with nothing dropped."""
    dims, sd, nm = natives('C322_T24')
    d = _diffusion('ddim6')
    x, xf, mask = synth_inputs(dims, B, T, seed=93, lengths=LENGTHS)
    steps = [5, 0, 2]
    ctx = nm.context(B, T, max_steps=6)
    try:
        ctx.enable_capture()
        if cf == 0:
            ctx.set_capacity_factor(0)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        out2 = ctx.denoise_rows(x.cuda(), steps).cpu()
        forced = [ctx.routing(i) for i in range(dims['NL'])]
        uni = ctx.denoise(x.cuda(), 2).cpu()
    finally:
        ctx.close()
    assert not torch.equal(out2[0], uni[0]) and not torch.equal(out2[1], uni[1])      # rows 0, 1 sit at other steps than 2
    torch.set_num_threads(4)
    ts = [int(d.timestep_map[i]) for i in steps]
    ref = rowstep_ref.denoise_rows(sd, dims, x, ts, xf, mask, forced_routing=forced, capacity_factor=float(dims['E']) if cf == 0 else None,
                                   out2=True)
    err = float((out2 - ref).abs().max())
    wrong = float((uni - ref).abs().max())
    print(f'cf {cf}: |mc_denoise_rows - rowstep_ref| {err:.2e} (every row at step 2 instead: {wrong:.2e}); |out| {float(ref.abs().max()):.2f}')
    assert err <= TOL_CALL
    assert wrong > 10 * TOL_CALL                   # the bound tells the rows' timesteps apart


# ---- 3. / 4. / 6. the serving loop -----------------------------------------------------------------------
def _requests(seed, n, scales=None):
    from motioncraft_amd.serve import Request
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        xf = torch.nn.functional.layer_norm(torch.randn(SMALL['Nt'], SMALL['Dt'], generator=g), (SMALL['Dt'],))
        out.append(Request(length=(24, 17, 20, 9, 24)[i % 5], seed=seed * 100 + 7 * i, xf_out=xf, guidance_scale=None if scales is None else scales[i]))
    return out


def _with_scale(r, scale):
    from motioncraft_amd.serve import Request
    return Request(length=r.length, seed=r.seed, xf_out=r.xf_out, guidance_scale=scale)


def _serve(a, sampler, arrivals, steps=6):
    """arrivals: [(tick, Request)] in submission order -> ({index: result}, the batcher)"""
    from motioncraft_amd.serve import ContinuousBatcher
    bt = ContinuousBatcher(a, batch=B, frames=T, sampler=sampler, steps=steps)
    handles, out, k = {}, {}, 0
    while k < len(arrivals) or any(h is not None for h in bt.occupied) or bt._pending:
        while k < len(arrivals) and arrivals[k][0] <= bt.ticks:
            handles[bt.submit(arrivals[k][1])] = k
            k += 1
        if bt.tick() == 0:
            assert k < len(arrivals)
            bt.ticks = arrivals[k][0]              # (an idle batcher: the clock jumps to the next arrival)
        for h, v in bt.poll().items():
            out[handles[h]] = v.clone()
    torch.cuda.synchronize()
    return out, bt


def test_a_request_joining_mid_walk_gets_the_bits_of_its_own_batch(arch):
    """R walks ddim6 (eta 0.5: noise is drawn every step) in row 0 from tick 0 of a batch of its own; the same R admitted in row 2 at
    tick 3 of a batch whose other rows are mid-walk with other prompts, lengths, seeds and guidance scales: bit-equal.  Control: with
    another guidance scale on R the result differs."""
    from motioncraft_amd.serve import ContinuousBatcher
    sd, a = arch
    R = _requests(31, 1)[0]
    others = _requests(32, 2, scales=[1.25, 4.0])

    def serve(arrivals):
        bt = ContinuousBatcher(a, batch=B, frames=T, sampler='ddim', steps=6, eta=0.5)
        rows, out, k = {}, {}, 0
        for _ in range(40):
            while k < len(arrivals) and arrivals[k][0] <= bt.ticks:
                h = bt.submit(arrivals[k][1])
                k += 1
            bt.tick()
            rows.update({h_: b for b, h_ in enumerate(bt.occupied) if h_ is not None})
            out.update(bt.poll())
            if k == len(arrivals) and not any(h_ is not None for h_ in bt.occupied):
                break
        torch.cuda.synchronize()
        return out[h].clone(), rows[h], bt.submitted_at[h], bt.finished_at[h]          # of the LAST submitted request
    alone, row_a, t0_a, t1_a = serve([(0, R)])
    joined, row_j, t0_j, t1_j = serve([(0, others[0]), (0, others[1]), (3, R)])
    assert (row_a, t0_a, t1_a) == (0, 0, 6) and (row_j, t0_j, t1_j) == (2, 3, 9)
    assert bool(torch.isfinite(alone).all()) and tuple(alone.shape) == (R.length, SMALL['input_feats'])
    assert torch.equal(alone, joined), float((alone - joined).abs().max())
    other_scale, _, _, _ = serve([(0, others[0]), (0, others[1]), (3, _with_scale(R, 1.0))])
    assert float((other_scale - joined).abs().max()) > 1e-3


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp'])
def test_a_rows_guidance_scale_is_its_own(arch, sampler):
    """three requests with three guidance scales, the third joining at tick 2: each is bit-equal to the same request served in a batch
    where every row uses its scale.  With dpmpp (mode 2, the history per row) this fails if admitting the third request clears the
    running rows' history -- or does not clear the new row's."""
    sd, a = arch
    scales = [1.0, 2.5, 4.0]
    reqs = _requests(33, 3)
    mixed, bt = _serve(a, sampler, [(0, _with_scale(reqs[0], scales[0])), (0, _with_scale(reqs[1], scales[1])), (2, _with_scale(reqs[2], scales[2]))])
    assert sorted(mixed) == [0, 1, 2] and bt.finished_at[2] == 8
    for b, s in enumerate(scales):
        same, _ = _serve(a, sampler, [(0 if i < 2 else 2, _with_scale(r, s)) for i, r in enumerate(reqs)])
        assert bool(torch.isfinite(same[b]).all())
        assert torch.equal(mixed[b], same[b]), (sampler, b, float((mixed[b] - same[b]).abs().max()))
        for o in range(3):
            if o != b:
                assert not torch.equal(mixed[o], same[o]), (sampler, b, o)


def test_continuous_and_request_batcher_agree_and_meet_the_oracle_alone(arch, monkeypatch):
    """five requests through B = 3, 6-step DDIM, in two arrival patterns: ContinuousBatcher == RequestBatcher bit for bit, and every
    request within the per-trajectory bound of the oracle's B = 1 walk on the same draws without drops"""
    from motioncraft_amd.serve import RequestBatcher
    from oracle import philox_oracle as P
    from oracle import stmogen_oracle as O
    sd, a = arch
    C = SMALL['input_feats']
    reqs = _requests(34, 5)
    rb = RequestBatcher(a, batch=B, frames=T, sampler='ddim', steps=6)
    handles = [rb.submit(r) for r in reqs]
    want = rb.run()
    torch.cuda.synchronize()
    for pattern in ([0, 0, 0, 0, 0], [0, 1, 1, 4, 11]):
        got, bt = _serve(a, 'ddim', list(zip(pattern, reqs)))
        assert sorted(got) == list(range(5))
        for i, r in enumerate(reqs):
            assert tuple(got[i].shape) == (r.length, C)
            assert torch.equal(got[i], want[handles[i]]), (pattern, i, float((got[i] - want[handles[i]]).abs().max()))
    monkeypatch.setattr(O, 'CAPACITY_FACTOR', float(SMALL['E']))
    torch.set_num_threads(4)
    sched = O.Schedule(1000, 'ddim6')
    for i, r in enumerate(reqs):
        mask = torch.zeros(1, T)
        mask[0, :r.length] = 1
        x_T = torch.from_numpy(P.draw_normal(T * C, r.seed, 0)).view(1, T, C)
        ref = O.sample_loop(sd, SMALL, sched, 'ddim', x_T, r.xf_out[None], mask, step_noise=lambda i_: torch.zeros(1, T, C))
        err = float((got[i].cpu() - ref[0, :r.length]).abs().max())
        print(f'request {i}: |continuous batcher - oracle alone| {err:.2e}; |x| {float(ref.abs().max()):.2f}')
        assert err <= TOL_TRAJ, (i, err)


# ---- 5. op level -------------------------------------------------------------------------------------------
def _row_coefs(scales_t):
    from motioncraft_amd import lib as L_
    arr = (L_.StepCoefs * len(scales_t))()
    for c, (wc, wu) in zip(arr, scales_t):
        c.mode, c.text_coef, c.none_coef = 1, wc, wu
    return arr


@pytest.mark.parametrize('M,Tn', [(72, 24), (69, 23)])
@pytest.mark.parametrize('variant', [1, 2, 3], ids=['column_tiles', 'block_ranges', 'pair_grouped'])
def test_per_row_tail_forms_vs_fp64(variant, M, Tn):
    """mc_op_gemm_tail_rows: C[r] = (wc_r h[r] + wu_r h[r + M]) W0^T + (wc_r a[r] + wu_r a[r + M]) W1^T + b0 + b1 with (wc_r, wu_r) of
    request row r / T, against fp64 within the bound tests/test_gpu_parity.py holds mc_op_gemm_tail to (1e-4); T divides neither tile
    height (64, 16), so row tiles span two request rows; nothing is stored past the last row"""
    lib, ptr, stream = _lib()
    N, K = (322, 384) if Tn == 24 else (263, 256)
    g = torch.Generator(device='cuda').manual_seed(M)
    h = torch.randn(2 * M, K, device='cuda', generator=g)
    a = torch.randn(2 * M, K, device='cuda', generator=g)
    w = torch.randn(2, N, K, device='cuda', generator=g) / K ** 0.5
    b = torch.randn(2, N, device='cuda', generator=g)
    wts = [(3.25, -2.25), (1.0, 0.0), (-0.5, 1.5)]
    coefs = _row_coefs(wts)
    wc = torch.tensor([wts[r // Tn][0] for r in range(M)], device='cuda', dtype=torch.float64)[:, None]
    wu = torch.tensor([wts[r // Tn][1] for r in range(M)], device='cuda', dtype=torch.float64)[:, None]
    ref = ((wc * h[:M].double() + wu * h[M:].double()) @ w[0].double().t() + (wc * a[:M].double() + wu * a[M:].double()) @ w[1].double().t()
           + b[0].double() + b[1].double())
    c = torch.full((M + 2, N), 777.0, device='cuda')
    c2 = torch.full((M + 2, N), 777.0, device='cuda')
    rc = lib.mc_op_gemm_tail_rows(ptr(h), ptr(a), ptr(w), ptr(b), ptr(c), ptr(c2), M, N, K, coefs, Tn, variant, stream())
    assert rc == 0, lib.mc_last_error()
    torch.cuda.synchronize()
    assert bool((c[M:] == 777.0).all()) and bool((c2[M:] == 777.0).all())
    err = float((c[:M].double() - ref).abs().max())
    uniform = ((wts[0][0] * h[:M].double() + wts[0][1] * h[M:].double()) @ w[0].double().t()
               + (wts[0][0] * a[:M].double() + wts[0][1] * a[M:].double()) @ w[1].double().t() + b[0].double() + b[1].double())
    print(f'variant {variant} M={M} T={Tn}: |C - fp64| {err:.2e}')
    assert err <= 1e-4
    assert float((c[:M].double() - uniform).abs().max()) > 0.1                       # rows 1, 2 really took their own weights
    # uniform weights: the per-row kernel gives the bits of the uniform one (variants 1, 2: the same kernel form)
    if variant != 3:
        cu, cu2 = torch.empty(M, N, device='cuda'), torch.empty(M, N, device='cuda')
        cr, cr2 = torch.empty(M, N, device='cuda'), torch.empty(M, N, device='cuda')
        assert lib.mc_op_gemm_tail(ptr(h), ptr(a), ptr(w), ptr(b), ptr(cu), ptr(cu2), M, N, K, 3.25, -2.25, variant, stream()) == 0
        assert lib.mc_op_gemm_tail_rows(ptr(h), ptr(a), ptr(w), ptr(b), ptr(cr), ptr(cr2), M, N, K, _row_coefs([wts[0]] * 3), Tn, variant, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(cu, cr)


@pytest.mark.parametrize('form', ['vector', 'element'])
@pytest.mark.parametrize('mode', ['ddpm', 'ddim', 'dpmpp'])
def test_per_row_sampler_kernels_vs_fp64(mode, form):
    """mc_op_sampler_rows at C = 263, T = 23, B = 3 (T C = 6049: flat groups of four straddle both row boundaries) with three different
    entries, against the fp64 per-element restatement; the four elements at every row boundary are checked by name.  'element': operands
    off 16-byte alignment take the element form of the kernel.  Mode 2: row 0 has eta = 0 and must not read its (NaN) history."""
    lib, ptr, stream = _lib()
    Bn, TC = 3, 23 * 263
    n = Bn * TC
    d = _diffusion('ddim6')
    if mode == 'dpmpp':
        walk = d.multistep_coefs(list(range(6))[::-1], 2.5, 2)
        rows = [walk[0], walk[2], walk[3]]
        assert rows[0].eta == 0 and rows[1].eta != 0 and rows[2].eta != 0
    else:
        rows = [d.step_coefs(i, mode, 2.5, 0.5 if mode == 'ddim' else 0.0) for i in (5, 0, 2)]
    coefs = (type(rows[0]) * Bn)(*rows)
    off = 0 if form == 'vector' else 1
    g = torch.Generator(device='cuda').manual_seed(7)
    bufs = [torch.randn(n + 8, device='cuda', generator=g) for _ in range(5)]
    x, ot, on, nz, hist = (t[off:off + n] for t in bufs)
    if mode == 'dpmpp':
        hist[:TC] = float('nan')
    want, want0 = rowstep_ref.sampler_rows(x.cpu().numpy(), ot.cpu().numpy(), on.cpu().numpy(), nz.cpu().numpy(), hist.cpu().numpy(), rows, TC)
    outb, x0b = torch.full((n + 8,), 777.0, device='cuda'), torch.full((n + 8,), 777.0, device='cuda')
    out, x0 = outb[off:off + n], x0b[off:off + n]
    rc = lib.mc_op_sampler_rows(x.data_ptr(), ot.data_ptr(), on.data_ptr(), None if mode == 'dpmpp' else nz.data_ptr(),
                                hist.data_ptr() if mode == 'dpmpp' else None, out.data_ptr(), x0.data_ptr(), Bn, TC, coefs, stream())
    assert rc == 0, lib.mc_last_error()
    torch.cuda.synchronize()
    assert bool((outb[:off] == 777.0).all()) and bool((outb[off + n:] == 777.0).all()) and bool((x0b[off + n:] == 777.0).all())
    got, got0 = out.cpu().numpy().astype(np.float64), x0.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    tol = 2e-5 * max(1.0, float(np.abs(want).max()))          # fp32 round-off of five fused operations on values up to |want| max
    assert np.abs(got0 - want0).max() <= 1e-6 and np.abs(got - want).max() <= tol, (np.abs(got - want).max(), tol)
    for edge in (TC, 2 * TC):                                 # the last two elements of a row and the first two of the next
        for e in (edge - 2, edge - 1, edge, edge + 1):
            assert abs(got[e] - want[e]) <= tol, (mode, form, e, got[e], want[e])
            other = rowstep_ref.sampler_rows(x[e:e + 1].cpu().numpy(), ot[e:e + 1].cpu().numpy(), on[e:e + 1].cpu().numpy(), nz[e:e + 1].cpu().numpy(),
                                             hist[e:e + 1].cpu().numpy(), [rows[(e // TC + 1) % Bn]], 1)[0][0]
            if np.isfinite(other):
                assert abs(got[e] - other) > 10 * tol, (mode, form, e, 'took a neighbouring row\'s coefficients')
    if mode == 'dpmpp':
        assert torch.equal(hist, x0)                          # the history now holds this step's x0, row 0's NaNs gone


# ---- 7. state rules ------------------------------------------------------------------------------------------
def test_rows_mode_refusals_leave_the_context_as_it_was(natives):
    """graph held / capturing stream / seam table -> MC_ERR_STATE (3); an index outside the schedule, mixed modes, too many ticks ->
    MC_ERR_ARG (1); noise_dev == NULL without a seed table -> 3, with one but without draw numbers -> 1; mode 2 with eta != 0 on a row
    without history -> 3.  After all of them a plain mc_sample_step gives the bits it gave before."""
    dims, _, nm = natives('C322_T24')
    lib, ptr, stream = _lib()
    C = dims['input_feats']
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, T, seed=95, lengths=LENGTHS)
    noise = torch.randn(B, T, C, generator=torch.Generator().manual_seed(96)).cuda()
    c5 = d.step_coefs(5, 'ddim', dims['scale'], 0.5)
    ms = d.multistep_coefs([5, 4, 3, 2, 1, 0], dims['scale'], 2)
    ctx = nm.context(B, T, max_steps=6)
    try:
        ctx.set_capacity_factor(0)                            # (the last check compares a row across batchmates at other steps)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        before = ctx.sample_step(x_T.cuda(), 5, c5, noise).clone()
        x = x_T.cuda().clone()

        def code(fn):
            with pytest.raises(RuntimeError) as e:
                fn()
            torch.cuda.synchronize()
            assert torch.equal(x, x_T.cuda())                 # nothing ran
            return str(e.value)
        rows = lambda idx, c, **kw: ctx.sample_rows(x, [idx], [c], **kw)
        assert '(code 1)' in code(lambda: rows([5, 6, 0], [c5] * B, noise=noise[None]))
        assert '(code 1)' in code(lambda: rows([5, -1, 0], [c5] * B, noise=noise[None]))
        assert '(code 1)' in code(lambda: ctx.denoise_rows(x, [5, 6, 0]))
        assert '(code 1)' in code(lambda: rows([5, 5, 5], [c5, d.step_coefs(5, 'ddpm', dims['scale']), c5], noise=noise[None]))
        assert '(code 1)' in code(lambda: ctx.sample_rows(x, [[5] * B] * 7, [[c5] * B] * 7, noise=noise[None].repeat(7, 1, 1, 1)))
        assert '(code 3)' in code(lambda: rows([5] * B, [c5] * B))                                   # no noise, no seed table
        ctx.set_row_seeds(SEEDS)
        assert '(code 1)' in code(lambda: rows([5] * B, [c5] * B))                                   # ... no draw numbers
        ctx.clear_row_seeds()
        assert '(code 3)' in code(lambda: rows([4] * B, [ms[0], ms[1], ms[0]]))                      # row 1: eta != 0 without history
        ctx.set_seams([0, T - 4, 2 * (T - 4)], 4)
        assert '(code 3)' in code(lambda: rows([5] * B, [c5] * B, noise=noise[None]))
        assert '(code 3)' in code(lambda: ctx.denoise_rows(x, [5, 0, 2]))
        ctx.clear_seams()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            gx, gn = x_T.cuda().clone(), noise.clone()
            ctx.graph_capture(gx, gn, [d.step_coefs(i, 'ddim', dims['scale'], 0.5) for i in range(6)])
            assert '(code 3)' in code(lambda: rows([5] * B, [c5] * B, noise=noise[None]))
            ctx.graph_release()
        side.synchronize()
        # a capturing stream: refused before anything is enqueued into the capture
        hip = ctypes.CDLL('libamdhip64.so')
        hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
        hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
        with torch.cuda.stream(side):
            assert hip.hipStreamBeginCapture(ctypes.c_void_p(side.cuda_stream), 2) == 0          # (relaxed mode)
            try:
                with pytest.raises(RuntimeError, match=r'\(code 3\).*capturing'):
                    rows([5] * B, [c5] * B, noise=noise[None])
                with pytest.raises(RuntimeError, match=r'\(code 3\).*capturing'):
                    ctx.denoise_rows(x, [5, 0, 2])
            finally:
                graph = ctypes.c_void_p()
                rc = hip.hipStreamEndCapture(ctypes.c_void_p(side.cuda_stream), ctypes.byref(graph))
                if graph.value:
                    hip.hipGraphDestroy(graph)
            assert rc == 0
        side.synchronize()
        assert torch.equal(x, x_T.cuda())
        after = ctx.sample_step(x_T.cuda(), 5, c5, noise).clone()
        torch.cuda.synchronize()
        assert torch.equal(before, after)
        # and the mode still works on this context: one tick, rows at three steps, equal to itself and finite
        got = ctx.sample_rows(x, [[5, 0, 2]], [[d.step_coefs(i, 'ddim', dims['scale'], 0.5) for i in (5, 0, 2)]], noise=noise[None]).clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got).all()) and torch.equal(got[0], before[0]) and not torch.equal(got[1], before[1])
    finally:
        ctx.close()


def test_condition_rows_keeps_the_history_of_running_rows(natives):
    """mode 2: after a tick every row has history; mc_ctx_set_condition_rows with row 1 fresh clears row 1's flag alone -- eta != 0 on
    row 1 is MC_ERR_STATE, on rows 0 and 2 it runs; mc_ctx_set_condition clears all three"""
    dims, _, nm = natives('C322_T24')
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, T, seed=97, lengths=LENGTHS)
    ms = d.multistep_coefs([5, 4, 3, 2, 1, 0], dims['scale'], 2)
    ctx = nm.context(B, T, max_steps=6)
    try:
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        x = x_T.cuda().clone()
        ctx.sample_rows(x, [[5, 5, 5]], [[ms[0]] * B])
        ctx.set_condition_rows(xf.cuda(), mask.cuda(), [False, True, False])
        with pytest.raises(RuntimeError, match=r'\(code 3\).*row 1'):
            ctx.sample_rows(x, [[4, 4, 4]], [[ms[1]] * B])
        ctx.sample_rows(x, [[4, 5, 4]], [[ms[1], ms[0], ms[1]]])
        ctx.sample_rows(x, [[3, 4, 3]], [[ms[2], ms[1], ms[2]]])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(x).all())
        ctx.set_condition(xf.cuda(), mask.cuda())
        with pytest.raises(RuntimeError, match=r'\(code 3\).*row 0'):
            ctx.sample_rows(x, [[2, 3, 2]], [[ms[3], ms[2], ms[3]]])
    finally:
        ctx.close()


# ---- control requests ------------------------------------------------------------------------------------------
def test_successive_control_batches_get_their_own_control_condition():
    """four requests with control conditions of one shape and different contents through B = 3: two control batches one after the
    other.  ContinuousBatcher == RequestBatcher bit for bit, and the request of the second batch depends on ITS control rows (a batcher
    that kept the first batch's control features in the context would fail both)"""
    import motioncraft_amd as mc
    from motioncraft_amd.serve import ContinuousBatcher, Request, RequestBatcher
    from oracle import weights as W
    sd = W.make_state_dict(CTRL, SMALL_SEED, shapes=W.control_param_shapes(CTRL, CTRL_COPY, CTRL_FEATS))
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_small.py'))
    cfg.model.model.num_layers = 3
    cfg.model.diffusion_test = dict(BASE, respace='ddim10')
    cfg.merge_from_dict({'condition_encode_cfg': dict(dataset_name='nothing', condition_pre_encode=False, condition_pre_encode_type='nothing',
                                                      control_cond_feats=CTRL_FEATS, condition_latent_dim=CTRL['L'] * CTRL['H'],
                                                      condition_cfg=True)})
    a = mc.build_architecture(cfg.model)
    a.model = mc.ControlT2MHalf(a.model, copy_blocks_num=CTRL_COPY, control_cond_feats=CTRL_FEATS, cfg=cfg)
    a.load_state_dict({'model.' + k: v for k, v in sd.items()})
    try:
        g = torch.Generator().manual_seed(41)

        def make(i, c=None):
            xf = torch.nn.functional.layer_norm(torch.randn(CTRL['Nt'], CTRL['Dt'], generator=torch.Generator().manual_seed(410 + i)), (CTRL['Dt'],))
            return Request(length=(24, 17, 20, 22)[i], seed=4100 + i, xf_out=xf, c=c)
        cs = [torch.randn(CTRL_TC, CTRL_FEATS, generator=g) for _ in range(5)]
        reqs = [make(i, cs[i]) for i in range(4)]

        def run(cls, rs):
            bt = cls(a, batch=B, frames=T, sampler='ddim', steps=4)
            hs = [bt.submit(r) for r in rs]
            out = bt.run()
            torch.cuda.synchronize()
            return [out[h].clone() for h in hs]
        want = run(RequestBatcher, reqs)
        got = run(ContinuousBatcher, reqs)
        for i in range(4):
            assert bool(torch.isfinite(got[i]).all())
            assert torch.equal(got[i], want[i]), (i, float((got[i] - want[i]).abs().max()))
        moved = run(ContinuousBatcher, reqs[:3] + [make(3, cs[4])])
        assert torch.equal(moved[0], got[0]) and not torch.equal(moved[3], got[3])
    finally:
        a.model.release()

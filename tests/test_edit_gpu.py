"""GPU (MI355X): edited rows -- ``mc_ctx_set_edit_rows`` / ``mc_op_sampler_edit_rows``, the two edit kernels behind them and
``serve.Edit`` through both batchers.

Shapes are those of tests/test_rowsteps_gpu.py: the reduced config at B = 3, T = 24, C = 322, lengths (24, 17, 20), and C = 263 at T = 23,
where flat groups of four straddle both row boundaries.  Device against device is exact (torch.equal); the fp64 comparisons use the
bounds of ``test_per_row_sampler_kernels_vs_fp64``."""
import faulthandler
import os

import numpy as np
import pytest
import torch

import edit_ref
from helpers import HML_SMALL, SMALL, SMALL_SEED, synth_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B, T = 3, 24
LENGTHS = (24, 17, 20)
SEEDS = [11, 2 ** 63 + 5, 11 + 2 ** 32]
BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
SHAPES = {'C322_T24': (SMALL, 24), 'C263_T23': (HML_SMALL, 23)}
MODES = ('ddpm', 'ddim', 'dpmpp')
FLIP = edit_ref.DRAW_FLIP


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
    from motioncraft_amd.engine import NativeModel
    from oracle import weights as W
    made = {}

    def get(name):
        if name not in made:
            dims, _ = SHAPES[name]
            made[name] = (dims, NativeModel(dims, W.make_state_dict(dims, SMALL_SEED), cfg_scale=dims['scale']))
        return made[name]
    yield get
    for _, nm in made.values():
        nm.close()


def _walk_coefs(d, dims, mode):
    idx = list(range(d.num_timesteps))[::-1]
    if mode == 'dpmpp':
        return idx, d.multistep_coefs(idx, dims['scale'], 2)
    return idx, [d.step_coefs(i, mode, dims['scale'], 0.5 if mode == 'ddim' else 0.0) for i in idx]


def _three_rows(d, mode):
    if mode == 'dpmpp':
        walk = d.multistep_coefs(list(range(6))[::-1], 2.5, 2)
        rows = [walk[0], walk[2], walk[3]]
        assert rows[0].eta == 0 and rows[1].eta != 0 and rows[2].eta != 0
        return rows
    return [d.step_coefs(i, mode, 2.5, 0.5 if mode == 'ddim' else 0.0) for i in (5, 0, 2)]


def _keep_mask(Bn, TC, seed):
    """the last two elements of every row kept, the first two of the next free, a seeded 30 % elsewhere"""
    keep = torch.rand(Bn * TC, generator=torch.Generator().manual_seed(seed)) < 0.3
    for edge in range(TC, Bn * TC + 1, TC):
        keep[edge - 2:edge] = True
        if edge < Bn * TC:
            keep[edge:edge + 2] = False
    return keep


# ---- 1. the kernels against fp64 ------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['vector', 'element'])
@pytest.mark.parametrize('mode', MODES)
def test_edit_kernels_vs_fp64(mode, form):
    """mc_op_sampler_edit_rows at C = 263, T = 23, B = 3 with three different entries against edit_ref ('element': every float operand
    off 16-byte and the keep bytes off 4-byte alignment); gt is NaN wherever keep == 0 and
    the history of the eta == 0 row is NaN: neither may reach an output.  x0 == gt bit for bit on kept elements, hist == x0 after mode 2,
    sentinels around every output, the row boundaries by name."""
    lib, ptr, stream = _lib()
    Bn, TC = 3, 23 * 263
    n = Bn * TC
    d = _diffusion('ddim6')
    rows = _three_rows(d, mode)
    coefs = (type(rows[0]) * Bn)(*rows)
    off = 0 if form == 'vector' else 1
    g = torch.Generator(device='cuda').manual_seed(17)
    bufs = [torch.randn(n + 8, device='cuda', generator=g) for _ in range(7)]
    x, ot, on, nz, hist, gt, z2 = (t[off:off + n] for t in bufs)
    keepb = torch.zeros(n + 8, dtype=torch.bool, device='cuda')
    keep = keepb[off:off + n]                                 # 'element': the keep bytes off 4-byte alignment too (byte-wise keep reads)
    keep[:] = _keep_mask(Bn, TC, 18).cuda()
    assert keep.data_ptr() % 4 == off
    gt_clean = gt.clone()
    gt[~keep] = float('nan')
    if mode == 'dpmpp':
        hist[:TC] = float('nan')
    want, want0 = edit_ref.edit_rows(x.cpu().numpy(), ot.cpu().numpy(), on.cpu().numpy(), nz.cpu().numpy(), hist.cpu().numpy(),
                                     gt.cpu().numpy(), keep.cpu().numpy(), z2.cpu().numpy(), rows, TC)
    outb, x0b = torch.full((n + 8,), 777.0, device='cuda'), torch.full((n + 8,), 777.0, device='cuda')
    out, x0 = outb[off:off + n], x0b[off:off + n]
    ms = mode == 'dpmpp'
    rc = lib.mc_op_sampler_edit_rows(x.data_ptr(), ot.data_ptr(), on.data_ptr(), None if ms else nz.data_ptr(),
                                     z2.data_ptr() if mode == 'ddim' else None, gt.data_ptr(), keep.data_ptr(), None, None,
                                     hist.data_ptr() if ms else None, out.data_ptr(), x0.data_ptr(), Bn, TC, coefs, stream())
    assert rc == 0, lib.mc_last_error()
    torch.cuda.synchronize()
    for buf in (outb, x0b):
        assert bool((buf[:off] == 777.0).all()) and bool((buf[off + n:] == 777.0).all())
    got, got0 = out.cpu().numpy().astype(np.float64), x0.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(got0).all()
    tol = 2e-5 * max(1.0, float(np.abs(want).max()))          # fp32 round-off of five fused operations on values up to |want| max
    print(f'{mode} {form}: |x_prev - fp64| {np.abs(got - want).max():.2e} (tol {tol:.2e}), |x0 - fp64| {np.abs(got0 - want0).max():.2e}')
    assert np.abs(got0 - want0).max() <= 1e-6 and np.abs(got - want).max() <= tol, (np.abs(got - want).max(), tol)
    assert torch.equal(x0[keep], gt_clean[keep])
    free = (~keep).cpu().numpy()
    assert np.abs(got0 - (ot + on).double().cpu().numpy())[free].max() <= 1e-6
    knp = keep.cpu().numpy()
    for edge in (TC, 2 * TC):                                 # the last two elements of a row (kept) and the first two of the next (free)
        for e in (edge - 2, edge - 1, edge, edge + 1):
            assert abs(got[e] - want[e]) <= tol, (mode, form, e, got[e], want[e])
            sl = slice(e, e + 1)
            other = edit_ref.edit_rows(x[sl].cpu().numpy(), ot[sl].cpu().numpy(), on[sl].cpu().numpy(), nz[sl].cpu().numpy(), hist[sl].cpu().numpy(),
                                       gt[sl].cpu().numpy(), knp[sl], z2[sl].cpu().numpy(), [rows[(e // TC + 1) % Bn]], 1)[0][0]
            if np.isfinite(other) and abs(other - want[e]) > 20 * tol:
                assert abs(got[e] - other) > 10 * tol, (mode, form, e, 'took a neighbouring row\'s coefficients')
    if ms:
        assert torch.equal(hist, x0)                          # the history holds the EDITED x0, row 0's NaNs gone


@pytest.mark.parametrize('mode', MODES)
def test_op_refuses_mixed_modes_and_mixed_noise_sources(mode):
    lib, ptr, stream = _lib()
    d = _diffusion('ddim6')
    rows = _three_rows(d, mode)
    other = d.step_coefs(5, 'ddpm' if mode != 'ddpm' else 'ddim', 2.5, 0.0)
    t = torch.zeros(3 * 8, device='cuda')
    keep = torch.zeros(3 * 8, dtype=torch.uint8, device='cuda')
    out = torch.full((3 * 8,), 5.0, device='cuda')
    seeds = (__import__('ctypes').c_uint64 * 3)(1, 2, 3)

    def call(coefs, noise, gtn, sd, hist):
        arr = (type(coefs[0]) * 3)(*coefs)
        return lib.mc_op_sampler_edit_rows(t.data_ptr(), t.data_ptr(), t.data_ptr(), noise, gtn, t.data_ptr(), keep.data_ptr(), sd, sd, hist,
                                           out.data_ptr(), None, 3, 8, arr, stream())
    hist = torch.zeros(3 * 8, device='cuda')
    h = hist.data_ptr() if mode == 'dpmpp' else None
    nz = None if mode == 'dpmpp' else t.data_ptr()
    assert call([rows[0], other, rows[2]], nz, nz, None, h) == 1
    if mode == 'dpmpp':
        assert call(rows, t.data_ptr(), None, None, h) == 1 and call(rows, None, None, seeds, h) == 1 and call(rows, None, None, None, None) == 1
    else:
        assert call(rows, t.data_ptr(), t.data_ptr(), seeds, None) == 1          # both noise sources
        assert call(rows, None, None, None, None) == 1                            # none
    if mode == 'ddim':
        assert call(rows, t.data_ptr(), None, None, None) == 1                    # a noise tensor without the kept region's
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


# ---- 2. keep all zero: the row kernels' bits ----------------------------------------------------------------
@pytest.mark.parametrize('form', ['vector', 'element'])
@pytest.mark.parametrize('mode', MODES)
def test_zero_keep_gives_the_row_kernels_bits(mode, form):
    lib, ptr, stream = _lib()
    Bn, TC = 3, 23 * 263
    n = Bn * TC
    d = _diffusion('ddim6')
    rows = _three_rows(d, mode)
    coefs = (type(rows[0]) * Bn)(*rows)
    off = 0 if form == 'vector' else 1
    g = torch.Generator(device='cuda').manual_seed(27)
    bufs = [torch.randn(n + 8, device='cuda', generator=g) for _ in range(5)]
    x, ot, on, nz, hist = (t[off:off + n] for t in bufs)
    ms = mode == 'dpmpp'
    if ms:
        hist[:TC] = float('nan')
    gt = torch.full((n + 8,), float('nan'), device='cuda')[off:off + n]
    keep = torch.zeros(n + 8, dtype=torch.uint8, device='cuda')[off:off + n]
    ha, hb = hist.clone(), hist.clone()
    (xa, x0a), (xb, x0b) = ((torch.empty(n + 8, device='cuda')[off:off + n] for _ in range(2)) for _ in range(2))
    assert lib.mc_op_sampler_rows(x.data_ptr(), ot.data_ptr(), on.data_ptr(), None if ms else nz.data_ptr(), ha.data_ptr() if ms else None,
                                  xa.data_ptr(), x0a.data_ptr(), Bn, TC, coefs, stream()) == 0, lib.mc_last_error()
    assert lib.mc_op_sampler_edit_rows(x.data_ptr(), ot.data_ptr(), on.data_ptr(), None if ms else nz.data_ptr(),
                                       nz.data_ptr() if mode == 'ddim' else None, gt.data_ptr(), keep.data_ptr(), None, None,
                                       hb.data_ptr() if ms else None, xb.data_ptr(), x0b.data_ptr(), Bn, TC, coefs, stream()) == 0, lib.mc_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xa).all())
    assert torch.equal(xa, xb) and torch.equal(x0a, x0b)
    if ms:
        assert torch.equal(ha, hb)


def _ctx(nm, Tn, d, xf, mask, cf=0):
    ctx = nm.context(B, Tn, max_steps=d.num_timesteps)
    ctx.set_capacity_factor(cf)
    ctx.set_timesteps(d.timestep_map)
    ctx.set_condition(xf.cuda(), mask.cuda())
    ctx.set_row_seeds(SEEDS)
    return ctx


def _walk(ctx, x, idx, coefs, mode, one_call=True):
    n = len(idx)
    draws = [[1 + k] * B for k in range(n)]
    x0 = torch.empty_like(x)
    if one_call:
        ctx.sample_rows(x, [[i] * B for i in idx], [[c] * B for c in coefs], draws=None if mode == 'dpmpp' else draws, x0=x0)
    else:
        for k in range(n):
            ctx.sample_rows(x, [[idx[k]] * B], [[coefs[k]] * B], draws=None if mode == 'dpmpp' else [draws[k]], x0=x0)
    return x, x0


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('mode', MODES)
def test_zero_table_through_a_context_changes_no_bit(natives, mode, shape):
    """six ticks with a table whose keep bytes are all zero (gt all NaN) == six ticks with no table, device-drawn noise"""
    dims, nm = natives(shape)
    Tn, C = SHAPES[shape][1], dims['input_feats']
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, Tn, seed=191, lengths=[Tn, Tn - 7, Tn - 4])
    idx, coefs = _walk_coefs(d, dims, mode)
    ctx = _ctx(nm, Tn, d, xf, mask)
    try:
        xa, x0a = _walk(ctx, x_T.cuda().clone(), idx, coefs, mode)
        ctx.set_condition(xf.cuda(), mask.cuda())
        ctx.set_edit_rows(torch.full((B, Tn, C), float('nan'), device='cuda'), torch.zeros(B, Tn, C, dtype=torch.bool, device='cuda'))
        xb, x0b = _walk(ctx, x_T.cuda().clone(), idx, coefs, mode)
        torch.cuda.synchronize()
        ctx.check()
    finally:
        ctx.close()
    assert bool(torch.isfinite(xa).all()) and not torch.equal(xa, x_T.cuda())
    assert torch.equal(xa, xb) and torch.equal(x0a, x0b)


# ---- 3. the kept region's draw ----------------------------------------------------------------------------------
def test_kept_region_noise_is_the_flipped_draw_of_the_rows_seed():
    """mode 1, both noises drawn in the kernel: a kept element of x_prev is sqrt(ab_prev) g + sqrt(1 - ab_prev) z with z element r of
    mc_op_philox_normal(TC, seed_b, draw_b ^ 2^63) -- and not of draw_b itself; the row boundaries at C = 263 (kept by _keep_mask) included"""
    import ctypes
    lib, ptr, stream = _lib()
    Bn, TC = 3, 23 * 263
    n = Bn * TC
    d = _diffusion('ddim6')
    rows = [d.step_coefs(i, 'ddim', 2.5, 0.5) for i in (5, 3, 2)]
    coefs = (type(rows[0]) * Bn)(*rows)
    draws = [1, 4, 2 ** 63 + 2]
    g = torch.Generator(device='cuda').manual_seed(37)
    x, ot, on, gt = (torch.randn(n, device='cuda', generator=g) for _ in range(4))
    keep = _keep_mask(Bn, TC, 38).cuda()
    out = torch.empty(n, device='cuda')
    rc = lib.mc_op_sampler_edit_rows(x.data_ptr(), ot.data_ptr(), on.data_ptr(), None, None, gt.data_ptr(), keep.data_ptr(),
                                     (ctypes.c_uint64 * Bn)(*SEEDS), (ctypes.c_uint64 * Bn)(*draws), None, out.data_ptr(), None, Bn, TC, coefs, stream())
    assert rc == 0, lib.mc_last_error()

    def normals(flip):
        z = torch.empty(Bn, TC, device='cuda')
        for b in range(Bn):
            assert lib.mc_op_philox_normal(z[b].data_ptr(), None, TC, SEEDS[b], draws[b] ^ flip, stream()) == 0
        return z.view(-1).double().cpu().numpy()
    z2, z1 = normals(FLIP), normals(0)
    torch.cuda.synchronize()
    got, knp, gnp = out.double().cpu().numpy(), keep.cpu().numpy(), gt.double().cpu().numpy()
    abp = np.repeat([float(r.ab_prev) for r in rows], TC)
    want = np.sqrt(abp) * gnp + np.sqrt(1 - abp) * z2
    miss = np.sqrt(abp) * gnp + np.sqrt(1 - abp) * z1
    tol = 2e-5 * max(1.0, float(np.abs(want).max()))
    print(f'kept-region draw: |x_prev - formula| {np.abs(got - want)[knp].max():.2e} (tol {tol:.2e})')
    assert np.abs(got - want)[knp].max() <= tol
    far = np.abs(want - miss) > 20 * tol                      # (two normals closer than that cannot tell the draws apart)
    assert far[knp].mean() > 0.99 and (np.abs(got - miss) > 10 * tol)[knp & far].all()
    for edge in (TC, 2 * TC, 3 * TC):
        assert knp[edge - 2] and knp[edge - 1] and abs(got[edge - 1] - want[edge - 1]) <= tol and abs(got[edge - 2] - want[edge - 2]) <= tol
    # the free elements are the row kernel's under the step draw: the same call with nothing kept
    free = torch.empty(n, device='cuda')
    rc = lib.mc_op_sampler_edit_rows(x.data_ptr(), ot.data_ptr(), on.data_ptr(), None, None, gt.data_ptr(), torch.zeros_like(keep).data_ptr(),
                                     (ctypes.c_uint64 * Bn)(*SEEDS), (ctypes.c_uint64 * Bn)(*draws), None, free.data_ptr(), None, Bn, TC, coefs, stream())
    assert rc == 0, lib.mc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out[~keep], free[~keep]) and not torch.equal(out[keep], free[keep])


# ---- 4 / 6. walks through a context: the end of a walk, one call against single ticks ----------------------------------
def _edit_tables(dims, Tn, seed):
    """frames {0, 1, 11, Tn - 1} on all channels plus a block of channels on frames 4-8, in every row; gt seeded, NaN where free"""
    C = dims['input_feats']
    keep = torch.zeros(B, Tn, C, dtype=torch.bool)
    keep[:, [0, 1, 11, Tn - 1]] = True
    keep[:, 4:9, 3:C // 3] = True
    keep[1] = keep[1].roll(5, dims=1)                          # (rows differ)
    gt = torch.randn(B, Tn, C, generator=torch.Generator().manual_seed(seed))
    return gt, keep


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('mode', MODES)
def test_end_of_walk_kept_region_is_gt_bit_for_bit(natives, mode, shape):
    """a whole ddim6 walk under an edit table: the kept region of the final x equals gt bit for bit in all three samplers (schedule
    index 0: c1 = 1, c2 = 0, nonzero = 0, ab_prev = 1, multistep (0, 1, 0)); the free region is finite and differs from the walk
    without the table; six ticks in one call == six single-tick calls; row 2 with nothing kept has the bits of the walk without a table"""
    dims, nm = natives(shape)
    Tn, C = SHAPES[shape][1], dims['input_feats']
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, Tn, seed=291, lengths=[Tn, Tn - 7, Tn - 4])
    idx, coefs = _walk_coefs(d, dims, mode)
    gt, keep = _edit_tables(dims, Tn, 292)
    keep[2] = False
    gtd = gt.clone()
    gtd[~keep] = float('nan')
    ctx = _ctx(nm, Tn, d, xf, mask)
    try:
        plain, _ = _walk(ctx, x_T.cuda().clone(), idx, coefs, mode)
        ctx.set_condition(xf.cuda(), mask.cuda())
        ctx.set_edit_rows(gtd.cuda(), keep.cuda())
        xa, x0a = _walk(ctx, x_T.cuda().clone(), idx, coefs, mode)
        ctx.set_condition(xf.cuda(), mask.cuda())              # (does not touch the table)
        xb, x0b = _walk(ctx, x_T.cuda().clone(), idx, coefs, mode, one_call=False)
        ctx.clear_edit_rows()
        ctx.set_condition(xf.cuda(), mask.cuda())
        again, _ = _walk(ctx, x_T.cuda().clone(), idx, coefs, mode)
        torch.cuda.synchronize()
        ctx.check()
    finally:
        ctx.close()
    kd = keep.cuda()
    assert bool(torch.isfinite(xa).all()) and bool(torch.isfinite(x0a).all())
    assert torch.equal(xa[kd], gt.cuda()[kd]) and torch.equal(x0a[kd], gt.cuda()[kd])
    assert torch.equal(xa, xb) and torch.equal(x0a, x0b)
    assert torch.equal(again, plain)
    assert torch.equal(xa[2], plain[2])                        # capacity factor 0: a row without an edit keeps its bits beside edited rows
    for b in (0, 1):
        fr = ~kd[b]
        assert float((xa[b][fr] - plain[b][fr]).abs().max()) > 1e-3


# ---- 7. state rules ---------------------------------------------------------------------------------------------
def test_edit_table_refusals_leave_the_context_as_it_was(natives):
    """every refusal of the header returns its code and runs nothing; after all of them a plain mc_sample_step gives the bits it gave
    before, and clearing the table restores mc_sample_loop"""
    dims, nm = natives('C322_T24')
    lib, ptr, stream = _lib()
    C = dims['input_feats']
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, T, seed=395, lengths=LENGTHS)
    noise = torch.randn(B, T, C, generator=torch.Generator().manual_seed(396)).cuda()
    c5 = d.step_coefs(5, 'ddim', dims['scale'], 0.5)
    p5 = d.step_coefs(5, 'ddpm', dims['scale'])
    ms = d.multistep_coefs([5, 4, 3, 2, 1, 0], dims['scale'], 2)
    walk = [d.step_coefs(i, 'ddim', dims['scale'], 0.5) for i in range(6)]
    gt, keep = _edit_tables(dims, T, 397)
    gt, keep = gt.cuda(), keep.cuda()
    ctx = nm.context(B, T, max_steps=6)
    try:
        ctx.set_capacity_factor(0)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        before = ctx.sample_step(x_T.cuda(), 5, c5, noise).clone()
        loop_before = ctx.sample_loop(x_T.cuda().clone(), [5, 4], [walk[5], walk[4]], noise=torch.stack([noise, noise])).clone()
        x = x_T.cuda().clone()

        def code(fn):
            with pytest.raises(RuntimeError) as e:
                fn()
            torch.cuda.synchronize()
            assert torch.equal(x, x_T.cuda())                 # nothing ran
            return str(e.value)
        # exactly one of the two NULL
        assert lib.mc_ctx_set_edit_rows(ctx.handle, gt.data_ptr(), None, None, stream()) == 1
        assert lib.mc_ctx_set_edit_rows(ctx.handle, None, keep.data_ptr(), None, stream()) == 1
        # a seam table / a captured graph in the context: setting is refused, and no table is set afterwards
        ctx.set_seams([0, T - 4, 2 * (T - 4)], 4)
        assert '(code 3)' in code(lambda: ctx.set_edit_rows(gt, keep))
        ctx.clear_seams()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            gx, gn = x_T.cuda().clone(), noise.clone()
            ctx.graph_capture(gx, gn, walk)
            assert '(code 3)' in code(lambda: ctx.set_edit_rows(gt, keep))
            ctx.graph_release()
        side.synchronize()
        assert torch.equal(ctx.sample_step(x_T.cuda(), 5, c5, noise), before)
        # while a table is set
        ctx.set_edit_rows(gt, keep)
        assert '(code 3)' in code(lambda: ctx.set_seams([0, T - 4, 2 * (T - 4)], 4))
        assert '(code 3)' in code(lambda: ctx.sample_step(x, 5, c5, noise, x_prev=x))
        assert '(code 3)' in code(lambda: ctx.sample_loop(x, [5, 4], [walk[5], walk[4]], noise=torch.stack([noise, noise])))
        assert '(code 3)' in code(lambda: ctx.sample_step_inpaint(x, 5, c5, noise, gt, keep, gt_noise=noise, x_prev=x))
        assert '(code 3)' in code(lambda: ctx.sample_step_seeded(x, 5, c5, noise, 1.0, 0.0, x_prev=x))
        assert lib.mc_ctx_graph_step(ctx.handle, 0, stream()) == 3
        with torch.cuda.stream(side):
            assert '(code 3)' in code(lambda: ctx.graph_capture(x_T.cuda().clone(), noise.clone(), walk))
        side.synchronize()
        assert '(code 1)' in code(lambda: ctx.sample_rows(x, [[5] * B], [[c5] * B], noise=noise[None]))     # mode 1 + a noise tensor
        assert '(code 3)' in code(lambda: ctx.sample_rows(x, [[5] * B], [[c5] * B], draws=[[1] * B]))       # mode 1, no seed table
        # modes 0 and 2 take either source
        y = ctx.sample_rows(x_T.cuda().clone(), [[5] * B], [[p5] * B], noise=noise[None])
        ctx.set_row_seeds(SEEDS)
        y2 = ctx.sample_rows(x_T.cuda().clone(), [[5] * B], [[p5] * B], draws=[[1] * B])
        y3 = ctx.sample_rows(x_T.cuda().clone(), [[5] * B], [[ms[0]] * B])
        y4 = ctx.sample_rows(x_T.cuda().clone(), [[5] * B], [[c5] * B], draws=[[1] * B])
        ctx.clear_row_seeds()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in (y, y2, y3, y4))
        # clearing: the uniform entries are back with their bits
        ctx.clear_edit_rows()
        ctx.set_condition(xf.cuda(), mask.cuda())
        after = ctx.sample_step(x_T.cuda(), 5, c5, noise).clone()
        loop_after = ctx.sample_loop(x_T.cuda().clone(), [5, 4], [walk[5], walk[4]], noise=torch.stack([noise, noise])).clone()
        torch.cuda.synchronize()
        assert torch.equal(before, after) and torch.equal(loop_before, loop_after)
        assert torch.equal(x, x_T.cuda())
    finally:
        ctx.close()


def test_fresh_rows_alone_are_replaced(natives):
    """mc_ctx_set_edit_rows with fresh = (0, 1, 0): row 1 takes the new table, rows 0 and 2 keep theirs -- one DDPM tick at schedule
    index 0 (x_prev = x0 there) shows which gt every row holds"""
    dims, nm = natives('C322_T24')
    C = dims['input_feats']
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, T, seed=495, lengths=LENGTHS)
    p0 = d.step_coefs(0, 'ddpm', dims['scale'])
    noise = torch.zeros(1, B, T, C, device='cuda')
    keep = torch.ones(B, T, C, dtype=torch.uint8, device='cuda')
    g1, g2 = torch.full((B, T, C), 1.5, device='cuda'), torch.full((B, T, C), -2.5, device='cuda')
    ctx = nm.context(B, T, max_steps=6)
    try:
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        ctx.set_edit_rows(g1, keep)
        ctx.set_edit_rows(g2, keep, fresh=[False, True, False])
        y = ctx.sample_rows(x_T.cuda().clone(), [[0] * B], [[p0] * B], noise=noise)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert bool((y[0] == 1.5).all()) and bool((y[1] == -2.5).all()) and bool((y[2] == 1.5).all())


# ---- 5. against the reference itself --------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['ddim', 'ddpm'])
def test_edited_walk_vs_reference_golden(natives, mode):
    """tests/golden/edit_small.npz (make_golden_edit.py: the reference's ddim_sample_loop / p_sample_loop with y = {gt, outpainting_mask}
    on row-keyed draws) through set_row_seeds + set_edit_rows + sample_rows at the default capacity factor: the final x within the
    project's end-to-end 1e-3, the kept region equal to gt bit for bit"""
    dims, nm = natives('C322_T24')
    z = np.load(os.path.join(HERE, 'golden', 'edit_small.npz'))
    x_T, xf, mask = (torch.from_numpy(z[k]) for k in ('x_T', 'xf_out', 'motion_mask'))
    gt, keep = torch.from_numpy(z['gt']).cuda(), torch.from_numpy(z['keep']).cuda()
    Bn, Tn, C = x_T.shape
    d = _diffusion('ddim10' if mode == 'ddim' else '10')
    idx = list(range(10))[::-1]
    coefs = [d.step_coefs(i, mode, dims['scale'], 0.0) for i in idx]
    ctx = nm.context(Bn, Tn, max_steps=10)
    try:
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        ctx.set_row_seeds([int(s) for s in z['seeds']])
        x0_draw = ctx.draw_rows(0)
        ctx.set_edit_rows(gt, keep)
        x = ctx.sample_rows(x_T.cuda().clone(), [[i] * Bn for i in idx], [[c] * Bn for c in coefs], draws=[[1 + k] * Bn for k in range(10)])
        torch.cuda.synchronize()
        ctx.check()
    finally:
        ctx.close()
    assert float((x0_draw.cpu() - x_T).abs().max()) <= 1e-5       # x_T of the golden is draw 0 of the rows' seeds
    err = float((x.cpu() - torch.from_numpy(z[f'final_{mode}'])).abs().max())
    print(f'edit golden {mode}: |hip - reference| {err:.2e}')
    assert err <= 1e-3
    assert torch.equal(x[keep], gt[keep])


# ---- 6. requests with an edit through both batchers ------------------------------------------------------------------
@pytest.fixture(scope='module')
def arch():
    import motioncraft_amd as mc
    from oracle import weights as W
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_small.py'))
    cfg.model.diffusion_test = dict(BASE, respace='ddim10')
    a = mc.build_architecture(cfg.model)
    a.load_state_dict({'model.' + k: v for k, v in W.make_state_dict(SMALL, SMALL_SEED).items()})
    yield a
    a.model.release()


@pytest.mark.parametrize('sampler', MODES)
def test_edited_request_is_a_function_of_the_request_in_both_batchers(arch, sampler):
    """ContinuousBatcher at capacity factor 0, 6 steps: the kept region of the result equals pre_process(motion) bit for bit (model space;
    the test config has no post_process_cfg: the identity), the free region differs from the same request without its edit, a batchmate
    without an edit has the bits it has with no edit anywhere; the edited request keeps its bits in another row, beside other batchmates,
    joining three ticks after the batch started, and from RequestBatcher"""
    from motioncraft_amd.serve import ContinuousBatcher, Edit, Request, RequestBatcher
    C = SMALL['input_feats']
    assert arch.model.post_process_cfg is None

    def make(i, length, edit=None):
        xf = torch.nn.functional.layer_norm(torch.randn(SMALL['Nt'], SMALL['Dt'], generator=torch.Generator().manual_seed(710 + i)), (SMALL['Dt'],))
        return Request(length=length, seed=7100 + i, xf_out=xf, edit=edit)
    motion = torch.randn(20, C, generator=torch.Generator().manual_seed(72))
    keep = Edit.keyframes(motion, [0, 1, 19]).keep | Edit.parts(motion, ['lleg', 'root'], 'motionx', frames=range(5, 9)).keep
    assert bool(torch.equal(arch.model.pre_process(motion), motion))
    A, A0 = make(0, 20, Edit(motion, keep)), make(0, 20)
    P, Q, R, S = make(1, 17), make(2, 24), make(3, 22), make(4, 9)

    def cont(first, late=()):
        bt = ContinuousBatcher(arch, batch=B, frames=T, sampler=sampler, steps=6)
        hs = [(r, bt.submit(r)) for r in first]
        if late:
            for _ in range(3):
                bt.tick()
            hs += [(r, bt.submit(r)) for r in late]
        out = bt.run()
        torch.cuda.synchronize()
        return {id(r): out[h].clone() for r, h in hs}
    base = cont([A, P, Q])
    plain = cont([A0, P, Q])
    got = base[id(A)]
    assert tuple(got.shape) == (20, C) and bool(torch.isfinite(got).all())
    assert torch.equal(got.cpu()[keep], motion[keep])
    assert float((got.cpu()[~keep] - plain[id(A0)].cpu()[~keep]).abs().max()) > 1e-3
    assert torch.equal(base[id(P)], plain[id(P)]) and torch.equal(base[id(Q)], plain[id(Q)])
    assert torch.equal(cont([P, Q, A])[id(A)], got)                       # another row
    assert torch.equal(cont([A, R, S])[id(A)], got)                       # other batchmates
    assert torch.equal(cont([P, Q], late=[A])[id(A)], got)                # joins a running batch
    rb = RequestBatcher(arch, batch=B, frames=T, sampler=sampler, steps=6, capacity_factor=0)
    ha, hp = rb.submit(A), rb.submit(P)
    out = rb.run()
    torch.cuda.synchronize()
    assert torch.equal(out[ha], got) and torch.equal(out[hp], base[id(P)])
    hq = rb.submit(Q)                                                     # a batch without an edit: the fused loop, no table left behind
    assert bool(torch.isfinite(rb.run()[hq]).all())


# ---- 4. lockstep with the oracle, rows at mixed walk positions -----------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_mixed_positions_in_lockstep_with_the_oracle(natives, mode):
    """rows 0 / 1 / 2 start their ddim6 walks at schedule indices 5 / 3 / 4 and tick together, capacity factor 0, one tick per call.  Every
    tick against the oracle teacher-forced to the device's x_t and expert ids: rowstep_ref.denoise_rows, then edit_ref.edit_rows on the
    device's own draws (step draw d, kept region d ^ 2^63) -- within the per-call bound 2e-4"""
    import rowstep_ref
    from oracle import weights as W
    dims, nm = natives('C322_T24')
    sd = W.make_state_dict(dims, SMALL_SEED)
    C = dims['input_feats']
    TC = T * C
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, T, seed=591, lengths=LENGTHS)
    gt, keep = _edit_tables(dims, T, 592)
    starts = [5, 3, 4]
    if mode == 'dpmpp':                                        # every row its own walk from its start: a first step reads no history
        walks = [d.multistep_coefs(list(range(s, -1, -1)), dims['scale'], 2) for s in starts]
    else:
        walks = [[d.step_coefs(i, mode, dims['scale'], 0.5 if mode == 'ddim' else 0.0) for i in range(s, -1, -1)] for s in starts]
    ctx = nm.context(B, T, max_steps=6)
    worst = 0.0
    try:
        ctx.enable_capture()
        ctx.set_capacity_factor(0)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        ctx.set_row_seeds(SEEDS)
        ctx.set_edit_rows(gt.cuda(), keep.cuda())
        x, x0 = x_T.cuda().clone(), torch.zeros(B, T, C, device='cuda')
        torch.set_num_threads(4)
        for k in range(4):
            idx = [s - k for s in starts]
            coefs = [walks[b][k] for b in range(B)]
            draws = [1 + k + 10 * b for b in range(B)]
            before, hist = x.cpu(), x0.cpu()
            nz = torch.stack([ctx.draw_rows(dr)[b] for b, dr in enumerate(draws)]).cpu()
            z2 = torch.stack([ctx.draw_rows(dr ^ FLIP)[b] for b, dr in enumerate(draws)]).cpu()
            ctx.sample_rows(x, [idx], [coefs], draws=None if mode == 'dpmpp' else [draws], x0=x0)
            torch.cuda.synchronize()
            forced = [ctx.routing(i) for i in range(dims['NL'])]
            x0m = rowstep_ref.denoise_rows(sd, dims, before, [int(d.timestep_map[i]) for i in idx], xf, mask, forced_routing=forced,
                                           capacity_factor=float(dims['E']))
            want, want0 = edit_ref.edit_rows(before, x0m, torch.zeros_like(x0m), nz, hist, gt, keep, z2, coefs, TC)
            err = float(np.abs(x.cpu().double().numpy().reshape(-1) - want).max())
            err0 = float(np.abs(x0.cpu().double().numpy().reshape(-1) - want0).max())
            print(f'{mode} tick {k} at indices {idx}: |x - oracle| {err:.2e}, |x0 - oracle| {err0:.2e}')
            worst = max(worst, err, err0)
        ctx.check()
    finally:
        ctx.close()
    assert worst <= 2e-4
    assert torch.equal(x[1][keep[1].cuda()], gt[1][keep[1]].cuda())        # row 1 reached schedule index 0


# ---- a cleared table leaves nothing behind ---------------------------------------------------------------------------
def test_a_clear_leaves_no_row_kept(natives):
    """every row kept at 1.5, cleared, then row 1 alone uploaded at -2.5: rows 0 and 2 hold NOTHING (a clear zeroes the keep bytes) --
    one DDPM tick at schedule index 0 gives them the model's x0, the bits of the tick without a table"""
    dims, nm = natives('C322_T24')
    C = dims['input_feats']
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, T, seed=695, lengths=LENGTHS)
    p0 = d.step_coefs(0, 'ddpm', dims['scale'])
    noise = torch.zeros(1, B, T, C, device='cuda')
    keep = torch.ones(B, T, C, dtype=torch.uint8, device='cuda')
    ctx = nm.context(B, T, max_steps=6)
    try:
        ctx.set_capacity_factor(0)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        plain = ctx.sample_rows(x_T.cuda().clone(), [[0] * B], [[p0] * B], noise=noise).clone()
        ctx.set_edit_rows(torch.full((B, T, C), 1.5, device='cuda'), keep)
        ctx.clear_edit_rows()
        ctx.set_edit_rows(torch.full((B, T, C), -2.5, device='cuda'), keep, fresh=[False, True, False])
        y = ctx.sample_rows(x_T.cuda().clone(), [[0] * B], [[p0] * B], noise=noise)
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert bool((y[1] == -2.5).all()) and torch.equal(y[0], plain[0]) and torch.equal(y[2], plain[2])
    assert not bool((plain == 1.5).any())


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp'])
def test_a_table_set_again_spares_a_running_request_without_an_edit(arch, sampler):
    """batch 2, walk 4: A (edit) in row 0; P joins row 1 at tick 2; A retires at tick 4 and the table is cleared; Q (no edit) takes row 0;
    P retires at tick 6 and R (edit) takes row 1, which sets a table again with Q mid-walk on the row A left.  Q has the bits it has
    served alone, and A's kept region is nowhere in it; R ends on its own edit"""
    from motioncraft_amd.serve import ContinuousBatcher, Edit, Request
    C = SMALL['input_feats']

    def make(i, edit=None):
        xf = torch.nn.functional.layer_norm(torch.randn(SMALL['Nt'], SMALL['Dt'], generator=torch.Generator().manual_seed(810 + i)), (SMALL['Dt'],))
        return Request(length=T, seed=8100 + i, xf_out=xf, edit=edit)
    ma, mr = (torch.randn(T, C, generator=torch.Generator().manual_seed(s)) for s in (82, 83))
    ea, er = Edit.keyframes(ma, [0, 1, 2, 12, 23]), Edit.keyframes(mr, [5, 6, 20])
    A, P, Q, R = make(0, ea), make(1), make(2), make(3, er)

    def serve(arrivals):
        bt = ContinuousBatcher(arch, batch=2, frames=T, sampler=sampler, steps=4)
        hs, out, k = {}, {}, 0
        while k < len(arrivals) or any(h is not None for h in bt.occupied):
            while k < len(arrivals) and arrivals[k][0] <= bt.ticks:
                hs[id(arrivals[k][1])] = bt.submit(arrivals[k][1])
                k += 1
            assert bt.tick() == 1
            out.update(bt.poll())
        torch.cuda.synchronize()
        return {key: out[h].clone() for key, h in hs.items()}, bt
    alone, _ = serve([(0, Q)])
    got, bt = serve([(0, A), (2, P), (4, Q), (6, R)])
    assert (bt.finished_at[2], bt.submitted_at[3], bt.finished_at[3]) == (8, 6, 10)       # Q walked ticks 4-8, R joined beside it at 6
    q = got[id(Q)]
    assert torch.equal(q, alone[id(Q)]), float((q - alone[id(Q)]).abs().max())
    assert not bool((q.cpu()[ea.keep] == ma[ea.keep]).any())
    assert torch.equal(got[id(A)].cpu()[ea.keep], ma[ea.keep]) and torch.equal(got[id(R)].cpu()[er.keep], mr[er.keep])

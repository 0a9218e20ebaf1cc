"""GPU (MI355X): a row of a batch as an independent request -- row-keyed noise (``mc_ctx_set_row_seeds`` / ``mc_ctx_draw_rows``, the
fused loop and the seam kernel with row keys), drop-free routing (``mc_ctx_set_capacity_factor(0)``: the keep-all short cut on all
routing paths) and what follows from the two: a row's result does not depend on its batchmates or on its place in the batch.

Shapes: the reduced config (``helpers.SMALL``: L = 32, NL = 2, C = 322) at B = 3, T = 24, lengths (24, 17, 20), with ``hot_pair`` gates so
that the default capacity factor really drops tokens; C = 263, T = 23 (``HML_SMALL``) where a flat group of four straddles two rows.
Device-against-device comparisons are exact (torch.equal); oracle comparisons use the project's bounds (2e-4 per call, 1e-3 per
trajectory)."""
import contextlib
import faulthandler
import os

import numpy as np
import pytest
import torch

import rowseed_ref
import seam_ref as S
from helpers import HML_SMALL, SMALL, SMALL_SEED, bpr_keep, skew_gates, synth_inputs

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
    torch.set_num_threads(threads)             # (the oracle calls below run on 4 threads; later tests keep theirs)
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
    """shape id -> (dims, state dict, NativeModel); SMALL with hot_pair gates"""
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
    """the Python model (MotionDiffusion over the reduced config) with hot_pair gates"""
    import motioncraft_amd as mc
    from oracle import weights as W
    sd = skew_gates(W.make_state_dict(SMALL, SMALL_SEED), SMALL, 'hot_pair')
    cfg = mc.Config.fromfile(os.path.join(HERE, 'configs', 'stmogen_small.py'))
    cfg.model.diffusion_test = dict(BASE, respace='ddim10')
    a = mc.build_architecture(cfg.model)
    a.load_state_dict({'model.' + k: v for k, v in sd.items()})
    yield sd, a
    a.model.release()


# ---- 1. mc_ctx_draw_rows ------------------------------------------------------------------------
@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('offset', [32, 33], ids=['aligned', 'unaligned'])
def test_draw_rows_gives_every_row_its_b1_stream(natives, shape, offset):
    """every row of mc_ctx_draw_rows is mc_op_philox_normal with that row's seed, bit for bit (and the numpy restatement's row); the
    words in front of and behind the buffer stay untouched; equal seeds give equal rows, distinct seeds distinct ones"""
    dims, _, nm = natives(shape)
    Tn, C = SHAPES[shape][1], dims['input_feats']
    lib, ptr, stream = _lib()
    seeds = [SEEDS[0], SEEDS[1], SEEDS[0]]
    ctx = nm.context(B, Tn, max_steps=1)
    try:
        with pytest.raises(RuntimeError, match=r'\(code 3\).*no seed table'):
            ctx.draw_rows(0)
        ctx.set_row_seeds(seeds)
        n, guard = B * Tn * C, 64
        for draw in (0, 5):
            buf = torch.full((offset + n + guard,), -7.5, device='cuda')
            out = buf[offset:offset + n].view(B, Tn, C)
            ctx.draw_rows(draw, out=out)
            torch.cuda.synchronize()
            assert bool((buf[:offset] == -7.5).all()) and bool((buf[offset + n:] == -7.5).all())
            want = rowseed_ref.draw_rows(seeds, Tn, C, draw)
            for b, s in enumerate(seeds):
                one = torch.empty(Tn * C, device='cuda')
                assert lib.mc_op_philox_normal(ptr(one), None, Tn * C, s, draw, stream()) == 0
                torch.cuda.synchronize()
                assert torch.equal(out[b].reshape(-1), one), (b, draw)
                # (numpy's log / sin / cos against the device's: the bound tests/test_gpu_parity.py holds mc_op_philox_normal to)
                assert np.abs(out[b].cpu().numpy().astype(np.float64) - want[b]).max() <= 4e-6, (b, draw)
            assert torch.equal(out[0], out[2]) and not torch.equal(out[0], out[1])
        ctx.clear_row_seeds()
        with pytest.raises(RuntimeError, match=r'\(code 3\)'):
            ctx.draw_rows(0)
    finally:
        ctx.close()


# ---- 2. the fused loop with a seed table ----------------------------------------------------------
@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('mode,eta', [('ddpm', 0.0), ('ddim', 0.5)])
def test_fused_loop_with_a_seed_table_equals_the_loop_fed_its_draws(natives, shape, mode, eta):
    """6 steps in place: noise_dev == NULL under a seed table (draw 1 + k, the seed argument ignored) equals the same loop reading
    noise_dev stacked from mc_ctx_draw_rows(1 + k), bit for bit; without the table the flat stream gives other bits"""
    dims, _, nm = natives(shape)
    Tn, C = SHAPES[shape][1], dims['input_feats']
    d = _diffusion('ddim6')
    x_T, xf, mask = synth_inputs(dims, B, Tn, seed=61, lengths=[Tn, Tn - 7, Tn - 4])
    idx = list(range(6))[::-1]
    coefs = [d.step_coefs(i, mode, dims['scale'], eta) for i in idx]
    ctx = nm.context(B, Tn, max_steps=6)
    try:
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        flat = ctx.sample_loop(x_T.cuda().clone(), idx, coefs, noise=None, seed=99, draw0=1).clone()
        ctx.set_row_seeds(SEEDS)
        got = [ctx.sample_loop(x_T.cuda().clone(), idx, coefs, noise=None, seed=s, draw0=1).clone() for s in (99, 12345)]
        nz = torch.stack([ctx.draw_rows(1 + k) for k in range(6)])
        fed = ctx.sample_loop(x_T.cuda().clone(), idx, coefs, noise=nz).clone()
        torch.cuda.synchronize()
    finally:
        ctx.close()
    assert bool(torch.isfinite(fed).all())
    assert torch.equal(got[0], fed), float((got[0] - fed).abs().max())
    assert torch.equal(got[0], got[1])
    assert not torch.equal(got[0], flat)


def test_python_seeds_give_the_same_bits_fused_per_step_and_replayed(arch):
    """p_sample_loop(seeds=...): x_T is draw 0, the n-th randn_like draw 1 + n -- the fused loop, one mc_sample_step per step and graph
    replay (the host refills the noise buffer from mc_ctx_draw_rows) walk the same bits; a seeds list of the wrong length raises"""
    sd, a = arch
    d = _diffusion('ddim6')
    _, xf, mask = synth_inputs(SMALL, B, T, seed=62, lengths=LENGTHS)
    kw = dict(xf_out=xf, motion_mask=mask, y={})
    C = SMALL['input_feats']
    outs = {}
    for name, extra in (('fused', dict(fused=True)), ('per_step', dict(fused=False)), ('graph', dict(graph=True))):
        outs[name] = d.p_sample_loop(a.model, (B, T, C), clip_denoised=False, model_kwargs=kw, seeds=SEEDS, **extra).clone()
        torch.cuda.synchronize()
        assert a.model._ctx[(B, T)].row_seeds is None                      # the loop cleared the table behind it
    assert bool(torch.isfinite(outs['fused']).all())
    assert torch.equal(outs['fused'], outs['per_step']) and torch.equal(outs['fused'], outs['graph'])
    other = d.p_sample_loop(a.model, (B, T, C), clip_denoised=False, model_kwargs=kw, seeds=[SEEDS[0], SEEDS[1], 4]).clone()
    assert not torch.equal(other[2], outs['fused'][2])
    for bad in ([1, 2], [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            d.p_sample_loop(a.model, (B, T, C), clip_denoised=False, model_kwargs=kw, seeds=bad)
    with pytest.raises(ValueError, match='exclusive'):
        d.p_sample_loop(a.model, (B, T, C), clip_denoised=False, model_kwargs=kw, seeds=SEEDS, noise=torch.zeros(B, T, C))


# ---- 3. keep-all routing --------------------------------------------------------------------------
PATHS = {                    # name -> (MC_ROUTE_SMALL_CTX or None, options)
    'one_workgroup': (None, {}),
    'cooperative': ('0', {'route_coop': 1}),
    'launch_sequence': ('0', {'route_coop': 0}),
    'two_groups_early': ('0', {'big_tokens': 0, 'route_early': 1}),
    'two_groups_joined': ('0', {'big_tokens': 0, 'route_early': 0, 'route_coop': 0}),
    'two_groups_joined_coop': ('0', {'big_tokens': 0, 'route_early': 0, 'route_coop': 1}),
}


def _path_context(nm, monkeypatch, path, xf, mask, timesteps=(640,)):
    env, options = PATHS[path]
    if env is not None:
        monkeypatch.setenv('MC_ROUTE_SMALL_CTX', env)          # read when a context is created: no one-workgroup routing kernel
    ctx = nm.context(B, T, max_steps=len(timesteps))
    for k, v in options.items():
        ctx.set_option(k, v)
    if path == 'cooperative':
        assert ctx.uses_coop_routing
    ctx.set_timesteps(list(timesteps))
    ctx.set_condition(xf.cuda(), mask.cuda())
    return ctx


def _check_slots(ctx, nsrc, E, what):
    """every (token, choice) of the source tokens owns exactly one slot, inside a tile of its expert; the tiles cover the slots once"""
    idx = ctx.buffer('idx', dtype=torch.int32)[:2 * nsrc].cpu().numpy()
    dst = ctx.buffer('dst_row', dtype=torch.int32)[:2 * nsrc].cpu().numpy()
    src = ctx.buffer('src_row', dtype=torch.int32)[:2 * nsrc].cpu().numpy()
    tg, tr0, tn = (ctx.buffer(n, dtype=torch.int32).cpu().numpy() for n in ('tile_group', 'tile_row0', 'tile_nrows'))
    nt = ctx.buffer('num_tiles', dtype=torch.int32).cpu().numpy()
    assert np.array_equal(np.sort(dst), np.arange(2 * nsrc)), what
    assert np.array_equal(src, dst >> 1), what
    max_tiles = tg.shape[0] // 2
    expert_of_slot = np.full(2 * nsrc, -1, dtype=np.int64)
    for g in range(2):
        for t in range(g * max_tiles, g * max_tiles + int(nt[g])):
            e, r0, nr = int(tg[t]), int(tr0[t]), int(tn[t])
            assert 0 <= e < E and 1 <= nr <= 128 and 0 <= r0 and r0 + nr <= 2 * nsrc, (what, g, e, r0, nr)
            assert (expert_of_slot[r0:r0 + nr] == -1).all(), (what, 'tiles overlap')
            expert_of_slot[r0:r0 + nr] = e
    assert np.array_equal(expert_of_slot, idx[dst]), (what, 'the tile that holds a pair belongs to idx[token][choice]')


@pytest.mark.parametrize('path', sorted(PATHS))
def test_keep_all_routing_on_every_path(natives, monkeypatch, path):
    """Routing capture on.  At 1.5 the inputs drop pairs (zeros in cap_w, the keep flags of the last layer = helpers.bpr_keep); at
    capacity factor 0, layer by layer: comb_w == gate bit for bit for all N pairs, route_split == 0, every pair owns a slot in a tile of
    its expert.  A negative factor is MC_ERR_ARG, and the call clears the condition."""
    dims, _, nm = natives('C322_T24')
    E, H, NL = dims['E'], dims['H'], dims['NL']
    N = 2 * B * T * H
    x, xf, mask = synth_inputs(dims, B, T, seed=63, lengths=LENGTHS)
    ctx = _path_context(nm, monkeypatch, path, xf, mask)
    try:
        ctx.enable_capture()
        assert ctx.capacity_factor == 1.5
        ctx.denoise(x.cuda(), 0)
        torch.cuda.synchronize()
        idx, keep = ctx.routing(NL - 1)
        want = bpr_keep(ctx.buffer('idx', dtype=torch.int32), ctx.buffer('key', dtype=torch.int32), E, 2 * int(1.5 * ((N + E - 1) // E)))
        assert np.array_equal(keep.numpy(), want) and not want.all(), 'precondition: the default factor drops pairs of these inputs'
        assert all(bool((ctx.buffer('cap_w', l) == 0).any()) for l in range(NL))
        with pytest.raises(RuntimeError, match=r'\(code 1\)'):
            ctx.set_capacity_factor(-1.0)
        ctx.set_capacity_factor(0)
        assert ctx.capacity_factor == 0.0
        with pytest.raises(RuntimeError, match='mc_ctx_set_condition not called'):
            ctx.denoise(x.cuda(), 0)
        ctx.set_condition(xf.cuda(), mask.cuda())
        for l in range(NL):
            ctx.denoise(x.cuda(), 0, stop_after_layers=l + 1)
            torch.cuda.synchronize()
            nsrc = N // 2 if l == 0 else N                     # base layer 0 is the CFG-twin layer: gate outputs for the first half only
            comb, gate = ctx.buffer('comb_w'), ctx.buffer('gate')
            assert torch.equal(comb[:2 * nsrc], gate[:2 * nsrc]), (path, l)
            if nsrc < N:
                assert torch.equal(comb[2 * nsrc:2 * N], gate[:2 * nsrc]), (path, l)
            assert bool((comb[:2 * N] > 0).all())
            assert int(ctx.buffer('route_split', dtype=torch.int32)[0]) == 0
            _check_slots(ctx, nsrc, E, f'{path} layer {l}')
        out = ctx.denoise(x.cuda(), 0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        assert all(bool((ctx.buffer('cap_w', l) != 0).all()) for l in range(NL))
        ctx.check()
    finally:
        ctx.close()


@pytest.mark.parametrize('prec', ['f32', 'f16x3'])
@pytest.mark.parametrize('path', ['one_workgroup', 'two_groups_early'])
def test_keep_all_call_meets_the_oracle_without_drops(natives, monkeypatch, path, prec):
    """one denoiser call at capacity factor 0 against oracle.denoise(capacity_factor = E), teacher-forced to the device's expert ids
    (a top-2 choice may flip at a near tie): the per-call bound, 2e-4, in fp32 and in the fp16 split mode"""
    from oracle import stmogen_oracle as O
    dims, sd, nm = natives('C322_T24')
    x, xf, mask = synth_inputs(dims, B, T, seed=64, lengths=LENGTHS)
    env, options = PATHS[path]
    if env is not None:
        monkeypatch.setenv('MC_ROUTE_SMALL_CTX', env)
    ctx = nm.context(B, T, max_steps=1)
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        if prec != 'f32':
            ctx.set_option('half_min_rows', 0)
            ctx.set_precision(prec)
            assert ctx.effective_precision == prec
        ctx.enable_capture()
        ctx.set_capacity_factor(0)
        ctx.set_timesteps([640])
        ctx.set_condition(xf.cuda(), mask.cuda())
        out2 = ctx.denoise(x.cuda(), 0).cpu()
        forced = [ctx.routing(i) for i in range(dims['NL'])]
    finally:
        ctx.close()
    assert all(bool(k.all()) for _, k in forced)
    torch.set_num_threads(4)
    ref = O.denoise(sd, dims, x, 640, xf, mask, forced_routing=forced, capacity_factor=float(dims['E']))
    w = (1 - (1000 - 640) / 1000) * dims['scale'] + 1
    err = float((out2[:B] * w + out2[B:] * (1 - w) - ref).abs().max())
    print(f'{path} {prec}: |device - oracle (no drops, teacher-forced ids)| {err:.2e}; |out| {float(ref.abs().max()):.2f}')
    assert err <= TOL_CALL


# ---- 4. / 5. independence -------------------------------------------------------------------------
def _requests(seed, lengths):
    _, xf, mask = synth_inputs(SMALL, B, T, seed=seed, lengths=lengths)
    return xf, mask


@contextlib.contextmanager
def _arch_context(a, d, monkeypatch, two_groups=False, prec='f32'):
    """a fresh cached (B, T) context of the Python model under the named schedule / precision; dropped again afterwards"""
    old = a.model._ctx.pop((B, T), None)
    if old is not None:
        old.close()
    if two_groups:
        monkeypatch.setenv('MC_ROUTE_SMALL_CTX', '0')
    old_prec = a.model.precision
    a.model.precision = prec
    xf, mask = _requests(70, LENGTHS)
    ctx = a.model.sampling_context(B, T, d.timestep_map, dict(xf_out=xf, motion_mask=mask))
    if two_groups:                                 # the way tests/test_route_early.py forces the large-batch schedule
        ctx.set_option('big_tokens', 0)
        ctx.set_option('route_early', 1)
    if prec != 'f32':
        ctx.set_option('half_min_rows', 0)
    try:
        yield ctx
    finally:
        a.model.precision = old_prec
        a.model._ctx.pop((B, T)).close()
        monkeypatch.delenv('MC_ROUTE_SMALL_CTX', raising=False)


def _walk6(a, d, xf, mask, seeds, cf):
    kw = dict(xf_out=xf, motion_mask=mask, y={})
    if cf is not None:
        kw['capacity_factor'] = cf
    out = d.p_sample_loop(a.model, (B, T, SMALL['input_feats']), clip_denoised=False, model_kwargs=kw, seeds=seeds).clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('variant', ['default', 'two_groups', 'f16x3'])
def test_row_does_not_depend_on_its_batchmates(arch, monkeypatch, variant):
    """6-step DDPM walk, seeds=, capacity factor 0: replacing rows 1-2 (prompt features, lengths, seeds) leaves row 0 bit-equal.
    Control (default variant): at 1.5 the same replacement moves row 0 by more than 1e-3 -- the test cannot pass without the feature."""
    sd, a = arch
    d = _diffusion('ddim6')
    xf, mask = _requests(71, LENGTHS)
    xf2, mask2 = _requests(72, (24, 9, 24))
    xfr, maskr = xf.clone(), mask.clone()
    xfr[1:], maskr[1:] = xf2[1:], mask2[1:]
    seeds_r = [SEEDS[0], 1234, 2 ** 40 + 1]
    with _arch_context(a, d, monkeypatch, two_groups=variant == 'two_groups', prec='f16x3' if variant == 'f16x3' else 'f32') as ctx:
        full = _walk6(a, d, xf, mask, SEEDS, 0)
        repl = _walk6(a, d, xfr, maskr, seeds_r, 0)
        if variant == 'f16x3':
            assert ctx.effective_precision == 'f16x3'
        assert bool(torch.isfinite(full).all())
        assert torch.equal(full[0], repl[0]), float((full[0] - repl[0]).abs().max())
        assert not torch.equal(full[1], repl[1])
        if variant == 'default':
            full15 = _walk6(a, d, xf, mask, SEEDS, None)
            repl15 = _walk6(a, d, xfr, maskr, seeds_r, None)
            moved = float((full15[0] - repl15[0]).abs().max())
            print(f'row 0 under replaced batchmates: 0 at capacity factor 0, {moved:.2e} at 1.5')
            assert moved > 1e-3
            assert ctx.capacity_factor == 1.5                      # a call without the setting is back on the model's factor


@pytest.mark.parametrize('variant', ['default', 'two_groups'])
def test_row_does_not_depend_on_its_place(arch, monkeypatch, variant):
    """the request of row 0 placed in row 2 gives the same bits (no kernel's result depends on a row's place: the sample groups are the
    CFG halves, every GEMM row keeps its k-order)"""
    sd, a = arch
    d = _diffusion('ddim6')
    xf, mask = _requests(73, LENGTHS)
    perm = [2, 1, 0]
    with _arch_context(a, d, monkeypatch, two_groups=variant == 'two_groups'):
        first = _walk6(a, d, xf, mask, SEEDS, 0)
        moved = _walk6(a, d, xf[perm].contiguous(), mask[perm].contiguous(), [SEEDS[p] for p in perm], 0)
    for b in range(B):
        assert torch.equal(first[b], moved[perm.index(b)]), (b, float((first[b] - moved[perm.index(b)]).abs().max()))


# ---- 6. batch against alone -----------------------------------------------------------------------
def test_batch_rows_and_lone_requests_meet_the_oracle_alone(arch, monkeypatch):
    """10-step DDIM: row b of the B = 3 walk and the B = 1 walk with seed = seeds[b] are each within 1e-3 (the per-trajectory bound) of
    the oracle's B = 1 walk on the same draws without drops.  (Across batch sizes the kernel selection changes: no bit equality.)"""
    from oracle import philox_oracle as P
    from oracle import stmogen_oracle as O
    sd, a = arch
    d = _diffusion('ddim10')
    C = SMALL['input_feats']
    xf, mask = _requests(74, LENGTHS)
    kw = dict(xf_out=xf, motion_mask=mask, y={}, capacity_factor=0)
    batch = d.ddim_sample_loop(a.model, (B, T, C), clip_denoised=False, model_kwargs=kw, seeds=SEEDS).cpu()
    monkeypatch.setattr(O, 'CAPACITY_FACTOR', float(SMALL['E']))           # read by precompute_text and every MoE of the walk
    torch.set_num_threads(4)
    sched = O.Schedule(1000, 'ddim10')
    for b in range(B):
        kw1 = dict(xf_out=xf[b:b + 1], motion_mask=mask[b:b + 1], y={}, capacity_factor=0)
        alone = d.ddim_sample_loop(a.model, (1, T, C), clip_denoised=False, model_kwargs=kw1, seeds=[SEEDS[b]]).cpu()
        x_T = torch.from_numpy(P.draw_normal(T * C, SEEDS[b], 0)).view(1, T, C)
        ref = O.sample_loop(sd, SMALL, sched, 'ddim', x_T, xf[b:b + 1], mask[b:b + 1], step_noise=lambda i: torch.zeros(1, T, C))
        e_batch, e_alone = float((batch[b] - ref[0]).abs().max()), float((alone[0] - ref[0]).abs().max())
        print(f'row {b}: |batch row - oracle alone| {e_batch:.2e}, |alone - oracle alone| {e_alone:.2e}; |x| {float(ref.abs().max()):.2f}')
        assert e_batch <= TOL_TRAJ and e_alone <= TOL_TRAJ, (b, e_batch, e_alone)


# ---- 7. seams with row keys -------------------------------------------------------------------------
def test_seam_kernel_takes_the_left_rows_key(natives):
    """B = 3 chain, overlap 6, 4-step DDPM, one fused step at a time under a seed table: seam pairs are bit-equal after every step, the
    walk equals the one fed noise_dev from mc_ctx_draw_rows (the seam kernel reads the LEFT row's element there), and off the seams one
    step equals the uncoupled row-keyed step from the same x"""
    dims, _, nm = natives('C322_T24')
    C, ov = dims['input_feats'], 6
    ff = [0, T - ov, 2 * (T - ov)]
    flags = S.plan_flags(ff, T, ov)
    d = _diffusion('ddim4')
    _, xf, mask = synth_inputs(dims, B, T, seed=65)
    z = torch.randn(ff[-1] + T, C, generator=torch.Generator().manual_seed(66))
    x_T = torch.stack([z[f:f + T] for f in ff])                            # equal on shared frames
    idx = list(range(4))[::-1]
    coefs = [d.step_coefs(i, 'ddpm', dims['scale']) for i in idx]
    ctx = nm.context(B, T, max_steps=4)
    try:
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        ctx.set_row_seeds(SEEDS)
        plain1 = ctx.sample_loop(x_T.cuda().clone(), idx[:1], coefs[:1], noise=None, draw0=1).clone()
        ctx.set_seams(ff, ov)
        x = x_T.cuda().clone()
        fed = x_T.cuda().clone()
        for k in range(4):
            ctx.sample_loop(x, idx[k:k + 1], coefs[k:k + 1], noise=None, draw0=1 + k)
            ctx.sample_loop(fed, idx[k:k + 1], coefs[k:k + 1], noise=ctx.draw_rows(1 + k)[None])
            torch.cuda.synchronize()
            assert S.seams_equal(x.cpu().numpy(), flags, ov), k
            assert torch.equal(x, fed), (k, float((x - fed).abs().max()))
            if k == 0:
                off = ~torch.from_numpy(S.seam_mask(flags, T, ov))
                assert torch.equal(x.cpu()[off], plain1.cpu()[off])
                assert not S.seams_equal(plain1.cpu().numpy(), flags, ov)
        whole = ctx.sample_loop(x_T.cuda().clone(), idx, coefs, noise=None, draw0=1)
        torch.cuda.synchronize()
        assert torch.equal(whole, x) and bool(torch.isfinite(x).all())
    finally:
        ctx.close()


# ---- 7b. every drawn-noise form of the sampler update at both operand alignments -------------------
@pytest.mark.parametrize('Bn', [3, 4], ids=['odd_elements', 'whole_vectors'])
def test_drawn_noise_forms_equal_the_forms_fed_their_draws_at_both_alignments(natives, Bn):
    """C = 263, T = 7 (T C = 1841 is odd: flat groups of four straddle every row boundary; at B = 3 the element count is odd too, so the
    second partial product of the decoder tail is off 16-byte alignment and n % 4 == 3 leaves a ragged last group; at B = 4 every operand
    is aligned).  Two fused steps, modes 0 and 1, without and with a seam table (overlap 3, first frames 0, 4, 8, ..): the loop that draws
    in the kernel -- from the call's stream, and from the rows' keys -- equals the loop fed the same normals as a tensor
    (mc_op_philox_normal / mc_ctx_draw_rows), bit for bit; one tick of per-row schedules at mixed steps and draw numbers likewise.
    This pins the NOISE path only (which key, which counter, which draw number, the left row's element on a seam).  It depends on the
    op tests for the rest: the tensor-fed forms it compares with are held against fp64, with guard sentinels around every output, by
    test_seam_op, test_seam_rows_op, test_per_row_sampler_kernels_vs_fp64 and test_multistep_op_vs_fp64 at the same C and T; a context
    owns its buffers, so a store outside an output cannot show here.  No op entry draws from row keys under a seam table."""
    lib, ptr, stream = _lib()
    dims, _, nm = natives('C263_T23')
    Tn, C, ov = 7, dims['input_feats'], 3
    assert C == 263
    n, TC = Bn * Tn * C, Tn * C
    d = _diffusion('ddim4')
    seeds = (SEEDS + [77])[:Bn]
    ff = [b * (Tn - ov) for b in range(Bn)]
    z = torch.randn(ff[-1] + Tn, C, generator=torch.Generator().manual_seed(68))
    x_T = torch.stack([z[f:f + Tn] for f in ff]).cuda()                       # equal on shared frames
    _, xf, mask = synth_inputs(dims, Bn, Tn, seed=67)
    idx = [3, 2]

    def normals(count, seed, draw):
        out = torch.empty(count, device='cuda')
        assert lib.mc_op_philox_normal(ptr(out), None, count, seed & (2 ** 64 - 1), draw, stream()) == 0, lib.mc_last_error()
        return out

    ctx = nm.context(Bn, Tn, max_steps=4)
    try:
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        for mode, eta in (('ddpm', 0.0), ('ddim', 0.5)):
            coefs = [d.step_coefs(i, mode, dims['scale'], eta) for i in idx]
            for seam in (False, True):
                if seam:
                    ctx.set_seams(ff, ov)
                ctx.clear_row_seeds()
                got = ctx.sample_loop(x_T.clone(), idx, coefs, noise=None, seed=99, draw0=1).clone()
                fed = ctx.sample_loop(x_T.clone(), idx, coefs, noise=torch.stack([normals(n, 99, 1 + k).view(Bn, Tn, C) for k in range(2)])).clone()
                assert torch.equal(got, fed) and bool(torch.isfinite(got).all()), (mode, seam, 'call stream', float((got - fed).abs().max()))
                ctx.set_row_seeds(seeds)
                keyed = ctx.sample_loop(x_T.clone(), idx, coefs, noise=None, draw0=1).clone()
                fed = ctx.sample_loop(x_T.clone(), idx, coefs, noise=torch.stack([ctx.draw_rows(1 + k) for k in range(2)])).clone()
                assert torch.equal(keyed, fed) and bool(torch.isfinite(keyed).all()), (mode, seam, 'row keys', float((keyed - fed).abs().max()))
                assert not torch.equal(keyed, got)
                if seam:
                    flags = S.plan_flags(ff, Tn, ov)
                    assert S.seams_equal(got.cpu().numpy(), flags, ov) and S.seams_equal(keyed.cpu().numpy(), flags, ov)
                    ctx.clear_seams()
            # per-row schedules: row b at its own step and draw number
            st = [[3, 2, 1, 3][b] for b in range(Bn)]
            dr = [[1, 5, 2 ** 63 + 2, 9][b] for b in range(Bn)]
            cf = [d.step_coefs(s, mode, dims['scale'], eta) for s in st]
            rows_got = ctx.sample_rows(x_T.clone(), [st], [cf], draws=[dr]).clone()
            nz = torch.stack([normals(TC, seeds[b], dr[b]).view(Tn, C) for b in range(Bn)])
            rows_fed = ctx.sample_rows(x_T.clone(), [st], [cf], noise=nz[None]).clone()
            assert torch.equal(rows_got, rows_fed) and bool(torch.isfinite(rows_got).all()), (mode, 'rows', float((rows_got - rows_fed).abs().max()))
        torch.cuda.synchronize()
    finally:
        ctx.close()


# ---- 8. state rules -------------------------------------------------------------------------------
def test_capacity_factor_state_rules(natives):
    """cf < 0 -> MC_ERR_ARG (1); a denoiser call after the setting without a new condition fails as on a fresh context; with a captured
    graph the setting is MC_ERR_STATE (3); a positive factor is tutel's formula with it (a huge one drops nothing: every cap_w != 0)"""
    dims, _, nm = natives('C322_T24')
    lib, ptr, stream = _lib()
    x, xf, mask = synth_inputs(dims, B, T, seed=67, lengths=LENGTHS)
    d = _diffusion('ddim4')
    ctx = nm.context(B, T, max_steps=4)
    try:
        fresh = nm.context(B, T, max_steps=4)
        try:
            fresh.set_timesteps(d.timestep_map)
            with pytest.raises(RuntimeError) as e_fresh:
                fresh.denoise(x.cuda(), 0)
        finally:
            fresh.close()
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        for bad in (-1.0, -1e-3, float('nan')):
            assert lib.mc_ctx_set_capacity_factor(ctx.handle, bad) == 1
        assert ctx.capacity_factor == 1.5
        ctx.set_capacity_factor(16.0)
        with pytest.raises(RuntimeError) as e_set:
            ctx.denoise(x.cuda(), 0)
        assert str(e_set.value) == str(e_fresh.value)
        ctx.enable_capture()
        ctx.set_condition(xf.cuda(), mask.cuda())
        ctx.denoise(x.cuda(), 0)
        torch.cuda.synchronize()
        assert all(bool((ctx.buffer('cap_w', l) != 0).all()) for l in range(dims['NL']))
    finally:
        ctx.close()
    ctx = nm.context(B, T, max_steps=4)
    try:
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf.cuda(), mask.cuda())
        stream_ = torch.cuda.Stream()
        with torch.cuda.stream(stream_):
            xd, noise = x.cuda().clone(), torch.zeros(B, T, dims['input_feats'], device='cuda')
            ctx.graph_capture(xd, noise, [d.step_coefs(i, 'ddpm', dims['scale']) for i in range(4)])
            assert lib.mc_ctx_set_capacity_factor(ctx.handle, 0.0) == 3
            assert ctx.capacity_factor == 1.5
            ctx.set_row_seeds(SEEDS)                           # graph capture is unaffected by a seed table: replay reads the host-filled buffer
            noise.copy_(ctx.draw_rows(1))
            ctx.graph_step(3)
            stream_.synchronize()
            assert bool(torch.isfinite(xd).all())
            ctx.graph_release()
            assert lib.mc_ctx_set_capacity_factor(ctx.handle, 0.0) == 0
    finally:
        ctx.close()


# ---- 9. the batcher -------------------------------------------------------------------------------
def test_request_batcher_results_do_not_depend_on_the_submission_order(arch):
    """five requests through a B = 3 context, then the same five submitted in another order (other batchmates, other rows, another
    call holding the dummy row): every request's result is bit-equal across the two runs"""
    from motioncraft_amd.serve import Request, RequestBatcher
    sd, a = arch
    g = torch.Generator().manual_seed(75)
    reqs = []
    for i, n in enumerate((24, 17, 20, 9, 24)):
        xf = torch.nn.functional.layer_norm(torch.randn(SMALL['Nt'], SMALL['Dt'], generator=g), (SMALL['Dt'],))
        reqs.append(Request(length=n, seed=1000 + 7 * i, xf_out=xf))
    runs = []
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        bt = RequestBatcher(a, batch=B, frames=T, sampler='ddim', steps=4)
        handles = {i: bt.submit(reqs[i]) for i in order}
        out = bt.run()
        torch.cuda.synchronize()
        runs.append({i: out[handles[i]].clone() for i in order})
    for i, r in enumerate(reqs):
        assert tuple(runs[0][i].shape) == (r.length, SMALL['input_feats']) and bool(torch.isfinite(runs[0][i]).all())
        assert torch.equal(runs[0][i], runs[1][i]), (i, float((runs[0][i] - runs[1][i]).abs().max()))
    assert not torch.equal(runs[0][0][:9], runs[0][3][:9])

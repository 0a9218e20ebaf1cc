"""GPU (MI355X): early routing (option ``route_early``) -- in the two-stream schedule each sample group's experts start behind
the group's own gate, over a slot plan of ALL its (token, choice) pairs, and the whole-batch capacity cut (comb_w, the twin-split
flag) runs beside them -- against the joined routing (``route_early = 0``: both groups meet in front of the routing).

Every comparison is between two device paths of the same library and exact (torch.equal): a dropped pair's expert row is now
computed, but the projection behind the experts masks it by a select, so no bit of the result may change.

Shapes: the reduced config (L = 32) and the full width (L = 128) at B = 3 x 24 frames with mixed lengths, pushed into the
large-batch schedule (big_tokens = 0) and out of the one-workgroup routing kernels (MC_ROUTE_SMALL_CTX = 0).  B is odd, so the
twin layer's two sample sub-groups are unequal (1 and 2 samples).

Which layers run early: every layer of the two-stream schedule.  Base layer 0 under the stable tie order is the CFG-twin layer:
on the production path its first CFG half goes down the two streams as two sub-groups (two slot groups over N/2 source tokens);
under ``stop_after_layers`` (no aliasing) its one gate launch feeds one slot group and the second group is empty."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import FULL, SMALL, SMALL_SEED, skew_gates, synth_inputs

pytestmark = pytest.mark.gpu

B, T = 3, 24
LENGTHS = [24, 20, 7]
DEFAULT_CHAIN = 762806311                      # kChainDefault (mc_options.h)
DIMS = {'SMALL': SMALL, 'FULL': FULL}


@pytest.fixture(scope='module')
def models():
    """(dims name, gate kind, layers or None) -> (dims, NativeModel), each built once for the module."""
    from motioncraft_amd.engine import NativeModel
    from oracle import weights as W
    base, made = {}, {}

    def get(name, kind, layers=None):
        k = (name, kind, layers)
        if k not in made:
            dims = DIMS[name]
            if name not in base:
                base[name] = W.make_state_dict(dims, SMALL_SEED if name == 'SMALL' else 0)
            sd = skew_gates(base[name], dims, kind)
            if layers is not None:                      # the first `layers` base layers only
                dims = dict(dims, NL=layers)
                keep = tuple(f'temporal_decoder_blocks.{l}.' for l in range(layers))
                sd = {n: v for n, v in sd.items() if not n.startswith('temporal_decoder_blocks.') or n.startswith(keep)}
            made[k] = (dims, NativeModel(dims, sd, cfg_scale=dims['scale']))
        return made[k]
    yield get
    for _, nm in made.values():
        nm.close()


@pytest.fixture
def big_paths(monkeypatch):
    monkeypatch.setenv('MC_ROUTE_SMALL_CTX', '0')          # read when a context is created: no one-workgroup routing kernel


def _diffusion():
    from motioncraft_amd.diffusion import build_diffusion
    return build_diffusion(dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large'))


def _inputs(dims, seed=71):
    x, xf, mask = synth_inputs(dims, B, T, seed=seed, lengths=LENGTHS)
    eps = torch.randn(2, B, T, dims['input_feats'], generator=torch.Generator().manual_seed(seed + 1))
    return x, xf, mask, eps


def _context(nm, xf, mask, early, tie='stable', delay=0, max_steps=2, timesteps=None, chain=None):
    ctx = nm.context(B, T, max_steps=max_steps)
    ctx.set_option('big_tokens', 0)
    if chain is not None:
        ctx.set_option('chain', chain)
    ctx.set_option('route_early', early)
    if delay:
        ctx.set_option('dbg_delay_us', delay)
    if tie != 'stable':
        ctx.set_tie_policy(tie)
    ctx.set_timesteps(timesteps if timesteps is not None else _diffusion().timestep_map[-max_steps:])
    ctx.set_condition(xf.cuda(), mask.cuda())
    return ctx


def _two_steps(ctx, dims, x, eps):
    d = _diffusion()
    xd = x.cuda().clone()
    ctx.sample_loop(xd, [1, 0], [d.step_coefs(999, 'ddpm', dims['scale']), d.step_coefs(998, 'ddpm', dims['scale'])], noise=eps.cuda())
    torch.cuda.synchronize()
    return xd


def _routing_buffers(ctx):
    return {n: ctx.buffer(n, dtype=torch.int32 if n in ('idx', 'key') else torch.float32) for n in ('idx', 'gate', 'key', 'comb_w')}


@pytest.mark.parametrize('name', ['SMALL', 'FULL'])
@pytest.mark.parametrize('kind,tie', [('balanced', 'stable'), ('hot_pair', 'stable'), ('all_ties', 'stable'), ('all_ties', 'reverse')])
def test_early_routing_equals_joined_routing(models, big_paths, name, kind, tie):
    """Two sample_loop steps: x, idx, gate, key and comb_w of route_early = 1 equal those of route_early = 0 bit for bit.  hot_pair
    drops at least 15 % of the second choices and leaves an expert empty; all_ties sends every pair of a group to one expert (fourteen
    empty) and, under the stable order, cuts twin pairs apart, so layer 0 runs with the twin-split flag raised."""
    dims, nm = models(name, kind)
    x, xf, mask, eps = _inputs(dims)
    got = {}
    for early in (0, 1):
        ctx = _context(nm, xf, mask, early, tie)
        try:
            ctx.enable_capture()
            got[early] = (_two_steps(ctx, dims, x, eps), _routing_buffers(ctx), [ctx.routing(l) for l in range(dims['NL'])])
        finally:
            ctx.close()
    assert bool(torch.isfinite(got[1][0]).all())
    assert torch.equal(got[0][0], got[1][0]), float((got[0][0] - got[1][0]).abs().max())
    for n in ('idx', 'gate', 'key', 'comb_w'):
        assert torch.equal(got[0][1][n], got[1][1][n]), n
    E, N = dims['E'], 2 * B * T * dims['H']
    stats = []
    for (i0, k0), (i1, k1) in zip(got[0][2], got[1][2]):
        assert torch.equal(i0, i1) and torch.equal(k0, k1)
        kept = np.bincount(i1[k1].numpy(), minlength=E)
        stats.append((float((~k1[:, 0]).float().mean()), float((~k1[:, 1]).float().mean()), int((kept == 0).sum())))
    print(f'{name} {kind} {tie}: per layer (dropped 1st, dropped 2nd, empty experts) {stats}')
    if kind == 'hot_pair':
        assert all(s[1] >= 0.15 and s[2] >= 1 for s in stats), stats
    if kind == 'all_ties':
        assert all(s[2] == E - 2 for s in stats), stats
        i1, k1 = got[1][2][0]
        assert bool((i1[:, 0] == i1[0, 0]).all()) and bool((i1[:, 1] == i1[0, 1]).all())
        if tie == 'stable':                             # the cut falls inside the first CFG half: twins kept, originals too, later twins not
            assert bool((k1[:N // 2] != k1[N // 2:]).any())


def _check_slot_map(ctx, dims, nsrc, gsplit, what):
    idx = ctx.buffer('idx', dtype=torch.int32)[:2 * nsrc].cpu().numpy()
    dst = ctx.buffer('dst_row', dtype=torch.int32).cpu().numpy()
    src = ctx.buffer('src_row', dtype=torch.int32).cpu().numpy()
    tg, tr0, tn = (ctx.buffer(n, dtype=torch.int32).cpu().numpy() for n in ('tile_group', 'tile_row0', 'tile_nrows'))
    nt = ctx.buffer('num_tiles', dtype=torch.int32).cpu().numpy()
    max_tiles = tg.shape[0] // 2
    for g, (t0, t1) in enumerate(((0, gsplit), (gsplit, nsrc))):
        lo, hi = 2 * t0, 2 * t1
        d = dst[lo:hi]
        assert np.array_equal(np.sort(d), np.arange(lo, hi)), (what, g, 'every pair of the group exactly once, inside its own range')
        assert np.array_equal(src[lo:hi], d >> 1), (what, g)
        n = int(nt[g])
        assert 0 <= n <= max_tiles, (what, g, n)
        sl = slice(g * max_tiles, g * max_tiles + n)
        assert int(tn[sl].sum()) == hi - lo, (what, g, int(tn[sl].sum()), hi - lo)
        if n:
            assert int(tr0[g * max_tiles]) == lo, (what, g, int(tr0[g * max_tiles]), lo)      # group 1's first slot is 2 gsplit
        expert_of_slot = np.full(hi - lo, -1, dtype=np.int64)
        for e, r0, nr in zip(tg[sl], tr0[sl], tn[sl]):
            assert 1 <= nr <= 128 and lo <= r0 and r0 + nr <= hi, (what, g, int(r0), int(nr))
            assert (expert_of_slot[r0 - lo:r0 - lo + nr] == -1).all(), (what, g, 'tiles overlap')
            expert_of_slot[r0 - lo:r0 - lo + nr] = e
        assert np.array_equal(expert_of_slot, idx[d]), (what, g, 'the tile that holds a pair belongs to idx[token][choice]')


@pytest.mark.parametrize('name', ['SMALL', 'FULL'])
@pytest.mark.parametrize('kind,tie', [('hot_pair', 'stable'), ('all_ties', 'stable'), ('all_ties', 'reverse')])
def test_slot_map_invariants(models, big_paths, name, kind, tie):
    """After denoise(stop_after_layers = l + 1) the slot map of layer l holds every (token, choice) of a group's source tokens exactly
    once inside the group's own slot range, in a tile of its expert; tile_nrows sums to twice the group's tokens; group 1 starts at
    2 gsplit.  (Layer 0, stable order, stop_after_layers: the twin layer's one gate launch -- one group over the first CFG half, the
    second one empty.)  The twin layer's two SUB-groups exist on the production path only (aliasing on): a one-layer model, full call."""
    dims, nm = models(name, kind)
    x, xf, mask, _ = _inputs(dims)
    H, N = dims['H'], 2 * B * T * dims['H']
    ctx = _context(nm, xf, mask, 1, tie, max_steps=1, timesteps=[640])
    try:
        for l in range(dims['NL']):
            ctx.denoise(x.cuda(), 0, stop_after_layers=l + 1)
            torch.cuda.synchronize()
            twin = l == 0 and tie == 'stable'
            _check_slot_map(ctx, dims, N // 2 if twin else N, N // 2, f'{name} {kind} {tie} layer {l}')
    finally:
        ctx.close()
    if tie != 'stable':
        return
    dims1, nm1 = models(name, kind, 1)
    ctx = _context(nm1, xf, mask, 1, tie, max_steps=1, timesteps=[640])
    try:
        out = ctx.denoise(x.cuda(), 0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        _check_slot_map(ctx, dims1, N // 2, (B // 2) * T * H, f'{name} {kind} twin sub-groups')
        if kind == 'all_ties':
            assert int(ctx.buffer('route_split', dtype=torch.int32)[0]) == 1
    finally:
        ctx.close()


@pytest.mark.parametrize('name', ['SMALL', 'FULL'])
def test_graph_replay_equals_eager(models, big_paths, name):
    """A replayed step (hipGraph capture of the early schedule: the same events, fills and selection) equals the eager step."""
    dims, nm = models(name, 'hot_pair')
    x, xf, mask, eps = _inputs(dims)
    d = _diffusion()
    coefs = [d.step_coefs(998, 'ddpm', dims['scale']), d.step_coefs(999, 'ddpm', dims['scale'])]
    got = {}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for arm in ('eager', 'graph'):
            ctx = _context(nm, xf, mask, 1)
            try:
                xd, noise = x.cuda().clone(), torch.empty(B, T, dims['input_feats'], device='cuda')
                if arm == 'graph':
                    ctx.graph_capture(xd, noise, coefs)
                    xd.copy_(x)
                for n, i in enumerate((1, 0)):
                    noise.copy_(eps[n])
                    if arm == 'graph':
                        ctx.graph_step(i)
                    else:
                        ctx.sample_step(xd, i, coefs[i], noise, x_prev=xd)
                    stream.synchronize()
                got[arm] = xd.clone()
                if arm == 'graph':
                    ctx.graph_release()
            finally:
                ctx.close()
    assert bool(torch.isfinite(got['eager']).all())
    assert torch.equal(got['eager'], got['graph']), float((got['eager'] - got['graph']).abs().max())


_undelayed = {}          # (name, early, chain) -> (x, routing buffers) of the run without a delay, computed once per module


def _late_run(models, name, early, chain, delay):
    dims, nm = models(name, 'hot_pair')
    x, xf, mask, eps = _inputs(dims)
    key = (name, early, chain)
    if delay == 0 and key in _undelayed:
        return _undelayed[key]
    ctx = _context(nm, xf, mask, early, delay=delay, chain=chain)
    try:
        got = (_two_steps(ctx, dims, x, eps), _routing_buffers(ctx))
    finally:
        ctx.close()
    if delay == 0:
        _undelayed[key] = got
    return got


@pytest.mark.parametrize('name', ['SMALL', 'FULL'])
@pytest.mark.parametrize('chain', [DEFAULT_CHAIN, DEFAULT_CHAIN & ~(1 << 16)], ids=['default', 'no_twin_split'])
@pytest.mark.parametrize('early', [1, 0])
def test_late_streams_do_not_change_the_result(models, big_paths, name, chain, early):
    """dbg_delay_us holds the second (+300) or the first (-300) group's stream in front of every layer tail, so that group reaches the
    next layer's gate late: the selection (early) or the join in front of the routing (route_early = 0) must wait for the late gate,
    the late group's projection for the selection and -- in the joined form and the unsplit twin layer (chain bit 16 cleared) -- for
    the expert rows launched behind the routing.  Within each (early, chain) pair x and comb_w of the delayed runs equal the undelayed
    run bit for bit, and the undelayed x of every pair equals that of (early, default)."""
    base = _late_run(models, name, early, chain, 0)
    assert bool(torch.isfinite(base[0]).all())
    for delay in (300, -300):
        got = _late_run(models, name, early, chain, delay)
        assert torch.equal(base[0], got[0]), (delay, float((base[0] - got[0]).abs().max()))
        assert torch.equal(base[1]['comb_w'], got[1]['comb_w']), delay
    ref = _late_run(models, name, 1, DEFAULT_CHAIN, 0)
    assert torch.equal(ref[0], base[0]), float((ref[0] - base[0]).abs().max())


def _ledger(lib, fn):
    lib.mc_debug_flop_ledger(1)
    try:
        fn()
        torch.cuda.synchronize()
        n = lib.mc_debug_flop_ledger_dump(None, 0)
        buf = ctypes.create_string_buffer(n)
        lib.mc_debug_flop_ledger_dump(buf, n)
    finally:
        lib.mc_debug_flop_ledger(0)
    return buf.value.decode()


def test_option_values_and_one_stream_ledger(models, monkeypatch):
    """route_early takes 0 or 1 (anything else: MC_ERR_ARG = code 1, the message names the range); an invalid MC_ROUTE_EARLY fails
    context creation naming the variable; at a one-stream size the option is inert: the same launches under 0 and 1."""
    dims, nm = models('SMALL', 'balanced')
    x, xf, mask, eps = _inputs(dims)
    ctx = nm.context(B, T, max_steps=2)
    try:
        for bad in (2, -1, 7):
            with pytest.raises(RuntimeError, match=r'\(code 1\): route_early: 0 or 1'):
                ctx.set_option('route_early', bad)
        ctx.set_timesteps(_diffusion().timestep_map[-2:])
        ctx.set_condition(xf.cuda(), mask.cuda())
        led, outs = {}, {}
        for early in (0, 1):
            ctx.set_option('route_early', early)
            _two_steps(ctx, dims, x, eps)                # (first use of a setting: side-stream probe and the like are behind us)
            led[early] = _ledger(ctx.lib, lambda: outs.__setitem__(early, _two_steps(ctx, dims, x, eps)))
        assert led[0] == led[1] and len(led[0].splitlines()) > 5
        assert torch.equal(outs[0], outs[1])
    finally:
        ctx.close()
    monkeypatch.setenv('MC_ROUTE_EARLY', '2')
    with pytest.raises(RuntimeError, match='MC_ROUTE_EARLY=2'):
        nm.context(B, T, max_steps=1)
    monkeypatch.setenv('MC_ROUTE_EARLY', '0')
    nm.context(B, T, max_steps=1).close()

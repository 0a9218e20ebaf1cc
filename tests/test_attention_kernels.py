"""GPU (MI355X): the MC-Attn cores against fp64 at op level, on inputs the test controls.

``mc_op_body_attention`` (body_reg_k<HD, H>) and ``mc_op_temporal_attention`` (temporal_k<L, LSPLIT, PAIR>, temporal_h_k<L, SPLIT>,
the form named explicitly) against ``attention_ref.py``; the body phase of pqbody_k / pqbody_h_k and the temporal kernel of the
default chain through a context, on the context's own mf / tf.  Inputs, cases and bounds live in ``attention_ref.py`` (the
derivation is in its docstring); ``tests/test_attention_ref_host.py`` shows on the CPU that every case sees a subtly wrong
evaluation at 10x its bound and that an fp32 evaluation of the formula stays inside it.  Every output buffer is pre-filled with
777.0 and carries guard rows: rows outside the launched range and the guard rows must stay untouched, everything written must be
finite.  Each case checks through the FLOP ledger that exactly the kernel forms it asked for were launched.

Every test prints error / bound per form and case.  Measured (MI355X), largest ratio over all cases: temporal whole 0.012 (L = 32),
0.010 (64), 0.012 (128); LSPLIT 0.007 / 0.010; PAIR 0.009; f16x3 0.010 / 0.013; f16 0.14 / 0.21; body 0.006 / 0.004 / 0.003
(L = 32 / 64 / 128); through a context (L = 64 / 128): y_s 0.0006 / 0.0003 (f32), 0.0008 / 0.0004 (f16x3), 0.050 / 0.026 (f16), y_t 0.003.
"""
import ctypes

import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu

GUARD = 3
TCASES = R.temporal_cases()
BCASES = R.body_cases()


def _lib():
    from motioncraft_amd import lib as L_
    return L_, L_.load(require_gpu=True)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ledger_keys(lib):
    n = lib.mc_debug_flop_ledger_dump(None, 0)
    buf = ctypes.create_string_buffer(int(n))
    lib.mc_debug_flop_ledger_dump(buf, n)
    return sorted(l.split('\t')[0] for l in buf.value.decode().splitlines() if l)


def _temporal_key(form, L, H, nb):
    NT = L // 32
    if form == 'whole':
        return f'temporal_k<{L}@{nb * H * 256}'
    if form == 'lsplit':
        return f'temporal_k<{L}@{nb * H * NT * (2 if nb * H * NT * 2 <= 256 else 1) * 256}'
    if form == 'pair':
        return f'temporal_k<{L}@{nb * (H // 2) * 256}'
    return f'temporal_h_k<{L}, {"true" if form == "f16x3" else "false"}>@{nb * H * 256}'


class Temporal:
    """Device copies of one case and its launches."""

    def __init__(self, c, poison_twins=False):
        self.c = c
        self.L_, self.lib = _lib()
        self.cpu = R.temporal_inputs(c)
        mf, tf, mask = self.cpu
        if poison_twins:
            mf = mf.clone()
            mf[mf.shape[0] // 2:] = float('nan')
        self.dev = (mf.cuda(), tf.cuda(), mask.cuda())
        self.dims = (c['B'], c['T'], c['Nt'], c['H'], c['L'])

    def bound(self, form):
        B, T, Nt, H, L = self.dims
        return R.temporal_bound(form, *self.cpu, B, T, Nt, H, L)

    def ref(self, alias=False):
        B, T, Nt, H, L = self.dims
        return R.temporal_ref(*self.cpu, B, T, Nt, H, L, alias=alias)

    def run(self, form, skip=1, b0=0, nb=None, flag=None):
        """yt [2B*T][H*L] of one launch (fp64 on the host); rows outside [b0, b0 + nb) and the guard rows are checked here."""
        B, T, Nt, H, L = self.dims
        nb = 2 * B if nb is None else nb
        yt = torch.full((2 * B * T + GUARD, H * L), R.SENTINEL, device='cuda')
        fl = None if flag is None else torch.tensor([flag], dtype=torch.int32, device='cuda')
        mf, tf, mask = self.dev
        self.L_.check(self.lib.mc_op_temporal_attention(_ptr(mf), _ptr(tf), _ptr(mask), _ptr(yt), b0, nb, B, T, Nt, H, L,
                                                        self.L_.TEMPORAL_FORMS[form], skip, _ptr(fl), _stream()), form)
        torch.cuda.synchronize()
        out = yt.cpu()
        lo, hi = b0 * T, (b0 + nb) * T
        assert bool((out[:lo] == R.SENTINEL).all()) and bool((out[hi:] == R.SENTINEL).all()), (form, 'rows outside the launch were written')
        assert bool(torch.isfinite(out[lo:hi]).all()), (form, 'not finite')
        return out[:2 * B * T].double()


def _ratio(got, ref, bound, rows=slice(None)):
    return float((got[rows] - ref[rows]).abs().max()) / bound


@pytest.mark.parametrize('c', TCASES, ids=R.case_id)
def test_temporal_attention_every_form_vs_fp64(c):
    """All forms that exist for the shape, whole batch: error <= bound; skip_text on / off bit-identical; two runs bit-identical; a
    fully masked sample's unconditioned half exactly 0; the step's own choice inside the fp32 bound; the ledger names the forms."""
    tc = Temporal(c)
    B, T, Nt, H, L = tc.dims
    ref = tc.ref()
    forms = R.forms_of(L, H)
    tc.lib.mc_debug_flop_ledger(1)
    try:
        got = {f: [tc.run(f, skip=1), tc.run(f, skip=1), tc.run(f, skip=0)] for f in forms}
        keys = _ledger_keys(tc.lib)
        step = tc.run('step')
    finally:
        tc.lib.mc_debug_flop_ledger(0)
    assert keys == sorted({_temporal_key(f, L, H, 2 * B) for f in forms}), keys
    for f in forms:
        a, a2, ns = got[f]
        r = _ratio(a, ref, tc.bound(f))
        print(f'temporal {f} {R.case_id(c)}: error / bound {r:.4f}')
        assert r <= 1.0, (f, r)
        assert torch.equal(a, a2), (f, 'two runs differ')
        assert torch.equal(a, ns), (f, 'skip_text changes bits')
        if c['mask'] == 'one_masked':
            assert not bool(a.reshape(2 * B, T, -1)[2 * B - 1].any()), (f, 'fully masked unconditioned sample is not exactly 0')
    assert _ratio(step, ref, tc.bound('step')) <= 1.0


def _case_at(L, H, T=33):
    return next(c for c in TCASES if (c['L'], c['H'], c['T'], c['B']) == (L, H, T, 2))


@pytest.mark.parametrize('L,H', [(L, H) for L in (32, 64, 128) for H in (8, 12)])
def test_temporal_attention_twin_aliasing_and_sample_sub_ranges(L, H):
    """Flag 0: the samples b >= B read sample b - B's motion rows (their own hold NaN).  Flag 1: their own.  A launch of samples
    [1, 3) of 4 crosses the conditioned / unconditioned boundary and writes exactly those rows."""
    c = _case_at(L, H)
    B, T = c['B'], c['T']
    poisoned, plain = Temporal(c, poison_twins=True), Temporal(c)
    ref_alias, ref = plain.ref(alias=True), plain.ref()
    for f in R.forms_of(L, H):
        b = plain.bound(f)
        for skip in (0, 1):
            ra = _ratio(poisoned.run(f, skip=skip, flag=0), ref_alias, b)
            ro = _ratio(plain.run(f, skip=skip, flag=1), ref, b)
            rows = slice(T, 3 * T)
            rs = _ratio(plain.run(f, skip=skip, b0=1, nb=2), ref, b, rows)
            rsa = _ratio(poisoned.run(f, skip=skip, b0=1, nb=2, flag=0), ref_alias, b, rows)
            print(f'temporal {f} L{L}-H{H} skip {skip}: error / bound aliased {ra:.4f}, own rows {ro:.4f}, samples [1, 3) {rs:.4f}, aliased {rsa:.4f}')
            assert max(ra, ro, rs, rsa) <= 1.0, (f, skip, ra, ro, rs, rsa)


def test_temporal_attention_refuses_forms_that_do_not_exist():
    L_, lib = _lib()
    buf = torch.zeros(1 << 16, device='cuda')
    for form, name, L, H in (('lsplit', 'LSPLIT', 32, 8), ('pair', 'PAIR', 32, 8), ('pair', 'PAIR', 128, 12), ('pair', 'PAIR', 64, 7),
                             ('f16x3', 'F16X3', 32, 12), ('f16', 'F16', 32, 8)):
        rc = lib.mc_op_temporal_attention(_ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf), 0, 2, 1, 2, 2, H, L, L_.TEMPORAL_FORMS[form], 1, None, _stream())
        assert rc != 0 and name in L_.last_error(), (form, L, H, rc, L_.last_error())
    assert lib.mc_op_temporal_attention(_ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf), 0, 2, 1, 2, 2, 8, 64, 9, 1, None, _stream()) != 0
    torch.cuda.synchronize()
    assert not bool(buf.any())


def _run_body(c, mf, qkv, wsm, frames, frame0=0, twin_from=0, flag=None, row0=0):
    """ys [frames][H*L] of one launch over the frames [row0, row0 + frames) of the case's buffers."""
    L_, lib = _lib()
    L, H = c['L'], c['H']
    ys = torch.full((frames + GUARD, H * L), R.SENTINEL, device='cuda')
    fl = None if flag is None else torch.tensor([flag], dtype=torch.int32, device='cuda')
    dmf, dq, dw = mf[row0 * H:].contiguous().cuda(), qkv[row0 * H:].contiguous().cuda(), wsm.cuda()
    L_.check(lib.mc_op_body_attention(_ptr(dmf), mf.shape[1], _ptr(dq), _ptr(dw), _ptr(ys), frames, H, L, twin_from, _ptr(fl), frame0, _stream()))
    torch.cuda.synchronize()
    out = ys.cpu()
    assert bool((out[frames:] == R.SENTINEL).all()), 'guard rows written'
    return out[:frames].double()


@pytest.mark.parametrize('c', BCASES, ids=R.body_case_id)
def test_body_attention_vs_fp64(c):
    """body_reg_k<L / 8, H> at partial waves and workgroups, ldmf = 4 L and a wider one (pad columns NaN)."""
    L, H, F = c['L'], c['H'], c['frames']
    _, lib = _lib()
    lib.mc_debug_flop_ledger(1)
    try:
        for pad in (0, 8):
            mf, qkv, wsm = R.body_inputs(c, pad)
            ref = R.body_ref(mf, qkv, wsm, H, L)
            got = _run_body(c, mf, qkv, wsm, F)
            assert bool(torch.isfinite(got).all())
            r = float((got - ref).abs().max()) / R.body_bound(mf, qkv, H, L)
            print(f'body {R.body_case_id(c)} ldmf {4 * L + pad}: error / bound {r:.4f}')
            assert r <= 1.0
            assert torch.equal(got, _run_body(c, mf, qkv, wsm, F))
        keys = _ledger_keys(lib)
    finally:
        lib.mc_debug_flop_ledger(0)
    waves = (F * 8 * (L // 8) + 63) // 64
    assert keys == [f'body_reg_k@{(waves + 3) // 4 * 256}'], keys


@pytest.mark.parametrize('L,H', [(L, H) for L in (32, 64, 128) for H in (8, 12)])
def test_body_attention_twin_aliasing(L, H):
    """A launch of frames [13, 100) with twin_from = 60: with the flag at 0 the frames >= 60 keep the sentinel, the rest match; with
    the flag at 1 all frames match."""
    c = next(c for c in BCASES if (c['L'], c['H'], c['frames'], c['kind']) == (L, H, 100, 'normal'))
    mf, qkv, wsm = R.body_inputs(c)
    ref = R.body_ref(mf, qkv, wsm, H, L)[13:]
    bound = R.body_bound(mf, qkv, H, L)
    got = _run_body(c, mf, qkv, wsm, 87, frame0=13, twin_from=60, flag=0, row0=13)
    assert bool((got[47:] == R.SENTINEL).all()), 'aliased frames were produced'
    r0 = float((got[:47] - ref[:47]).abs().max()) / bound
    got1 = _run_body(c, mf, qkv, wsm, 87, frame0=13, twin_from=60, flag=1, row0=13)
    r1 = float((got1 - ref).abs().max()) / bound
    print(f'body L{L}-H{H} aliasing: error / bound flag 0 {r0:.4f}, flag 1 {r1:.4f}')
    assert bool(torch.isfinite(got1).all()) and max(r0, r1) <= 1.0
    assert torch.equal(got[:47], got1[:47])


@pytest.mark.parametrize('L', [64, 128])
def test_fused_body_phase_and_chain_temporal_kernel_vs_fp64(L):
    """pqbody_k / pqbody_h_k never write q/k/v: they are recomputed in fp64 from the context's own mf (LayerNorm + Linear of the state
    dict's body_d_attn), then body_ref / temporal_ref on the context's mf and tf against its ys and yt, on the rows the schedule
    produces: after layer 1 (no aliasing) and after layer 0 alone (twin aliasing: the second half of mf / ys is not produced; the
    routing of these inputs splits no twin pair, which is asserted).  f32, f16x3 and f16 contexts at small default dims, B = 3,
    T = 24, ragged lengths, big_tokens = 0; at this batch the chain launches the column-sliced fp32 temporal kernel in all three
    (asserted), so y_t is held to the fp32 bound.  The host tests judge these bounds on the oracle's capture of the same case."""
    from motioncraft_amd.engine import NativeModel
    dims, sd, x, xf, mask, B, T = R.fused_case(L)
    H, Nt = dims['H'], dims['Nt']
    nm = NativeModel(dims, sd, cfg_scale=dims['scale'])
    _, lib = _lib()

    def run(ctx, prec, layers):
        lib.mc_debug_flop_ledger(1)
        try:
            ctx.denoise(x.cuda(), 0, stop_after_layers=layers)
            torch.cuda.synchronize()
            keys = _ledger_keys(lib)
        finally:
            lib.mc_debug_flop_ledger(0)
        fused = 'pqbody_k<' if prec == 'f32' else f'pqbody_h_k<{L}, 12, {"true" if prec == "f16x3" else "false"}>'
        assert any(k.startswith(fused) for k in keys) and not any(k.startswith('body_reg_k') for k in keys), keys
        tkeys = [k for k in keys if k.startswith('temporal')]
        assert tkeys and all(k.startswith(f'temporal_k<{L}@') for k in tkeys), keys
        return tkeys

    def check(ctx, prec, layer, aliased, tkeys):
        mf = ctx.buffer('mf').cpu().reshape(2 * B * T * H, 4 * L)
        tf = ctx.buffer('tf', layer=layer).cpu().reshape(2 * B, Nt, 2 * L)
        ys, yt = (ctx.buffer(n).cpu().reshape(2 * B * T, H * L).double() for n in ('ys', 'yt'))
        g, b, Wq, bq, wsm = R.body_weights(sd, layer)
        rows = B * T if aliased else 2 * B * T
        qkv, d = R.qkv_from_mf(mf[:rows * H], g, b, Wq, bq, L, prec)
        bound = R.body_bound(mf[:rows * H], qkv, H, L, R.qkv_error_term(qkv, d, H, L))
        rs = float(((ys[:rows] - R.body_ref(mf[:rows * H], qkv, wsm, H, L)).abs() / bound).max())
        rt = float((yt - R.temporal_ref(mf, tf, mask, B, T, Nt, H, L, alias=aliased)).abs().max()) / R.temporal_bound('f32', mf, tf, mask, B, T, Nt, H, L)
        print(f'fused L{L} {prec} layer {layer} (aliased {aliased}, {", ".join(tkeys)}): error / bound ys {rs:.4f}, yt {rt:.4f}')
        assert bool(torch.isfinite(ys[:rows]).all()) and bool(torch.isfinite(yt).all()) and rs <= 1.0 and rt <= 1.0

    for prec in ('f32', 'f16x3', 'f16'):
        ctx = nm.context(B, T, max_steps=1)
        ctx.set_option('big_tokens', 0)
        if prec != 'f32':
            ctx.set_option('half_min_rows', 0)
            ctx.set_precision(prec)
        ctx.set_timesteps([700])
        ctx.set_condition(xf.cuda(), mask.cuda())
        check(ctx, prec, 1, False, run(ctx, prec, 2))
        tkeys = run(ctx, prec, 1)
        assert int(ctx.buffer('route_split', dtype=torch.int32).cpu()[0]) == 0, 'the routing split a twin pair: layer 0 ran unaliased'
        check(ctx, prec, 0, True, tkeys)
        ctx.close()
    nm.close()

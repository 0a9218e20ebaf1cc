"""GPU (MI355X): the kernels of the four step-invariant encoders against fp64 at op level, on inputs the test controls.

``mc_op_enc_ln`` (ln_wide_k), ``mc_op_enc_embed_tokens`` (embed_tokens_k), ``mc_op_enc_attention`` (mha_small_k / mha_masked_k, the
form named explicitly), ``mc_op_bigru_steps`` (the grouped recurrence GEMM + gru_gate_k), ``mc_op_conv1d_k4s2`` (pad_time_k, the window
GEMM, lrelu_k) and ``mc_op_gemm_strided`` (gemm_k<0>, gemm_k<4>, gemm_wp_k behind mc_launch_gemm's strided forms) against
``encoder_ref.py``.  Cases, inputs and bounds live there (the derivation is in its docstring); ``tests/test_encoder_ref_host.py``
shows on the CPU that an fp32 evaluation of each formula stays inside its bound on every case and that every subtly wrong
evaluation is seen at 10x the bound by some case.  Every output buffer is pre-filled with 777.0 and carries guard rows that must
stay untouched; everything inside the launched range must be written and finite; every float input is followed by NaN, and holds
NaN wherever its contract says "never read".  All elements of every case are compared; rows defined to be 0 and elements the
launch must not write are compared exactly.  The FLOP ledger names the kernel that ran.

Every test prints error / bound per case.  Measured (MI355X), largest ratio over all cases: ln_wide_k 0.16 (L = 4), 0.25 (64), 0.54
(256), 0.41 (260), 0.93 (768: an element with gamma near 0, where the bound is little more than the rounding of the last addition),
0.60 (4096); mha_small_k 0.004 (moderate scale), 0.003 (large); mha_masked_k 0.004 / 0.004; the GRU step 0.048; the convolution 0.052;
strided gemm_k<0> 0.037, gemm_k<4> 0.13, gemm_wp_k 0.011.  The embedding is exact.
"""
import ctypes

import pytest
import torch

import encoder_ref as R

pytestmark = pytest.mark.gpu

GUARD = 3
MOAT = 64
MC_ERR_ARG = 1
F32 = torch.float32


def _lib():
    from motioncraft_amd import lib as L_
    return L_, L_.load(require_gpu=True)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    """a device copy of a float tensor with NaN behind it (a read past the end shows in the result); None stays None"""
    if t is None:
        return None
    buf = torch.full((t.numel() + MOAT,), R.NAN, device='cuda')
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf


def _out(rows, width):
    return torch.full((rows + GUARD, width), R.SENTINEL, device='cuda')


def _take(buf, rows, what):
    """rows of an output buffer on the host: written and finite; the guard rows behind them untouched"""
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[rows:] == R.SENTINEL).all()), (what, 'guard rows were written')
    assert bool(torch.isfinite(out[:rows]).all()), (what, 'not finite')
    return out[:rows]


def _ledger(lib, fn):
    """kernel names (without the grid) booked while fn runs"""
    lib.mc_debug_flop_ledger(1)
    try:
        fn()
        n = lib.mc_debug_flop_ledger_dump(None, 0)
        buf = ctypes.create_string_buffer(int(n))
        lib.mc_debug_flop_ledger_dump(buf, n)
    finally:
        lib.mc_debug_flop_ledger(0)
    return sorted(l.split('\t')[0] for l in buf.value.decode().splitlines() if l)


def _show(kernel, what, r):
    print(f'RATIO {kernel} {what}: error / bound = {r:.4f}')


# -------------------------------------------------------------------------------------------------------------------------
# ln_wide_k, embed_tokens_k
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.ln_cases(), ids=lambda c: f"rows{c['rows']}-L{c['L']}-eps{c['eps']}-relu{c['relu']}")
def test_enc_ln_vs_fp64(c):
    L_, lib = _lib()
    rows, L, eps, relu = c['rows'], c['L'], c['eps'], c['relu']
    x, g, b = R.ln_inputs(c)
    xd, gd, bd = _dev(x), _dev(g), _dev(b)
    y = _out(rows, L)
    L_.check(lib.mc_op_enc_ln(_ptr(xd), _ptr(gd), _ptr(bd), _ptr(y), rows, L, eps, relu, _stream()), 'enc_ln')
    got = _take(y, rows, c)
    ref = R.ln_ref(x, g, b, eps, relu)
    r = R.ratio(got, ref, R.ln_bound(x, g, b, eps))
    _show('ln_wide_k', c, r)
    assert r <= 1.0
    for i in range(rows):
        if R.LN_KINDS[i] == 'const':         # a constant row gives beta itself
            assert torch.equal(got[i], b.relu() if relu else b), 'constant row'
    z = _out(rows, L)                        # in place: X == Y
    z[:rows] = x.cuda()
    L_.check(lib.mc_op_enc_ln(_ptr(z), _ptr(gd), _ptr(bd), _ptr(z), rows, L, eps, relu, _stream()), 'enc_ln in place')
    assert torch.equal(_take(z, rows, c), got), 'in place differs from out of place'


@pytest.mark.parametrize('c', R.embed_cases(), ids=lambda c: f"B{c['B']}S{c['S']}d{c['d']}")
def test_enc_embed_tokens_is_the_fp32_sum(c):
    """ids outside [0, vocab) are clamped: the defined behaviour"""
    L_, lib = _lib()
    rows, S, d = c['B'] * c['S'], c['S'], c['d']
    ids, emb, pos = R.embed_inputs(c)
    assert int(ids.min()) < 0 and int(ids.max()) >= R.EMBED_VOCAB and (rows * d // 4) % 256 != 0 and 256 % S != 0
    x = _out(rows, d)
    idd, ed, pd = ids.cuda(), _dev(emb), _dev(pos)
    L_.check(lib.mc_op_enc_embed_tokens(_ptr(idd), _ptr(ed), _ptr(pd), _ptr(x), rows, S, d, R.EMBED_VOCAB, _stream()), 'enc_embed_tokens')
    assert torch.equal(_take(x, rows, c), R.embed_ref(ids, emb, pos, S, dtype=F32))


# -------------------------------------------------------------------------------------------------------------------------
# mha_small_k, mha_masked_k
# -------------------------------------------------------------------------------------------------------------------------
class Attention:
    def __init__(self, c):
        self.c = c
        self.L_, self.lib = _lib()
        self.B, self.S, self.heads = c['B'], c['S'], c['heads']
        self.d = self.heads * R.HD
        self.qkv, self.valid = R.attention_inputs(c), R.attention_mask(c)
        self.qkv_dev = _dev(self.qkv)
        self.valid_dev = None if self.valid is None else self.valid.cuda()
        self.ref = R.attention_ref(self.qkv, self.valid, self.B, self.S, self.d, self.heads, c['causal'])
        self.bound = R.attention_bound(self.qkv, self.B, self.S, self.d, self.heads)
        self.zero = R.attention_zero_rows(self.valid, self.B, self.S, c['causal'])

    def key(self, form):
        if form == 'small':
            return f'mha_small_k@{self.B * self.heads * 256}'
        return f'mha_masked_k@{self.B * self.heads * ((self.S + 15) // 16) * 256}'

    def run(self, form, masked=True):
        rows = self.B * self.S
        out = _out(rows, self.d)
        valid = self.valid_dev if masked else None
        keys = _ledger(self.lib, lambda: self.L_.check(self.lib.mc_op_enc_attention(
            _ptr(self.qkv_dev), _ptr(valid), _ptr(out), self.B, self.S, self.d, self.heads, self.c['causal'],
            self.L_.ENC_ATTN_FORMS[form], _stream()), form))
        return _take(out, rows, (self.c, form)), keys

    def check(self, got, kernel):
        assert bool((got[self.zero] == 0).all()), 'a query with no usable key must give an exactly zero row'
        bound = torch.full((self.B * self.S, 1), self.bound, dtype=torch.float64)
        bound[self.zero] = 0
        r = R.ratio(got, self.ref, bound)
        _show(kernel, R.attention_case_id(self.c), r)
        assert r <= 1.0


@pytest.mark.parametrize('c', R.attention_small_cases(), ids=R.attention_case_id)
def test_enc_attention_small_form_vs_fp64(c):
    """SMALL inside its bound, twice the same bits; STREAM on the same input inside its own and so within the sum of both of SMALL;
    LAYER is SMALL bit for bit (no key mask, S <= 128)"""
    a = Attention(c)
    small, k1 = a.run('small')
    again, _ = a.run('small')
    stream, k2 = a.run('stream')
    layer, k3 = a.run('layer')
    assert k1 == [a.key('small')] and k2 == [a.key('stream')] and k3 == [a.key('small')], (k1, k2, k3)
    a.check(small, 'mha_small_k')
    a.check(stream, 'mha_masked_k')
    assert torch.equal(small, again) and torch.equal(layer, small)
    assert float((small.double() - stream.double()).abs().max()) <= 2 * a.bound


@pytest.mark.parametrize('c', R.attention_stream_cases(), ids=R.attention_case_id)
def test_enc_attention_stream_form_vs_fp64(c):
    """STREAM inside its bound, twice the same bits; LAYER is the form the layer's rule names, bit for bit"""
    a = Attention(c)
    stream, k1 = a.run('stream')
    again, _ = a.run('stream')
    layer, k3 = a.run('layer')
    assert k1 == [a.key('stream')], k1
    a.check(stream, 'mha_masked_k')
    assert torch.equal(stream, again)
    if a.valid is None and a.S <= 128:
        small, _ = a.run('small')
        assert k3 == [a.key('small')] and torch.equal(layer, small), k3
        assert float((small.double() - stream.double()).abs().max()) <= 2 * a.bound
    else:
        assert k3 == [a.key('stream')] and torch.equal(layer, stream), k3


def test_enc_attention_refuses_a_form_that_does_not_exist():
    """MC_ERR_ARG, nothing launched, nothing written"""
    L_, lib = _lib()
    for c, form, masked in ((dict(form='stream', B=3, heads=2, S=17, causal=0, mask='prefix', scale='moderate'), 1, True),
                            (dict(form='stream', B=3, heads=2, S=129, causal=0, mask='none', scale='moderate'), 1, False),
                            (dict(form='stream', B=3, heads=2, S=17, causal=0, mask='none', scale='moderate'), 3, False)):
        a = Attention(c)
        out = _out(a.B * a.S, a.d)
        rcs = []
        keys = _ledger(lib, lambda: rcs.append(lib.mc_op_enc_attention(_ptr(a.qkv_dev), _ptr(a.valid_dev if masked else None), _ptr(out),
                                                                        a.B, a.S, a.d, a.heads, 0, form, _stream())))
        torch.cuda.synchronize()
        assert rcs == [MC_ERR_ARG] and keys == [] and bool((out == R.SENTINEL).all()), (c, form, rcs, keys)
    a = Attention(dict(form='small', B=2, heads=1, S=5, causal=0, mask='none', scale='moderate'))
    out = _out(10, 64)
    assert lib.mc_op_enc_attention(_ptr(a.qkv_dev), None, _ptr(out), 2, 5, 128, 1, 0, 0, _stream()) == MC_ERR_ARG       # d != 64 heads
    torch.cuda.synchronize()
    assert bool((out == R.SENTINEL).all())


# -------------------------------------------------------------------------------------------------------------------------
# the BiGRU recurrence
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.gru_cases(), ids=lambda c: f"B{c['B']}S{c['S']}H{c['H']}div{c['len_div']}")
def test_bigru_steps_vs_fp64_step_by_step(c):
    """S calls of one step: each against the fp64 step from the device's own previous h (a sample that is not updated keeps its bits:
    bound 0).  One call of S steps gives the same bits."""
    L_, lib = _lib()
    B, S, H, div = c['B'], c['S'], c['H'], c['len_div']
    gi, whh, bhh, h0, lens = R.gru_inputs(c)
    gid, wd, bd, ld = _dev(gi), _dev(whh), _dev(bhh), lens.cuda()

    def run(h, s0, steps):
        L_.check(lib.mc_op_bigru_steps(_ptr(gid), _ptr(wd), _ptr(bd), _ptr(h), _ptr(ld), div, B, S, H, s0, steps, _stream()), 'bigru_steps')

    h = _out(B, 2 * H)
    h[:B] = h0.reshape(B, 2 * H).cuda()
    prev, worst = h0.reshape(B, 2 * H), 0.0
    keys = []
    for s in range(S):
        keys += _ledger(lib, lambda: run(h, s, 1))
        got = _take(h, B, (c, s))
        ref, bound = R.gru_step_ref(gi, whh, bhh, prev, lens, div, B, S, H, s)
        worst = max(worst, R.ratio(got, ref.reshape(B, 2 * H), bound.reshape(B, 2 * H)))
        prev = got
    _show('gru_step', c, worst)
    assert worst <= 1.0
    assert set(k.split('@')[0] for k in keys) == {'gemm_k<0>'}, keys
    never = R.gru_lens(lens, div, S) == 0
    assert torch.equal(prev[never], h0.reshape(B, 2 * H)[never])
    whole = _out(B, 2 * H)
    whole[:B] = h0.reshape(B, 2 * H).cuda()
    run(whole, 0, S)
    assert torch.equal(_take(whole, B, c), prev), 'one call of S steps differs from S calls of one step'


# -------------------------------------------------------------------------------------------------------------------------
# the k = 4 / s = 2 / p = 1 convolution
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.conv_cases(), ids=lambda c: f"B{c['B']}T{c['T']}C{c['C']}O{c['O']}")
def test_conv1d_k4s2_vs_fp64(c):
    """the first-layer form: frames of ldx = C + 4 floats (the 4 trailing ones never read: NaN), tap-major weight [O][4][Cp], output
    into the padded buffer of a next convolution (pad rows exactly 0).  A sample of NaN frames leaves the other samples' bits alone."""
    L_, lib = _lib()
    B, T, C, O = c['B'], c['T'], c['C'], c['O']
    Cp, ldx, T1 = (C + 3) // 4 * 4, C + 4, (T - 2) // 2 + 1
    x, w, bias = R.conv_inputs(c)
    wd, bd = _dev(R.tap_major(w, Cp)), _dev(bias)

    def run(x):
        xs = torch.full((B * T, ldx), R.NAN)
        xs[:, :C] = x.reshape(B * T, C)
        y, xd = _out(B * (T1 + 2), O), _dev(xs)
        keys = _ledger(lib, lambda: L_.check(lib.mc_op_conv1d_k4s2(_ptr(xd), ldx, _ptr(wd), _ptr(bd), _ptr(y), B, T, C, Cp, O, 0.2,
                                                                   _stream()), 'conv1d_k4s2'))
        assert [k.split('@')[0] for k in keys] == ['gemm_k<0>'], keys
        torch.cuda.synchronize()
        out = y.cpu()
        assert bool((out[B * (T1 + 2):] == R.SENTINEL).all()), 'guard rows were written'
        return out[:B * (T1 + 2)].reshape(B, T1 + 2, O)

    got = run(x)
    ref, bound = R.conv_k4s2_ref(x, w, bias, 0.2, Cp)
    assert bool((got[:, 0] == 0).all()) and bool((got[:, -1] == 0).all()), 'pad rows'
    r = R.ratio(got, ref, bound)
    _show('conv1d_k4s2', c, r)
    assert r <= 1.0
    if B > 1:
        xn = x.clone()
        xn[1] = R.NAN
        other = run(xn)
        keep = [b for b in range(B) if b != 1]
        assert torch.equal(other[keep], got[keep]), "a sample's frames entered another sample's windows"
        assert bool(torch.isnan(other[1, 1:-1]).all()) and bool((other[1, (0, -1)] == 0).all())


# -------------------------------------------------------------------------------------------------------------------------
# the strided forms of mc_launch_gemm
# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', R.gemm_cases(), ids=lambda c: c['name'])
def test_gemm_strided_vs_fp64(c):
    """all of C is compared: the launch's elements against fp64 inside the elementwise bound, everything else (pad rows of a padded
    buffer, the guard behind it) still the sentinel"""
    L_, lib = _lib()
    ops = R.gemm_inputs(c)
    dev = {k: _dev(ops[k]) for k in ('A', 'W', 'bias', 'R', 'add')}
    nc = ops['nc']
    C = torch.full((nc + GUARD * c['ldc'],), R.SENTINEL, device='cuda')
    g = L_.GemmStrided(a_dev=_ptr(dev['A']), lda=c['lda'], a_gstride=c['a_gstride'], w_dev=_ptr(dev['W']), ldw=c['ldw'],
                       w_gstride=c['w_gstride'], bias_dev=_ptr(dev['bias']), b_gstride=c['b_gstride'],
                       c_dev=ctypes.c_void_p(C.data_ptr() + 4 * c['c_off']), ldc=c['ldc'], c_gstride=c['c_gstride'],
                       res_dev=_ptr(dev['R']), ldr=c['ldr'], r_gstride=c['r_gstride'], add_dev=_ptr(dev['add']), ld_add=c['ld_add'],
                       dup_rows=c['dup_rows'], add_mod=c['add_mod'], act=c['act'], act_after_res=c['act_after_res'], M=c['M'], N=c['N'],
                       K=c['K'])
    keys = _ledger(lib, lambda: L_.check(lib.mc_op_gemm_strided(c['mode'], c['groups'], ctypes.byref(g), _stream()), c['name']))
    assert [k.split('@')[0] for k in keys] == [c['kernel']], keys
    torch.cuda.synchronize()
    out = C.cpu()
    assert bool((out[nc:] == R.SENTINEL).all()), 'guard rows were written'
    c0 = dict(c, c_off=0)                   # the reference indexes from the pointer the launch was given
    ref, bound = R.gemm_expected(c0, dict(ops, nc=nc - c['c_off']))
    r = R.ratio(out[c['c_off']:nc], ref, bound)
    _show(c['kernel'], c['name'], r)
    assert bool((out[:c['c_off']] == R.SENTINEL).all()) and r <= 1.0


def test_gemm_strided_refuses_a_table_on_unaligned_output_rows():
    """the row-periodic table and the duplicate rows exist in the vector epilogue only: N % 4 != 0 is MC_ERR_ARG, not a silent drop"""
    L_, lib = _lib()
    c = dict(next(c for c in R.gemm_cases() if c['name'] == 'enc_K322_res_table_dup'), N=126, res=0, dup_rows=0)
    ops = R.gemm_inputs(c)
    dev = {k: _dev(ops[k]) for k in ('A', 'W', 'bias', 'add')}
    C = torch.full((ops['nc'],), R.SENTINEL, device='cuda')
    g = L_.GemmStrided(a_dev=_ptr(dev['A']), lda=c['lda'], w_dev=_ptr(dev['W']), ldw=c['ldw'], bias_dev=_ptr(dev['bias']), c_dev=_ptr(C),
                       ldc=c['ldc'], r_gstride=-1, add_dev=_ptr(dev['add']), ld_add=c['ld_add'], add_mod=c['add_mod'], M=c['M'], N=c['N'],
                       K=c['K'])
    assert lib.mc_op_gemm_strided(4, 1, ctypes.byref(g), _stream()) == MC_ERR_ARG
    torch.cuda.synchronize()
    assert bool((C == R.SENTINEL).all())

"""CPU: the yardstick of tests/test_encoder_kernels.py is itself checked here.

1. every fp64 reference of ``encoder_ref.py`` against torch's own module in fp64 (1e-12 relative);
2. for every case of the GPU test, the fp32 evaluation of the same formula stays inside the derived bound (a bound that an honest
   fp32 evaluation breaks would be wrong, not strict);
3. every ``wrong=`` variant, evaluated in fp32 like a kernel, exceeds 10x the bound on at least one case of its kernel (a variant no
   case sees would be a hole in the case list).
Each test prints the figures it asserts on."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import encoder_ref as R

F32, F64 = torch.float32, torch.float64


def _close(a, b, what):
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    print(f'{what}: relative {err:.2e}')
    assert err <= 1e-12, (what, err)


# -------------------------------------------------------------------------------------------------------------------------
# 1. the references against torch
# -------------------------------------------------------------------------------------------------------------------------
def test_ln_ref_is_torch_layer_norm():
    for c in (dict(rows=5, L=260, eps=1e-5, relu=0), dict(rows=9, L=64, eps=1e-12, relu=1)):
        x, g, b = (t.double() for t in R.ln_inputs(c))
        t = F.layer_norm(x, (c['L'],), g, b, c['eps'])
        _close(R.ln_ref(x, g, b, c['eps'], c['relu']), t.relu() if c['relu'] else t, f'layer_norm {c}')


def test_embed_ref_is_torch_embedding():
    c = R.embed_cases()[1]
    ids, emb, pos = R.embed_inputs(c)
    i = ids.long().clamp(0, R.EMBED_VOCAB - 1)
    t = F.embedding(i, emb.double()).reshape(c['B'], c['S'], -1) + pos.double()
    assert torch.equal(R.embed_ref(ids, emb, pos, c['S']), t.reshape(-1, c['d']))


@pytest.mark.parametrize('c', [c for c in R.attention_stream_cases() if c['scale'] == 'moderate' and c['S'] in (17, 129, 198)],
                         ids=R.attention_case_id)
def test_attention_ref_is_torch_sdpa(c):
    B, S, heads = c['B'], c['S'], c['heads']
    d = heads * R.HD
    qkv, valid = R.attention_inputs(c).double(), R.attention_mask(c)
    q, k, v = R._qkv_heads(qkv, B, S, d, heads, F64)
    allow = torch.ones(B, 1, S, S, dtype=torch.bool)
    if valid is not None:
        allow = allow & (valid != 0)[:, None, None, :]
    if c['causal']:
        allow = allow & torch.ones(S, S, dtype=torch.bool).tril()
    t = F.scaled_dot_product_attention(q, k, v, attn_mask=allow.expand(B, heads, S, S)).permute(0, 2, 1, 3).reshape(B * S, d)
    ref = R.attention_ref(qkv, valid, B, S, d, heads, c['causal'])
    zero = R.attention_zero_rows(valid, B, S, c['causal'])
    assert bool((ref[zero] == 0).all())
    if c['mask'] == 'holes':
        assert int(zero.sum()) >= S + (1 if c['causal'] else 0)        # the fully masked sample (and query 0 behind an invalid key 0)
    _close(ref[~zero], t[~zero], 'attention')


def test_gru_step_ref_is_torch_gru():
    B, S, Hin, H = 4, 6, 10, 8
    g = torch.Generator().manual_seed(3)
    gru = torch.nn.GRU(Hin, H, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, S, Hin, generator=g, dtype=F64)
    h0 = torch.randn(2, B, H, generator=g, dtype=F64)
    lens = torch.tensor([6, 3, 1, 5])
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False)
    with torch.no_grad():
        _, hn = gru(packed, h0)
        p = dict(gru.named_parameters())
        gi = torch.stack([x.reshape(B * S, Hin) @ p['weight_ih_l0' + sfx].T + p['bias_ih_l0' + sfx] for sfx in ('', '_reverse')])
        whh = torch.stack([p['weight_hh_l0'], p['weight_hh_l0_reverse']])
        bhh = torch.stack([p['bias_hh_l0'], p['bias_hh_l0_reverse']])
    h = h0.permute(1, 0, 2).contiguous()
    for s in range(S):
        h, _ = R.gru_step_ref(gi, whh, bhh, h, lens, 1, B, S, H, s)
    _close(h, hn.permute(1, 0, 2), 'gru')
    h4 = h0.permute(1, 0, 2).contiguous()                              # lens // 4 with len_div = 4 is the same recurrence
    for s in range(S):
        h4, _ = R.gru_step_ref(gi, whh, bhh, h4, lens * 4 + torch.tensor([0, 1, 2, 3]), 4, B, S, H, s)
    assert torch.equal(h4, h)


@pytest.mark.parametrize('c', R.conv_cases(), ids=lambda c: f"T{c['T']}C{c['C']}")
def test_conv_ref_is_torch_conv1d(c):
    x, w, b = (t.double() for t in R.conv_inputs(c))
    t = F.leaky_relu(F.conv1d(x.transpose(1, 2), w, b, stride=2, padding=1), 0.2).transpose(1, 2)
    yp, bound = R.conv_k4s2_ref(x, w, b, 0.2)
    T1 = t.shape[1]
    assert yp.shape[1] == T1 + 2 and bool((yp[:, 0] == 0).all()) and bool((yp[:, -1] == 0).all())
    assert bool((bound[:, 0] == 0).all()) and bool((bound[:, 1:-1] > 0).all())
    _close(yp[:, 1:-1], t, 'conv1d')
    # the tap-major order as mc_t2meval.hip states it: out[(o * 4 + k) * Cp + c] = w[(o * C + c) * 4 + k]
    Cp = (c['C'] + 3) // 4 * 4
    tm = R.tap_major(w, Cp).reshape(-1)
    for o, ch, k in ((0, 0, 0), (c['O'] - 1, c['C'] - 1, 3), (1, c['C'] // 2, 2)):
        assert tm[(o * 4 + k) * Cp + ch] == w.reshape(-1)[(o * c['C'] + ch) * 4 + k]
    assert float(tm.abs().sum()) == float(w.abs().sum())


def test_gemm_strided_ref_is_matmul_on_gathered_rows():
    for c in R.gemm_cases():
        ops = R.gemm_inputs(c)
        G, M, N, K = c['groups'], c['M'], c['N'], c['K']
        ic, ref, _ = R.gemm_strided_ref(c, ops)
        if c['dup_rows']:
            assert torch.equal(ref[0], ref[1]) and torch.equal(ic[1], ic[0] + c['dup_rows'] * c['ldc'])
            ref = ref[0]
        for g in range(G):
            A = torch.stack([ops['A'][g * c['a_gstride'] + r * c['lda']:][:K] for r in range(M)]).double()
            W = ops['W'][g * c['w_gstride']:].reshape(-1, c['ldw'])[:N, :K].double()
            pre = A @ W.T + ops['bias'][g * c['b_gstride']:][:N].double()
            Rg = None
            if c['res']:
                rgs = c['r_gstride'] if c['r_gstride'] >= 0 else c['c_gstride']
                Rg = torch.stack([ops['R'][g * rgs + r * c['ldr']:][:N] for r in range(M)]).double()
            if Rg is not None and c['act_after_res']:
                pre = pre + Rg
            t = R.act64(pre, c['act'])
            if c['add']:
                t = t + torch.stack([ops['add'][(r % c['add_mod']) * c['ld_add']:][:N] for r in range(M)]).double()
            if Rg is not None and not c['act_after_res']:
                t = t + Rg
            _close(ref[g], t, f"{c['name']} group {g}")
        C, Bd = R.gemm_expected(c, ops)
        assert int((Bd > 0).sum()) == G * M * N * (2 if c['dup_rows'] else 1), 'output elements overlap'
        if c['c_off']:
            assert bool((C.reshape(G, M + 2, N)[:, (0, -1)] == R.SENTINEL).all())


def test_window_case_is_the_convolution():
    """the GM_PLAIN window launch is the convolution: lda = 2C < K = 4C over padded frames"""
    c = R.gemm_cases()[0]
    ops = R.gemm_inputs(c)
    G, M, N, Cc = c['groups'], c['M'], c['N'], c['lda'] // 2
    xp = ops['A'].double().reshape(G, 2 * M + 2, Cc)
    w = ops['W'].double().reshape(N, 4, Cc)
    t = F.conv1d(xp.transpose(1, 2), w.permute(0, 2, 1), ops['bias'].double(), stride=2).transpose(1, 2)
    _close(R.gemm_strided_ref(c, ops)[1], t, 'windows')


# -------------------------------------------------------------------------------------------------------------------------
# 2. + 3. fp32 inside the bound on every case; every wrong variant seen at 10x on some case
# -------------------------------------------------------------------------------------------------------------------------
def _report(kernel, worst32, seen, wrongs):
    print(f'{kernel}: fp32 restatement at most {worst32:.4f} of the bound')
    for w in wrongs:
        print(f'  wrong={w}: {seen[w][0]:.3g}x the bound at best ({seen[w][1]})')
    assert worst32 <= 1.0
    for w in wrongs:
        assert seen[w][0] >= 10, (kernel, w, seen[w])


def _note(seen, w, r, what):
    if r > seen[w][0]:
        seen[w] = (r, what)


def test_ln_cases_fp32_inside_and_wrong_variants_seen():
    worst, seen = 0.0, {w: (0.0, None) for w in R.LN_WRONG}
    by_L = {}
    for c in R.ln_cases():
        x, g, b = R.ln_inputs(c)
        ref = R.ln_ref(x, g, b, c['eps'], c['relu'])
        bound = R.ln_bound(x, g, b, c['eps'])
        r32 = R.ratio(R.ln_ref(x, g, b, c['eps'], c['relu'], dtype=F32), ref, bound)
        worst = max(worst, r32)
        k = [i for i in range(c['rows']) if R.LN_KINDS[i] == 'const']
        if k:
            assert torch.equal(ref[k[0]], b.double().relu() if c['relu'] else b.double())
        for w in R.LN_WRONG:
            rw = R.ratio(R.ln_ref(x, g, b, c['eps'], c['relu'], dtype=F32, wrong=w), ref, bound)
            _note(seen, w, rw, c)
            if w == 'one_pass' and c['rows'] > 1:
                by_L[c['L']] = max(by_L.get(c['L'], 0.0), rw)
    print('one_pass by L (rows offset by 1e3):', {L: round(v, 1) for L, v in by_L.items()})
    assert all(by_L[L] >= 10 for L in (64, 256, 260, 768)), by_L       # the one-pass sensitivity is carried by the L <= 768 cases
    _report('ln_wide_k', worst, seen, R.LN_WRONG)


def _attention_sweep(cases, wrongs):
    worst, seen = 0.0, {w: (0.0, None) for w in wrongs}
    for c in cases:
        B, S, heads = c['B'], c['S'], c['heads']
        d = heads * R.HD
        qkv, valid = R.attention_inputs(c), R.attention_mask(c)
        ref = R.attention_ref(qkv, valid, B, S, d, heads, c['causal'])
        bound = R.attention_bound(qkv, B, S, d, heads)
        zero = R.attention_zero_rows(valid, B, S, c['causal'])
        got = R.attention_ref(qkv, valid, B, S, d, heads, c['causal'], dtype=F32)
        assert bool((got[zero] == 0).all()) and bool((ref[zero] == 0).all())
        worst = max(worst, R.ratio(got, ref, bound))
        for w in wrongs:
            if (w == 'mask_shift' and valid is None) or (w == 'causal_ge' and not c['causal']) or (w == 'drop_key_64' and S <= 64) or \
                    (w == 'no_rescale' and S <= 64) or (w == 'scale_d' and heads == 1):
                continue
            _note(seen, w, R.ratio(R.attention_ref(qkv, valid, B, S, d, heads, c['causal'], dtype=F32, wrong=w), ref, bound),
                  R.attention_case_id(c))
    return worst, seen


def test_attention_small_cases_fp32_inside_and_wrong_variants_seen():
    wrongs = ('drop_last_key', 'drop_key_64', 'causal_ge', 'scale_d')       # no key mask and no chunks in this form
    worst, seen = _attention_sweep(R.attention_small_cases(), wrongs)
    _report('mha_small_k', worst, seen, wrongs)


def test_attention_stream_cases_fp32_inside_and_wrong_variants_seen():
    worst, seen = _attention_sweep(R.attention_stream_cases(), R.ATTN_WRONG)
    _report('mha_masked_k', worst, seen, R.ATTN_WRONG)


def test_gru_cases_fp32_inside_and_wrong_variants_seen():
    worst, seen = 0.0, {w: (0.0, None) for w in R.GRU_WRONG}
    for c in R.gru_cases():
        B, S, H = c['B'], c['S'], c['H']
        gi, whh, bhh, h, lens = R.gru_inputs(c)
        gi_full = R.gru_inputs(c, poison=False)[0]       # the wrong variants read rows the step never reads: finite here
        h = h.double()
        for s in range(S):
            ref, bound = R.gru_step_ref(gi, whh, bhh, h, lens, c['len_div'], B, S, H, s)
            got, _ = R.gru_step_ref(gi, whh, bhh, h.float(), lens, c['len_div'], B, S, H, s, dtype=F32)
            worst = max(worst, R.ratio(got, ref, bound))
            idle = R.gru_lens(lens, c['len_div'], S) <= s
            assert torch.equal(ref[idle], h[idle])
            for w in R.GRU_WRONG:
                gw, _ = R.gru_step_ref(gi_full, whh, bhh, h.float(), lens, c['len_div'], B, S, H, s, dtype=F32, wrong=w)
                _note(seen, w, R.ratio(gw, ref, bound), (c['H'], c['len_div'], s))
            h = got.double()             # continue from the fp32 state, as the device test continues from the device's
    _report('gru step', worst, seen, R.GRU_WRONG)


def test_conv_cases_fp32_inside():
    worst = 0.0
    for c in R.conv_cases():
        x, w, b = R.conv_inputs(c)
        Cp = (c['C'] + 3) // 4 * 4
        ref, bound = R.conv_k4s2_ref(x, w, b, 0.2, Cp)
        got, _ = R.conv_k4s2_ref(x, w, b, 0.2, Cp, dtype=F32)
        worst = max(worst, R.ratio(got, ref, bound))
    print(f'conv: fp32 restatement at most {worst:.4f} of the bound')
    assert worst <= 1.0


def test_gemm_cases_fp32_inside_and_wrong_variants_seen():
    worst, seen = 0.0, {w: (0.0, None) for w in R.GEMM_WRONG}
    for c in R.gemm_cases():
        ops = R.gemm_inputs(c)
        ref, bound = R.gemm_expected(c, ops)
        worst = max(worst, R.ratio(R.gemm_expected(c, ops, dtype=F32)[0], ref, bound))
        for w in R.GEMM_WRONG:
            if (w == 'window_stride_K' and c['lda'] >= c['K']) or (w == 'add_row_abs' and not c['add']) or \
                    (w == 'act_before_res' and not c['act_after_res']):
                continue
            _note(seen, w, R.ratio(R.gemm_expected(c, ops, dtype=F32, wrong=w)[0], ref, bound), c['name'])
    _report('strided gemm', worst, seen, R.GEMM_WRONG)


def test_encoder_ops_are_bound():
    from motioncraft_amd import lib as L
    lib = L.load(require_gpu=False)
    for name in ('mc_op_enc_ln', 'mc_op_enc_embed_tokens', 'mc_op_enc_attention', 'mc_op_gemm_strided', 'mc_op_bigru_steps',
                 'mc_op_conv1d_k4s2'):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert ctypes.sizeof(L.GemmStrided) == 17 * 8 + 6 * 4           # mc_gemm_strided: 17 pointers / int64, 6 int32
    assert L.ENC_ATTN_FORMS == dict(layer=0, small=1, stream=2) and (L.GM_PLAIN, L.GM_ENC) == (0, 4)

"""Torch-CPU restatement of the kernels of the four step-invariant encoders (text, evaluation, BiGRU evaluator, wav encoder), the
yardstick of ``mc_op_enc_ln`` (ln_wide_k), ``mc_op_enc_embed_tokens`` (embed_tokens_k), ``mc_op_enc_attention`` (mha_small_k,
mha_masked_k), ``mc_op_bigru_steps`` (grouped gemm_k<0> + gru_gate_k), ``mc_op_conv1d_k4s2`` (pad_time_k, gemm_k<0>, lrelu_k) and
``mc_op_gemm_strided`` (gemm_k<0>, gemm_k<4>, gemm_wp_k).  Tests import it; the product does not.  Written from the formulas and
pinned to torch's own modules in fp64 by ``tests/test_encoder_ref_host.py``.  It also holds the cases and the inputs of
``tests/test_encoder_kernels.py``, so that the host test can show on the CPU what each case is able to see.

``dtype=torch.float64`` is the exact side; ``torch.float32`` runs the same formula in fp32 (the restatement whose distance from fp64
every bound below must cover).  ``wrong=`` selects a deliberately wrong evaluation, run in fp32 like a kernel would:
    LayerNorm   'one_pass' (E[x^2] - mean^2), 'n_minus_1' (unbiased variance), 'drop_tail' (the last float4 of the row missing from
                both sums), 'eps_outside' (1 / (sqrt(var) + eps))
    attention   'drop_last_key', 'drop_key_64' (the first key of the second 64-key chunk), 'mask_shift' (the key mask read one key
                late), 'causal_ge' (key == query masked too), 'no_rescale' (running-max softmax over 64-key chunks without the
                rescale of the earlier chunks), 'scale_d' (q / sqrt(d) instead of q / sqrt(64))
    GRU step    'r_outside' (tanh(r (a + g))), 'z_swap' (z n + (1 - z) h), 'reverse_from_S' (reverse direction indexed from S - 1,
                not len - 1), 'no_len_div'
    GEMM        'window_stride_K' (row stride K: windows do not overlap), 'add_row_abs' (table row r, not r % add_mod),
                'act_before_res' (where act_after_res = 1)

Error bounds (u = 2^-24; first order, with a factor 1.01 for the products of the terms; nothing is tuned on a device)
-----------------------------------------------------------------------------------------------------------------------------------
LayerNorm (``ln_bound``, elementwise).  A sum of n terms in ANY order is only known to n u sum|x|, and at that width a row with a
large mean hides a one-pass variance.  So the two sums are bounded by the DEPTH of a wave-per-row reduction instead: a lane adds
ceil(L / 256) float4s (4 additions each), the butterfly over 64 lanes has 6 levels, and the division by L and one spare make
    D = 4 ceil(L / 256) + 8,      |sum - exact| <= D u sum|x_i|.
A kernel that reduces a row in a deeper chain (one thread per row, say) is outside this bound on purpose.  With d = x - mean,
var = mean(d^2), rstd = 1 / sqrt(var + eps), n = d rstd:
    dmean = D u mean|x|
    var: sum_i 2 d_i dmean = 0 (the exact d sum to 0), so the mean's error enters at second order, dmean^2; each d_i^2 carries
         3 u (rounding of d twice, of the square once) and the sum D u:  dvar = (D + 4) u var + dmean^2
    rstd: relative  e_r = dvar / (2 (var + eps)) + 4 u   (the addition of eps, rsqrt at 2 ulp, the division by L is in D)
    y = n g + b:    |y - ref| <= |g| rstd (dmean + u |d|) + |n g| (e_r + 3 u) + u (|n g| + |b|)
A constant row of a value c with exact multiples (c = 0.75) has d = 0 exactly: y = beta (relu(beta)) bit for bit.

Embedding: one fp32 addition of two fp32 values, so the fp32 sum exactly.

Attention (``attention_bound``, one number per case).  The output is a convex combination of value rows, so an error of relative size
r in the weights moves it by at most r max|v|.
    score: q / 8 is exact (a power of two); a dot product of 64 terms in any order is within 64 u sum_c |q_c k_c| / 8, and the
           subtraction of the maximum adds u |s - m| <= 2 u max|s|:  a = 66 u max_{q,k} sum_c |q_c k_c| / 8  (absolute, in the
           exponent: a relative error a of the exponential).  The maximum itself cancels between numerator and sum, and so does every
           rescale factor exp(m_old - m_new) of the streaming form, which multiplies both.
    weight = e / l: numerator a + 2 u (expf), sum a + 2 u + its additions, together 2 a + 4 u + additions.
    additions: l is a sum of positive terms, 6 butterfly levels plus per 64-key chunk one multiply-add (2 roundings): 6 + 2 ceil(S / 64);
           p v is a chain of S multiply-adds (padding keys add exact zeros) plus 2 roundings per chunk for the rescale, one for the
           product; the division and the normalisation of the small form 2 more:  S + 4 ceil(S / 64) + 10 <= S + 72 for S <= 960.
    r = 2 a + 4 u + (S + 72) u,      bound = 1.01 r max|v|.
A query with no usable key is defined to give a zero row (torch gives NaN there); such rows are compared exactly.

GRU step (``gru_step_ref`` returns the bound tensor).  gh = h W^T + b: (H + 2) u (|h| |W|^T + |b|) = dgh.  Through the gates, with
slope 1/4 of the sigmoid, slope 1 of tanh and 4 u per transcendental (expf or tanhf, the division):
    dr = (dgh_r + u |a_r + g_r|) / 4 + 4 u,     dz likewise
    dn = dr |g_n| + r dgh_n + 2 u |r g_n| + u |a_n + r g_n| + 4 u
    dh = |n - h| dz + (1 - z) dn + 3 u (|n| + |h|)
No bound is accumulated over the S steps: every step is compared with the fp64 step taken from the device's own previous h.  A sample
that is not updated at a step (s >= len) keeps h bit for bit.

Strided GEMM and the convolution (``gemm_bound``): the elementwise bound at the top of tests/test_gemm_kernels.py, restated:
    |C - ref| <= s (K u (|A| |W|^T + |bias|) + 4 u |pre|) + e_act + u (|R| + |add|) + 4 u |ref|
with s the activation's largest slope and e_act = 2^-21 |pre| + 8 u |act(pre)|; with act_after_res the residual is part of pre
(+ u |R| + u |pre| inside the activation).  The convolution's LeakyReLU(0.2) is a kernel of its own: s = 1 and the same e_act.
"""
import itertools
import math
import zlib

import torch

U = 2.0 ** -24
SENTINEL = 777.0
NAN = float('nan')
HD = 64                                   # head_dim of the encoder attention
LN_WRONG = ('one_pass', 'n_minus_1', 'drop_tail', 'eps_outside')
ATTN_WRONG = ('drop_last_key', 'drop_key_64', 'mask_shift', 'causal_ge', 'no_rescale', 'scale_d')
GRU_WRONG = ('r_outside', 'z_swap', 'reverse_from_S', 'no_len_div')
GEMM_WRONG = ('window_stride_K', 'add_row_abs', 'act_before_res')
SLOPE = {0: 1.0, 1: 1.1289, 2: 1.0998, 3: 1.0, 4: 1.0998}      # max |act'|: GELU, SiLU, LeakyReLU(0.01), x sigmoid(1.702 x)


def ratio(got, ref, bound):
    """largest |got - ref| / bound over all elements; inf if anything is not finite.  Elements with bound 0 must be equal."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float('inf')
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# -------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# -------------------------------------------------------------------------------------------------------------------------
def ln_ref(x, gamma, beta, eps, relu=False, dtype=torch.float64, wrong=None):
    x, g, b = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    L = x.shape[-1]
    xs = x[..., :L - 4] if wrong == 'drop_tail' else x
    mean = xs.sum(-1, keepdim=True) / L
    if wrong == 'one_pass':
        var = (xs * xs).sum(-1, keepdim=True) / L - mean * mean
        var = var.clamp_min(0)
    else:
        var = ((xs - mean) ** 2).sum(-1, keepdim=True) / L
    if wrong == 'n_minus_1':
        var = var * L / max(L - 1, 1)
    rstd = 1 / (var.sqrt() + eps) if wrong == 'eps_outside' else 1 / (var + eps).sqrt()
    y = (x - mean) * rstd * g + b
    return y.clamp_min(0) if relu else y


def ln_bound(x, gamma, beta, eps):
    x, g = x.double(), gamma.double()
    L = x.shape[-1]
    D = 4 * math.ceil(L / 256) + 8
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1 / (var + eps).sqrt()
    dmean = D * U * x.abs().mean(-1, keepdim=True)
    e_r = ((D + 4) * U * var + dmean ** 2) / (2 * (var + eps)) + 4 * U
    n = d * rstd
    ref = n * g
    return 1.01 * (g.abs() * rstd * (dmean + U * d.abs()) + ref.abs() * (e_r + 3 * U) + U * (ref.abs() + beta.double().abs()))


LN_KINDS = ('plain', 'offset', 'const', 'small', 'offset', 'plain', 'small', 'offset', 'plain')
LN_CONST = 0.75


def ln_cases():
    return [dict(rows=r, L=L, eps=eps, relu=relu) for r, L, eps, relu in
            itertools.product((1, 5, 9), (4, 64, 256, 260, 768, 4096), (1e-5, 1e-12), (0, 1))]


def ln_inputs(c):
    """x [rows][L]: plain rows (unit spread), rows offset by 1e3, rows of spread 1e-2, one constant row; gamma, beta of both signs"""
    g = _gen('ln', c['rows'], c['L'])
    rows, L = c['rows'], c['L']
    x = torch.randn(rows, L, generator=g)
    for r in range(rows):
        k = LN_KINDS[r]
        if k == 'offset':
            x[r] += 1e3
        elif k == 'small':
            x[r] = 0.3 + 1e-2 * x[r]
        elif k == 'const':
            x[r] = LN_CONST
    gamma = 1 + 0.5 * torch.randn(L, generator=g)
    beta = torch.randn(L, generator=g)
    return x, gamma, beta


# -------------------------------------------------------------------------------------------------------------------------
# token embedding
# -------------------------------------------------------------------------------------------------------------------------
def embed_ref(ids, emb, pos, S, dtype=torch.float64):
    """x[r] = emb[clamp(ids[r], 0, vocab - 1)] + pos[r % S]"""
    vocab = emb.shape[0]
    i = ids.long().clamp(0, vocab - 1)
    r = torch.arange(ids.numel())
    return emb.to(dtype)[i] + pos.to(dtype)[r % S]


EMBED_VOCAB = 11


def embed_cases():
    return [dict(B=3, S=7, d=4), dict(B=3, S=7, d=512), dict(B=5, S=3, d=52)]


def embed_inputs(c):
    g = _gen('embed', c['d'])
    rows = c['B'] * c['S']
    ids = torch.randint(0, EMBED_VOCAB, (rows,), generator=g, dtype=torch.int32)
    ids[:4] = torch.tensor([0, EMBED_VOCAB - 1, -1, EMBED_VOCAB], dtype=torch.int32)
    ids[-1] = EMBED_VOCAB + 1000
    return ids, torch.randn(EMBED_VOCAB, c['d'], generator=g), torch.randn(c['S'], c['d'], generator=g)


# -------------------------------------------------------------------------------------------------------------------------
# multi-head attention over [B*S][3d] rows
# -------------------------------------------------------------------------------------------------------------------------
def _qkv_heads(qkv, B, S, d, heads, dtype):
    x = qkv[:B * S, :3 * d].to(dtype).reshape(B, S, 3, heads, HD)
    return (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))        # [B][heads][S][64]


def attention_ref(qkv, valid, B, S, d, heads, causal, dtype=torch.float64, wrong=None):
    """out [B*S][d]; valid: [B][S] (0 = the key is not attended) or None; a query with no usable key gives a zero row"""
    q, k, v = _qkv_heads(qkv, B, S, d, heads, dtype)
    q = q * (1 / math.sqrt(d) if wrong == 'scale_d' else 0.125)
    sc = q @ k.transpose(-1, -2)
    allow = torch.ones(B, 1, S, S, dtype=torch.bool)
    if valid is not None:
        m = valid.reshape(B, S) != 0
        if wrong == 'mask_shift':
            m = m[:, torch.arange(S).add(1).clamp_max(S - 1)]
        allow = allow & m[:, None, None, :]
    if causal:
        allow = allow & torch.ones(S, S, dtype=torch.bool).tril(-1 if wrong == 'causal_ge' else 0)
    if wrong == 'drop_last_key':
        allow = allow.clone()
        allow[..., S - 1] = False
    if wrong == 'drop_key_64' and S > 64:
        allow = allow.clone()
        allow[..., 64] = False
    allow = allow.expand(B, heads, S, S)
    ninf = torch.full_like(sc, -float('inf'))
    sc = torch.where(allow, sc, ninf)
    if wrong == 'no_rescale':            # every chunk's numerators are taken against the running maximum at that chunk and never rescaled
        mx = torch.empty_like(sc)
        run = torch.full_like(sc[..., :1], -float('inf'))
        for k0 in range(0, S, 64):
            run = torch.maximum(run, sc[..., k0:k0 + 64].amax(-1, keepdim=True))
            mx[..., k0:k0 + 64] = run
    else:
        mx = sc.amax(-1, keepdim=True).expand_as(sc)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.where(allow, (sc - mx).exp(), torch.zeros_like(sc))
    l = e.sum(-1, keepdim=True)
    p = torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))
    return (p @ v).permute(0, 2, 1, 3).reshape(B * S, d)


def attention_zero_rows(valid, B, S, causal):
    """bool [B*S]: queries with no usable key"""
    allow = torch.ones(B, S, S, dtype=torch.bool)
    if valid is not None:
        allow = allow & (valid.reshape(B, 1, S) != 0)
    if causal:
        allow = allow & torch.ones(S, S, dtype=torch.bool).tril()
    return ~allow.any(-1).reshape(B * S)


def attention_bound(qkv, B, S, d, heads):
    q, k, v = _qkv_heads(qkv, B, S, d, heads, torch.float64)
    a = 66 * U * float(((q.abs() * 0.125) @ k.abs().transpose(-1, -2)).max())
    r = 2 * a + 4 * U + (S + 72) * U
    return 1.01 * r * float(v.abs().max())


ATTN_SCALES = {'moderate': 1.2, 'large': 3.5}        # q, k ~ N(0, a^2): |score| up to ~8 and ~50
ATTN_MASKS = ('none', 'prefix', 'holes', 'first64', 'mid64')


def attention_small_cases():
    return [dict(form='small', B=2, heads=h, S=S, causal=c, mask='none', scale=sc)
            for h, S, c, sc in itertools.product((1, 4), (1, 5, 63, 64, 65, 77, 127, 128), (0, 1), ATTN_SCALES)]


def attention_stream_cases():
    out = []
    for S, c, sc in itertools.product((1, 15, 16, 17, 63, 64, 65, 128, 129, 198), (0, 1), ATTN_SCALES):
        for mask in ATTN_MASKS:
            if (mask == 'first64' and S <= 64) or (mask == 'mid64' and S != 198):
                continue
            out.append(dict(form='stream', B=3, heads=2, S=S, causal=c, mask=mask, scale=sc))
    return out


def attention_case_id(c):
    return f"{c['form']}-h{c['heads']}-S{c['S']}-{'causal' if c['causal'] else 'full'}-{c['mask']}-{c['scale']}"


def attention_mask(c):
    """uint8 [B][S] or None.  prefix: lengths 1, S, S // 2.  holes: scattered; sample 1 without key 0 (causal: query 0 has no key),
    sample 2 fully masked.  first64: keys 0..63 invalid (sample 1 with holes behind them, sample 2 only key 0 invalid).  mid64: keys
    64..127 invalid (sample 2 also 0..63: its first two chunks are empty)."""
    B, S, kind = c['B'], c['S'], c['mask']
    if kind == 'none':
        return None
    g = _gen('mask', S, kind)
    m = torch.ones(B, S, dtype=torch.uint8)
    if kind == 'prefix':
        for b, n in enumerate((1, S, max(S // 2, 1))):
            m[b, n:] = 0
    elif kind == 'holes':
        m = (torch.rand(B, S, generator=g) < 0.6).to(torch.uint8)
        m[0, S - 1] = 1
        m[1, 0] = 0
        m[1, S - 1] = 1
        m[2] = 0
    elif kind == 'first64':
        m[0, :64] = 0
        m[1] = (torch.rand(S, generator=g) < 0.6).to(torch.uint8)
        m[1, :64] = 0
        m[1, S - 1] = 1
        m[2, 0] = 0
    elif kind == 'mid64':
        m[:, 64:128] = 0
        m[2, :64] = 0
    return m


def attention_inputs(c):
    """qkv [B*S][3d]: q, k ~ N(0, a^2) with one key per sample pushed up (a running maximum that rises in a later chunk), v ~ N(0, 1)
    with per-key offsets so that a dropped or misplaced key moves the output"""
    B, S, heads = c['B'], c['S'], c['heads']
    d = heads * HD
    g = _gen('attn', B, S, heads, c['scale'])
    a = ATTN_SCALES[c['scale']]
    x = torch.randn(B, S, 3, d, generator=g)
    x[:, :, :2] *= a
    x[:, :, 1] *= torch.linspace(0.6, 1.4, S).reshape(1, S, 1)      # later keys larger: later chunks raise the maximum
    x[:, :, 2] += torch.randn(B, S, 1, generator=g)
    return x.reshape(B * S, 3 * d).contiguous()


# -------------------------------------------------------------------------------------------------------------------------
# one BiGRU recurrence step
# -------------------------------------------------------------------------------------------------------------------------
def gru_lens(lens, len_div, S):
    return (lens.long() // len_div).clamp(max=S)


def gru_step_ref(gi, whh, bhh, h, lens, len_div, B, S, H, s, dtype=torch.float64, wrong=None):
    """step s of both directions.  gi [2][B*S][3H] (r | z | n, input products + b_ih), whh [2][3H][H], bhh [2][3H], h [B][2][H].
    Returns (h_new [B][2][H], bound [B][2][H]); samples with s >= len keep h (bound 0)."""
    h = h.to(dtype).reshape(B, 2, H)
    W, b = whh.to(dtype).reshape(2, 3 * H, H), bhh.to(dtype).reshape(2, 3 * H)
    ln = lens.long().clamp(max=S) if wrong == 'no_len_div' else gru_lens(lens, len_div, S)
    active = (s < ln)
    t_rev = (S - 1 - s) if wrong == 'reverse_from_S' else (ln - 1 - s)
    t = torch.stack([torch.full_like(ln, s), torch.as_tensor(t_rev).expand_as(ln)], 1).clamp(0, S - 1)      # [B][2]
    G = gi.to(dtype).reshape(2, B, S, 3 * H)
    a = G[torch.arange(2)[None, :], torch.arange(B)[:, None], t]                                          # [B][2][3H]
    a = torch.where(active[:, None, None], a, torch.zeros_like(a))
    gh = torch.einsum('bdk,dnk->bdn', h, W) + b
    ar, az, an = a[..., :H], a[..., H:2 * H], a[..., 2 * H:]
    gr, gz, gn = gh[..., :H], gh[..., H:2 * H], gh[..., 2 * H:]
    r = torch.sigmoid(ar + gr)
    z = torch.sigmoid(az + gz)
    n = torch.tanh(r * (an + gn)) if wrong == 'r_outside' else torch.tanh(an + r * gn)
    hn = z * n + (1 - z) * h if wrong == 'z_swap' else (1 - z) * n + z * h
    out = torch.where(active[:, None, None], hn, h)
    dgh = (H + 2) * U * (torch.einsum('bdk,dnk->bdn', h.abs(), W.abs()) + b.abs())
    dr = (dgh[..., :H] + U * (ar + gr).abs()) / 4 + 4 * U
    dz = (dgh[..., H:2 * H] + U * (az + gz).abs()) / 4 + 4 * U
    dn = dr * gn.abs() + r * dgh[..., 2 * H:] + 2 * U * (r * gn).abs() + U * (an + r * gn).abs() + 4 * U
    dh = 1.01 * ((n - h).abs() * dz + (1 - z) * dn + 3 * U * (n.abs() + h.abs()))
    return out, torch.where(active[:, None, None], dh, torch.zeros_like(dh)).double()


def gru_cases():
    """lens: 0 (never updated), 1, S, S + 3 (clamped), and with len_div = 4 values that it does not divide"""
    return [dict(B=6, S=12, H=64, len_div=1, lens=(0, 1, 12, 15, 7, 10)),
            dict(B=6, S=12, H=64, len_div=4, lens=(0, 6, 48, 63, 30, 41)),
            dict(B=3, S=5, H=512, len_div=1, lens=(1, 5, 8)),
            dict(B=3, S=5, H=512, len_div=4, lens=(3, 22, 14))]


def gru_inputs(c, poison=True):
    """poison: gi rows at t >= len, which are never read, are NaN"""
    B, S, H = c['B'], c['S'], c['H']
    g = _gen('gru', B, S, H)
    gi = torch.randn(2, B, S, 3 * H, generator=g)
    lens = torch.tensor(c['lens'], dtype=torch.int32)
    ln = gru_lens(lens, c['len_div'], S)
    for b in range(B if poison else 0):
        gi[:, b, int(ln[b]):] = NAN
    whh = torch.randn(2, 3 * H, H, generator=g) / H ** 0.5
    bhh = 0.5 * torch.randn(2, 3 * H, generator=g)
    h0 = torch.rand(B, 2, H, generator=g) * 2 - 1
    return gi.reshape(2, B * S, 3 * H), whh, bhh, h0, lens


# -------------------------------------------------------------------------------------------------------------------------
# GEMM bound, the k = 4 / s = 2 / p = 1 convolution, the strided GEMM
# -------------------------------------------------------------------------------------------------------------------------
def act64(y, act):
    F = torch.nn.functional
    return {0: lambda v: v, 1: F.gelu, 2: F.silu, 3: lambda v: F.leaky_relu(v, 0.01), 4: lambda v: v * torch.sigmoid(1.702 * v)}[act](y)


def gemm_bound(K, absprod, bias_abs, pre, y, ref, res_abs=None, add_abs=None, slope=1.0, act=True, res_inside=False):
    """the elementwise bound of the module docstring.  pre = A W^T + bias (+ R when res_inside), y = act(pre), ref = the output"""
    bound = K * U * (absprod + bias_abs) + 4 * U * pre.abs()
    if res_inside:
        bound = bound + U * res_abs + U * pre.abs()
    if act:
        bound = slope * bound + 2.0 ** -21 * pre.abs() + 8 * U * y.abs()
    if res_abs is not None and not res_inside:
        bound = bound + U * res_abs
    if add_abs is not None:
        bound = bound + U * add_abs
    return bound + 4 * U * ref.abs()


def conv_k4s2_ref(x, w, bias, slope, Cp=None, dtype=torch.float64):
    """x [B][T][C], w [O][C][4], bias [O] -> (y_padded [B][T1 + 2][O] with zero rows 0 and T1 + 1, bound of the same shape: 0 on the
    pad rows); the kernel sums 4 Cp products per output (Cp >= C: the zero padded channels)"""
    x, w, bias = x.to(dtype), w.to(dtype), bias.to(dtype)
    B, T, C = x.shape
    O = w.shape[0]
    T1 = (T - 2) // 2 + 1
    xp = torch.zeros(B, T + 2, C, dtype=dtype)
    xp[:, 1:T + 1] = x
    win = torch.stack([xp[:, k:k + 2 * T1:2] for k in range(4)], 2)              # [B][T1][4][C]: padded frames 2t + k
    pre = torch.einsum('btkc,ock->bto', win, w) + bias
    absprod = torch.einsum('btkc,ock->bto', win.abs(), w.abs())
    y = torch.where(pre >= 0, pre, slope * pre)
    yp = torch.zeros(B, T1 + 2, O, dtype=dtype)
    yp[:, 1:T1 + 1] = y
    bound = torch.zeros(B, T1 + 2, O, dtype=torch.float64)
    bound[:, 1:T1 + 1] = gemm_bound(4 * (Cp or C), absprod.double(), bias.double().abs(), pre.double(), y.double(), y.double())
    return yp, bound


def tap_major(w, Cp):
    """conv weight [O][C][4] -> [O][4][Cp], element (o, tap, c) = w[o][c][tap], zero for c >= C"""
    O, C, _ = w.shape
    out = torch.zeros(O, 4, Cp, dtype=w.dtype)
    out[:, :, :C] = w.permute(0, 2, 1)
    return out


def conv_cases():
    return [dict(B=3, T=98, C=259, O=64), dict(B=2, T=7, C=8, O=128), dict(B=1, T=4, C=12, O=64)]


def conv_inputs(c):
    g = _gen('conv', c['T'], c['C'])
    x = torch.randn(c['B'], c['T'], c['C'], generator=g) + torch.randn(c['B'], c['T'], 1, generator=g)
    w = torch.randn(c['O'], c['C'], 4, generator=g) / (4 * c['C']) ** 0.5
    return x, w, torch.randn(c['O'], generator=g)


GEMM_DEFAULTS = dict(groups=1, a_gstride=0, w_gstride=0, b_gstride=0, c_gstride=0, c_off=0, ldr=0, r_gstride=-1, act=0,
                     act_after_res=0, add_mod=1, ld_add=0, dup_rows=0, bias=1, res=0, add=0)


def gemm_cases():
    """modelled on the real callers (mc_t2meval.hip, mc_wavenc.hip, mc_evalenc.hip, mc_step.hip); mode 0 = GM_PLAIN, 4 = GM_ENC"""
    C, H = 32, 64
    cs = []
    for M in (49, 5):                       # k = 4 / s = 2 windows over padded frames, written into the interior of a padded buffer
        T = 2 * M
        cs.append(dict(name=f'plain_windows_M{M}', mode=0, kernel='gemm_k<0>', groups=3, M=M, N=64, K=4 * C, lda=2 * C,
                       a_gstride=(T + 2) * C, ldw=4 * C, ldc=64, c_gstride=(M + 2) * 64, c_off=64))
    cs.append(dict(name='plain_gru', mode=0, kernel='gemm_k<0>', groups=2, M=6, N=3 * H, K=H, lda=2 * H, a_gstride=H, ldw=H,
                   w_gstride=3 * H * H, b_gstride=3 * H, ldc=6 * H, c_gstride=3 * H))
    cs.append(dict(name='enc_K15', mode=4, kernel='gemm_k<4>', M=37, N=64, K=15, lda=15, ldw=20, ldc=64))
    cs.append(dict(name='enc_K259', mode=4, kernel='gemm_k<4>', M=130, N=132, K=259, lda=259, ldw=260, ldc=132))
    cs.append(dict(name='enc_K322_res_table_dup', mode=4, kernel='gemm_k<4>', M=50, N=128, K=322, lda=322, ldw=324, ldc=128, res=1,
                   ldr=128, add=1, add_mod=24, ld_add=128, dup_rows=50))
    for cin, after in itertools.product((1, 2), (0, 1)):      # wav encoder first layer: k = 15, stride 5, unpadded rows of Cin floats
        Tp = 211
        cs.append(dict(name=f'enc_wav_cin{cin}_after{after}', mode=4, kernel='gemm_k<4>', groups=2, M=40, N=32, K=15 * cin,
                       lda=5 * cin, a_gstride=Tp * cin, ldw=(15 * cin + 3) // 4 * 4, ldc=32, c_gstride=40 * 32, res=1, ldr=32,
                       r_gstride=40 * 32, act=3, act_after_res=after))
    cs.append(dict(name='enc_aligned_table_dup', mode=4, kernel='gemm_wp_k', M=256, N=256, K=352, lda=352, ldw=352, ldc=256, add=1,
                   add_mod=64, ld_add=256, dup_rows=256))
    return [dict(GEMM_DEFAULTS, **c) for c in cs]


def gemm_inputs(c):
    """flat operands of a case.  W rows hold K values, zeros up to the next multiple of 4 in the encoder mode (the contract: zero
    padded) and NaN beyond (never read); the residual and table rows are NaN beyond N."""
    g = _gen('gemm', c['name'])
    G, M, N, K = c['groups'], c['M'], c['N'], c['K']
    na = (G - 1) * c['a_gstride'] + (M - 1) * c['lda'] + K
    A = torch.randn(na, generator=g) + 0.5
    A[::7] *= 1e-3
    nwg = (G - 1) * c['w_gstride'] // (N * c['ldw']) + 1
    W = torch.full((nwg * N, c['ldw']), NAN)
    W[:, :K] = torch.randn(nwg * N, K, generator=g) / K ** 0.5
    if c['mode'] == 4:
        W[:, K:(K + 3) // 4 * 4] = 0
    W = W.reshape(-1)
    bias = torch.randn((G - 1) * c['b_gstride'] + N, generator=g) if c['bias'] else None
    R = add = None
    rows_c = M + c['dup_rows']
    if c['res']:
        rgs = c['r_gstride'] if c['r_gstride'] >= 0 else c['c_gstride']
        R = torch.randn((G - 1) * rgs + (M - 1) * c['ldr'] + N, generator=g)
    if c['add']:
        add = torch.randn((c['add_mod'] - 1) * c['ld_add'] + N, generator=g)
    nc = c['c_off'] + (G - 1) * c['c_gstride'] + (rows_c - 1) * c['ldc'] + N
    if c['c_off']:
        nc += c['c_off']                    # the trailing pad row of the last sample
    return dict(A=A, W=W, bias=bias, R=R, add=add, nc=nc)


def gemm_strided_ref(c, ops, dtype=torch.float64, wrong=None):
    """the launch as an explicit gather over the index formula of GemmArgs.  Returns (ic, ref, bound): flat indices into C [G][M][N]
    (with dup_rows a second set, stacked on a leading axis of 2), the values, the elementwise bound."""
    G, M, N, K = c['groups'], c['M'], c['N'], c['K']
    gi, r, n, k = torch.arange(G)[:, None, None], torch.arange(M)[None, :, None], torch.arange(N)[None, None, :], torch.arange(K)
    lda = K if wrong == 'window_stride_K' else c['lda']
    A = ops['A'].to(dtype)[(gi * c['a_gstride'] + r * lda)[..., None].clamp_max(ops['A'].numel() - K) + k][:, :, 0]      # [G][M][K]
    Wt = ops['W'].to(dtype)[(gi * c['w_gstride'] + n * c['ldw'])[..., None] + k][:, 0]                                    # [G][N][K]
    b = ops['bias'].to(dtype)[gi * c['b_gstride'] + n] if ops['bias'] is not None else torch.zeros(G, 1, N, dtype=dtype)
    pre = torch.einsum('gmk,gnk->gmn', A, Wt) + b
    absprod = torch.einsum('gmk,gnk->gmn', A.abs(), Wt.abs())
    R = Ra = None
    if ops['R'] is not None:
        rgs = c['r_gstride'] if c['r_gstride'] >= 0 else c['c_gstride']
        R = ops['R'].to(dtype)[gi * rgs + r * c['ldr'] + n]
    if ops['add'] is not None:
        row = r if wrong == 'add_row_abs' else r % c['add_mod']
        idx = row * c['ld_add'] + n
        tab = ops['add'].flip(0).repeat(int(idx.max()) // ops['add'].numel() + 2)     # add_row_abs: whatever lies behind the table
        tab[:ops['add'].numel()] = ops['add']
        Ra = tab.to(dtype)[idx].expand(G, M, N)
    inside = bool(c['act_after_res']) and R is not None and wrong != 'act_before_res'
    if inside:
        pre = pre + R
    y = act64(pre, c['act'])
    ref = y
    if Ra is not None:
        ref = ref + Ra
    if R is not None and not inside:
        ref = ref + R
    bound = gemm_bound(K, absprod.double(), b.double().abs(), pre.double(), y.double(), ref.double(),
                       res_abs=R.double().abs() if R is not None else None, add_abs=Ra.double().abs() if Ra is not None else None,
                       slope=SLOPE[c['act']], act=bool(c['act']), res_inside=inside)
    ic = c['c_off'] + gi * c['c_gstride'] + r * c['ldc'] + n
    if c['dup_rows']:
        ic = torch.stack([ic, ic + c['dup_rows'] * c['ldc']])
        ref, bound = torch.stack([ref, ref]), torch.stack([bound, bound])
    return ic, ref, bound


def gemm_expected(c, ops, dtype=torch.float64, wrong=None):
    """(C, bound) as flat buffers of ops['nc'] elements: the sentinel (bound 0) wherever the launch does not write"""
    ic, ref, bound = gemm_strided_ref(c, ops, dtype, wrong)
    C = torch.full((ops['nc'],), SENTINEL, dtype=torch.float64)
    Bd = torch.zeros(ops['nc'], dtype=torch.float64)
    C[ic.reshape(-1)] = ref.double().reshape(-1)
    Bd[ic.reshape(-1)] = bound.reshape(-1)
    return C, Bd

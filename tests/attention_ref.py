"""Torch-CPU restatement of the two MC-Attn cores over the flat buffers the step keeps, the yardstick of ``body_reg_k``,
``temporal_k``, ``temporal_h_k`` and the body phase of ``pqbody_k`` / ``pqbody_h_k`` (``mc_op_body_attention``,
``mc_op_temporal_attention``).  Tests import it; the product does not.  Written from the formula (st_attention.py:105-179,
efficient_attention.py:25-46) and pinned to ``oracle.stmogen_oracle.stma`` by ``tests/test_attention_ref_host.py``.

Layouts (include/motioncraft_amd.h):
    mf [2B*T*H][ld >= 4L] = [body_value | key | value | query], row (b T + t) H + h      tf [2B][Nt][2L] = [key | value]
    qkv [frames*H][3L] = [q | k | v]      wsm [H][H] = softmax(body_weight, dim 1)      mask [B][T]      ys / yt [rows][H*L]

``dtype=torch.float64`` is the exact side; ``torch.float32`` runs the same formula in fp32 (the restatement whose distance from
fp64 every bound below must cover).  One addition is fp32 in both: ``key + (1 - m) * -1e6`` (st_attention.py:153-154) is an fp32
addition in the reference project and in the kernels, and a fully masked column's softmax weights depend on its rounding.

``wrong=`` selects a deliberately wrong evaluation (the sensitivity tests): 'stats_last' / 'stats_seam' leave one key row (the last
one / the one at the text | motion seam) out of the column maximum and sum, 'mask_shift' reads the mask one frame late,
'no_last_text' ignores the last text row, 'q_channel' takes softmax(q) over L - 1 channels; body: 'contraction' drops the last
channel of a head from both contractions, 'wsm_T' reads the static weight transposed.

Error bounds (u = 2^-24; every bound is first order with a factor 1.01 for the products of the terms)
----------------------------------------------------------------------------------------------------
Both outputs are convex combinations of value rows: y = sum_d sq[d] sum_n p[n][d] v[n], with p a softmax over the rows n and sq
one over channels, so an error of relative size r in any weight moves y by at most r max|v|.  The scale of a temporal case is
V = max|v| (text and motion values); of a body case V = max|v| + 2 max|bv| (the static mix, a convex combination of bv rows, and the
residual bv).
  * exponent argument: the kernels evaluate exp(x - max) as exp2(x log2(e) - max log2(e)) with both products rounded (and the
    constant log2(e) rounded) before the subtraction, so the argument's absolute error in the log2 domain is at most
    6 max|x| log2(e) u (2 u per product for rounding and constant, on both, plus the subtraction), a relative error of the
    exponential of a(x) = 6 max|x| u  (ln 2 log2(e) = 1).  max|k| runs over the rows a softmax can see (mask or condition 1).
  * one v_exp_f32: 1 ulp, e = 2 u.
  * a weight = numerator / sum: the numerator carries a + e, the sum of n terms n u + a + e (+ 2 (a + e + u) for the two rescales
    of the online column statistics, temporal only), the reciprocal and the product 4 u.
  * the two contractions add n u each (n fp32 additions in any order, MFMA or VALU).
  temporal, fp32 forms (n = Nseq = Nt + T rows, then L channels):
      r32 = 4 a(k) + 2 a(q) + 6 e + (2 Nseq + 2 L + 12) u
  body (n = H parts for k, HD = L / 8 channels for q; static mix H + 1, residual additions 4):
      r32 = 2 a(k) + 2 a(q) + 4 e + (3 H + 2 HD + 13) u
  f16x3 (temporal_h_k<., true>): r32 + 2 * 2^-22, the lo * lo products the three-product form leaves out of each contraction.
  f16 (temporal_h_k<., false>):  r32 + (1 + 2^-11)^4 - 1, one fp16 rounding of each operand on the path: e, V, q' and A2.
  bound = 1.01 r V.
Fused kernels through a context (pqbody_k / pqbody_h_k): q/k/v are recomputed in fp64 from the context's own mf, so the kernel's
q/k/v differ by the error of its LayerNorm and its K = L GEMM: dn = (2 L + 16) u max|n| per normalised element (mean, variance and
the scaling in fp32), d = g sum |n'| |W| + |bias| u + sum dn |gamma| |W| per output with g = (L + 2) u in fp32, + 2^-21 in the
three-product form, + 2 * 2^-11 with plain fp16 operands.  These are carried through the two softmaxes and the two contractions
element by element (``qkv_error_term``), so the fused body bound is a tensor: the fp32 bound above plus that term.
"""
import torch

U = 2.0 ** -24
EXP_ULP = 2 * U
G = 8                                    # dynamic heads
SENTINEL = 777.0
NEG = -1000000.0
TEMPORAL_WRONG = ('stats_last', 'stats_seam', 'mask_shift', 'no_last_text', 'q_channel')
BODY_WRONG = ('contraction', 'wsm_T')


def _softmax(x, dim, keep=None):
    """softmax over ``dim``; keep (bool, broadcastable): entries outside it do not enter the maximum or the sum (their own
    numerator is still divided by that sum)."""
    if keep is None:
        return torch.softmax(x, dim)
    big = torch.finfo(x.dtype).max
    m = torch.where(keep, x, torch.full_like(x, -big)).amax(dim, keepdim=True)
    e = torch.exp(x - m)
    return e / (e * keep).sum(dim, keepdim=True)


# -------------------------------------------------------------------------------------------------------------------------
# the two cores
# -------------------------------------------------------------------------------------------------------------------------
def body_ref(mf, qkv, wsm, H, L, dtype=torch.float64, wrong=None):
    """ys [frames][H*L] = softmax(body_weight) bv + bv + the 8-head linear attention over the H parts of each frame."""
    HD = L // G
    F = qkv.shape[0] // H
    bv = mf[:F * H, :L].to(dtype).reshape(F, H, L)
    q, k, v = (qkv[:F * H, i * L:(i + 1) * L].to(dtype).reshape(F, H, G, HD) for i in range(3))
    w = wsm.to(dtype).reshape(H, H)
    if wrong == 'wsm_T':
        w = w.t()
    static = torch.einsum('hj,fjc->fhc', w, bv)
    q = torch.softmax(q, dim=-1)
    k = torch.softmax(k, dim=1)
    if wrong == 'contraction':
        q, k = q[..., :HD - 1], k[..., :HD - 1]
    att = torch.einsum('fhgd,fhgl->fgdl', k, v)
    dy = torch.einsum('fhgd,fgdl->fhgl', q, att).reshape(F, H, L)
    return (static + (bv + dy)).reshape(F, H * L)


def temporal_ref(mf, tf, mask, B, T, Nt, H, L, dtype=torch.float64, wrong=None, alias=False):
    """yt [2B*T][H*L]: softmax of [text | motion] keys over the Nt + T rows, A2 = K^T V per (sample, part), softmax_L(Q) A2.
    alias: the samples b >= B read the motion rows of sample b - B (twin aliasing with the flag at 0)."""
    B2 = 2 * B
    m4 = mf[:, :4 * L].reshape(B2, T, H, 4 * L)
    if alias:
        m4 = torch.cat((m4[:B], m4[:B]), 0)
    cnd = torch.cat((torch.ones(B), torch.zeros(B))).reshape(B2, 1, 1, 1)
    msk = mask.reshape(B, T).float().repeat(2, 1).reshape(B2, T, 1, 1)
    if wrong == 'mask_shift':
        msk = torch.cat((torch.zeros_like(msk[:, :1]), msk[:, :-1]), 1)
    t4 = tf.reshape(B2, Nt, 1, 2 * L)
    # the one fp32 addition
    key = torch.cat(((t4[..., :L].float() + (1 - cnd) * NEG).expand(B2, Nt, H, L), m4[..., L:2 * L].float() + (1 - msk) * NEG), 1).to(dtype)
    val = torch.cat(((t4[..., L:].to(dtype) * cnd.to(dtype)).expand(B2, Nt, H, L), m4[..., 2 * L:3 * L].to(dtype) * msk.to(dtype)), 1)
    qry = m4[..., 3 * L:].to(dtype)
    if wrong == 'no_last_text':
        sel = [n for n in range(Nt + T) if n != Nt - 1]
        key, val = key[:, sel], val[:, sel]
    keep = None
    if wrong in ('stats_last', 'stats_seam'):
        keep = torch.ones(1, Nt + T, 1, 1, dtype=torch.bool)
        keep[0, Nt + T - 1 if wrong == 'stats_last' else seam_row(mask, Nt)] = False
    p = _softmax(key, 1, keep)
    if wrong == 'q_channel':
        kq = torch.ones(L, dtype=torch.bool)
        kq[L - 1] = False
        sq = _softmax(qry, -1, kq) * kq
    else:
        sq = torch.softmax(qry, -1)
    att = torch.einsum('bnhd,bnhl->bhdl', p, val)
    return torch.einsum('bthd,bhdl->bthl', sq, att).reshape(B2 * T, H * L)


def seam_row(mask, Nt):
    """The key row at the text | motion seam whose loss a softmax can see: frame 0 if some sample keeps it, else the last text row."""
    return Nt if bool((mask.reshape(-1, mask.shape[-1])[:, 0] != 0).any()) else Nt - 1


# -------------------------------------------------------------------------------------------------------------------------
# bounds
# -------------------------------------------------------------------------------------------------------------------------
def _arg(x):
    return 6.0 * float(x) * U


def temporal_scales(mf, tf, mask, B, T, Nt, H, L):
    """(max|k| over the rows a softmax can see, max|q|, max|v|) of a case."""
    m4 = mf[:, :4 * L].reshape(2 * B, T, H, 4 * L).double()
    t3 = tf.reshape(2 * B, Nt, 2 * L).double()
    vis = mask.reshape(B, T).repeat(2, 1).reshape(2 * B, T, 1, 1) != 0
    km = (m4[..., L:2 * L].abs() * vis).max()
    kt = t3[:B, :, :L].abs().max()
    return float(torch.maximum(km, kt)), float(m4[..., 3 * L:].abs().max()), float(max(m4[..., 2 * L:3 * L].abs().max(), t3[..., L:].abs().max()))


def temporal_bound(form, mf, tf, mask, B, T, Nt, H, L):
    """Largest admissible |yt - fp64| of a temporal case for a kernel form ('whole', 'lsplit', 'pair', 'step': fp32)."""
    kmax, qmax, vmax = temporal_scales(mf, tf, mask, B, T, Nt, H, L)
    r = 4 * _arg(kmax) + 2 * _arg(qmax) + 6 * EXP_ULP + (2 * (Nt + T) + 2 * L + 12) * U
    if form == 'f16x3':
        r += 2 * 2.0 ** -22
    elif form == 'f16':
        r += (1 + 2.0 ** -11) ** 4 - 1
    else:
        assert form in ('whole', 'lsplit', 'pair', 'step', 'f32'), form
    return 1.01 * r * vmax


def body_bound(mf, qkv, H, L, extra=0.0):
    """Largest admissible |ys - fp64| of a body case (extra: the q/k/v error term of the fused kernels, qkv_error_term, which
    makes the bound a tensor [frames][H*L])."""
    F = qkv.shape[0] // H
    HD = L // G
    q, k, v = (float(qkv[:, i * L:(i + 1) * L].abs().max()) for i in range(3))
    bv = float(mf[:F * H, :L].abs().max())
    r = 2 * _arg(k) + 2 * _arg(q) + 4 * EXP_ULP + (3 * H + 2 * HD + 13) * U
    return 1.01 * r * (v + 2 * bv) + extra


def qkv_from_mf(mf, gamma, beta, W, bias, L, prec='f32'):
    """(qkv in fp64 [tokens][3L], the bound d [tokens][3L] on the error of a kernel's own q/k/v): LayerNorm_L + Linear of mf[:, :L]."""
    x = mf[:, :L].double()
    n = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + 1e-5)
    g, b, Wd = gamma.double(), beta.double(), W.double()
    n2 = n * g + b
    qkv = n2 @ Wd.t() + bias.double()
    dn = (2 * L + 16) * U * n.abs().amax(-1, keepdim=True) * g.abs() + 2 * U * (n2.abs())
    gk = (L + 2) * U + {'f32': 0.0, 'f16x3': 2.0 ** -21, 'f16': 2 * 2.0 ** -11}[prec]
    d = gk * (n2.abs() @ Wd.abs().t()) + U * bias.double().abs() + dn.expand_as(n2) @ Wd.abs().t()
    return qkv, d


def qkv_lowp(mf, gamma, beta, W, bias, L, prec='f32'):
    """q/k/v [tokens][3L] as an fp32 evaluation forms them (the restatement the fused bound must cover): LayerNorm and Linear in
    fp32; 'f16': both GEMM operands rounded to fp16 first, products and sums fp32 ('f16x3' is fp32-class: evaluated as fp32)."""
    n2 = torch.nn.functional.layer_norm(mf[:, :L].float(), (L,), gamma.float(), beta.float())
    Wf = W.float()
    if prec == 'f16':
        n2, Wf = n2.half().float(), Wf.half().float()
    return n2 @ Wf.t() + bias.float()


def fused_case(L):
    """(dims, state dict, x, xf, mask, B, T) of the fused-kernel cases: small default dims, B = 3, T = 24, ragged lengths."""
    from helpers import synth_inputs
    from oracle import weights as W
    dims = W.default_dims(L=L, F=256, max_seq_len=24)
    B, T = 3, 24
    x, xf, mask = synth_inputs(dims, B, T, seed=6, lengths=[24, 18, 11])
    return dims, W.make_state_dict(dims, 3), x, xf, mask, B, T


def body_weights(sd, layer):
    """(gamma, beta, W [3L][L], bias [3L], wsm [H][H] fp64) of a layer's dynamic and static body topology."""
    pre = f'temporal_decoder_blocks.{layer}.ca_block.'
    a = pre + 'body_d_attn.'
    W = torch.cat([sd[a + f'{n}.weight'] for n in ('query', 'key', 'value')])
    b = torch.cat([sd[a + f'{n}.bias'] for n in ('query', 'key', 'value')])
    return sd[a + 'norm.weight'], sd[a + 'norm.bias'], W, b, torch.softmax(sd[pre + 'body_weight'].double(), dim=1)


def qkv_error_term(qkv, d, H, L):
    """[frames][H*L]: how far errors |dq|, |dk|, |dv| <= d [tokens][3L] of q/k/v can move the dynamic part of ys, per element.
    A softmax p of arguments x moves under |dx_i| <= d_i by |dp_i| <= c p_i (d_i + sum_j p_j d_j), c = exp(4 max d) (the derivative
    of p_i along the segment is p_i (dx_i - sum_j p_j dx_j), and every p on the segment is within exp(2 max d) of its end value).
    With dq and dk those weight bounds and A[d][l] = sum_h k[h][d] v[h][l]:
        |dA| <= sum_h (dk |v| + k dv + dk dv),    |dy[h][l]| <= sum_d (dq |A| + q dA + dq dA)."""
    HD = L // G
    F = qkv.shape[0] // H
    q, k, v = (qkv[:, i * L:(i + 1) * L].double().reshape(F, H, G, HD) for i in range(3))
    eq, ek, ev = (d[:, i * L:(i + 1) * L].double().reshape(F, H, G, HD) for i in range(3))
    c = float(torch.exp(4 * torch.maximum(eq.max(), ek.max())))
    sq, sk = torch.softmax(q, -1), torch.softmax(k, 1)
    dq = c * sq * (eq + (sq * eq).sum(-1, keepdim=True))
    dk = c * sk * (ek + (sk * ek).sum(1, keepdim=True))
    A = torch.einsum('fhgd,fhgl->fgdl', sk, v).abs()
    dA = torch.einsum('fhgd,fhgl->fgdl', dk, v.abs() + ev) + torch.einsum('fhgd,fhgl->fgdl', sk, ev)
    dy = torch.einsum('fhgd,fgdl->fhgl', dq, A + dA) + torch.einsum('fhgd,fgdl->fhgl', sq, dA)
    return dy.reshape(F, H * L)


# -------------------------------------------------------------------------------------------------------------------------
# cases: the inputs of tests/test_attention_kernels.py, shared with the host tests that judge their bounds
# -------------------------------------------------------------------------------------------------------------------------
TN = ((1, 8), (31, 77), (32, 32), (33, 77), (24, 64), (70, 77))
MASKS = ('ones', 'ragged', 'holes', 'single_last', 'one_masked')
KEYS = ('normal', 'big', 'mask_wins')
FORMS = ('whole', 'lsplit', 'pair', 'f16x3', 'f16')


def forms_of(L, H):
    """The kernel forms that exist for a shape."""
    return tuple(f for f in FORMS if f == 'whole' or (L >= 64 and (f != 'pair' or (L == 64 and H % 2 == 0))))


def make_mask(kind, B, T):
    """[B][T].  Sample 0 keeps its last frame wherever the kind allows it, so the last key row is one a softmax can see."""
    m = torch.ones(B, T)
    if kind == 'ragged':
        for b in range(1, B):
            m[b, max(1, (T * (B - b)) // (B + 1)):] = 0
        if B == 1:
            m[0, max(1, T // 2):] = 0
    elif kind == 'holes':
        for b in range(B):
            for t in range(1, T - 1):
                if t % 5 == 2 + b % 2:
                    m[b, t] = 0
            if b:
                m[b, max(1, T - 3 * b):] = 0
    elif kind == 'single_last':
        m[:] = 0
        m[:, T - 1] = 1
    elif kind == 'one_masked':
        m[B - 1] = 0
    else:
        assert kind == 'ones', kind
    return m


def applicable(mask_kind, key_kind, B, T):
    """'mask_wins' needs a masked-out frame."""
    return key_kind != 'mask_wins' or bool((make_mask(mask_kind, B, T) == 0).any())


def temporal_cases():
    """dict(L, H, T, Nt, B, mask, keys, seed) per input set: every shape of the table with the mask and key kinds dealt round
    robin, then every applicable (mask, keys) pair at three shapes, then B = 3 at L = 64 (the only way to temporal_k<64, true>'s
    gridDim.z = 1: 6 * 12 * 2 * 2 > 256)."""
    out, i = [], 0
    for L in (32, 64, 128):
        for H in (8, 12):
            for T, Nt in TN:
                mk, kk = MASKS[i % 5], KEYS[(i // 5 + i) % 3]
                if not applicable(mk, kk, 2, T):
                    kk = 'normal'
                out.append(dict(L=L, H=H, T=T, Nt=Nt, B=2, mask=mk, keys=kk, seed=100 + i))
                i += 1
    for L, H, T, Nt in ((32, 12, 33, 77), (64, 12, 70, 77), (128, 8, 70, 77)):
        for mk in MASKS:
            for kk in KEYS:
                if applicable(mk, kk, 2, T) and not any((o['L'], o['H'], o['T'], o['mask'], o['keys']) == (L, H, T, mk, kk) for o in out):
                    out.append(dict(L=L, H=H, T=T, Nt=Nt, B=2, mask=mk, keys=kk, seed=100 + i))
                    i += 1
    out.append(dict(L=64, H=12, T=70, Nt=77, B=3, mask='ragged', keys='normal', seed=100 + i))
    return out


def case_id(c):
    return '-'.join(f'{k}{c[k]}' for k in ('L', 'H', 'T', 'Nt', 'B')) + f'-{c["mask"]}-{c["keys"]}'


def temporal_inputs(c):
    """(mf [2B*T*H][4L], tf [2B][Nt][2L], mask [B][T]) of a case, fp32.  Standard normal, the keys scaled as the kind says; on top, a
    few planted entries in sample 0 of both halves (parts 0 and H - 1) that make the errors of TEMPORAL_WRONG loud at every shape: the
    last text row, frame 0 and the last frame each hold the largest key of one column (3, L / 2, L - 1) by two key scales, and the
    queries of frames 0 and T - 1 lean on those three columns."""
    L, H, T, Nt, B = c['L'], c['H'], c['T'], c['Nt'], c['B']
    g = torch.Generator().manual_seed(c['seed'])
    mf = torch.randn(2 * B * T * H, 4 * L, generator=g)
    tf = torch.randn(2 * B, Nt, 2 * L, generator=g)
    mask = make_mask(c['mask'], B, T)
    s, off = (8.0, 50.0) if c['keys'] == 'big' else (1.0, 0.0)
    mf[:, L:2 * L] = mf[:, L:2 * L] * s + off
    tf[:, :, :L] = tf[:, :, :L] * s + off
    m4 = mf.view(2 * B, T, H, 4 * L)
    dA, dB, dC = 3, L // 2, L - 1
    for b in (0, B):
        top = torch.maximum(m4[b, :, :, L:2 * L].amax((0, 1)), tf[b, :, :L].amax(0))     # column maxima over all rows and parts
        tf[b, Nt - 1, dA] = top[dA] + 2 * s
        for h in (0, H - 1):
            m4[b, 0, h, L + dB] = top[dB] + 2 * s
            m4[b, T - 1, h, L + dC] = top[dC] + 2 * s
            for t in (0, T - 1):
                m4[b, t, h, 3 * L + torch.tensor([dA, dB, dC])] = m4[b, t, h, 3 * L:].max() + 3.0
    if c['keys'] == 'mask_wins':
        # one column where a single masked-out frame holds the largest raw key
        bs, ts = [(int(b), int(t)) for b, t in (mask == 0).nonzero()][0]
        for b in (bs, bs + B):
            m4[b, ts, :, L + 7] = 100.0
    return mf, tf, mask


BODY_FRAMES = (1, 7, 33, 100)


def body_cases():
    """dict(L, H, frames, kind, seed): every (L, H, frames) with standard-normal inputs; q and k scaled by 8 and offset by +30 at
    frames = 33."""
    out, i = [], 0
    for L in (32, 64, 128):
        for H in (8, 12):
            for F in BODY_FRAMES:
                out.append(dict(L=L, H=H, frames=F, kind='normal', seed=500 + i))
                i += 1
            out.append(dict(L=L, H=H, frames=33, kind='big', seed=500 + i))
            i += 1
    return out


def body_case_id(c):
    return f'L{c["L"]}-H{c["H"]}-F{c["frames"]}-{c["kind"]}'


def body_inputs(c, pad=0):
    """(mf [frames*H][4L + pad], qkv [frames*H][3L], wsm [H][H]) of a case, fp32; the pad columns hold NaN (never read)."""
    L, H, F = c['L'], c['H'], c['frames']
    g = torch.Generator().manual_seed(c['seed'])
    mf = torch.randn(F * H, 4 * L, generator=g)
    qkv = torch.randn(F * H, 3 * L, generator=g)
    wsm = torch.softmax(torch.randn(H, H, generator=g), dim=1)
    if c['kind'] == 'big':
        qkv[:, :2 * L] = qkv[:, :2 * L] * 8.0 + 30.0
    if pad:
        mf = torch.cat((mf, torch.full((F * H, pad), float('nan'))), 1)
    return mf.contiguous(), qkv, wsm

"""Host checks of ``attention_ref.py``, the fp64 yardstick of the MC-Attn kernels (no GPU).

  * the restatement over the flat buffers agrees with ``oracle.stmogen_oracle.stma``'s captured y_t / y_s to the oracle's fp32
    round-off (the fp32 bound of the captured inputs), so the yardstick is pinned to the project's existing one, not to itself;
  * every input set of ``tests/test_attention_kernels.py`` can see the subtle errors these kernels can make: each deliberately
    wrong evaluation differs from the right one by at least 10x the case's bound, for every kernel form the case runs (the
    fused-kernel cases on the oracle's capture of the same model and batch, in the three precisions);
  * every bound is loose enough for an honest fp32 evaluation: the same formula in fp32 stays inside it on every case.
"""
import pytest
import torch

import attention_ref as R
from helpers import HML_SMALL, SMALL, SMALL_SEED, synth_inputs

TCASES = R.temporal_cases()
BCASES = R.body_cases()


def _layer_buffers(sd, dims, lcap, i, prec='f32'):
    L, H = dims['L'], dims['H']
    mf = lcap['motion_feat'].reshape(-1, 4 * L)
    tf = lcap['text_feat'].reshape(lcap['text_feat'].shape[0], -1, 2 * L)
    g, b, W, bias, wsm = R.body_weights(sd, i)
    qkv, d = R.qkv_from_mf(mf, g, b, W, bias, L, prec)
    return mf, tf, qkv, R.qkv_error_term(qkv, d, H, L), wsm


@pytest.mark.parametrize('name', ['motionx_small', 'humanml3d_small'])
def test_reference_agrees_with_the_oracle(name):
    from oracle import stmogen_oracle as O, weights as W
    dims = SMALL if name == 'motionx_small' else HML_SMALL
    L, H, Nt = dims['L'], dims['H'], dims['Nt']
    assert H == (12 if name == 'motionx_small' else 8)
    sd = W.make_state_dict(dims, SMALL_SEED)
    B, T = 2, 24
    x, xf, mask = synth_inputs(dims, B, T, seed=31, lengths=[24, 15])
    cap = {}
    O.denoise(sd, dims, x, 500, xf, mask, cap=cap)
    for i in range(dims['NL']):
        lcap = cap[f'layer{i}']
        mf, tf, qkv, extra, wsm = _layer_buffers(sd, dims, lcap, i)
        yt = R.temporal_ref(mf, tf, mask, B, T, Nt, H, L)
        et = float((yt - lcap['y_t'].reshape(yt.shape).double()).abs().max())
        bt = R.temporal_bound('f32', mf, tf, mask, B, T, Nt, H, L)
        ys = R.body_ref(mf, qkv, wsm, H, L)
        rs = float(((ys - lcap['y_s'].reshape(ys.shape).double()).abs() / R.body_bound(mf, qkv, H, L, extra)).max())
        print(f'{name} layer {i}: |y_t - oracle| {et:.2e} (bound {bt:.2e}), |y_s - oracle| / bound {rs:.4f}')
        assert et <= bt and rs <= 1.0
        assert float(yt.abs().max()) > 0.05 and float(ys.abs().max()) > 0.05


@pytest.mark.parametrize('L', [64, 128])
def test_fused_cases_see_the_wrong_references_and_hold_an_fp32_evaluation(L):
    """The inputs of the fused-kernel GPU cases, as the oracle produces them on the CPU (mf and the text rows of layers 0 and 1 of
    the same model, batch and timestep): in each precision the body bound, widened element by element by the q/k/v error term,
    still tells both wrong body evaluations apart at 10x, and an evaluation with q/k/v formed in fp32 (fp16 GEMM operands for
    'f16') stays inside it; the same two checks for the temporal core at the fp32 bound, the form the chain launches there."""
    from oracle import stmogen_oracle as O
    dims, sd, x, xf, mask, B, T = R.fused_case(L)
    H, Nt = dims['H'], dims['Nt']
    cap = {}
    O.denoise(sd, dims, x, 700, xf, mask, cap=cap)
    for i in (0, 1):
        lcap = cap[f'layer{i}']
        g, b, W, bias, wsm = R.body_weights(sd, i)
        for prec in ('f32', 'f16x3', 'f16'):
            mf, tf, qkv, extra, _ = _layer_buffers(sd, dims, lcap, i, prec)
            bound = R.body_bound(mf, qkv, H, L, extra)
            right = R.body_ref(mf, qkv, wsm, H, L)
            for wrong in R.BODY_WRONG:
                d = float(((R.body_ref(mf, qkv, wsm, H, L, wrong=wrong) - right).abs() / bound).max())
                print(f'fused L{L} layer {i} {prec} {wrong}: {d:.0f} x the bound')
                assert d >= 10, (prec, wrong, d)
            low = R.body_ref(mf, R.qkv_lowp(mf, g, b, W, bias, L, prec), wsm, H, L, dtype=torch.float32).double()
            e = float(((low - right).abs() / bound).max())
            print(f'fused L{L} layer {i} {prec} fp32 restatement: {e:.3f} of the bound')
            assert e <= 1.0
        args = (mf, tf, mask, B, T, Nt, H, L)
        right, bt = R.temporal_ref(*args), R.temporal_bound('f32', *args)
        for wrong in R.TEMPORAL_WRONG:
            d = float((R.temporal_ref(*args, wrong=wrong) - right).abs().max()) / bt
            print(f'fused L{L} layer {i} temporal {wrong}: {d:.0f} x the bound')
            assert d >= 10, (wrong, d)          # (finite: NaN fails)
        assert float((R.temporal_ref(*args, dtype=torch.float32).double() - right).abs().max()) <= bt


@pytest.mark.parametrize('c', TCASES, ids=R.case_id)
def test_temporal_case_sees_the_wrong_references_and_holds_an_fp32_evaluation(c):
    L, H, T, Nt, B = c['L'], c['H'], c['T'], c['Nt'], c['B']
    mf, tf, mask = R.temporal_inputs(c)
    args = (mf, tf, mask, B, T, Nt, H, L)
    right = R.temporal_ref(*args)
    assert bool(torch.isfinite(right).all())
    bounds = {f: R.temporal_bound(f, *args) for f in R.forms_of(L, H)}
    worst = max(bounds.values())
    for wrong in R.TEMPORAL_WRONG:
        # (a wrong evaluation overflows where it loses the only row a column can see -- 'stats_last' / 'stats_seam' at T = 1 and
        # under 'single_last' masks: counted as seen, the GPU tests assert finiteness; the other factors are finite, 26 x and up)
        d = float(torch.nan_to_num((R.temporal_ref(*args, wrong=wrong) - right).abs(), nan=float('inf')).max())
        print(f'{R.case_id(c)} {wrong}: {d:.2e} = {d / worst:.0f} x the widest bound')
        assert d >= 10 * worst, (wrong, d, worst)
    e32 = float((R.temporal_ref(*args, dtype=torch.float32).double() - right).abs().max())
    ea = float((R.temporal_ref(*args, dtype=torch.float32, alias=True).double() - R.temporal_ref(*args, alias=True)).abs().max())
    print(f'{R.case_id(c)} fp32 restatement: {e32 / bounds["whole"]:.3f} of the fp32 bound (aliased {ea / bounds["whole"]:.3f})')
    assert e32 <= bounds['whole'] and ea <= bounds['whole']
    if c['mask'] == 'one_masked':          # the masked sample's unconditioned half is exactly 0
        assert not bool(right.reshape(2 * B, T, -1)[2 * B - 1].any())


@pytest.mark.parametrize('c', BCASES, ids=R.body_case_id)
def test_body_case_sees_the_wrong_references_and_holds_an_fp32_evaluation(c):
    L, H = c['L'], c['H']
    mf, qkv, wsm = R.body_inputs(c)
    right = R.body_ref(mf, qkv, wsm, H, L)
    bound = R.body_bound(mf, qkv, H, L)
    for wrong in R.BODY_WRONG:
        d = float((R.body_ref(mf, qkv, wsm, H, L, wrong=wrong) - right).abs().max())
        print(f'{R.body_case_id(c)} {wrong}: {d / bound:.0f} x the bound')
        assert d >= 10 * bound, (wrong, d, bound)
    e32 = float((R.body_ref(mf, qkv, wsm, H, L, dtype=torch.float32).double() - right).abs().max())
    print(f'{R.body_case_id(c)} fp32 restatement: {e32 / bound:.3f} of the bound')
    assert e32 <= bound


def test_case_lists_cover_what_the_kernels_branch_on():
    """Every (L, H, (T, Nt)) of the table, every mask and key kind, and both gridDim.z of the column-sliced kernel at both widths."""
    shapes = {(c['L'], c['H'], c['T'], c['Nt']) for c in TCASES}
    assert shapes >= {(L, H, T, Nt) for L in (32, 64, 128) for H in (8, 12) for T, Nt in R.TN}
    assert {c['mask'] for c in TCASES} == set(R.MASKS) and {c['keys'] for c in TCASES} == set(R.KEYS)
    for L in (64, 128):
        z = {2 if 2 * c['B'] * c['H'] * (L // 32) * 2 <= 256 else 1 for c in TCASES if c['L'] == L}
        assert z == {1, 2}, (L, z)
    assert {(c['L'], c['H'], c['frames']) for c in BCASES} == {(L, H, F) for L in (32, 64, 128) for H in (8, 12) for F in R.BODY_FRAMES}
    for c in TCASES:          # 'mask_wins': the raw maximum of the column sits on a masked-out frame
        if c['keys'] == 'mask_wins':
            mf, tf, mask = R.temporal_inputs(c)
            L, B, T, H = c['L'], c['B'], c['T'], c['H']
            k = mf.view(2 * B, T, H, 4 * L)[..., L + 7]
            b, t, h = [int(v) for v in (k == k.max()).nonzero()[0]]
            assert mask[b % B, t] == 0 and float(k.max()) == 100.0 > float(tf[..., :L].max())


def test_ops_are_exported_and_refuse_forms_that_do_not_exist():
    """The argument checks run before any launch, so the refusals can be seen without a GPU: the error names the form."""
    import ctypes
    from motioncraft_amd import lib as L_
    lib = L_.load(require_gpu=False)
    for name in ('mc_op_body_attention', 'mc_op_temporal_attention'):
        assert name in L_.EXPORTED_SYMBOLS and hasattr(lib, name), name
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for form, name, L, H in (('lsplit', 'LSPLIT', 32, 8), ('pair', 'PAIR', 32, 8), ('pair', 'PAIR', 128, 12), ('pair', 'PAIR', 64, 7),
                             ('f16x3', 'F16X3', 32, 12), ('f16', 'F16', 32, 8)):
        rc = lib.mc_op_temporal_attention(p, p, p, p, 0, 2, 1, 2, 2, H, L, L_.TEMPORAL_FORMS[form], 1, None, None)
        assert rc != 0 and name in L_.last_error(), (form, L, H, rc, L_.last_error())
    assert lib.mc_op_temporal_attention(p, p, p, p, 0, 2, 1, 2, 2, 8, 64, 9, 1, None, None) != 0
    assert lib.mc_op_body_attention(p, 4 * 40, p, p, p, 1, 12, 40, 0, None, 0, None) != 0          # L = 40: no kernel

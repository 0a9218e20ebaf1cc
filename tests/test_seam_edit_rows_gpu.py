"""GPU (MI355X): kept regions on seam-coupled rows -- ``sampler_seam_edit_rows_k`` through ``mc_op_sampler_seam_edit_rows``, the context
(``mc_ctx_set_long_edits`` + both tables + ``mc_sample_rows``), the switch's refusals, and ``serve.ContinuousBatcher(overlap=,
long_edits=True)`` -- against tests/seam_edit_rows_ref.py (fp64), the seam rows op, the edit rows op and the plain rows op (DESIGN.md
section 4s).

Shapes, tables, coefficients and operand helpers are those of tests/test_seam_rows_gpu.py (imported).  Device against device is exact
(torch.equal).  The blend meets fp64 under section 4m's bound as that file states it -- ``8 eps (w M_r + (1 - w) M_l)`` on a seam,
``4 eps M`` off it, ``M = |a| + |b|``, eps = 2^-24 -- a kept element holds gt exactly; the whole step meets the restatement within that
file's ``1e-5 (1 + max|ref|)``; a context step meets the oracle within the project's per-call 2e-4, a whole walk the reference within
its end-to-end 1e-3.

Measured (MI355X): x0 at most 0.24 of the blend bound on free seam elements, 0.25 off the seams, 0 on kept elements; |x_prev - fp64| at
most 4.4e-07; context x0 against the oracle 1.07e-05 in both samplers; the golden walk through the new kernel 3.3e-06 from the
reference at the golden's own setting (see ``test_golden_edit_walk_through_the_new_kernel`` for the other settings)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import rowstep_ref
import seam_edit_rows_ref as SE
import seam_ref as S
import seam_rows_ref as SR
import test_seam_rows_gpu as Q
from helpers import SMALL
from test_seam_rows_gpu import (C, CB, EPS, GUARD, K_FIRST, K_REQ, K_RIGHT, K_SEEDS, KB, KC, KOV, KT, LAYOUTS, OV, SEED_L, SEED_S, STRIDE, T,
                                TOL_STEP, U64, f64, small, time_limit)  # noqa: F401  (small, time_limit: fixtures)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FLIP = SE.DRAW_FLIP
TOL_E2E = 1e-3
NAN = float('nan')


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
def _k_tables(rows, seed=7):
    """-> (keep uint8 [B,T,C] as the DEVICE gets it, gt float [B,T,C] as the device gets it, kept bool: what the outputs must show).
    Owner entries: a whole kept frame inside each seam, scattered single channels, kept elements on both sides of a row boundary that
    a group straddles, row 1 with nothing kept, bytes of 255 and of 1.  gt is NaN wherever keep == 0, and in the head copy of every
    shared frame keep = 0 / gt = NaN: those entries are never read."""
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(KB, KT, KC, generator=g) < 0.08                      # scattered single channels
    keep[3, KT - KOV + 1] = True                                           # a whole frame inside the seam 3 -> 0
    keep[0, KT - 1] = True                                                 # ... and the last frame of row 0 (seam 0 -> 4): up to the row boundary
    keep[2, KT - 1, KC - 3:] = True                                        # the last three elements of row 2 ...
    keep[3, 0, :2] = True                                                  # ... and the first two of row 3: T C % 4 == 1, one group holds both
    keep[1] = False                                                        # one row with nothing kept
    for b, (_, has_left, _) in enumerate(rows):
        if has_left:
            keep[b, :KOV] = False                                          # head copies: the first ov frames of a row with a left neighbour
    kept = torch.from_numpy(SR.share_left(keep.numpy(), rows, KOV) != 0)   # what the outputs show: the owner's entry in both copies
    words = keep.reshape(-1)[:KB * KT * KC // 4 * 4].view(-1, 4).sum(1)
    assert {1, 2, 3} <= set(words.tolist())                                # keep words with 1, 2 and 3 of 4 bytes set
    straddle = (2 * KT * KC + KT * KC - 3) // 4
    assert keep.reshape(-1)[4 * straddle:4 * straddle + 4].tolist() == [True] * 4 and (4 * straddle + 3) // (KT * KC) == 3
    bytes_ = torch.where(torch.arange(KB * KT * KC).view(KB, KT, KC) % 2 == 1, 255, 1).to(torch.uint8) * keep.to(torch.uint8)
    assert {0, 1, 255} == set(bytes_.unique().tolist())
    gt = torch.randn(KB, KT, KC, generator=g)
    gt_dev = gt.clone()
    gt_dev[~keep] = NAN
    return bytes_, gt_dev, kept


def _dev_bytes(o, fill):
    """keep bytes on the device, `offset` BYTES into their allocation (off 4-byte alignment in the element form), sentinels around"""
    t = torch.full((o.offset + o.n + GUARD,), 77, dtype=torch.uint8, device='cuda')
    t[o.offset:o.offset + o.n] = fill.reshape(-1).cuda()
    v = t[o.offset:o.offset + o.n]
    assert v.data_ptr() % 4 == o.offset
    return v


def _op(o, coefs, x, a, b, noise, gt_noise, gt, keep, hist, xp, x0, weights=None, seeds=None, draws=None, rows=None):
    L_, lib, _ptr, _stream = Q._lib()
    B, T_, C_ = o.shape
    rows = o.rows if rows is None else rows
    right = (ctypes.c_int32 * B)(*[r for r, _, _ in rows])
    ff = (ctypes.c_int32 * B)(*[f for _, _, f in rows])
    w = (ctypes.c_float * o.ov)(*weights) if weights is not None else None
    sd = (ctypes.c_uint64 * B)(*[s & U64 for s in seeds]) if seeds is not None else None
    dr = (ctypes.c_uint64 * B)(*draws) if draws is not None else None
    rc = lib.mc_op_sampler_seam_edit_rows(_ptr(x), _ptr(a), _ptr(b), _ptr(noise), _ptr(gt_noise), _ptr(gt), keep.data_ptr(), sd, dr, _ptr(hist),
                                          _ptr(xp), _ptr(x0), B, T_, C_, o.ov, right, ff, w, (L_.StepCoefs * B)(*coefs), _stream())
    torch.cuda.synchronize()
    L_.check(rc, 'mc_op_sampler_seam_edit_rows')


def _edit_op(o, coefs, x, a, b, noise, gt_noise, gt, keep, hist, xp, x0, seeds=None, draws=None):
    L_, lib, _ptr, _stream = Q._lib()
    B, T_, C_ = o.shape
    sd = (ctypes.c_uint64 * B)(*[s & U64 for s in seeds]) if seeds is not None else None
    dr = (ctypes.c_uint64 * B)(*draws) if draws is not None else None
    L_.check(lib.mc_op_sampler_edit_rows(_ptr(x), _ptr(a), _ptr(b), _ptr(noise), _ptr(gt_noise), _ptr(gt), keep.data_ptr(), sd, dr, _ptr(hist),
                                         _ptr(xp), _ptr(x0), B, T_ * C_, (L_.StepCoefs * B)(*coefs), _stream()), 'mc_op_sampler_edit_rows')
    torch.cuda.synchronize()


def _index0_coefs(mode):
    """the entry of schedule index 0 (the end of a walk): x_prev = x0 there, in mode 1 ab_prev = 1, in mode 2 (kx, k0, k1) = (0, 1, 0)"""
    d = Q._diffusion()
    if mode == 2:
        c = d.multistep_coefs(list(range(d.num_timesteps))[::-1], 6.5)[-1]
        assert c.eta == 0.0
        return c
    return d.step_coefs(0, 'ddpm' if mode == 0 else 'ddim', 6.5, **({} if mode == 0 else dict(eta=0.5)))


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'element_form'])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_seam_edit_rows_op(mode, offset):
    rows = SR.plan_rows(K_RIGHT, K_FIRST, KT, KOV)
    o = Q.Ops(rows, offset, seed=600 + 10 * mode + offset)
    req_coefs = Q._request_coefs(mode)
    coefs = [req_coefs[q] for q in K_REQ]
    ms, m1 = mode == 2, mode == 1
    sh, ov = o.shape, KOV
    seam = torch.from_numpy(SR.seam_mask(rows, KT, ov))[:, :, None].expand(*sh)
    pairs = SR.pairs(rows)
    assert sorted(pairs) == [(0, 4), (3, 0)]
    kb, gt_dev, kept = _k_tables(rows)
    assert bool((kept & seam).any()) and bool((kept & ~seam).any()) and not bool(kept[1].any())
    hist0 = o.hist.clone()
    if ms:
        hist0[2] = NAN                                                     # row 2 takes a first step (k1 == 0): its history is not read
    g2 = torch.randn(sh, generator=torch.Generator().manual_seed(9))       # the kept region's noise tensor (mode 1)
    xd, ad, bd, nd, z2d = o.dev(o.x), o.dev(o.a), o.dev(o.b), o.dev(o.noise), o.dev(g2)
    gtd, kd = o.dev(gt_dev), _dev_bytes(o, kb)
    hist = o.dev(hist0) if ms else None
    xp, x0 = o.dev(), o.dev()
    nz_arg, z2_arg = (None if ms else nd), (z2d if m1 else None)
    _op(o, coefs, xd, ad, bd, nz_arg, z2_arg, gtd, kd, hist, xp, x0)
    XP, X0 = xp.view(sh).cpu(), x0.view(sh).cpu()
    assert bool(torch.isfinite(XP).all()) and bool(torch.isfinite(X0).all())              # no NaN of gt or of row 2's history came through
    # (a) seam pairs bit-equal: x_prev, x0, history
    for l, r in pairs:
        assert torch.equal(XP[l, KT - ov:], XP[r, :ov]) and torch.equal(X0[l, KT - ov:], X0[r, :ov]), (l, r)
    if ms:
        assert torch.equal(hist.view(sh).cpu(), X0)
    # (b) x0 of a kept element is gt, in both copies, bit for bit
    gt_owner = torch.from_numpy(SR.share_left(np.nan_to_num(gt_dev.numpy()), rows, ov)).float()
    assert torch.equal(X0[kept], gt_owner[kept])
    # (c) keep all zero: the seam rows kernel's bits
    zero_k = _dev_bytes(o, torch.zeros(sh, dtype=torch.uint8))
    all_nan = o.dev(torch.full(sh, NAN))
    h_z, h_s = (o.dev(hist0), o.dev(hist0)) if ms else (None, None)
    xp_z, x0_z, xp_s, x0_s = o.dev(), o.dev(), o.dev(), o.dev()
    _op(o, coefs, xd, ad, bd, nz_arg, z2_arg, all_nan, zero_k, h_z, xp_z, x0_z)
    Q._rows_op(o, coefs, xd, ad, bd, nz_arg, h_s, xp_s, x0_s)
    assert torch.equal(xp_z, xp_s) and torch.equal(x0_z, x0_s) and (not ms or torch.equal(h_z, h_s))
    # (d) neither kept nor on a seam: the plain row kernels' bits;  free seam elements: the seam rows kernel's
    h_p = o.dev(hist0) if ms else None
    xp_p, x0_p = o.dev(), o.dev()
    Q._plain_rows_op(o, coefs, xd, ad, bd, nz_arg, h_p, xp_p, x0_p)
    plain = ~kept & ~seam
    assert torch.equal(XP[plain], xp_p.view(sh).cpu()[plain]) and torch.equal(X0[plain], x0_p.view(sh).cpu()[plain])
    free = ~kept
    assert torch.equal(XP[free], xp_s.view(sh).cpu()[free]) and torch.equal(X0[free], x0_s.view(sh).cpu()[free])
    assert not torch.equal(X0[kept], x0_s.view(sh).cpu()[kept])
    # (e) a table without neighbours at first frame 0: the edit rows kernels' bits, on the same device tables
    lone = SR.plan_rows([-1] * KB, [0] * KB, KT, KOV)
    h_l, h_e = (o.dev(hist0), o.dev(hist0)) if ms else (None, None)
    xp_l, x0_l, xp_e, x0_e = o.dev(), o.dev(), o.dev(), o.dev()
    _op(o, coefs, xd, ad, bd, nz_arg, z2_arg, gtd, kd, h_l, xp_l, x0_l, rows=lone)
    _edit_op(o, coefs, xd, ad, bd, nz_arg, z2_arg, gtd, kd, h_e, xp_e, x0_e)
    assert torch.equal(xp_l, xp_e) and torch.equal(x0_l, x0_e) and (not ms or torch.equal(h_l, h_e))
    assert bool(torch.isfinite(xp_l).all())
    # (f) fp64: the blend under 4m's bound, a kept element exact, the whole step against the restatement
    A, Bn = f64(o.a), f64(o.b)
    mag = np.abs(A) + np.abs(Bn)
    wt = S.default_weights(ov)
    hist_ref = np.nan_to_num(f64(hist0)) if ms else None
    ref_step, ref0 = SE.step(coefs, f64(o.x), A, Bn, rows, ov, f64(gt_dev), kb.numpy(), wt, noise=None if ms else f64(o.noise), hist=hist_ref,
                             gt_noise=f64(g2) if m1 else None)
    bound = 4 * EPS * mag
    for l, r in pairs:
        bl = 8 * EPS * (wt[:, None] * mag[r, :ov] + (1 - wt)[:, None] * mag[l, KT - ov:])
        bound[l, KT - ov:], bound[r, :ov] = bl, bl
    bound[kept.numpy()] = 0.0
    err = np.abs(f64(X0) - ref0)
    fr, sm = free.numpy(), seam.numpy()
    print(f'mode {mode} offset {offset}: x0 err/bound on free seam elements {float((err[fr & sm] / bound[fr & sm]).max()):.3f}, off seams '
          f'{float((err[fr & ~sm] / bound[fr & ~sm]).max()):.3f}; kept {float(err[~fr].max()):.1e}; '
          f'|x_prev - fp64| {float(np.abs(f64(XP) - ref_step).max()):.2e}')
    assert bool((err <= bound).all())
    assert np.allclose(f64(XP), ref_step, rtol=0, atol=1e-5 * (1 + np.abs(ref_step).max()))
    # (g) in place = out of place
    x_in = o.dev(o.x)
    h_in = o.dev(hist0) if ms else None
    _op(o, coefs, x_in, ad, bd, nz_arg, z2_arg, gtd, kd, h_in, x_in, None)
    assert torch.equal(x_in.view(sh).cpu(), XP) and (not ms or torch.equal(h_in.view(sh).cpu(), X0))
    # (h) device noise = host noise fed the requests' global fields: the step draw d, and (mode 1) z2 = draw d ^ 2^63 of the same field,
    # the lone row at a non-zero first frame (row 2, kept elements on its last frame) included
    if not ms:
        seeds = [K_SEEDS[q] for q in K_REQ]
        xp_l, xp_e = o.dev(), o.dev()                                      # first frame 0 everywhere: what sampler_edit_rows_k draws
        _op(o, coefs, xd, ad, bd, None, None, gtd, kd, None, xp_l, None, seeds=[3, 4, 5, 6, 7], draws=[1, 2, 3, 4, 2 ** 63 + 5], rows=lone)
        _edit_op(o, coefs, xd, ad, bd, None, None, gtd, kd, None, xp_e, None, seeds=[3, 4, 5, 6, 7], draws=[1, 2, 3, 4, 2 ** 63 + 5])
        assert torch.equal(xp_l, xp_e)
        for draw in (0, 1 + 3):
            def gathered(dn):
                fields = [Q._field(K_SEEDS[q], dn, (f + KT) * KC).cpu().numpy() for q, (_, _, f) in zip(K_REQ, rows)]
                return torch.from_numpy(SR.gather_field(fields, rows, KT, KC)).float()
            pz, pz2 = o.dev(gathered(draw)), o.dev(gathered(draw ^ FLIP))
            xp_h, xp_d, x0_d = o.dev(), o.dev(), o.dev()
            _op(o, coefs, xd, ad, bd, pz, pz2 if m1 else None, gtd, kd, None, xp_h, None)
            _op(o, coefs, xd, ad, bd, None, None, gtd, kd, None, xp_d, x0_d, seeds=seeds, draws=[draw] * KB)
            assert torch.equal(xp_h, xp_d) and torch.equal(x0_d.view(sh).cpu(), X0), draw
            assert kept[2].any() and rows[2][2] != 0
            if m1:                                                         # ... and z2 is NOT the step draw: fed the unflipped field the kept region differs
                xp_w = o.dev()
                _op(o, coefs, xd, ad, bd, pz, pz, gtd, kd, None, xp_w, None)
                assert not torch.equal(xp_w.view(sh).cpu()[kept], xp_d.view(sh).cpu()[kept])
                assert torch.equal(xp_w.view(sh).cpu()[free], xp_d.view(sh).cpu()[free])
    # (i) schedule index 0: the kept region of x_prev IS gt, in both copies
    c0 = _index0_coefs(mode)
    h_0 = o.dev(torch.full(sh, NAN)) if ms else None                       # (k1 == 0 on every row: the history is not read at all)
    xp_0 = o.dev()
    _op(o, [c0] * KB, xd, ad, bd, nz_arg, z2_arg, gtd, kd, h_0, xp_0, None)
    XP0 = xp_0.view(sh).cpu()
    assert bool(torch.isfinite(XP0).all()) and torch.equal(XP0[kept], gt_owner[kept])
    for l, r in pairs:
        assert torch.equal(XP0[l, KT - ov:], XP0[r, :ov])
    # (j) nothing was stored before or behind any operand or output; the keep bytes are untouched
    assert o.guards_intact() and torch.equal(kd.cpu(), kb.reshape(-1))


def test_op_refusals_launch_nothing():
    L_, lib, _ptr, _stream = Q._lib()
    rows = SR.plan_rows(K_RIGHT, K_FIRST, KT, KOV)
    o = Q.Ops(rows, 0, seed=2)
    kb, gt_dev, _ = _k_tables(rows)
    xd, ad, bd, nd, gtd, kd, xp = o.dev(o.x), o.dev(o.a), o.dev(o.b), o.dev(o.noise), o.dev(gt_dev), _dev_bytes(o, kb), o.dev()
    good = [Q._request_coefs(1)[q] for q in K_REQ]
    with pytest.raises(RuntimeError, match='gt_noise_dev'):                # mode 1 beside a noise tensor needs the kept region's
        _op(o, good, xd, ad, bd, nd, None, gtd, kd, None, xp, None)
    with pytest.raises(RuntimeError, match='exclude'):                     # both noise sources
        _op(o, good, xd, ad, bd, nd, nd, gtd, kd, None, xp, None, seeds=[1, 2, 3, 1, 1], draws=[1] * KB)
    with pytest.raises(RuntimeError, match='share a seam'):
        _op(o, good, xd, ad, bd, None, None, gtd, kd, None, xp, None, seeds=[1, 2, 3, 4, 1], draws=[1] * KB)
    assert lib.mc_op_sampler_seam_edit_rows(_ptr(xd), _ptr(ad), _ptr(bd), _ptr(nd), _ptr(nd), None, kd.data_ptr(), None, None, None, _ptr(xp), None,
                                            KB, KT, KC, KOV, (ctypes.c_int32 * KB)(*K_RIGHT), (ctypes.c_int32 * KB)(*K_FIRST), None,
                                            (L_.StepCoefs * KB)(*good), _stream()) == L_.MC_ERR_ARG
    torch.cuda.synchronize()
    assert bool((xp == 777.0).all())


# ---- the context --------------------------------------------------------------------------------------------------------------------
WALK = 6                                                                   # ddim6: the long request walks to schedule index 0
LEAD = 2                                                                   # the short request is this many steps ahead
F_LONG = T + 2 * STRIDE


def _diffusion6():
    return Q._diffusion('ddim6')


def _request_edit():
    """the long request's edit, request-global [F_LONG, C]: keyframes on shared frames (19: windows 0 | 1; 38, 41: windows 1 | 2) and
    off them, plus a channel range over frames 8 .. 44 (through both seams); gt seeded"""
    keep = torch.zeros(F_LONG, C, dtype=torch.bool)
    keep[[0, 3, STRIDE + 1, 30, 2 * STRIDE + 2, 2 * STRIDE + 5, F_LONG - 1]] = True
    keep[8:45, 3:50] = True
    gt = torch.randn(F_LONG, C, generator=torch.Generator().manual_seed(41))
    return gt, keep


def _ctx_walk(nm, mode, layout, edit=True, table=True, ticks=LEAD + WALK):
    """Q._ctx_walk on ddim6 with the long request's edit uploaded at its admission, the way the batcher does it (every window its slice
    of the request-global edit, both copies of a shared frame equal; gt NaN where nothing is kept).  The short request (scale 2.0, no
    edit) starts LEAD ticks earlier; past the end of its walk its row restarts at position 0.
    -> per tick with the long request: (x before, schedule index per row, x after, x0)"""
    d = _diffusion6()
    long_rows, short_row = LAYOUTS[layout]
    right, first = Q._table(long_rows)
    xfs = Q._xf(2, 60)
    xf = torch.stack([xfs[1] if b == short_row else xfs[0] for b in range(CB)]).cuda()
    mask = torch.ones(CB, T, device='cuda')
    seeds = [SEED_S if b == short_row else SEED_L for b in range(CB)]
    walks = {False: Q._walk_coefs(d, mode, 2.0), True: Q._walk_coefs(d, mode, SMALL['scale'])}
    gt_r, keep_r = _request_edit()
    G, K = SE.window_tables(gt_r.numpy(), keep_r.numpy(), [j * STRIDE for j in range(3)], T)
    gt = torch.full((CB, T, C), NAN)
    keep = torch.zeros(CB, T, C, dtype=torch.bool)
    for j, b in enumerate(long_rows):
        keep[b] = torch.from_numpy(K[j])
        gt[b][keep[b]] = torch.from_numpy(G[j])[keep[b]]
    ctx = nm.context(CB, T, max_steps=d.num_timesteps)
    out = []
    try:
        ctx.set_capacity_factor(0)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_condition(xf, mask)
        ctx.set_row_seeds(seeds)
        ctx.set_long_edits(True)
        x = torch.zeros(CB, T, C, device='cuda')
        x[short_row] = Q._field(SEED_S, 0, T * C).view(T, C)
        x0 = torch.empty_like(x)
        for k in range(ticks):
            if k == LEAD:
                ctx.set_condition_rows(xf, mask, [b != short_row for b in range(CB)])
                z = Q._field(SEED_L, 0, F_LONG * C).view(-1, C)
                for b in long_rows:
                    x[b] = z[first[b]:first[b] + T]
                if edit:
                    ctx.set_edit_rows(gt.cuda(), keep.cuda())
                if table:
                    ctx.set_seam_rows(right, first, OV)
            pos = [(k % WALK) if b == short_row else max(k - LEAD, 0) for b in range(CB)]
            if k % WALK == 0 and k:
                ctx.set_condition_rows(xf, mask, [b == short_row for b in range(CB)])      # (the short row restarts: a first step again)
                x[short_row] = Q._field(SEED_S, 0, T * C).view(T, C)
            idx = [d.num_timesteps - 1 - p for p in pos]
            coefs = [walks[b != short_row][p] for b, p in enumerate(pos)]
            before = x.clone()
            ctx.sample_rows(x, [idx], [coefs], draws=None if mode == 'dpmpp' else [[1 + p for p in pos]], x0=x0)
            torch.cuda.synchronize()
            if k >= LEAD:
                out.append((before.cpu(), idx, x.clone().cpu(), x0.clone().cpu()))
        ctx.check()
    finally:
        ctx.close()
    return out, gt, keep


@pytest.fixture(scope='module')
def edit_walks(small):
    sd, arch = small
    nm = arch.model.native
    return {(mode, layout, edit, table): _ctx_walk(nm, mode, layout, edit, table)
            for mode in ('ddim', 'dpmpp') for layout, edit, table in (('scattered', True, True), ('packed', True, True), ('scattered', False, False))}


@pytest.mark.parametrize('mode', ['ddim', 'dpmpp'])
def test_context_long_edited_request_in_rows_2_0_3_beside_a_short_one(edit_walks, mode):
    (sc, gt, keep), (pk, gt_p, keep_p), (plain, _, _) = (edit_walks[(mode, l, e, t)] for l, e, t in
                                                        (('scattered', True, True), ('packed', True, True), ('scattered', False, False)))
    (rows_s, short_s), (rows_p, short_p) = LAYOUTS['scattered'], LAYOUTS['packed']
    table = SR.plan_rows(*Q._table(rows_s), T, OV)
    assert SR.pairs(table) == [(0, 3), (2, 0)]
    seam = torch.from_numpy(SR.seam_mask(table, T, OV))[:, :, None].expand(CB, T, C)
    assert bool((keep & seam).any()) and bool((keep & ~seam).any()) and not bool(keep[short_s].any())
    for l, r in SR.pairs(table):                                           # the tables agree on both copies, as the batcher builds them
        assert torch.equal(keep[l, T - OV:], keep[r, :OV])
    for k in range(WALK):
        before, idx, x, x0 = sc[k]
        assert idx[short_s] != idx[rows_s[0]] and bool(torch.isfinite(x).all()) and bool(torch.isfinite(x0).all())
        assert SR.seams_equal(x.numpy(), table, OV) and SR.seams_equal(x0.numpy(), table, OV), (mode, k)      # after every tick
        assert torch.equal(x0[keep], gt[keep])                                                               # x0 of a kept element is gt
        assert torch.equal(x[short_s], plain[k][2][short_s]) and torch.equal(x0[short_s], plain[k][3][short_s])   # the short row never notices
        assert torch.equal(x[short_s], pk[k][2][short_p])
        assert torch.equal(Q._stitched(x, rows_s), Q._stitched(pk[k][2], rows_p)), (mode, k)     # the rows a request lands in do not matter
        assert torch.equal(Q._stitched(x0, rows_s), Q._stitched(pk[k][3], rows_p))
    x_end = sc[-1][2]
    assert sc[-1][1][rows_s[0]] == 0                                       # the long request reached schedule index 0
    assert torch.equal(x_end[keep], gt[keep])                              # the kept region IS gt, in every copy
    gt_r, keep_r = _request_edit()
    st = Q._stitched(x_end, rows_s)
    assert tuple(st.shape) == (F_LONG, C) and torch.equal(st[keep_r], gt_r[keep_r])
    fr = ~keep[rows_s[1]]
    assert float((x_end[rows_s[1]][fr] - plain[-1][2][rows_s[1]][fr]).abs().max()) > 1e-3      # the free region was generated around it


@pytest.mark.parametrize('mode', ['ddim', 'dpmpp'])
def test_context_x0_meets_the_oracle_blended_then_selected(small, edit_walks, mode):
    """teacher-forced: at the device's own x of every tick the oracle's per-row x0 (each row at its own timestep and scale), blended in
    fp64 and then replaced by gt where kept -- both steps add nothing to the denoiser's bound"""
    sd, _ = small
    d = _diffusion6()
    rows_s, short_s = LAYOUTS['scattered']
    table = SR.plan_rows(*Q._table(rows_s), T, OV)
    walk, gt, keep = edit_walks[(mode, 'scattered', True, True)]
    xfs = Q._xf(2, 60)
    xf = torch.stack([xfs[1] if b == short_s else xfs[0] for b in range(CB)])
    torch.set_num_threads(4)
    worst = 0.0
    for before, idx, _, x0 in walk[:4]:
        ts = [int(d.timestep_map[i]) for i in idx]
        scales = [2.0 if b == short_s else SMALL['scale'] for b in range(CB)]
        ref = rowstep_ref.denoise_rows(sd, SMALL, before, ts, xf, torch.ones(CB, T), capacity_factor=float(SMALL['E']), scales=scales)
        want = np.where(keep.numpy(), np.nan_to_num(f64(gt)), SR.blend(ref.double().numpy(), table, OV))
        worst = max(worst, float(np.abs(f64(x0) - want).max()))
    print(f'{mode}: worst |x0 - blended, selected oracle| over 4 ticks {worst:.2e}')
    assert worst <= TOL_STEP


def _golden_walk(nm, mode, Bc, cf, tables):
    """tests/golden/edit_small.npz in rows 0, 1 of a context of Bc rows with the switch on; rows 2, 3 (Bc = 4) are the two windows of one
    more request.  -> {table: final x of the golden rows} for every row seam table in ``tables`` (None: no table), gt, keep, reference"""
    z = np.load(os.path.join(HERE, 'golden', 'edit_small.npz'))
    x_T, xf, mask = (torch.from_numpy(z[k]) for k in ('x_T', 'xf_out', 'motion_mask'))
    Bn = x_T.shape[0]
    assert tuple(x_T.shape) == (2, T, C)
    gt, keep = torch.zeros(Bc, T, C), torch.zeros(Bc, T, C, dtype=torch.bool)
    gt[:Bn], keep[:Bn] = torch.from_numpy(z['gt']), torch.from_numpy(z['keep'])
    d = Q._diffusion('ddim10' if mode == 'ddim' else '10')
    idx = list(range(10))[::-1]
    coefs = [d.step_coefs(i, mode, SMALL['scale'], 0.0) for i in idx]
    seeds = ([int(s) for s in z['seeds']] + [SEED_L, SEED_L])[:Bc]
    xfc, maskc = torch.cat([xf, xf])[:Bc].cuda(), torch.cat([mask, torch.ones(2, T)])[:Bc].cuda()
    got = {}
    ctx = nm.context(Bc, T, max_steps=10)
    try:
        if cf is not None:
            ctx.set_capacity_factor(cf)
        ctx.set_timesteps(d.timestep_map)
        ctx.set_long_edits(True)
        for name, table in tables.items():
            ctx.set_condition(xfc, maskc)
            ctx.set_row_seeds(seeds)
            x = torch.zeros(Bc, T, C, device='cuda')
            x[:Bn] = x_T.cuda()
            if Bc > Bn:
                zf = Q._field(SEED_L, 0, (STRIDE + T) * C).view(-1, C)
                x[2], x[3] = zf[:T], zf[STRIDE:STRIDE + T]
            ctx.set_edit_rows(gt.cuda(), keep.cuda())
            if table is not None:
                ctx.set_seam_rows(table[0], table[1], OV)
            ctx.sample_rows(x, [[i] * Bc for i in idx], [[c] * Bc for c in coefs], draws=[[1 + k] * Bc for k in range(10)])
            torch.cuda.synchronize()
            got[name] = x.cpu()
            ctx.clear_seam_rows()
            ctx.clear_edit_rows()
        ctx.check()
    finally:
        ctx.close()
    return got, gt, keep, torch.from_numpy(z[f'final_{mode}'])


@pytest.mark.parametrize('mode', ['ddim', 'ddpm'])
def test_golden_edit_walk_through_the_new_kernel(small, mode):
    """tests/golden/edit_small.npz (the reference's own loops with a kept region) through a context with the switch on and a row seam
    table set, so that sampler_seam_edit_rows_k runs on the golden rows.

    (1) B = 4, capacity factor 0, the table couples rows 2 and 3 only: the golden rows are bit-equal to the same walk without the seam
        table, and their kept region equals gt bit for bit.
    (2) the reference's result within the end-to-end 1e-3: at the golden's own setting, B = 2 at the model's capacity factor, under a
        row seam table that couples no row at all -- the new kernel still runs on both rows -- and again bit-equal to no table.
    Why (2) is not asserted on the walk of (1): the golden was recorded with the reference's token drops at B = 2 (whole-batch ranking
    at capacity factor 1.5).  Measured on the MI355X, |hip - reference| of the edit-only walk (no seam table, the parent's kernels) is
    3.3e-06 at B = 2 / default capacity factor, 6.9e-01 at capacity factor 0 (B = 2 and B = 4 alike) and 4.6e-01 at B = 4 / default:
    the distance is the routing's, whatever sampler kernel runs, and no four-row context can reproduce the two-row call's drops."""
    sd, arch = small
    nm = arch.model.native
    got, gt, keep, _ = _golden_walk(nm, mode, CB, 0, dict(none=None, other_rows=([-1, -1, 3, -1], [0, 0, 0, STRIDE])))
    assert torch.equal(got['other_rows'][:2], got['none'][:2])
    assert not torch.equal(got['other_rows'][2:], got['none'][2:])         # (the coupled rows did run coupled)
    assert torch.equal(got['other_rows'][keep], gt[keep])
    got2, gt2, keep2, ref = _golden_walk(nm, mode, 2, None, dict(none=None, no_chain=([-1, -1], [0, 0])))
    err = float((got2['no_chain'] - ref).abs().max())
    print(f'edit golden {mode} through sampler_seam_edit_rows_k: |hip - reference| {err:.2e}; at B = 4, capacity factor 0: '
          f'{float((got["other_rows"][:2] - ref).abs().max()):.2e}')
    assert torch.equal(got2['no_chain'], got2['none'])
    assert err <= TOL_E2E
    assert torch.equal(got2['no_chain'][keep2], gt2[keep2])


def test_the_switch(small):
    L_, lib, _ptr, _stream = Q._lib()
    sd, arch = small
    nm = arch.model.native
    d = Q._diffusion()
    idx = list(range(d.num_timesteps))[::-1]
    ddim = [d.step_coefs(i, 'ddim', SMALL['scale']) for i in idx]
    rows_s, short_s = LAYOUTS['scattered']
    right, first = Q._table(rows_s)
    gt_r, keep_r = _request_edit()
    G, K = SE.window_tables(gt_r.numpy(), keep_r.numpy(), [j * STRIDE for j in range(3)], T)
    gt, keep = torch.zeros(CB, T, C), torch.zeros(CB, T, C, dtype=torch.uint8)
    for j, b in enumerate(rows_s):
        gt[b], keep[b] = torch.from_numpy(G[j]), torch.from_numpy(K[j]).to(torch.uint8)
    gt, keep = gt.cuda(), keep.cuda()
    ctx = nm.context(CB, T, max_steps=10)
    ctx.set_capacity_factor(0)
    ctx.set_timesteps(d.timestep_map)
    ctx.set_condition(Q._xf(CB, 61).cuda(), torch.ones(CB, T, device='cuda'))
    ctx.set_row_seeds([SEED_S if b == short_s else SEED_L for b in range(CB)])
    x = torch.randn(CB, T, C, generator=torch.Generator().manual_seed(5)).cuda()
    x = torch.from_numpy(SR.share_left(x.cpu().numpy(), SR.plan_rows(right, first, T, OV), OV)).float().cuda()

    def code(rc):
        return pytest.raises(RuntimeError, match=rf'\(code {rc}\)')

    def tick(rows_idx=None, draws=None, xx=None, noise=None):
        xx = x.clone() if xx is None else xx
        ctx.sample_rows(xx, [rows_idx or [9] * CB], [[ddim[0]] * CB], draws=None if noise is not None else [draws or [1] * CB], noise=noise)
        torch.cuda.synchronize()
        return xx
    try:
        # off (the default): both mutual refusals as ever
        assert ctx.long_edits is False
        ctx.set_edit_rows(gt, keep)
        with code(L_.MC_ERR_STATE):
            ctx.set_seam_rows(right, first, OV)
        assert 'edit table' in L_.last_error()
        edit_only = tick()
        ctx.clear_edit_rows()
        ctx.set_seam_rows(right, first, OV)
        with code(L_.MC_ERR_STATE):
            ctx.set_edit_rows(gt, keep)
        assert 'row seam table' in L_.last_error()
        seam_only = tick()
        # on: both orders are accepted, and the tick is neither table's alone
        ctx.set_long_edits(True)
        ctx.set_edit_rows(gt, keep)                                        # beside a row seam table
        want = tick()
        assert not torch.equal(want, seam_only) and not torch.equal(want, edit_only)
        ctx.clear_seam_rows()
        ctx.set_seam_rows(right, first, OV)                                # beside an edit table
        assert torch.equal(tick(), want)
        # still refused with the switch on; the context is unchanged by each
        nz = torch.zeros_like(x)
        for call in (lambda: ctx.sample_step(x, idx[0], ddim[0], nz), lambda: ctx.sample_loop(x.clone(), idx[:2], ddim[:2], noise=torch.zeros(2, CB, T, C, device='cuda')),
                     lambda: ctx.sample_step_inpaint(x, idx[0], ddim[0], nz, nz, torch.zeros(CB, T, C, dtype=torch.bool, device='cuda'), gt_noise=nz),
                     lambda: ctx.sample_step_seeded(x, idx[0], ddim[0], nz, 1.0, 0.0),
                     lambda: ctx.set_seams([0, STRIDE, 2 * STRIDE, 100], OV)):
            with code(L_.MC_ERR_STATE):
                call()
        assert lib.mc_ctx_graph_step(ctx.handle, 0, _stream()) == L_.MC_ERR_STATE
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            gx, gn = torch.empty_like(x), torch.zeros_like(x)
            with code(L_.MC_ERR_STATE):
                ctx.graph_capture(gx, gn, ddim[::-1])
        torch.cuda.current_stream().wait_stream(side)
        xx = x.clone()
        with code(L_.MC_ERR_ARG):                                          # mode 1 with a noise tensor beside an edit table
            tick(xx=xx, noise=nz[None])
        for kw in (dict(rows_idx=[9, 9, 8, 9]), dict(draws=[1, 1, 1, 2])):  # the seam-pair checks
            with code(L_.MC_ERR_ARG):
                tick(xx=xx, **kw)
            assert 'share a seam' in L_.last_error()
        assert torch.equal(xx, x)
        with code(L_.MC_ERR_STATE):                                        # switching off while both tables are set
            ctx.set_long_edits(False)
        assert 'mc_ctx_set_long_edits' in L_.last_error() and ctx.long_edits is True
        assert torch.equal(tick(), want)                                   # after all of them: the same bits
        # a captured graph or the whole-batch seam table in the context still refuse either table
        ctx.clear_seam_rows()
        ctx.clear_edit_rows()
        ctx.set_seams([0, STRIDE, 2 * STRIDE, 100], OV)
        with code(L_.MC_ERR_STATE):
            ctx.set_edit_rows(gt, keep)
        with code(L_.MC_ERR_STATE):
            ctx.set_seam_rows(right, first, OV)
        ctx.clear_seams()
        with torch.cuda.stream(side):
            ctx.graph_capture(gx, gn, ddim[::-1])
            with code(L_.MC_ERR_STATE):
                ctx.set_edit_rows(gt, keep)
            with code(L_.MC_ERR_STATE):
                ctx.set_seam_rows(right, first, OV)
            ctx.graph_release()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # one table set: switching off is fine, and the refusals are back
        ctx.set_edit_rows(gt, keep)
        ctx.set_long_edits(False)
        with code(L_.MC_ERR_STATE):
            ctx.set_seam_rows(right, first, OV)
        assert torch.equal(tick(), edit_only)
    finally:
        ctx.close()


# ---- the batcher --------------------------------------------------------------------------------------------------------------------
def _serve(arch, arrivals, sampler='ddim', batch=CB, steps=6, eta=0.5):
    """arrivals: [(tick, Request)] -> ({id(request): result}, {id(request): rows}, the batcher)"""
    from motioncraft_amd.serve import ContinuousBatcher
    bt = ContinuousBatcher(arch, batch=batch, frames=T, sampler=sampler, steps=steps, eta=eta, overlap=OV, long_edits=True)
    rows, out, k, hs = {}, {}, 0, {}
    for _ in range(60):
        while k < len(arrivals) and arrivals[k][0] <= bt.ticks:
            hs[bt.submit(arrivals[k][1])] = arrivals[k][1]
            k += 1
        bt.tick()
        for b, h_ in enumerate(bt.occupied):
            if h_ is not None:
                rows.setdefault(h_, set()).add(b)
        out.update(bt.poll())
        if k == len(arrivals) and not any(h_ is not None for h_ in bt.occupied):
            break
    torch.cuda.synchronize()
    return {id(r): out[h].clone() for h, r in hs.items()}, {id(r): (sorted(rows[h]), bt.submitted_at[h], bt.finished_at[h]) for h, r in hs.items()}, bt


def _long_edit(n=F_LONG):
    from motioncraft_amd.serve import Edit
    gt_r, keep_r = _request_edit()
    return Edit(gt_r[:n].clone(), keep_r[:n].clone())


def _request(F, seed, xf_seed, edit=None, scale=None):
    from motioncraft_amd.serve import Request
    return Request(length=F, seed=seed, xf_out=Q._xf(1, xf_seed)[0], guidance_scale=scale, edit=edit)


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp'])
def test_a_long_edited_request_joining_at_tick_3_gets_the_bits_it_gets_alone(small, sampler):
    sd, arch = small
    assert arch.model.post_process_cfg is None                             # (data space = model space in the test config)
    e = _long_edit()
    R = _request(F_LONG, SEED_L, 70, edit=e)
    other = _request(17, 5, 71, scale=1.25)
    alone, where_a, _ = _serve(arch, [(0, R)], sampler=sampler)
    joined, where_j, bt = _serve(arch, [(0, other), (3, R)], sampler=sampler)
    assert where_a[id(R)] == ([0, 1, 2], 0, 6) and where_j[id(R)] == ([1, 2, 3], 3, 9)
    got = alone[id(R)]
    assert tuple(got.shape) == (F_LONG, C) and bool(torch.isfinite(got).all())
    assert torch.equal(got, joined[id(R)]), float((got - joined[id(R)]).abs().max())
    assert torch.equal(got.cpu()[e.keep], e.motion[e.keep])                # the kept elements ARE the given ones
    assert bt.runner.ctx.seam_rows is None and not bt.runner.ctx.edit_rows and bt.runner.ctx.long_edits


def test_a_long_request_keeps_its_bits_beside_a_short_edited_one(small):
    """the co-residency that used to wait: L (no edit) alone, and L admitted at tick 0 beside a short edited request mid-walk"""
    from motioncraft_amd.serve import Edit
    sd, arch = small
    L = _request(F_LONG, SEED_L, 70)
    m = torch.randn(20, C, generator=torch.Generator().manual_seed(43))
    E = _request(20, 9, 72, edit=Edit.keyframes(m, [0, 7, 19]))
    alone, where_a, _ = _serve(arch, [(0, L)])
    both, where_b, _ = _serve(arch, [(0, E), (2, L)])
    assert where_b[id(E)] == ([0], 0, 6) and where_b[id(L)] == ([1, 2, 3], 2, 8)            # L did not wait for E to retire
    assert torch.equal(alone[id(L)], both[id(L)]), float((alone[id(L)] - both[id(L)]).abs().max())
    assert torch.equal(both[id(E)].cpu()[[0, 7, 19]], m[[0, 7, 19]])
    late, where_l, _ = _serve(arch, [(0, L), (2, E)])                      # ... and the other way round: E joins beside the running L
    assert where_l[id(E)] == ([3], 2, 8)
    assert torch.equal(late[id(L)], alone[id(L)]) and torch.equal(late[id(E)], both[id(E)])


def test_a_ragged_last_window_and_an_edit_shorter_than_the_request(small):
    sd, arch = small
    F = F_LONG - 7                                                         # windows of 24, 24, 17 frames
    e = _long_edit(40)                                                     # the edit ends inside window 2's head: frames 40 .. F - 1 are free
    R = _request(F, SEED_L, 70, edit=e)
    plain = _request(F, SEED_L, 70)
    got, where, _ = _serve(arch, [(0, R)], batch=3)
    ref, _, _ = _serve(arch, [(0, plain)], batch=3)
    y, y0 = got[id(R)].cpu(), ref[id(plain)].cpu()
    assert where[id(R)][0] == [0, 1, 2] and tuple(y.shape) == (F, C) and bool(torch.isfinite(y).all())
    assert torch.equal(y[:40][e.keep], e.motion[e.keep])
    assert float((y[:40][~e.keep] - y0[:40][~e.keep]).abs().max()) > 1e-3                  # generated around the edit
    assert float((y[45:] - y0[45:]).abs().max()) > 0                       # (the free tail is this request's own walk, coupled to the edited part)

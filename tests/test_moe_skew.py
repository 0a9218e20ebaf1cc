"""GPU (MI355X): the motion MoE -- gate, batch-prioritised capacity routing, expert MLPs, combine + MOE.proj -- at the full
batch sizes under gates that route like a trained checkpoint (tests/helpers.skew_gates), each stage against a plain
reference of the same operation computed from the kernels' own inputs:

  R1  keep flags (comb_w != 0) == helpers.bpr_keep(idx, key): exact integer decision, both tie policies;
  R2  idx / gate / key vs the cosine_top gate in fp64 from the kernel's own z (observed: gate <= 2e-7, key <= 5 x 2^-23 of
      the top score at the default logit scale 2, <= 40 x at the hot-pair scale 20);
  R3  y2 of every kept (token, choice) vs FC2(gelu(FC1(z))) of its expert in fp64 (dropped pairs' rows are never written,
      never read);
  R4  mf vs GELU(sum_k w_k y2_k) Wproj^T + b in fp64 from the kernel's own y2 and comb_w (pqbody_k writes every mf column
      at these sizes: the whole row is compared); a token with both choices dropped gives exactly the bias.

Each layer l is read after ``denoise(x, 0, stop_after_layers=l + 1)`` (no CFG-twin aliasing, every row materialised).  In
base layer 0 under the stable tie order the routing runs in twin mode: gate outputs, z and expert rows exist for the first
CFG half only, token i + N/2 is the twin of token i (same scores, own index, own keep flags).  The fp64 references run
on the device through torch (float64 GEMMs), which keeps the module within its time budget."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import FULL, bpr_keep, key_bits, skew_gates, synth_inputs

pytestmark = pytest.mark.gpu

DEFAULT_CHAIN = 762806311                      # kChainDefault (mc_options.h)
TOL_STEP = 2e-4
TAU = 1e-5                                     # R2: a token is "decided" when both fp64 gaps (1st-2nd, 2nd-3rd) exceed TAU * s1
M2D = dict(FULL, L=64, F=256)                  # the L = 64 width (W.default_dims(L=64, F=256))
MOE = 'temporal_decoder_blocks.{}.ca_block.motion_moe.'


def _lengths(B, T, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [int(v) for v in torch.randint(T // 3, T + 1, (B,), generator=g)]


@pytest.fixture(scope='module')
def models():
    """(dims name, gate kind) -> (state dict, NativeModel), each built once for the module."""
    from motioncraft_amd.engine import NativeModel
    from oracle import weights as W
    base, made = {}, {}

    def get(name, kind):
        if (name, kind) not in made:
            dims = {'FULL': FULL, 'M2D': M2D}[name]
            if name not in base:
                base[name] = W.make_state_dict(dims, 0)
            sd = skew_gates(base[name], dims, kind)
            made[(name, kind)] = (sd, NativeModel(dims, sd, cfg_scale=dims['scale']))
        return made[(name, kind)]
    yield get
    for _, nm in made.values():
        nm.close()


def _stats(idx, keep, E, capacity):
    kept = np.bincount(idx[keep], minlength=E)
    return dict(drop0=float((~keep[:, 0]).mean()), drop1=float((~keep[:, 1]).mean()), empty=int((kept == 0).sum()),
                at_cap=int((kept == capacity).sum()), kept=kept)


def check_layer(ctx, sd, dims, l, B, T, x, kind, tie):
    """R1 - R4 for layer l of ``ctx`` (state dict ``sd``); returns the measured numbers."""
    torch.cuda.synchronize()
    ctx.denoise(x, 0, stop_after_layers=l + 1)
    torch.cuda.synchronize()
    L, H, E = dims['L'], dims['H'], dims['E']
    N = 2 * B * T * H
    twin = l == 0 and tie == 'stable'
    ns = N // 2 if twin else N                                # tokens with their own gate outputs / expert rows
    dev = 'cuda'
    idx = ctx.buffer('idx', dtype=torch.int32)[:2 * ns].view(ns, 2).long()
    gate = ctx.buffer('gate')[:2 * ns].view(ns, 2)
    key = ctx.buffer('key', dtype=torch.int32)[:ns]
    z = ctx.buffer('z')[:ns * L].view(ns, L)
    comb_w = ctx.buffer('comb_w').view(N, 2)
    y2 = ctx.buffer('y2').view(N, 2, L)
    mf = ctx.buffer('mf').view(N, 4 * L)
    if twin:
        idx_all, key_all, gate_all = idx.repeat(2, 1), key.repeat(2), gate.repeat(2, 1)
    else:
        idx_all, key_all, gate_all = idx, key, gate
    from oracle import tutel_restated as TR
    capacity = TR.capacity_of(N, E, 2, 1.5)
    out = dict(layer=l)

    # ---- R1: the drop decision, exact ----
    assert bool((gate > 0).all()), 'a zero gate would hide its keep flag in comb_w'
    keep_hip = (comb_w != 0).cpu().numpy()
    idx_np = idx_all.cpu().numpy()
    keep_ref = bpr_keep(idx_np, key_all.cpu(), E, capacity, tie)
    n_bad = int((keep_hip != keep_ref).sum())
    assert n_bad == 0, f'layer {l}: {n_bad} keep flags differ from the BPR reference ({kind}, {tie})'
    keep_t = torch.from_numpy(keep_ref).to(dev)
    assert torch.equal(comb_w[keep_t], gate_all[keep_t])           # a kept pair's combine weight is its renormalised gate
    st = _stats(idx_np, keep_ref, E, capacity)
    out.update({k: v for k, v in st.items() if k != 'kept'})
    if kind == 'hot_pair':
        assert st['drop1'] >= 0.15 and st['drop0'] >= 0.01 and st['empty'] >= 1 and st['at_cap'] >= 1, (l, st)
    if kind == 'all_ties':
        e0, e1 = int(idx_np[0, 0]), int(idx_np[0, 1])
        assert (idx_np[:, 0] == e0).all() and (idx_np[:, 1] == e1).all() and e0 != e1
        assert st['empty'] == E - 2 and st['kept'][e0] == capacity and st['kept'][e1] == capacity, (l, st)
        want = np.zeros(N, dtype=bool)
        want[:capacity] = True
        if tie == 'reverse':
            want = want[::-1]
        assert np.array_equal(keep_ref[:, 0], want) and np.array_equal(keep_ref[:, 1], want)

    # ---- R2: the gate vs fp64 from the kernel's own z ----
    m = MOE.format(l) + 'model.gates.0.'
    sc = TR.gate_scores(z.double(), sd[m + 'cosine_projector.weight'].to(dev), sd[m + 'cosine_projector.bias'].to(dev),
                        sd[m + 'sim_matrix'].to(dev), sd[m + 'temperature'].to(dev))
    top = torch.topk(sc, 3, dim=1)
    s1 = top.values[:, 0]
    decided = ((top.values[:, 0] - top.values[:, 1]) > TAU * s1) & ((top.values[:, 1] - top.values[:, 2]) > TAU * s1)
    undecided = int((~decided).sum())
    idx_flip = int((idx != top.indices[:, :2]).any(1)[decided].sum())
    g_sel = sc.gather(1, idx)
    gate_ref = g_sel / g_sel.sum(1, keepdim=True).clamp_min(torch.finfo(torch.float32).eps)
    key_f = torch.from_numpy(key_bits(key).view(np.float32).copy()).to(dev).double()
    out['r2_undecided'] = undecided
    out['r2_gate'] = float((gate.double() - gate_ref).abs().max())
    out['r2_key_ulp'] = float(((key_f - s1).abs() / (s1 * 2.0 ** -23)).max())      # in units of 2^-23 * s1 (<= 1 ulp of s1)
    assert idx_flip == 0, f'layer {l}: {idx_flip} decided tokens with another top-2 than fp64'
    assert undecided <= max(8, ns // 1000), (l, undecided)
    assert out['r2_gate'] <= 1e-5, out
    # an fp32 softmax carries the logits' rounding (~ulp x logit scale) into every score: the key bound scales with it
    scale = float(torch.clamp(sd[m + 'temperature'].double(), max=np.log(100.0)).exp())
    assert out['r2_key_ulp'] <= 4 * (1 + scale), (out, scale)

    # ---- R3: expert MLP of every kept pair vs fp64 (twin layer: only the first half has expert rows) ----
    e = MOE.format(l) + 'model.experts.'
    w1, b1 = sd[e + 'batched_fc1_w'].to(dev).double(), sd[e + 'batched_fc1_bias'].to(dev).double()
    w2, b2 = sd[e + 'batched_fc2_w'].to(dev).double(), sd[e + 'batched_fc2_bias'].to(dev).double()
    kept_src = keep_t[:ns]
    r3 = 0.0
    z64 = z.double()
    for ex in range(E):
        sel = kept_src & (idx == ex)
        if not bool(sel.any()):
            continue
        tok, k = sel.nonzero(as_tuple=True)
        ref = F.gelu(z64[tok] @ w1[ex].T + b1[ex]) @ w2[ex] + b2[ex]
        err = float((y2[tok, k].double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        r3 = max(r3, err)
    out['r3'] = r3

    # ---- R4: combine + GELU + MOE.proj vs fp64 from the kernel's y2 / comb_w ----
    src = torch.arange(N, device=dev)
    if twin:
        src = src % ns                                         # a twin combines its original's expert rows (twin_from)
    ys = y2[src].double()
    w = comb_w.double()
    comb = torch.where(keep_t[:, :, None], w[:, :, None] * ys, torch.zeros((), dtype=torch.float64, device=dev)).sum(1)
    pw, pb = sd[MOE.format(l) + 'proj.weight'].to(dev).double(), sd[MOE.format(l) + 'proj.bias'].to(dev).double()
    mf_ref = F.gelu(comb) @ pw.T + pb
    out['r4'] = float((mf.double() - mf_ref).abs().max()) / max(1.0, float(mf_ref.abs().max()))
    none = ~keep_t.any(1)
    out['both_dropped'] = int(none.sum())
    if out['both_dropped']:
        assert torch.equal(mf[none], sd[MOE.format(l) + 'proj.bias'].to(dev).expand(int(none.sum()), -1)), l
    return out


def _run(models, name, kind, B, T, tie='stable', chain=None, route_coop=None, prec=None, layers=None, seed=33):
    sd, nm = models(name, kind)
    dims = nm.dims
    x, xf, mask = synth_inputs(dims, B, T, seed=seed, lengths=_lengths(B, T))
    ctx = nm.context(B, T, max_steps=1)
    try:
        if chain is not None:
            ctx.set_option('chain', chain)
        if route_coop is not None:
            ctx.set_option('route_coop', route_coop)
        if prec is not None:
            ctx.set_precision(prec)
        if tie != 'stable':
            ctx.set_tie_policy(tie)
        ctx.set_timesteps([640])
        ctx.set_condition(xf.cuda(), mask.cuda())
        coop = ctx.uses_coop_routing
        xd = x.cuda()
        res = [check_layer(ctx, sd, dims, l, B, T, xd, kind, tie) for l in (layers or range(dims['NL']))]
    finally:
        ctx.close()
    for r in res:
        print(f"{name} B={B} {kind} {tie} chain={chain} coop={coop} prec={prec}: layer {r['layer']}: dropped 1st "
              f"{r['drop0']:.4f} 2nd {r['drop1']:.4f}, empty experts {r['empty']}, at capacity {r['at_cap']}, both dropped "
              f"{r['both_dropped']}, below tau {r['r2_undecided']}, R2 gate {r['r2_gate']:.1e} key {r['r2_key_ulp']:.1f} x 2^-23 s1, "
              f"R3 {r['r3']:.2e}, R4 {r['r4']:.2e}")
    return res, coop


R3_TOL, R4_TOL = 3e-5, 3e-5


@pytest.mark.parametrize('kind,tie', [('balanced', 'stable'), ('hot_pair', 'stable'), ('all_ties', 'stable'),
                                      ('all_ties', 'reverse')])
def test_full_batch_64_skewed_routing_and_experts_vs_references(models, kind, tie):
    """B = 64 x 196, mixed lengths (301 056 tokens): gate_k<128>, route_coop_k, two slot groups, fused mlp2d_k, pqbody_k.
    Observed R3 / R4 (fp32): <= 1.4e-6 / 4.2e-7 (bound 3e-5 x max(1, max|ref|))."""
    res, coop = _run(models, 'FULL', kind, 64, 196, tie)
    assert coop
    for r in res:
        assert r['r3'] <= R3_TOL and r['r4'] <= R4_TOL, r


@pytest.mark.parametrize('arm', ['launch_sequence', 'grouped_gemm'])
def test_full_batch_64_hot_pair_other_routing_and_expert_paths(models, arm):
    """The same size and skew through the 12-launch routing sequence (route_coop 0) and through the grouped GM_EXP1 /
    GM_EXP2 expert GEMMs over a tile map dominated by two experts (chain bit 0, kChainMlp, cleared)."""
    if arm == 'launch_sequence':
        res, coop = _run(models, 'FULL', 'hot_pair', 64, 196, route_coop=0)
        assert not coop
    else:
        res, coop = _run(models, 'FULL', 'hot_pair', 64, 196, chain=DEFAULT_CHAIN & ~1)
    for r in res:
        assert r['r3'] <= R3_TOL and r['r4'] <= R4_TOL, r


def test_full_batch_16_hot_pair(models):
    """B = 16: the smallest two-stream batch, a smaller cooperative routing grid."""
    res, coop = _run(models, 'FULL', 'hot_pair', 16, 196)
    assert coop
    for r in res:
        assert r['r3'] <= R3_TOL and r['r4'] <= R4_TOL, r


@pytest.mark.parametrize('kind', ['hot_pair', 'all_ties'])
def test_batch_1_skewed_small_kernels(models, kind):
    """B = 1 x 196: gate_small_k, route_small_k, the split-hidden expert MLP whose slice count is chosen on
    the device from the real tile count -- which under skew (two experts at capacity, most others empty) is not the host's
    estimate."""
    res, coop = _run(models, 'FULL', kind, 1, 196)
    assert not coop
    for r in res:
        assert r['r3'] <= R3_TOL and r['r4'] <= R4_TOL, r


def test_m2d_width_batch_160_hot_pair(models):
    """W.default_dims(L=64, F=256) at B = 160 x 120 (921 600 pairs): gate_k<64>, the larger cooperative routing grid, the
    L = 64 expert MLP; base layers."""
    res, coop = _run(models, 'M2D', 'hot_pair', 160, 120)
    assert coop
    for r in res:
        assert r['r3'] <= R3_TOL and r['r4'] <= R4_TOL, r


def test_f16x3_expert_path_under_skew_vs_balanced(models):
    """precision f16x3 at B = 64: mlp_h and pqbody_h_k.  The hot-pair errors may be at most 4x those of the balanced gate
    at the same shape and precision (the skew must not expose an error the control does not have)."""
    bal, _ = _run(models, 'FULL', 'balanced', 64, 196, prec='f16x3')
    hot, _ = _run(models, 'FULL', 'hot_pair', 64, 196, prec='f16x3')
    for q in ('r3', 'r4'):
        b, h = max(r[q] for r in bal), max(r[q] for r in hot)
        print(f'f16x3 {q}: balanced {b:.2e}, hot_pair {h:.2e}')
        assert b <= 1e-4 and h <= 4 * b, (q, b, h)


@pytest.mark.parametrize('kind', ['hot_pair', 'all_ties'])
def test_production_layer_0_twin_dedupe_and_split_vs_oracle(models, kind):
    """A full-width model with NL = 1 at B = 64 on the production path (no stop_after_layers): twin dedupe and aliasing
    (base layer 0), the twin split (chain bit 16), the large-batch schedule.  R1 against the captured routing, the twin-split
    flag against what the reference keep flags imply (some token and its CFG twin kept differently), out2 against the
    oracle teacher-forced to the HIP routing, and two calls bit-identical."""
    from motioncraft_amd.engine import NativeModel
    from oracle import stmogen_oracle as O, tutel_restated as TR
    sd_full, _ = models('FULL', kind)
    dims = dict(FULL, NL=1)
    sd = {k: v for k, v in sd_full.items() if not k.startswith('temporal_decoder_blocks.') or k.startswith('temporal_decoder_blocks.0.')}
    B, T = 64, 196
    x, xf, mask = synth_inputs(dims, B, T, seed=33, lengths=_lengths(B, T))
    nm = NativeModel(dims, sd, cfg_scale=dims['scale'])
    ctx = nm.context(B, T, max_steps=1)
    try:
        ctx.enable_capture()
        ctx.set_timesteps([640])
        ctx.set_condition(xf.cuda(), mask.cuda())
        out2 = ctx.denoise(x.cuda(), 0)
        torch.cuda.synchronize()
        again = ctx.denoise(x.cuda(), 0)
        torch.cuda.synchronize()
        assert torch.equal(out2, again)
        flag = int(ctx.buffer('route_split', dtype=torch.int32)[0])
        N = 2 * B * T * dims['H']
        idx, keep = ctx.routing(0)
        key = ctx.buffer('key', dtype=torch.int32)[:N // 2].cpu()            # first CFG half; twins share their source's key
        ref = bpr_keep(idx.numpy(), key.repeat(2), dims['E'], TR.capacity_of(N, dims['E'], 2, 1.5), 'stable')
        assert np.array_equal(keep.numpy(), ref), int((keep.numpy() != ref).sum())
        split = bool((ref[:N // 2] != ref[N // 2:]).any())
        if kind == 'all_ties':
            assert split                                          # the cut falls inside the first CFG half
        assert bool(flag) == split, (flag, split)
        forced = [ctx.routing(0)]
    finally:
        ctx.close()
        nm.close()
    torch.set_num_threads(min(16, os.cpu_count()))
    cap = {}
    O.denoise(sd, dims, x, 640, xf, mask, forced_routing=forced, cap=cap)
    err = float((out2.cpu().double() - cap['out2'].double()).abs().max())
    print(f'production layer 0 ({kind}): twin split {split}, |out2 - oracle| {err:.2e}')
    assert err <= TOL_STEP, err

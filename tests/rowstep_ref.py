"""Per-row timesteps and guidance scales, restated from the oracle's own functions (``time_embed`` with a ``ts`` vector, ``stma``,
``sffn``, ``pose_decoder``): the body of ``stmogen_oracle._denoise`` with ``ts`` and ``w`` as vectors -- what the reference's denoiser
computes when it is handed ``ts`` as a [B] tensor (its guidance weight ``1 + scale * t / 1000`` is per sample).  Plus the per-element
fp64 sampler updates the per-row sampler kernels are held to."""
import numpy as np
import torch

from oracle import stmogen_oracle as O


def guidance_weight(t_orig, scale):
    return (1 - (1000 - int(t_orig)) / 1000) * float(scale) + 1           # stmogen.py:655-659


def denoise_rows(p, dims, x_t, ts, xf_out, motion_mask, forced_routing=None, capacity_factor=None, scales=None, out2=False):
    """x_t [B,T,C], ts [B] original (un-spaced) timesteps, one per row -> the CFG-combined x0 prediction [B,T,C] with row b under
    ``guidance_weight(ts[b], scales[b])`` (``scales`` None: the model's), or with ``out2`` both decoded halves [2B,T,C]."""
    old = O.CAPACITY_FACTOR
    if capacity_factor is not None:
        O.CAPACITY_FACTOR = float(capacity_factor)
    try:
        B, T, C = x_t.shape
        L, H, NL = dims['L'], dims['H'], dims['NL']
        ts = torch.as_tensor([int(t) for t in ts], dtype=torch.long)
        assert ts.shape == (B,)
        emb = O.time_embed(p, ts, L * H)
        h = O.pose_encoder(p, x_t, dims.get('dataset', 'motionx')) + p['sequence_embedding'].unsqueeze(0)[:, :T, :]
        cond = torch.cat((torch.ones(B, 1, 1), torch.zeros(B, 1, 1)), dim=0)
        h = h.repeat(2, 1, 1)
        xf2 = xf_out.repeat(2, 1, 1)
        emb2 = emb.repeat(2, 1)
        mask2 = motion_mask.reshape(B, T).repeat(2, 1)
        for i in range(NL):
            pre = f'temporal_decoder_blocks.{i}.'
            h = O.stma(p, pre + 'ca_block.', h, xf2, emb2, mask2, cond, dims, forced=None if forced_routing is None else forced_routing[i])
            h = O.sffn(p, pre + 'ffn.', h, emb2, dims)
        out = O.pose_decoder(p, h, L, C, dims.get('dataset', 'motionx')).view(2 * B, T, -1)
        if out2:
            return out
        scales = [dims['scale']] * B if scales is None else scales
        w = torch.tensor([guidance_weight(t, s) for t, s in zip(ts.tolist(), scales)], dtype=out.dtype).view(B, 1, 1)
        return out[:B] * w + out[B:] * (1 - w)
    finally:
        O.CAPACITY_FACTOR = old


# ---- the sampler updates per element, fp64 (mc_kernels.hip: sampler_elem / multistep_elem over x0 = a + b) ----
def coefs_dict(c):
    return {k: float(getattr(c, k)) for k in ('text_coef', 'none_coef', 'c1', 'c2', 'log_var', 'sqrt_recip', 'sqrt_recipm1', 'ab',
                                              'ab_prev', 'eta', 'nonzero')} | {'mode': int(c.mode)}


def sampler_rows(x, a, b, noise, hist, coefs, TC):
    """flat fp64 arrays [B * TC]; element e takes ``coefs[e // TC]`` -> (x_prev, x0); mode 2 reads ``hist`` where the row's eta != 0"""
    x, a, b = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (x, a, b))
    x0 = a + b
    out = np.empty_like(x)
    for r, c in enumerate(coefs):
        k = coefs_dict(c) if not isinstance(c, dict) else c
        s = slice(r * TC, (r + 1) * TC)
        if k['mode'] == 2:
            hp = np.asarray(hist, dtype=np.float64).reshape(-1)[s] if k['eta'] != 0 else 0.0
            out[s] = k['eta'] * hp + k['c2'] * x[s] + k['c1'] * x0[s]
            continue
        nz = np.asarray(noise, dtype=np.float64).reshape(-1)[s]
        if k['mode'] == 0:
            out[s] = k['c1'] * x0[s] + k['c2'] * x[s] + k['nonzero'] * np.exp(0.5 * k['log_var']) * nz
        else:
            sigma = k['eta'] * np.sqrt((1 - k['ab_prev']) / (1 - k['ab'])) * np.sqrt(1 - k['ab'] / k['ab_prev'])
            eps = (k['sqrt_recip'] * x[s] - x0[s]) / k['sqrt_recipm1']
            out[s] = x0[s] * np.sqrt(k['ab_prev']) + np.sqrt(1 - k['ab_prev'] - sigma ** 2) * eps + k['nonzero'] * sigma * nz
    return out, x0

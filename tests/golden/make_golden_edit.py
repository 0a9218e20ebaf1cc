"""Regenerates tests/golden/edit_small.npz: the reference's own sampler loops with a kept region (model_kwargs['y'] = {gt,
outpainting_mask}: gaussian_diffusion.py:492-501, 855-877) on row-keyed noise -- what ``mc_ctx_set_edit_rows`` + ``mc_sample_rows``
compute.  Needs the reference tree (oracle/ref_shim.py), like make_golden.py; stores inputs and the reference's
outputs only.

  SMALL weights (SMALL_SEED, unskewed), B = 2, T = 24, lengths (24, 21); keep = frames {0, 1, 11, 23} on all channels plus the lleg /
  rleg / root channels on frames 4-8; gt seeded.
  ddim_sample_loop (respace 'ddim10', eta 0, no_repaint=True, addBlend=False) and p_sample_loop (respace '10').
  th.randn_like is patched for the run: row b of the k-th step's noise is draw 1 + k of seeds[b] (oracle/philox_oracle.draw_normal),
  the kept region's second draw of that step (DDIM) is draw (1 + k) ^ 2^63; x_T is draw 0.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import philox_oracle, ref_shim, stmogen_oracle as O  # noqa: E402
from make_golden import SMALL, SMALL_SEED, build_ref, maxabs, model_kwargs, synth_inputs  # noqa: E402
from motioncraft_amd.synthetic import part_layout  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEEDS = [2024, 2 ** 63 + 77]
FLIP = 1 << 63
BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')


def row_draw(shape, d):
    B, T, C = shape
    return torch.from_numpy(np.stack([philox_oracle.draw_normal(T * C, SEEDS[b], d)[:T * C].reshape(T, C) for b in range(B)]))


class Draws:
    """stands in for th.randn_like during one loop: the reference's order is step noise, then (DDIM, kept region) the second draw"""

    def __init__(self, per_step):
        self.per_step, self.n, self.log = per_step, 0, []

    def __call__(self, x, **kw):
        k, second = divmod(self.n, self.per_step)
        self.n += 1
        d = (1 + k) ^ (FLIP if second else 0)
        self.log.append(d)
        return row_draw(tuple(x.shape), d).to(x.dtype)


def main():
    dims, B, T = SMALL, 2, 24
    C = dims['input_feats']
    m, sd = build_ref(dims, SMALL_SEED)
    _, xf, mask = synth_inputs(dims, B, T, seed=51, lengths=[24, 21])
    x_T = row_draw((B, T, C), 0)
    _, channels, _ = part_layout('motionx')
    keep = torch.zeros(B, T, C, dtype=torch.bool)
    keep[:, [0, 1, 11, 23]] = True
    cols = sorted({c for n in ('lleg', 'rleg', 'root') for c in channels[n]})
    keep[:, 4:9, cols] = True
    gt = torch.randn(B, T, C, generator=torch.Generator().manual_seed(52))
    save = dict(x_T=x_T.numpy(), xf_out=xf.numpy(), motion_mask=mask.numpy(), gt=gt.numpy(), keep=keep.numpy(),
                seeds=np.array(SEEDS, dtype=np.uint64))
    opt = types.SimpleNamespace(same_overlap_noisy=False, no_repaint=True, addBlend=False, overlap_len=0, no_resample=True, jump_length=3,
                                jump_n_sample=5, timestep_respacing='ddim10')
    real = torch.randn_like
    for mode, respace in (('ddim', 'ddim10'), ('ddpm', '10')):
        diff = ref_shim.build_reference_diffusion(dict(BASE, respace=respace), opt)
        kw = model_kwargs(xf, mask)
        kw['y'] = dict(gt=gt.clone(), outpainting_mask=keep.clone())
        draws = Draws(2 if mode == 'ddim' else 1)
        torch.randn_like = draws
        try:
            with torch.no_grad():
                if mode == 'ddim':
                    ref = diff.ddim_sample_loop(m, (B, T, C), noise=x_T.clone(), clip_denoised=False, model_kwargs=kw, eta=0)
                else:
                    ref = diff.p_sample_loop(m, (B, T, C), noise=x_T.clone(), clip_denoised=False, model_kwargs=kw)
        finally:
            torch.randn_like = real
        want = [d for k in range(10) for d in ((1 + k, (1 + k) ^ FLIP) if mode == 'ddim' else (1 + k,))]
        assert draws.log == want, draws.log
        sched = O.Schedule(1000, respace)
        x = x_T
        tf = O.precompute_text(sd, xf, dims)
        for k, i in enumerate(range(9, -1, -1)):
            x0m = O.denoise(sd, dims, x, sched.timestep_map[i], xf, mask, text_feats=tf)
            nz = row_draw((B, T, C), 1 + k)
            if mode == 'ddim':
                x, _ = O.ddim_step_repaint(sched, i, x, x0m, nz, keep, gt, row_draw((B, T, C), (1 + k) ^ FLIP), 0, add_blend=False)
            else:
                x = O.ddpm_step(sched, i, x, torch.where(keep, gt, x0m), nz)
        print(f'edit {mode}: oracle vs reference {maxabs(ref, x):.2e}; |kept region - gt| {maxabs(ref[keep], gt[keep]):.2e}; '
              f'|free - gt| {maxabs(ref[~keep], gt[~keep]):.2e}')
        assert maxabs(ref, x) <= 1e-5
        save[f'final_{mode}'] = ref.numpy()
    np.savez_compressed(os.path.join(OUT, 'edit_small.npz'), **save)
    print('wrote', os.path.join(OUT, 'edit_small.npz'), os.path.getsize(os.path.join(OUT, 'edit_small.npz')), 'bytes')


if __name__ == '__main__':
    main()

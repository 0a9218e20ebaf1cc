#!/usr/bin/env python
"""Wall time of the three ways to cover ONE long sequence with W windows (longform.py), through MotionDiffusion.forward:

  repaint   sample_long(repaint=True): W sequential B = 1 walks, window i keeps its first frames from window i - 1 (RePaint; with the
            resampling jumps of the reference tools' schedule, and with --no_resample without them)
  batch     sample_long_batched(repaint=False): the W windows as ONE batch, nothing couples them (the motion jumps at every seam)
  coupled   sample_long_coupled: the W windows as ONE batch, shared frames blended after every denoiser call (sampler_seam_k)

and the sampler update alone at the batch's [W, T, C]: sampler_update_k (mc_op_sampler_update) against sampler_seam_k
(mc_op_sampler_seam, one chain of W windows), bracketed by events.  The seam op uploads its table and synchronises inside the call, so
its bracket holds two small copies besides the kernel: the kernel's own duration is what a kernel trace of this tool shows
(tools/prof_cmd.sh <tag> tools/longform_time.py ...).

usage: longform_time.py [--small] [--windows W] [--steps N] [--overlap OV] [--reps R]
  --small: the reduced test config (24-frame windows) instead of the 0.125b architecture (196-frame windows)"""
import argparse
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
import motioncraft_amd as mc                                                  # noqa: E402
from motioncraft_amd import lib as L_, longform                               # noqa: E402
from motioncraft_amd.diffusion import build_diffusion                         # noqa: E402
from motioncraft_amd.engine import _ptr, _stream                              # noqa: E402
from motioncraft_amd.synthetic import default_dims, make_state_dict           # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--small', action='store_true')
p.add_argument('--windows', type=int, default=8)
p.add_argument('--steps', type=int, default=50)
p.add_argument('--overlap', type=int, default=None, help='shared frames of neighbouring windows (default 30; 6 with --small)')
p.add_argument('--reps', type=int, default=3)
a = p.parse_args()

cfg = mc.Config.fromfile(os.path.join(ROOT, 'tests', 'configs', 'stmogen_small.py'))
T = 24 if a.small else 196
ov = a.overlap if a.overlap is not None else (6 if a.small else 30)
if not a.small:
    d = default_dims()
    m = cfg.model.model
    m.max_seq_len, m.latent_dim, m.num_layers, m.time_embed_dim = T, d['L'] * d['H'], d['NL'], d['Te']
    blk = m.ca_block_cfg
    blk.latent_dim, blk.text_latent_dim, blk.time_embed_dim, blk.max_seq_len, blk.max_text_seq_len = d['L'], d['Dt'], d['Te'], T, d['Nt']
    blk.ffn_dim = d['F']
    m.ffn_cfg.latent_dim, m.ffn_cfg.ffn_dim, m.ffn_cfg.time_embed_dim = d['L'], d['F'], d['Te']
    m.text_encoder.latent_dim = d['Dt']
    m.pose_encoder_cfg.latent_dim = m.pose_decoder_cfg.latent_dim = d['L']
schedule = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large',
                respace='15,15,8,6,6' if a.steps == 50 else f'ddim{a.steps}')
cfg.model.diffusion_test = schedule
W, C = a.windows, 322
total = ov + W * (T - ov)
assert longform.seam_plan(total, T, ov)[0] == W


def build(no_resample):
    # the long-sequence options the sampler reads through cfg.model['opt'] (tools/s2g_test.py:551-560; the tools' defaults)
    cfg.model['opt'] = argparse.Namespace(overlap_len=ov, timestep_respacing=f'ddim{a.steps}', jump_length=3, jump_n_sample=5, addBlend=True,
                                          no_repaint=False, no_resample=no_resample, same_overlap_noisy=False)
    arch = mc.build_architecture(cfg.model)
    arch.load_state_dict({'model.' + k: v for k, v in make_state_dict(arch.model.dims, 0).items()})
    return arch


def timed(name, fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    med = sorted(ts)[len(ts) // 2]
    print(f'{name:58s} median {med * 1e3:8.1f} ms   min {min(ts) * 1e3:8.1f}   max {max(ts) * 1e3:8.1f}   ({a.reps} runs after one warm-up)', flush=True)
    return med


arch = build(no_resample=False)
dims = arch.model.dims
g = torch.Generator().manual_seed(0)
xf = torch.nn.functional.layer_norm(torch.randn(1, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda()
gen = torch.Generator(device='cuda').manual_seed(1)
inf = dict(generator=gen)
print(f'# {"small" if a.small else "0.125b"} config, ONE sequence of {total} frames = {W} windows of {T} frames sharing {ov}, {a.steps}-step DDIM, fp32;'
      f' wall time of the driver call (condition hoist, sampling, stitching on the host)')
t_rp = timed(f'sample_long(repaint=True)  {W} x B=1, resampling jumps',
             lambda: longform.sample_long(arch, total, T, ov, text='', repaint=True, overlap_len=ov, fix_very_first=False, input_dim=C,
                                          condition_kwargs=dict(xf_out=xf), inference_kwargs=inf))
t_b = timed(f'sample_long_batched(repaint=False)  B={W}, uncoupled',
            lambda: longform.sample_long_batched(arch, [total], T, ov, text=[''], repaint=False, input_dim=C, condition_kwargs=dict(xf_out=xf),
                                                 inference_kwargs=inf, shard=False))
t_c = timed(f'sample_long_coupled  B={W}, seams blended per step',
            lambda: longform.sample_long_coupled(arch, [total], T, ov, text=[''], input_dim=C, condition_kwargs=dict(xf_out=xf),
                                                 inference_kwargs=inf, shard=False))
arch.model.release()
arch = build(no_resample=True)
t_rn = timed(f'sample_long(repaint=True)  {W} x B=1, --no_resample',
             lambda: longform.sample_long(arch, total, T, ov, text='', repaint=True, overlap_len=ov, fix_very_first=False, input_dim=C,
                                          condition_kwargs=dict(xf_out=xf), inference_kwargs=inf))
arch.model.release()
print(f'# coupled / uncoupled batch {t_c / t_b:.3f};  RePaint (jumps) / coupled {t_rp / t_c:.2f};  RePaint (no_resample) / coupled {t_rn / t_c:.2f}')

# ---- the sampler update alone at [W, T, C] ----
lib = L_.load(require_gpu=True)
dd = build_diffusion(schedule)
c = dd.step_coefs(dd.num_timesteps // 2, 'ddim', 6.5)
n = W * T * C
x, o_t, o_n, nz, xp = (torch.randn(n, device='cuda') for _ in range(5))
ff = (ctypes.c_int32 * W)(*[i * (T - ov) for i in range(W)])


def plain():
    L_.check(lib.mc_op_sampler_update(_ptr(x), _ptr(o_t), _ptr(o_n), _ptr(nz), _ptr(xp), None, n, ctypes.byref(c), _stream()), 'mc_op_sampler_update')


def seam():
    L_.check(lib.mc_op_sampler_seam(_ptr(x), _ptr(o_t), _ptr(o_n), _ptr(nz), 0, 0, None, _ptr(xp), None, W, T, C, ov, ff, None, ctypes.byref(c),
                                    _stream()), 'mc_op_sampler_seam')


for name, fn in (('sampler_update_k (mc_op_sampler_update)', plain), ('sampler_seam_k (mc_op_sampler_seam: + table upload)', seam)):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    us.sort()
    print(f'[{W}, {T}, {C}] {name:52s} event bracket: median {us[len(us) // 2]:7.1f} us   min {us[0]:7.1f} us', flush=True)

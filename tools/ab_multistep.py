#!/usr/bin/env python
"""Same-box A/B of ONE sampler step by mode: DDIM (mode 1, twice: the spread of an arm against itself) against the multistep update
(mode 2) at order 2 (k1 != 0: the history buffer is read and written) and at order 1 (k1 = 0: DDIM's trajectory, history written only),
one context each, timed interleaved over several rounds the way tools/ab_step.py alternates its arms, the first arm of a round rotating
(box drift and position in the round hit every arm alike).  A step = denoiser + CFG + sampler update inside mc_sample_loop.

    python tools/ab_multistep.py [--batch 1 64] [--rounds 8] [--steps 10]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
from motioncraft_amd.diffusion import build_diffusion
from motioncraft_amd.engine import NativeModel
from motioncraft_amd.synthetic import default_dims, make_state_dict

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, nargs='+', default=[1, 64])
ap.add_argument('--frames', type=int, default=196)
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--steps', type=int, default=10)
a = ap.parse_args()

dims = default_dims()
nm = NativeModel(dims, make_state_dict(dims, 0), cfg_scale=6.5)
T = a.frames
diff = build_diffusion(dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large',
                            respace='ddim20'))
S = diff.num_timesteps
walk = list(range(S))[::-1]
ARMS = ('ddim', 'ddim (again)', 'multistep', 'multistep order 1')
ddim = [diff.step_coefs(i, 'ddim', 6.5) for i in walk]
ms = diff.multistep_coefs(walk, 6.5)
ms1 = diff.multistep_coefs(walk, 6.5, order=1)
# the timed steps: the middle of the walk, where every multistep update is second order
first = 2
if any(c.eta == 0.0 for c in ms[first:first + a.steps]):
    sys.exit(f'--steps {a.steps}: the 20-step walk has {S - 2 - first} second-order steps behind its first {first}')

for B in a.batch:
    g = torch.Generator().manual_seed(0)
    xf = torch.nn.functional.layer_norm(torch.randn(B, 77, 256, generator=g), (256,)).cuda()
    mask = torch.ones(B, T).cuda()
    ctxs, xs = [], []
    for _ in ARMS:
        c = nm.context(B, T, max_steps=S)
        c.set_timesteps(diff.timestep_map)
        c.set_condition(xf, mask)
        ctxs.append(c)
        xs.append(torch.randn(B, T, 322, generator=g).cuda())

    def run(j, k0, n):
        coefs = {'multistep': ms, 'multistep order 1': ms1}.get(ARMS[j], ddim)
        ctxs[j].sample_loop(xs[j], walk[k0:k0 + n], coefs[k0:k0 + n], noise=None, seed=7, draw0=0)

    for j in range(len(ARMS)):
        run(j, 0, first + 2)            # warm-up from the head of the walk (the multistep arm: its history becomes valid)
    torch.cuda.synchronize()
    ts = [[] for _ in ARMS]
    for r in range(a.rounds):
        for j in [(r + k) % len(ARMS) for k in range(len(ARMS))]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(j, first, a.steps)
            e1.record()
            torch.cuda.synchronize()
            ts[j].append(e0.elapsed_time(e1) / a.steps)
            xs[j].normal_()
    for name, t in zip(ARMS, ts):
        t = sorted(t)
        print(f'B={B:3d} {name:18s} median {t[len(t) // 2]:.4f} ms/step  min {t[0]:.4f}  max {t[-1]:.4f}   ({a.rounds} rounds x {a.steps} steps)')
    for c in ctxs:
        c.close()

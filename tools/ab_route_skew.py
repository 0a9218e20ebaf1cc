#!/usr/bin/env python
"""What early routing (option route_early) costs when the capacity cut drops many pairs: with route_early = 1 the expert MLP also
computes the rows of dropped (token, choice) pairs, with 0 only the kept ones.  Same-box A/B on the headline step (B=64, 196 frames,
one mc_sample_loop step) under gates that route like a skewed checkpoint (tests/helpers.skew_gates), two contexts timed interleaved
as tools/ab_step.py does, plus the dropped share of every layer from one captured denoiser call:

    python tools/ab_route_skew.py [--kind hot_pair] [--batch 64] [--rounds 8] [--steps 10] [--prec f32]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from helpers import FULL, skew_gates
from motioncraft_amd.diffusion import build_diffusion
from motioncraft_amd.engine import NativeModel
from oracle import weights as W

ap = argparse.ArgumentParser()
ap.add_argument('--kind', default='hot_pair', choices=['balanced', 'hot_pair', 'all_ties'])
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--frames', type=int, default=196)
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--prec', default='f32')
a = ap.parse_args()

dims = FULL
nm = NativeModel(dims, skew_gates(W.make_state_dict(dims, 0), dims, a.kind), cfg_scale=dims['scale'])
B, T = a.batch, a.frames
g = torch.Generator().manual_seed(0)
xf = torch.nn.functional.layer_norm(torch.randn(B, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda()
mask = torch.ones(B, T).cuda()
diff = build_diffusion(dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large'))
coefs = [diff.step_coefs(992 + j, 'ddpm', dims['scale']) for j in range(8)]


def context(early):
    c = nm.context(B, T, max_steps=8)
    c.set_option('route_early', early)
    c.set_precision(a.prec)
    c.set_timesteps(diff.timestep_map[-8:])
    c.set_condition(xf, mask)
    return c


# the dropped share of every layer (one denoiser call with the routing capture on)
c = context(1)
c.enable_capture()
x0 = torch.randn(B, T, dims['input_feats'], generator=g).cuda()
c.denoise(x0, 7)
torch.cuda.synchronize()
print(f'# tools/ab_route_skew.py --kind {a.kind}: B={B} x {T} frames, {a.prec}; dropped share of the (token, choice) pairs per layer '
      f'(= rows the expert MLP computes with route_early = 1 and skips with 0)')
shares = []
for l in range(dims['NL']):
    _, keep = c.routing(l)
    shares.append(float((~keep).float().mean()))
    print(f'layer {l}: dropped 1st choices {float((~keep[:, 0]).float().mean()):.4f}, 2nd choices {float((~keep[:, 1]).float().mean()):.4f}, '
          f'all pairs {shares[-1]:.4f}')
print(f'mean over layers: {sum(shares) / len(shares):.4f} of all pairs dropped')
c.close()

ctxs = [context(0), context(1)]
xs = [torch.randn(B, T, dims['input_feats'], generator=g).cuda() for _ in ctxs]


def run(j, n):
    order = [s % 8 for s in range(n)]
    ctxs[j].sample_loop(xs[j], order, [coefs[s] for s in order], noise=None, seed=7, draw0=0)


for j in range(2):
    run(j, 4)
torch.cuda.synchronize()
ts = [[], []]
for r in range(a.rounds):
    for j in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(j, a.steps)
        e1.record()
        torch.cuda.synchronize()
        ts[j].append(e0.elapsed_time(e1) / a.steps)
        xs[j].normal_()
for j, t in enumerate(ts):
    t = sorted(t)
    print(f'route_early={j}  median {t[len(t) // 2]:.3f} ms/step  min {t[0]:.3f}  max {t[-1]:.3f}   ({a.rounds} rounds x {a.steps} steps, {a.kind})')

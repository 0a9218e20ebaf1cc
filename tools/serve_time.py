#!/usr/bin/env python
"""Timing of independent requests in one batch, synthetic weights, fp32, each figure the median of --reps runs
after one warm-up:

  routing   one denoiser call (mc_denoise) at capacity factor 1.5 against 0 (keep-all routing: no selection work); the difference over
            the layers is the routing time a layer saves.  The two calls also differ in the expert rows they compute where the schedule
            computes kept pairs only (one stream / joined groups); the early two-group schedule computes every pair either way
  noise     the fused DDPM loop (mc_sample_loop, noise drawn in the sampler-update kernel): one seed per call (flat) against a seed table
  batcher   serve.RequestBatcher: R requests of a --steps DDIM walk through B = 1 calls against through one B = R batch
  rows       one sampler step: mc_sample_step against mc_sample_rows with the same index and coefficients in
            every row (the same kernel forms, the weights and the FiLM row read through the row tables), interleaved; and one
            mc_ctx_set_condition_rows (the whole batch's text MoE per layer: the cost of an admission) beside it
  arrivals  the fixed arrival list ARRIVALS below (request i arrives at tick ARRIVALS[i]; a tick is one sampler step of the batch)
            replayed through serve.RequestBatcher (a batch starts when the batcher is idle, with whatever has arrived, and runs its
            whole walk) and through serve.ContinuousBatcher (a request takes an open row at the next tick): requests/s and the mean
            and maximum ticks from arrival to completion

  edits      one mc_sample_rows tick (DDIM, capacity factor 0, noise drawn from the seed table) in three versions,
            alternated in one process: (a) no edit table, (b) a table whose keep bytes are all zero, (c) a table with 25 % of the
            elements kept; and mc_ctx_set_edit_rows for one fresh row beside mc_ctx_set_condition_rows

  long       one mc_sample_rows tick (DDIM eta 0.5, capacity factor 0, noise drawn from the seed table) without a
            row seam table and with one of B / 8 chains of 8 windows, alternated in one process, and mc_ctx_set_seam_rows itself; then
            the arrival list LONG_ARRIVALS, which mixes short requests and requests of 2 .. 8 windows, through
            serve.ContinuousBatcher(overlap=), beside its long requests alone through longform.sample_long_coupled batches

  long_edits the long arm's tick with the row seam table AND an edit table (sampler_seam_edit_rows_k; keep bytes all
            zero, and 25 % kept) against the table alone and no table, alternated in one process

usage: serve_time.py [--small] [--batch B] [--requests R] [--steps N] [--reps K]
                     [--only routing,noise,batcher,rows,arrivals,edits,long,long_edits]
  --small: the reduced test config (24 frames) instead of the 0.125b architecture (196 frames)"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
import motioncraft_amd as mc                                                  # noqa: E402
from motioncraft_amd.diffusion import build_diffusion                         # noqa: E402
from motioncraft_amd.serve import ContinuousBatcher, Request, RequestBatcher  # noqa: E402
from motioncraft_amd.synthetic import make_state_dict, default_dims           # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--small', action='store_true')
p.add_argument('--batch', type=int, default=64)
p.add_argument('--requests', type=int, default=16)
p.add_argument('--steps', type=int, default=50)
p.add_argument('--reps', type=int, default=3)
p.add_argument('--only', default='routing,noise,batcher')
p.add_argument('--skip_arrivals', action='store_true', help='--only long: the tick arms alone (a kernel trace of them)')
# request i arrives at tick ARRIVALS[i]: a burst, a trickle one step apart, a lull, a second burst that overfills B = 16, stragglers
ARRIVALS = [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 15, 20, 26, 33, 41, 50, 70, 70, 70, 70, 70, 70, 70, 70, 70, 70, 70, 70, 70, 70, 70, 70,
            70, 70, 71, 73, 76, 80, 85, 91, 98, 120, 150, 151]
a = p.parse_args()
only = set(a.only.split(','))

cfg = mc.Config.fromfile(os.path.join(ROOT, 'tests', 'configs', 'stmogen_small.py'))
T = 24 if a.small else 196
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
schedule = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
cfg.model.diffusion_test = dict(schedule, respace=f'ddim{a.steps}')
arch = mc.build_architecture(cfg.model)
arch.load_state_dict({'model.' + k: v for k, v in make_state_dict(arch.model.dims, 0).items()})
dims = arch.model.dims
C = dims['input_feats']
print(f'# {"small" if a.small else "0.125b"} config, T = {T}, fp32, synthetic weights; medians of {a.reps} after one warm-up', flush=True)


def median_of(fn):
    fn()
    vals = sorted(fn() for _ in range(a.reps))
    return vals[len(vals) // 2], vals[0], vals[-1]


def events_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    xf = torch.nn.functional.layer_norm(torch.randn(B, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda()
    lengths = [int(v) for v in torch.randint(T // 3, T + 1, (B,), generator=g)]
    mask = torch.zeros(B, T, device='cuda')
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    return torch.randn(B, T, C, generator=g).cuda(), xf, mask, lengths


B = a.batch
if 'routing' in only or 'noise' in only:
    x, xf, mask, _ = inputs(B)
    dd = build_diffusion(dict(schedule, respace='ddim10'))
    ctx = arch.model.native.context(B, T, max_steps=10)
    ctx.set_timesteps(dd.timestep_map)
    if 'routing' in only:
        NL = dims['NL']
        res = {}
        for cf in (1.5, 0.0, 1.5, 0.0):            # (twice, interleaved: a drift of the machine shows as a difference between equal settings)
            ctx.set_capacity_factor(cf)
            ctx.set_condition(xf, mask)
            out2 = torch.empty(2 * B, T, C, device='cuda')
            med, lo, hi = median_of(lambda: events_ms(lambda: ctx.denoise(x, 5, out2=out2), 5))
            res.setdefault(cf, []).append(med)
            print(f'B={B} denoiser call, capacity factor {cf:3.1f}: median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   (5 calls per run)', flush=True)
        diff = min(res[1.5]) - min(res[0.0])
        print(f'B={B} keep-all routing saves {diff * 1e3:7.1f} us per call = {diff * 1e3 / NL:6.1f} us per layer ({NL} layers; coop routing: '
              f'{ctx.uses_coop_routing})', flush=True)
        ctx.set_capacity_factor(1.5)
        ctx.set_condition(xf, mask)
    if 'noise' in only:
        idx = list(range(10))[::-1]
        coefs = [dd.step_coefs(i, 'ddpm', arch.model.cfg_scale) for i in idx]
        for name, seeds in (('flat (one seed per call)', None), ('seed table (row keys)', list(range(100, 100 + B))),
                            ('flat (one seed per call)', None), ('seed table (row keys)', list(range(100, 100 + B)))):
            ctx.set_row_seeds(seeds)
            xd = x.clone()
            med, lo, hi = median_of(lambda: events_ms(lambda: ctx.sample_loop(xd, idx, coefs, noise=None, seed=7, draw0=1), 1) / 10)
            print(f'B={B} fused DDPM loop, {name:26s}: median {med:8.4f} ms per step   min {lo:8.4f}   max {hi:8.4f}   (10-step loops)', flush=True)
        ctx.clear_row_seeds()
    ctx.close()

if 'batcher' in only:
    R = a.requests
    g = torch.Generator().manual_seed(1)
    reqs = [Request(length=int(torch.randint(T // 3, T + 1, (1,), generator=g)), seed=500 + i,
                    xf_out=torch.nn.functional.layer_norm(torch.randn(dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda())
            for i in range(R)]
    for batch in (1, R):
        bt = RequestBatcher(arch, batch=batch, frames=T, sampler='ddim', steps=a.steps)

        def run():
            for r in reqs:
                bt.submit(r)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = bt.run()
            torch.cuda.synchronize()
            assert len(out) == R
            return time.perf_counter() - t0
        med, lo, hi = median_of(run)
        print(f'{R} requests, {a.steps}-step DDIM, through B={batch:<3d} calls: median {med * 1e3:8.1f} ms = {R / med:7.2f} requests/s   '
              f'(min {lo * 1e3:8.1f} ms, max {hi * 1e3:8.1f} ms)', flush=True)
if 'rows' in only:
    x, xf, mask, _ = inputs(B)
    dd = build_diffusion(dict(schedule, respace='ddim10'))
    ctx = arch.model.native.context(B, T, max_steps=10)
    ctx.set_timesteps(dd.timestep_map)
    ctx.set_condition(xf, mask)
    c5 = dd.step_coefs(5, 'ddim', arch.model.cfg_scale)
    noise = torch.randn(1, B, T, C, device='cuda')
    xd = x.clone()
    arms = {'mc_sample_step': lambda: ctx.sample_step(xd, 5, c5, noise[0], x_prev=xd),
            'mc_sample_rows (uniform tables)': lambda: ctx.sample_rows(xd, [[5] * B], [[c5] * B], noise=noise),
            'mc_ctx_set_condition_rows': lambda: ctx.set_condition_rows(xf, mask, [True] + [False] * (B - 1))}
    for name in list(arms) * 2:                    # (twice, interleaved)
        med, lo, hi = median_of(lambda: events_ms(arms[name], 5))
        print(f'B={B} {name:32s}: median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   (5 calls per run)', flush=True)
    ctx.close()

if 'edits' in only:
    x, xf, mask, _ = inputs(B)
    dd = build_diffusion(dict(schedule, respace=f'ddim{a.steps}'))
    ctx = arch.model.native.context(B, T, max_steps=a.steps)
    ctx.set_capacity_factor(0)
    ctx.set_timesteps(dd.timestep_map)
    ctx.set_condition(xf, mask)
    ctx.set_row_seeds(list(range(100, 100 + B)))
    step = a.steps // 2
    ck = dd.step_coefs(step, 'ddim', arch.model.cfg_scale)
    g = torch.Generator().manual_seed(3)
    gt = torch.randn(B, T, C, generator=g).cuda()
    keep0 = torch.zeros(B, T, C, dtype=torch.uint8, device='cuda')
    keep25 = (torch.rand(B, T, C, generator=g) < 0.25).to(torch.uint8).cuda()
    xd = x.clone()
    fresh1 = [True] + [False] * (B - 1)
    tick = lambda: ctx.sample_rows(xd, [[step] * B], [[ck] * B], draws=[[1] * B])

    def version(keep):
        if keep is None:
            ctx.clear_edit_rows()
        else:
            ctx.set_edit_rows(gt, keep)
        return median_of(lambda: events_ms(tick, 5))
    arms = {'(a) mc_sample_rows tick, no table': lambda: version(None),
            '(b) ... keep all zero': lambda: version(keep0),
            '(c) ... 25 % kept': lambda: version(keep25),
            'mc_ctx_set_edit_rows (one fresh row)': lambda: median_of(lambda: events_ms(lambda: ctx.set_edit_rows(gt, keep25, fresh1), 5)),
            'mc_ctx_set_condition_rows': lambda: (ctx.clear_edit_rows(), median_of(lambda: events_ms(lambda: ctx.set_condition_rows(xf, mask, fresh1), 5)))[1]}
    for name in list(arms) * 3:                    # (three rounds, alternated: the spread of equal settings is the machine's drift)
        med, lo, hi = arms[name]()
        print(f'B={B} {name:38s}: median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   (5 calls per run)', flush=True)
    ctx.clear_edit_rows()
    ctx.close()

if 'arrivals' in only:
    g = torch.Generator().manual_seed(2)
    reqs = [Request(length=int(torch.randint(T // 3, T + 1, (1,), generator=g)), seed=900 + i,
                    xf_out=torch.nn.functional.layer_norm(torch.randn(dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda())
            for i in range(len(ARRIVALS))]
    R = len(reqs)

    def replay_whole():
        """RequestBatcher: idle -> one batch of what has arrived (at most B), its whole walk; the clock advances by the walk"""
        bt = RequestBatcher(arch, batch=B, frames=T, sampler='ddim', steps=a.steps)
        tick, k, waiting, lat = 0, 0, [], []
        while k < R or waiting:
            while k < R and ARRIVALS[k] <= tick:
                waiting.append(k)
                k += 1
            if not waiting:
                tick = ARRIVALS[k]
                continue
            part, waiting = waiting[:B], waiting[B:]
            for i in part:
                bt.submit(reqs[i])
            assert len(bt.run()) == len(part)
            tick += a.steps
            lat += [tick - ARRIVALS[i] for i in part]
        return lat

    def replay_continuous():
        bt = ContinuousBatcher(arch, batch=B, frames=T, sampler='ddim', steps=a.steps)
        k, done, lat = 0, 0, []
        while done < R:
            while k < R and ARRIVALS[k] <= bt.ticks:
                bt.submit(reqs[k])
                k += 1
            if bt.tick() == 0:
                bt.ticks = ARRIVALS[k]              # idle: the clock jumps to the next arrival
            for h in bt.poll():
                lat.append(bt.finished_at[h] - ARRIVALS[h])
                done += 1
        return lat

    for name, fn in (('RequestBatcher', replay_whole), ('ContinuousBatcher', replay_continuous)) * 2:
        box = {}

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            box['lat'] = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        med, lo, hi = median_of(run)
        lat = box['lat']
        print(f'{R} arrivals, {a.steps}-step DDIM, B={B}, {name:17s}: median {med * 1e3:8.1f} ms = {R / med:7.2f} requests/s   '
              f'(min {lo * 1e3:8.1f}, max {hi * 1e3:8.1f} ms);  ticks to completion: mean {sum(lat) / len(lat):6.1f}, max {max(lat)}', flush=True)
if 'long' in only:
    # (a) one tick with and without a row seam table: B rows as B / 8 chains of 8 windows, chain c on rows c, c + B/8, c + 2 B/8, ...
    ov = T // 7 if not a.small else 6
    stride = T - ov
    x, xf, mask, _ = inputs(B)
    mask[:] = 1
    dd = build_diffusion(dict(schedule, respace=f'ddim{a.steps}'))
    ctx = arch.model.native.context(B, T, max_steps=a.steps)
    ctx.set_capacity_factor(0)
    ctx.set_timesteps(dd.timestep_map)
    ctx.set_condition(xf, mask)
    nch = max(B // 8, 1)
    ctx.set_row_seeds([100 + b % nch for b in range(B)])
    step = a.steps // 2
    ck = dd.step_coefs(step, 'ddim', arch.model.cfg_scale, 0.5)
    right = [b + nch if b + nch < B else -1 for b in range(B)]
    first = [(b // nch) * stride for b in range(B)]
    xd = x.clone()
    tick = lambda: ctx.sample_rows(xd, [[step] * B], [[ck] * B], draws=[[1] * B])

    def version(table):
        if table:
            ctx.set_seam_rows(right, first, ov)
        else:
            ctx.clear_seam_rows()
        return median_of(lambda: events_ms(tick, 5))
    # (c) the whole-batch path of section 4m at the same shape: mc_sample_step under mc_ctx_set_seams, nch sequences of adjacent windows
    noise1 = torch.randn(B, T, C, device='cuda')
    per = B // nch
    first_adj = [(b // per) * (per * T + T) + (b % per) * stride for b in range(B)]

    def whole_batch():
        ctx.clear_seam_rows()
        ctx.set_seams(first_adj, ov)
        try:
            return median_of(lambda: events_ms(lambda: ctx.sample_step(xd, step, ck, noise1, x_prev=xd), 5))
        finally:
            ctx.clear_seams()
    arms = {'(a) mc_sample_rows tick, no table': lambda: version(False),
            f'(b) ... {nch} chains of {B // nch} windows': lambda: version(True),
            '(c) mc_sample_step, mc_ctx_set_seams': whole_batch,
            'mc_ctx_set_seam_rows': lambda: median_of(lambda: events_ms(lambda: ctx.set_seam_rows(right, first, ov), 5))}
    for name in list(arms) * 2:                    # (the comparison twice, alternated: the spread of equal settings is the machine's drift)
        med, lo, hi = arms[name]()
        print(f'B={B} {name:38s}: median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   (5 calls per run)', flush=True)
    ctx.clear_seam_rows()
    ctx.close()
if 'long' in only and not a.skip_arrivals:
    ov = T // 7 if not a.small else 6
    stride = T - ov

    # (b) a fixed arrival list that mixes short requests (windows = 1) and requests of 2 .. 8 windows, through ContinuousBatcher(overlap=);
    # beside it the list's long requests alone through longform.sample_long_coupled batches (idle -> whatever has arrived, whole
    # sequences up to B windows, its whole walk): the only way such a request could run before
    from motioncraft_amd import longform
    LONG_ARRIVALS = [(0, 1), (0, 3), (1, 1), (2, 1), (4, 2), (5, 1), (8, 4), (10, 1), (12, 1), (20, 8), (21, 1), (30, 2), (30, 1), (45, 3),
                     (60, 1), (70, 4), (70, 1), (70, 1), (90, 2)]
    g = torch.Generator().manual_seed(4)
    lreqs = []
    for i, (_, w) in enumerate(LONG_ARRIVALS):
        n = int(torch.randint(T // 3, T + 1, (1,), generator=g)) if w == 1 else T + (w - 1) * stride
        lreqs.append(Request(length=n, seed=700 + i, xf_out=torch.nn.functional.layer_norm(torch.randn(dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda()))
    R = len(lreqs)
    longs = [i for i, (_, w) in enumerate(LONG_ARRIVALS) if w > 1]

    def replay_mixed():
        bt = ContinuousBatcher(arch, batch=B, frames=T, sampler='ddim', steps=a.steps, overlap=ov)
        k, done, lat = 0, 0, {}
        while done < R:
            while k < R and LONG_ARRIVALS[k][0] <= bt.ticks:
                bt.submit(lreqs[k])
                k += 1
            if bt.tick() == 0:
                bt.ticks = LONG_ARRIVALS[k][0]      # idle: the clock jumps to the next arrival
            for h in bt.poll():
                lat[h] = bt.finished_at[h] - LONG_ARRIVALS[h][0]
                done += 1
        return [lat[i] for i in longs], [lat[i] for i in range(R) if i not in longs]

    def replay_coupled():
        old, arch.inference_type = arch.inference_type, 'ddim'
        tick_, k, waiting, lat = 0, 0, [], []
        try:
            while k < len(longs) or waiting:
                while k < len(longs) and LONG_ARRIVALS[longs[k]][0] <= tick_:
                    waiting.append(longs[k])
                    k += 1
                if not waiting:
                    tick_ = LONG_ARRIVALS[longs[k]][0]
                    continue
                part, used = [], 0
                while waiting and used + LONG_ARRIVALS[waiting[0]][1] <= B:
                    used += LONG_ARRIVALS[waiting[0]][1]
                    part.append(waiting.pop(0))
                longform.sample_long_coupled(arch, [lreqs[i].length for i in part], T, ov, text=['a'] * len(part), input_dim=C,
                                             condition_kwargs=dict(xf_out=torch.stack([lreqs[i].xf_out for i in part])),
                                             inference_kwargs=dict(capacity_factor=0), max_batch=B, shard=False)
                tick_ += a.steps
                lat += [tick_ - LONG_ARRIVALS[i][0] for i in part]
        finally:
            arch.inference_type = old
        return lat, []

    for name, fn in (('ContinuousBatcher(overlap), all requests', replay_mixed), ('sample_long_coupled, the long ones alone', replay_coupled)) * 2:
        box = {}

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            box['lat'] = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        med, lo, hi = median_of(run)
        ll, ls = box['lat']
        nreq = len(ll) + len(ls)
        short = f'; short: mean {sum(ls) / len(ls):6.1f}, max {max(ls)}' if ls else ''
        print(f'{nreq} arrivals ({len(ll)} long, overlap {ov}), {a.steps}-step DDIM, B={B}, {name:42s}: median {med * 1e3:8.1f} ms = '
              f'{nreq / med:7.2f} requests/s   (min {lo * 1e3:8.1f}, max {hi * 1e3:8.1f} ms);  ticks to completion, long: mean '
              f'{sum(ll) / len(ll):6.1f}, max {max(ll)}{short}', flush=True)
if 'long_edits' in only:
    #  one tick with both tables set (sampler_seam_edit_rows_k) against the same tick with the row seam table alone
    # (sampler_seam_rows_k) and with no table (sampler_update_rows_k), alternated in one process; the chains are those of the long arm
    ov = T // 7 if not a.small else 6
    stride = T - ov
    x, xf, mask, _ = inputs(B)
    mask[:] = 1
    dd = build_diffusion(dict(schedule, respace=f'ddim{a.steps}'))
    ctx = arch.model.native.context(B, T, max_steps=a.steps)
    ctx.set_capacity_factor(0)
    ctx.set_timesteps(dd.timestep_map)
    ctx.set_condition(xf, mask)
    ctx.set_long_edits(True)
    nch = max(B // 8, 1)
    ctx.set_row_seeds([100 + b % nch for b in range(B)])
    step = a.steps // 2
    ck = dd.step_coefs(step, 'ddim', arch.model.cfg_scale, 0.5)
    right = [b + nch if b + nch < B else -1 for b in range(B)]
    first = [(b // nch) * stride for b in range(B)]
    g = torch.Generator().manual_seed(5)
    gt = torch.randn(B, T, C, generator=g).cuda()
    keep0 = torch.zeros(B, T, C, dtype=torch.uint8, device='cuda')
    # 25 % kept, cut per chain from one request-global mask so that both copies of a shared frame agree
    glob = torch.rand(nch, (B // nch - 1) * stride + T, C, generator=g) < 0.25
    keep25 = torch.stack([glob[b % nch, first[b]:first[b] + T] for b in range(B)]).to(torch.uint8).cuda()
    xd = x.clone()
    tick = lambda: ctx.sample_rows(xd, [[step] * B], [[ck] * B], draws=[[1] * B])

    def version(table, keep):
        if table:
            ctx.set_seam_rows(right, first, ov)
        else:
            ctx.clear_seam_rows()
        if keep is None:
            ctx.clear_edit_rows()
        else:
            ctx.set_edit_rows(gt, keep)
        return median_of(lambda: events_ms(tick, 5))
    arms = {'(a) mc_sample_rows tick, no table': lambda: version(False, None),
            f'(b) ... {nch} chains of {B // nch} windows': lambda: version(True, None),
            '(c) ... chains + keep all zero': lambda: version(True, keep0),
            '(d) ... chains + 25 % kept': lambda: version(True, keep25)}
    for name in list(arms) * 3:                    # (three rounds, alternated: the spread of equal settings is the machine's drift)
        med, lo, hi = arms[name]()
        print(f'B={B} {name:38s}: median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   (5 calls per run)', flush=True)
    ctx.clear_seam_rows()
    ctx.clear_edit_rows()
    ctx.close()
arch.model.release()

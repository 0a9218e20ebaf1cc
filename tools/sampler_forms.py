"""Drive every form of the sampler update family (8 kernel templates, 30 symbols) and print one sha256 per output.

  python tools/sampler_forms.py --B 3 --T 7 [--C 263] [--reps 1] [--only ops|ctx]

Forms with an op entry (mc_op_sampler_*) run at [B][T][C], once on 16-byte aligned operands and once with every operand one float
(the keep table one byte) into its allocation.  Forms no op reaches -- noise drawn from the call's stream or from row keys, the
graph-table entry, the padded copy -- run through a context of the small config for three steps: the fused loop with and without a
seed table, a captured step, and two ticks of mc_sample_rows, at (B, min(T, 24)) and at the next batch whose B T is a multiple of
four (the two alignments of the decoder's second partial product).  Inputs come from fixed torch CPU generators, so two builds of the
library can be compared digest by digest; under a kernel trace the same run gives every symbol's time (--reps repeats each op launch and each fused loop;
--only ops / --only ctx keep one operand size per symbol in a trace).  The padded copy (PadOut) lives in a workspace no entry hands
out: it shows in the next step's x_prev, which the three-step loops and two-tick calls print.
"""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)
import motioncraft_amd as mc                                                  # noqa: E402
from motioncraft_amd import lib as L_                                         # noqa: E402
from motioncraft_amd.diffusion import build_diffusion                         # noqa: E402
from motioncraft_amd.synthetic import make_state_dict                         # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--B', type=int, default=3)
p.add_argument('--T', type=int, default=7)
p.add_argument('--C', type=int, default=263)
p.add_argument('--reps', type=int, default=1)
p.add_argument('--only', default='ops,ctx', help='ops: the op forms at [B][T][C]; ctx: the context forms (a kernel trace of one of them holds one size per symbol)')
a = p.parse_args()
B, T, C = a.B, a.T, a.C
TC, n = T * C, B * T * C
OV = min(3, T // 2)
GUARD = 8
lib = L_.load(require_gpu=True)
u64 = ctypes.c_uint64
_stream = L_.stream
dd = build_diffusion(dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large', respace='ddim10'))
gen = torch.Generator().manual_seed(20240607)


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def show(label, **arrays):
    for k, v in arrays.items():
        if v is not None:
            print(f'{label:58s} {k:7s} {sha(v)}', flush=True)


def dev(src, off, dtype=torch.float32):
    """`src` on the device, `off` elements into an allocation with GUARD elements behind"""
    buf = torch.zeros(off + src.numel() + GUARD, dtype=dtype, device='cuda')
    buf[off:off + src.numel()] = src.to(dtype).flatten()
    return buf[off:off + src.numel()]


def ptr(t):
    return None if t is None else t.data_ptr()


def row_entries(mode, nrows, scale=2.5):
    """an entry per row: three different steps in turn (mode 2: one row at its first step, k1 == 0)"""
    if mode == 'dpmpp':
        walk = dd.multistep_coefs(list(range(6))[::-1], scale, 2)
        pick = [walk[0], walk[2], walk[3]]
    else:
        pick = [dd.step_coefs(i, mode, scale, 0.5 if mode == 'ddim' else 0.0) for i in (5, 0, 2)]
    return [pick[b % 3] for b in range(nrows)]


def carr(rows):
    return (type(rows[0]) * len(rows))(*rows)


SRC = {k: torch.randn(n, generator=gen) for k in ('x', 'ot', 'on', 'nz', 'z2', 'gt', 'hist')}
KEEP = torch.rand(n, generator=gen) < 0.3
KEEP[TC - 2:TC] = True                                   # (kept elements on both sides of a row boundary)
SRC['gt'][~KEEP] = float('nan')                          # (gt where nothing is kept reaches no output)
SEEDS = [0x9E3779B97F4A7C15 ^ (b * 0x1000193) for b in range(B)]
DRAWS = [1 + 3 * b for b in range(B)]


def ops(off):
    t = {k: dev(v, off) for k, v in SRC.items()}
    t['keep'] = dev(KEEP, off, torch.uint8)
    t['out'], t['x0'] = dev(torch.full((n,), 7.0), off), dev(torch.full((n,), 7.0), off)
    return t


def run(fn):
    for _ in range(a.reps):
        rc = fn()
        if rc != 0:
            raise RuntimeError(lib.mc_last_error())


def op_forms(off):
    tag = 'aligned' if off == 0 else 'offset'
    for mode in ('ddpm', 'ddim', 'dpmpp'):
        ms = mode == 'dpmpp'
        rows = row_entries(mode, B)
        for k1, c in enumerate(rows[:2] if ms else rows[:1]):                              # uniform: k1 == 0 and k1 != 0 in mode 2
            t = ops(off)
            if ms:
                run(lambda: lib.mc_op_sampler_multistep(ptr(t['x']), ptr(t['ot']), ptr(t['on']), ptr(t['hist']), ptr(t['out']), ptr(t['x0']), n, ctypes.byref(c), _stream()))
            else:
                run(lambda: lib.mc_op_sampler_update(ptr(t['x']), ptr(t['ot']), ptr(t['on']), ptr(t['nz']), ptr(t['out']), ptr(t['x0']), n, ctypes.byref(c), _stream()))
            show(f'op uniform {mode} #{k1} {tag}', x_prev=t['out'], x0=t['x0'], hist=t['hist'] if ms and a.reps == 1 else None)
        t = ops(off)
        run(lambda: lib.mc_op_sampler_rows(ptr(t['x']), ptr(t['ot']), ptr(t['on']), None if ms else ptr(t['nz']), ptr(t['hist']) if ms else None,
                                           ptr(t['out']), ptr(t['x0']), B, TC, carr(rows), _stream()))
        show(f'op rows {mode} {tag}', x_prev=t['out'], x0=t['x0'], hist=t['hist'] if ms and a.reps == 1 else None)
        for drawn in ((False,) if ms else (False, True)):
            t = ops(off)
            run(lambda: lib.mc_op_sampler_edit_rows(ptr(t['x']), ptr(t['ot']), ptr(t['on']), None if ms or drawn else ptr(t['nz']),
                                                    ptr(t['z2']) if mode == 'ddim' and not drawn else None, ptr(t['gt']), ptr(t['keep']),
                                                    (u64 * B)(*SEEDS) if drawn else None, (u64 * B)(*DRAWS) if drawn else None,
                                                    ptr(t['hist']) if ms else None, ptr(t['out']), ptr(t['x0']), B, TC, carr(rows), _stream()))
            show(f'op edit rows {mode} {"drawn" if drawn else "tensor"} {tag}', x_prev=t['out'], x0=t['x0'], hist=t['hist'] if ms and a.reps == 1 else None)
        if OV < 1:
            continue
        # the batch as one chain of windows
        first = (ctypes.c_int32 * B)(*[b * (T - OV) for b in range(B)])
        for drawn in ((False,) if ms else (False, True)):
            t = ops(off)
            c = rows[1]
            run(lambda: lib.mc_op_sampler_seam(ptr(t['x']), ptr(t['ot']), ptr(t['on']), None if ms or drawn else ptr(t['nz']), 77 if drawn else 0, 5 if drawn else 0,
                                               ptr(t['hist']) if ms else None, ptr(t['out']), ptr(t['x0']), B, T, C, OV, first, None, ctypes.byref(c), _stream()))
            show(f'op seam {mode} {"drawn" if drawn else "tensor"} {tag}', x_prev=t['out'], x0=t['x0'], hist=t['hist'] if ms and a.reps == 1 else None)
        # requests of up to three windows over the rows B - 1, 0, 1, ..: one right neighbour sits at a lower row
        order = [B - 1] + list(range(B - 1))
        right, ff, req = [-1] * B, [0] * B, [0] * B
        for k, b in enumerate(order):
            ff[b], req[b] = (k % 3) * (T - OV), k // 3
            if k % 3:
                right[order[k - 1]] = b
        entries = row_entries(mode, B)
        srows = [entries[req[b]] for b in range(B)]
        for drawn in ((False,) if ms else (False, True)):
            t = ops(off)
            run(lambda: lib.mc_op_sampler_seam_rows(ptr(t['x']), ptr(t['ot']), ptr(t['on']), None if ms or drawn else ptr(t['nz']),
                                                    (u64 * B)(*[SEEDS[req[b]] for b in range(B)]) if drawn else None,
                                                    (u64 * B)(*[DRAWS[req[b]] for b in range(B)]) if drawn else None, ptr(t['hist']) if ms else None,
                                                    ptr(t['out']), ptr(t['x0']), B, T, C, OV, (ctypes.c_int32 * B)(*right), (ctypes.c_int32 * B)(*ff), None,
                                                    carr(srows), _stream()))
            show(f'op seam rows {mode} {"drawn" if drawn else "tensor"} {tag}', x_prev=t['out'], x0=t['x0'], hist=t['hist'] if ms and a.reps == 1 else None)


def ctx_forms(arch, Bc, Tc):
    dims = arch.model.dims
    Cc, scale = dims['input_feats'], arch.model.cfg_scale
    tag = f'ctx B={Bc} T={Tc}'
    g = torch.Generator().manual_seed(77 + Bc)
    x_T = torch.randn(Bc, Tc, Cc, generator=g)
    xf = torch.nn.functional.layer_norm(torch.randn(Bc, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).cuda()
    mask = torch.ones(Bc, Tc, device='cuda')
    noise = torch.randn(3, Bc, Tc, Cc, generator=g).cuda()
    idx = [9, 8, 7]
    seeds = [1000 + 7 * b for b in range(Bc)]
    coefs = {m: [dd.step_coefs(i, m, scale, 0.5 if m == 'ddim' else 0.0) for i in idx] for m in ('ddpm', 'ddim')}
    coefs['dpmpp'] = dd.multistep_coefs(idx, scale, 2)
    ov = min(3, Tc // 2)
    ctx = arch.model.native.context(Bc, Tc, max_steps=10)
    try:
        ctx.set_timesteps(dd.timestep_map)
        ctx.set_condition(xf, mask)
        for seam in (False, True):
            if seam:
                ctx.set_seams([b * (Tc - ov) for b in range(Bc)], ov)
            for mode in ('ddpm', 'ddim', 'dpmpp'):
                for name, kw in (('tensor', dict(noise=noise)), ('call stream', dict(seed=5, draw0=1)), ('row keys', dict(draw0=1))):
                    if mode == 'dpmpp' and name != 'tensor':
                        continue
                    ctx.set_row_seeds(seeds if name == 'row keys' else None)
                    for _ in range(a.reps):                                  # (from the same x_T every time: the last run is printed)
                        x, x0 = x_T.cuda().clone(), torch.zeros(Bc, Tc, Cc, device='cuda')
                        ctx.sample_loop(x, idx, coefs[mode], x0=x0, **({} if mode == 'dpmpp' else kw))
                    show(f'{tag} loop{" seams" if seam else ""} {mode} {name}', x_prev=x, x0=x0, hist=ctx.buffer('x0_hist') if mode == 'dpmpp' else None)
            ctx.set_row_seeds(None)
        ctx.clear_seams()
        # a captured step: the entry from the device table
        side = torch.cuda.Stream()
        for mode in ('ddpm', 'dpmpp'):
            with torch.cuda.stream(side):
                gx, gn = x_T.cuda().clone(), (noise[0].clone() if mode == 'ddpm' else None)
                table = [dd.step_coefs(i, 'ddpm', scale) for i in range(10)] if mode == 'ddpm' else dd.multistep_coefs(list(range(10))[::-1], scale, 2)[::-1]
                ctx.graph_capture(gx, gn, table)
                for i in idx:
                    ctx.graph_step(i)
                side.synchronize()
                show(f'{tag} graph {mode}', x_prev=gx)
                ctx.graph_release()
        # two ticks of per-row schedules: plain, edited, seam-coupled
        steps = [[9 - (b % 3) for b in range(Bc)], [8 - (b % 3) for b in range(Bc)]]
        gt = torch.randn(Bc, Tc, Cc, generator=g).cuda()
        keep = (torch.rand(Bc, Tc, Cc, generator=g) < 0.3).cuda()
        order = [Bc - 1] + list(range(Bc - 1))
        right, ff, req = [-1] * Bc, [0] * Bc, [0] * Bc
        for k, b in enumerate(order):
            ff[b], req[b] = (k % 3) * (Tc - ov), k // 3
            if k % 3:
                right[order[k - 1]] = b
        for form in ('rows', 'edit rows', 'seam rows'):
            if form == 'edit rows':
                ctx.set_edit_rows(gt, keep)
            if form == 'seam rows':
                ctx.clear_edit_rows()
                ctx.set_seam_rows(right, ff, ov)
            by = req if form == 'seam rows' else list(range(Bc))         # (the rows of a request walk together)
            ctx.set_row_seeds([seeds[by[b]] for b in range(Bc)])
            for mode in ('ddpm', 'ddim', 'dpmpp'):
                for drawn in ((False,) if mode == 'dpmpp' else (True, False)):
                    if form == 'edit rows' and mode == 'ddim' and not drawn:
                        continue                                             # (mode 1 draws the kept region's noise from the seed table)
                    st = [[steps[k][by[b]] for b in range(Bc)] for k in range(2)]
                    if mode == 'dpmpp':
                        walk = dd.multistep_coefs([9, 8], scale, 2)      # (the history is the batch's: every row at the same step)
                        st = [[9] * Bc, [8] * Bc]
                        cf = [[walk[0]] * Bc, [walk[1]] * Bc]
                    else:
                        cf = [[dd.step_coefs(s, mode, scale, 0.5 if mode == 'ddim' else 0.0) for s in st[k]] for k in range(2)]
                    x, x0 = x_T.cuda().clone(), torch.zeros(Bc, Tc, Cc, device='cuda')
                    ctx.sample_rows(x, st, cf, draws=[[1 + k + 2 * by[b] for b in range(Bc)] for k in range(2)] if drawn else None,
                                    noise=None if drawn or mode == 'dpmpp' else noise[:2], x0=x0)
                    show(f'{tag} {form} {mode} {"drawn" if drawn else "tensor"}', x_prev=x, x0=x0, hist=ctx.buffer('x0_hist') if mode == 'dpmpp' else None)
        ctx.set_row_seeds(seeds)
        show(f'{tag} draw_rows', draw=ctx.draw_rows(3))
    finally:
        ctx.close()


print(f'# sampler forms at B={B} T={T} C={C}, overlap {OV}, reps {a.reps}', flush=True)
for off in (0, 1) if 'ops' in a.only else ():
    op_forms(off)
cfg = mc.Config.fromfile(os.path.join(ROOT, 'tests', 'configs', 'stmogen_small.py'))
cfg.model.diffusion_test = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large', respace='ddim10')
arch = mc.build_architecture(cfg.model)
arch.load_state_dict({'model.' + k: v for k, v in make_state_dict(arch.model.dims, 0).items()})
Tc = min(T, 24)
shapes = [(B, Tc)]
if (B * Tc) % 4:
    shapes.append((B + (-B) % 4, Tc))
for Bc, Tcc in shapes if 'ctx' in a.only else ():
    ctx_forms(arch, Bc, Tcc)
torch.cuda.synchronize()
print('# done', flush=True)

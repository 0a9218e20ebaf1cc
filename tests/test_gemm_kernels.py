"""GPU (MI355X): every kernel the two GEMM dispatchers can pick, against fp64 at op level.

fp32 family (mc_op_gemm -> dense(): mc_launch_gemm_small / mc_launch_gemm): the choice depends on the shape and on the process
options small_gemm_rows, gemm_tune, small_tile_n and gemm_wp_grid, which a process reads once.  So each option set runs in a
child process of its own (this file with --child), one after another, and reports per shape the kernel the FLOP ledger booked
(kernel@grid_threads) and the largest error as a fraction of its bound.  Every launch: C pre-filled with NaN (all of it must be
written), two sentinel rows behind C (never written), W rows padded to ldw with NaN (never read); the in-place form res == C is
the FiLM GEMMs' residual update.  One launch has M K 4 >= 2^32 bytes of A: gemm_wp_k is refused there and gemm_dma_k must be
right past the 4 GB offset.

fp16 family (mc_launch_gemm_h): gemm_h_k through mc_op_gemm_f16, the plane kernels gemm_hd_k<split, pre> / gemm_hf_k<split>
through mc_op_gemm_f16_planes on planes built here (hi = fp16(a), lo = fp16(a - hi); fragment-major order restated from the
index formula).  The reference is the fp64 sum of exactly the products the kernel forms (hi Wh, + hi Wl + lo Wh when split), so
what is left is fp32 accumulation; in addition the error must sit far below each product class it includes or leaves out, so a
dropped lo term or a plane read in place of the other fails.  gemm_hf_k == gemm_hd_k and pre == no pre bit for bit.

Elementwise bound (u = 2^-24, n = products per output):
    |C - ref| <= s (n u (|A| |W|^T + |bias|) + 4 u |pre|) + e_act + u |R| + 4 u |ref|
with s the activation's largest slope and e_act = 2^-21 |pre| + 8 u |act(pre)| (fp32 evaluation of the activation)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = 2.0 ** -24
SENTINEL = 1234.5
SLOPE = {0: 1.0, 1: 1.1289, 2: 1.0998, 3: 1.0, 4: 1.0998}      # max |act'|: GELU, SiLU, LeakyReLU(0.01), x sigmoid(1.702 x)
MC_VARS = ('MC_SMALL_GEMM_ROWS', 'MC_GEMM_TUNE', 'MC_GEMM_WP_GRID', 'MC_SMALL_TILE_N')
TUNE = 1841                                     # kTuneDefault (mc_gemm.h): bits 0 staging, 4 DMA, 5 wave-private, 8 small XCD order, 9, 10
WP_GRID = 512                                   # gemm_wp_grid default

# (M, N, K, act, bias, res, ldw - K, in place)
SHAPES = [
    (128, 128, 32, 0, 1, 0, 0, 0),
    (128, 322, 64, 1, 1, 1, 4, 0),              # N % 4 != 0: scalar epilogue
    (300, 130, 40, 3, 1, 1, 4, 0),              # K % 32 != 0: gemm_k's guarded loop
    (2000, 256, 100, 0, 1, 1, 32, 0),           # ... with act 0 (dense() leaves the small kernels)
    (640, 256, 1536, 4, 1, 1, 0, 0),            # QuickGELU: gemm_k on full tiles too
    (1280, 384, 192, 1, 0, 0, 32, 0),           # 30 tiles: a persistent grid of 7 does not divide them
    (4992, 512, 512, 1, 1, 0, 0, 0),            # 192 x 26 evaluator rows, GELU
    (1000, 100, 32, 0, 1, 1, 0, 0),
    (384, 1536, 1536, 0, 1, 1, 4, 1),
    (5600, 1536, 1536, 0, 1, 1, 32, 1),         # the last row count of the small kernels (default options)
    (5601, 128, 1536, 2, 1, 0, 0, 0),
    (5601, 1536, 64, 0, 0, 1, 4, 0),
    (6272, 128, 1536, 0, 1, 0, 0, 0),
    (6272, 1536, 1536, 0, 1, 1, 0, 1),          # 588 tiles: the default grid of 512 walks some twice
    (7000, 200, 96, 0, 0, 1, 32, 0),            # beyond 6400 rows the small kernels take ragged tiles of any width
    (12544, 322, 1536, 0, 1, 0, 0, 0),
    (12544, 1536, 256, 1, 1, 1, 4, 0),
]
BIG = (699136, 128, 1536, 0, 1, 1, 0, 0)        # A is 4.3 GB: 32-bit byte offsets do not reach its last rows

SMALL = ('gemm_small_k', 'gemm_small16_k<3', 'gemm_small16_k<6')
# name, environment, kernels the set must reach, kernels it must not
SETS = [
    ('defaults', {}, ('gemm_small_k', 'gemm_k<0>', 'gemm_wp_k', 'gemm_dma_k'), ()),
    ('big_kernels', {'MC_SMALL_GEMM_ROWS': '0'}, ('gemm_k<0>', 'gemm_wp_k'), SMALL + ('gemm_dma_k',)),
    ('dma_no_xcd', {'MC_SMALL_GEMM_ROWS': '0', 'MC_GEMM_TUNE': str((TUNE & ~(1 << 5)) | 1 << 6)}, ('gemm_k<0>', 'gemm_dma_k'),
     SMALL + ('gemm_wp_k',)),
    ('gemm_k_only', {'MC_SMALL_GEMM_ROWS': '0', 'MC_GEMM_TUNE': str(TUNE & ~(1 << 4) & ~1)}, ('gemm_k<0>',),
     SMALL + ('gemm_wp_k', 'gemm_dma_k')),
    ('wp_grid7_no_staging_no_xcd', {'MC_SMALL_GEMM_ROWS': '0', 'MC_GEMM_TUNE': str((TUNE & ~1) | 1 << 6), 'MC_GEMM_WP_GRID': '7'},
     ('gemm_k<0>', 'gemm_wp_k'), SMALL + ('gemm_dma_k',)),
    ('wp_one_per_tile', {'MC_SMALL_GEMM_ROWS': '0', 'MC_GEMM_WP_GRID': '0'}, ('gemm_wp_k',), SMALL + ('gemm_dma_k',)),
    ('tile48_wp_grid_above_tiles', {'MC_SMALL_GEMM_ROWS': '100000', 'MC_SMALL_TILE_N': '48', 'MC_GEMM_WP_GRID': '100000'},
     ('gemm_small16_k<3', 'gemm_wp_k'), ('gemm_small_k', 'gemm_small16_k<6')),
    ('tile96_no_xcd', {'MC_SMALL_GEMM_ROWS': '100000', 'MC_SMALL_TILE_N': '96', 'MC_GEMM_TUNE': str(TUNE & ~(1 << 8))},
     ('gemm_small16_k<6',), ('gemm_small_k', 'gemm_small16_k<3')),
    ('tile64_no_xcd', {'MC_SMALL_GEMM_ROWS': '100000', 'MC_SMALL_TILE_N': '64', 'MC_GEMM_TUNE': str(TUNE & ~(1 << 8))},
     ('gemm_small_k',), ('gemm_small16_k<3', 'gemm_small16_k<6')),
]

# (M, N, K, split, bias, res, in place): gemm_h_k always; gemm_hd_k (and <., pre> with a residual) when K % 64 == 0;
# gemm_hf_k when also M % 32 == 0 and K >= 192
F16_SHAPES = [
    (300, 128, 32, 1, 1, 1, 0),
    (300, 128, 192, 1, 1, 1, 0),
    (300, 384, 256, 0, 1, 1, 1),
    (1000, 384, 384, 0, 1, 1, 0),
    (4097, 128, 256, 0, 0, 0, 0),
    (4097, 1536, 1536, 1, 1, 1, 1),
    (4128, 384, 192, 1, 1, 1, 0),
    (4128, 1536, 1536, 0, 1, 1, 1),
    (12544, 128, 192, 0, 1, 0, 0),
    (12544, 384, 256, 1, 0, 1, 0),
    (12544, 1536, 1536, 1, 1, 1, 1),
    # gemm_hf_k walks three slabs per trip (64 halves of K per slab in the f16 mode, 32 in the split mode); the shapes above leave a
    # remainder of 0 (f16) and of 0 or 2 (split).  M = 160: five 32-row blocks, so the second tile has one real block and three
    # waves clamped to it
    (160, 128, 256, 0, 1, 1, 0),        # f16, 4 slabs: remainder 1
    (160, 128, 320, 0, 1, 1, 0),        # f16, 5 slabs: remainder 2
    (160, 128, 320, 1, 1, 1, 0),        # split, 10 slabs: remainder 1
]

EVERY_KERNEL = ('gemm_small_k', 'gemm_small16_k<3', 'gemm_small16_k<6', 'gemm_k<0>', 'gemm_dma_k', 'gemm_wp_k',
                'gemm_h_k<true>', 'gemm_h_k<false>', 'gemm_hd_k<true>', 'gemm_hd_k<false>', 'gemm_hf_k<true>', 'gemm_hf_k<false>')


# ---------------------------------------------------------------------------------------------------------------------------
# child process: one option set (or the fp16 sweep); prints one JSON line
# ---------------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _ledger_keys(lib):
    n = lib.mc_debug_flop_ledger_dump(None, 0)
    buf = ctypes.create_string_buffer(int(n))
    lib.mc_debug_flop_ledger_dump(buf, n)
    return sorted(l.split('\t')[0] for l in buf.value.decode().splitlines() if l)


def _rows(torch, M, K):
    """Rows the fp64 reference is computed for: all of a small launch, else the first and last tiles, the rows around the
    small-kernel limits and the 4 GB offset of A, and a random sample."""
    if M <= 1200:
        return torch.arange(M)
    g = torch.Generator().manual_seed(M)
    s = set(range(64)) | set(range(M - 192, M)) | set(torch.randint(0, M, (128,), generator=g).tolist())
    r4g = (1 << 32) // (4 * K)
    s |= {r for r in (5599, 5600, 6271, 6400, r4g - 1, r4g, r4g + 1) if r < M}
    return torch.tensor(sorted(s))


def _operands(torch, M, N, K, seed):
    """Inputs whose mistakes show: per-row offsets, every 7th column of A and every 5th row of W (output column) ~1e-3, the last
    k-slab of A one-signed and larger than the rest.  Generated on the device (A of the 4 GB launch never visits the host)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    a = torch.randn(M, K, device='cuda', generator=g)
    a.add_(torch.randn(M, 1, device='cuda', generator=g))
    a[:, ::7] *= 1e-3
    k0 = (K - 1) // 32 * 32
    a[:, k0:] = 2.0 + torch.rand(M, K - k0, device='cuda', generator=g)
    w = torch.randn(N, K, device='cuda', generator=g) / K ** 0.5
    w[::5] *= 1e-3
    b = torch.randn(N, device='cuda', generator=g)
    r = torch.randn(M, N, device='cuda', generator=g)
    return a, w, b, r


def _act64(torch, y, act):
    F = torch.nn.functional
    return {0: lambda v: v, 1: F.gelu, 2: F.silu, 3: lambda v: F.leaky_relu(v, 0.01), 4: lambda v: v * torch.sigmoid(1.702 * v)}[act](y)


def _fp32_shape(torch, L, lib, shape, seed):
    M, N, K, act, bias, res, pad, inplace = shape
    a, w, b, r = _operands(torch, M, N, K, seed)
    ldw = K + pad
    wbuf = torch.full((N, ldw), float('nan'), device='cuda')
    wbuf[:, :K] = w
    cbuf = torch.full((M + 2, N), float('nan'), device='cuda')
    cbuf[M:] = SENTINEL
    if inplace:
        cbuf[:M] = r
    rptr = (cbuf if inplace else r) if res else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.mc_debug_flop_ledger(1)
    rc = lib.mc_op_gemm(_ptr(a), _ptr(wbuf), _ptr(b if bias else None), _ptr(rptr), _ptr(cbuf), M, N, K, ldw, act, st)
    lib.mc_debug_flop_ledger(0)
    rec = dict(shape=list(shape), kernels=_ledger_keys(lib))
    if rc != 0:
        rec['error'] = f'mc_op_gemm failed (code {rc}): {L.last_error()}'
        return rec
    torch.cuda.synchronize()
    rec['sentinel_ok'] = bool((cbuf[M:] == SENTINEL).all())
    rec['all_written'] = bool(torch.isfinite(cbuf[:M]).all())
    idx = _rows(torch, M, K)
    ic = idx.cuda()
    c = cbuf[ic].double().cpu()
    A, W = a[ic].double().cpu(), w.double().cpu()
    B = b.double().cpu() if bias else torch.zeros(N, dtype=torch.float64)
    R = r[ic].double().cpu() if res else torch.zeros(len(idx), N, dtype=torch.float64)
    del a, w, b, r, wbuf, cbuf
    pre = A @ W.T + B
    bound = K * U * (A.abs() @ W.abs().T + B.abs()) + 4 * U * pre.abs()
    y = _act64(torch, pre, act)
    if act:
        bound = SLOPE[act] * bound + 2.0 ** -21 * pre.abs() + 8 * U * y.abs()
    ref = y + R
    bound = bound + U * R.abs() + 4 * U * ref.abs()
    ratio = (c - ref).abs() / bound
    rec['ratio'] = float(ratio.max()) if bool(torch.isfinite(c).all()) else float('inf')
    rec['rows'] = len(idx)
    return rec


def _planes(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


def _frag_major(p, M, K):
    """Fragment-major order (film_rows_k's `planes & 4` store, gemm_hf_k's A fragments): half
    (((r >> 5) (K >> 4) + s) 64 + (r & 31) + 32 h) 8 + e holds column 16 s + 8 h + e of row r."""
    return p.reshape(M // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()


def _f16_shape(torch, L, lib, shape, seed):
    M, N, K, split, bias, res, inplace = shape
    a, w, b, r = _operands(torch, M, N, K, seed)
    w = w * 8.0                                  # (the ~1e-3 rows stay fp16 normals)
    ah, al = _planes(a)
    wh, wl = _planes(w)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    kinds = [('gemm_h_k', None)]
    if K % 64 == 0:
        kinds += [('gemm_hd_k', 0)] + ([('gemm_hd_k pre', 1)] if res else [])
        if M % 32 == 0 and K >= 192:
            kinds += [('gemm_hf_k', 2)]
    fm = (_frag_major(ah, M, K), _frag_major(al, M, K)) if any(k[1] == 2 for k in kinds) else None
    outs, recs = {}, []
    for name, mode in kinds:
        cbuf = torch.full((M + 2, N), float('nan'), device='cuda')
        cbuf[M:] = SENTINEL
        if inplace:
            cbuf[:M] = r
        rptr = (cbuf if inplace else r) if res else None
        bp = b if bias else None
        lib.mc_debug_flop_ledger(1)
        if mode is None:
            rc = lib.mc_op_gemm_f16(_ptr(a), _ptr(w), _ptr(bp), _ptr(rptr), _ptr(cbuf), M, N, K, split, st)
        else:
            ph, pl = fm if mode == 2 else (ah, al)
            rc = lib.mc_op_gemm_f16_planes(_ptr(ph), _ptr(pl), _ptr(w), _ptr(bp), _ptr(rptr), _ptr(cbuf), M, N, K, split,
                                           int(mode == 1), int(mode == 2), st)
        lib.mc_debug_flop_ledger(0)
        rec = dict(shape=list(shape), kind=name, kernels=_ledger_keys(lib))
        recs.append(rec)
        if rc != 0:
            rec['error'] = f'{name} failed (code {rc}): {L.last_error()}'
            return recs
        torch.cuda.synchronize()
        rec['sentinel_ok'] = bool((cbuf[M:] == SENTINEL).all())
        rec['all_written'] = bool(torch.isfinite(cbuf[:M]).all())
        outs[name] = cbuf[:M]
    # the documented bit identities on the same planes
    if 'gemm_hd_k' in outs:
        for name in ('gemm_hd_k pre', 'gemm_hf_k'):
            if name in outs:
                same = bool(torch.equal(outs[name], outs['gemm_hd_k']))
                next(rc for rc in recs if rc['kind'] == name)['bitwise_vs_hd'] = same
    idx = _rows(torch, M, K)
    ic = idx.cuda()
    Ah, Al = ah[ic].double().cpu(), al[ic].double().cpu()
    Wh, Wl = wh.double().cpu(), wl.double().cpu()
    B = b.double().cpu() if bias else torch.zeros(N, dtype=torch.float64)
    R = r[ic].double().cpu() if res else torch.zeros(len(idx), N, dtype=torch.float64)
    main = Ah @ Wh.T
    t_wl, t_al = Ah @ Wl.T, Al @ Wh.T             # the two products of the split form beyond hi Wh
    pre = main + B + ((t_wl + t_al) if split else 0)
    absdot = Ah.abs() @ Wh.abs().T + ((Ah.abs() @ Wl.abs().T + Al.abs() @ Wh.abs().T) if split else 0)
    ref = pre + R
    bound = (3 if split else 1) * K * U * (absdot + B.abs()) + 4 * U * pre.abs() + U * R.abs() + 4 * U * ref.abs()
    for rec in recs:
        c = outs[rec['kind']][ic].double().cpu()
        e = c - ref
        rec['ratio'] = float(((e).abs() / bound).max()) if bool(torch.isfinite(c).all()) else float('inf')
        # each product class the form includes (split) or leaves out (plain) is far above what is left
        en = float(e.norm())
        rec['term_ratio'] = max(en / float(t_wl.norm()), en / float(t_al.norm()))
        rec['rows'] = len(idx)
    return recs


def _child(spec):
    sys.path.insert(0, ROOT)
    import torch
    from motioncraft_amd import lib as L
    lib = L.load(require_gpu=True)
    torch.cuda.set_device(0)
    out = []
    for i, shape in enumerate(spec['shapes']):
        if spec['kind'] == 'f16':
            recs = _f16_shape(torch, L, lib, shape, seed=100 + i)
        else:
            recs = [_fp32_shape(torch, L, lib, shape, seed=i)]
        out += recs
        torch.cuda.empty_cache()
        if any('error' in r for r in recs):
            break                               # a launch that failed: nothing more on this device in this process
    return dict(shapes=out)


# ---------------------------------------------------------------------------------------------------------------------------
# parent: the children one after another, each under a time limit; no child after one that died
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs():
    jobs = [(name, env, dict(kind='f32', shapes=SHAPES + ([BIG] if name == 'defaults' else []))) for name, env, _, _ in SETS]
    jobs.append(('f16', {}, dict(kind='f16', shapes=F16_SHAPES)))
    out, dead = {}, None
    for name, env, spec in jobs:
        if dead:
            out[name] = dict(error=f'not run: {dead}')
            continue
        penv = {k: v for k, v in os.environ.items() if k not in MC_VARS}
        penv.update(env)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', json.dumps(spec)], cwd=ROOT, env=penv,
                               capture_output=True, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            dead = f'the child of option set {name} timed out'
            out[name] = dict(error=dead)
            continue
        if p.returncode != 0:
            dead = f'the child of option set {name} exited with {p.returncode}'
            out[name] = dict(error=f'{dead}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}')
            continue
        out[name] = json.loads(p.stdout.strip().splitlines()[-1])
    return out


def _kernel(key):
    return key.split('@')[0]


def _check_records(tag, recs):
    bad = []
    for rec in recs:
        print(f"{tag}: {rec['shape']} {rec.get('kind', '')} {','.join(rec['kernels'])}: max err / bound "
              f"{rec.get('ratio', float('nan')):.3f}" + (f", error / smallest product class {rec['term_ratio']:.1e}" if 'term_ratio' in rec else '')
              + f" over {rec.get('rows', 0)} rows")
        if 'error' in rec:
            bad.append((rec['shape'], rec['error']))
            continue
        if len(rec['kernels']) != 1:
            bad.append((rec['shape'], 'ledger', rec['kernels']))
        if not rec['sentinel_ok']:
            bad.append((rec['shape'], rec.get('kind'), 'wrote past the last row of C'))
        if not rec['all_written']:
            bad.append((rec['shape'], rec.get('kind'), 'C holds NaN: an element not written or a padding column of W read'))
        if not rec['ratio'] <= 1.0:
            bad.append((rec['shape'], rec.get('kind'), 'max err / bound', rec['ratio']))
        if rec.get('term_ratio', 0.0) > 1 / 8:
            bad.append((rec['shape'], rec.get('kind'), 'error not far below a product class', rec['term_ratio']))
        if rec.get('bitwise_vs_hd') is False:
            bad.append((rec['shape'], rec['kind'], 'not bit-identical to gemm_hd_k on the same planes'))
    return bad


@pytest.mark.parametrize('name', [s[0] for s in SETS])
def test_fp32_gemm_kernels_vs_fp64(runs, name):
    _, env, must, must_not = next(s for s in SETS if s[0] == name)
    run = runs[name]
    assert 'error' not in run, run['error']
    recs = run['shapes']
    want = len(SHAPES) + (name == 'defaults')
    assert len(recs) == want, (name, len(recs), want)
    bad = _check_records(name, recs)
    reached = {_kernel(k) for r in recs for k in r['kernels']}
    assert set(must) <= reached, (name, 'not reached', set(must) - reached)
    assert not set(must_not) & reached, (name, 'reached', set(must_not) & reached)
    wp = int(env.get('MC_GEMM_WP_GRID', WP_GRID))
    for rec in recs:
        M, N = rec['shape'][:2]
        for key in rec['kernels']:
            if _kernel(key) == 'gemm_wp_k':
                tiles = (M // 128) * (N // 128)
                grid = min(tiles, wp) if wp > 0 else tiles
                if int(key.split('@')[1]) != grid * 256:
                    bad.append((rec['shape'], key, 'persistent grid', grid))
        if rec['shape'] == list(BIG) and rec['kernels'] and _kernel(rec['kernels'][0]) != 'gemm_dma_k':
            bad.append((rec['shape'], rec['kernels'], 'a launch beyond 32-bit offsets must take gemm_dma_k'))
    assert not bad, bad


def test_fp16_gemm_kernels_vs_fp64(runs):
    run = runs['f16']
    assert 'error' not in run, run['error']
    recs = run['shapes']
    assert {tuple(r['shape']) for r in recs} == set(F16_SHAPES)
    bad = _check_records('f16', recs)
    for rec in recs:
        kind, keys = rec['kind'], rec['kernels']
        split = 'true' if rec['shape'][3] else 'false'
        name = kind.split()[0]
        if [_kernel(k) for k in keys] != [f'{name}<{split}>']:
            bad.append((rec['shape'], kind, 'ran', keys))
    assert not bad, bad


def test_every_gemm_kernel_was_reached(runs):
    reached = {_kernel(k) for run in runs.values() for r in run.get('shapes', []) for k in r['kernels']}
    print('GEMM kernels reached:', sorted(reached))
    assert set(EVERY_KERNEL) <= reached, set(EVERY_KERNEL) - reached


if __name__ == '__main__' and len(sys.argv) == 3 and sys.argv[1] == '--child':
    print(json.dumps(_child(json.loads(sys.argv[2]))))

"""CPU: the sequence of context calls the three sampler loops of ``diffusion.py`` make, pinned call by call.

``sampling_context`` of a stand-in model returns a recording context on the CPU: every method the loops call is logged in order with
its arguments reduced to plain data (ints, the bytes of a ``StepCoefs`` as hex, a tensor as ``[shape, sha256 of its bytes]``), and its
outputs are a fixed function of its inputs, so a wrong buffer swap or a wrong draw order changes a later hash.  The traces of every
case live in ``golden/walk_traces.json``; ``python tests/test_walk_trace_host.py --record`` rewrites that file.  A change of
``diffusion.py`` that is meant to keep behaviour must not change a byte of it.  Graph replay needs ``torch.cuda.Stream`` and stays with
the GPU tests."""
import hashlib
import itertools
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from motioncraft_amd import diffusion as D                       # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'walk_traces.json')
BASE = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
B, T, C = 2, 8, 5
SHAPE = (B, T, C)
CPU = torch.device('cpu')
SCALE = 6.5
SEEDS = [11, 2 ** 63 + 5]
SEAMS = dict(first_frame=[0, 6], overlap=2)


# ---- plain data ---------------------------------------------------------------------------------------------------------------------
def _t(x):
    """a tensor as [shape, sha256 of its bytes], or None"""
    if x is None:
        return None
    x = x.detach().cpu().contiguous()
    return [list(x.shape), hashlib.sha256(x.numpy().tobytes()).hexdigest()]


def _plain(v):
    if isinstance(v, torch.Tensor):
        return _t(v)
    if isinstance(v, (list, tuple)):
        return [_plain(e) for e in v]
    if isinstance(v, dict):
        return {k: _plain(e) for k, e in sorted(v.items())}
    if v is None or isinstance(v, (bool, int, str)):
        return v
    return float(v)


def _field(key, d, n):
    """n numbers in [-1, 1): an exact integer function of (key, d)"""
    k = torch.arange(n, dtype=torch.int64)
    v = (k * 7919 + (int(key) % 100003) * 40503 + int(d) * 9973) % 1000
    return (v.to(torch.float32) / 500 - 1)


# ---- the recording context ----------------------------------------------------------------------------------------------------------
class Boom(RuntimeError):
    pass


class Recorder:
    """the stand-in for ``NativeContext``: logs, and computes ``x_prev = 0.5 x_t + 0.25 noise``, ``x0 = x_t - 1``"""
    uses_coop_routing = True

    def __init__(self, log, fail_at_step=None):
        self.log, self.fail_at_step, self.steps_seen, self.row_seeds = log, fail_at_step, 0, None

    # tables
    def set_seams(self, **kw):
        self.log.append(['set_seams', _plain(kw)])

    def clear_seams(self):
        self.log.append(['clear_seams'])

    def set_row_seeds(self, seeds):
        self.log.append(['set_row_seeds', [int(s) for s in seeds]])
        self.row_seeds = [int(s) for s in seeds]

    def clear_row_seeds(self):
        self.log.append(['clear_row_seeds'])
        self.row_seeds = None

    def draw_rows(self, draw, out=None):
        self.log.append(['draw_rows', int(draw)])
        z = torch.stack([_field(s, draw, T * C).reshape(T, C) for s in self.row_seeds])
        if out is not None:
            out.copy_(z)
            return out
        return z

    def check(self):
        self.log.append(['check'])

    # steps
    @staticmethod
    def _update(x_t, noise, x_prev, x0):
        new = 0.5 * x_t + (0.25 * noise if noise is not None else 0)
        if x0 is not None:
            x0.copy_(x_t - 1)
        if x_prev is None:
            return new
        x_prev.copy_(new)
        return x_prev

    def _count_step(self):
        self.steps_seen += 1
        if self.fail_at_step is not None and self.steps_seen == self.fail_at_step:
            raise Boom(f'step {self.steps_seen} fails')

    def sample_step(self, x_t, step_index, coefs, noise, x_prev=None, x0=None):
        self.log.append(['sample_step', int(step_index), bytes(coefs).hex(), _t(x_t), _t(noise), x_prev is not None, x0 is not None])
        self._count_step()
        return self._update(x_t, noise, x_prev, x0)

    def sample_loop(self, x, step_indices, coefs, noise=None, seed=0, draw0=0, x0=None):
        self.log.append(['sample_loop', [int(i) for i in step_indices], [bytes(c).hex() for c in coefs], _t(x), _t(noise), int(seed), int(draw0),
                         x0 is not None])
        assert len(step_indices) == len(coefs) and (noise is None or noise.shape[0] == len(coefs))
        for k in range(len(coefs)):
            if noise is not None:
                e = noise[k]
            elif self.row_seeds is not None:
                e = torch.stack([_field(s, draw0 + k, T * C).reshape(T, C) for s in self.row_seeds])
            elif coefs[k].mode == 2:
                e = None                                         # the multistep mode draws nothing
            else:
                e = _field(seed, draw0 + k, B * T * C).reshape(B, T, C)
            self._update(x, e, x, x0)
        return x

    def sample_step_seeded(self, x_t, step_index, coefs, noise, sqrt_ab, sqrt_1mab, pre_seq=None, pre_noise=None, transl=(), x_prev=None,
                           x0=None):
        self.log.append(['sample_step_seeded', int(step_index), bytes(coefs).hex(), _t(x_t), _t(noise), float(sqrt_ab), float(sqrt_1mab),
                         _t(pre_seq), _t(pre_noise), [[int(c), float(a), float(b)] for c, a, b in transl], x_prev is not None, x0 is not None])
        self._count_step()
        if pre_seq is not None:
            x_t[:, :pre_seq.shape[1]] = float(sqrt_ab) * pre_seq + float(sqrt_1mab) * pre_noise
        for ch, v0, v1 in transl:
            x_t[:, 0, ch], x_t[:, 1, ch] = v0, v1
        return self._update(x_t, noise, x_prev, x0)

    def sample_step_inpaint(self, x_t, step_index, coefs, noise, gt, keep, gt_noise=None, blend_w=None, blend_len=0, x_prev=None, x0=None):
        self.log.append(['sample_step_inpaint', int(step_index), bytes(coefs).hex(), _t(x_t), _t(noise), _t(gt), _t(keep), _t(gt_noise),
                         _t(blend_w), int(blend_len), x_prev is not None, x0 is not None])
        self._count_step()
        out = self._update(x_t, noise, x_prev, x0)
        kept = gt + (0.125 * gt_noise if gt_noise is not None else 0)
        out.copy_(torch.where(keep, kept, out))
        return out

    def renoise(self, x, noise, a, b, out=None):
        self.log.append(['renoise', _t(x), _t(noise), float(a), float(b), out is not None])
        new = float(a) * x + float(b) * noise
        if out is None:
            return new
        out.copy_(new)
        return out


class Model:
    cfg_scale = SCALE

    def __init__(self, fail_at_step=None):
        self.log, self.fail_at_step = [], fail_at_step

    def sampling_context(self, b, t, timestep_map, model_kwargs, device):
        self.log.append(['sampling_context', int(b), int(t), [int(v) for v in timestep_map], sorted(model_kwargs), str(device)])
        return Recorder(self.log, self.fail_at_step)


class NoModel:
    cfg_scale = SCALE

    def sampling_context(self, *a, **k):
        raise AssertionError('reached the context')


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _diffusion(mode, opt=None):
    return D.build_diffusion(dict(BASE, respace='6' if mode == 'ddpm' else 'ddim6'), opt=opt)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _noise_iter(shapes, seed=100):
    """the tensors of ``shapes``, cycled, each a fresh draw"""
    for n, s in enumerate(itertools.cycle(shapes)):
        yield _randn(seed + n, *s)


def _source(name, sampler):
    """the keywords of one noise source"""
    if name == 'generator':
        return dict(generator=torch.Generator().manual_seed(7))
    if name == 'seeds':
        return dict(seeds=list(SEEDS))
    table = [_randn(20 + i, *SHAPE) for i in range(6)]
    if sampler == 'dpmpp':
        return dict(noise=_randn(5, *SHAPE))
    if name == 'noise':
        return dict(noise=_randn(5, *SHAPE), step_noise=table)
    if name == 'callable':
        return dict(step_noise=lambda i: table[i], generator=torch.Generator().manual_seed(8))
    raise KeyError(name)


def _loop(d, sampler):
    return {'ddpm': d.p_sample_loop, 'ddim': d.ddim_sample_loop, 'dpmpp': d.dpm_solver_sample_loop}[sampler]


def _run(sampler, model=None, opt=None, shape=SHAPE, model_kwargs=None, **kw):
    """one call of a loop -> its trace: the context's log, then what came back"""
    d = _diffusion('ddpm' if sampler == 'ddpm' else 'ddim', opt)
    model = Model() if model is None else model
    if sampler == 'ddim':
        kw.setdefault('eta', 0.5)
    trajectory = kw.get('trajectory', None)
    try:
        out = _loop(d, sampler)(model, shape, clip_denoised=False, device=CPU, model_kwargs={} if model_kwargs is None else model_kwargs, **kw)
    except Exception as e:                                       # noqa: BLE001 (the trace records what was raised)
        return getattr(model, 'log', []) + [['raised', type(e).__name__, str(e)]]
    log = model.log + [['result', _t(out)]]
    if trajectory is not None:
        log.append(['trajectory', [[int(i), _t(x), _t(x0)] for i, x, x0 in trajectory]])
    return log


def _mask():
    keep = torch.zeros(SHAPE, dtype=torch.bool)
    keep[:, :3] = True
    return keep


def _opt(**kw):
    return types.SimpleNamespace(timestep_respacing='ddim6', jump_length=2, jump_n_sample=2, overlap_len=2, addBlend=True, **kw)


PATHS = dict(fused=lambda: dict(), steps=lambda: dict(fused=False), traj=lambda: dict(fused=False, trajectory=[]))


def _cases():
    """id -> a function that runs the case and returns its trace"""
    cases = {}

    def add(name, f):
        assert name not in cases, name
        cases[name] = f

    for sampler, orders in (('ddpm', [None]), ('ddim', [None]), ('dpmpp', [1, 2])):
        for order in orders:
            tag = sampler if order is None else f'{sampler}{order}'
            extra = {} if order is None else dict(order=order)
            for path, src in itertools.product(PATHS, ('generator', 'noise', 'callable', 'seeds')):
                if sampler == 'dpmpp' and src == 'callable':
                    continue
                add(f'{tag}-{path}-{src}', lambda s=sampler, p=path, n=src, e=extra: _run(s, **PATHS[p](), **_source(n, s), **e))
            add(f'{tag}-fused-num_steps3', lambda s=sampler, e=extra: _run(s, num_steps=3, **_source('generator', s), **e))
            add(f'{tag}-steps-num_steps3', lambda s=sampler, e=extra: _run(s, num_steps=3, fused=False, **_source('noise', s), **e))
            for path in ('fused', 'steps'):
                add(f'{tag}-{path}-seams', lambda s=sampler, p=path, e=extra: _run(s, model_kwargs=dict(seams=dict(SEAMS)), **PATHS[p](),
                                                                                  **_source('generator', s), **e))
                add(f'{tag}-{path}-seams-seeds', lambda s=sampler, p=path, e=extra: _run(
                    s, model_kwargs=dict(seams=dict(SEAMS, weights=[0.25, 0.75])), **PATHS[p](), **_source('seeds', s), **e))
    for sampler in ('ddpm', 'ddim'):
        add(f'{sampler}-fused-chunked', lambda s=sampler: _chunked(s))

    # outpainting
    y = lambda: dict(gt=_randn(31, *SHAPE), outpainting_mask=_mask())                                              # noqa: E731
    add('ddim-outpaint-resample', lambda: _run('ddim', opt=_opt(), model_kwargs=dict(y=y()), step_noise=_noise_iter([SHAPE]), noise=_randn(5, *SHAPE)))
    add('ddim-outpaint-no_resample', lambda: _run('ddim', opt=_opt(no_resample=True), model_kwargs=dict(y=y()), step_noise=_noise_iter([SHAPE]),
                                                  noise=_randn(5, *SHAPE)))
    add('ddim-outpaint-no_repaint', lambda: _run('ddim', opt=_opt(no_repaint=True), model_kwargs=dict(y=y()), step_noise=_noise_iter([SHAPE]),
                                                 noise=_randn(5, *SHAPE), trajectory=[]))
    add('ddpm-outpaint-gt', lambda: _run('ddpm', model_kwargs=dict(y=y()), step_noise=_noise_iter([SHAPE]), generator=torch.Generator().manual_seed(9)))
    add('ddpm-outpaint-generator', lambda: _run('ddpm', model_kwargs=dict(y=y()), generator=torch.Generator().manual_seed(9)))
    add('ddpm-mask-no-gt', lambda: _run('ddpm', model_kwargs=dict(y=dict(outpainting_mask=_mask())), fused=False, **_source('noise', 'ddpm')))
    add('ddim-mask-all-false', lambda: _run('ddim', opt=_opt(), model_kwargs=dict(y=dict(gt=_randn(31, *SHAPE), outpainting_mask=torch.zeros(SHAPE, dtype=torch.bool))),
                                            **_source('generator', 'ddim')))

    # seeding
    pre = lambda: _randn(41, B, 3, C)                                                                              # noqa: E731
    add('ddpm-pre_seq', lambda: _run('ddpm', pre_seq=pre(), generator=torch.Generator().manual_seed(10)))
    add('ddim-pre_seq-trajectory', lambda: _run('ddim', pre_seq=pre(), generator=torch.Generator().manual_seed(10), trajectory=[]))
    add('ddpm-pre_seq-transl_req-iterator', lambda: _run('ddpm', pre_seq=pre(), transl_req=[[0, 0.5, -0.5], (3, 1.0, 2.0)],
                                                         step_noise=_noise_iter([(B, 3, C), (2,), (2,), SHAPE]), noise=_randn(5, *SHAPE)))
    add('ddpm-transl_req-generator', lambda: _run('ddpm', transl_req=[[1, 0.25, 0.75]], generator=torch.Generator().manual_seed(12)))
    add('ddim-pre_seq-seeds', lambda: _run('ddim', pre_seq=pre(), seeds=list(SEEDS)))

    # cleanup: the third step fails under a table
    for sampler in ('ddpm', 'ddim', 'dpmpp'):
        add(f'{sampler}-cleanup-seams', lambda s=sampler: _run(s, model=Model(fail_at_step=3), model_kwargs=dict(seams=dict(SEAMS)), fused=False,
                                                               **_source('generator', s)))
        add(f'{sampler}-cleanup-seams-seeds', lambda s=sampler: _run(s, model=Model(fail_at_step=3), model_kwargs=dict(seams=dict(SEAMS)), fused=False,
                                                                     **_source('seeds', s)))

    # refusals that come after the context but before any step (the trace shows the context was asked for and nothing ran)
    for sampler in ('ddpm', 'ddim', 'dpmpp'):
        add(f'{sampler}-refuse-graph-trajectory', lambda s=sampler: _run(s, graph=True, trajectory=[], **_source('generator', s)))
    for sampler in ('ddpm', 'ddim'):
        add(f'{sampler}-refuse-graph-outpainting', lambda s=sampler: _run(s, opt=_opt(no_repaint=True), graph=True, model_kwargs=dict(y=y()),
                                                                          generator=torch.Generator().manual_seed(9)))
        add(f'{sampler}-refuse-graph-pre_seq', lambda s=sampler: _run(s, graph=True, pre_seq=pre(), generator=torch.Generator().manual_seed(9)))
        add(f'{sampler}-refuse-outpainting-pre_seq', lambda s=sampler: _run(s, opt=_opt(), model_kwargs=dict(y=y()), pre_seq=pre(),
                                                                            generator=torch.Generator().manual_seed(9)))
        add(f'{sampler}-refuse-outpainting-step_noise-list', lambda s=sampler: _run(s, opt=_opt(), model_kwargs=dict(y=y()), **_source('noise', s)))
        add(f'{sampler}-refuse-pre_seq-step_noise-list', lambda s=sampler: _run(s, pre_seq=pre(), **_source('noise', s)))
    add('ddpm-refuse-graph-transl_req', lambda: _run('ddpm', graph=True, transl_req=[[0, 1.0, 2.0]], generator=torch.Generator().manual_seed(9)))
    add('ddim-refuse-resample-num_steps', lambda: _run('ddim', opt=_opt(), model_kwargs=dict(y=y()), num_steps=3, step_noise=_noise_iter([SHAPE])))
    add('ddpm-refuse-transl_req-batch3', lambda: _run('ddpm', shape=(3, T, C), transl_req=[[0, 1.0, 2.0]], generator=torch.Generator().manual_seed(9)))
    add('ddpm-refuse-transl_req-item', lambda: _run('ddpm', transl_req=[[0, 1.0]], generator=torch.Generator().manual_seed(9)))
    add('ddpm-refuse-pre_seq-shape', lambda: _run('ddpm', pre_seq=_randn(41, B, 3, C + 1), generator=torch.Generator().manual_seed(9)))

    # refusals before any context is asked for
    def refuse(sampler, **kw):
        return lambda: _run(sampler, model=NoModel(), **kw)

    mask24 = lambda: dict(gt=torch.zeros(SHAPE), outpainting_mask=_mask())                                         # noqa: E731
    for sampler in ('ddpm', 'ddim', 'dpmpp'):
        kw = lambda: dict(seams=dict(SEAMS), y={})                                                                 # noqa: E731
        add(f'{sampler}-refuse-seams-graph', refuse(sampler, model_kwargs=kw(), graph=True))
        add(f'{sampler}-refuse-seams-pre_seq', refuse(sampler, model_kwargs=kw(), pre_seq=torch.zeros(B, 2, C)))
        add(f'{sampler}-refuse-seams-outpainting', refuse(sampler, model_kwargs=dict(seams=dict(SEAMS), y=mask24())))
        add(f'{sampler}-refuse-seams-keys', refuse(sampler, model_kwargs=dict(seams=dict(first=[0]), y={})))
        add(f'{sampler}-refuse-seeds-noise', refuse(sampler, seeds=list(SEEDS), noise=torch.zeros(SHAPE)))
        add(f'{sampler}-refuse-seeds-generator', refuse(sampler, seeds=list(SEEDS), generator=torch.Generator().manual_seed(1)))
        add(f'{sampler}-refuse-seeds-count', refuse(sampler, seeds=[1, 2, 3]))
        add(f'{sampler}-refuse-shape', refuse(sampler, shape=torch.Size(SHAPE).numel()))
    for sampler in ('ddpm', 'ddim'):
        add(f'{sampler}-refuse-seeds-step_noise', refuse(sampler, seeds=list(SEEDS), step_noise=[torch.zeros(SHAPE)] * 6))
        add(f'{sampler}-refuse-mask-shape', refuse(sampler, model_kwargs=dict(y=dict(gt=torch.zeros(SHAPE), outpainting_mask=torch.ones(B, T, dtype=torch.bool)))))
        add(f'{sampler}-refuse-gt-shape', refuse(sampler, model_kwargs=dict(y=dict(gt=torch.zeros(B, T), outpainting_mask=_mask()))))
    add('ddim-refuse-mask-no-gt', refuse('ddim', model_kwargs=dict(y=dict(outpainting_mask=_mask()))))
    add('ddim-refuse-outpainting-no-opt', refuse('ddim', model_kwargs=dict(y=mask24())))
    for sampler in ('ddpm', 'dpmpp'):
        add(f'{sampler}-refuse-seams-transl_req', refuse(sampler, model_kwargs=dict(seams=dict(SEAMS), y={}), transl_req=[[0, 1.0, 2.0]]))
        add(f'{sampler}-refuse-seeds-transl_req', refuse(sampler, seeds=list(SEEDS), transl_req=[[0, 1.0, 2.0]]))
    add('dpmpp-refuse-outpainting', refuse('dpmpp', model_kwargs=dict(y=mask24())))
    add('dpmpp-refuse-pre_seq', refuse('dpmpp', pre_seq=torch.zeros(B, 2, C)))
    add('dpmpp-refuse-transl_req', refuse('dpmpp', transl_req=[[0, 0.0, 0.0]]))
    add('dpmpp-refuse-order3', refuse('dpmpp', order=3))
    add('dpmpp-refuse-graph-outpainting', refuse('dpmpp', graph=True, model_kwargs=dict(y=mask24())))
    add('dpmpp-refuse-graph-pre_seq', refuse('dpmpp', graph=True, pre_seq=torch.zeros(B, 2, C)))
    add('ddim-refuse-same_overlap_noisy', refuse('ddim', opt=_opt(same_overlap_noisy=True)))
    add('ddpm-refuse-clip_denoised', lambda: _unsupported())
    return cases


def _chunked(sampler):
    """fused with step_noise, the chunk rule forced to split the six steps into three calls"""
    old = D.FUSED_NOISE_CHUNK_BYTES
    D.FUSED_NOISE_CHUNK_BYTES = 2 * 4 * B * T * C
    try:
        return _run(sampler, **_source('noise', sampler))
    finally:
        D.FUSED_NOISE_CHUNK_BYTES = old


def _unsupported():
    try:
        _diffusion('ddpm').p_sample_loop(NoModel(), SHAPE, device=CPU)
    except Exception as e:                                       # noqa: BLE001
        return [['raised', type(e).__name__, str(e)]]
    return [['returned']]


CASES = _cases()


def record():
    return {name: json.loads(json.dumps(CASES[name]())) for name in sorted(CASES)}


def dump(traces):
    """one call per line: a change shows as the lines of the calls it moved"""
    out = ['{']
    for k, name in enumerate(sorted(traces)):
        out.append(f' {json.dumps(name)}: [')
        out.extend(f'  {json.dumps(e, sort_keys=True)}' + (',' if j + 1 < len(traces[name]) else '') for j, e in enumerate(traces[name]))
        out.append(' ]' + (',' if k + 1 < len(traces) else ''))
    out.append('}')
    return '\n'.join(out) + '\n'


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_walk_makes_the_recorded_calls(name, golden):
    got = json.loads(json.dumps(CASES[name]()))
    want = golden[name]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'{name}: call {k} differs'
    assert len(got) == len(want), f'{name}: {len(got)} calls, recorded {len(want)}'


@pytest.mark.parametrize('name', sorted(n for n in CASES if '-cleanup-' in n))
def test_tables_are_cleared_exactly_once_when_a_step_fails(name):
    trace = CASES[name]()
    calls = [e[0] for e in trace]
    assert trace[-1][:2] == ['raised', 'Boom']                   # the step's own exception, not one of the cleanup
    assert calls.count('set_seams') == 1 and calls.count('clear_seams') == 1
    seeded = name.endswith('-seeds')
    assert calls.count('set_row_seeds') == calls.count('clear_row_seeds') == (1 if seeded else 0)
    assert calls[-3:] == ['clear_seams', 'clear_row_seeds', 'raised'] if seeded else calls[-2:] == ['clear_seams', 'raised']
    assert calls.count('sample_step') == 3 and 'check' not in calls


@pytest.mark.parametrize('name', sorted(n for n in CASES if '-refuse-' in n))
def test_refusals_run_nothing(name, golden):
    """a refusal ends the trace; none of them comes after a step, a draw or a table"""
    calls = [e[0] for e in golden[name]]
    assert calls[-1] == 'raised' and set(calls[:-1]) <= {'sampling_context'}


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: python tests/test_walk_trace_host.py --record')
    text = dump(record())
    with open(GOLDEN, 'w') as f:
        f.write(text)
    print(f'{GOLDEN}: {len(CASES)} cases, {len(text)} bytes')

"""Sampler host side: schedule tables + DDPM / DDIM loops driving the native denoiser.

Mirrors the sampling half of the reference's ``mogen/models/utils/gaussian_diffusion.py`` API
(``get_named_beta_schedule`` :235-260, ``space_timesteps`` :1346-1404, ``GaussianDiffusion`` tables
:336-387, ``p_sample_loop`` :698-797, ``ddim_sample_loop`` :925-1049, ``SpacedDiffusion`` :1407-1448)
so callers written against it keep working; the per-step arithmetic itself (network, CFG combine,
posterior / DDIM update) runs in libmotioncraft_amd.so.  The RePaint / outpainting mode of the DDIM loop
(``y = {gt, outpainting_mask}``: :492-501, :855-877, the resampling ``harmonize`` loop :1050-1118 and its jump
schedule ``mogen/models/utils/scheduler.py:178-208``) is covered too.  ``dpm_solver_sample_loop`` (DPM-Solver++ 2M, ``multistep_coefs``,
``logsnr_timesteps``) is this project's own: the reference has no second-order sampler.  Training losses, learned variances and
cond_fn guidance are outside this path and raise loudly.
"""
import contextlib
import enum
import itertools
import math

import numpy as np
import torch

from . import lib as _lib

FUSED_NOISE_CHUNK_BYTES = 512 << 20     # the fused loop with step_noise gathers the draws into [steps, B, T, C] chunks of at most this


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    if schedule_name == 'linear':
        k = 1000 / num_diffusion_timesteps
        return np.linspace(k * 0.0001, k * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == 'cosine':
        f = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
        n = num_diffusion_timesteps
        return np.array([min(1 - f((i + 1) / n) / f(i / n), 0.999) for i in range(n)], dtype=np.float64)
    raise NotImplementedError(f'unknown beta schedule: {schedule_name}')


def space_timesteps(num_timesteps, section_counts):
    """Retained original timesteps for a respacing spec ('15,15,8,6,6', [..], 'ddimN', or 'logsnrN': the linear schedule's
    ``logsnr_timesteps``; ``build_diffusion`` passes the configured schedule's betas itself)."""
    if isinstance(section_counts, str):
        if section_counts.startswith('logsnr'):
            return logsnr_timesteps(num_timesteps, int(section_counts[6:]))
        if section_counts.startswith('ddim'):
            want = int(section_counts[4:])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == want:
                    return set(range(0, num_timesteps, stride))
            raise ValueError(f'cannot create exactly {num_timesteps} steps with an integer stride')
        section_counts = [int(v) for v in section_counts.split(',')]
    base, extra = divmod(num_timesteps, len(section_counts))
    kept, start = [], 0
    for i, count in enumerate(section_counts):
        size = base + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f'cannot divide section of {size} steps into {count}')
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        pos = 0.0
        for _ in range(count):
            kept.append(start + round(pos))
            pos += stride
        start += size
    return set(kept)


def logsnr_timesteps(num_timesteps_or_betas, S):
    """Original timesteps for ``SpacedDiffusion(use_timesteps=...)`` spaced uniformly in the log-SNR half
    ``lambda(t) = log(sqrt(ab_t) / sqrt(1 - ab_t))``: ``S`` points between ``lambda(T-1)`` and ``lambda(0)``, each snapped to the
    integer timestep whose ``lambda`` is nearest.  ``T-1`` and ``0`` are always in the set.  Neighbouring points can snap to the same
    timestep (the schedule is flat in ``lambda`` where it is steep in ``t``), so the set may hold FEWER than ``S`` values.  An
    integer argument means the linear schedule of that many steps; otherwise it is the ``betas`` array."""
    if np.ndim(num_timesteps_or_betas) == 0:
        betas = get_named_beta_schedule('linear', int(num_timesteps_or_betas))
    else:
        betas = np.asarray(num_timesteps_or_betas, dtype=np.float64)
    S, T = int(S), len(betas)
    if S < 2 or T < 2:
        raise ValueError(f'logsnr_timesteps: S={S} points of a {T}-step schedule (both must be at least 2)')
    ac = np.cumprod(1.0 - betas)
    lam = 0.5 * (np.log(ac) - np.log1p(-ac))                   # decreasing in t
    kept = {0, T - 1}
    for v in np.linspace(lam[T - 1], lam[0], S):
        j = int(np.searchsorted(-lam, -v))                      # first t with lam[t] <= v
        j = min(max(j, 0), T - 1)
        if j > 0 and abs(lam[j - 1] - v) <= abs(lam[j] - v):
            j -= 1
        kept.add(j)
    return kept


class GaussianDiffusion:
    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type=None, rescale_timesteps=False,
                 opt=None):
        self.opt = opt
        self.model_mean_type, self.model_var_type, self.loss_type = model_mean_type, model_var_type, loss_type
        self.rescale_timesteps = rescale_timesteps
        betas = np.array(betas, dtype=np.float64)
        if betas.ndim != 1 or not ((betas > 0).all() and (betas <= 1).all()):
            raise ValueError('betas must be a 1-D array in (0, 1]')
        self.betas = betas
        self.num_timesteps = int(betas.shape[0])
        if not hasattr(self, 'timestep_map'):
            self.timestep_map = list(range(self.num_timesteps))
        alphas = 1.0 - betas
        ac = np.cumprod(alphas, axis=0)
        self.alphas_cumprod = ac
        self.alphas_cumprod_prev = np.append(1.0, ac[:-1])
        self.alphas_cumprod_next = np.append(ac[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(ac)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - ac)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / ac)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / ac - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - ac)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - ac)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - ac)

    # ------------------------------------------------------------------------------------------
    def _check_supported(self, clip_denoised, denoised_fn, cond_fn, model_kwargs, pre_seq=None, transl_req=None):
        if self.model_mean_type != ModelMeanType.START_X:
            raise NotImplementedError('the MI355X path implements model_mean_type="start_x" (all stmogen configs)')
        if self.model_var_type != ModelVarType.FIXED_LARGE:
            raise NotImplementedError('the MI355X path implements model_var_type="fixed_large" (all stmogen configs)')
        if clip_denoised or denoised_fn is not None or cond_fn is not None:
            raise NotImplementedError('clip_denoised / denoised_fn / cond_fn are not on the MotionDiffusion eval path '
                                      '(diffusion_architecture.py:177-191 passes clip_denoised=False)')

    def _inpaint_operands(self, mode, model_kwargs, shape, device):
        """y = {gt, outpainting_mask} of the long-sequence windows (tools/m2d_test.py:177-195) -> device operands,
        or None when the mode is off (no mask / all-False mask, like the reference's ``True in mask`` tests)."""
        y = (model_kwargs or {}).get('y', {}) or {}
        if 'outpainting_mask' not in y:
            return None
        keep = y['outpainting_mask']
        if keep.dtype != torch.bool or tuple(keep.shape) != tuple(shape):
            raise AssertionError('outpainting_mask must be a bool tensor of the shape of the sample')
        if not bool(keep.any()):
            return None
        if 'gt' not in y:
            if mode == 'ddpm':
                return None                 # p_mean_variance :493-496 needs both keys, p_sample has no other use
            raise KeyError('gt')
        if tuple(y['gt'].shape) != tuple(shape):
            raise AssertionError('gt must have the shape of the sample')
        if mode == 'ddim' and self.opt is None:
            raise ValueError("the outpainting mode of ddim_sample reads opt.overlap_len / opt.addBlend: build the "
                             "architecture with cfg.model['opt'] = args as the reference tools do")
        return dict(keep=keep.to(device).contiguous(), gt=y['gt'].to(device=device, dtype=torch.float32).contiguous())

    def _cfg_weight(self, i, scale):
        """the text branch's share of the classifier-free combination at spaced index i (the other branch gets 1 - w)"""
        return (1 - (1000 - int(self.timestep_map[i])) / 1000) * scale + 1

    def step_coefs(self, i, mode, scale, eta=0.0):
        """fp64 tables -> fp32 scalars exactly like _extract_into_tensor(...).float()."""
        w = self._cfg_weight(i, scale)
        c = _lib.StepCoefs()
        c.mode = 0 if mode == 'ddpm' else 1
        c.text_coef, c.none_coef = w, 1 - w
        c.c1, c.c2 = self.posterior_mean_coef1[i], self.posterior_mean_coef2[i]
        c.log_var = math.log(self.posterior_variance[1] if i == 0 else self.betas[i])
        c.sqrt_recip, c.sqrt_recipm1 = self.sqrt_recip_alphas_cumprod[i], self.sqrt_recipm1_alphas_cumprod[i]
        c.ab, c.ab_prev, c.eta = self.alphas_cumprod[i], self.alphas_cumprod_prev[i], eta
        c.nonzero = 0.0 if i == 0 else 1.0
        return c

    def multistep_coefs(self, indices, scale, order=2):
        """DPM-Solver++ (2M) on the data prediction: the ``StepCoefs`` (mode 2) of a whole walk through the schedule indices
        ``indices``.  Every update is ``x_prev = kx x + k0 x0 + k1 x0_prev`` (``c2``, ``c1`` and ``eta`` of the struct), computed in fp64
        and cast to fp32 like ``step_coefs`` casts its tables.  With ``alpha = sqrt(ab)``, ``sigma = sqrt(1 - ab)``, ``lambda =
        log(alpha / sigma)``, s = index i and t = the level below it, ``h = lambda_t - lambda_s``:

          order 1:  kx = sigma_t / sigma_s,  k0 = -alpha_t expm1(-h),  k1 = 0          (DDIM with eta = 0)
          order 2:  r = h_prev / h,  k0 = -alpha_t expm1(-h) (1 + 1 / (2 r)),  k1 = alpha_t expm1(-h) / (2 r)

        ``k1`` weighs the x0 of the step taken just before, so the coefficients belong to the sequence, not to an index.  First-order
        are: the first step of the walk (no history), the step at i == 1 (the last one with a finite h: the lower-order final step,
        always on) and the step at i == 0, which has sigma_t = 0 and is emitted as exactly (0, 1, 0): x_prev = x0."""
        if order not in (1, 2):
            raise ValueError(f'order={order!r}: the multistep solver is implemented for order 1 and 2')
        out, h_prev = [], None
        for i in indices:
            i = int(i)
            w = self._cfg_weight(i, scale)
            c = _lib.StepCoefs()
            c.mode = _lib.MC_SAMPLER_MULTISTEP
            c.text_coef, c.none_coef = w, 1 - w
            ab_s, ab_t = float(self.alphas_cumprod[i]), float(self.alphas_cumprod_prev[i])
            if ab_t >= 1.0:
                kx, k0, k1, h = 0.0, 1.0, 0.0, None
            else:
                a_s, s_s, a_t, s_t = math.sqrt(ab_s), math.sqrt(1 - ab_s), math.sqrt(ab_t), math.sqrt(1 - ab_t)
                h = math.log(a_t / s_t) - math.log(a_s / s_s)
                kx, k0, k1 = s_t / s_s, -a_t * math.expm1(-h), 0.0
                if order == 2 and h_prev is not None and i != 1:
                    r = h_prev / h
                    k0, k1 = k0 * (1 + 1 / (2 * r)), -k0 / (2 * r)
            c.c2, c.c1, c.eta = kx, k0, k1
            c.ab, c.ab_prev = ab_s, ab_t            # (informative: mode 2 reads c1, c2, eta and the two CFG weights only)
            c.nonzero = 0.0 if i == 0 else 1.0
            out.append(c)
            h_prev = h
        return out

    @staticmethod
    def _seams_of(model_kwargs, graph, pre_seq, transl_req):
        """``model_kwargs['seams'] = dict(first_frame=..., overlap=..., weights=None)``: the rows of the batch are coupled windows of a
        long sequence (``NativeContext.set_seams``; ``longform.sample_long_coupled`` builds it).  What does not go with it raises here,
        before anything runs."""
        seams = (model_kwargs or {}).get('seams', None)
        if seams is None:
            return None
        if graph:
            raise ValueError('graph replay does not cover coupled windows (model_kwargs["seams"]): the captured step is the uncoupled one')
        keep = ((model_kwargs.get('y', {}) or {}).get('outpainting_mask', None))
        if keep is not None and bool(keep.any()):
            raise NotImplementedError('coupled windows (model_kwargs["seams"]) together with an outpainting mask (RePaint)')
        if pre_seq is not None or transl_req:
            raise NotImplementedError('coupled windows (model_kwargs["seams"]) together with pre_seq / transl_req seeding')
        extra = set(seams) - {'first_frame', 'overlap', 'weights'}
        if extra or 'first_frame' not in seams or 'overlap' not in seams:
            raise ValueError(f'model_kwargs["seams"]: dict(first_frame=..., overlap=..., weights=None), got keys {sorted(seams)}')
        return dict(first_frame=seams['first_frame'], overlap=seams['overlap'], weights=seams.get('weights', None))

    @staticmethod
    def _seeds_of(seeds, shape, noise, step_noise, generator, transl_req=None):
        """``seeds``: one Philox key per batch row (``NativeContext.set_row_seeds``) -- x_T is draw 0 of every row's own stream and
        the n-th ``randn_like`` of the walk is draw ``1 + n``, so a row's noise depends on its seed alone.  Exclusive with every other
        source of noise."""
        if seeds is None:
            return None
        if noise is not None or step_noise is not None or generator is not None:
            raise ValueError('seeds= is exclusive with noise=, step_noise= and generator=: every draw comes from the rows\' own streams')
        if transl_req:
            raise NotImplementedError('seeds= together with transl_req: its randn(2) draws are per call, not per row')
        from .engine import check_seeds
        return check_seeds(seeds, shape[0])

    # ---- the walk: one description of the call, one context, one table guard, one x_T, one step loop -------------
    def _sample(self, run):
        """The walk of one public call.  With ``model_kwargs['seams']`` the context's seam table is set before it and cleared after
        it, whatever happens in between (per-step and fused path alike: the library picks the coupled update wherever a table is set);
        the seed table of ``seeds`` likewise."""
        if run.model_kwargs is None:
            run.model_kwargs = {}
        if not isinstance(run.shape, (tuple, list)):
            raise AssertionError('shape must be a tuple or list')
        B, T, C = run.shape
        if run.device is None:
            run.device = torch.device('cuda', torch.cuda.current_device())
        inp = None if run.mode == 'dpmpp' else self._inpaint_operands(run.mode, run.model_kwargs, run.shape, run.device)
        ctx = run.model.sampling_context(B, T, self.timestep_map, run.model_kwargs, run.device)
        with _tables(ctx, run.seams, run.seeds):
            img = self._walk(ctx, run, inp, self._x_T(ctx, run))
            if getattr(ctx, 'uses_coop_routing', False):
                ctx.check()            # one sync after the last step: a timed-out grid barrier of the routing kernel raises here
        return img

    @staticmethod
    def _x_T(ctx, run):
        if run.seeds is not None:
            return ctx.draw_rows(0)                                           # draw 0 of every row's own stream
        if run.noise is not None:
            return run.noise.to(device=run.device, dtype=torch.float32).contiguous().clone()
        return torch.randn(*run.shape, device=run.device, generator=run.generator)

    def _coefs(self, run, indices):
        """the ``StepCoefs`` at the schedule indices ``indices``.  k1 of a multistep step belongs to the walk: those are picked from the
        coefficients of the whole descent, so a truncated run is a prefix of it"""
        scale = run.model.cfg_scale
        if run.mode == 'dpmpp':
            whole = self.multistep_coefs(range(self.num_timesteps - 1, -1, -1), scale, run.order)[::-1]
            return [whole[i] for i in indices]
        return [self.step_coefs(i, run.mode, scale, run.eta) for i in indices]

    def _plan(self, run, inp):
        """the schedule: (i, StepCoefs) = denoise at spaced index i, (i, None) = forward "undo" step with beta[i]"""
        if inp is not None and run.mode == 'ddim' and not getattr(self.opt, 'no_repaint', False):
            if run.num_steps is not None:
                raise ValueError('num_steps truncation is not defined for the resampling schedule')
            n_ddim = int(str(self.opt.timestep_respacing)[4:])
            if getattr(self.opt, 'no_resample', False):
                times = get_schedule_jump_cjm_ddim(n_ddim)
            else:
                times = get_schedule_jump_cjm_ddim(n_ddim, jump_length=self.opt.jump_length,
                                                   jump_n_sample=self.opt.jump_n_sample)
            if max(times) >= self.num_timesteps:
                raise ValueError(f'opt.timestep_respacing={self.opt.timestep_respacing!r} starts the resampling loop at '
                                 f'step {max(times)} of a {self.num_timesteps}-step schedule')
            visits = [(a, b < a) for a, b in zip(times[:-1], times[1:])]
        else:
            visits = [(i, True) for i in list(range(self.num_timesteps))[::-1][:run.num_steps]]
        coefs = iter(self._coefs(run, [i for i, down in visits if down]))
        return [(i, next(coefs) if down else None) for i, down in visits]

    @staticmethod
    def _seeding(run, inp):
        """p_sample :664-674 / ddim_sample :816-820: every step re-noises pre_seq (and the requested translation channels of frames
        0-1) to the step's level and writes it over the first frames of x before the network call.  -> None (no seeding), or
        (pre_seq on the device or None, the transl_req items as lists)"""
        pre_seq, step_noise = run.pre_seq, run.step_noise
        if pre_seq is None and not run.transl_req:
            return None
        if inp is not None:
            raise NotImplementedError('pre_seq / transl_req together with the outpainting mask: no reference tool combines them')
        B, T, C = run.shape
        if pre_seq is not None:
            pre_seq = pre_seq.to(device=run.device, dtype=torch.float32).contiguous()
            if pre_seq.dim() != 3 or pre_seq.shape[0] != B or pre_seq.shape[2] != C or pre_seq.shape[1] > T:
                raise RuntimeError(f'pre_seq of shape {tuple(pre_seq.shape)} cannot be written into x[:, :T, :] of {tuple(run.shape)}')
        transl_req = [list(it) for it in (run.transl_req or [])]
        if transl_req and B > 2:
            # _extract_into_tensor(arr, t, (2,)) expands a [B] tensor to (2,): the reference raises for B > 2 as well
            raise RuntimeError(f'transl_req: the expanded size of the tensor (2) must match the batch size ({B})')
        if any(len(it) != 3 for it in transl_req):
            raise ValueError('transl_req items are [channel, value_frame0, value_frame1]')
        if step_noise is not None and not hasattr(step_noise, '__next__'):
            raise ValueError('with pre_seq / transl_req several tensors of different shapes are drawn per step: '
                             'step_noise must be an iterator yielding them in the order the reference draws them '
                             '(randn_like(pre_seq), one randn(2) per transl_req item, randn_like(x))')
        return pre_seq, transl_req

    @staticmethod
    def _draws(ctx, run, inp):
        """-> ``draw(i)``: the next randn_like(x) of the reference loop; in the outpainting mode several are drawn per step, so there
        ``step_noise`` is an iterator (or a callable of the running draw number).  The multistep walk draws nothing."""
        if run.mode == 'dpmpp':
            return lambda i: None
        step_noise, device = run.step_noise, run.device
        if inp is not None and step_noise is not None and not (hasattr(step_noise, '__next__') or callable(step_noise)):
            raise ValueError('the outpainting mode draws several independent randn_like tensors per step index: '
                             'step_noise must be an iterator or a callable of the running draw number there, not a '
                             'sequence indexed by step (every draw of a step would get the same tensor)')
        count = itertools.count()

        def draw(i):
            n = next(count)
            if run.seeds is not None:
                return ctx.draw_rows(1 + n)                                   # the n-th randn_like of the walk: draw 1 + n
            if step_noise is None:
                return torch.randn(*run.shape, device=device, generator=run.generator)
            if hasattr(step_noise, '__next__'):
                e = next(step_noise)
            elif callable(step_noise):
                e = step_noise(n if inp is not None else i)
            else:
                e = step_noise[i]
            return e.to(device=device, dtype=torch.float32).contiguous()
        return draw

    def _seeded_step(self, ctx, run, seeding, draw):
        pre_seq, transl_req = seeding
        step_noise, generator, device = run.step_noise, run.generator, run.device

        def step(i, c, x, nxt, x0):
            a_, b_ = np.float32(self.sqrt_alphas_cumprod[i]), np.float32(self.sqrt_one_minus_alphas_cumprod[i])
            pre_noise = None
            if pre_seq is not None and run.seeds is not None:
                pre_noise = draw(i)[:, :pre_seq.shape[1]].contiguous()        # a smaller tensor: the leading elements of each row's draw
            elif pre_seq is not None:
                pre_noise = (next(step_noise).to(device=device, dtype=torch.float32).contiguous() if step_noise is not None
                             else torch.randn(*pre_seq.shape, device=device, generator=generator))
            transl = []
            for it in transl_req:                                            # th.randn(2) on the host, then q_sample in fp32
                n2 = (next(step_noise) if step_noise is not None else torch.randn(2, generator=generator if generator is not None and generator.device.type == 'cpu' else None))
                n2 = n2.detach().cpu().numpy().astype(np.float32)
                v = a_ * np.asarray(it[1:], dtype=np.float32) + b_ * n2
                transl.append((int(it[0]), float(v[0]), float(v[1])))
            ctx.sample_step_seeded(x, i, c, draw(i), a_, b_, pre_seq=pre_seq, pre_noise=pre_noise, transl=transl, x_prev=nxt, x0=x0)
        return step

    def _inpaint_step(self, ctx, run, inp, draw):
        T, blend_w = run.shape[1], None
        if run.mode == 'ddim':
            ov = int(self.opt.overlap_len)
            if not 0 <= ov <= T:
                raise ValueError(f'opt.overlap_len={ov} outside the {T}-frame window')
            blend_w = torch.linspace(0, 1, ov, device=run.device) if ov > 0 else None

        def step(i, c, x, nxt, x0):
            eps = draw(i)
            gt_noise, blend_len = None, 0
            if run.mode == 'ddim':
                gt_noise = draw(i)                                            # :868
                noise_weight = np.sqrt(np.float32(1) - np.float32(self.alphas_cumprod_prev[i]))
                if noise_weight < np.float32(0.2) and getattr(self.opt, 'addBlend', True) and blend_w is not None:
                    blend_len = int(self.opt.overlap_len)                     # :872-875
            ctx.sample_step_inpaint(x, i, c, eps, inp['gt'], inp['keep'], gt_noise=gt_noise, blend_w=blend_w, blend_len=blend_len,
                                    x_prev=nxt, x0=x0)
        return step

    def _walk(self, ctx, run, inp, img):
        mode, scale = run.mode, run.model.cfg_scale
        plan = self._plan(run, inp)
        if run.progress:
            from tqdm.auto import tqdm
            plan = tqdm(plan)
        seeding = self._seeding(run, inp)
        draw = self._draws(ctx, run, inp)
        if seeding is not None:
            denoise = self._seeded_step(ctx, run, seeding, draw)
        elif inp is not None:
            denoise = self._inpaint_step(ctx, run, inp, draw)
        else:                                                                 # (eps is drawn every step, DDIM too; None in the multistep walk)
            denoise = lambda i, c, x, nxt, x0: ctx.sample_step(x, i, c, draw(i), x_prev=nxt, x0=x0)    # noqa: E731
        plain = inp is None and seeding is None and run.trajectory is None
        if run.graph:
            # hipGraph replay (BASELINE configs[4]): one captured graph of the step for the whole schedule, x updated in
            # place, the per-step noise refilled in place; bit-identical to the eager sequence, 2-3 % faster for B <= 4
            # (profiles/r02_graph_vs_eager.txt)
            if not plain:
                raise ValueError('graph replay covers the plain step (no trajectory)' if mode == 'dpmpp' else
                                 'graph replay covers the plain p_sample / ddim_sample step (no outpainting, seeding or trajectory)')
            key = (mode, int(run.order) if mode == 'dpmpp' else float(run.eta), float(scale), tuple(int(t) for t in self.timestep_map))
            return _replay(ctx, run.device, img, key, lambda: self._coefs(run, range(self.num_timesteps)), (i for i, _ in plan),
                           None if mode == 'dpmpp' else draw)
        if run.fused and plain and not run.progress:
            self._fused(ctx, run, img, plan, draw)
            return img
        nxt = torch.empty_like(img)
        x0 = torch.empty_like(img) if run.trajectory is not None else None
        for i, c in plan:
            if c is None:                                                     # _undo (:429-435)
                beta = np.float32(self.betas[i])
                ctx.renoise(img, draw(i), np.sqrt(np.float32(1) - beta), np.sqrt(beta), out=nxt)
            else:
                denoise(i, c, img, nxt, x0)
            img, nxt = nxt, img
            if run.trajectory is not None:
                run.trajectory.append((i, img.clone(), x0.clone()))
        return img

    @staticmethod
    def _fused(ctx, run, img, plan, draw):
        """The whole loop inside the library (mc_sample_loop): no return to Python between steps.  Without step_noise the per-step
        randn_like is drawn INSIDE the sampler-update kernel (Philox4x32-10; the loop's 64-bit key is one draw from `generator`, so a
        seeded generator reproduces the run and successive calls differ; with ``seeds`` step k is draw 1 + k of every row's own stream;
        the multistep walk draws nothing); with step_noise the draws are gathered into [steps, B, T, C] chunks of at most
        ``FUSED_NOISE_CHUNK_BYTES`` and the same entry point reads them"""
        idx, coefs = [i for i, _ in plan], [c for _, c in plan]
        if run.step_noise is not None:
            chunk = max(1, int(FUSED_NOISE_CHUNK_BYTES // (4 * img.numel())))
            for k0 in range(0, len(idx), chunk):
                part = idx[k0:k0 + chunk]
                ctx.sample_loop(img, part, coefs[k0:k0 + chunk], noise=torch.stack([draw(i) for i in part]))
            return
        seed, draw0 = 0, 0
        if run.mode == 'dpmpp':
            pass
        elif run.seeds is not None:
            draw0 = 1
        else:
            gdev = run.generator.device if run.generator is not None else torch.device('cpu')
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=run.generator, device=gdev).item())
        ctx.sample_loop(img, idx, coefs, noise=None, seed=seed, draw0=draw0)

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, pre_seq=None, transl_req=None, progress=False,
                      step_noise=None, generator=None, num_steps=None, trajectory=None, graph=False, fused=True, seeds=None):
        """gaussian_diffusion.py:698-797.  Extras beside the reference's arguments: ``step_noise`` (the per-step draws, for runs on
        the reference's seeds), ``generator``, ``num_steps``, ``trajectory``, ``graph`` (hipGraph replay) and ``fused`` (default:
        the whole loop is ONE library call, mc_sample_loop, with the per-step noise drawn on the device when no step_noise is
        given; False: one mc_sample_step per step with torch.randn draws).  ``seeds``: B ints in [0, 2^64), one per batch row -- x_T and
        every per-step draw then come from the row's own Philox stream (``_seeds_of``), the same bits on the fused, the per-step and
        the graph path; exclusive with ``noise``, ``step_noise`` and ``generator``."""
        self._check_supported(clip_denoised, denoised_fn, cond_fn, model_kwargs, pre_seq, transl_req)
        return self._sample(_Run('ddpm', model, shape, noise=noise, model_kwargs=model_kwargs, device=device, progress=progress,
                                             step_noise=step_noise, generator=generator, num_steps=num_steps, trajectory=trajectory,
                                             pre_seq=pre_seq, transl_req=transl_req, graph=graph, fused=fused, seeds=seeds))

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, pre_seq=None,
                         step_noise=None, generator=None, num_steps=None, trajectory=None, graph=False, fused=True, seeds=None):
        self._check_supported(clip_denoised, denoised_fn, cond_fn, model_kwargs, pre_seq)
        if self.opt is not None and getattr(self.opt, 'same_overlap_noisy', False):
            raise NotImplementedError('opt.same_overlap_noisy: the reference writes self.saved_noisy_tail '
                                      '(gaussian_diffusion.py:879-881) without ever creating it, so that option has '
                                      'no defined behaviour to reproduce')
        return self._sample(_Run('ddim', model, shape, noise=noise, model_kwargs=model_kwargs, device=device, progress=progress,
                                             eta=float(eta), step_noise=step_noise, generator=generator, num_steps=num_steps,
                                             trajectory=trajectory, pre_seq=pre_seq, graph=graph, fused=fused, seeds=seeds))

    def dpm_solver_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                               model_kwargs=None, device=None, progress=False, order=2, generator=None, num_steps=None,
                               trajectory=None, graph=False, fused=True, pre_seq=None, transl_req=None, seeds=None):
        """DPM-Solver++ (2M) on the model's x0 prediction: a second-order multistep walk down the (spaced) schedule, one denoiser call
        per step like DDIM, meant for 10-20 steps (``respace='ddimN'`` or ``'logsnrN'``).  The reference has no such sampler; the
        coefficients are ``multistep_coefs`` (first-order first and last finite step, ``x = x0`` at index 0), ``order=1`` is DDIM with
        eta = 0.  Deterministic given ``noise``: no per-step draw exists, ``generator`` only draws x_T when ``noise`` is None.
        ``num_steps`` / ``trajectory`` / ``graph`` / ``fused`` as in the other two loops; ``seeds`` (one per row) draws x_T from the rows'
        own streams instead (draw 0), exclusive with ``noise`` and ``generator``.  No outpainting (RePaint) and no
        pre_seq / transl_req seeding: those raise."""
        self._check_supported(clip_denoised, denoised_fn, cond_fn, model_kwargs, pre_seq, transl_req)
        if order not in (1, 2):
            raise ValueError(f'order={order!r}: the multistep solver is implemented for order 1 and 2')
        run = _Run('dpmpp', model, shape, noise=noise, model_kwargs=model_kwargs, device=device, progress=progress, order=order,
                   generator=generator, num_steps=num_steps, trajectory=trajectory, pre_seq=pre_seq, transl_req=transl_req, graph=graph,
                   fused=fused, seeds=seeds)
        keep = (((model_kwargs or {}).get('y', {}) or {}).get('outpainting_mask', None))
        if keep is not None and bool(keep.any()):
            raise NotImplementedError('dpm_solver_sample_loop with an outpainting mask (RePaint): not implemented for the '
                                      'multistep sampler, use ddim_sample_loop')
        if pre_seq is not None:
            raise NotImplementedError('dpm_solver_sample_loop with pre_seq seeding: not implemented for the multistep sampler')
        if transl_req:
            raise NotImplementedError('dpm_solver_sample_loop with transl_req seeding: not implemented for the multistep sampler')
        return self._sample(run)


class _Run:
    """What one call of a sampler loop asked for: ``mode`` ('ddpm', 'ddim' or 'dpmpp'), the model, the shape of the sample and the
    loop's keywords.  What does not go with coupled windows or row seeds raises here, first of all; ``seams`` / ``seeds`` are the
    checked tables."""
    noise = step_noise = generator = num_steps = trajectory = pre_seq = transl_req = seeds = model_kwargs = device = None
    progress, graph, fused, eta, order = False, False, True, 0.0, 2

    def __init__(self, mode, model, shape, **asked):
        self.mode, self.model, self.shape = mode, model, shape
        self.__dict__.update(asked)
        self.seams = GaussianDiffusion._seams_of(self.model_kwargs, self.graph, self.pre_seq, self.transl_req)
        transl_req = None if mode == 'dpmpp' else self.transl_req          # (the multistep loop refuses it under its own name)
        self.seeds = GaussianDiffusion._seeds_of(self.seeds, shape, self.noise, self.step_noise, self.generator, transl_req)


@contextlib.contextmanager
def _tables(ctx, seams, seeds):
    """the seam table, then the seed table, set on ``ctx`` for the ``with`` block only: each one that was attempted is cleared once"""
    clear = []
    try:
        if seams is not None:
            clear.append(ctx.clear_seams)
            ctx.set_seams(**seams)
        if seeds is not None:
            clear.append(ctx.clear_row_seeds)
            ctx.set_row_seeds(seeds)
        yield
    finally:
        for f in clear:
            f()


def _replay(ctx, device, img, key, table, steps, refill=None):
    """``img`` through the schedule indices ``steps`` by replaying the captured graph of the step.  The graph (and the x / noise buffers
    baked into it) lives on the context and is reused by later calls with the same ``key``: capture + instantiate cost a few ms,
    more than one small-batch loop gains.  ``table()``: the ``StepCoefs`` of every schedule index, asked for when a graph is captured;
    ``refill(i)``: the noise of step i (None: the captured step reads none)."""
    now = torch.cuda.current_stream(device)
    st = getattr(ctx, '_graph_state', None)
    if st is None or st['key'] != key:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(now)
        with torch.cuda.stream(side):
            gx, nbuf = torch.empty_like(img), (torch.empty_like(img) if refill is not None else None)
            ctx.graph_capture(gx, nbuf, table())
        st = ctx._graph_state = dict(key=key, stream=side, x=gx, noise=nbuf)
    side = st['stream']
    side.wait_stream(now)
    with torch.cuda.stream(side):
        st['x'].copy_(img)
        for i in steps:
            if refill is not None:
                st['noise'].copy_(refill(i))
            ctx.graph_step(i)
        img.copy_(st['x'])
    now.wait_stream(side)
    return img


def get_schedule_jump_cjm_ddim(time_respacing=25, jump_length=1, jump_n_sample=1):
    """Visit order of the resampling ("harmonize") DDIM loop, mirrors mogen/models/utils/scheduler.py:178-208:
    start 60 % into the schedule (step 15 of 25), walk down to 0, and the first jump_n_sample-1 times a multiple
    of jump_length (below t_T - jump_length) is reached, walk jump_length steps back up first.  Ends with -1."""
    t_T = 15 if time_respacing == 25 else int(time_respacing * 0.6)
    revisits = dict.fromkeys(range(0, t_T - jump_length, jump_length), jump_n_sample - 1)
    ts, t = [], t_T - 1
    while t >= 0:
        ts.append(t)
        if revisits.get(t, 0) > 0:
            revisits[t] -= 1
            ts.extend(range(t + 1, t + jump_length + 1))
            t += jump_length
        t -= 1
    ts.append(-1)
    if any(abs(a - b) != 1 for a, b in zip(ts[:-1], ts[1:])) or ts[0] >= t_T:
        raise AssertionError('inconsistent jump schedule')
    return ts


class SpacedDiffusion(GaussianDiffusion):
    """Skips steps of a base process: betas re-derived from the retained alpha-bars; the network is
    fed ``timestep_map[i]`` (the original timestep), as the reference's ``_WrappedModel`` does."""

    def __init__(self, use_timesteps, **kwargs):
        self.use_timesteps = set(use_timesteps)
        self.original_num_steps = len(kwargs['betas'])
        base_ac = np.cumprod(1.0 - np.array(kwargs['betas'], dtype=np.float64), axis=0)
        self.timestep_map, new_betas, last = [], [], 1.0
        for i, a in enumerate(base_ac):
            if i in self.use_timesteps:
                new_betas.append(1 - a / last)
                last = a
                self.timestep_map.append(i)
        kwargs['betas'] = np.array(new_betas)
        super().__init__(**kwargs)


def build_diffusion(cfg, opt=None):
    """cfg = diffusion_test / diffusion_train dict of the configs (diffusion_architecture.py:25-54)."""
    betas = get_named_beta_schedule(cfg['beta_scheduler'], cfg['diffusion_steps'])
    mean_type = {'start_x': ModelMeanType.START_X, 'previous_x': ModelMeanType.PREVIOUS_X,
                 'epsilon': ModelMeanType.EPSILON}[cfg['model_mean_type']]
    var_type = {'learned': ModelVarType.LEARNED, 'fixed_small': ModelVarType.FIXED_SMALL,
                'fixed_large': ModelVarType.FIXED_LARGE, 'learned_range': ModelVarType.LEARNED_RANGE}[cfg['model_var_type']]
    if cfg.get('respace', None) is not None:
        respace = cfg['respace']
        if isinstance(respace, str) and respace.startswith('logsnr'):
            use = logsnr_timesteps(betas, int(respace[6:]))
        else:
            use = space_timesteps(cfg['diffusion_steps'], respace)
        return SpacedDiffusion(use_timesteps=use, betas=betas,
                               model_mean_type=mean_type, model_var_type=var_type, loss_type=LossType.MSE, opt=opt)
    return GaussianDiffusion(betas=betas, model_mean_type=mean_type, model_var_type=var_type, loss_type=LossType.MSE)

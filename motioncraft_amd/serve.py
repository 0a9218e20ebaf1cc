"""Independent requests through one batched context: ``Request`` + ``RequestBatcher``.

The library is fastest when it batches, and with row-keyed noise (``seeds=``) and drop-free MoE routing (``capacity_factor=0``) a row
of a batch is a request: its result does not depend on what the other rows hold.

Contract: the result of a request is a function of (the request, ``batch``, ``frames``, the sampler settings, ``capacity_factor = 0``)
only.  It does not depend on the other requests, on the submission order or on the row the request lands in -- bit for bit, because
every model call here has the same shape (open rows are filled with a fixed dummy request, never left out).  Across *different*
``batch`` / ``frames`` the library picks other kernels (small-batch GEMMs, split-K), so there only a tolerance holds.  With a
``capacity_factor`` other than 0 tokens are dropped by whole-batch ranking and the contract does not hold.

Checkpoints were trained with drops (capacity factor 1.5); sample quality at 0 is unmeasured.
"""
import torch

SAMPLERS = ('ddpm', 'ddim', 'dpmpp')
DUMMY_SEED = 0


class Request:
    """One generation request: the condition (``xf_out`` [Nt, Dt], the text encoder's output -- or ``text``, encoded on submit),
    ``length`` frames (1 .. the batcher's ``frames``), ``seed`` in [0, 2^64) and optionally a control condition ``c`` [Tc, Fc]."""

    def __init__(self, length, seed, xf_out=None, text=None, c=None):
        if (xf_out is None) == (text is None):
            raise ValueError('a request carries exactly one of xf_out and text')
        if text is not None and not isinstance(text, str):
            raise ValueError(f'text must be a string, got {type(text).__name__}')
        if isinstance(length, bool) or int(length) != length or int(length) < 1:
            raise ValueError(f'length must be a positive integer, got {length!r}')
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f'seed must be an integer in [0, 2^64), got {seed!r}')
        if xf_out is not None and xf_out.dim() != 2:
            raise ValueError(f'xf_out of one request is [Nt, Dt], got {tuple(xf_out.shape)}')
        if c is not None and c.dim() != 2:
            raise ValueError(f'the control condition of one request is [Tc, Fc], got {tuple(c.shape)}')
        self.length, self.seed, self.xf_out, self.text, self.c = int(length), int(seed), xf_out, text, c


class RequestBatcher:
    """``submit()`` requests, ``run()`` them ``batch`` at a time through one (batch, frames) context.

    ``model``: a ``MotionDiffusion`` (its denoiser and its test schedule's configuration are used).  ``sampler`` in ``SAMPLERS``;
    ``steps``: respace the schedule to that many steps (None: the configured schedule).  ``runner`` replaces the model call (tests):
    ``runner(xf_out [B,Nt,Dt], lengths [B], seeds [B], c [B,Tc,Fc] or None) -> [B, frames, C]``."""

    def __init__(self, model, batch, frames, sampler='ddim', steps=None, capacity_factor=0, eta=0.0, order=2, runner=None):
        if sampler not in SAMPLERS:
            raise ValueError(f'sampler {sampler!r}: one of {SAMPLERS}')
        if int(batch) < 1 or int(frames) < 1:
            raise ValueError(f'batch and frames must be positive, got {batch!r}, {frames!r}')
        if steps is not None and int(steps) < 1:
            raise ValueError(f'steps must be positive, got {steps!r}')
        if float(capacity_factor) < 0:
            raise ValueError(f'capacity_factor must be >= 0, got {capacity_factor!r}')
        self.model, self.batch, self.frames = model, int(batch), int(frames)
        self.sampler, self.steps, self.capacity_factor = sampler, None if steps is None else int(steps), float(capacity_factor)
        self.eta, self.order = float(eta), int(order)
        self.runner = runner if runner is not None else self._run_model
        self._diffusion = None
        self._pending = []             # (handle, Request with xf_out set)
        self._next = 0

    # ---- queue ------------------------------------------------------------------------------------
    def submit(self, request):
        """Queue ``request``; -> its handle (the key of ``run()``'s result)."""
        if not isinstance(request, Request):
            raise ValueError('submit() takes a Request')
        if request.length > self.frames:
            raise ValueError(f'request of {request.length} frames in a batcher of {self.frames}')
        if request.xf_out is None:
            # one prompt per encoder call: the condition of a request must not depend on what it is encoded beside
            xf = self.model.model.encode_text([request.text], None, None)[0]
            request = Request(request.length, request.seed, xf_out=xf, c=request.c)
        handle = self._next
        self._next += 1
        self._pending.append((handle, request))
        return handle

    def plan(self):
        """The model calls ``run()`` will make: a list of batches, each a list of ``batch`` entries -- a pending handle, or None for a
        row filled with the dummy request.  Requests with a control condition (of one shape) and requests without never share a call:
        the control branch is on or off per call."""
        groups = {}
        for handle, r in self._pending:
            groups.setdefault(None if r.c is None else tuple(r.c.shape), []).append(handle)
        out = []
        for handles in groups.values():
            for k in range(0, len(handles), self.batch):
                part = handles[k:k + self.batch]
                out.append(part + [None] * (self.batch - len(part)))
        return out

    def run(self):
        """Run every pending request; -> ``{handle: pred_motion[:length]}`` (de-normalised by the model's ``post_process``)."""
        reqs = dict(self._pending)
        results = {}
        for rows in self.plan():
            first = reqs[rows[0]]
            xf = torch.stack([reqs[h].xf_out if h is not None else torch.zeros_like(first.xf_out) for h in rows])
            lengths = [reqs[h].length if h is not None else self.frames for h in rows]
            seeds = [reqs[h].seed if h is not None else DUMMY_SEED for h in rows]
            c = None
            if first.c is not None:
                c = torch.stack([reqs[h].c if h is not None else torch.zeros_like(first.c) for h in rows])
            pred = self.runner(xf, lengths, seeds, c)
            for b, h in enumerate(rows):
                if h is not None:
                    results[h] = pred[b, :reqs[h].length]
        self._pending = []
        return results

    # ---- the model call ---------------------------------------------------------------------------
    def _schedule(self):
        if self._diffusion is None:
            from .diffusion import build_diffusion
            cfg = dict(self.model.diffusion_test_cfg)
            if self.steps is not None:
                cfg['respace'] = str(self.steps) if self.sampler == 'ddpm' else f'ddim{self.steps}'
            self._diffusion = build_diffusion(cfg, opt=self.model.opt)
        return self._diffusion

    def _run_model(self, xf_out, lengths, seeds, c):
        net, diffusion = self.model.model, self._schedule()
        dev = torch.device('cuda', torch.cuda.current_device())
        B, T, C = self.batch, self.frames, net.dims['input_feats']
        mask = torch.zeros(B, T, device=dev)
        for b, n in enumerate(lengths):
            mask[b, :n] = 1
        kw = dict(xf_out=xf_out.to(dev), motion_mask=mask, motion_length=torch.tensor(lengths, device=dev).long(), c=c, y={},
                  capacity_factor=self.capacity_factor)
        common = dict(clip_denoised=False, progress=False, model_kwargs=kw, seeds=seeds)
        if self.sampler == 'ddpm':
            out = diffusion.p_sample_loop(net, (B, T, C), **common)
        elif self.sampler == 'ddim':
            out = diffusion.ddim_sample_loop(net, (B, T, C), eta=self.eta, **common)
        else:
            out = diffusion.dpm_solver_sample_loop(net, (B, T, C), order=self.order, **common)
        return net.post_process(out)

"""Independent requests through one batched context: ``Request`` + ``RequestBatcher`` (whole batches, one walk per call) and
``ContinuousBatcher`` (requests join a running batch at any step and leave when their own walk ends: DESIGN.md section 4o; with
``overlap=`` a request longer than ``frames`` runs as seam-coupled windows on any open rows: section 4q).

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


class Edit:
    """The given part of a motion: ``motion`` [n, C] in de-normalised (data) space and ``keep`` bool [n, C] --
    where ``keep`` is set the element is given, everything else (and frames n .. the request's length) is generated around it.
    ``keyframes`` / ``inbetween`` / ``parts`` build the usual masks.  The batchers normalise ``motion`` with the model's
    ``pre_process`` and hand the row to ``mc_ctx_set_edit_rows``; at the end of the walk the kept elements ARE the given ones."""

    def __init__(self, motion, keep):
        if not isinstance(motion, torch.Tensor) or motion.dim() != 2 or not motion.is_floating_point():
            raise ValueError(f'motion of an edit is a float tensor [n, C], got {getattr(motion, "shape", type(motion).__name__)}')
        if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or tuple(keep.shape) != tuple(motion.shape):
            raise ValueError(f'keep must be a bool tensor of motion\'s shape {tuple(motion.shape)}, got '
                             f'{getattr(keep, "dtype", type(keep).__name__)} {tuple(getattr(keep, "shape", ()))}')
        if motion.shape[0] < 1:
            raise ValueError('an edit holds at least one frame')
        if not bool(keep.any()):
            raise ValueError('keep is all False: nothing is given (submit the request without an edit)')
        if not bool(torch.isfinite(motion[keep]).all()):
            raise ValueError('motion is not finite where keep is set')
        self.motion, self.keep = motion, keep

    @property
    def frames(self):
        return int(self.motion.shape[0])

    @property
    def feats(self):
        return int(self.motion.shape[1])

    @staticmethod
    def _frame_list(frames, n):
        out = []
        for f in frames:
            if isinstance(f, bool) or int(f) != f or not 0 <= int(f) < n:
                raise ValueError(f'frame {f!r} outside the {n} frames of motion')
            out.append(int(f))
        if not out:
            raise ValueError('no frame given')
        return out

    @classmethod
    def keyframes(cls, motion, frames):
        """``frames`` of ``motion`` are given on all channels"""
        keep = torch.zeros(motion.shape, dtype=torch.bool)
        keep[cls._frame_list(frames, motion.shape[0])] = True
        return cls(motion, keep)

    @classmethod
    def inbetween(cls, motion, head, tail):
        """the first ``head`` and the last ``tail`` frames of ``motion`` are given, the frames between them generated"""
        n = motion.shape[0]
        for v in (head, tail):
            if isinstance(v, bool) or int(v) != v or int(v) < 0:
                raise ValueError(f'head / tail are frame counts, got {v!r}')
        if head + tail < 1 or head + tail > n:
            raise ValueError(f'head + tail = {head + tail} outside [1, {n}]')
        return cls.keyframes(motion, list(range(int(head))) + list(range(n - int(tail), n)))

    @classmethod
    def parts(cls, motion, names, dataset, frames=None):
        """the channels of the body parts ``names`` (``synthetic.part_layout(dataset)``) are given, on ``frames`` (None: all)"""
        from .synthetic import part_layout
        known, channels, _ = part_layout(dataset)
        names = [names] if isinstance(names, str) else list(names)
        bad = [n for n in names if n not in known]
        if bad or not names:
            raise ValueError(f'parts {bad or names!r}: the parts of {dataset!r} are {known}')
        C = 1 + max(c for n in known for c in channels[n])
        if motion.dim() != 2 or motion.shape[1] < C:
            raise ValueError(f'motion has {tuple(motion.shape)[-1]} channels, the {dataset!r} layout reaches channel {C - 1}')
        rows = list(range(motion.shape[0])) if frames is None else cls._frame_list(frames, motion.shape[0])
        keep = torch.zeros(motion.shape, dtype=torch.bool)
        cols = sorted({c for n in names for c in channels[n]})
        keep[torch.tensor(rows)[:, None], torch.tensor(cols)[None, :]] = True
        return cls(motion, keep)

    def tables(self, frames, pre_process=None, first_frame=0):
        """-> (gt [frames, C] float32 in model space, keep [frames, C] uint8) on the CPU: frames past the edit's are free.
        ``first_frame``: the window form -- the slice of the edit that starts at that frame of the request, for
        the row that shows frames ``[first_frame, first_frame + frames)``; two windows that share a frame get equal entries for it."""
        if isinstance(first_frame, bool) or int(first_frame) != first_frame or int(first_frame) < 0:
            raise ValueError(f'first_frame must be a non-negative integer, got {first_frame!r}')
        first = int(first_frame)
        motion = self.motion.detach().float().cpu()
        keep = self.keep.cpu()
        motion = torch.where(keep, motion, torch.zeros_like(motion))          # (what is not given never reaches the device)
        if pre_process is not None:
            motion = pre_process(motion)
        gt = torch.zeros(frames, self.feats)
        kp = torch.zeros(frames, self.feats, dtype=torch.uint8)
        n = max(0, min(self.frames - first, frames))
        gt[:n] = motion[first:first + n]
        kp[:n] = keep[first:first + n].to(torch.uint8)
        return gt, kp


class Request:
    """One generation request: the condition (``xf_out`` [Nt, Dt], the text encoder's output -- or ``text``, encoded on submit),
    ``length`` frames (1 .. the batcher's ``frames``; longer in a ``ContinuousBatcher`` with ``overlap=``), ``seed`` in [0, 2^64) and
    optionally a control condition ``c`` [Tc, Fc].
    ``guidance_scale``: the request's own classifier-free guidance scale (``ContinuousBatcher``; None: the model's).
    ``edit``: an ``Edit`` -- the frames / channels of the result that are given (at most ``length`` frames)."""

    def __init__(self, length, seed, xf_out=None, text=None, c=None, guidance_scale=None, edit=None):
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
        if guidance_scale is not None and (isinstance(guidance_scale, bool) or float(guidance_scale) != float(guidance_scale)):
            raise ValueError(f'guidance_scale must be a number or None, got {guidance_scale!r}')
        if edit is not None:
            if not isinstance(edit, Edit):
                raise ValueError(f'edit must be an Edit, got {type(edit).__name__}')
            if edit.frames > int(length):
                raise ValueError(f'the edit holds {edit.frames} frames, the request {int(length)}')
        self.length, self.seed, self.xf_out, self.text, self.c = int(length), int(seed), xf_out, text, c
        self.edit = edit
        self.guidance_scale = None if guidance_scale is None else float(guidance_scale)


def _check_edit(model, request):
    """an edit's channel count against the model's (host tests run without a model)"""
    if request.edit is not None and model is not None:
        C = model.model.dims['input_feats']
        if request.edit.feats != C:
            raise ValueError(f'the edit has {request.edit.feats} channels, the model {C}')


def plan_windows(length, frames, overlap):
    """The windows of a request of ``length`` frames in a batcher of ``frames`` with ``overlap`` shared frames:
    ``[(first_frame, window length)]``.  Up to ``frames`` it is one window; beyond that ``W = ceil((length - overlap) / stride)``
    windows, ``stride = frames - overlap``, window j at ``j * stride`` with ``min(frames, length - j * stride)`` frames -- the last one
    may be ragged, its length in ``(overlap, frames]``."""
    F, T, ov = int(length), int(frames), int(overlap)
    if not 0 < 2 * ov <= T:
        raise ValueError(f'overlap={overlap!r}: an integer with 0 < 2 overlap <= frames ({T})')
    if F <= T:
        return [(0, F)]
    stride = T - ov
    W = -((ov - F) // stride)                     # ceil((F - ov) / stride)
    return [(j * stride, min(T, F - j * stride)) for j in range(W)]


class _Batcher:
    """what the two batchers share: the sampler settings, the respaced schedule and the queue"""

    def __init__(self, model, batch, frames, sampler, steps, capacity_factor, eta, order):
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
        self._pending = []             # (handle, Request with xf_out set)
        self._next = 0

    def _respaced(self):
        """the model's test schedule, respaced to ``steps``"""
        from .diffusion import build_diffusion
        cfg = dict(self.model.diffusion_test_cfg)
        if self.steps is not None:
            cfg['respace'] = str(self.steps) if self.sampler == 'ddpm' else f'ddim{self.steps}'
        return build_diffusion(cfg, opt=self.model.opt)

    def _is_long(self, request):
        return request.length > self.frames

    def _queue(self, request):
        """``request`` with its text encoded and every other field carried, into the queue; -> its handle"""
        _check_edit(self.model, request)
        if request.xf_out is None:
            # one prompt per encoder call: the condition of a request must not depend on what it is encoded beside
            xf = self.model.model.encode_text([request.text], None, None)[0]
            request = Request(request.length, request.seed, xf_out=xf, c=request.c, guidance_scale=request.guidance_scale, edit=request.edit)
        handle = self._next
        self._next += 1
        self._pending.append((handle, request))
        return handle


class RequestBatcher(_Batcher):
    """``submit()`` requests, ``run()`` them ``batch`` at a time through one (batch, frames) context.

    ``model``: a ``MotionDiffusion`` (its denoiser and its test schedule's configuration are used).  ``sampler`` in ``SAMPLERS``;
    ``steps``: respace the schedule to that many steps (None: the configured schedule).  ``runner`` replaces the model call (tests):
    ``runner(xf_out [B,Nt,Dt], lengths [B], seeds [B], c [B,Tc,Fc] or None) -> [B, frames, C]``; a batch that holds a request with an
    ``Edit`` calls it with ``edits=[Edit or None] * B`` too.

    A batch with an edit runs through ``mc_sample_rows`` with uniform tables (every row at walk position k in tick k, draw 1 + k): the
    path ``ContinuousBatcher`` takes, so a request gets the same bits from both.  Batches without one take the fused loop as before."""

    def __init__(self, model, batch, frames, sampler='ddim', steps=None, capacity_factor=0, eta=0.0, order=2, runner=None):
        super().__init__(model, batch, frames, sampler, steps, capacity_factor, eta, order)
        self.runner = runner if runner is not None else self._run_model
        self._diffusion = None

    # ---- queue ------------------------------------------------------------------------------------
    def submit(self, request):
        """Queue ``request``; -> its handle (the key of ``run()``'s result)."""
        if not isinstance(request, Request):
            raise ValueError('submit() takes a Request')
        if self._is_long(request):
            raise ValueError(f'request of {request.length} frames in a batcher of {self.frames}')
        return self._queue(request)

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
            edits = [reqs[h].edit if h is not None else None for h in rows]
            pred = self.runner(xf, lengths, seeds, c, edits=edits) if any(e is not None for e in edits) else self.runner(xf, lengths, seeds, c)
            for b, h in enumerate(rows):
                if h is not None:
                    results[h] = pred[b, :reqs[h].length]
        self._pending = []
        return results

    # ---- the model call ---------------------------------------------------------------------------
    def _schedule(self):
        if self._diffusion is None:
            self._diffusion = self._respaced()
        return self._diffusion

    def _run_model(self, xf_out, lengths, seeds, c, edits=None):
        if edits is not None and any(e is not None for e in edits):
            return self._run_rows(xf_out, lengths, seeds, c, edits)
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

    def _run_rows(self, xf_out, lengths, seeds, c, edits):
        """a batch with an edit: ``ContinuousBatcher``'s model call with every row fresh and the whole walk in one call"""
        rr = _RowsRunner(self)
        B = self.batch
        rr.condition(xf_out, lengths, seeds, [True] * B, c, edits=edits)
        try:
            rr.advance([[k] * B for k in range(rr.steps)], [None] * B)
            return rr.result()
        finally:
            rr.clear_edits()           # (the context is the model's cached one: the fused loop refuses it while a table is set)


class ContinuousBatcher(_Batcher):
    """Requests join a running batch at any step and leave when their own walk ends.

    Every row of the (batch, frames) context walks the same schedule, each from its own start: a row admitted at tick t sits at walk
    position 0 while its neighbours are anywhere else, and takes its own guidance scale (``Request.guidance_scale``).  The result of a
    request is the function ``RequestBatcher`` states (capacity factor 0), bit for bit the bits ``RequestBatcher`` gives it.

    Same constructor vocabulary as ``RequestBatcher``.  ``submit()`` -> handle; ``tick(n=1)`` does one round; ``run()`` ticks until the
    queue and the rows are empty; ``poll()`` -> the finished ``{handle: pred_motion[:length]}`` since the last poll.

    One ``tick(n)`` round:
      1. pending requests are admitted into open rows (lowest row first, submission order).  x_T of such a row is draw 0 of its seed;
         the condition of the batch is replaced with only the new rows marked fresh (``set_condition_rows``).
      2. every row advances by the same number of steps in ONE ``mc_sample_rows`` call: ``n``, clipped to the smallest remaining walk of
         an occupied row, so that no row passes its end (its result would be overwritten) and a waiting request gets the row at once.
         The walk's k-th step of a row takes draw 1 + k of its seed.
      3. rows that reached the end of their walk are retired.
    Open rows run the fixed dummy request at walk position 0 (a retired row keeps its old condition until the next admission replaces
    it), so the call shape never changes.  Requests with and without a control condition never share a call: a request whose control
    shape differs from the running rows' waits until they drained, and control requests are admitted into an empty batch only (setting
    the control condition clears every row's multistep history).

    The context is the model's cached (batch, frames) one: do not interleave another sampler on the same model and shape with a
    running batcher.

    Edits (``Request.edit``): the kept region of an admitted row is uploaded with its admission; rows without an edit, dummy rows and
    (at the next admission) stale retired rows get an empty one, and the table is cleared when the last running row with an edit
    retires.  A request without an edit keeps its bits whatever its batchmates carry.

    ``runner`` (host tests) replaces the model: an object with ``steps`` and
      ``condition(xf_out [B,Nt,Dt], lengths [B], seeds [B], fresh [B], c)``  -- rows with ``fresh[b]`` start at draw 0 of ``seeds[b]``;
                                   called with ``edits=[Edit or None] * B`` too (the rows as they stand; those with ``fresh[b]`` are to
                                   be uploaded) while a running row carries an edit or a table is set
      ``clear_edits()``                       -- no running row carries an edit any more (only ever called after such a ``condition``)
      ``advance(pos [n][B], scales [B])``     -- n steps, row b of step k at walk position ``pos[k][b]`` (schedule index steps-1-pos)
      ``result()`` -> [B, frames, C]          -- the rows as they stand, post-processed.

    Long requests (``overlap=``).  Without ``overlap`` a request longer than ``frames`` is a ``ValueError``, as
    ever.  With it (``0 < 2 overlap <= frames``; ``seam_weights``: the right window's share per shared frame, default
    ``(f + 1) / (overlap + 1)``) such a request is planned into ``W`` windows (``plan_windows``), takes the ``W`` lowest open rows --
    they need not be contiguous -- and walks as ONE request: its rows are admitted, advance and retire together, the shared frames of
    neighbouring windows are blended after every denoiser call (``set_seam_rows``), and its noise is one field over its global frames
    (x_T = draw 0, step k = draw 1 + k of its seed), so the result does not depend on the rows it lands in.  ``xf_out`` is repeated per
    window; a control condition ``c`` [length * r, Fc] is sliced per window by its ``r`` rows per frame.  The result is the stitched
    motion [length, C]: the first ``stride`` frames of every window but the last, then the last window's valid frames.
    Admission is then strict FIFO: the head of the queue waits until ``W`` rows are open (and, a control request, until the batch is
    empty) and nothing overtakes it -- no request starves, but a short request can wait behind a long one.  ``W > batch`` and an
    ``edit`` on a request longer than ``frames`` are ``ValueError`` at ``submit()``; a long request waits while a running row carries
    an edit and a request with an edit waits while a long request runs (the two tables exclude each other in the library).
    The runner sees two more calls, both only while long requests are involved: ``condition(..., first_frames=[...] * B)`` (the global
    frame of every row's frame 0; a fresh row's x_T is its part of draw 0 of the request's field) and, after every admission and every
    retirement of a long request, ``seams(right [B], first_frame [B])`` with the table as it now stands, or ``clear_seams()`` once no
    long request runs.

    Edits on long requests (``long_edits=True``, needs ``overlap=``).  ``submit()`` then takes an ``Edit`` on a
    request longer than ``frames`` (keyframes over the whole sequence, a given opening, given body parts), and neither kind of
    request waits for the other: the context holds both tables (``set_long_edits``).  Every window row is uploaded at admission with
    its slice of the request's edit (``Edit.tables(frames, pre_process, first_frame)``), so the two copies of a shared frame carry
    equal entries; the runner's ``condition`` then gets ``edits=`` and ``first_frames=`` in one call.  At the end of the walk the kept
    elements of the stitched result are the given ones.  With ``long_edits=False`` nothing of this changes anything."""

    def __init__(self, model, batch, frames, sampler='ddim', steps=None, capacity_factor=0, eta=0.0, order=2, runner=None, overlap=None,
                 seam_weights=None, long_edits=False):
        super().__init__(model, batch, frames, sampler, steps, capacity_factor, eta, order)
        if overlap is None:
            if seam_weights is not None:
                raise ValueError('seam_weights without overlap')
        else:
            if isinstance(overlap, bool) or int(overlap) != overlap or not 0 < 2 * int(overlap) <= self.frames:
                raise ValueError(f'overlap={overlap!r}: an integer with 0 < 2 overlap <= frames ({self.frames})')
            overlap = int(overlap)
            if seam_weights is not None:
                seam_weights = [float(v) for v in seam_weights]
                if len(seam_weights) != overlap or not all(0.0 <= v <= 1.0 for v in seam_weights):
                    raise ValueError(f'seam_weights: {overlap} numbers in [0, 1]')
        if long_edits and overlap is None:
            raise ValueError('long_edits without overlap: edits on long requests need the windows of overlap=')
        self.overlap, self.seam_weights, self.long_edits = overlap, seam_weights, bool(long_edits)
        self._seams_on = False                        # the runner holds a row seam table
        self.runner = runner if runner is not None else _RowsRunner(self)
        self.walk = int(self.runner.steps)            # steps of one request's walk
        if self.walk < 1:
            raise ValueError(f'the schedule has {self.walk} steps')
        self._rows = [None] * self.batch              # per row: None (open) or [handle, Request, walk position, window of the request]
        self._done = {}
        self._conditioned = False
        self._edit_on = False                         # the runner holds an edit table
        self._stale = [False] * self.batch            # rows retired since the last condition call (still holding their old condition)
        self.ticks = 0                                # steps the batch has taken
        self.submitted_at, self.finished_at = {}, {}  # handle -> self.ticks at submit() / at retirement

    # ---- queue ------------------------------------------------------------------------------------
    def submit(self, request):
        """Queue ``request``; -> its handle (the key of ``poll()``'s result)."""
        if not isinstance(request, Request):
            raise ValueError('submit() takes a Request')
        if self._is_long(request):
            if self.overlap is None:
                raise ValueError(f'request of {request.length} frames in a batcher of {self.frames}')
            if request.edit is not None and not self.long_edits:
                raise ValueError(f'an edit on a request of {request.length} frames, longer than the batcher\'s {self.frames}: edits on long requests are not served')
            W = len(plan_windows(request.length, self.frames, self.overlap))
            if W > self.batch:
                raise ValueError(f'request of {request.length} frames is {W} windows of {self.frames} (overlap {self.overlap}) in a batcher of {self.batch} rows')
            if request.c is not None and request.c.shape[0] % request.length:
                raise ValueError(f'the control condition has {request.c.shape[0]} rows for {request.length} frames: a whole number of rows per frame')
        handle = self._queue(request)
        self.submitted_at[handle] = self.ticks
        return handle

    @property
    def occupied(self):
        """handles of the running rows (None: an open row)"""
        return [None if r is None else r[0] for r in self._rows]

    def _group(self, r):
        """the shape of one row's control condition (None: no control); the windows of a long request hold ``frames`` frames of it"""
        if r.c is None:
            return None
        if self._is_long(r):
            return (self.frames * (r.c.shape[0] // r.length), int(r.c.shape[1]))
        return tuple(r.c.shape)

    def _windows(self, r):
        return plan_windows(r.length, self.frames, self.overlap) if self._is_long(r) else [(0, r.length)]

    def _admit_fifo(self, group):
        """``_admit`` with ``overlap`` set: strict FIFO, the head of the queue takes the lowest open rows or everyone waits"""
        fresh = []
        while self._pending:
            handle, r = self._pending[0]
            if self._group(r) != group:
                break
            long_runs = any(q is not None and self._is_long(q[1]) for q in self._rows)
            edit_runs = self._edit_on or any(q is not None and q[1].edit is not None for q in self._rows)
            if not self.long_edits and ((self._is_long(r) and edit_runs) or (r.edit is not None and long_runs)):
                break                                 # the edit table and the row seam table exclude each other (without long_edits)
            wins = self._windows(r)
            open_rows = [b for b in range(self.batch) if self._rows[b] is None]
            if len(open_rows) < len(wins):
                break
            self._pending.pop(0)
            for j, b in enumerate(open_rows[:len(wins)]):
                self._rows[b] = [handle, r, 0, j]
                fresh.append(b)
        return fresh

    def _admit(self):
        """step 1 of a round; -> the rows that took a new request"""
        running = [r for r in self._rows if r is not None]
        fresh = []
        if not self._pending:
            return fresh
        group = self._group(running[0][1]) if running else self._group(self._pending[0][1])
        if group is not None and running:
            return fresh                              # control requests start in an empty batch only
        if self.overlap is not None:
            return self._admit_fifo(group)
        for b in range(self.batch):
            if self._rows[b] is not None:
                continue
            k = next((k for k, (_, r) in enumerate(self._pending) if self._group(r) == group), None)
            if k is None:
                break
            handle, r = self._pending.pop(k)
            self._rows[b] = [handle, r, 0, 0]
            fresh.append(b)
        return fresh

    def _condition(self, fresh):
        live = [r[1] for r in self._rows if r is not None]
        first = live[0]
        flags = [b in fresh for b in range(self.batch)]
        if not self._conditioned or first.c is not None:      # the first call, or a control group (an empty batch): the open rows' dummy starts too
            flags = [True] * self.batch
        else:                                         # a retired row that stays open takes the dummy now
            flags = [f or (self._rows[b] is None and self._stale[b]) for b, f in enumerate(flags)]
        xf = torch.stack([r[1].xf_out if r is not None else torch.zeros_like(first.xf_out) for r in self._rows])
        wins = [self._windows(r[1])[r[3]] if r is not None else (0, self.frames) for r in self._rows]      # (first frame, frames) per row
        lengths = [n for _, n in wins]
        seeds = [r[1].seed if r is not None else DUMMY_SEED for r in self._rows]
        c = None
        if first.c is not None:
            c = torch.stack([self._row_control(r, wins[b], first) for b, r in enumerate(self._rows)])
        edits = [r[1].edit if r is not None else None for r in self._rows]
        more = {}                                     # the keywords a runner sees only while edits / long requests are involved
        if self._edit_on or any(e is not None for e in edits):
            more['edits'] = edits
        if any(r is not None and self._is_long(r[1]) for r in self._rows):
            more['first_frames'] = [f for f, _ in wins]   # (long_edits: every row's slice of its request's edit starts at its first frame)
        self.runner.condition(xf, lengths, seeds, flags, c, **more)
        if 'edits' in more:
            self._edit_on = True
            self._settle_edits()
        self._conditioned = True
        self._stale = [False] * self.batch
        if any(self._rows[b] is not None and self._is_long(self._rows[b][1]) for b in fresh):
            self._send_seams()

    def _row_control(self, r, win, first):
        """the control condition of one row: the request's, the rows of a long request's window (zero rows behind a ragged last
        window), or zeros for an open row"""
        shape = self._group(first)
        if r is None:
            return torch.zeros(shape, dtype=first.c.dtype)
        c = r[1].c
        if not self._is_long(r[1]):
            return c
        per = c.shape[0] // r[1].length
        out = torch.zeros(shape, dtype=c.dtype)
        out[:win[1] * per] = c[win[0] * per:(win[0] + win[1]) * per]
        return out

    def _send_seams(self):
        """the row seam table as the rows now stand (after an admission or a retirement of a long request), or none"""
        by_handle = {}
        for b, r in enumerate(self._rows):
            if r is not None and self._is_long(r[1]):
                by_handle.setdefault(r[0], {})[r[3]] = b
        if not by_handle:
            if self._seams_on:
                self.runner.clear_seams()
                self._seams_on = False
            return
        right, first = [-1] * self.batch, [0] * self.batch
        stride = self.frames - self.overlap
        for rows in by_handle.values():
            for j, b in rows.items():
                right[b] = rows.get(j + 1, -1)
                first[b] = j * stride
        self.runner.seams(right, first)
        self._seams_on = True

    def _settle_edits(self):
        """clear the runner's table once no running row carries an edit"""
        if self._edit_on and not any(r is not None and r[1].edit is not None for r in self._rows):
            self.runner.clear_edits()
            self._edit_on = False

    def tick(self, n=1):
        """One round (class docstring); -> the steps the batch advanced by (0: nothing to run)."""
        if isinstance(n, bool) or int(n) != n or int(n) < 1:
            raise ValueError(f'tick(n): a positive number of steps, got {n!r}')
        fresh = self._admit()
        if fresh:
            self._condition(fresh)
        live = [r for r in self._rows if r is not None]
        if not live:
            return 0
        n = min(int(n), min(self.walk - r[2] for r in live))
        pos = [[(r[2] + k) if r is not None else 0 for r in self._rows] for k in range(n)]
        scales = [r[1].guidance_scale if r is not None else None for r in self._rows]
        self.runner.advance(pos, scales)
        self.ticks += n
        out = None
        parts = {}                                    # handle of a retiring long request -> (its length, {window: its frames})
        for b, r in enumerate(self._rows):
            if r is None:
                continue
            r[2] += n
            if r[2] == self.walk:
                if out is None:
                    out = self.runner.result()
                if self._is_long(r[1]):               # (the rows of a request were admitted together: they all retire in this round)
                    parts.setdefault(r[0], (r[1].length, {}))[1][r[3]] = out[b]
                else:
                    self._done[r[0]] = out[b, :r[1].length].clone()
                self.finished_at[r[0]] = self.ticks
                self._rows[b] = None
                self._stale[b] = True
        for handle, (length, wins) in parts.items():
            self._done[handle] = self._stitch([wins[j] for j in range(len(wins))], length)
        if parts:
            self._send_seams()
        self._settle_edits()
        return n

    def _stitch(self, wins, length):
        """the windows of one request [frames, C] each, in order -> [length, C]: the first ``stride`` frames of every window but the
        last, then the last window's valid frames"""
        stride = self.frames - self.overlap
        return torch.cat([w[:stride] for w in wins[:-1]] + [wins[-1]])[:length].clone()

    def run(self):
        """Tick until the queue and the rows are empty; -> ``poll()``."""
        while self._pending or any(r is not None for r in self._rows):
            if self.tick(self.walk) == 0:
                raise RuntimeError('pending requests but nothing to run')      # (cannot happen: an empty batch admits the head of the queue)
        return self.poll()

    def poll(self):
        """-> ``{handle: pred_motion[:length]}`` of the requests finished since the last poll"""
        out, self._done = self._done, {}
        return out


class _RowsRunner:
    """the model behind ``ContinuousBatcher``: the (batch, frames) context of the model, ``x`` [B, frames, C] in place"""

    def __init__(self, owner):
        self.o = owner
        self.diffusion = owner._respaced()
        self.steps = self.diffusion.num_timesteps
        self.ctx, self.x, self.group = None, None, ()
        self._coefs = {}                              # scale -> the StepCoefs of a whole walk, by walk position

    def condition(self, xf_out, lengths, seeds, fresh, c, edits=None, first_frames=None):
        from . import lib as _lib
        from .engine import _ptr, _stream
        o, net = self.o, self.o.model.model
        dev = torch.device('cuda', torch.cuda.current_device())
        B, T, C = o.batch, o.frames, net.dims['input_feats']
        mask = torch.zeros(B, T, device=dev)
        for b, n in enumerate(lengths):
            mask[b, :n] = 1
        group = None if c is None else tuple(c.shape)
        # The control features reach the context through sampling_context alone, so every admission of a control group goes through it
        # (such a group starts in an empty batch: every row is fresh, the history of no running row is lost); so does a change of group.
        if self.ctx is None or c is not None or group != self.group:
            kw = dict(xf_out=xf_out.to(dev), motion_mask=mask, c=c, capacity_factor=o.capacity_factor)
            self.ctx = net.sampling_context(B, T, self.diffusion.timestep_map, kw, dev)
            self.group = group
            if self.ctx.long_edits != bool(getattr(o, 'long_edits', False)):      # (the context is the model's cached one)
                self.ctx.set_long_edits(not self.ctx.long_edits)
            if self.x is None:
                self.x = torch.zeros(B, T, C, device=dev)
        else:
            self.ctx.set_condition_rows(xf_out.to(dev), mask, fresh)
        if edits is not None:
            self._upload_edits(edits, fresh, dev, first_frames)
        self.ctx.set_row_seeds(seeds)
        # x_T of a fresh row: its frames of draw 0 of its seed's field (a short request, or window 0: elements [0, T C)).  The field is
        # a function of the seed alone, so it is drawn once per seed, as far as the last fresh window reaches, and gathered
        first = [0] * B if first_frames is None else [int(v) for v in first_frames]
        reach = {}
        for b, f in enumerate(fresh):
            if f:
                reach[seeds[b]] = max(reach.get(seeds[b], 0), first[b] + T)
        for seed, frames in reach.items():
            z = torch.empty(frames, C, device=dev)
            _lib.check(self.ctx.lib.mc_op_philox_normal(_ptr(z), None, z.numel(), int(seed) & (2 ** 64 - 1), 0, _stream()), 'mc_op_philox_normal')
            for b, f in enumerate(fresh):
                if f and seeds[b] == seed:
                    self.x[b] = z[first[b]:first[b] + T]

    def seams(self, right, first_frame):
        self.ctx.set_seam_rows(right, first_frame, self.o.overlap, self.o.seam_weights)

    def clear_seams(self):
        if self.ctx is not None:
            self.ctx.clear_seam_rows()

    def _upload_edits(self, edits, fresh, dev, first_frames=None):
        """the tables of the rows with ``fresh[b]``: the row's edit in model space (the window of a long request: the slice that starts
        at its first frame), or nothing kept.  Into a context that holds no table
        (the first edit, or the first after a clear) EVERY row is uploaded, each with its own edit or nothing kept: whatever
        an earlier table left on a row that now runs a request without an edit must not come back with the flag."""
        o, net = self.o, self.o.model.model
        B, T, C = o.batch, o.frames, net.dims['input_feats']
        every = not getattr(self.ctx, 'edit_rows', False)
        gt = torch.zeros(B, T, C)
        keep = torch.zeros(B, T, C, dtype=torch.uint8)
        for b, e in enumerate(edits):
            if e is not None and (fresh[b] or every):
                gt[b], keep[b] = e.tables(T, net.pre_process, 0 if first_frames is None else int(first_frames[b]))
        self.ctx.set_edit_rows(gt.to(dev), keep.to(dev), None if every else fresh)

    def clear_edits(self):
        if self.ctx is not None:
            self.ctx.clear_edit_rows()

    def _walk_coefs(self, scale):
        o, d = self.o, self.diffusion
        scale = float(o.model.model.cfg_scale if scale is None else scale)
        if scale not in self._coefs:
            idx = list(range(self.steps))[::-1]
            if o.sampler == 'dpmpp':
                self._coefs[scale] = d.multistep_coefs(idx, scale, o.order)
            else:
                self._coefs[scale] = [d.step_coefs(i, o.sampler, scale, o.eta if o.sampler == 'ddim' else 0.0) for i in idx]
        return self._coefs[scale]

    def advance(self, pos, scales):
        walks = [self._walk_coefs(s) for s in scales]
        idx = [[self.steps - 1 - p for p in row] for row in pos]
        coefs = [[walks[b][p] for b, p in enumerate(row)] for row in pos]
        draws = [[1 + p for p in row] for row in pos]
        self.ctx.sample_rows(self.x, idx, coefs, draws=draws)

    def result(self):
        return self.o.model.model.post_process(self.x.clone())

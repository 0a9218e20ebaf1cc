"""Thin Python owner of the native handles: ``NativeModel`` (weights in HBM) and ``NativeContext``
(workspace + schedule tables + condition K/V for one (batch, frames) shape).

PyTorch is used only for device memory and the stream handle; every compute step is a call into
libmotioncraft_amd.so.
"""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _ptr, stream as _stream
from .weights import control_info, pack_state_dict

PRECISIONS = _lib.named('MC_PREC_')               # 'f32', 'f16', 'f16x3' -> mc_ctx_set_precision's code
TIE_POLICIES = _lib.named('MC_TIE_')              # 'stable', 'reverse' -> mc_ctx_set_tie_policy's code


def _dev_f32(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f'{name} must be a contiguous float32 tensor in device (HBM) memory')
    return t


def check_seeds(seeds, rows):
    """``seeds`` as a list of ``rows`` ints in [0, 2^64) (one Philox key per batch row), or ValueError"""
    try:
        out = [int(s) for s in seeds]
    except (TypeError, ValueError):
        raise ValueError(f'seeds must be a sequence of {rows} ints, got {seeds!r}') from None
    if len(out) != rows:
        raise ValueError(f'{len(out)} seeds for a batch of {rows} rows')
    if any(not 0 <= s < 2 ** 64 for s in out):
        raise ValueError('every seed must lie in [0, 2^64)')
    return out


class NativeModel(_lib.NativeObject):
    def __init__(self, dims, state_dict, cfg_scale=6.5, capacity_factor=1.5, dyn_heads=8, device=None,
                 condition_cfg=True):
        lib = _lib.load(require_gpu=True)
        if device is not None:
            torch.cuda.set_device(device)
            _lib.check(lib.mc_set_device(torch.cuda.current_device()), 'mc_set_device')
        self.dims = dict(dims)
        self.copy_blocks_num, self.control_cond_feats = control_info(state_dict)
        cfg = _lib.ModelConfig(
            input_feats=dims['input_feats'], max_seq_len=dims['max_seq_len'], latent_dim=dims['L'],
            num_parts=dims['H'], num_layers=dims['NL'], ffn_dim=dims['F'], time_embed_dim=dims['Te'],
            text_latent_dim=dims['Dt'], max_text_len=dims['Nt'], num_experts=dims['E'], topk=dims.get('topk', 2),
            dyn_heads=dyn_heads, capacity_factor=capacity_factor, cfg_scale=cfg_scale,
            num_ctrl_layers=self.copy_blocks_num, ctrl_cond_feats=self.control_cond_feats,
            ctrl_condition_cfg=int(bool(condition_cfg)))
        self.cfg, self.cfg_scale = cfg, float(cfg_scale)
        super().__init__('model', ctypes.byref(cfg))
        self.upload(pack_state_dict(state_dict, dims).items())
        self.finalize()

    def context(self, batch, frames, max_steps=1000):
        return NativeContext(self, batch, frames, max_steps)


class NativeContext:
    def __init__(self, model, batch, frames, max_steps):
        self.model, self.lib = model, model.lib
        self.B, self.T, self.C = int(batch), int(frames), model.dims['input_feats']
        h = ctypes.c_void_p()
        _lib.check(self.lib.mc_ctx_create(model.handle, self.B, self.T, int(max_steps), ctypes.byref(h)), 'mc_ctx_create')
        self.handle = h
        self.timesteps = None
        self._keep = []
        self._graph_state = None
        self.seams = None              # dict(first_frame, overlap) while a seam table is set (set_seams)
        self.row_seeds = None          # the rows' Philox keys while a seed table is set (set_row_seeds)
        self.edit_rows = False         # an edit table is set (set_edit_rows); read by serve: the first upload after a clear sends every row
        self.seam_rows = None          # dict(right, first_frame, overlap) while a row seam table is set (set_seam_rows)
        self.long_edits = False        # the two tables may be set side by side (set_long_edits)

    @property
    def workspace_bytes(self):
        return int(self.lib.mc_ctx_workspace_bytes(self.handle))

    def check(self):
        """Synchronise the current stream and raise if a kernel of this context flagged an error (the cooperative routing
        kernel's bounded grid barrier); the sampler loops call it once after the last step."""
        _lib.check(self.lib.mc_ctx_check(self.handle, _stream()), 'mc_ctx_check')

    def profile(self, on=True):
        """Bracket every FiLM out_layers GEMM launch with HIP events on its launch stream (bench.py's dominant-kernel figure)."""
        _lib.check(self.lib.mc_ctx_profile(self.handle, int(bool(on))), 'mc_ctx_profile')

    def profile_read(self, rows=0):
        """(average duration in us, launches, algorithmic GFLOP per launch) of the bracketed launches (of `rows` rows if given)."""
        us, n, gf = ctypes.c_double(), ctypes.c_int32(), ctypes.c_double()
        _lib.check(self.lib.mc_ctx_profile_read(self.handle, int(rows), ctypes.byref(us), ctypes.byref(n), ctypes.byref(gf)),
                   'mc_ctx_profile_read')
        return us.value, n.value, gf.value

    @property
    def effective_precision(self):
        """'f32' / 'f16' / 'f16x3' the per-step kernels really run in (a reduced-precision mode falls back to the fp32 small-batch
        kernels up to 512 residual rows, i.e. B = 1 at 196 frames)."""
        code = int(self.lib.mc_ctx_effective_precision(self.handle))
        return next(name for name, c in PRECISIONS.items() if c == code)

    @property
    def uses_coop_routing(self):
        return bool(self.lib.mc_ctx_uses_coop_routing(self.handle))

    def enable_capture(self):
        """Keep every layer's routing decisions of the last denoise call (tests)."""
        self._drop_graph()
        _lib.check(self.lib.mc_ctx_enable_capture(self.handle), 'mc_ctx_enable_capture')

    def _drop_graph(self):
        # a captured graph bakes in the kernel selection and the condition buffers of the moment of capture
        if getattr(self, '_graph_state', None) is not None:
            self.graph_release()

    def set_precision(self, precision):
        """'f32' (default, exact fp32 MFMA), 'f16' (fp16 operands, fp32 accumulate) or 'f16x3' (fp16 hi/lo split, three
        products: fp32-class) for the per-step GEMM-shaped kernels; gate / routing / normalisations stay fp32."""
        code = PRECISIONS[precision]
        self._drop_graph()
        _lib.check(self.lib.mc_ctx_set_precision(self.handle, code), 'mc_ctx_set_precision')
        self.precision = precision

    def set_option(self, key, value):
        """Kernel-selection switch of THIS context (mc_ctx_set_option); the MC_* variable of a key only seeds the default of
        contexts created afterwards.  Key (variable, default):
        'chain' (MC_CHAIN, 762806311; retired bits 3, 4, 6 - 14, 19, 23, 25, 28 and bits >= 30 raise), 'small_gemm_rows' (MC_SMALL_GEMM_ROWS, 5600),
        'split_rows_expert' (MC_SPLIT_ROWS_EXPERT, 2048), 'split_rows_sffn' (MC_SPLIT_ROWS_SFFN, 8192),
        'temporal_split' (MC_TEMPORAL_SPLIT, 96), 'big_tokens' (MC_BIG_TOKENS, 65536), 'rowchain_split' (MC_ROWCHAIN_SPLIT, 20480),
        'gemm_tune' (MC_GEMM_TUNE, 1841; bits 0, 4, 5, 6, 8, 9, 10), 'small_tile_n' (MC_SMALL_TILE_N, 0; 0, 48, 64 or 96),
        'gemm_wp_grid' (MC_GEMM_WP_GRID, 512; <= 0 one workgroup per tile), 'half_min_rows' (MC_HALF_MIN_ROWS, 512),
        'gate_small' (MC_GATE_SMALL, 12000), 'split_expert' (MC_SPLIT_EXPERT, 0), 'split_sffn' (MC_SPLIT_SFFN, 0),
        'route_reg' (MC_ROUTE_REG, 1), 'route_coop' (MC_ROUTE_COOP, 1),
        'route_small' (MC_ROUTE_SMALL_CTX, else MC_ROUTE_SMALL, 20480; 0 .. 131072), 'route_per' (no variable, 0; 0, 10 or 16),
        'route_early' (MC_ROUTE_EARLY, 1 -- 0 for an L = 64 model; 0 or 1),
        'dbg_delay_us' (no variable, 0; -100000 .. 100000).  An unknown key or an invalid value raises."""
        self._drop_graph()
        _lib.check(self.lib.mc_ctx_set_option(self.handle, str(key).encode(), int(value)), 'mc_ctx_set_option')

    def set_tie_policy(self, policy):
        """'stable' (default) or 'reverse': order of equal-importance tokens at a capacity cut (tutel boundary, a16).
        Call before set_condition."""
        code = TIE_POLICIES[policy]
        self._drop_graph()             # a captured graph has the tie key and the twin-mode launch sequence baked in
        self._keep = []                # the library forgets the condition: set_condition must follow
        _lib.check(self.lib.mc_ctx_set_tie_policy(self.handle, code), 'mc_ctx_set_tie_policy')

    def routing(self, layer):
        """(expert ids [N,2] long, keep [N,2] bool) of `layer` from the last denoise call, on CPU."""
        idx = self.buffer('cap_idx', layer, dtype=torch.int32).view(-1, 2).cpu().long()
        keep = (self.buffer('cap_w', layer).view(-1, 2) != 0).cpu()
        return idx, keep

    def set_timesteps(self, t_orig):
        self._drop_graph()
        t = np.ascontiguousarray(np.asarray(t_orig, dtype=np.int32))
        _lib.check(self.lib.mc_ctx_set_timesteps(self.handle, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                 len(t), _stream()), 'mc_ctx_set_timesteps')
        self.timesteps = [int(v) for v in t]

    def set_condition(self, xf_out, motion_mask):
        xf = _dev_f32(xf_out, 'xf_out')
        mask = _dev_f32(motion_mask, 'motion_mask')
        d = self.model.dims
        if tuple(xf.shape) != (self.B, d['Nt'], d['Dt']):
            raise ValueError(f'xf_out shape {tuple(xf.shape)} != {(self.B, d["Nt"], d["Dt"])}')
        if mask.numel() != self.B * self.T:
            raise ValueError(f'motion_mask has {mask.numel()} elements, expected {self.B * self.T}')
        self._keep = [xf, mask]        # (the library copies the mask; a captured graph stays valid across conditions)
        _lib.check(self.lib.mc_ctx_set_condition(self.handle, _ptr(xf), _ptr(mask), _stream()), 'mc_ctx_set_condition')

    def set_control(self, c_feat):
        """c_feat [B, Tc, control_cond_feats] (output of the step-invariant condition pre-encoder) or None."""
        if (c_feat is None) != (not getattr(self, '_ctrl_on', False)):
            self._drop_graph()         # control branch on / off changes the captured launch sequence
        self._ctrl_on = c_feat is not None
        if c_feat is None:
            _lib.check(self.lib.mc_ctx_set_control(self.handle, None, 0, _stream()), 'mc_ctx_set_control')
            return
        c = _dev_f32(c_feat, 'c')
        if c.dim() != 3 or c.shape[0] != self.B or c.shape[2] != self.model.control_cond_feats:
            raise ValueError(f'c shape {tuple(c.shape)} != (B={self.B}, Tc, {self.model.control_cond_feats})')
        self._keep_c = c
        _lib.check(self.lib.mc_ctx_set_control(self.handle, _ptr(c), int(c.shape[1]), _stream()), 'mc_ctx_set_control')

    def denoise(self, x_t, step_index, out2=None, stop_after_layers=-1):
        x = _dev_f32(x_t, 'x_t')
        if tuple(x.shape) != (self.B, self.T, self.C):
            raise ValueError(f'x_t shape {tuple(x.shape)} != {(self.B, self.T, self.C)}')
        if out2 is None and stop_after_layers < 0:
            out2 = torch.empty(2 * self.B, self.T, self.C, device=x.device, dtype=torch.float32)
        _lib.check(self.lib.mc_denoise(self.handle, _ptr(x), int(step_index), _ptr(out2), int(stop_after_layers),
                                       _stream()), 'mc_denoise')
        return out2

    def sample_step(self, x_t, step_index, coefs, noise, x_prev=None, x0=None):
        """One step (mc_sample_step).  ``noise`` may be None for multistep coefficients (mode 2) only: that mode draws nothing and
        keeps the previous x0 in the context instead."""
        x = _dev_f32(x_t, 'x_t')
        n = _dev_f32(noise, 'noise') if noise is not None else None
        if x_prev is None:
            x_prev = torch.empty_like(x)
        _lib.check(self.lib.mc_sample_step(self.handle, _ptr(x), int(step_index), ctypes.byref(coefs), _ptr(n),
                                           _ptr(x_prev), _ptr(x0), _stream()), 'mc_sample_step')
        return x_prev

    def sample_loop(self, x, step_indices, coefs, noise=None, seed=0, draw0=0, x0=None):
        """The whole sampler loop in one library call (mc_sample_loop): ``x`` [B,T,C] is updated IN PLACE through the schedule
        indices ``step_indices`` with ``coefs[k]``; ``noise`` [len, B,T,C] = the per-step draws, or None: drawn on the device
        (Philox4x32-10 keyed by ``seed``, draw index ``draw0 + k``).  Asynchronous on the current stream."""
        x = _dev_f32(x, 'x')
        if tuple(x.shape) != (self.B, self.T, self.C):
            raise ValueError(f'x shape {tuple(x.shape)} != {(self.B, self.T, self.C)}')
        n = len(step_indices)
        if len(coefs) != n:
            raise ValueError('one StepCoefs per step index')
        if noise is not None:
            noise = _dev_f32(noise, 'noise')
            if tuple(noise.shape) != (n, self.B, self.T, self.C):
                raise ValueError(f'noise shape {tuple(noise.shape)} != {(n, self.B, self.T, self.C)}')
        idx = (ctypes.c_int32 * n)(*[int(i) for i in step_indices])
        arr = (_lib.StepCoefs * n)(*coefs)
        _lib.check(self.lib.mc_sample_loop(self.handle, _ptr(x), idx, arr, n, _ptr(noise), int(seed) & (2 ** 64 - 1),
                                           int(draw0) & (2 ** 64 - 1), _ptr(x0), _stream()), 'mc_sample_loop')
        return x

    # ---- per-row schedules ---------------------------------------------------
    def _row_table(self, rows, what, conv=int):
        rows = [[conv(v) for v in r] for r in rows]
        if any(len(r) != self.B for r in rows):
            raise ValueError(f'{what}: every tick has one entry per row ({self.B})')
        return rows

    def denoise_rows(self, x_t, step_index, out2=None):
        """``denoise`` with row b at schedule index ``step_index[b]`` (mc_denoise_rows): -> out2 [2B,T,C], both decoded halves."""
        x = _dev_f32(x_t, 'x_t')
        if tuple(x.shape) != (self.B, self.T, self.C):
            raise ValueError(f'x_t shape {tuple(x.shape)} != {(self.B, self.T, self.C)}')
        idx = self._row_table([step_index], 'step_index')[0]
        if out2 is None:
            out2 = torch.empty(2 * self.B, self.T, self.C, device=x.device, dtype=torch.float32)
        _lib.check(self.lib.mc_denoise_rows(self.handle, _ptr(x), (ctypes.c_int32 * self.B)(*idx), _ptr(out2), _stream()),
                   'mc_denoise_rows')
        return out2

    def sample_rows(self, x, step_index, coefs, draws=None, noise=None, x0=None):
        """Ticks back to back in one library call (mc_sample_rows): in tick k row b takes the step at schedule index
        ``step_index[k][b]`` under ``coefs[k][b]`` (its guidance weight included); ``x`` [B,T,C] is updated IN PLACE.  ``noise``
        [ticks,B,T,C], or None: drawn on the device from the rows' seed table, row b at draw number ``draws[k][b]``.  One sampler mode
        per call.  Asynchronous on the current stream."""
        x = _dev_f32(x, 'x')
        if tuple(x.shape) != (self.B, self.T, self.C):
            raise ValueError(f'x shape {tuple(x.shape)} != {(self.B, self.T, self.C)}')
        idx = self._row_table(step_index, 'step_index')
        n = len(idx)
        if len(coefs) != n or any(len(r) != self.B for r in coefs):
            raise ValueError('coefs: one StepCoefs per tick and row')
        if noise is not None:
            noise = _dev_f32(noise, 'noise')
            if tuple(noise.shape) != (n, self.B, self.T, self.C):
                raise ValueError(f'noise shape {tuple(noise.shape)} != {(n, self.B, self.T, self.C)}')
        darr = None
        if draws is not None:
            d = self._row_table(draws, 'draws', lambda v: int(v) & (2 ** 64 - 1))
            if len(d) != n:
                raise ValueError('draws: one row of draw numbers per tick')
            darr = (ctypes.c_uint64 * (n * self.B))(*[v for r in d for v in r])
        iarr = (ctypes.c_int32 * (n * self.B))(*[v for r in idx for v in r])
        carr = (_lib.StepCoefs * (n * self.B))(*[c for r in coefs for c in r])
        _lib.check(self.lib.mc_sample_rows(self.handle, _ptr(x), n, iarr, carr, darr, _ptr(noise), _ptr(x0), _stream()),
                   'mc_sample_rows')
        return x

    def set_condition_rows(self, xf_out, motion_mask, fresh):
        """``set_condition`` for a batch in which only the rows with ``fresh[b]`` true hold a new request (mc_ctx_set_condition_rows):
        the text K/V of the whole batch are recomputed, the multistep history of the other rows stays valid."""
        xf = _dev_f32(xf_out, 'xf_out')
        mask = _dev_f32(motion_mask, 'motion_mask')
        d = self.model.dims
        if tuple(xf.shape) != (self.B, d['Nt'], d['Dt']):
            raise ValueError(f'xf_out shape {tuple(xf.shape)} != {(self.B, d["Nt"], d["Dt"])}')
        if mask.numel() != self.B * self.T:
            raise ValueError(f'motion_mask has {mask.numel()} elements, expected {self.B * self.T}')
        fresh = [bool(f) for f in fresh]
        if len(fresh) != self.B:
            raise ValueError(f'fresh: one flag per row ({self.B}), got {len(fresh)}')
        self._keep = [xf, mask]
        _lib.check(self.lib.mc_ctx_set_condition_rows(self.handle, _ptr(xf), _ptr(mask), (ctypes.c_uint8 * self.B)(*fresh), _stream()),
                   'mc_ctx_set_condition_rows')

    def set_edit_rows(self, gt, keep, fresh=None):
        """The kept region of every request row (mc_ctx_set_edit_rows): ``gt`` [B,T,C] float32 and ``keep``
        [B,T,C] bool / uint8 (non-zero: the element is given), both in model space, contiguous on the device.  Rows with ``fresh[b]``
        true (None: every row) are copied into the context's tables; the others keep what they hold.  While a table is set,
        ``sample_rows`` takes x0 = gt on the kept elements (and, DDIM, re-noises them from the row's own seed); every entry without a
        rows form raises."""
        g = _dev_f32(gt, 'gt')
        shape = (self.B, self.T, self.C)
        if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'keep must be a bool or uint8 tensor, got {getattr(keep, "dtype", type(keep).__name__)}')
        if not keep.is_cuda or not keep.is_contiguous():
            raise ValueError('keep must be a contiguous device tensor')
        if tuple(g.shape) != shape or tuple(keep.shape) != shape:
            raise ValueError(f'gt / keep shape {tuple(g.shape)} / {tuple(keep.shape)} != {shape}')
        farr = None
        if fresh is not None:
            fresh = [bool(f) for f in fresh]
            if len(fresh) != self.B:
                raise ValueError(f'fresh: one flag per row ({self.B}), got {len(fresh)}')
            farr = (ctypes.c_uint8 * self.B)(*fresh)
        _lib.check(self.lib.mc_ctx_set_edit_rows(self.handle, _ptr(g), keep.data_ptr(), farr, _stream()), 'mc_ctx_set_edit_rows')
        self._keep_edit = (g, keep)    # (the copies are asynchronous on the current stream; a refused call keeps the previous sources)
        self.edit_rows = True

    def clear_edit_rows(self):
        _lib.check(self.lib.mc_ctx_set_edit_rows(self.handle, None, None, None, _stream()), 'mc_ctx_set_edit_rows')
        self._keep_edit = None
        self.edit_rows = False

    def set_seams(self, first_frame, overlap, weights=None):
        """Couple the B rows of this context as windows of a long sequence (mc_ctx_set_seams): ``first_frame[b]`` = the global frame
        index of row b's frame 0; rows whose first frames differ by ``T - overlap`` are neighbours and share ``overlap`` frames, every
        other pair of consecutive rows must be disjoint.  While the table is set, ``sample_step`` / ``sample_loop`` blend the two x0
        predictions of a shared frame (``weights[f]`` = the right window's share, default ``(f + 1) / (overlap + 1)``) and keep the
        shared frames of x bit-equal in both rows -- given an x_T that is equal there, which is the caller's part.  The plan is
        checked here (``longform.check_seams``) before the library sees it; ``overlap=0`` clears the table."""
        from .longform import check_seams
        if int(overlap) == 0:
            return self.clear_seams()
        ff, w = check_seams(first_frame, self.T, overlap, weights, rows=self.B)
        self._drop_graph()             # a captured graph replays the uncoupled update
        arr = (ctypes.c_int32 * self.B)(*ff)
        warr = (ctypes.c_float * len(w))(*w) if w is not None else None
        _lib.check(self.lib.mc_ctx_set_seams(self.handle, int(overlap), arr, warr, _stream()), 'mc_ctx_set_seams')
        self.seams = dict(first_frame=ff, overlap=int(overlap))

    def clear_seams(self):
        _lib.check(self.lib.mc_ctx_set_seams(self.handle, 0, None, None, _stream()), 'mc_ctx_set_seams')
        self.seams = None

    def set_seam_rows(self, right, first_frame, overlap, weights=None):
        """Couple request rows of ``sample_rows`` as the windows of long requests (mc_ctx_set_seam_rows): row b
        shows frames ``first_frame[b] ..`` of its request and ``right[b]`` is the row that holds the request's next window (any row),
        or -1.  While the table is set, ``sample_rows`` blends the two x0 predictions of a shared frame (``weights[f]`` = the right
        window's share, default ``(f + 1) / (overlap + 1)``), keeps the shared frames of x bit-equal in both rows and, without
        ``noise``, draws every row at its request-global counter.  The rows of a seam must walk together (same step, coefficients,
        draw number and seed).  The library checks the table; a refused call leaves the previous one set.  ``overlap=0`` clears it."""
        if int(overlap) == 0:
            return self.clear_seam_rows()
        right, ff = [int(v) for v in right], [int(v) for v in first_frame]
        if len(right) != self.B or len(ff) != self.B:
            raise ValueError(f'right / first_frame: one entry per row ({self.B}), got {len(right)} / {len(ff)}')
        warr = None
        if weights is not None:
            w = [float(v) for v in weights]
            if len(w) != int(overlap):
                raise ValueError(f'weights: one per shared frame ({int(overlap)}), got {len(w)}')
            warr = (ctypes.c_float * len(w))(*w)
        _lib.check(self.lib.mc_ctx_set_seam_rows(self.handle, int(overlap), (ctypes.c_int32 * self.B)(*right), (ctypes.c_int32 * self.B)(*ff),
                                                 warr, _stream()), 'mc_ctx_set_seam_rows')
        self.seam_rows = dict(right=right, first_frame=ff, overlap=int(overlap))

    def clear_seam_rows(self):
        _lib.check(self.lib.mc_ctx_set_seam_rows(self.handle, 0, None, None, None, _stream()), 'mc_ctx_set_seam_rows')
        self.seam_rows = None

    def set_long_edits(self, on=True):
        """Let the edit table and the row seam table be set side by side (mc_ctx_set_long_edits): kept regions
        on the windows of long requests.  Off (the default) the two setters refuse each other.  On, ``sample_rows`` blends a shared
        frame's two x0 predictions and then takes x0 = gt where the OWNER's (the left row's) keep byte is set: upload equal ``keep`` /
        ``gt`` for both copies of a shared frame.  Switching off while both tables are set raises."""
        _lib.check(self.lib.mc_ctx_set_long_edits(self.handle, 1 if on else 0), 'mc_ctx_set_long_edits')
        self.long_edits = bool(on)

    def set_capacity_factor(self, cf):
        """Capacity factor of every MoE of this context (mc_ctx_set_capacity_factor): > 0 tutel's formula with it, 0 = no (token,
        choice) is dropped and no selection work runs; negative raises.  The library forgets the condition (the hoisted text MoE is
        routed too): ``set_condition`` must follow."""
        self._drop_graph()             # a captured graph has the routing launches of the old factor baked in
        self._keep = []
        _lib.check(self.lib.mc_ctx_set_capacity_factor(self.handle, float(cf)), 'mc_ctx_set_capacity_factor')

    @property
    def capacity_factor(self):
        return float(self.lib.mc_ctx_capacity_factor(self.handle))

    def set_row_seeds(self, seeds):
        """One Philox key per row (mc_ctx_set_row_seeds): ``seeds`` = B ints in [0, 2^64).  While set, ``sample_loop`` without
        ``noise`` and ``draw_rows`` give row b element r of draw d of ``mc_op_philox_normal(T * C, seeds[b], d)``, whatever B is and
        wherever the row sits; ``None`` clears the table."""
        if seeds is None:
            return self.clear_row_seeds()
        seeds = check_seeds(seeds, self.B)
        arr = (ctypes.c_uint64 * self.B)(*seeds)
        _lib.check(self.lib.mc_ctx_set_row_seeds(self.handle, arr, _stream()), 'mc_ctx_set_row_seeds')
        self.row_seeds = seeds

    def clear_row_seeds(self):
        _lib.check(self.lib.mc_ctx_set_row_seeds(self.handle, None, _stream()), 'mc_ctx_set_row_seeds')
        self.row_seeds = None

    def draw_rows(self, draw, out=None):
        """[B,T,C] = draw number ``draw`` of every row's own stream (mc_ctx_draw_rows); needs a seed table."""
        if out is None:
            out = torch.empty(self.B, self.T, self.C, device='cuda', dtype=torch.float32)
        out = _dev_f32(out, 'out')
        if tuple(out.shape) != (self.B, self.T, self.C):
            raise ValueError(f'out shape {tuple(out.shape)} != {(self.B, self.T, self.C)}')
        _lib.check(self.lib.mc_ctx_draw_rows(self.handle, _ptr(out), int(draw) & (2 ** 64 - 1), _stream()), 'mc_ctx_draw_rows')
        return out

    def graph_capture(self, x, noise, coefs):
        """Capture mc_sample_step into ONE hipGraph for the whole schedule.  ``x`` [B,T,C] is updated in place by every
        ``graph_step``, ``noise`` [B,T,C] is read by every replay (refill it in place between steps); both tensors must stay
        alive and keep their addresses.  ``coefs``: list of StepCoefs for every schedule index.  Call on a non-default
        torch stream (``with torch.cuda.stream(s):``).  A table of multistep coefficients (mode 2, all entries) takes ``noise=None``."""
        x, noise = _dev_f32(x, 'x'), (_dev_f32(noise, 'noise') if noise is not None else None)
        if tuple(x.shape) != (self.B, self.T, self.C) or (noise is not None and noise.shape != x.shape):
            raise ValueError(f'x / noise shape {tuple(x.shape)} != {(self.B, self.T, self.C)}')
        arr = (_lib.StepCoefs * len(coefs))(*coefs)
        self._graph_keep = (x, noise)
        _lib.check(self.lib.mc_ctx_graph_capture(self.handle, _ptr(x), _ptr(noise), arr, len(coefs), _stream()),
                   'mc_ctx_graph_capture')

    def graph_step(self, step_index):
        _lib.check(self.lib.mc_ctx_graph_step(self.handle, int(step_index), _stream()), 'mc_ctx_graph_step')

    def graph_release(self):
        _lib.check(self.lib.mc_ctx_graph_release(self.handle), 'mc_ctx_graph_release')
        self._graph_keep = None
        self._graph_state = None

    def sample_step_seeded(self, x_t, step_index, coefs, noise, sqrt_ab, sqrt_1mab, pre_seq=None, pre_noise=None,
                           transl=(), x_prev=None, x0=None):
        """One step with the reference's pre_seq / transl_req seeding: ``x_t`` is overwritten IN PLACE on its first
        frames (q_sample of ``pre_seq`` with ``pre_noise``; ``transl`` = [(channel, v0, v1), ...] already q-sampled)."""
        x = _dev_f32(x_t, 'x_t')
        n = _dev_f32(noise, 'noise')
        sd = _lib.Seed()
        sd.pre_len = 0
        if pre_seq is not None:
            p, pn = _dev_f32(pre_seq, 'pre_seq'), _dev_f32(pre_noise, 'pre_noise')
            if p.dim() != 3 or p.shape[0] != self.B or p.shape[2] != self.C or p.shape[1] > self.T or pn.shape != p.shape:
                raise ValueError(f'pre_seq shape {tuple(p.shape)} does not fit the window {(self.B, self.T, self.C)}')
            sd.pre_seq_dev, sd.pre_noise_dev, sd.pre_len = p.data_ptr(), pn.data_ptr(), int(p.shape[1])
        sd.sqrt_ab, sd.sqrt_1mab = float(sqrt_ab), float(sqrt_1mab)
        if len(transl) > _lib.MAX_TRANSL:
            raise ValueError(f'at most {_lib.MAX_TRANSL} transl_req items')
        sd.num_transl = len(transl)
        for k, (ch, v0, v1) in enumerate(transl):
            sd.transl_channel[k] = int(ch)
            sd.transl_value[k][0], sd.transl_value[k][1] = float(v0), float(v1)
        if x_prev is None:
            x_prev = torch.empty_like(x)
        _lib.check(self.lib.mc_sample_step_seeded(self.handle, _ptr(x), int(step_index), ctypes.byref(coefs), _ptr(n),
                                                  ctypes.byref(sd), _ptr(x_prev), _ptr(x0), _stream()), 'mc_sample_step_seeded')
        return x_prev

    def sample_step_inpaint(self, x_t, step_index, coefs, noise, gt, keep, gt_noise=None, blend_w=None, blend_len=0,
                            x_prev=None, x0=None):
        """RePaint step: ``keep`` is the bool outpainting_mask, ``gt`` the kept motion (both [B,T,C] on the device)."""
        x = _dev_f32(x_t, 'x_t')
        n = _dev_f32(noise, 'noise')
        g = _dev_f32(gt, 'gt')
        if keep.dtype != torch.bool or not keep.is_cuda or not keep.is_contiguous() or keep.shape != x.shape \
                or g.shape != x.shape:
            raise ValueError('outpainting_mask must be a contiguous bool device tensor of the shape of x_t (and gt too)')
        ip = _lib.Inpaint()
        ip.gt_dev, ip.keep_dev = g.data_ptr(), keep.data_ptr()
        gn = _dev_f32(gt_noise, 'gt_noise') if gt_noise is not None else None
        ip.gt_noise_dev = gn.data_ptr() if gn is not None else None
        bw = _dev_f32(blend_w, 'blend_w') if blend_len else None
        ip.blend_w_dev, ip.blend_len = (bw.data_ptr() if bw is not None else None), int(blend_len)
        if x_prev is None:
            x_prev = torch.empty_like(x)
        _lib.check(self.lib.mc_sample_step_inpaint(self.handle, _ptr(x), int(step_index), ctypes.byref(coefs), _ptr(n),
                                                   ctypes.byref(ip), _ptr(x_prev), _ptr(x0), _stream()),
                   'mc_sample_step_inpaint')
        return x_prev

    def renoise(self, x, noise, a, b, out=None):
        """out = a x + b noise (the forward ``_undo`` step of the resampling schedule)."""
        x, noise = _dev_f32(x, 'x'), _dev_f32(noise, 'noise')
        if out is None:
            out = torch.empty_like(x)
        _lib.check(self.lib.mc_op_renoise(_ptr(x), _ptr(noise), float(a), float(b), _ptr(out), x.numel(), _stream()),
                   'mc_op_renoise')
        return out

    def buffer(self, name, layer=0, dtype=torch.float32):
        """Copy of a named workspace buffer (tests)."""
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        _lib.check(self.lib.mc_ctx_get_buffer(self.handle, name.encode(), int(layer), ctypes.byref(p), ctypes.byref(n)),
                   'mc_ctx_get_buffer')
        out = torch.empty(n.value, device='cuda', dtype=dtype)
        # stream-ordered copy on the CURRENT torch stream: a plain hipMemcpy device-to-device is enqueued on the null stream and does not
        # block the host, so under a non-default (non-blocking) torch stream the reads of `out` that follow could overtake it
        import ctypes as _c
        hip = _c.CDLL('libamdhip64.so')
        hip.hipMemcpyAsync.argtypes = [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]
        rc = hip.hipMemcpyAsync(_c.c_void_p(out.data_ptr()), p, n.value * out.element_size(), 3, _c.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f'hipMemcpyAsync failed: {rc}')
        torch.cuda.current_stream().synchronize()
        return out

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.mc_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""Long-sequence generation by overlapping windows: the caller side of the RePaint mode.

Mirrors the window loop of the reference's ``finedance_eval`` (``tools/m2d_test.py:139-225``; the same scheme is in
``tools/s2g_test.py:180-260``): a sequence of ``total_frames`` is covered by windows of ``motion_length`` frames that
advance by ``motion_length - pre_frames``; in RePaint mode every window after the first keeps its first
``overlap_len`` frames equal to the previous window's last ones (``y = {gt, outpainting_mask}``), so the windows are
sequentially dependent; otherwise they are independent and the overlap is simply cut away when stitching.

Reference quirk kept as the default: the ``gt`` handed to the next window is the previous output AFTER
``* std + mean`` (``m2d_test.py:193,206-212``), although the sampler works on normalised motion; pass
``gt_space='normalised'`` to feed the normalised frames instead.

``sample_long_coupled`` (end of the file) is a third mode with no counterpart in the reference: all windows of a sequence in one
batch, their shared frames coupled at every sampler step.
"""
import numpy as np
import torch


def window_starts(total_frames, motion_length, pre_frames):
    """(number of windows, stride): m2d_test.py:143-145."""
    stride = motion_length - pre_frames
    if stride <= 0:
        raise ValueError('pre_frames must be smaller than motion_length')
    return (total_frames - pre_frames) // stride, stride


def _rows_per_frame(r):
    if int(r) != r or r < 1:
        raise ValueError(f'c_rows_per_frame={r}: a positive integer')
    return int(r)


def _condition_rows(c, total_frames, r, name='c'):
    """``c`` as a float32 tensor on the device it is on, holding the rows of ``total_frames`` frames at ``r`` rows per frame"""
    c = torch.as_tensor(c, dtype=torch.float32)
    if c.shape[0] < total_frames * r:
        raise ValueError(f'{name} holds {c.shape[0]} rows, {total_frames} frames at {r} rows per frame need {total_frames * r}')
    return c


def sample_long(model, total_frames, motion_length, pre_frames=30, c=None, text='', repaint=False, overlap_len=30,
                fix_very_first=True, first_gt=None, mean=None, std=None, gt_space='denormalised', input_dim=322,
                device=None, condition_kwargs=None, inference_kwargs=None, c_rows_per_frame=1):
    """model: MotionDiffusion mirror (``mc.build_architecture``), opt set on it like the reference tools do.
    c: control condition [total_frames * c_rows_per_frame, F] or None: one row per frame (music features), or ``c_rows_per_frame``
    rows per frame (the S2G audio condition: 16000 // 30 = 533 audio samples per frame, s2g_test.py:155); window i reads the rows
    of its frames, and a ``c`` that is a device tensor is sliced where it is.  condition_kwargs: ``xf_out`` /
    ``clip_feat`` for ONE window ([1, 77, *]).  inference_kwargs: dict or callable(window index) -> dict.
    Returns (stitched de-normalised motion [frames, input_dim] as float32 numpy, list of per-window outputs)."""
    dev = device or torch.device('cuda', torch.cuda.current_device())
    n_win, stride = window_starts(total_frames, motion_length, pre_frames)
    if n_win < 1:
        raise ValueError('sequence shorter than one window')
    mean = np.zeros(input_dim, np.float32) if mean is None else np.asarray(mean)
    std = np.ones(input_dim, np.float32) if std is None else np.asarray(std)
    r = _rows_per_frame(c_rows_per_frame)
    if c is not None:
        c = _condition_rows(c, total_frames, r)
    pieces_repaint, pieces_plain, windows, outputs = [], [], [], None
    for i in range(n_win):
        lo = i * stride
        kw = dict(motion=torch.zeros(1, motion_length, input_dim, device=dev),
                  motion_mask=torch.ones(1, motion_length, device=dev),
                  motion_length=torch.tensor([motion_length], device=dev).long(), num_intervals=1,
                  motion_metas=[{'text': text}])
        if c is not None:
            kw['c'] = c[lo * r:(lo + motion_length) * r].unsqueeze(0).to(dev)
        kw.update(condition_kwargs or {})
        inf = inference_kwargs(i) if callable(inference_kwargs) else dict(inference_kwargs or {})
        kw['inference_kwargs'] = inf
        if repaint:
            y = {}
            if overlap_len > 0:
                gt = torch.zeros(1, motion_length, input_dim, device=dev)
                keep = torch.zeros(1, motion_length, input_dim, dtype=torch.bool, device=dev)
                if i == 0:
                    if fix_very_first:
                        if first_gt is None:
                            raise ValueError('fix_very_first needs first_gt [>= overlap_len, input_dim]')
                        keep[:, :overlap_len] = True
                        gt[:, :overlap_len] = torch.as_tensor(first_gt, dtype=torch.float32)[:overlap_len].to(dev)
                else:
                    keep[:, :overlap_len] = True
                    gt[:, :overlap_len] = outputs[:, -overlap_len:]
                y = dict(gt=gt, outpainting_mask=keep)
            kw['y'] = y
        out = model(**kw)
        pred = out[0]['pred_motion'][:motion_length].detach().cpu().numpy()
        windows.append(pred)
        den = pred * std + mean                                   # m2d_test.py:206
        outputs = torch.as_tensor(den if gt_space == 'denormalised' else pred, dtype=torch.float32).unsqueeze(0).to(dev)
        pieces_repaint.append(den if i == n_win - 1 else den[:stride])          # :214-217
        pieces_plain.append(den if i == 0 else den[pre_frames:])                # :219-222
    rec = np.concatenate(pieces_repaint if repaint else pieces_plain, axis=0)   # :227-232
    return rec.astype(np.float32), windows


# ---- batched window driver ---------------------------------------------------------------------------------------------------
# BASELINE configs[3] ("batch=128, 512-frame long-sequence chunked attention, 4 GPUs") and SURVEY.md section 5 "Long-context": the
# reference's finedance_eval walks ONE window of ONE sequence per model call (tools/m2d_test.py:139-232, B = 1).  The windows of a
# sequence are independent when repaint=False (m2d_test.py:146-153 only rewrites `motion`, which the test branch never reads), and in
# RePaint mode window i only needs window i-1 of the SAME sequence -- so S sequences x W windows fold into the batch:
#   repaint=False   one batch of all S*W windows (chunked to `max_batch` windows per model call)
#   repaint=True    window i of all S sequences per batch, sequentially over i
# and the sequences shard over the ranks of torch.distributed (dist.py: no per-step collective, one gather of the stitched motions).
# NB the tutel MoE capacity couples the tokens of one model call (capacity = 1.5 x tokens / experts, batch-prioritised dropping), so
# a window sampled inside a batch is NOT bit-equal to the same window sampled alone: parity is "this batch on the oracle", exactly as
# for every other batched call of the path; the STITCHING is identical to sample_long's.


def stitch_windows(windows, pre_frames, repaint, mean=None, std=None):
    """De-normalise and stitch the windows of ONE sequence exactly as ``sample_long`` / m2d_test.py:206-232 do:
    RePaint mode keeps the first ``stride`` frames of every window but the last, plain mode cuts the first ``pre_frames``
    frames of every window but the first."""
    L = windows[0].shape[0]
    stride = L - pre_frames
    mean = 0.0 if mean is None else np.asarray(mean)
    std = 1.0 if std is None else np.asarray(std)
    den = [np.asarray(w) * std + mean for w in windows]
    n = len(den)
    if repaint:
        parts = [d if i == n - 1 else d[:stride] for i, d in enumerate(den)]
    else:
        parts = [d if i == 0 else d[pre_frames:] for i, d in enumerate(den)]
    return np.concatenate(parts, axis=0).astype(np.float32)


def rank_sequences(n_seq, rank, ws):
    """Contiguous block of sequence indices rank `rank` of `ws` owns (uneven counts allowed: the first ranks take one more)."""
    base, extra = divmod(n_seq, ws)
    lo = rank * base + min(rank, extra)
    return list(range(lo, lo + base + (1 if rank < extra else 0)))


def _gather_ragged(local, lengths, owners, input_dim, device):
    """all-gather of per-sequence motions of different lengths in ONE collective (dist.gather_results): every rank pads its block to
    the longest sequence of the job.  No length exchange: a stitched motion has (n_windows - 1) * stride + window frames, which every
    rank computes from the global `total_frames` list (`lengths`: sequence -> frames)."""
    from . import dist as mcd
    if not mcd.is_dist():
        return local
    rank, ws = mcd.world()
    per = max(len(o) for o in owners)
    maxlen = max(lengths)
    buf = torch.zeros(per, maxlen, input_dim, device=device)
    for k, s in enumerate(owners[rank]):
        if local[s].shape[0] != lengths[s]:
            raise RuntimeError(f'sequence {s}: stitched {local[s].shape[0]} frames, expected {lengths[s]}')
        buf[k, :lengths[s]] = torch.as_tensor(local[s], device=device)
    allb = mcd.gather_results(buf).view(ws, per, maxlen, input_dim).cpu().numpy()
    out = {}
    for r in range(ws):
        for k, s in enumerate(owners[r]):
            out[s] = allb[r, k, :lengths[s]]
    return out


def sample_long_batched(model, total_frames, motion_length, pre_frames=30, c=None, text=None, repaint=False, overlap_len=30,
                        fix_very_first=True, first_gt=None, mean=None, std=None, gt_space='denormalised', input_dim=322,
                        device=None, condition_kwargs=None, inference_kwargs=None, max_batch=160, shard=True, c_rows_per_frame=1):
    """S sequences x their windows through as few model calls as the mode allows (see the block comment above).

    total_frames: int (every sequence) or a list of S ints.  c: list of S conditions [total_s * c_rows_per_frame, F] (or a tensor
    [S, total * c_rows_per_frame, F]) or None; ``c_rows_per_frame`` as in ``sample_long``.  text: list of S prompts (or one string).  condition_kwargs: per-SEQUENCE tensors with leading dimension S
    (``xf_out`` [S, 77, *] / ``clip_feat``); every window of sequence s gets row s.  first_gt: [S, >= overlap_len, input_dim] (RePaint,
    fix_very_first).  inference_kwargs: dict, or callable(pairs) -> dict for one model call, ``pairs`` = [(sequence, window), ...] in
    batch order (noise [b, L, C] / step_noise for parity runs).  max_batch: windows per model call (the per-GPU batch; BASELINE
    configs[3]: 128 sequences x 5 windows / 4 GPUs = 160).  shard: split the SEQUENCES over the ranks of an initialised process group
    (contiguous blocks) and gather the stitched motions on every rank.

    Returns (list of S stitched de-normalised motions [frames_s, input_dim] float32 numpy -- ALL S sequences on every rank, gathered
    by one padded all-gather --, dict (sequence, window) -> window output of THIS RANK's sequences only: the raw windows are not
    gathered)."""
    dev = device or torch.device('cuda', torch.cuda.current_device())
    S = len(total_frames) if not isinstance(total_frames, int) else (len(c) if c is not None else (len(text) if isinstance(text, (list, tuple)) else 1))
    totals = [int(total_frames)] * S if isinstance(total_frames, int) else [int(t) for t in total_frames]
    texts = list(text) if isinstance(text, (list, tuple)) else [text or ''] * S
    if len(texts) != S or (c is not None and len(c) != S):
        raise ValueError('text / c must have one entry per sequence')
    n_wins = []
    for t in totals:
        n, stride = window_starts(t, motion_length, pre_frames)
        if n < 1:
            raise ValueError('sequence shorter than one window')
        n_wins.append(n)
    from . import dist as mcd
    rank, ws = mcd.world() if shard else (0, 1)
    owners = [rank_sequences(S, r, ws) for r in range(ws)]
    mine = owners[rank]
    stride = motion_length - pre_frames
    r = _rows_per_frame(c_rows_per_frame)
    cs = None if c is None else [_condition_rows(x, totals[s], r, f'c[{s}]') for s, x in enumerate(c)]
    cond = {k: v for k, v in (condition_kwargs or {}).items()}
    for k, v in cond.items():
        if not torch.is_tensor(v) or v.shape[0] != S:
            raise ValueError(f'condition_kwargs[{k!r}] must be a tensor with one row per sequence ({S})')
    windows, prev = {}, {}

    def run(pairs):
        b = len(pairs)
        kw = dict(motion=torch.zeros(b, motion_length, input_dim, device=dev), motion_mask=torch.ones(b, motion_length, device=dev),
                  motion_length=torch.full((b, 1), motion_length, device=dev).long(), num_intervals=1,
                  motion_metas=[{'text': texts[s]} for s, _ in pairs])
        if cs is not None:
            kw['c'] = torch.stack([cs[s][w * stride * r:(w * stride + motion_length) * r] for s, w in pairs]).to(dev)
        idx = torch.tensor([s for s, _ in pairs])
        for k, v in cond.items():
            kw[k] = v[idx.to(v.device)]
        kw['inference_kwargs'] = inference_kwargs(pairs) if callable(inference_kwargs) else dict(inference_kwargs or {})
        if repaint:
            y = {}
            if overlap_len > 0:
                gt = torch.zeros(b, motion_length, input_dim, device=dev)
                keep = torch.zeros(b, motion_length, input_dim, dtype=torch.bool, device=dev)
                for j, (s, w) in enumerate(pairs):
                    if w == 0:
                        if fix_very_first:
                            if first_gt is None:
                                raise ValueError('fix_very_first needs first_gt [S, >= overlap_len, input_dim]')
                            keep[j, :overlap_len] = True
                            gt[j, :overlap_len] = torch.as_tensor(first_gt[s], dtype=torch.float32)[:overlap_len].to(dev)
                    else:
                        keep[j, :overlap_len] = True
                        gt[j, :overlap_len] = prev[s][-overlap_len:]
                y = dict(gt=gt, outpainting_mask=keep)
            kw['y'] = y
        out = model(**kw)
        for j, (s, w) in enumerate(pairs):
            pred = out[j]['pred_motion'][:motion_length].detach().cpu().numpy()
            windows[(s, w)] = pred
            if repaint:          # what the next window of this sequence keeps (m2d_test.py:193,206-212: the DE-normalised frames by default)
                den = pred * (1.0 if std is None else np.asarray(std)) + (0.0 if mean is None else np.asarray(mean))
                prev[s] = torch.as_tensor(den if gt_space == 'denormalised' else pred, dtype=torch.float32).to(dev)

    if repaint:
        for w in range(max((n_wins[s] for s in mine), default=0)):
            todo = [(s, w) for s in mine if w < n_wins[s]]
            for k in range(0, len(todo), max_batch):
                run(todo[k:k + max_batch])
    else:
        todo = [(s, w) for s in mine for w in range(n_wins[s])]
        for k in range(0, len(todo), max_batch):
            run(todo[k:k + max_batch])
    local = {s: stitch_windows([windows[(s, w)] for w in range(n_wins[s])], pre_frames, repaint, mean, std) for s in mine}
    lengths = [(n_wins[s] - 1) * stride + motion_length for s in range(S)]
    full = _gather_ragged(local, lengths, owners, input_dim, dev) if (shard and mcd.is_dist()) else local
    return [full[s] for s in range(S)], windows



# ---- coupled windows: all windows of a sequence in ONE batch, seams blended per step --------------------------------------------------
# The third mode beside the two above (no reference counterpart; the window-parallel scheme of PriorMDM's DoubleTake handshake and of
# MultiDiffusion's overlap averaging): every window of a sequence is a row of the same model call, after every denoiser call the two x0
# predictions that cover the same frames are blended into one, and both windows take their sampler update from it with the same noise
# (engine.NativeContext.set_seams, csrc sampler_seam_k).  The overlapping frames of x_t stay bit-equal in both windows through the whole
# walk, so the stitched motion has no seam by construction -- and nothing is sequential across windows.  What it does to sample QUALITY
# against RePaint windows is unmeasured (no trained checkpoint here).  As for every batched call, the tutel capacity couples the tokens
# of one model call: parity of a coupled batch is "this batch on the oracle".


def check_seams(first_frame, motion_length, overlap, weights=None, rows=None):
    """The plan rules of ``mc_ctx_set_seams``, checked on the host: ``0 < 2 overlap <= motion_length`` (a frame lies in two windows at
    most); consecutive rows are neighbours (``first_frame[b + 1] == first_frame[b] + motion_length - overlap``) or disjoint
    (``>= first_frame[b] + motion_length``); no negative entry; ``weights``: ``overlap`` numbers in [0, 1].  Returns (first_frame as a
    list of ints, weights as a list of floats or None); raises ValueError."""
    T = int(motion_length)
    if int(overlap) != overlap or not 0 < 2 * int(overlap) <= T:
        raise ValueError(f'overlap={overlap!r}: an integer with 0 < 2 overlap <= motion_length ({T})')
    ov = int(overlap)
    ff = [int(v) for v in first_frame]
    if any(int(v) != v for v in first_frame):
        raise ValueError('first_frame: integers')
    if not ff or (rows is not None and len(ff) != int(rows)):
        raise ValueError(f'first_frame has {len(ff)} entries for {rows if rows is not None else "at least one"} rows')
    if any(v < 0 or v >= 2 ** 31 - T for v in ff):
        raise ValueError('first_frame: entries in [0, 2^31 - motion_length)')
    for b in range(len(ff) - 1):
        gap = ff[b + 1] - ff[b]
        if gap != T - ov and gap < T:
            raise ValueError(f'first_frame[{b + 1}] = {ff[b + 1]} after first_frame[{b}] = {ff[b]}: neither its neighbour (+{T - ov}) '
                             f'nor disjoint from it (>= +{T})')
    w = None
    if weights is not None:
        w = [float(v) for v in weights]
        if len(w) != ov or not all(0.0 <= v <= 1.0 for v in w):
            raise ValueError(f'weights: {ov} numbers in [0, 1]')
    return ff, w


def seam_plan(total_frames, motion_length, overlap):
    """(number of windows, first frame of every window, stitched length) of one sequence: ``window_starts`` with ``pre_frames = overlap``."""
    if not 0 < 2 * int(overlap) <= int(motion_length):
        raise ValueError(f'overlap={overlap!r}: 0 < 2 overlap <= motion_length ({motion_length})')
    n, stride = window_starts(int(total_frames), int(motion_length), int(overlap))
    if n < 1:
        raise ValueError('sequence shorter than one window')
    return n, [i * stride for i in range(n)], (n - 1) * stride + int(motion_length)


def sample_long_coupled(model, total_frames, motion_length, overlap, c=None, text=None, weights=None, noise=None, mean=None, std=None,
                        input_dim=322, device=None, condition_kwargs=None, inference_kwargs=None, max_batch=160, shard=True,
                        c_rows_per_frame=1):
    """S sequences, ALL windows of a sequence as consecutive rows of one model call, seams coupled at every step (block comment above).

    total_frames / c / text / condition_kwargs / c_rows_per_frame / shard as in ``sample_long_batched``; ``overlap`` plays the part of
    ``pre_frames`` (stride = motion_length - overlap, 0 < 2 overlap <= motion_length).  weights: the right window's share per shared
    frame (default ``(f + 1) / (overlap + 1)``).  The model calls are chunked by WHOLE sequences up to ``max_batch`` windows; a sequence
    with more windows than that is an error.  The initial noise is drawn once per GLOBAL frame (``inference_kwargs['generator']``, or
    ``noise``: a list of S tensors [stitched frames of s, input_dim]) and gathered into the windows, so x_T agrees on shared frames.
    inference_kwargs: dict, or callable(pairs) -> dict as in ``sample_long_batched`` (``noise`` / ``graph`` / ``pre_seq`` do not go
    with this mode).  Stitching is RePaint mode's: the first stride frames of every window but the last; the shared frames are
    asserted equal first.  Returns (list of S stitched de-normalised motions -- all S on every rank --, dict (sequence, window) ->
    window output of this rank's sequences)."""
    dev = device or torch.device('cuda', torch.cuda.current_device())
    S = len(total_frames) if not isinstance(total_frames, int) else (len(c) if c is not None else (len(text) if isinstance(text, (list, tuple)) else 1))
    totals = [int(total_frames)] * S if isinstance(total_frames, int) else [int(t) for t in total_frames]
    texts = list(text) if isinstance(text, (list, tuple)) else [text or ''] * S
    if len(texts) != S or (c is not None and len(c) != S) or (noise is not None and len(noise) != S):
        raise ValueError('text / c / noise must have one entry per sequence')
    L, ov = int(motion_length), int(overlap)
    plans = [seam_plan(t, L, ov) for t in totals]
    stride = L - ov
    if weights is not None:
        check_seams([0], L, ov, weights)
    for s, (n, _, _) in enumerate(plans):
        if n > max_batch:
            raise ValueError(f'sequence {s} has {n} windows, more than max_batch={max_batch}: the windows of one sequence share a model call')
    from . import dist as mcd
    rank, ws = mcd.world() if shard else (0, 1)
    owners = [rank_sequences(S, r, ws) for r in range(ws)]
    mine = owners[rank]
    r = _rows_per_frame(c_rows_per_frame)
    cs = None if c is None else [_condition_rows(x, totals[s], r, f'c[{s}]') for s, x in enumerate(c)]
    cond = {k: v for k, v in (condition_kwargs or {}).items()}
    for k, v in cond.items():
        if not torch.is_tensor(v) or v.shape[0] != S:
            raise ValueError(f'condition_kwargs[{k!r}] must be a tensor with one row per sequence ({S})')
    windows = {}

    def run(seqs):
        pairs = [(s, w) for s in seqs for w in range(plans[s][0])]
        b = len(pairs)
        inf = inference_kwargs(pairs) if callable(inference_kwargs) else dict(inference_kwargs or {})
        for k in ('noise', 'graph', 'pre_seq', 'transl_req'):
            if inf.get(k) is not None and inf.get(k) is not False:
                raise ValueError(f'inference_kwargs[{k!r}] does not go with coupled windows')
        first, x_T, base = [], [], 0
        for s in seqs:
            n, ff, frames = plans[s]
            if noise is not None:
                z = torch.as_tensor(noise[s], dtype=torch.float32).to(dev)
                if tuple(z.shape) != (frames, input_dim):
                    raise ValueError(f'noise[{s}] of shape {tuple(z.shape)}: expected {(frames, input_dim)}')
            else:
                z = torch.randn(frames, input_dim, device=dev, generator=inf.get('generator'))
            x_T += [z[f:f + L] for f in ff]                 # one draw per global frame: x_T agrees on shared frames
            first += [base + f for f in ff]
            base += frames                                  # the next sequence starts past this one's last window: disjoint rows
        inf['noise'] = torch.stack(x_T)
        kw = dict(motion=torch.zeros(b, L, input_dim, device=dev), motion_mask=torch.ones(b, L, device=dev),
                  motion_length=torch.full((b, 1), L, device=dev).long(), num_intervals=1,
                  motion_metas=[{'text': texts[s]} for s, _ in pairs], seams=dict(first_frame=first, overlap=ov, weights=weights))
        if cs is not None:
            kw['c'] = torch.stack([cs[s][w * stride * r:(w * stride + L) * r] for s, w in pairs]).to(dev)
        idx = torch.tensor([s for s, _ in pairs])
        for k, v in cond.items():
            kw[k] = v[idx.to(v.device)]
        kw['inference_kwargs'] = inf
        out = model(**kw)
        for j, (s, w) in enumerate(pairs):
            windows[(s, w)] = out[j]['pred_motion'][:L].detach().cpu().numpy()

    chunk, used = [], 0
    for s in mine:
        if chunk and used + plans[s][0] > max_batch:
            run(chunk)
            chunk, used = [], 0
        chunk.append(s)
        used += plans[s][0]
    if chunk:
        run(chunk)
    local = {}
    for s in mine:
        ws_ = [windows[(s, w)] for w in range(plans[s][0])]
        for w in range(len(ws_) - 1):
            if not np.array_equal(ws_[w][stride:], ws_[w + 1][:ov]):
                raise RuntimeError(f'sequence {s}: windows {w} and {w + 1} differ on their shared frames (the sampler did not run coupled)')
        local[s] = stitch_windows(ws_, ov, True, mean, std)
    lengths = [p[2] for p in plans]
    full = _gather_ragged(local, lengths, owners, input_dim, dev) if (shard and mcd.is_dist()) else local
    return [full[s] for s in range(S)], windows

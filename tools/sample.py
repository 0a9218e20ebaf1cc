#!/usr/bin/env python
"""Thin counterpart of the reference's tools/visualize.py for the MI355X path: config + checkpoint -> sampled motion
-> de-normalised SMPL-X .npz (motionx; + the body model's joints / vertices with --smplx_model) or feature .npy (+ joint
positions with --pose_npy), everything between the condition features and the finished arrays on the device.

    python tools/sample.py CONFIG CHECKPOINT --text "a person walks" --motion_length 120 --out ./samples \\
        [--clip_feat feats.npy | --xf_out xf.npy | --random-condition SEED]  [--mean mean.npy --std std.npy]  [--pose_npy joints.npy]
        [--anim_dir frames/ | --anim_avi clip.avi [--anim_size 1000x1000] [--anim_fps 20]]
        [--smplx_model SMPLX_NEUTRAL.npz --joints_npy joints.npy [--verts_npy verts.npy] [--render_dir frames/ | --render_avi clip.avi [--render_size 960x720]]]
        [--avi_quality 90]  [--sampler ddpm|ddim|dpmpp [--steps N [--spacing time|logsnr]]]  [--seeds a,b,c] [--no_drop]
        [--edit_npz edit.npz [--keep_frames 0-9,150-195] [--keep_parts lleg,rleg,root]]     (one --text, with --no_drop)

The CLIP tokenizer is not available offline: prompts only name the output file unless the `clip` package is importable
(then they are tokenized and encoded by the device CLIP tower when the checkpoint carries clip.* weights).
CHECKPOINT may be "synthetic[:SEED]" for deterministic random-init weights of the configured architecture.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)

import motioncraft_amd as mc                                    # noqa: E402
from motioncraft_amd import postprocess, render, skeleton, synthetic, video   # noqa: E402
from motioncraft_amd.checkpoint import load_checkpoint          # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='motioncraft_amd sampling')
    p.add_argument('config')
    p.add_argument('checkpoint')
    p.add_argument('--text', nargs='+', required=True)
    p.add_argument('--motion_length', type=int, nargs='+', required=True)
    p.add_argument('--out', default='./samples')
    p.add_argument('--pose_npy', default=None, metavar='PATH',
                   help='human_ml3d / kit_ml configs: also save the stitched, filtered joint positions [frames, J, 3] (tools/visualize.py:55-56)')
    p.add_argument('--anim_dir', default=None, metavar='DIR',
                   help='human_ml3d / kit_ml configs: draw the stitched, filtered joints as the skeleton animation of plot_3d_motion on the '
                        'device and write frame_%%d.bmp there (+ an mp4 when ffmpeg is on PATH); no title, no anti-aliasing')
    p.add_argument('--anim_size', default='1000x1000', metavar='WxH', help='frame size of --anim_dir (the reference: 1000x1000)')
    p.add_argument('--anim_fps', type=float, default=20.0, help='frame rate of the mp4 of --anim_dir (the reference: 20)')
    p.add_argument('--smplx_model', default=None, metavar='PATH', help='motionx configs: the published SMPL-X model file (.npz)')
    p.add_argument('--joints_npy', default=None, metavar='PATH',
                   help='with --smplx_model: save the 55 SMPL-X joints [frames, 55, 3] of the stitched, filtered motion (tools/s2g_test.py:406)')
    p.add_argument('--verts_npy', default=None, metavar='PATH', help='with --smplx_model: save the skinned vertices [frames, V, 3]')
    p.add_argument('--render_dir', default=None, metavar='DIR',
                   help='with --smplx_model: render the stitched, filtered motion on the device and write frame_%%d.bmp there '
                        '(+ an mp4 when ffmpeg is on PATH); the reference scene of fast_render.py, colours not pinned to pyrender')
    p.add_argument('--render_size', default='960x720', metavar='WxH', help='frame size of --render_dir (the reference: 960x720)')
    p.add_argument('--render_fps', type=float, default=30.0, help='frame rate of the mp4 of --render_dir')
    p.add_argument('--render_avi', default=None, metavar='FILE',
                   help='with --smplx_model: encode the rendered frames on the device into one Motion-JPEG AVI (no --render_dir needed)')
    p.add_argument('--anim_avi', default=None, metavar='FILE',
                   help='human_ml3d / kit_ml configs: encode the skeleton animation on the device into one Motion-JPEG AVI (no --anim_dir needed)')
    p.add_argument('--avi_quality', type=int, default=90, metavar='N', help='JPEG quality of --render_avi / --anim_avi, 1..100')
    p.add_argument('--clip_feat', help='.npy [n,77,512] CLIP text features (ln_final output)')
    p.add_argument('--xf_out', help='.npy [n,77,text_latent_dim] frozen condition embedding')
    p.add_argument('--random-condition', type=int, default=None, metavar='SEED')
    p.add_argument('--mean'), p.add_argument('--std')
    p.add_argument('--seed', type=int, default=0)
    # independent requests: one Philox key per sample instead of the one --seed of the call, and routing without token drops -- with both,
    # a sample is a function of its own prompt, length and seed at this batch size (quality at --no_drop with trained weights: unmeasured)
    p.add_argument('--seeds', default=None, metavar='A,B,C', help='one integer seed per sample (replaces --seed): row-keyed noise')
    p.add_argument('--no_drop', action='store_true', help='MoE capacity factor 0: no token is dropped (default: the model\'s 1.5)')
    # long-sequence / RePaint options read by the sampler through cfg.model['opt'] (tools/visualize.py:96-110)
    p.add_argument('--repaint', action='store_true'), p.add_argument('--overlap_len', type=int, default=0)
    p.add_argument('--same_overlap_noisy', action='store_true'), p.add_argument('--no_resample', action='store_true')
    p.add_argument('--timestep_respacing', default='ddim50'), p.add_argument('--jump_n_sample', type=int, default=5)
    p.add_argument('--jump_length', type=int, default=3), p.add_argument('--addBlend', type=bool, default=True)
    p.add_argument('--no_repaint', action='store_true')
    # MI355X options: fp16 MFMA (also switched on by a top-level `fp16 = dict(...)` in the config, tools/test.py:95-97), replay
    p.add_argument('--fp16', choices=['split', 'plain'], default=None, help='fp16-MFMA mode: split = fp32-class hi/lo form')
    p.add_argument('--graph', action='store_true', help='hipGraph replay of the sampler step')
    # the sampler: default = the config's inference_type; dpmpp = DPM-Solver++ (2M), a second-order multistep walk for 10-20 steps (no
    # counterpart in the reference; sample quality with trained weights at those step counts is unmeasured)
    p.add_argument('--sampler', choices=['ddpm', 'ddim', 'dpmpp'], default=None, help="default: the config's inference_type")
    p.add_argument('--steps', type=int, default=None, metavar='N', help='with --sampler dpmpp: respace the test schedule to N steps')
    p.add_argument('--spacing', choices=['time', 'logsnr'], default=None,
                   help='with --sampler dpmpp --steps N: uniform in the timestep (ddimN, default) or in the log-SNR (logsnrN)')
    # an edited motion: frames / channels of the ONE sample are given, the rest is generated around them.  The file
    # holds `motion` [n, C] in the space of the saved result and `keep` [n, C], or `keep_frames` [k] and / or `keep_channels` [m] (one of
    # them alone: all channels of the frames / the channels on all frames; both: their product); the two flags replace the file's mask.
    # Sample quality of edited motions with released weights is unmeasured.
    p.add_argument('--edit_npz', default=None, metavar='FILE', help='npz with motion [n,C] and keep [n,C] (or keep_frames / keep_channels): '
                   'the given part of the sample; one --text, with --no_drop')
    p.add_argument('--keep_frames', default=None, metavar='A-B,C', help='with --edit_npz: the given frames, e.g. 0-9,150-195')
    p.add_argument('--keep_parts', default=None, metavar='P,Q', help='with --edit_npz: the given body parts, e.g. lleg,rleg,root')
    return p.parse_args(argv)


def parse_frames(spec, n):
    """'0-9,150-195' -> the sorted frame list, every frame in [0, n)"""
    out = set()
    for part in spec.split(','):
        try:
            lo, _, hi = part.strip().partition('-')
            lo, hi = int(lo), int(hi) if hi else int(lo)
        except ValueError:
            raise SystemExit(f'--keep_frames takes ranges like 0-9,150-195, got {spec!r}')
        if not 0 <= lo <= hi < n:
            raise SystemExit(f'--keep_frames {part!r} outside the {n} frames of the edit\'s motion')
        out.update(range(lo, hi + 1))
    return sorted(out)


def check_edit_args(a):
    """--edit_npz against the options it cannot run beside (before anything is built)"""
    if a.edit_npz is None:
        if a.keep_frames is not None or a.keep_parts is not None:
            raise SystemExit('--keep_frames / --keep_parts belong to --edit_npz FILE')
        return
    if a.repaint or a.overlap_len or a.same_overlap_noisy:
        raise SystemExit('--edit_npz edits ONE window: the long-sequence window modes (--repaint, --overlap_len, --same_overlap_noisy) keep '
                         'their own outpainting')
    if a.graph:
        raise SystemExit('--edit_npz does not run under --graph (edited rows are not replayed)')
    if len(a.text) != 1:
        raise SystemExit(f'--edit_npz edits one sample, got {len(a.text)} prompts')
    if not a.no_drop:
        raise SystemExit('--edit_npz runs the request at MoE capacity factor 0: pass --no_drop')
    if a.clip_feat:
        raise SystemExit('--edit_npz takes the prompt, --xf_out or --random-condition, not --clip_feat')


def load_edit(a, dataset, C, mean=None, std=None):
    """-> serve.Edit from --edit_npz / --keep_frames / --keep_parts; ``mean`` / ``std`` (--mean / --std): the motion is normalised with
    them, (motion - mean) / (std + 1e-9), like the saved result is de-normalised"""
    from motioncraft_amd.serve import Edit
    z = np.load(a.edit_npz)
    if 'motion' not in z:
        raise SystemExit(f'{a.edit_npz}: no array `motion`')
    motion = np.asarray(z['motion'], dtype=np.float32)
    if motion.ndim != 2 or motion.shape[1] != C:
        raise SystemExit(f'{a.edit_npz}: motion is {motion.shape}, expected [n, {C}]')
    n = motion.shape[0]
    if n > a.motion_length[0]:
        raise SystemExit(f'{a.edit_npz}: motion has {n} frames, --motion_length is {a.motion_length[0]}')
    if mean is not None and std is not None:
        motion = ((motion - mean) / (std + 1e-9)).astype(np.float32)
    motion = torch.from_numpy(motion)
    if a.keep_frames is not None or a.keep_parts is not None:
        frames = parse_frames(a.keep_frames, n) if a.keep_frames is not None else None
        if a.keep_parts is not None:
            try:
                return Edit.parts(motion, [v.strip() for v in a.keep_parts.split(',')], dataset, frames)
            except ValueError as e:
                raise SystemExit(f'--keep_parts: {e}')
        return Edit.keyframes(motion, frames)
    if 'keep' in z:
        keep = np.asarray(z['keep'])
        if keep.shape != motion.shape:
            raise SystemExit(f'{a.edit_npz}: keep is {keep.shape}, motion {tuple(motion.shape)}')
        keep = torch.from_numpy(keep != 0)
    elif 'keep_frames' in z or 'keep_channels' in z:
        fr = np.asarray(z['keep_frames']).astype(np.int64).reshape(-1) if 'keep_frames' in z else np.arange(n)
        ch = np.asarray(z['keep_channels']).astype(np.int64).reshape(-1) if 'keep_channels' in z else np.arange(C)
        if fr.size == 0 or ch.size == 0 or fr.min() < 0 or fr.max() >= n or ch.min() < 0 or ch.max() >= C:
            raise SystemExit(f'{a.edit_npz}: keep_frames / keep_channels outside motion {tuple(motion.shape)}')
        keep = torch.zeros(n, C, dtype=torch.bool)
        keep[torch.from_numpy(fr)[:, None], torch.from_numpy(ch)[None, :]] = True
    else:
        raise SystemExit(f'{a.edit_npz}: no mask -- keep, keep_frames / keep_channels, or --keep_frames / --keep_parts')
    try:
        return Edit(motion, keep)
    except ValueError as e:
        raise SystemExit(f'{a.edit_npz}: {e}')


def run_edit(model, a, edit, T, dev):
    """the one request through serve.RequestBatcher at capacity factor 0 -> what model(**kw) returns for it"""
    from motioncraft_amd.serve import Request, RequestBatcher
    dims = model.model.dims
    seed = int(a.seeds.split(',')[0], 0) if a.seeds is not None else a.seed
    if a.xf_out:
        cond = dict(xf_out=torch.from_numpy(np.load(a.xf_out)).float()[0].to(dev))
    elif a.random_condition is not None:
        g = torch.Generator().manual_seed(a.random_condition)
        cond = dict(xf_out=torch.nn.functional.layer_norm(torch.randn(dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).to(dev))
    else:
        cond = dict(text=a.text[0])
    # the schedule is the model's (apply_sampler has respaced it); eta = 0 and order 2 are what MotionDiffusion.forward samples with
    bt = RequestBatcher(model, batch=1, frames=T, sampler=model.inference_type, capacity_factor=0, eta=0.0, order=2)
    h = bt.submit(Request(length=a.motion_length[0], seed=seed & (2 ** 64 - 1), edit=edit, **cond))
    pred = bt.run()[h]
    out = torch.zeros(T, dims['input_feats'])
    out[:pred.shape[0]] = pred.cpu()
    return [{'pred_motion': out}]


def apply_sampler(cfg, a):
    """--sampler / --steps / --spacing -> cfg.model (inference_type, diffusion_test.respace)"""
    if a.sampler != 'dpmpp':
        if a.steps is not None or a.spacing is not None:
            raise SystemExit('--steps / --spacing belong to --sampler dpmpp (the other samplers take the schedule of the config / '
                             '--timestep_respacing)')
        if a.sampler is not None:
            cfg.model['inference_type'] = a.sampler
        return
    if a.repaint:
        raise SystemExit('--sampler dpmpp has no outpainting (RePaint) form: use --sampler ddim with --repaint')
    cfg.model['inference_type'] = 'dpmpp'
    if a.steps is None:
        if a.spacing is not None:
            raise SystemExit('--spacing needs --steps N')
        return
    if a.steps < 2:
        raise SystemExit(f'--steps must be at least 2, got {a.steps}')
    test = dict(cfg.model['diffusion_test'])
    test['respace'] = ('logsnr' if a.spacing == 'logsnr' else 'ddim') + str(a.steps)
    cfg.model['diffusion_test'] = test


def main():
    a = parse_args()
    assert len(a.text) == len(a.motion_length)
    check_edit_args(a)
    cfg = mc.Config.fromfile(a.config)
    cfg.model['opt'] = a
    apply_sampler(cfg, a)
    model = mc.build_architecture(cfg.model)
    if a.checkpoint.startswith('synthetic'):
        seed = int(a.checkpoint.split(':')[1]) if ':' in a.checkpoint else 0
        model.load_state_dict({'model.' + k: v for k, v in synthetic.make_state_dict(model.model.dims, seed).items()})
    else:
        load_checkpoint(model, a.checkpoint, map_location='cpu')
    model.eval()
    if a.fp16 or cfg.get('fp16', None) is not None:
        mc.wrap_fp16_model(model, split=(a.fp16 != 'plain'))
    dims = model.model.dims
    if a.pose_npy and dims.get('dataset', 'motionx') == 'motionx':
        raise ValueError('--pose_npy saves joint positions recovered from human_ml3d / kit_ml features; a motionx config '
                         'writes the SMPL-X .npz instead')
    if (a.anim_dir or a.anim_avi) and dims.get('dataset', 'motionx') == 'motionx':
        raise ValueError('--anim_dir / --anim_avi draw the skeleton of a human_ml3d / kit_ml sample; a motionx config renders the mesh with '
                         '--smplx_model PATH --render_dir DIR')
    anim_size = render.parse_size(a.anim_size, '--anim_size')
    if max(anim_size) > skeleton.MAX_SIZE:
        raise ValueError(f'--anim_size: at most {skeleton.MAX_SIZE} pixels a side, got {a.anim_size!r}')
    if not a.anim_fps > 0:
        raise ValueError(f'--anim_fps must be positive, got {a.anim_fps}')
    if (a.joints_npy or a.verts_npy or a.smplx_model) and dims.get('dataset', 'motionx') != 'motionx':
        raise ValueError('--smplx_model / --joints_npy / --verts_npy run the SMPL-X body model on a motionx sample; a human_ml3d / '
                         'kit_ml config saves joints with --pose_npy')
    if (a.joints_npy or a.verts_npy or a.render_dir or a.render_avi) and not a.smplx_model:
        raise ValueError('--joints_npy / --verts_npy / --render_dir / --render_avi need the body model file: --smplx_model PATH')
    if a.smplx_model and not (a.joints_npy or a.verts_npy or a.render_dir or a.render_avi):
        raise ValueError('--smplx_model alone writes nothing: name an output with --joints_npy PATH, --verts_npy PATH, '
                         '--render_dir DIR and / or --render_avi FILE')
    if not 1 <= a.avi_quality <= 100:
        raise ValueError(f'--avi_quality must be in 1..100, got {a.avi_quality}')
    render_size = render.parse_size(a.render_size)
    if not a.render_fps > 0:
        raise ValueError(f'--render_fps must be positive, got {a.render_fps}')
    n, T, C = len(a.text), max(a.motion_length), dims['input_feats']
    if not 1 <= T <= dims['max_seq_len']:
        raise ValueError(f'motion_length must be in [1, {dims["max_seq_len"]}]')
    dev = torch.device('cuda', torch.cuda.current_device())
    mask = torch.zeros(n, T, device=dev)
    for i, m in enumerate(a.motion_length):
        mask[i, :m] = 1
    mean = np.load(a.mean) if a.mean else None
    std = np.load(a.std) if a.std else None
    if a.edit_npz:
        out = run_edit(model, a, load_edit(a, dims.get('dataset', 'motionx'), C, mean, std), T, dev)
    else:
        if a.seeds is not None:
            try:
                seeds = [int(v, 0) for v in a.seeds.split(',')]
            except ValueError:
                raise SystemExit(f'--seeds takes comma-separated integers, got {a.seeds!r}')
            if len(seeds) != n:
                raise SystemExit(f'--seeds names {len(seeds)} seeds for {n} samples')
            ikw = dict(seeds=seeds)
        else:
            ikw = dict(generator=torch.Generator(device=dev).manual_seed(a.seed))
        if a.no_drop:
            ikw['capacity_factor'] = 0
        if a.graph:
            ikw['graph'] = True
        kw = dict(motion=torch.zeros(n, T, C, device=dev), motion_mask=mask,
                  motion_length=torch.tensor(a.motion_length, device=dev).long(), num_intervals=n,
                  motion_metas=[{'text': t} for t in a.text], inference_kwargs=ikw)
        if a.xf_out:
            kw['xf_out'] = torch.from_numpy(np.load(a.xf_out)).float().to(dev)
        elif a.clip_feat:
            kw['clip_feat'] = torch.from_numpy(np.load(a.clip_feat)).float().to(dev)
        elif a.random_condition is not None:
            g = torch.Generator().manual_seed(a.random_condition)
            kw['xf_out'] = torch.nn.functional.layer_norm(torch.randn(n, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],)).to(dev)
        out = model(**kw)
    os.makedirs(a.out, exist_ok=True)
    if dims.get('dataset', 'motionx') == 'motionx':
        pred = torch.stack([o['pred_motion'] for o in out]).to(dev).contiguous()
        post = postprocess.postprocess_smplx_stitched(pred, a.motion_length, mean, std)          # what save_smplx_npz writes
        path = os.path.join(a.out, postprocess.result_name(a.text[0], a.motion_length[0]) + '.npz')
        np.savez(path, **postprocess.smplx_npz_dict(post))
        if a.smplx_model:
            from motioncraft_amd.body_model import SMPLXBodyModel
            body = SMPLXBodyModel.from_npz(a.smplx_model)
            if a.joints_npy:
                np.save(a.joints_npy, postprocess.smplx_joints(post, body).cpu().numpy())
            if a.verts_npy:
                np.save(a.verts_npy, postprocess.smplx_vertices(post, body).cpu().numpy())
            if a.render_dir or a.render_avi:
                if body.faces.shape[0] == 0:
                    raise ValueError(f'{a.smplx_model} holds no faces (key f): nothing to draw')
                renderer = render.MeshRenderer(body.faces, body.num_vertices, width=render_size[0], height=render_size[1])
                frames = postprocess.smplx_render(post, body, renderer)
                if a.render_dir:
                    paths, mp4 = render.save_frames(frames, a.render_dir, a.render_fps, postprocess.result_name(a.text[0], a.motion_length[0]))
                    print(f'rendered {len(paths)} frames -> {a.render_dir}' + (f', {mp4}' if mp4 else ' (no ffmpeg on PATH: frames only)'))
                if a.render_avi:
                    size = video.save_avi(frames, a.render_avi, a.render_fps, quality=a.avi_quality)
                    print(f'rendered {frames.shape[0]} frames -> {a.render_avi} ({size} bytes)')
    else:
        arrs = [o['pred_motion'][:m].numpy() * (std if std is not None else 1.0) + (mean if mean is not None else 0.0)
                for o, m in zip(out, a.motion_length)]
        path = os.path.join(a.out, postprocess.result_name(a.text[0], a.motion_length[0]) + '.npy')
        np.save(path, np.concatenate(arrs, axis=0))
        if a.pose_npy or a.anim_dir or a.anim_avi:
            pred = torch.stack([o['pred_motion'] for o in out]).to(dev).contiguous()
        if a.pose_npy:
            postprocess.save_joints_npy(a.pose_npy, pred, a.motion_length, mean, std)
        if a.anim_dir or a.anim_avi:
            chains = skeleton.KIT_CHAINS if dims['input_feats'] == 251 else skeleton.T2M_CHAINS
            renderer = skeleton.SkeletonRenderer(chains, width=anim_size[0], height=anim_size[1])
            frames = postprocess.t2m_render(pred, a.motion_length, renderer, mean, std)
            if a.anim_dir:
                paths, mp4 = render.save_frames(frames, a.anim_dir, a.anim_fps, postprocess.result_name(a.text[0], a.motion_length[0]))
                print(f'drew {len(paths)} frames -> {a.anim_dir}' + (f', {mp4}' if mp4 else ' (no ffmpeg on PATH: frames only)'))
            if a.anim_avi:
                size = video.save_avi(frames, a.anim_avi, a.anim_fps, quality=a.avi_quality)
                print(f'drew {frames.shape[0]} frames -> {a.anim_avi} ({size} bytes)')
    print(f'pred_motion: {n} x {T} x {C} -> {path}')


if __name__ == '__main__':
    main()

"""Result post-processing + on-disk formats: the 322-d SMPL-X motion and the joint positions
of the HumanML3D / KIT feature vectors.

Mirrors what the reference tools do with ``output[i]['pred_motion']`` on the host
(``tools/visualize.py:217-263``, ``tools/s2g_visualize.py:236-246``, ``tools/s2g_test.py:289-297,431-448``):
de-normalise with the dataset's ``mean.npy`` / ``std.npy``, re-pack the 322 channels into SMPL-X
``poses[165] / expressions[100] / trans[3]``, smooth every channel over time with
``scipy.ndimage.gaussian_filter(sigma, mode="nearest")`` and ``np.savez`` the AMASS-style file.  Here the
arithmetic runs in one HIP kernel (``mc_postprocess_smplx``) on the sampler's output while it is still in HBM;
only the finished arrays cross PCIe.

For ``dataset_name == "human_ml3d"`` the reference tool instead recovers 3-D joint positions from the 263-d features
(``plot_t2m``, ``tools/visualize.py:46-56``: ``recover_from_ric`` of ``mogen/utils/plot_utils.py:40-104``, then the
temporal filter at sigma 2.5) and saves them as ``--pose_npy``: ``recover_joints`` / ``recover_joints_stitched`` /
``save_joints_npy`` (``mc_postprocess_t2m_joints``), also for the 251-d KIT layout.

For the 322-d layout the tools go on through the SMPL-X body model (``tools/s2g_test.py:364-412``): ``smplx_joints`` /
``smplx_vertices`` run ``body_model.SMPLXBodyModel`` (``mc_smplx_*``) on the arrays ``postprocess_smplx[_stitched]`` returns.
"""
import ctypes
import os

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _p, stream as _stream

# per-tool filter widths: (body + jaw, hands, trans, expressions); None = unfiltered
SIGMAS_T2M = (3.5, 3.5, 3.0, 2.0)      # tools/visualize.py:244-246 (whole poses array at 3.5)
SIGMAS_S2G = (3.5, 1.0, 3.5, None)     # tools/s2g_visualize.py:243-245
JOINTS_T2M, JOINTS_KIT = 22, 21        # joints of the 263-d human_ml3d / 251-d kit_ml feature vectors
SIGMA_T2M_JOINTS = 2.5                 # tools/visualize.py:48


def gaussian_taps(sigma, truncate=4.0):
    """The normalised taps scipy.ndimage.gaussian_filter1d correlates with (order 0): radius int(truncate*sigma+.5)."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return radius, w / w.sum()


def _filter_operands(C, mean, std, sigmas, dev):
    mean = np.zeros(C) if mean is None else np.asarray(mean)         # visualize.py:187-190 default: 0 and 1
    std = np.ones(C) if std is None else np.asarray(std)
    if mean.shape != (C,) or std.shape != (C,):
        raise ValueError('mean / std must have shape (322,)')
    stats_f32 = int(mean.dtype == np.float32 and std.dtype == np.float32)
    mean_d = torch.from_numpy(mean.astype(np.float64)).to(dev)
    std_d = torch.from_numpy(std.astype(np.float64)).to(dev)
    taps = np.zeros((4, _lib.POST_MAXTAP), np.float64)
    radius = (ctypes.c_int32 * 4)()
    for g, sg in enumerate(sigmas):
        if sg is None or sg <= 0:
            radius[g] = -1
            continue
        r, w = gaussian_taps(sg)
        if 2 * r + 1 > _lib.POST_MAXTAP:
            raise ValueError(f'sigma={sg} needs {2 * r + 1} taps (max {_lib.POST_MAXTAP})')
        radius[g] = r
        taps[g, :2 * r + 1] = w
    return mean_d, std_d, torch.from_numpy(taps).to(dev), radius, stats_f32


def _check_pred(x):
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3):
        raise ValueError('pred_motion must be a contiguous float32 [B,T,322] tensor in device (HBM) memory')
    if x.shape[2] != 322:
        raise ValueError(f'SMPL-X post-processing expects the 322-d motionx layout, got {x.shape[2]}')




def postprocess_smplx(pred_motion, motion_length=None, mean=None, std=None, sigmas=SIGMAS_T2M):
    """Every sample filtered on its own: pred_motion [B,T,322] fp32 device tensor (normalised sampler output) -> dict of
    device fp64 tensors poses [B,T,165], expressions [B,T,100], trans [B,T,3]; frames >= motion_length[b] are zero.
    (The file the T2M tool saves filters AFTER stitching the intervals: ``postprocess_smplx_stitched``.)"""
    lib = _lib.load(require_gpu=True)
    x = pred_motion
    _check_pred(x)
    B, T, C = x.shape
    dev = x.device
    mean_d, std_d, taps_d, radius, stats_f32 = _filter_operands(C, mean, std, sigmas, dev)
    len_d = None
    if motion_length is not None:
        len_d = torch.as_tensor(motion_length).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        if len_d.numel() != B:
            raise ValueError('motion_length must have one entry per sample')
    poses = torch.empty(B, T, 165, device=dev, dtype=torch.float64)
    expr = torch.empty(B, T, 100, device=dev, dtype=torch.float64)
    trans = torch.empty(B, T, 3, device=dev, dtype=torch.float64)
    _lib.check(lib.mc_postprocess_smplx(_p(x), _p(len_d), _p(mean_d), _p(std_d), _p(taps_d), ctypes.byref(radius), stats_f32,
                                        B, T, C, _p(poses), _p(expr), _p(trans),
                                        _stream()),
               'mc_postprocess_smplx')
    return dict(poses=poses, expressions=expr, trans=trans, stats_f32=bool(stats_f32))


def postprocess_smplx_stitched(pred_motion, motion_length, mean=None, std=None, sigmas=SIGMAS_T2M):
    """tools/visualize.py:216-246 for ``num_intervals`` >= 1: the valid frames ``pred[b, :motion_length[b]]`` of all
    intervals are concatenated FIRST and the Gaussian filter runs over the stitched sequence (the smoothing crosses the
    interval seams; only the two ends of the whole sequence replicate their edge frame).  Returns device fp64 tensors
    poses [sum(len),165], expressions [sum(len),100], trans [sum(len),3]."""
    lib = _lib.load(require_gpu=True)
    x = pred_motion
    _check_pred(x)
    B, T, C = x.shape
    lens = [int(v) for v in torch.as_tensor(motion_length).reshape(-1)]
    if len(lens) != B or any(n < 0 or n > T for n in lens):
        raise ValueError('motion_length must have one entry in [0, T] per interval')
    dev = x.device
    rows = np.concatenate([b * T + np.arange(n, dtype=np.int32) for b, n in enumerate(lens)] or [np.zeros(0, np.int32)])
    n = int(rows.size)
    rows_d = torch.from_numpy(rows.astype(np.int32)).to(dev)
    mean_d, std_d, taps_d, radius, stats_f32 = _filter_operands(C, mean, std, sigmas, dev)
    poses = torch.empty(n, 165, device=dev, dtype=torch.float64)
    expr = torch.empty(n, 100, device=dev, dtype=torch.float64)
    trans = torch.empty(n, 3, device=dev, dtype=torch.float64)
    if n:
        _lib.check(lib.mc_postprocess_smplx_stitched(_p(x), _p(rows_d), n, _p(mean_d), _p(std_d), _p(taps_d),
                                                     ctypes.byref(radius), stats_f32, C, _p(poses), _p(expr), _p(trans),
                                                     _stream()),
                   'mc_postprocess_smplx_stitched')
    return dict(poses=poses, expressions=expr, trans=trans, stats_f32=bool(stats_f32))


def smplx_npz_dict(post):
    """Arrays of the AMASS-style file the tools save (visualize.py:247-256) from ``postprocess_smplx_stitched``: poses
    fp64; expressions / trans keep the dtype numpy would have produced (float32 when mean/std are float32 files)."""
    dt = np.float32 if post['stats_f32'] else np.float64
    return dict(betas=np.zeros(300), poses=post['poses'].cpu().numpy(), expressions=post['expressions'].cpu().numpy().astype(dt),
                trans=post['trans'].cpu().numpy().astype(dt), model='smplx2020', gender='neutral', mocap_frame_rate=30)


def smplx_joints(post, model, betas=None):
    """The 55 SMPL-X joints of every frame of ``post`` (the dict ``postprocess_smplx[_stitched]`` returns) under ``model``
    (``body_model.SMPLXBodyModel``): device fp32 [..., 55, 3].  ``betas`` [nb] or one row per frame; default zeros, as the
    tool saves them (tools/visualize.py:242)."""
    return model.joints(post['poses'], post['expressions'], post['trans'], betas)


def smplx_vertices(post, model, betas=None, return_joints=False):
    """The skinned SMPL-X vertices of every frame of ``post``: device fp32 [..., V, 3] (``model.faces`` indexes them)."""
    return model.vertices(post['poses'], post['expressions'], post['trans'], betas, return_joints=return_joints)


def smplx_render(post, body, renderer, betas=None, work_bytes=None):
    """The frames of ``post`` under ``body`` drawn by ``renderer`` (``render.MeshRenderer`` over ``body.faces``): device uint8
    [frames, H, W, 3], what the reference's tools hand to ffmpeg (fast_render.py:63-81).  The vertices never leave the device."""
    verts = smplx_vertices(post, body, betas)
    verts = verts.reshape(-1, body.num_vertices, 3)
    return renderer.render(verts) if work_bytes is None else renderer.render(verts, work_bytes=work_bytes)


def result_name(text, motion_length):
    """visualize.py:247: 'res_' + caption with '/', ' ' -> '_' and '.' removed + '_<length>'."""
    return 'res_' + text.replace('/', '_').replace(' ', '_').replace('.', '') + f'_{int(motion_length)}'


def save_smplx_npz(save_path, text, pred_motion, motion_length, mean=None, std=None, sigmas=SIGMAS_T2M):
    post = postprocess_smplx_stitched(pred_motion, motion_length, mean, std, sigmas)
    d = smplx_npz_dict(post)
    lens = torch.as_tensor(motion_length).reshape(-1)
    path = os.path.join(save_path, result_name(text, lens[0]) + '.npz')
    np.savez(path, **d)
    return path


def _joint_feats(J):
    return 4 + 9 * (J - 1) + 3 * J + 4          # root (4) + ric + rot6d (J - 1 joints) + velocities (J) + foot contacts (4)


def _joints_operands(x, motion_length, mean, std, joints_num, sigma):
    """Argument checks of the joint recovery + the host-side operands; everything here runs before the library is
    loaded, and the device check comes last so that every other message can be reached with a host tensor."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 3):
        raise ValueError('pred_motion must be a [B,T,C] tensor')
    if x.dtype != torch.float32:
        raise ValueError(f'pred_motion must be float32, got {x.dtype}')
    B, T, C = x.shape
    by_feats = {_joint_feats(JOINTS_T2M): JOINTS_T2M, _joint_feats(JOINTS_KIT): JOINTS_KIT}
    if C not in by_feats:
        raise ValueError(f'joint recovery expects the 263-d human_ml3d or the 251-d kit_ml layout, got {C}')
    if joints_num is not None and int(joints_num) != by_feats[C]:
        raise ValueError(f'joints_num={joints_num} contradicts the {C}-d layout ({by_feats[C]} joints)')
    mean = np.zeros(C) if mean is None else np.asarray(mean)
    std = np.ones(C) if std is None else np.asarray(std)
    if mean.shape != (C,) or std.shape != (C,):
        raise ValueError(f'mean / std must have shape ({C},)')
    lens = None
    if motion_length is not None:
        lens = [int(v) for v in torch.as_tensor(motion_length).reshape(-1)]
        if len(lens) != B or any(n < 0 or n > T for n in lens):
            raise ValueError(f'motion_length must have one entry in [0, {T}] per sample')
    taps, radius = np.zeros(_lib.POST_MAXTAP, np.float64), -1
    if sigma is not None and sigma > 0:
        radius, w = gaussian_taps(sigma)
        if 2 * radius + 1 > _lib.POST_MAXTAP:
            raise ValueError(f'sigma={sigma} needs {2 * radius + 1} taps (max {_lib.POST_MAXTAP})')
        taps[:2 * radius + 1] = w
    if not (x.is_cuda and x.is_contiguous()):
        raise ValueError('pred_motion must be a contiguous tensor in device (HBM) memory')
    stats_f32 = int(mean.dtype == np.float32 and std.dtype == np.float32)
    return by_feats[C], lens, mean.astype(np.float64), std.astype(np.float64), taps, radius, stats_f32


def recover_joints(pred_motion, motion_length=None, mean=None, std=None, joints_num=None, sigma=SIGMA_T2M_JOINTS):
    """Every sample on its own: pred_motion [B,T,263|251] fp32 device tensor (normalised sampler output) -> device fp32
    joint positions [B,T,J,3] (J = 22 | 21) of ``pred[b, :motion_length[b]]``, filtered over time at ``sigma`` (None =
    unfiltered); frames >= motion_length[b] are zero."""
    x = pred_motion
    J, lens, mean, std, taps, radius, stats_f32 = _joints_operands(x, motion_length, mean, std, joints_num, sigma)
    B, T, C = x.shape
    lib = _lib.load(require_gpu=True)
    dev = x.device
    to_dev = lambda a: torch.from_numpy(a).to(dev)
    mean_d, std_d, taps_d = to_dev(mean), to_dev(std), to_dev(taps)
    len_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    joints = torch.empty(B, T, J, 3, device=dev, dtype=torch.float32)
    _lib.check(lib.mc_postprocess_t2m_joints(_p(x), _p(len_d), _p(mean_d), _p(std_d), _p(taps_d), radius, stats_f32, B, T, C, J,
                                             _p(joints), _stream()),
               'mc_postprocess_t2m_joints')
    return joints


def recover_joints_stitched(pred_motion, motion_length, mean=None, std=None, joints_num=None, sigma=SIGMA_T2M_JOINTS):
    """tools/visualize.py:217-232 + plot_t2m: the valid frames ``pred[b, :motion_length[b]]`` of all intervals are
    concatenated FIRST; yaw, root position and the filter then run over the stitched sequence, so the motion carries
    across the seams.  Returns the device fp32 tensor [sum(motion_length), J, 3]."""
    x = pred_motion
    if motion_length is None:
        raise ValueError('the stitched form needs the motion_length of every interval')
    J, lens, mean, std, taps, radius, stats_f32 = _joints_operands(x, motion_length, mean, std, joints_num, sigma)
    B, T, C = x.shape
    lib = _lib.load(require_gpu=True)
    dev = x.device
    rows = np.concatenate([b * T + np.arange(n, dtype=np.int32) for b, n in enumerate(lens)] or [np.zeros(0, np.int32)])
    n = int(rows.size)
    joints = torch.empty(n, J, 3, device=dev, dtype=torch.float32)
    if n:
        to_dev = lambda a: torch.from_numpy(a).to(dev)
        rows_d, mean_d, std_d, taps_d = to_dev(rows.astype(np.int32)), to_dev(mean), to_dev(std), to_dev(taps)
        work = torch.empty(n, 4, device=dev, dtype=torch.float64)
        _lib.check(lib.mc_postprocess_t2m_joints_stitched(_p(x), _p(rows_d), n, _p(mean_d), _p(std_d), _p(taps_d), radius, stats_f32,
                                                          C, J, _p(work), _p(joints),
                                                          _stream()),
                   'mc_postprocess_t2m_joints_stitched')
    return joints


def t2m_render(pred_motion, motion_length, renderer, mean=None, std=None, joints_num=None, sigma=SIGMA_T2M_JOINTS, work_bytes=None):
    """``plot_t2m`` (tools/visualize.py:46-56) on the device: ``recover_joints_stitched``, then ``renderer``
    (``skeleton.SkeletonRenderer``) draws ONE animation over the concatenated intervals, as ``plot_3d_motion`` does: device uint8
    [sum(motion_length), H, W, 3].  The joints never leave the device."""
    joints = recover_joints_stitched(pred_motion, motion_length, mean, std, joints_num, sigma)
    return renderer.render(joints) if work_bytes is None else renderer.render(joints, work_bytes=work_bytes)


def save_joints_npy(path, pred_motion, motion_length, mean=None, std=None, joints_num=None, sigma=SIGMA_T2M_JOINTS):
    """The --pose_npy file of the reference tool (visualize.py:55-56): stitched, filtered joints [sum(len), J, 3] fp32."""
    joints = recover_joints_stitched(pred_motion, motion_length, mean, std, joints_num, sigma)
    np.save(path, joints.cpu().numpy())
    return path

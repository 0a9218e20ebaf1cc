"""Joint positions recovered from HumanML3D (263-d) / KIT (251-d) samples on the device: ``postprocess.recover_joints`` /
``recover_joints_stitched`` / ``save_joints_npy`` and ``tools/sample.py --pose_npy`` (mc_postprocess_t2m_joints).

Yardstick: ``tests/golden/t2m_joints.npz``, written by ``tests/golden/make_golden_joints.py`` from the reference's own
``recover_from_ric`` (mogen/utils/plot_utils.py:91-104) + ``scipy.ndimage.gaussian_filter`` as ``plot_t2m`` applies it
(tools/visualize.py:46-48).  Each case carries ``spread`` = max |reference in fp32 - reference in fp64|.

Bounds.  The golden is an fp32 evaluation that sits within ``spread`` of the exact result.
  * the fp64 numpy restatement below, rounded to fp32: 2 x spread (spread + its own output rounding);
  * the device result (fp64 arithmetic from the same fp32-rounded features, one fp32 rounding at the store): 4 x spread
    (spread + the output rounding at joint magnitudes of a few units + sin / cos differing in the last place);
  * device vs the un-rounded fp64 restatement, where no golden exists (edge lengths): one fp32 ulp at the largest
    magnitude of the case (half an ulp of output rounding; fp64 scan-order and libm differences are ~1e-15).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import HML_SMALL, load
from motioncraft_amd import postprocess as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
T = 196
CASES = ('hml_f32', 'hml_f64', 'kit_f32', 'hml_stitched', 'hml_raw')


def feats(J):
    return 4 + 9 * (J - 1) + 3 * J + 4


def golden_case(tag):
    g = load('t2m_joints.npz')
    J, lens = int(g[f'{tag}.joints_num']), [int(n) for n in g[f'{tag}.lengths']]
    pred = np.random.RandomState(int(g[f'{tag}.seed'])).randn(len(lens), T, feats(J)).astype(np.float32)
    sigma = float(g[f'{tag}.sigma']) or None
    return dict(J=J, lens=lens, pred=pred, mean=g[f'{tag}.mean'], std=g[f'{tag}.std'], joints=g[f'{tag}.joints'],
                spread=float(g[f'{tag}.spread']), sigma=sigma, stitched=bool(g[f'{tag}.stitched']))


def restated_joints(pred_seq, mean, std, J, sigma):
    """Steps 1-6 of the recipe on one sequence [n, C] in plain fp64 numpy; returns fp64 [n, J, 3] (not yet rounded)."""
    data = (pred_seq * std + mean).astype(np.float32).astype(np.float64)    # numpy's own dtype rules, then the fp32 rounding point
    n = data.shape[0]
    ang = np.concatenate([[0.0], np.cumsum(data[:-1, 0])])
    c, s = np.cos(ang), np.sin(ang)

    def rot(x, z, c, s):                  # v + 2 (w (u x v) + u x (u x v)) for the conjugate quaternion (w, u) = (c, (0, -s, 0))
        ux, uz = -s * z, s * x            # u x v, y component 0
        return x + 2 * (c * ux - s * uz), z + 2 * (c * uz + s * ux)
    v = np.zeros((n, 2))
    v[1:] = data[:-1, 1:3]
    vx, vz = rot(v[:, 0], v[:, 1], c, s)
    X, Z = np.cumsum(vx), np.cumsum(vz)
    out = np.zeros((n, J, 3))
    out[:, 0] = np.stack([X, data[:, 3], Z], axis=1)
    p = data[:, 4:4 + 3 * (J - 1)].reshape(n, J - 1, 3)
    px, pz = rot(p[..., 0], p[..., 2], c[:, None], s[:, None])
    out[:, 1:, 0], out[:, 1:, 1], out[:, 1:, 2] = px + X[:, None], p[..., 1], pz + Z[:, None]
    if sigma is not None:
        r, w = P.gaussian_taps(sigma)
        idx = np.clip(np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :], 0, n - 1)       # mode="nearest"
        out = np.einsum('tkjc,k->tjc', out[idx], w)
    return out


def restated_case(c):
    seqs = [c['pred'][b, :n] for b, n in enumerate(c['lens'])]
    if c['stitched']:
        seqs = [np.concatenate(seqs, axis=0)]
    return np.concatenate([restated_joints(s, c['mean'], c['std'], c['J'], c['sigma']) for s in seqs if len(s)], axis=0)


# ---- without a GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', CASES)
def test_numpy_restatement_reproduces_the_reference_golden(tag):
    c = golden_case(tag)
    assert c['joints'].dtype == np.float32 and c['joints'].shape == (sum(c['lens']), c['J'], 3)
    err = float(np.abs(restated_case(c).astype(np.float32).astype(np.float64) - c['joints']).max())
    print(f'{tag}: |restatement - reference| {err:.3e}  spread {c["spread"]:.3e}')
    assert 0 < c['spread'] < 1e-5
    assert err <= 2 * c['spread']


def test_fixture_covers_the_layouts_and_modes():
    cs = {t: golden_case(t) for t in CASES}
    assert cs['hml_f32']['mean'].dtype == np.float32 and cs['hml_f64']['mean'].dtype == np.float64
    assert cs['kit_f32']['J'] == P.JOINTS_KIT == 21 and cs['hml_f32']['J'] == P.JOINTS_T2M == 22
    assert cs['hml_stitched']['stitched'] and cs['hml_stitched']['lens'] == [196, 80, 40]
    assert cs['hml_raw']['sigma'] is None and cs['hml_f32']['sigma'] == P.SIGMA_T2M_JOINTS == 2.5
    assert cs['hml_f32']['lens'] == [196, 120, 16]


def test_wrappers_reject_bad_arguments_before_the_library_loads():
    ok = torch.zeros(2, 8, 263)
    for fn in (P.recover_joints, P.recover_joints_stitched):
        with pytest.raises(ValueError, match='device'):
            fn(ok, [8, 8])                                                   # host tensor
        with pytest.raises(ValueError, match='float32'):
            fn(ok.double(), [8, 8])
        with pytest.raises(ValueError, match='263-d human_ml3d or the 251-d kit_ml'):
            fn(torch.zeros(2, 8, 322), [8, 8])
        with pytest.raises(ValueError, match='contradicts'):
            fn(ok, [8, 8], joints_num=21)
        with pytest.raises(ValueError, match='contradicts'):
            fn(torch.zeros(2, 8, 251), [8, 8], joints_num=22)
        with pytest.raises(ValueError, match='motion_length'):
            fn(ok, [8, 9])
        with pytest.raises(ValueError, match='motion_length'):
            fn(ok, [-1, 8])
        with pytest.raises(ValueError, match='motion_length'):
            fn(ok, [8])
        with pytest.raises(ValueError, match='mean / std'):
            fn(ok, [8, 8], mean=np.zeros(251), std=np.ones(251))
        with pytest.raises(ValueError, match=r'\[B,T,C\]'):
            fn(torch.zeros(8, 263), [8])
    with pytest.raises(ValueError, match='motion_length'):
        P.recover_joints_stitched(ok, None)
    with pytest.raises(ValueError, match='device'):
        P.save_joints_npy('unused.npy', ok, [8, 8])


def test_sample_tool_lists_pose_npy():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--pose_npy' in r.stdout


# ---- on the MI355X, through the C-ABI -------------------------------------------------------------------------------------
def device_case(c):
    """The case through the public wrappers; returns (valid frames concatenated [sum(len), J, 3], full per-sample output or None)."""
    x = torch.from_numpy(c['pred']).cuda()
    if c['stitched']:
        return P.recover_joints_stitched(x, c['lens'], c['mean'], c['std'], sigma=c['sigma']).cpu().numpy(), None
    full = P.recover_joints(x, c['lens'], c['mean'], c['std'], sigma=c['sigma']).cpu().numpy()
    return np.concatenate([full[b, :n] for b, n in enumerate(c['lens'])], axis=0), full


@pytest.mark.gpu
@pytest.mark.parametrize('tag', CASES)
def test_device_joints_vs_reference_golden(tag):
    c = golden_case(tag)
    got, full = device_case(c)
    assert got.dtype == np.float32 and got.shape == c['joints'].shape
    err = float(np.abs(got.astype(np.float64) - c['joints']).max())
    err64 = float(np.abs(got.astype(np.float64) - restated_case(c)).max())
    print(f'{tag}: |hip - reference| {err:.3e}  bound {4 * c["spread"]:.3e}  |hip - fp64 restatement| {err64:.3e}  max|joint| {np.abs(got).max():.2f}')
    assert err <= 4 * c['spread']
    if full is not None:
        assert full.shape == (len(c['lens']), T, c['J'], 3)
        for b, n in enumerate(c['lens']):
            assert not full[b, n:].any(), b                                  # frames >= length are exactly zero


@pytest.mark.gpu
def test_device_joints_edge_lengths():
    """length 1, lengths below the filter radius (10 at sigma 2.5), length 0, and motion_length=None (= T)."""
    c = golden_case('hml_f32')
    lens = [1, 5, 0]
    x = torch.from_numpy(c['pred']).cuda()
    full = P.recover_joints(x, lens, c['mean'], c['std']).cpu().numpy()
    ulp = 2.0 ** -23
    for b, n in enumerate(lens):
        assert not full[b, n:].any()
        if n:
            want = restated_joints(c['pred'][b, :n], c['mean'], c['std'], 22, 2.5)
            err = float(np.abs(full[b, :n] - want).max())
            print(f'length {n}: |hip - fp64 restatement| {err:.3e}')
            assert err <= ulp * max(1.0, np.abs(want).max())
    want1 = restated_joints(c['pred'][0, :1], c['mean'], c['std'], 22, None)
    assert np.abs(full[0, :1] - want1).max() <= ulp * max(1.0, np.abs(want1).max())    # one frame: the filter is the identity
    st = P.recover_joints_stitched(x, lens, c['mean'], c['std']).cpu().numpy()
    want = restated_joints(np.concatenate([c['pred'][0, :1], c['pred'][1, :5]]), c['mean'], c['std'], 22, 2.5)
    assert st.shape == (6, 22, 3) and np.abs(st - want).max() <= ulp * max(1.0, np.abs(want).max())
    assert P.recover_joints_stitched(x, [0, 0, 0], c['mean'], c['std']).shape == (0, 22, 3)
    k = golden_case('kit_f32')
    xk = torch.from_numpy(k['pred']).cuda()
    whole = P.recover_joints(xk, None, k['mean'], k['std'], joints_num=21).cpu().numpy()
    same = P.recover_joints(xk, [T, T], k['mean'], k['std']).cpu().numpy()
    assert whole.shape == (2, T, 21, 3) and np.array_equal(whole, same)
    assert np.array_equal(whole[0], P.recover_joints(xk, k['lens'], k['mean'], k['std']).cpu().numpy()[0])   # lens[0] == T


@pytest.mark.gpu
def test_stitched_scans_carry_across_the_seams():
    c = golden_case('hml_stitched')
    x = torch.from_numpy(c['pred']).cuda()
    per = P.recover_joints(x, c['lens'], c['mean'], c['std']).cpu().numpy()
    st = P.recover_joints_stitched(x, c['lens'], c['mean'], c['std']).cpu().numpy()
    n0, n1 = c['lens'][0], c['lens'][1]
    r, _ = P.gaussian_taps(2.5)
    ulp = 2.0 ** -23 * max(1.0, np.abs(st).max())
    # first interval, out of the filter's reach from the seam: same scans, same taps
    assert np.abs(st[:n0 - r] - per[0, :n0 - r]).max() <= ulp
    # within reach of the seam the stitched filter sees the next interval instead of a replicated edge frame
    assert np.abs(st[n0 - r:n0] - per[0, n0 - r:n0]).max() > 100 * ulp
    # after the seam the yaw and the root position continue from the end of the first interval
    gap = float(np.abs(st[n0:n0 + n1] - per[1, :n1]).max())
    root_gap = float(np.abs(st[n0 + r, 0] - per[1, r, 0]).max())
    print(f'stitched vs per-sample after the first seam: max {gap:.3f}, root at seam + radius {root_gap:.3f}')
    assert gap > 1e-2 and root_gap > 1e-3
    # the root height is not a scan: away from the seams it is the same track
    assert np.abs(st[n0 + r:n0 + n1 - r, 0, 1] - per[1, r:n1 - r, 0, 1]).max() <= ulp


@pytest.mark.gpu
def test_device_joints_bit_identical_on_a_side_stream_and_twice():
    for tag in ('hml_f32', 'hml_stitched'):
        c = golden_case(tag)
        first, _ = device_case(c)
        again, _ = device_case(c)
        assert np.array_equal(first, again), tag
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other, _ = device_case(c)
        side.synchronize()
        assert np.array_equal(first, other), tag


@pytest.mark.gpu
def test_sample_tool_writes_pose_npy(tmp_path):
    """tools/sample.py in a child process: reduced human_ml3d config (the dims of the 8-part layout test), synthetic checkpoint,
    two intervals, --pose_npy: fp32 [sum(length), 22, 3] equal to recover_joints_stitched on the same pred_motion; the feature
    .npy stays what it was; a motionx config refuses the flag."""
    from motioncraft_amd import synthetic
    schedule = dict(beta_scheduler='linear', diffusion_steps=1000, model_mean_type='start_x', model_var_type='fixed_large')
    model = dict(type='MotionDiffusion', model=synthetic.reference_model_cfg(HML_SMALL),
                 loss_recon=dict(type='MSELoss', loss_weight=1, reduction='none'), diffusion_train=schedule,
                 diffusion_test=dict(schedule, respace='15,15,8,6,6'), inference_type='ddim', loss_reduction='batch')
    cfg = tmp_path / 'hml_small.py'
    cfg.write_text(f'model = {model!r}\n')
    pose = str(tmp_path / 'joints.npy')
    tool = [sys.executable, os.path.join(ROOT, 'tools', 'sample.py')]
    args = ['synthetic:3', '--random-condition', '5', '--out', str(tmp_path), '--text', 'a person walks', 'a dancer spins',
            '--motion_length', '24', '18', '--pose_npy', pose]
    r = subprocess.run(tool + [str(cfg)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    feat = np.load(os.path.join(str(tmp_path), 'res_a_person_walks_24.npy'))
    assert feat.shape == (42, 263) and feat.dtype == np.float32 and np.isfinite(feat).all()
    joints = np.load(pose)
    assert joints.shape == (42, 22, 3) and joints.dtype == np.float32 and np.isfinite(joints).all()
    pred = torch.zeros(2, 24, 263)
    pred[0], pred[1, :18] = torch.from_numpy(feat[:24]), torch.from_numpy(feat[24:])       # no --mean / --std: features = pred_motion
    assert np.array_equal(joints, P.recover_joints_stitched(pred.cuda(), [24, 18]).cpu().numpy())
    r = subprocess.run(tool + [os.path.join(HERE, 'configs', 'stmogen_small.py')] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and '--pose_npy' in r.stderr and 'motionx' in r.stderr

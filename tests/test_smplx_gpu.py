"""On the MI355X: ``body_model.SMPLXBodyModel`` (``mc_smplx_*``) against the numpy restatement ``smplx_lbs_ref.py`` on
synthetic model files with the published file's keys (SMPL-X package parity is unpinned: DESIGN.md section 2).

Bounds.
  * joints: the kernel is fp64 inside with one rounding at the fp32 store, so it is held to 4 x the restatement's own
    fp32-vs-fp64 spread of the case, the unit and margin of ``test_t2m_joints.py``.  Measured (MI355X): 0.10 .. 0.63 x spread
    over the nine cases (|hip - fp64 restatement| 3.0e-8 .. 1.9e-7 at joint magnitudes up to 4.2).
  * vertices: per element, the fp64 restatement +- the forward bound of an fp32 sum in arbitrary order,
    (K + 64) 2^-24 sum |leaves| (``smplx_lbs_ref.lbs_bound``); it holds for any k-order the GEMM picks.  Measured:
    0.0034 / 0.0039 / 0.0024 of the bound (V = 1031 per-call betas / per-frame betas / V = 10 475), i.e. 1.17 / 1.00 /
    1.02 x the fp32 restatement's own spread.
  * ``joints_out`` of the vertices call: bit for bit the joints call (the same kernel writes both).
  * a chunked run (small ``work_bytes``, frames not a multiple of the chunk): bit for bit the unchunked run.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import smplx_lbs_ref as ref
from motioncraft_amd import lib as L
from motioncraft_amd import postprocess as P
from motioncraft_amd.body_model import SMPLXBodyModel

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NB = 20


@pytest.fixture(scope='module')
def small():
    arrays = ref.synthetic_model(V=1031, shape_space=NB, seed=11)
    model = SMPLXBodyModel.from_npz(arrays, num_betas=NB)
    yield arrays, model
    model.close()


def inputs(n, seed, per_frame_betas=False, zero_rot=False, near_pi=False):
    rs = np.random.RandomState(seed)
    poses = ref.random_poses(n, seed + 1)
    if zero_rot:
        poses[:] = 0.0
    if near_pi:
        d = rs.randn(n, 55, 3)
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        poses = (d * (np.pi - 10.0 ** rs.uniform(-6, -3, (n, 55, 1)))).reshape(n, 165)
    return dict(poses=poses, expr=rs.randn(n, 100), trans=rs.randn(n, 3), betas=rs.randn(n, NB) if per_frame_betas else rs.randn(NB))


JOINT_CASES = {
    'n1_call': dict(n=1, seed=20), 'n1_frame': dict(n=1, seed=21, per_frame_betas=True),
    'n7_call': dict(n=7, seed=22), 'n7_frame': dict(n=7, seed=23, per_frame_betas=True),
    'n588_call': dict(n=588, seed=24), 'n588_frame': dict(n=588, seed=25, per_frame_betas=True),
    'n7_null_expr_trans': dict(n=7, seed=26), 'zero_rotations': dict(n=1, seed=27, zero_rot=True), 'near_pi': dict(n=1, seed=28, near_pi=True),
}


@pytest.mark.parametrize('tag', tuple(JOINT_CASES))
def test_device_joints_vs_fp64_restatement(small, tag):
    arrays, model = small
    x = inputs(**JOINT_CASES[tag])
    if tag == 'n7_null_expr_trans':
        x['expr'] = x['trans'] = None
    j64, _ = ref.lbs(arrays, x['poses'], x['expr'], x['trans'], x['betas'], nb=NB, vertices=False)
    j32, _ = ref.lbs(arrays, x['poses'], x['expr'], x['trans'], x['betas'], nb=NB, vertices=False, dtype=np.float32)
    spread = float(np.abs(j32.astype(np.float64) - j64).max())
    assert 0 < spread < 1e-4, spread                                  # the unit of the bound exists for this case
    got = model.joints(torch.from_numpy(x['poses']).cuda(), x['expr'], x['trans'], x['betas'])          # device tensor and numpy inputs
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (x['poses'].shape[0], 55, 3)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - j64).max())
    print(f'{tag}: |hip - fp64 restatement| {err:.3e}  spread {spread:.3e}  ratio {err / spread:.2f}  max|joint| {np.abs(j64).max():.2f}')
    assert err <= 4 * spread


def check_vertices(arrays, model, x, nb, work_bytes, tag):
    exact, bound = ref.lbs_bound(arrays, x['poses'], x['expr'], x['trans'], x['betas'], nb=nb)
    _, v32 = ref.lbs(arrays, x['poses'], x['expr'], x['trans'], x['betas'], nb=nb, dtype=np.float32)
    spread = float(np.abs(v32.astype(np.float64) - exact).max())
    verts, joints = model.vertices(x['poses'], x['expr'], x['trans'], x['betas'], return_joints=True, work_bytes=work_bytes)
    assert verts.dtype == torch.float32 and tuple(verts.shape) == exact.shape
    err = np.abs(verts.cpu().numpy().astype(np.float64) - exact)
    print(f'{tag}: |hip - fp64 restatement| {err.max():.3e}  measured / bound {float((err / bound).max()):.4f}  '
          f'measured / fp32 spread {err.max() / spread:.2f}  (spread {spread:.3e}, smallest bound {bound.min():.3e})')
    assert spread > 0 and (bound > 0).all()
    assert (err <= bound).all()
    assert torch.equal(joints, model.joints(x['poses'], x['expr'], x['trans'], x['betas']))       # bit for bit: one kernel writes both
    return verts


@pytest.mark.parametrize('per_frame', (False, True))
def test_device_vertices_within_the_forward_bound_and_chunking_is_exact(small, per_frame):
    arrays, model = small
    n = 37
    x = inputs(n, seed=40 + per_frame, per_frame_betas=per_frame)
    obj = model.native()
    chunk8 = int(obj.lib.mc_smplx_work_bytes(obj.handle, 8, int(per_frame)))
    assert chunk8 < int(obj.lib.mc_smplx_work_bytes(obj.handle, n, int(per_frame)))
    whole = check_vertices(arrays, model, x, NB, 1 << 30, f'V=1031 n={n} betas {"per frame" if per_frame else "per call"}')
    chunked = model.vertices(x['poses'], x['expr'], x['trans'], x['betas'], work_bytes=chunk8)       # 37 = 4 x 8 + 5
    assert torch.equal(whole, chunked)
    one = model.vertices(x['poses'], x['expr'], x['trans'], x['betas'], work_bytes=1)               # raised to one frame's need
    assert torch.equal(whole, one)
    lead = model.vertices(x['poses'][:36].reshape(4, 9, 165), x['expr'][:36].reshape(4, 9, 100), x['trans'][:36].reshape(4, 9, 3),
                          x['betas'][:36].reshape(4, 9, NB) if per_frame else x['betas'])
    assert tuple(lead.shape) == (4, 9, 1031, 3) and torch.equal(lead.reshape(36, 1031, 3), whole[:36])


def test_device_vertices_at_the_published_size():
    """V = 10 475 with all 300 betas, once; 11 frames in chunks of 4."""
    arrays = ref.synthetic_model(V=10475, shape_space=300, seed=12)
    model = SMPLXBodyModel.from_npz(arrays)
    rs = np.random.RandomState(50)
    x = dict(poses=ref.random_poses(11, 51), expr=rs.randn(11, 100), trans=rs.randn(11, 3), betas=rs.randn(300))
    obj = model.native()
    whole = check_vertices(arrays, model, x, 300, 1 << 30, 'V=10475 n=11 nb=300')
    chunked = model.vertices(x['poses'], x['expr'], x['trans'], x['betas'], work_bytes=int(obj.lib.mc_smplx_work_bytes(obj.handle, 4, 0)))
    assert torch.equal(whole, chunked)
    model.close()


def test_any_number_of_skin_weights_per_vertex():
    """1 .. 20 nonzero weights per vertex: wider than the register kernels' 16, so the any-width skinning kernel runs."""
    arrays = ref.synthetic_model(V=1031, shape_space=NB, seed=14, max_nz=20)
    assert (arrays['weights'] != 0).sum(1).max() == 20
    model = SMPLXBodyModel.from_npz(arrays, num_betas=NB)
    x = inputs(13, seed=60)
    obj = model.native()
    whole = check_vertices(arrays, model, x, NB, 1 << 30, 'V=1031 n=13, up to 20 weights per vertex')
    assert torch.equal(whole, model.vertices(x['poses'], x['expr'], x['trans'], x['betas'],
                                             work_bytes=int(obj.lib.mc_smplx_work_bytes(obj.handle, 5, 0))))
    model.close()


def test_mean_hand_pose_is_added_unless_flat(small):
    """hands_meanl / hands_meanr of the file: the model adds them to the hand joints of every pose (the package's
    flat_hand_mean=False), i.e. it gives what the mean-free model gives on poses + mean."""
    arrays, flat = small
    rs = np.random.RandomState(70)
    mean = np.zeros(165)
    mean[75:] = 0.2 * rs.randn(90)
    model = SMPLXBodyModel.from_npz(dict(arrays, hands_meanl=mean[75:120], hands_meanr=mean[120:165]), num_betas=NB)
    x = inputs(5, seed=71)
    got = model.joints(x['poses'], x['expr'], x['trans'], x['betas'])
    assert torch.equal(got, flat.joints(x['poses'] + mean, x['expr'], x['trans'], x['betas']))
    assert (got - flat.joints(x['poses'], x['expr'], x['trans'], x['betas'])).abs().max() > 1e-3
    assert torch.equal(got[:, :20], flat.joints(x['poses'], x['expr'], x['trans'], x['betas'])[:, :20])       # only below the wrists
    off = SMPLXBodyModel.from_npz(dict(arrays, hands_meanl=mean[75:120], hands_meanr=mean[120:165]), num_betas=NB, flat_hand_mean=True)
    assert torch.equal(off.joints(x['poses']), flat.joints(x['poses']))
    model.close(), off.close()


def test_native_object_checks(small):
    arrays, model = small
    cfg = L.SMPLXConfig(1031, 55, NB, 100, 486)
    import ctypes
    o = L.NativeObject('smplx', ctypes.byref(cfg))
    bad = dict(model.params, parents=model.params['parents'].copy())
    bad['parents'][7] = 9
    o.upload(bad.items())
    with pytest.raises(RuntimeError, match=r'mc_smplx_finalize failed \(code 1\).*parents\[7\] = 9.*topologically ordered'):
        o.finalize()
    x = torch.zeros(1, 165, dtype=torch.float64, device='cuda')
    b = torch.zeros(NB, dtype=torch.float64, device='cuda')
    out = torch.empty(1, 55, 3, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert o.lib.mc_smplx_joints(o.handle, p(x), None, None, p(b), 0, 1, p(out), None) != L.MC_OK and 'not finalized' in L.last_error()
    o.upload([('parents', model.params['parents'][:-1])])
    with pytest.raises(RuntimeError, match=r"code 3\): SMPL-X body model: parameter 'parents' has 54 elements, expected 55"):
        o.finalize()
    o.upload(model.params.items())
    o.finalize()
    assert o.lib.mc_smplx_joints(o.handle, p(x), None, None, p(b), 0, 1, p(out), None) == L.MC_OK, L.last_error()
    assert torch.equal(out, model.joints(x, betas=b))
    o.close()
    with pytest.raises(RuntimeError, match=r'mc_smplx_create failed \(code 1\)'):
        L.NativeObject('smplx', ctypes.byref(L.SMPLXConfig(1031, 24, NB, 100, 207)))


def test_sample_tool_writes_the_smplx_joints(tmp_path):
    """tools/sample.py in a child process on the small motionx config: --smplx_model + --joints_npy + --verts_npy write what the
    wrappers give on the arrays of the .npz the same run saved."""
    arrays = ref.synthetic_model(V=1031, shape_space=300, seed=13)
    mpath = str(tmp_path / 'model.npz')
    np.savez(mpath, **arrays)
    jpath, vpath = str(tmp_path / 'joints.npy'), str(tmp_path / 'verts.npy')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'sample.py'), os.path.join(HERE, 'configs', 'stmogen_small.py'), 'synthetic:3',
           '--random-condition', '5', '--out', str(tmp_path), '--text', 'a person walks', 'a dancer spins', '--motion_length', '24', '18',
           '--smplx_model', mpath, '--joints_npy', jpath, '--verts_npy', vpath]
    r = subprocess.run(['timeout', '-k', '10', '280'] + cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(os.path.join(str(tmp_path), 'res_a_person_walks_24.npz'))
    joints, verts = np.load(jpath), np.load(vpath)
    assert joints.shape == (42, 55, 3) and joints.dtype == np.float32 and np.isfinite(joints).all()
    assert verts.shape == (42, 1031, 3) and verts.dtype == np.float32 and np.isfinite(verts).all()
    model = SMPLXBodyModel.from_npz(mpath)
    post = dict(poses=torch.from_numpy(z['poses']).cuda(), expressions=torch.from_numpy(z['expressions']).cuda(),
                trans=torch.from_numpy(z['trans']).cuda())
    assert z['poses'].dtype == np.float64 and z['expressions'].dtype == np.float64            # no --mean / --std: nothing was rounded on the way
    assert np.array_equal(joints, P.smplx_joints(post, model).cpu().numpy())
    assert np.array_equal(verts, P.smplx_vertices(post, model).cpu().numpy())
    j64, _ = ref.lbs(arrays, z['poses'], z['expressions'], z['trans'], np.zeros(300), nb=300, vertices=False)
    assert np.abs(joints - j64).max() <= 2.0 ** -22 * max(1.0, np.abs(j64).max())
    model.close()
    r = subprocess.run(['timeout', '-k', '10', '280', sys.executable, os.path.join(ROOT, 'tools', 'sample.py'), '--help'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and '--smplx_model' in r.stdout and '--joints_npy' in r.stdout and '--verts_npy' in r.stdout

"""Without a GPU: the SMPL-X body model's C-ABI symbols, the loader's checks, and the numpy restatement the device is held to.

SMPL-X package parity is unpinned: the package and its model file are not available, so the yardstick
is ``smplx_lbs_ref.py``, the published algorithm in numpy.  What CAN be tied to the reference is tied here: the restatement's
Rodrigues against the reference's own ``axis_angle_to_matrix`` and ``evaluation.L1div`` against the reference's ``L1div``
(``tests/golden/smplx_rot.npz``, written by ``make_golden_smplx.py``).  The restatement is also checked against two
identities that need no reference: the rest pose and a rigid motion of the root.
"""
import ctypes

import numpy as np
import pytest

import smplx_lbs_ref as ref
from helpers import load
from motioncraft_amd import lib as L

NEW_SYMBOLS = ('mc_smplx_create', 'mc_smplx_destroy', 'mc_smplx_set_param', 'mc_smplx_finalize', 'mc_smplx_joints', 'mc_smplx_work_bytes',
               'mc_smplx_vertices')


def test_library_exports_the_body_model_symbols():
    lib = L.load(require_gpu=False)
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert 'smplx' in L.NATIVE_OBJECTS and ctypes.sizeof(L.SMPLXConfig) == 5 * 4


def test_loader_refuses_a_bad_model_file():
    from motioncraft_amd.body_model import SMPLXBodyModel
    good = ref.synthetic_model(V=64, shape_space=20, seed=1)
    SMPLXBodyModel.from_npz(good, num_betas=20)
    bad = dict(good, kintree_table=good['kintree_table'].copy())
    bad['kintree_table'][0, 7] = 9                                   # a joint below a later one
    with pytest.raises(ValueError, match=r'parents\[7\] = 9.*topologically ordered'):
        SMPLXBodyModel.from_npz(bad, num_betas=20)
    with pytest.raises(ValueError, match=r'posedirs must be \[64, 3, 486\]'):
        SMPLXBodyModel.from_npz(dict(good, posedirs=good['posedirs'][:, :, :477]), num_betas=20)
    with pytest.raises(ValueError, match='num_betas=21: the file has 20 shape directions'):
        SMPLXBodyModel.from_npz(good, num_betas=21)
    with pytest.raises(ValueError, match='num_betas=300: the file has 20 shape directions'):
        SMPLXBodyModel.from_npz(good)                                # the default asks for the published file's 300
    with pytest.raises(ValueError, match='num_expression_coeffs=101'):
        SMPLXBodyModel.from_npz(good, num_betas=20, num_expression_coeffs=101)


def test_loader_takes_both_layouts_of_the_expression_directions(tmp_path):
    from motioncraft_amd.body_model import SMPLXBodyModel
    wide = ref.synthetic_model(V=64, shape_space=20, seed=1)
    split = ref.synthetic_model(V=64, shape_space=20, seed=1, expr_key=True)
    assert wide['shapedirs'].shape == (64, 3, 120) and split['shapedirs'].shape == (64, 3, 20) and split['expr_dirs'].shape == (64, 3, 100)
    a = SMPLXBodyModel.from_npz(wide, num_betas=10, num_expression_coeffs=50)
    b = SMPLXBodyModel.from_npz(split, num_betas=10, num_expression_coeffs=50)
    assert a.params.keys() == b.params.keys()
    for k in a.params:
        assert a.params[k].dtype == np.float32 and np.array_equal(a.params[k], b.params[k]), k
    assert a.params['shapedirs'].shape == (64, 3, 10) and a.params['expr_dirs'].shape == (64, 3, 50)
    assert np.array_equal(a.params['expr_dirs'], wide['shapedirs'][:, :, 20:70].astype(np.float32))
    assert a.params['parents'][0] == -1 and np.array_equal(a.params['parents'][1:], ref.PARENTS[1:])
    assert a.faces.shape == (128, 3) and a.faces.dtype == np.int64
    path = tmp_path / 'model.npz'                                     # the same through a file
    np.savez(path, **wide)
    c = SMPLXBodyModel.from_npz(str(path), num_betas=10, num_expression_coeffs=50)
    assert all(np.array_equal(a.params[k], c.params[k]) for k in a.params)


def test_loader_reads_a_file_with_the_published_files_other_entries(tmp_path):
    """The published SMPLX_*.npz also holds landmark tables, hand components and PICKLED 0-d object entries (joint2num,
    part2num: name -> index dicts), which is why the package opens it with allow_pickle=True.  The loader reads only its own
    keys, so such a file loads without unpickling anything, and the mean hand pose is picked up unless flat_hand_mean."""
    from motioncraft_amd.body_model import SMPLXBodyModel
    m = ref.synthetic_model(V=64, shape_space=20, seed=1)
    rs = np.random.RandomState(2)
    meanl, meanr = 0.1 * rs.randn(45), 0.1 * rs.randn(45)
    extra = dict(hands_meanl=meanl, hands_meanr=meanr, hands_componentsl=rs.randn(45, 45), hands_componentsr=rs.randn(45, 45),
                 lmk_faces_idx=rs.randint(0, 128, 51), lmk_bary_coords=rs.rand(51, 3), dynamic_lmk_faces_idx=rs.randint(0, 128, (79, 17)),
                 dynamic_lmk_bary_coords=rs.rand(79, 17, 3), vt=rs.rand(70, 2), ft=rs.randint(0, 70, (128, 3)),
                 joint2num=np.array({'Pelvis': 0, 'L_Hip': 1}, dtype=object), part2num=np.array({'Global': 0}, dtype=object))
    path = str(tmp_path / 'published_like.npz')
    np.savez(path, **m, **extra)
    with np.load(path, allow_pickle=False) as z:
        with pytest.raises(ValueError, match='allow_pickle=False'):
            z['joint2num']                                            # the file really holds an entry that needs pickle
    a = SMPLXBodyModel.from_npz(path, num_betas=20)
    plain = SMPLXBodyModel.from_npz(m, num_betas=20)
    assert all(np.array_equal(a.params[k], plain.params[k]) for k in plain.params) and np.array_equal(a.faces, plain.faces)
    assert not plain.pose_mean.any()                                  # a file without hands_mean*: nothing to add
    assert np.array_equal(a.pose_mean[75:120], meanl) and np.array_equal(a.pose_mean[120:165], meanr) and not a.pose_mean[:75].any()
    assert not SMPLXBodyModel.from_npz(path, num_betas=20, flat_hand_mean=True).pose_mean.any()
    np.savez(str(tmp_path / 'other.npz'), v_template=m['v_template'])
    with pytest.raises(ValueError, match='not an SMPL-X model file, missing'):
        SMPLXBodyModel.from_npz(str(tmp_path / 'other.npz'))


def test_restated_rodrigues_vs_the_reference_conversion():
    g = load('smplx_rot.npz')
    aa, angle, want = g['rot.axis_angle'], g['rot.angle'], g['rot.matrix']
    assert angle[angle > 0].min() == 1e-6 and abs(angle.max() - (np.pi - 1e-6)) < 1e-12 and (angle == 0).sum() == 4
    err = np.abs(ref.rodrigues(aa) - want).reshape(len(aa), -1).max(1)
    big = angle >= 1e-4
    print(f'|restatement - reference|: {err[big].max():.3e} at angles >= 1e-4, {err[~big].max():.3e} below')
    assert big.sum() > 150 and (~big).sum() > 40
    assert err[big].max() <= 1e-7
    assert err[~big].max() <= 2e-8                                   # the two published forms differ by the 1e-8 offset there
    assert np.array_equal(ref.rodrigues(np.zeros((2, 3))), np.broadcast_to(np.eye(3), (2, 3, 3)))


def test_l1div_vs_the_reference_metric():
    from motioncraft_amd.evaluation import L1div
    g = load('smplx_rot.npz')
    calc = L1div()
    for i in range(int(g['l1div.count'])):
        j = g[f'l1div.joints{i}']
        before = j.copy()
        calc.run(j)
        assert np.array_equal(j, before)                             # the reference's run overwrites its argument; this one does not
        want = float(g[f'l1div.avg_after{i}'])
        print(f'L1div after sequence {i}: {float(calc.avg())!r}  reference {want!r}')
        assert abs(float(calc.avg()) - want) <= 2.0 ** -22 * want      # the same fp32 sums: a few ulp at most
    calc.reset()
    assert calc.counter == 0 and calc.sum == 0


def test_rest_pose_gives_back_the_template():
    m = ref.synthetic_model(V=257, shape_space=20, seed=3)
    vt, _, _, _, jr, _, _ = ref.model_arrays(m, 20, 100)
    joints, verts = ref.lbs(m, np.zeros((2, 165)), np.zeros((2, 100)), np.zeros((2, 3)), np.zeros(20), nb=20)
    # a zero rotation is exactly the identity in the published form (direction 0 / 1.7e-8 = 0), so every A_j is [I | 0]; the skin
    # weights are held in fp32 like the package's, so a vertex's weights sum to 1 within 2^-24 and not exactly
    assert np.abs(verts - vt).max() <= 2.0 ** -23 * np.abs(vt).max()
    assert np.abs(joints - jr @ vt).max() <= 1e-15


def test_rotating_the_root_moves_the_body_rigidly():
    m = ref.synthetic_model(V=257, shape_space=20, seed=4)
    rs = np.random.RandomState(5)
    poses = ref.random_poses(3, seed=6)
    expr, trans, betas = rs.randn(3, 100), rs.randn(3, 3), rs.randn(20)
    q = np.array([0.3, -1.1, 0.6])
    Q = ref.rodrigues(q)
    R0 = ref.rodrigues(poses[:, :3])
    QR = Q @ R0                                                       # the new global_orient as a matrix -> back to axis-angle
    ang = np.arccos(np.clip((np.trace(QR, axis1=1, axis2=2) - 1) / 2, -1, 1))
    axis = np.stack([QR[:, 2, 1] - QR[:, 1, 2], QR[:, 0, 2] - QR[:, 2, 0], QR[:, 1, 0] - QR[:, 0, 1]], 1) / (2 * np.sin(ang))[:, None]
    moved = poses.copy()
    moved[:, :3] = axis * ang[:, None]
    j0, v0 = ref.lbs(m, poses, expr, trans, betas, nb=20)
    j1, v1 = ref.lbs(m, moved, expr, trans, betas, nb=20)
    root = j0[:, :1] - trans[:, None]                                 # J_0: rotations turn about it, the translation comes after
    want_j = (j0 - trans[:, None] - root) @ Q.T + root + trans[:, None]
    want_v = (v0 - trans[:, None] - root) @ Q.T + root + trans[:, None]
    print(f'rigid motion: joints {np.abs(j1 - want_j).max():.2e}  vertices {np.abs(v1 - want_v).max():.2e}')
    assert np.abs(j1 - want_j).max() <= 1e-6 and np.abs(v1 - want_v).max() <= 1e-6     # the 1e-8 offset of the angle, times a few
    assert np.abs(j1 - j0).max() > 0.1


def test_fp32_restatement_sits_at_fp32_distance_from_fp64():
    m = ref.synthetic_model(V=257, shape_space=20, seed=7)
    poses = ref.random_poses(5, seed=8)
    j64, v64 = ref.lbs(m, poses, nb=20)
    j32, v32 = ref.lbs(m, poses, nb=20, dtype=np.float32)
    assert j32.dtype == np.float32 and v32.dtype == np.float32
    _, bound = ref.lbs_bound(m, poses, nb=20)
    sj, sv = float(np.abs(j32 - j64).max()), float((np.abs(v32 - v64) / bound).max())
    print(f'fp32 vs fp64 restatement: joints {sj:.3e}, vertices at most {sv:.3f} of the forward bound')
    assert 0 < sj < 1e-5 and 0 < sv < 1

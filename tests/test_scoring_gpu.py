"""On the MI355X: ``motioncraft_amd.scoring`` -- the beat alignment (``mc_beat_mask`` / ``mc_beat_align``), the face vertex
errors (``mc_smplx_vertex_errors``) and the two scorers.

Bounds.
  * beat masks: EQUAL to the reference's sets of ``tests/golden/s2g_scoring.npz`` and, at the shapes that stress the kernel's
    frame tiles, to the numpy restatement of ``test_scoring_host.py``; every input keeps a relative margin >= 1e-4 on each
    decision (asserted), so a difference is a defect and not a rounding.
  * align score: 1e-12 absolute (each term lies in [0, 1] and carries a few ulp of the fp64 ``exp``; means do not amplify it).
  * vertex error sums vs the same two expressions evaluated in numpy from the device's own ``vertices()`` (fp32 element
    operations, fp64 sums): 1e-12 relative -- only the order of the fp64 sum differs.
  * ``l2`` / ``lvel`` vs the float64 restatement: a bound derived below from ``smplx_lbs_ref.lbs_bound`` (``face_error_bounds``).
  * chunked runs, repeated runs: bit for bit.
"""
import numpy as np
import pytest
import torch

import smplx_lbs_ref as ref
import test_scoring_host as H
from helpers import EVAL_DIMS
from motioncraft_amd import scoring as S
from motioncraft_amd.body_model import SMPLXBodyModel
from motioncraft_amd.evaluation import L1div
from oracle import weights as W

pytestmark = pytest.mark.gpu

NB = 20
TF = 256                                     # slice frames per workgroup of beat_mask_k (csrc/mc_metrics.hip)
# tag: (frames, t_start, t_end, seed, mean_vel dtype); the seeds were searched on the CPU for a margin >= 1e-4 (asserted below)
STRESS = {
    'slice_of_1': (40, 10, 11, 0, np.float32),
    'slice_of_2': (40, 10, 12, 0, np.float64),
    'slice_of_3': (40, 10, 13, 0, np.float32),
    'three_tiles_plus_1_start_below_order': (800, 5, 5 + 3 * TF + 1, 10, np.float32),
    'three_tiles_minus_1': (800, 20, 20 + 3 * TF - 1, 10, np.float64),
}
NO_BEAT_JOINT = 12                           # an upper-body joint whose mean_vel is raised until no speed passes the threshold


def stress_inputs(tag):
    T, t0, t1, seed, dtype = STRESS[tag]
    joints, mv = H.synthetic_joints(T, 5000 + seed)
    mv[NO_BEAT_JOINT] *= 1e3
    rs = np.random.RandomState(seed + 1)
    span = (t1 - t0) / 30
    onsets = np.concatenate([np.sort(rs.uniform(0, span, 9)), [span + 5.0]])          # the last one lies beyond every beat
    return joints, mv.astype(dtype), t0, t1, onsets


def run_device(al, joints, t0, t1, onsets):
    beats = al.load_pose(torch.from_numpy(joints).cuda(), t0, t1, 30)
    assert beats.mask.is_cuda and beats.mask.dtype == torch.uint8 and tuple(beats.mask.shape) == (55, t1 - t0)
    return beats, al.calculate_align(onsets, beats, 30)


def test_beats_and_scores_equal_the_reference_fixture():
    _, cases = H.golden_cases()
    for tag, joints, mean_vel, t0, t1, want_beats, scores in cases:
        al = S.BeatAlignment(0.3, 7, mean_vel)
        beats, _ = run_device(al, joints, t0, t1, scores[9][0])
        want = H.masks_of(want_beats, t1 - t0)
        got = beats.mask.cpu().numpy()
        assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:8])
        assert all(np.array_equal(a, b) for a, b in zip(beats.lists(), want_beats))
        for n_on, (onsets, ref_score) in scores.items():
            have = al.calculate_align(onsets, beats, 30)
            one_call, again = al.score(joints, t0, t1, 30, onsets, return_beats=True)
            print(f'{tag} onsets {n_on}: score {have!r}  reference {ref_score!r}  |diff| {abs(have - ref_score):.1e}')
            assert abs(have - ref_score) <= 1e-12
            assert one_call == have and torch.equal(again.mask, beats.mask)              # two runs: the same bits


@pytest.mark.parametrize('tag', tuple(STRESS))
def test_beats_at_the_tile_edges_equal_the_restatement(tag):
    joints, mv, t0, t1, onsets = stress_inputs(tag)
    want_beats, margin = H.beat_sets(H.speeds(joints, 30, mv), t0, t1, 7)
    print(f'{tag}: {sum(len(b) for b in want_beats)} beats, margin {margin:.2e}')
    assert margin >= H.MARGIN
    assert len(want_beats[NO_BEAT_JOINT]) == 0 and NO_BEAT_JOINT in H.UPPER
    al = S.BeatAlignment(0.3, 7, mv)
    beats, score = run_device(al, joints, t0, t1, onsets)
    want = H.masks_of(want_beats, t1 - t0)
    got = beats.mask.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    last = max((int(b[-1]) for j, b in enumerate(want_beats) if j in H.UPPER and len(b)), default=-1)
    assert onsets[-1] > (last + 1) / 30
    want_score = H.align_score(want_beats, onsets, 30, 0.3)
    print(f'{tag}: score {score!r}  restatement {want_score!r}')
    assert abs(score - want_score) <= 1e-12
    if t1 - t0 > 2 * TF:
        assert want[:, TF - 8:TF + 8].any() and want[:, 2 * TF - 8:2 * TF + 8].any()                       # beats sit at the tile seams
        assert 0 < score < 1
    beats2, score2 = run_device(al, joints, t0, t1, onsets)
    assert torch.equal(beats2.mask, beats.mask) and score2 == score


# ---- face errors ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    arrays = ref.synthetic_model(V=1031, shape_space=NB, seed=11)
    model = SMPLXBodyModel.from_npz(arrays, num_betas=NB)
    yield arrays, model
    model.close()


def face_inputs(n, seed, nb=NB):
    rs = np.random.RandomState(seed)
    rec_pose, tar_pose = ref.random_poses(n, seed + 1), ref.random_poses(n, seed + 2)
    return dict(rec_pose=rec_pose, rec_exp=rs.randn(n, 100), tar_pose=tar_pose, tar_exp=rs.randn(n, 100), betas=rs.randn(n, nb),
                rec_trans=rs.randn(n, 3), tar_trans=rs.randn(n, 3))


def numpy_sums(va, vb):
    """The two sums from fp32 vertex arrays: fp32 element operations, float64 sums."""
    assert va.dtype == np.float32 and vb.dtype == np.float32
    d = va - vb
    e = (va[1:] - vb[:-1]) - (vb[1:] - vb[:-1])
    assert d.dtype == np.float32 and e.dtype == np.float32
    return float((d * d).astype(np.float64).sum()), float(np.abs(e).astype(np.float64).sum())


def check_sums_vs_own_vertices(model, x, tag, **kw):
    a = (x['rec_pose'], x['rec_exp'], x['rec_trans'])
    b = (x['tar_pose'], x['tar_exp'], x['tar_trans'])
    sums = model.vertex_error_sums(*a, *b, x['betas'], **kw)
    assert sums.is_cuda and sums.dtype == torch.float64 and tuple(sums.shape) == (2,)
    want = numpy_sums(model.vertices(*a, x['betas']).cpu().numpy(), model.vertices(*b, x['betas']).cpu().numpy())
    got = sums.tolist()
    rel = [abs(g - w) / w for g, w in zip(got, want)]
    print(f'{tag}: sums {got}  from the device vertices in numpy {list(want)}  relative {rel[0]:.1e} {rel[1]:.1e}')
    assert want[0] > 0 and want[1] > 0 and max(rel) <= 1e-12
    return sums


def test_vertex_error_sums_vs_the_devices_own_vertices_and_chunking_is_exact(small):
    arrays, model = small
    x = face_inputs(7, seed=80)
    whole = check_sums_vs_own_vertices(model, x, 'V=1031 n=7 per-frame betas', work_bytes=1 << 30)
    obj = model.native()
    a = (x['rec_pose'], x['rec_exp'], x['rec_trans'], x['tar_pose'], x['tar_exp'], x['tar_trans'], x['betas'])
    sizes = [int(obj.lib.mc_smplx_vertex_errors_work_bytes(obj.handle, c, 7, 1)) for c in (2, 3, 7)]
    assert sizes[0] < sizes[1] < sizes[2]
    for wb in sizes + [1]:                                              # 7 = 2 + 2 + 2 + 1 = 3 + 3 + 1; 1 is raised to one frame's need
        assert torch.equal(model.vertex_error_sums(*a, work_bytes=wb), whole), wb
    per_call = dict(x, betas=x['betas'][0])
    check_sums_vs_own_vertices(model, per_call, 'V=1031 n=7 per-call betas', work_bytes=sizes[0])
    one = model.vertex_error_sums(*(t[:1] for t in a))                  # one frame: no frame pair
    assert one[1].item() == 0.0 and one[0].item() > 0


def face_error_bounds(arrays, x, nb):
    """(l2, lvel, bound on l2, bound on lvel) of the jaw-and-expression-only calls in float64.  With the exact vertices A, B and the
    device's a = A + da, b = B + db, |da| <= Ba, |db| <= Bb per element (``lbs_bound``), and u = 2^-24 per fp32 operation:
      d = fl(a - b):            |d - D| <= Dd := Ba + Bb + u (|D| + Ba + Bb),  D = A - B
      fl(d d):                  |fl(d d) - D^2| <= Dd (2 |D| + Dd) + u (|D| + Dd)^2
      p = fl(a1 - b0), q = fl(b1 - b0):   |p - (A1 - B0)| <= P := Ba1 + Bb0 + u (|A1 - B0| + Ba1 + Bb0), Q likewise with B1
      e = fl(p - q):            ||e| - |E|| <= P + Q + u (|E| + P + Q),  E = (A1 - B0) - (B1 - B0)
    by the triangle inequality; the float64 sums add at most N 2^-53 relative (N < 2^20 nonnegative terms), taken as 2^-33."""
    u = 2.0 ** -24

    def jaw_only(p):
        z = np.zeros_like(p)
        z[:, 66:69] = p[:, 66:69]
        return z
    A, Ba = ref.lbs_bound(arrays, jaw_only(x['rec_pose']), x['rec_exp'], None, x['betas'], nb=nb)
    B, Bb = ref.lbs_bound(arrays, jaw_only(x['tar_pose']), x['tar_exp'], None, x['betas'], nb=nb)
    D = np.abs(A - B)
    Dd = Ba + Bb + u * (D + Ba + Bb)
    l2 = float((D * D).mean())
    l2_bound = float((Dd * (2 * D + Dd) + u * (D + Dd) ** 2).mean()) + 2.0 ** -33 * l2
    p, q = np.abs(A[1:] - B[:-1]), np.abs(B[1:] - B[:-1])
    P = Ba[1:] + Bb[:-1] + u * (p + Ba[1:] + Bb[:-1])
    Q = Bb[1:] + Bb[:-1] + u * (q + Bb[1:] + Bb[:-1])
    E = np.abs((A[1:] - B[:-1]) - (B[1:] - B[:-1]))
    lvel = float(E.mean())
    lvel_bound = float((P + Q + u * (E + P + Q)).mean()) + 2.0 ** -33 * lvel
    return l2, lvel, l2_bound, lvel_bound


def test_face_errors_within_the_bound_derived_from_the_vertex_bound(small):
    arrays, model = small
    x = face_inputs(7, seed=81)
    l2, lvel = S.face_errors(model, x['rec_pose'], x['rec_exp'], x['tar_pose'], x['tar_exp'], x['betas'])
    want_l2, want_lvel, b2, bv = face_error_bounds(arrays, x, NB)
    print(f'l2 {l2!r} exact {want_l2!r}: measured / bound {abs(l2 - want_l2) / b2:.3e}   '
          f'lvel {lvel!r} exact {want_lvel!r}: measured / bound {abs(lvel - want_lvel) / bv:.3e}')
    assert want_l2 > 0 and want_lvel > 0 and b2 > 0 and bv > 0
    assert abs(l2 - want_l2) <= b2 and abs(lvel - want_lvel) <= bv
    # the operands are the zeroed ones: body, hands and eyes of the inputs do not matter, jaw and expressions do
    moved = dict(x, rec_pose=x['rec_pose'].copy())
    moved['rec_pose'][:, :66] += 1.0
    moved['rec_pose'][:, 69:] -= 1.0
    assert S.face_errors(model, moved['rec_pose'], x['rec_exp'], x['tar_pose'], x['tar_exp'], x['betas']) == (l2, lvel)
    jaw = dict(x, rec_pose=x['rec_pose'].copy())
    jaw['rec_pose'][:, 66:69] += 0.1
    assert S.face_errors(model, jaw['rec_pose'], x['rec_exp'], x['tar_pose'], x['tar_exp'], x['betas'])[0] != l2
    with pytest.raises(ValueError, match='at least 2 frames'):          # lvel over zero frame pairs
        S.face_errors(model, x['rec_pose'][:1], x['rec_exp'][:1], x['tar_pose'][:1], x['tar_exp'][:1], x['betas'][:1])


def test_vertex_error_sums_at_the_published_size():
    """V = 10 475 with all 300 betas per frame, 5 frames, whole and in chunks of 2."""
    arrays = ref.synthetic_model(V=10475, shape_space=300, seed=12)
    model = SMPLXBodyModel.from_npz(arrays)
    x = face_inputs(5, seed=82, nb=300)
    whole = check_sums_vs_own_vertices(model, x, 'V=10475 n=5 nb=300', work_bytes=1 << 30)
    obj = model.native()
    chunked = model.vertex_error_sums(x['rec_pose'], x['rec_exp'], x['rec_trans'], x['tar_pose'], x['tar_exp'], x['tar_trans'], x['betas'],
                                      work_bytes=int(obj.lib.mc_smplx_vertex_errors_work_bytes(obj.handle, 2, 5, 1)))
    assert torch.equal(whole, chunked)
    model.close()


# ---- scorers -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def evaluator():
    import motioncraft_amd as mc
    sd = W.make_eval_encoder_state(W.eval_encoder_param_shapes(**EVAL_DIMS), seed=8)
    enc_cfg = {k: v for k, v in EVAL_DIMS.items() if k != 'nfeats'}
    model = mc.build_submodule(dict(type='T2MContrastiveModel_SMPLX', motion_encoder=dict(nfeats=EVAL_DIMS['nfeats'], vae=True, **enc_cfg),
                                    state_dict=sd))
    yield model
    model.encoder.close()


def embed(evaluator, motion):
    m = torch.as_tensor(motion).float().cuda()[None]
    return evaluator.encode_motion(m, torch.tensor([m.shape[1]]).cuda()).cpu().numpy()


def s2g_sequence(T, seed):
    g = torch.Generator().manual_seed(seed)
    rec_motion = 0.3 * torch.randn(T, 322, generator=g)
    joints, _ = H.synthetic_joints(T, seed)                             # smooth channels, so that the joints have beats
    rec_motion[:, :66] = 0.5 * torch.from_numpy(joints.reshape(T, 165)[:, :66])
    rs = np.random.RandomState(seed)
    return dict(rec_motion=rec_motion, tar_pose=0.3 * torch.randn(T, 165, generator=g), tar_exps=torch.randn(T, 100, generator=g),
                tar_trans=torch.randn(T, 3, generator=g), tar_beta=torch.randn(T, 300, generator=g),
                onset_times=np.sort(rs.uniform(0, (T - 120) / 30, 7)))


def test_s2g_scorer_assembles_the_separately_tested_pieces(small, evaluator):
    _, body = small
    mean_vel = np.full(55, 0.5, np.float32)
    sc = S.S2GScorer(body, evaluator, mean_vel, align_mask=60)
    al, l1 = S.BeatAlignment(0.3, 7, mean_vel), L1div()
    l2_all = lvel_all = align = 0.0
    total = 0
    emb = dict(pred=[], gt=[], hand_pred=[], hand_gt=[])
    for T, seed in ((150, 90), (131, 91)):
        q = s2g_sequence(T, seed)
        per_seq = sc.add_sequence(**q)
        rec_pose, rec_exp, rec_trans = S.unpack_rec_motion(q['rec_motion'])
        joints = body.joints(rec_pose, None, None, q['tar_beta'])
        l2, lvel = S.face_errors(body, rec_pose, rec_exp, q['tar_pose'], q['tar_exps'], q['tar_beta'])
        score = al.score(joints, 60, T - 60, 30, q['onset_times'])
        assert per_seq == dict(l2=l2, lvel=lvel, align=score)
        l2_all, lvel_all, align, total = l2_all + l2 * T, lvel_all + lvel * T, align + score * (T - 120), total + T
        l1.run(joints.reshape(T, 165))
        emb['pred'].append(embed(evaluator, q['rec_motion']))
        emb['gt'].append(embed(evaluator, S.pack_motion(q['tar_pose'], q['tar_exps'], q['tar_trans'])))
        emb['hand_pred'].append(embed(evaluator, S.hand_only_motion(rec_pose, rec_trans)))
        emb['hand_gt'].append(embed(evaluator, S.hand_only_motion(q['tar_pose'], q['tar_trans'])))
    cat = {k: np.concatenate(v) for k, v in emb.items()}
    want = {'l2 loss': l2_all / total, 'lvel loss': lvel_all / total, 'align score': align / (total - 2 * 2 * 60), 'l1div score': l1.avg(),
            'FID(Whole Body) score': S._fid(cat['gt'], cat['pred']), 'FID (Hands) score': S._fid(cat['hand_gt'], cat['hand_pred'])}
    got = sc.summary()
    print(got)
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k] and np.isfinite(got[k]), k
    assert got['l2 loss'] > 0 and got['lvel loss'] > 0 and 0 <= got['align score'] <= 1 and got['l1div score'] > 0


def test_m2d_scorer_assembles_the_separately_tested_pieces(evaluator):
    sc = S.M2DScorer(evaluator)
    g = torch.Generator().manual_seed(95)
    emb = dict(pred=[], gt=[], hand_pred=[], hand_gt=[])
    for T in (40, 33, 57, 24):
        rec, gt = torch.randn(T, 322, generator=g), torch.randn(T, 322, generator=g)
        sc.add_sequence(rec, gt)
        emb['pred'].append(embed(evaluator, rec))
        emb['gt'].append(embed(evaluator, gt))
        for k, m in (('hand_pred', rec), ('hand_gt', gt)):
            hand = torch.zeros(T, 322)
            hand[:, 66:156] = m[:, 66:156]
            emb[k].append(embed(evaluator, hand))
    cat = {k: np.concatenate(v) for k, v in emb.items()}
    np.random.seed(5)
    from motioncraft_amd.evaluation import calculate_diversity
    want_div = calculate_diversity(cat['pred'], 3, 1.0, 1.0)
    np.random.seed(5)
    got = sc.summary()
    print(got)
    assert list(got) == ['FID(Whole Body) score', 'FID (Hands) score', 'Diversity score']
    assert got['FID(Whole Body) score'] == S._fid(cat['gt'], cat['pred']) and got['FID (Hands) score'] == S._fid(cat['hand_gt'], cat['hand_pred'])
    assert got['Diversity score'] == want_div and want_div > 0
    with pytest.raises(ValueError, match='the sample holds 10 frames, the ground truth 12'):
        sc.add_sequence(torch.zeros(10, 322), torch.zeros(12, 322))

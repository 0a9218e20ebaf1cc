"""Host side of the skeleton renderer (no GPU): mplot3d's camera pinned to matplotlib itself, the restatement's own properties
(``skeleton_ref.py`` is what the device tests hold the kernels to), the scene's constants, the library's symbols and the argument
errors of ``SkeletonRenderer``."""
import ctypes

import numpy as np
import pytest
import torch

import skeleton_ref as R
import motioncraft_amd as mc
from motioncraft_amd import lib as L
from motioncraft_amd import postprocess
from motioncraft_amd import skeleton as sk


def test_camera_equals_matplotlibs_get_proj():
    """A real Axes3D with the reference's limits and view; ``_box_aspect`` is read back because matplotlib >= 3.9 scales it by
    another 25/24.  1e-12 relative to the largest entry of the matrix."""
    matplotlib = pytest.importorskip('matplotlib')
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    for radius, elev, azim, dist in ((4, 120, -90, 7.5), (4, 120, -90, 10.0), (3, 30, -60, 15.0), (4, -100, 45, 7.5)):
        fig = plt.figure(figsize=(10, 10))
        ax = fig.add_subplot(projection='3d')
        ax.set_xlim3d([-radius / 4, radius / 4]), ax.set_ylim3d([0, radius / 2]), ax.set_zlim3d([0, radius / 2])
        ax.view_init(elev=elev, azim=azim)
        ax._dist = dist
        limits = (ax.get_xlim3d(), ax.get_ylim3d(), ax.get_zlim3d())
        want = ax.get_proj()
        cam = sk.Mplot3dCamera(elev=elev, azim=azim, dist=dist, focal_length=ax._focal_length, radius=radius,
                               box_aspect=tuple(ax._box_aspect), box_scale=None, limits=limits)
        got = cam.proj_matrix64()
        plt.close(fig)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (elev, azim, dist, np.abs(got - want).max())
        # without margins the limits are the ones the camera derives from the radius
        auto = sk.Mplot3dCamera(radius=radius)
        assert np.allclose(auto.limits, [[-radius / 4, radius / 4], [0, radius / 2], [0, radius / 2]], rtol=0, atol=0)


def test_camera_defaults_and_screen_matrix():
    cam = sk.Mplot3dCamera()
    assert (cam.elev, cam.azim, cam.dist, cam.focal_length) == (120.0, -90.0, 7.5, 1.0)
    assert np.isclose(np.linalg.norm(cam.box), 1.8294640721620434, rtol=1e-15) and np.allclose(cam.box / cam.box[0], [1, 1, 0.75])
    assert np.array_equal(cam.view, [-0.095, 0.09, -0.095, 0.09])                     # set_top_view at the initial dist of 10
    m = cam.proj_matrix64()
    for W, H in ((1000, 1000), (96, 64), (37, 23)):
        s64, s32 = cam.screen_projective64(W, H), cam.screen_projective(W, H)
        assert s32.dtype == np.float32 and np.array_equal(s32, s64.astype(np.float32))
        side, rs = min(W, H), np.random.RandomState(1)
        for p in rs.uniform(-1, 1, (20, 3)) + [0, 1, 1]:
            h, q = m @ np.append(p, 1), s64 @ np.append(p, 1)
            tx, ty = h[0] / h[3], h[1] / h[3]
            assert h[3] > 0 and q[3] == h[3]
            assert np.isclose(q[0] / q[3], (W - side) / 2 + side * (tx + 0.095) / 0.185, rtol=0, atol=1e-9)
            assert np.isclose(q[1] / q[3], (H - side) / 2 + side * (1 - (ty + 0.095) / 0.185), rtol=0, atol=1e-9)
    # the motion's height runs up the screen, its x to the right, and the eye is where h_w vanishes
    s = cam.screen_projective64(1000, 1000)
    pix = lambda p: (s @ np.append(p, 1))[:2] / (s @ np.append(p, 1))[3]
    assert pix([0, 1.5, 0])[1] < pix([0, 0.5, 0])[1] and pix([0.5, 1, 0])[0] > pix([-0.5, 1, 0])[0]
    assert 0 < pix([0, 1, 0])[0] < 1000 and 0 < pix([0, 1, 0])[1] < 1000
    assert abs((s @ np.append(R.eye_world(cam), 1))[3]) < 1e-12
    for kw in (dict(dist=0), dict(focal_length=np.inf), dict(view=(0, 0, 0, 1)), dict(box_aspect=(4, 4)), dict(box_scale=-1),
               dict(limits=((0, 0), (0, 1), (0, 1))), dict(elev=np.nan)):
        with pytest.raises(ValueError):
            sk.Mplot3dCamera(**kw)


def brute_distance(a, b, p):
    """fp64 distance from p to the segment a -> b."""
    a, b, p = (np.asarray(v, np.float64) for v in (a, b, p))
    d = b - a
    dd = d @ d
    u = 0.0 if dd == 0 else min(1.0, max(0.0, ((p - a) @ d) / dd))
    return np.linalg.norm(p - (a + u * d))


def test_capsule_rule_equals_the_brute_force_distance():
    rs = np.random.RandomState(7)
    S, total, excluded = 24, 0, 0
    for trial in range(200):
        a, b = np.round(rs.uniform(-4, S + 4, (2, 2)) * 16).astype(np.int64)
        if trial % 10 == 0:
            b = a.copy()                                                     # a disc
        Rr = int(rs.choice([12, 13, 22, 44, 80, 200]))
        mask = R.capsule_mask(a, b, Rr, S, S)
        for y in range(S):
            for x in range(S):
                p = (16 * x + 8, 16 * y + 8)
                dist = brute_distance(a, b, p)
                total += 1
                if abs(dist - Rr) < 16e-6:                                   # within 1e-6 px of the boundary
                    excluded += 1
                    continue
                assert mask[y, x] == (dist < Rr), (trial, x, y, dist, Rr)
                if (x + y + trial) % 7 == 0:
                    assert mask[y, x] == R.capsule_covers(a, b, Rr, p)
    assert excluded < 1e-3 * total, (excluded, total)


def test_capsule_boundaries_are_covered():
    # end cap: e . e == R^2 with t <= 0 (the sample lies behind A)
    a, b, p = (8, 8), (8 - 160, 8), (8 + 48, 8 + 64)
    assert 48 * 48 + 64 * 64 == 80 * 80 and (p[0] - a[0]) * (b[0] - a[0]) < 0
    assert R.capsule_covers(a, b, 80, p) and not R.capsule_covers(a, b, 79, p)
    # side: cross^2 == R^2 dd strictly between the ends
    a, b, p = (8, 8), (168, 8), (88, 88)
    cross, dd, t = 160 * 80, 160 * 160, 80 * 160
    assert cross * cross == 80 * 80 * dd and 0 < t < dd
    assert R.capsule_covers(a, b, 80, p) and not R.capsule_covers(a, b, 79, p)
    # the far cap: |P - B|^2 == R^2
    assert R.capsule_covers((8, 8), (168, 8), 80, (168 + 48, 8 + 64)) and not R.capsule_covers((8, 8), (168, 8), 79, (168 + 48, 8 + 64))
    m = R.capsule_mask((8, 8), (168, 8), 80, 16, 8)
    assert m[5, 5] and m[4, 13] and not m[5, 13] and not m[6, 5] and m[0, 15] and not m[1, 15]
    disc = R.capsule_mask((88, 88), (88, 88), 80, 12, 12)                    # centre of pixel (5, 5), radius 5 px
    assert disc[5, 10] and disc[9, 8] and disc[8, 9] and not disc[9, 9] and not disc[5, 11] and disc.sum() == 81
    # the floor of 12 units keeps a thin capsule connected: every column of a shallow line holds a covered pixel
    thin = R.capsule_mask((3, 5), (16 * 30 + 11, 16 * 7 + 2), 12, 30, 10)
    assert thin.any(axis=0).all()


def test_cross_product_beyond_64_bits_is_decided_without_it():
    a, b = (-R.GUARD, -R.GUARD), (R.GUARD, R.GUARD - 16)
    p = (16 * 4095 + 8, 8)
    dx, dy, ex, ey = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    cross = dx * ey - dy * ex
    assert cross * cross > 2 ** 64 and 0 < ex * dx + ey * dy < dx * dx + dy * dy
    assert 512 * 512 * (dx * dx + dy * dy) < 2 ** 56
    assert not R.capsule_covers(a, b, 512, p)
    # the int64 form agrees with Python integers across the whole guard band, near and far from the line
    rs = np.random.RandomState(3)
    for trial in range(60):
        a, b = rs.randint(-R.GUARD, R.GUARD + 1, (2, 2))
        if trial % 2:
            a, b = np.array([-R.GUARD, -R.GUARD + trial]), np.array([R.GUARD, R.GUARD - 3 * trial])         # through the viewport
        Rr = int(rs.choice([12, 44, 512]))
        W = 64
        m = R.capsule_mask(a, b, Rr, W, W)
        for y in range(0, W, 3):
            for x in range(0, W, 3):
                assert m[y, x] == R.capsule_covers(a, b, Rr, (16 * x + 8, 16 * y + 8))
        if trial % 2:
            assert m.any() and not m.all()


def test_triangles_follow_the_top_left_rule():
    # two triangles of a quad share the diagonal: every sample of the quad exactly once, also with corners on pixel centres
    for c in (np.array([[8, 8], [8, 168], [168, 168], [168, 8]]), np.array([[3, 5], [20, 150], [170, 181], [160, 2]])):
        t0, t1 = R.triangle_mask(c[[0, 1, 2]], 12, 12), R.triangle_mask(c[[0, 2, 3]], 12, 12)
        assert not (t0 & t1).any() and (t0 | t1).any()
        assert np.array_equal(t0, R.triangle_mask(c[[2, 1, 0]], 12, 12))     # no culling: the winding does not matter
    sq = R.triangle_mask([[8, 8], [8, 168], [168, 168]], 12, 12) | R.triangle_mask([[8, 8], [168, 168], [168, 8]], 12, 12)
    assert sq.sum() == 100 and sq[:10, :10].all()                            # top and left edges own their samples, bottom and right do not
    assert not R.triangle_mask([[8, 8], [88, 88], [168, 168]], 12, 12).any()


def walk(n, J=22, seed=0):
    rs = np.random.RandomState(seed)
    j = rs.uniform(-0.4, 0.4, (n, J, 3)).astype(np.float32) + np.array([0, 0.9, 0], np.float32)
    j[:, :, [0, 2]] += np.cumsum(rs.uniform(0.0, 0.05, (n, 1, 2)), axis=0).astype(np.float32)
    return j


def test_scene_trail_starts_at_frame_two_and_layers_take_the_maximum():
    r = sk.SkeletonRenderer(sk.T2M_CHAINS, width=64, height=64)
    j = walk(6)
    out = R.render(j, [6], r.camera.screen_projective(64, 64), r.segments(), r.trail_radius, 64, 64)
    assert [len(t) for t in out['trails']] == [0, 0, 2, 3, 4, 5]
    mins, maxs, traj = R.sequence_stats(j)
    assert np.array_equal(mins, j.min(axis=(0, 1))) and np.array_equal(maxs, j.max(axis=(0, 1))) and np.array_equal(traj, j[:, 0][:, [0, 2]])
    body, trail = R.frame_points(j, 3, mins, maxs)
    assert np.array_equal(body[0], [0, j[3, 0, 1] - mins[1], 0]) and np.array_equal(body[22:, 1], np.zeros(4, np.float32))
    assert np.array_equal(trail[:, 1], np.zeros(3, np.float32)) and np.array_equal(trail[:, 0], j[:3, 0, 0] - j[3, 0, 0])
    assert not (out['layer'][:2] == 2).any() and (out['layer'][2:] == 2).any(axis=(1, 2)).all()
    for lay in out['layer']:
        assert (lay == 1).any() and (lay >= 3).any() and lay.max() <= 3 + 4
    # non-finite values are ignored by MINS / MAXS
    j[2, 5] = [np.nan, np.inf, -np.inf]
    m2, x2, _ = R.sequence_stats(j)
    assert np.isfinite(m2).all() and np.isfinite(x2).all()
    # the layer maximum: a later chain over an earlier one, chains over the trail over the plane
    scr = np.array([[40, 100], [600, 100], [300, 20], [300, 400], [0, 0], [0, 640], [640, 640], [640, 0]])
    lay = R.frame_layers(scr, [[8, 200], [500, 200], [500, 90]], [(0, 1, 44, 3), (2, 3, 22, 4)], 12, 40, 40)
    assert lay[6, 18] == 4 and lay[6, 10] == 3 and lay[12, 10] == 2 and lay[30, 30] == 1 and lay[6, 31] == 3 and lay[9, 31] == 2
    dropped = R.frame_layers(np.where(np.arange(8)[:, None] == 1, R.INVALID, scr), [], [(0, 1, 44, 3), (2, 3, 22, 4)], 12, 40, 40)
    assert not (dropped == 3).any() and (dropped == 4).any()


def test_defaults_follow_the_reference_figure():
    r = sk.SkeletonRenderer(sk.T2M_CHAINS)
    assert (r.width, r.height, r.dpi, r.num_joints) == (1000, 1000, 100.0, 22)
    assert r.palette.tolist() == [[255, 255, 255], [191, 191, 191], [0, 0, 255], [255, 0, 0], [0, 0, 255], [0, 0, 0], [255, 0, 0], [0, 0, 255]]
    assert sk.composite((0.5, 0.5, 0.5), 0.5, (255, 255, 255)) == (191, 191, 191)                 # the plane over white
    assert np.allclose(r.chain_width_px, 4.0 * 100 / 72) and np.isclose(r.trail_width_px, 100 / 72)
    assert r.chain_radius == [44] * 5 and r.trail_radius == 12                                   # floor(8 * 5.556 + 0.5); the floor of 12
    assert sk.line_radius(10.0) == 80 and sk.line_radius(0.1) == 12 and sk.line_radius(64.0) == 512
    for bad in (0, -1, np.nan, 64.1):
        with pytest.raises(ValueError):
            sk.line_radius(bad)
    hands = [[20, 22 + 3 * f, 23 + 3 * f, 24 + 3 * f] for f in range(5)] + [[21, 37 + 3 * f, 38 + 3 * f, 39 + 3 * f] for f in range(5)]
    r52 = sk.SkeletonRenderer(sk.T2M_CHAINS + hands)
    assert r52.num_joints == 52 and r52.chain_radius == [44] * 5 + [22] * 10
    assert r52.palette[8:13].tolist() == [[0, 0, 139]] * 5 and r52.palette[13:18].tolist() == [[139, 0, 0]] * 5
    assert sk.SkeletonRenderer(sk.T2M_CHAINS * 4).palette[3 + 15].tolist() == [255, 0, 0]        # the colours cycle
    assert len(r.segments()) == 21 and r.segments()[0] == (0, 2, 44, 3) and r.segments()[-1][3] == 7


@pytest.mark.parametrize('chains,parents', [(sk.T2M_CHAINS, sk.T2M_PARENTS), (sk.KIT_CHAINS, sk.KIT_PARENTS)])
def test_chains_draw_every_bone_once(chains, parents):
    bones = [(c[k], c[k + 1]) for c in chains for k in range(len(c) - 1)]
    assert sorted(bones) == sorted((p, j) for j, p in enumerate(parents) if p >= 0)            # parent -> child, each bone once
    assert len(chains) == 5 and all(c[0] in (0, chains[2][3]) for c in chains)                 # legs and spine from the root, arms from the chest
    assert [len(c) for c in chains] == ([5, 5, 6, 5, 5] if len(parents) == 22 else [6, 6, 5, 4, 4])


def test_library_exports_the_skeleton_entry_points():
    lib = L.load()
    for name in ('mc_skeleton_create', 'mc_skeleton_destroy', 'mc_skeleton_work_bytes', 'mc_skeleton_frames'):
        assert getattr(lib, name) is not None and name in L.EXPORTED_SYMBOLS
    assert lib.mc_skeleton_work_bytes(None, 1, 1, 64, 64) == -1
    assert ctypes.sizeof(L.SkeletonParams) == 72


def test_package_exports_the_new_names():
    for name in ('skeleton', 'Mplot3dCamera', 'SkeletonRenderer', 'T2M_CHAINS', 'KIT_CHAINS'):
        assert name in mc.__all__ and hasattr(mc, name)
    assert mc.SkeletonRenderer is sk.SkeletonRenderer and callable(postprocess.t2m_render)


def test_renderer_argument_errors():
    for kw in (dict(chains=[]), dict(chains=[[0]]), dict(chains=[[0, -1]]), dict(chains=[[0, 1]] * 62), dict(chains=[[0, 1]], num_joints=1),
               dict(chains=[[0, 1]], width=0), dict(chains=[[0, 1]], height=4097), dict(chains=[[0, 1]], dpi=0),
               dict(chains=[[0, 1]], camera='top'), dict(chains=[[0, 1]], colors=['red', 'blue']), dict(chains=[[0, 1]], colors=['pink']),
               dict(chains=[[0, 1]], widths_pt=[500.0]), dict(chains=[[0, 1]], plane_alpha=2), dict(chains=[[0, 1]], background=(256, 0, 0))):
        with pytest.raises(ValueError):
            sk.SkeletonRenderer(**kw)
    r = sk.SkeletonRenderer(sk.T2M_CHAINS, width=32, height=32)
    for bad, kw in ((np.zeros((2, 22, 3), np.float32), {}), (torch.zeros(2, 22, 3, dtype=torch.float64), {}), (torch.zeros(2, 21, 3), {}),
                    (torch.zeros(4, 22, 3), dict(lengths=[1, 2])), (torch.zeros(4, 22, 3), dict(lengths=[5, -1])),
                    (torch.zeros(4, 22, 3), dict(work_bytes=-1)), (torch.zeros(4, 22, 3), {})):                # the last: host memory
        with pytest.raises(ValueError):
            r.render(bad, **kw)

"""On the MI355X: ``skeleton.SkeletonRenderer`` (``mc_skeleton_*``, csrc/mc_skeleton.hip) against the restatement ``skeleton_ref.py``.

Rules, applied to every case by ``check``:
  * ``stats`` (MINS, MAXS) and ``traj`` equal numpy's fp32 exactly: minima, maxima and copies have no rounding.
  * ``screen`` and ``trail_screen`` are within +-1 unit (1/16 px) of floor(16 * fp64 projection + 0.5) of the same fp32 matrix and the
    same fp32 p', on points with h_w >= 0.1; a point the fp64 projection drops (not finite, h_w <= 0, more than a unit beyond the guard
    band) is dropped, one it keeps a unit inside the band is kept.
  * coverage is exact: the restatement, fed the kernel's OWN ``screen`` and ``trail_screen``, gives the same ``layer`` at every pixel.
    There are no excusable pixels.
  * ``rgb == palette[layer]`` exactly.
"""
import ctypes

import numpy as np
import pytest
import torch

import skeleton_ref as R
from helpers import load
from motioncraft_amd import lib as L
from motioncraft_amd import postprocess as P
from motioncraft_amd import skeleton as sk

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (64, 64), (96, 64)]
HANDS = [[20, 22 + 3 * f, 23 + 3 * f, 24 + 3 * f] for f in range(5)] + [[21, 37 + 3 * f, 38 + 3 * f, 39 + 3 * f] for f in range(5)]
NARROW = dict(view=(-0.001, 0.001, -0.001, 0.001))           # a long lens: 8000 px off the axis is still a small angle


def run(r, joints, lens=None, **kw):
    out = r.render(torch.from_numpy(np.ascontiguousarray(joints, np.float32)).cuda(), lens, return_buffers=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ('rgb', 'layer', 'screen', 'trail_screen', 'stats', 'traj'))


def check_points(got, pts, S, what):
    sx, sy, hw = R.project64(pts, S)
    with np.errstate(invalid='ignore', over='ignore'):
        exact = 16.0 * np.stack([sx, sy], axis=1) + 0.5
        finite = np.isfinite(np.asarray(pts, np.float64)).all(axis=1) & np.isfinite(exact).all(axis=1) & np.isfinite(hw)
        want = np.floor(np.where(finite[:, None], exact, 0))
        inside = finite & (hw >= 0.1) & (np.abs(want) <= R.GUARD - 1).all(axis=1)
        outside = ~finite | (hw <= 0) | ((hw >= 0.1) & (np.abs(want) > R.GUARD + 1).any(axis=1))
    valid = got[:, 0] != R.INVALID
    assert np.array_equal(valid, got[:, 1] != R.INVALID), what
    assert valid[inside].all() and not valid[outside].any(), (what, np.nonzero(inside & ~valid)[0], np.nonzero(outside & valid)[0])
    assert np.abs(got[inside] - want[inside]).max(initial=0) <= 1, (what, np.abs(got[inside] - want[inside]).max())
    return int(inside.sum())


def check(r, out, joints, lens=None):
    """The four rules on one result; returns the restatement's layers (= the device's)."""
    joints = np.ascontiguousarray(joints, np.float32)
    n, W, H = joints.shape[0], r.width, r.height
    lens = [n] if lens is None else lens
    S = r.camera.screen_projective(W, H)
    g = 0
    for s, m in enumerate(lens):
        mins, maxs, traj = R.sequence_stats(joints[g:g + m])
        assert np.array_equal(out['stats'][s], np.concatenate([mins, maxs])), s
        assert np.array_equal(out['traj'][g:g + m], traj, equal_nan=True), s
        for i in range(m):
            body, trail = R.frame_points(joints[g:g + m], i, mins, maxs)
            check_points(out['screen'][g + i], body, S, ('screen', s, i))
            k = len(trail)
            check_points(out['trail_screen'][g + i, :k], trail, S, ('trail', s, i))
            assert (out['trail_screen'][g + i, k:] == R.INVALID).all(), (s, i)
        g += m
    want = R.layers_from_buffers(out['screen'], out['trail_screen'], lens, r.segments(), r.trail_radius, W, H)
    assert out['layer'].shape == (n, H, W) and np.array_equal(out['layer'], want), np.argwhere(out['layer'] != want)[:5]
    assert out['rgb'].shape == (n, H, W, 3) and np.array_equal(out['rgb'], r.palette[out['layer']])
    return want


def walk(n, J=22, seed=0, step=0.05):
    rs = np.random.RandomState(seed)
    j = rs.uniform(-0.4, 0.4, (n, J, 3)).astype(np.float32) + np.array([0, 0.9, 0], np.float32)
    j[:, :, [0, 2]] += np.cumsum(rs.uniform(0.0, step, (n, 1, 2)), axis=0).astype(np.float32)
    return j


def placed(r, pixels, y=0.5):
    """One frame whose joints 1.. land on the pixel positions ``pixels``: the root stands at the origin and joint 0's height 0 is the
    lowest, so p' = p."""
    S = r.camera.screen_projective64(r.width, r.height)
    pts = [np.zeros(3)] + [R.unproject(S, sx, sy, y) for sx, sy in pixels]
    return np.asarray(pts, np.float64)[None].astype(np.float32)


def two_bones(size, camera=None, pt=7.2):
    """Chains (1, 2) and (3, 4) of width 10 px at 100 dpi: R = 80 units = 5 px."""
    return sk.SkeletonRenderer([[1, 2], [3, 4]], width=size[0], height=size[1], widths_pt=[pt, pt], camera=camera)


def test_endpoints_on_pixel_centres_put_boundary_pixels_exactly_on_the_circle():
    r = two_bones((64, 64))
    assert r.chain_radius == [80, 80]
    j = placed(r, [(20.5, 30.5), (40.5, 30.5), (50.5, 8.5), (50.5, 8.5)])                    # chain 1 is degenerate: a disc
    out = run(r, j)
    assert out['screen'][0, 1:5].tolist() == [[328, 488], [648, 488], [808, 136], [808, 136]]
    lay = check(r, out, j)[0]
    chain = lay == 3
    assert chain[35, 25] and chain[25, 30] and not chain[36, 25] and not chain[24, 30]        # cross^2 == R^2 dd on the long sides
    assert chain[26, 17] and chain[34, 43] and chain[30, 15] and not chain[30, 14] and not chain[26, 16] and not chain[34, 44]       # e . e == R^2
    disc = lay == 4
    assert disc[8, 55] and disc[8, 45] and disc[12, 53] and disc[4, 47] and not disc[8, 56] and not disc[12, 54] and disc.sum() == 81
    assert (lay == 1).any() and not (lay == 2).any()


@pytest.mark.parametrize('size', SIZES)
def test_crossing_chains_the_later_one_wins(size):
    W, H = size
    r = two_bones(size, pt=3.0)
    j = placed(r, [(2.3, 3.1), (W - 3.7, H - 2.2), (W - 2.9, 2.6), (3.4, H - 4.3)])
    out = run(r, j)
    lay = check(r, out, j)[0]
    a = R.capsule_mask(out['screen'][0, 1], out['screen'][0, 2], r.chain_radius[0], W, H)
    b = R.capsule_mask(out['screen'][0, 3], out['screen'][0, 4], r.chain_radius[1], W, H)
    assert (a & b).any() and (lay[a & b] == 4).all() and (lay[a & ~b] == 3).all() and (lay[b] == 4).all()


@pytest.mark.parametrize('size', SIZES)
def test_chains_over_the_trail_over_the_plane(size):
    r = sk.SkeletonRenderer(sk.T2M_CHAINS, width=size[0], height=size[1])
    j = walk(7, step=0.25)
    out = run(r, j)
    lay = check(r, out, j)
    assert (out['trail_screen'][:2] == R.INVALID).all() and not (lay[:2] == 2).any()          # frames 0 and 1 have no trail
    assert (lay[-1] == 2).any() and (lay == 1).any(axis=(1, 2)).all() and (lay >= 3).any(axis=(1, 2)).all()
    S = r.camera.screen_projective(*size)
    full = R.render(j, [7], S, r.segments(), r.trail_radius, *size)                           # from world joints, projected in fp64
    assert (lay != full['layer']).mean() < 0.02                                               # snapped points may differ by a unit


def test_segments_outside_the_viewport_past_the_guard_band_and_behind_the_eye():
    cam = sk.Mplot3dCamera(**NARROW)
    r = two_bones((64, 64), camera=cam)
    j = placed(r, [(-50.0, -50.0), (-20.0, -10.0), (10.2, 20.7), (9000.0, 30.0)])             # wholly outside; one vertex past the band
    out = run(r, j)
    lay = check(r, out, j)[0]
    assert (out['screen'][0, 1:4] != R.INVALID).all() and (out['screen'][0, 4] == R.INVALID).all()
    assert not (lay >= 3).any()
    j2 = placed(r, [(10.5, 12.5), (50.5, 40.5), (30.0, 5.0), (0.0, 0.0)])
    eye = R.eye_world(cam)
    centre = cam.limits[:, 0] + 0.5 * (cam.limits[:, 1] - cam.limits[:, 0])
    j2[0, 4] = eye + 0.5 * (eye - centre)                                                     # behind the eye: h_w < 0
    assert j2[0, 4, 1] > 0
    out = run(r, j2)
    lay = check(r, out, j2)[0]
    assert (out['screen'][0, 4] == R.INVALID).all() and (out['screen'][0, 1:4] != R.INVALID).all()
    assert (lay == 3).any() and not (lay == 4).any()


def test_diagonal_with_endpoints_near_the_guard_band():
    """Chain 0 runs through the centres of the corner pixels (0, 0) and (95, 63) from 84 viewport diagonals away on either side; chain
    1 passes about 1100 px from the viewport, its box holds every tile, and its cross product does not fit 64 bits when squared."""
    r = two_bones((96, 64), camera=sk.Mplot3dCamera(**NARROW), pt=4.0)
    j = placed(r, [(0.5 - 84 * 95, 0.5 - 84 * 63), (95.5 + 84 * 95, 63.5 + 84 * 63), (-8000.0, -8000.0), (5000.0, 8000.0)])
    out = run(r, j)
    assert (out['screen'][0, 1:5] != R.INVALID).all() and np.abs(out['screen'][0, 1:3, 0]).min() > 16 * 7900
    lay = check(r, out, j)[0]
    assert lay[0, 0] == 3 and lay[63, 95] == 3 and lay[32, 48] == 3 and (lay == 3).sum() < 96 * 64 // 4 and not (lay == 4).any()
    a, b = [[int(v) for v in q] for q in out['screen'][0, 3:5]]
    for px, py in ((8, 8), (16 * 95 + 8, 16 * 63 + 8)):
        cross = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
        assert cross * cross > 2 ** 64                                                        # decided without the product


@pytest.mark.parametrize('size', SIZES)
def test_a_nan_joint_drops_its_two_segments_only(size):
    r = sk.SkeletonRenderer(sk.T2M_CHAINS, width=size[0], height=size[1])
    j = walk(4, seed=2)
    j[1, 5], j[3, 8] = (j[1, 2] + j[1, 8]) / 2, (j[3, 5] + j[3, 11]) / 2                     # no extreme of the sequence
    clean = run(r, j)
    bad = j.copy()
    bad[1, 5] = [np.nan, -np.inf, np.inf]
    bad[3, 8, 1] = -np.inf
    out = run(r, bad)
    check(r, out, bad)
    assert np.array_equal(out['stats'], clean['stats'])                                       # joints 5 and 8 hold no extreme here
    invalid = np.zeros((4, 26), bool)
    invalid[1, 5] = invalid[3, 8] = True
    assert np.array_equal(out['screen'][..., 0] == R.INVALID, invalid)
    segs = [s for s in r.segments() if 5 not in s[:2]]
    want = R.frame_layers(clean['screen'][1], np.zeros((0, 2)), segs, r.trail_radius, *size)
    assert np.array_equal(out['layer'][1], want) and np.array_equal(out['layer'][[0, 2]], clean['layer'][[0, 2]])


def test_a_sequence_without_a_finite_value_draws_nothing():
    r = sk.SkeletonRenderer(sk.KIT_CHAINS, width=37, height=23)
    j = np.full((3, 21, 3), np.nan, np.float32)
    out = run(r, j)
    check(r, out, j)
    assert not out['layer'].any() and (out['rgb'] == 255).all()


def test_custom_52_joint_chains_with_thin_hands():
    r = sk.SkeletonRenderer(sk.T2M_CHAINS + HANDS, width=64, height=64)
    assert r.num_joints == 52 and r.chain_radius[5:] == [22] * 10
    j = walk(3, J=52, seed=5)
    lay = check(r, run(r, j), j)
    assert set(np.unique(lay)) >= {1, 3, 4, 5, 6, 7} and lay.max() > 7


def test_two_sequences_in_one_call_equal_two_calls():
    r = sk.SkeletonRenderer(sk.KIT_CHAINS, width=96, height=64)
    a, b = walk(5, J=21, seed=1), walk(4, J=21, seed=9) + np.array([0.3, 0.2, -0.1], np.float32)
    both = run(r, np.concatenate([a, b]), [5, 4])
    check(r, both, np.concatenate([a, b]), [5, 4])
    one, two = run(r, a), run(r, b)
    for k in ('rgb', 'layer', 'screen', 'traj'):
        assert np.array_equal(both[k], np.concatenate([one[k], two[k]])), k
    assert np.array_equal(both['stats'], np.concatenate([one['stats'], two['stats']]))
    assert np.array_equal(both['trail_screen'][:5], one['trail_screen']) and np.array_equal(both['trail_screen'][5:, :4], two['trail_screen'])
    with_empty = run(r, np.concatenate([a, b]), [0, 5, 0, 4])
    assert np.array_equal(with_empty['rgb'], both['rgb'])


def test_every_chunking_a_second_run_and_a_second_call_give_the_same_bits():
    r = sk.SkeletonRenderer(sk.T2M_CHAINS, width=37, height=23)
    j = walk(12, seed=3)
    whole = run(r, j, [7, 5])
    check(r, whole, j, [7, 5])
    obj = r.native()
    for c in range(1, 12):
        wb = int(obj.lib.mc_skeleton_work_bytes(obj.handle, c, 7, 37, 23))
        assert wb == c * (32 + 8 * (22 + 4 + 7))
        assert same(run(r, j, [7, 5], work_bytes=wb), whole), c
    assert same(run(r, j, [7, 5]), whole)                                                     # a second call on the same object
    other = sk.SkeletonRenderer(sk.T2M_CHAINS, width=37, height=23)
    assert same(run(other, j, [7, 5], work_bytes=0), whole)                                   # a second object, one frame per chunk
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert same(run(r, j, [7, 5]), whole)
    assert r.render(torch.zeros(0, 22, 3, device='cuda')).shape == (0, 23, 37, 3)
    r.close(), other.close()


def test_t2m_render_draws_the_stitched_golden_motion():
    g = load('t2m_joints.npz')
    tag = 'hml_stitched'
    lens = [int(n) for n in g[f'{tag}.lengths']]
    pred = torch.from_numpy(np.random.RandomState(int(g[f'{tag}.seed'])).randn(len(lens), 196, 263).astype(np.float32)).cuda()
    mean, std, sigma = g[f'{tag}.mean'], g[f'{tag}.std'], float(g[f'{tag}.sigma'])
    r = sk.SkeletonRenderer(sk.T2M_CHAINS, width=96, height=96)
    rgb = P.t2m_render(pred, lens, r, mean, std, sigma=sigma).cpu().numpy()
    assert rgb.shape == (sum(lens), 96, 96, 3) and rgb.dtype == np.uint8
    joints = P.recover_joints_stitched(pred, lens, mean, std, sigma=sigma)
    out = {k: v.cpu().numpy() for k, v in r.render(joints, return_buffers=True).items()}
    assert np.array_equal(rgb, out['rgb']) and np.array_equal(rgb, r.palette[out['layer']])
    assert np.array_equal(rgb, P.t2m_render(pred, lens, r, mean, std, sigma=sigma, work_bytes=40000).cpu().numpy())
    jn = joints.cpu().numpy()
    mins, maxs, traj = R.sequence_stats(jn)
    assert np.array_equal(out['stats'][0], np.concatenate([mins, maxs])) and np.array_equal(out['traj'], traj)
    S = r.camera.screen_projective(96, 96)
    frames = sorted(set(range(4)) | set(range(5, sum(lens), 23)) | {sum(lens) - 1})
    for i in frames:                                                                          # the restatement on a spread of frames
        body, trail = R.frame_points(jn, i, mins, maxs)
        check_points(out['screen'][i], body, S, ('screen', i))
        check_points(out['trail_screen'][i, :len(trail)], trail, S, ('trail', i))
        want = R.frame_layers(out['screen'][i], out['trail_screen'][i, :i] if i >= 2 else [], r.segments(), r.trail_radius, 96, 96)
        assert np.array_equal(out['layer'][i], want), i
    assert (out['layer'] >= 3).any(axis=(1, 2)).all()                                         # the body stays in the picture: it is centred on the root


def test_bad_arguments_fail_with_code_1_and_a_message():
    lib = L.load(require_gpu=True)
    ints = lambda *v: (ctypes.c_int32 * len(v))(*v)
    floats = lambda *v: (ctypes.c_float * len(v))(*v)
    pal = (ctypes.c_uint8 * 12)(*([255] * 12))
    h = ctypes.c_void_p()

    def fails(rc, text):
        assert rc == 1 and text in L.last_error(), (rc, L.last_error())
    create = lambda joints, start, nc, J, widths, trail=1.4: lib.mc_skeleton_create(joints, start, nc, J, widths, trail, pal, ctypes.byref(h))
    fails(create(ints(0), ints(0, 1), 1, 4, floats(2.0)), 'holds 1 joints')
    fails(create(ints(0, 4), ints(0, 2), 1, 4, floats(2.0)), 'names joint 4')
    fails(create(ints(0, 1), ints(0, 2), 1, 4, floats(0.0)), 'width_px')
    fails(create(ints(0, 1), ints(0, 2), 1, 4, floats(2.0), trail=100.0), 'trail_width_px')
    fails(create(ints(0, 1), ints(0, 2), 62, 4, floats(2.0)), 'num_chains')
    fails(create(ints(0, 1), ints(1, 2), 1, 4, floats(2.0)), 'chain_start[0]')
    fails(lib.mc_skeleton_create(None, ints(0, 2), 1, 4, floats(2.0), 1.4, pal, ctypes.byref(h)), 'null')
    assert create(ints(0, 1), ints(0, 2), 1, 4, floats(2.0)) == 0 and h.value
    assert lib.mc_skeleton_work_bytes(h, 3, 5, 64, 64) == 3 * (32 + 8 * 13)
    for bad in ((0, 5, 64, 64), (1, -1, 64, 64), (1, 5, 0, 64), (1, 5, 64, 4097)):
        assert lib.mc_skeleton_work_bytes(h, *bad) == -1
    joints = torch.zeros(3, 4, 3, device='cuda')
    work = torch.empty(4096, device='cuda', dtype=torch.uint8)
    rgb = torch.empty(3, 16, 16, 3, device='cuda', dtype=torch.uint8)
    p = L.SkeletonParams()
    p.screen[:] = [float(v) for v in sk.Mplot3dCamera().screen_projective(16, 16).reshape(-1)]
    p.width, p.height = 16, 16
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def frames(seq=ints(0, 3), S=1, params=p, work_ptr=ptr(work), wb=4096, out=ptr(rgb), handle=h, src=ptr(joints)):
        return lib.mc_skeleton_frames(handle, src, seq, S, ctypes.byref(params), work_ptr, wb, out, None, None, None, None, None, None)
    fails(frames(handle=None), 'null')
    fails(frames(out=None), 'null')
    fails(frames(src=None), 'null')
    fails(frames(seq=ints(1, 3)), 'seq_start[0]')
    fails(frames(seq=ints(0, 3, 2), S=2), 'decreases')
    fails(frames(S=-1), 'num_seqs')
    fails(frames(wb=32 + 8 * 11 - 1), 'work_bytes')
    fails(frames(work_ptr=ctypes.c_void_p(work.data_ptr() + 8)), 'aligned')
    fails(frames(out=ctypes.c_void_p(rgb.data_ptr() + 1)), 'aligned')
    for w, hh in ((0, 16), (16, 4097)):
        q = L.SkeletonParams()
        q.screen[:], q.width, q.height = list(p.screen), w, hh
        fails(frames(params=q), 'width=')
    q = L.SkeletonParams()
    q.screen[:], q.width, q.height = list(p.screen), 16, 16
    q.screen[5] = float('nan')
    fails(frames(params=q), 'not finite')
    assert frames() == 0 and frames(seq=ints(0, 0), S=1, out=None) == 0                       # the good call; no frames, nothing read
    torch.cuda.synchronize()
    lib.mc_skeleton_destroy(h)

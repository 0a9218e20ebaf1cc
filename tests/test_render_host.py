"""Host side of the renderer (no GPU): the reference's camera and light, the screen affine, the numpy restatement's own properties
(``raster_ref.py`` is what the device tests hold the kernels to), the BMP writer, and the argument errors of ``MeshRenderer`` and the
two tools."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_ref as R
from motioncraft_amd import lib as L
from motioncraft_amd import render as mr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_reference_poses_are_the_literal_matrices():
    """fast_render.py:16-33 at the angles it is called with (:51-52): -2 and -30 degrees."""
    c, s = 0.9993908270190958, -0.03489949670250097
    assert np.allclose(mr.reference_camera_pose(), [[1, 0, 0, 0], [0, c, -s, 1], [0, s, c, 5], [0, 0, 0, 1]], rtol=0, atol=1e-15)
    c, s = 0.8660254037844387, -0.5
    assert np.allclose(mr.reference_light_pose(), [[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 3], [0, 0, 0, 1]], rtol=0, atol=1e-15)
    light = mr.DirectionalLight()
    assert np.allclose(light.direction, [0, 0.5, c]) and light.gain == 4.0 / np.pi and light.ambient == 0.0
    assert mr.reference_camera_pose(10)[1, 2] == -np.sin(np.pi / 18)


@pytest.mark.parametrize('size', [(960, 720), (37, 23)])
def test_screen_affine_maps_the_view_volume_to_the_viewport(size):
    W, H = size
    cam = mr.OrthographicCamera()
    a64, a32 = cam.screen_affine64(W, H), cam.screen_affine(W, H)
    assert a32.dtype == np.float32 and a32.shape == (3, 4) and np.array_equal(a32, a64.astype(np.float32))
    for cx, cy, col, row in ((-1, 1, 0, 0), (1, 1, W, 0), (-1, -1, 0, H), (1, -1, W, H)):
        for depth in (0.05, 7.0):
            world = cam.pose @ np.array([cx, cy, -depth, 1.0])              # a corner of the [-1,1]^2 view volume, camera -> world
            s = a64 @ world
            assert np.allclose(s, [col, row, depth], rtol=0, atol=1e-9), (cx, cy, s)
    s = a64 @ np.array([0.0, 1.0, 0.0, 1.0])
    assert abs(s[0] - W / 2) < 1 and 0 < s[1] < H and abs(s[2] - 5.0) < 0.05
    wide = mr.OrthographicCamera(xmag=4 / 3).screen_affine64(W, H)           # no aspect correction unless the caller asks
    assert np.isclose(wide[0, 0], a64[0, 0] * 3 / 4)


def test_camera_and_light_argument_errors():
    for kw in (dict(xmag=0), dict(ymag=-1), dict(znear=0), dict(znear=2, zfar=1), dict(zfar=np.inf), dict(pose=np.eye(3))):
        with pytest.raises(ValueError):
            mr.OrthographicCamera(**kw)
    for kw in (dict(intensity=-1), dict(ambient=-0.1), dict(pose=np.zeros((4, 4)))):
        with pytest.raises(ValueError):
            mr.DirectionalLight(**kw)


def random_triangle(rs, size):
    return np.round(rs.uniform(-2, size + 2, (3, 2)) * 256).astype(np.int64)


def test_shared_edge_pairs_cover_their_union_exactly_once():
    rs = np.random.RandomState(0)
    S = 12
    for trial in range(300):
        q = random_triangle(rs, S)
        d = np.round(rs.uniform(-2, S + 2, 2) * 256).astype(np.int64)
        if trial % 3 == 0:                                                   # edges and vertices through pixel centres
            q = (q // 256) * 256 + 128
            d = (d // 256) * 256 + 128
        a, b = q, np.stack([q[1], q[0], d])                                  # share the edge q0-q1, opposite winding along it
        side = lambda p: np.sign(R.edge(*q[0], *q[1], *p))
        if side(q[2]) * side(d) >= 0:
            continue                                                         # both on one side: they overlap
        ca, cb = R.coverage(a, S, S), R.coverage(b, S, S)
        assert not (ca & cb).any(), trial
        # the union is the quadrilateral q0 d q1 q2 when it is convex: compare with the other diagonal's split
        c, e = np.stack([q[2], q[0], d]), np.stack([q[2], d, q[1]])
        o = lambda t: np.sign(R.edge(*t[0], *t[1], *t[2]))
        if o(c) == o(e) == o(a) and o(a) != 0:
            assert np.array_equal(ca | cb, R.coverage(c, S, S) | R.coverage(e, S, S)), trial
            assert not (R.coverage(c, S, S) & R.coverage(e, S, S)).any(), trial


def test_coverage_is_invariant_under_rotation_of_the_indices_and_matches_exact_rationals():
    rs = np.random.RandomState(1)
    S = 10
    for trial in range(60):
        t = random_triangle(rs, S)
        if trial % 4 == 0:
            t = (t // 128) * 128
        c = R.coverage(t, S, S)
        assert np.array_equal(c, R.coverage(t[[1, 2, 0]], S, S)) and np.array_equal(c, R.coverage(t[[2, 0, 1]], S, S)), trial
        assert np.array_equal(c, R.coverage(t[[0, 2, 1]], S, S)), trial      # culling off: the other winding covers the same samples
        area = R.edge(*t[0], *t[1], *t[2])
        assert np.array_equal(R.coverage(t, S, S, cull=True), c if area < 0 else np.zeros_like(c)), trial
        exact = R.covered_rational(t, S, S)
        assert c[exact > 0].all() and not c[exact < 0].any(), trial


def test_top_left_rule_on_edges_through_pixel_centres():
    px = lambda x, y: (256 * x + 128, 256 * y + 128)
    t = np.array([px(1, 1), px(1, 5), px(5, 1)])                             # front (counter-clockwise with y up); legs on a row and a column
    c = R.coverage(t, 8, 8, cull=True)
    assert c[1, 1:5].all() and not c[1, 5]                                   # the top edge owns its samples, up to the far corner
    assert c[1:5, 1].all() and not c[5, 1]                                   # so does the left edge
    assert not c[3, 3] and c[2, 3] and c[3, 2]                               # the hypotenuse x + y = 6 is neither top nor left
    t = np.array([px(5, 5), px(5, 1), px(1, 5)])                             # the mirrored triangle: bottom and right legs
    c = R.coverage(t, 8, 8, cull=True)
    assert not c[5, :].any() and not c[:, 5].any() and c[3, 3] and c[4, 4] and not c[2, 3]


def test_restatement_depth_order_and_normals():
    v, f = R.octahedron(level=2)
    assert f.shape == (128, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((v[f].mean(1) - [0, 1, 0]) * fn).sum(1).min() > 0                # outward orientation
    n = R.vertex_normals(v, f)
    assert np.allclose(n, (v - [0, 1, 0]) / 0.5, atol=0.1)                    # a coarse sphere: area weights pull a little
    cam = mr.OrthographicCamera()
    r = R.render_world(v, cam.screen_affine64(64, 64), f, 64, 64)
    rb = R.render_world(v, cam.screen_affine64(64, 64), f[:, [0, 2, 1]], 64, 64)
    assert (r['face'] >= 0).sum() > 300 and np.array_equal(r['face'] >= 0, rb['face'] >= 0)      # a closed mesh: the same silhouette
    both = r['face'] >= 0
    assert (rb['depth'][both] > r['depth'][both]).all()                      # inside out, the far side shows
    two = np.concatenate([f[:1], f[:1]])                                     # coincident triangles: the lower id wins
    assert set(np.unique(R.render_world(v, cam.screen_affine64(64, 64), two, 64, 64)['face'])) <= {-1, 0}
    img = R.shade(r['face'], R.snap(v, cam.screen_affine64(64, 64))[0], f, n, mr.DirectionalLight().direction)
    assert (img[~both] == 255).all() and img[both].max() == 255 and img[both].min() < 200


@pytest.mark.parametrize('shape', [(2, 5, 7), (3, 4, 8), (1, 1, 1)])
def test_bmp_frames_round_trip(tmp_path, shape):
    n, H, W = shape
    frames = np.random.RandomState(n).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    paths = mr.write_frames(torch.from_numpy(frames), str(tmp_path / 'out'))
    assert [os.path.basename(p) for p in paths] == [f'frame_{i}.bmp' for i in range(n)]
    for i, p in enumerate(paths):
        assert np.array_equal(R.read_bmp(p), frames[i])
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.asarray(Image.open(p).convert('RGB')), frames[i])
    with pytest.raises(ValueError, match='filetype'):
        mr.write_frames(frames, str(tmp_path), filetype='png')
    with pytest.raises(ValueError, match='uint8'):
        mr.write_frames(frames.astype(np.float32), str(tmp_path))


def test_mesh_renderer_argument_errors():
    faces = np.array([[0, 1, 2], [2, 1, 3]])
    ok = mr.MeshRenderer(faces, 4, width=8, height=8)
    start, adj = ok.adj_start, ok.adj_faces
    assert start.tolist() == [0, 1, 3, 5, 6] and adj.tolist() == [0, 0, 1, 0, 1, 1] and start.dtype == adj.dtype == np.int32
    assert ok.params().gain == np.float32(4 / np.pi) and list(ok.params().background) == [255, 255, 255] and ok.params().cull_backfaces == 1
    bad = [(dict(faces=faces.astype(np.float32)), 'faces'), (dict(faces=faces[:, :2]), 'faces'), (dict(faces=faces[:0]), 'faces'),
           (dict(num_vertices=3), 'num_vertices'), (dict(faces=faces - 1), 'num_vertices'), (dict(width=0), 'width'),
           (dict(height=16385), 'height'), (dict(width=9.5), 'width'), (dict(camera='persp'), 'camera'), (dict(light=3), 'light'),
           (dict(color=(1, 2)), 'color'), (dict(color=(0, 0, 256)), 'color'), (dict(background=(0.5, 0, 0)), 'background'),
           (dict(large_threshold=0), 'large_threshold'), (dict(large_slices=2000), 'large_slices')]
    for kw, name in bad:
        args = dict(faces=faces, num_vertices=4)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            mr.MeshRenderer(**args)
    with pytest.raises(ValueError, match='vertices'):
        ok.render(torch.zeros(1, 4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='vertices'):
        ok.render(torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match='vertices'):
        ok.render(np.zeros((1, 4, 3), np.float32))
    with pytest.raises(ValueError, match='vertices.*device'):
        ok.render(torch.zeros(1, 4, 3))
    ok.close()


def test_library_exports_the_renderer():
    lib = L.load()
    for name in ('mc_render_create', 'mc_render_destroy', 'mc_render_work_bytes', 'mc_render_frames'):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    import ctypes
    assert ctypes.sizeof(L.RenderParams) == 4 * (12 + 3 + 3 + 4 + 3 + 5)
    assert lib.mc_render_work_bytes(None, 1, 8, 8) == -1


def run_tool(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', name)] + list(args), capture_output=True, text=True, timeout=300)


def test_tool_argument_errors(tmp_path):
    """Both tools refuse a bad command line before they touch the device."""
    r = run_tool('render_npz.py', '--help')
    assert r.returncode == 0 and '--smplx_model' in r.stdout and '--gt' in r.stdout and '--render_size' in r.stdout
    r = run_tool('sample.py', '--help')
    assert r.returncode == 0 and '--render_dir' in r.stdout and '--render_size' in r.stdout and '--render_fps' in r.stdout
    npz = str(tmp_path / 'res_x.npz')
    np.savez(npz, poses=np.zeros((2, 165)), expressions=np.zeros((2, 100)), trans=np.zeros((2, 3)), betas=np.zeros(300))
    r = run_tool('render_npz.py', npz, '--out', str(tmp_path))
    assert r.returncode != 0 and '--smplx_model' in r.stderr
    for size in ('960', '0x720', '20000x10', 'axb'):
        r = run_tool('render_npz.py', npz, '--smplx_model', 'none.npz', '--out', str(tmp_path), '--render_size', size)
        assert r.returncode != 0 and '--render_size' in r.stderr, size
    r = run_tool('render_npz.py', npz, '--smplx_model', 'none.npz', '--out', str(tmp_path), '--render_fps', '0')
    assert r.returncode != 0 and '--render_fps' in r.stderr
    np.savez(str(tmp_path / 'bad.npz'), poses=np.zeros((2, 165)))
    r = run_tool('render_npz.py', str(tmp_path / 'bad.npz'), '--smplx_model', 'none.npz', '--out', str(tmp_path))
    assert r.returncode != 0 and 'expressions' in r.stderr
    cfg = os.path.join(HERE, 'configs', 'stmogen_small.py')
    base = [cfg, 'synthetic:3', '--text', 'a', '--motion_length', '8', '--out', str(tmp_path)]
    r = run_tool('sample.py', *base, '--render_dir', str(tmp_path / 'frames'))
    assert r.returncode != 0 and '--render_dir' in r.stderr and '--smplx_model' in r.stderr
    r = run_tool('sample.py', *base, '--render_dir', str(tmp_path / 'frames'), '--smplx_model', 'none.npz', '--render_size', '12')
    assert r.returncode != 0 and '--render_size' in r.stderr
    r = run_tool('sample.py', *base, '--smplx_model', 'none.npz')
    assert r.returncode != 0 and '--smplx_model alone writes nothing' in r.stderr and '--render_dir' in r.stderr

"""On the MI355X: ``render.MeshRenderer`` (``mc_render_*``, csrc/mc_render.hip) against the numpy restatement ``raster_ref.py``.

Rules.
  * projection: ``screen`` equals floor(256 * fp64 projection + 0.5) within +-1 sub-pixel unit, ``zcam`` is within 4 ulp of fp64.
  * coverage is exact: the restatement, fed the kernel's OWN ``screen`` / ``zcam``, must give the same ``face`` at every pixel, except
    where its two nearest covering faces lie within TAU = 1e-5 of each other in depth (about 20 fp32 ulp at the scenes' z of about 5:
    the rounding of the two-fma interpolation).  Such pixels must stay under 0.5 % of the covered pixels of a case; ``depth`` is within
    TAU on agreeing pixels.  The one case built to tie everywhere (two coincident triangles) is held to exact equality instead.
  * shading: on agreeing pixels every channel is within +-1 of the restatement's uint8 (one rounding boundary may be crossed);
    background pixels equal ``background`` exactly.
  * the wave path for large triangles, any chunking of the frames, a second run, and a second call on the same object give the same
    bits in every buffer.
Measured on the device: excusable shares per case, and the duration of this file.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_ref as R
import smplx_lbs_ref as lbs_ref
from motioncraft_amd import lib as L
from motioncraft_amd import postprocess as P
from motioncraft_amd import render as mr
from motioncraft_amd.body_model import SMPLXBodyModel

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAU = 1e-5
CAP = 0.005
SIZES = [(37, 23), (64, 64), (96, 64)]
FRONT = np.eye(4)
FRONT[2, 3] = 5.0                                # a camera at (0, 0, 5) looking down -Z: ndc = (x, y), depth = 5 - z


def tri(*pts):
    """vertices [(x_ndc, y_ndc, depth)] -> world coordinates under the FRONT camera"""
    a = np.asarray(pts, np.float64)
    return np.stack([a[:, 0], a[:, 1], 5.0 - a[:, 2]], axis=1)


def pixel_centres():
    """At 64 x 64 every vertex is a pixel centre: legs along a row and a column, one triangle owning them (top, left) and its mirror
    image not (bottom, right)."""
    c = lambda x, y, d: ((x + 0.5) / 32 - 1, 1 - (y + 0.5) / 32, d)
    v = tri(c(8, 8, 5), c(8, 40, 5), c(40, 8, 5), c(60, 60, 4), c(60, 28, 4), c(28, 60, 4))
    return v, [[0, 1, 2], [3, 4, 5]]


def shared_edge():
    return tri((-0.8, -0.7, 5), (0.7, -0.9, 5.5), (0.9, 0.8, 4.5), (-0.6, 0.9, 5)), [[0, 1, 2], [0, 2, 3]]


def zero_area():
    v = tri((-0.9, -0.9, 5), (0.0, 0.0, 5), (0.9, 0.9, 5), (-0.5, 0.5, 5), (0.5, -0.9, 6), (0.9, 0.3, 6), (-0.2, 0.6, 6))
    return v, [[0, 1, 2], [3, 3, 1], [4, 5, 6]]


def back_and_front():
    v = tri((-0.9, -0.8, 5), (-0.1, 0.9, 5), (0.3, -0.6, 5), (-0.2, -0.9, 6), (0.9, -0.7, 6), (0.5, 0.9, 4))
    return v, [[0, 1, 2], [3, 4, 5]]              # clockwise with y up = back; counter-clockwise = front, crossing it in depth


def outside():
    v = tri((-1.6, -0.5, 5), (0.4, -1.5, 5), (0.2, 0.7, 5), (1.2, 1.2, 5), (2.0, 1.3, 5), (1.5, 2.2, 5), (0.6, 0.2, 4), (0.99, 0.3, 4),
            (0.8, 0.97, 4))
    return v, [[0, 1, 2], [3, 4, 5], [6, 7, 8]]


def guard_band():
    """16384 px from the origin is ndc 2 * 16384 / W: a vertex beyond it drops its triangle, one just inside does not (a huge
    triangle, clamped to the viewport: the wave path)."""
    far, near = 2.0 * 16384 / 37 + 5.0, 2.0 * 16000 / 96 - 1.0
    return tri((-0.5, -0.5, 5), (far, -0.4, 5), (0.0, 0.8, 5), (-0.9, -0.9, 6), (near, -0.9, 6), (-0.9, near, 6)), [[0, 1, 2], [3, 4, 5]]


def nan_vertex():
    v = tri((-0.5, -0.5, 5), (0.6, -0.4, 5), (0.0, 0.8, 5), (-0.9, -0.9, 6), (0.9, -0.9, 6), (0.0, 0.9, 6), (0.1, 0.1, 4), (0.9, 0.2, 4), (0.4, 0.8, 4))
    v[1, 0], v[7, 2] = np.nan, np.inf
    return v, [[0, 1, 2], [3, 4, 5], [6, 7, 8]]


def znear_straddle():
    """one triangle through znear = 0.05 (and through the camera plane), one through zfar = 6"""
    return tri((-0.9, -0.8, -1.0), (0.9, -0.7, 0.02), (0.0, 0.9, 3.0), (-0.8, 0.8, 5.5), (-0.9, -0.2, 6.5), (0.8, 0.5, 6.2)), [[0, 1, 2], [3, 4, 5]]


def coincident():
    return tri((-0.8, -0.7, 4.7), (0.7, -0.9, 5.5), (0.1, 0.8, 4.9)), [[0, 1, 2], [0, 1, 2]]


def random_small(seed=5, count=2000):
    rs = np.random.RandomState(seed)
    c = np.concatenate([rs.uniform(-1.05, 1.05, (count, 1, 2)), rs.uniform(3.0, 7.0, (count, 1, 1))], axis=2)
    d = np.concatenate([rs.uniform(-0.12, 0.12, (count, 3, 2)), rs.uniform(-0.5, 0.5, (count, 3, 1))], axis=2)
    return tri(*(c + d).reshape(-1, 3)), np.arange(3 * count).reshape(count, 3)


def bodies():
    """two closed ellipsoids of 2048 faces each, the second pushed through the first"""
    v0, f0 = R.octahedron(4, 1.0, (-0.1, 0.0, 0.0), (0.55, 0.9, 0.5))
    v1, f1 = R.octahedron(4, 1.0, (0.25, 0.1, 0.2), (0.5, 0.7, 0.6))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + v0.shape[0]])


CASES = dict(pixel_centres=(pixel_centres, {}), shared_edge=(shared_edge, {}), zero_area=(zero_area, {}), back_cull_on=(back_and_front, {}),
             back_cull_off=(back_and_front, dict(cull_backfaces=False)), outside=(outside, {}), guard_band=(guard_band, {}),
             nan_vertex=(nan_vertex, {}), znear_straddle=(znear_straddle, dict(zfar=6.0)), random_small=(random_small, {}), bodies=(bodies, {}))
# how many faces must show at least one pixel, per case: what the case is about
VISIBLE = dict(pixel_centres={0, 1}, shared_edge={0, 1}, zero_area={2}, back_cull_on={1}, back_cull_off={0, 1}, outside={0, 2}, guard_band={1},
               nan_vertex={1}, znear_straddle={0, 1})


def front_camera(**kw):
    return mr.OrthographicCamera(pose=FRONT, **kw)


def against_restatement(renderer, verts, frames, tag, cap=CAP):
    """Rules 2, 3 and 5 of the module docstring on every frame of ``frames`` = (rgb, face, depth, screen, zcam); returns the
    excusable share of the worst frame."""
    rgb, face, depth, screen, zcam = [t.cpu().numpy() for t in frames]
    W, H, cam = renderer.width, renderer.height, renderer.camera
    worst = 0.0
    for i in range(rgb.shape[0]):
        ref = R.rasterize(screen[i], zcam[i], renderer.faces, W, H, cam.znear, cam.zfar, renderer.cull_backfaces)
        covered = ref['face'] >= 0
        with np.errstate(invalid='ignore'):                                  # inf - inf on the background
            excusable = covered & (ref['second'] - ref['depth'] <= TAU)
        share = excusable.sum() / max(1, covered.sum())
        worst = max(worst, share)
        differ = face[i] != ref['face']
        print(f'{tag} frame {i}: {covered.sum()} covered, {excusable.sum()} excusable ({100 * share:.3f} %), {differ.sum()} differ')
        assert share < cap, (tag, share)
        assert not (differ & ~excusable).any(), (tag, np.argwhere(differ & ~excusable)[:5])
        agree = covered & ~differ
        assert np.isinf(depth[i][face[i] < 0]).all()
        assert np.abs(depth[i][agree] - ref['depth'][agree]).max(initial=0.0) <= TAU, tag
        normals = R.vertex_normals(verts[i].astype(np.float64), renderer.faces)
        img = R.shade(np.where(agree, ref['face'], -1), screen[i], renderer.faces, normals, renderer.light.direction, renderer.color,
                      renderer.background, renderer.light.ambient, renderer.light.gain)
        assert (rgb[i][face[i] < 0] == np.asarray(renderer.background, np.uint8)).all(), tag
        err = np.abs(rgb[i][agree].astype(np.int32) - img[agree].astype(np.int32))
        assert err.max(initial=0) <= 1, (tag, err.max())
    return worst


def test_projection_at_the_reference_camera():
    rs = np.random.RandomState(3)
    verts = (rs.uniform(-1, 1, (3, 100, 3)) + [0, 1, 0]).astype(np.float32)
    r = mr.MeshRenderer([[0, 1, 2]], 100)
    _, _, _, screen, zcam = r.render(torch.from_numpy(verts).cuda(), return_buffers=True)
    a = r.camera.screen_affine64(960, 720)
    s = verts.astype(np.float64) @ a[:, :3].T + a[:, 3]
    want = np.floor(256 * s[..., :2] + 0.5)
    assert screen.dtype == torch.int32 and np.abs(screen.cpu().numpy() - want).max() <= 1
    z = zcam.cpu().numpy()
    ulps = np.abs(z.astype(np.float64) - s[..., 2]) / np.spacing(s[..., 2].astype(np.float32)).astype(np.float64)
    print(f'zcam: max {ulps.max():.2f} ulp, screen: max {np.abs(screen.cpu().numpy() - want).max():.0f} sub-pixel units')
    assert ulps.max() <= 4
    r.close()


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('case', list(CASES))
def test_coverage_depth_and_shading_equal_the_restatement(case, size):
    build, kw = CASES[case]
    kw = dict(kw)
    verts, faces = build()
    verts = verts.astype(np.float32)[None]
    r = mr.MeshRenderer(faces, verts.shape[1], width=size[0], height=size[1], camera=front_camera(zfar=kw.pop('zfar', 100.0)), **kw)
    out = r.render(torch.from_numpy(verts).cuda(), return_buffers=True)
    against_restatement(r, verts, out, f'{case} {size[0]}x{size[1]}')
    face = out[1].cpu().numpy()
    if case in VISIBLE:
        assert set(np.unique(face)) - {-1} == VISIBLE[case], np.unique(face)
    else:
        assert len(np.unique(face)) > 150
    if case == 'pixel_centres' and size == (64, 64):
        f = face[0]
        assert (f[8, 8:40] == 0).all() and f[8, 40] == -1 and (f[8:40, 8] == 0).all() and f[40, 8] == -1 and f[24, 24] == -1 and f[23, 24] == 0
        assert (f[60, :] != 1).all() and (f[:, 60] != 1).all() and f[44, 44] == 1 and f[59, 59] == 1
    r.close()


@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_coincident_triangles_go_to_the_lower_id(size):
    verts, faces = coincident()
    verts = verts.astype(np.float32)[None]
    r = mr.MeshRenderer(faces, 3, width=size[0], height=size[1], camera=front_camera())
    _, face, depth, screen, zcam = [t.cpu().numpy() for t in r.render(torch.from_numpy(verts).cuda(), return_buffers=True)]
    ref = R.rasterize(screen[0], zcam[0], faces, size[0], size[1])
    assert np.array_equal(face[0], ref['face']) and set(np.unique(face)) == {-1, 0} and (ref['second'][face[0] == 0] == ref['depth'][face[0] == 0]).all()
    r.close()


def sheet(n=10):
    """a wavy n x n sheet of 2 n^2 front-facing triangles in front of a full-viewport quad"""
    g = np.linspace(-0.7, 0.7, n + 1)
    x, y = np.meshgrid(g, g, indexing='xy')
    v = tri(*np.stack([x.ravel(), y.ravel(), 4.0 + 0.3 * np.sin(3 * x.ravel()) * np.cos(2 * y.ravel())], axis=1))
    idx = lambda i, j: j * (n + 1) + i
    f = [t for j in range(n) for i in range(n) for t in ([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])]
    quad = tri((-1.2, -1.2, 6), (1.2, -1.2, 6.5), (1.2, 1.2, 6), (-1.2, 1.2, 5.5))
    k = v.shape[0]
    return np.concatenate([v, quad]), np.asarray(f + [[k, k + 1, k + 2], [k, k + 2, k + 3]])


def test_large_triangle_path_gives_the_same_bits():
    verts, faces = sheet()
    assert faces.shape[0] == 202
    verts = torch.from_numpy(verts.astype(np.float32)[None]).cuda()
    outs = {}
    for name, threshold, slices in (('all_large', 1, None), ('one_wave', 1, 1), ('default', None, None), ('mixed', 40, 3), ('all_small', 2 ** 31 - 1, None)):
        r = mr.MeshRenderer(faces, verts.shape[1], width=96, height=64, camera=front_camera(), large_threshold=threshold, large_slices=slices)
        outs[name] = r.render(verts, return_buffers=True)
        if name == 'mixed':
            against_restatement(r, verts.cpu().numpy(), outs[name], 'sheet over a quad')
        r.close()
    face = outs['all_small'][1]
    assert (face >= 0).all() and (face >= 200).sum() > 1000 and (face < 200).sum() > 1000
    for name in ('all_large', 'one_wave', 'default', 'mixed'):
        for a, b in zip(outs[name], outs['all_small']):
            assert torch.equal(a, b), name


def test_flat_shading_of_a_triangle_that_faces_the_light():
    d = mr.DirectionalLight().direction
    u = np.cross(d, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    w = np.cross(d, u)                            # (u, w, d) is right-handed: the normal of (0, u, w) is +d
    verts = (np.stack([-0.5 * u - 0.4 * w, 0.9 * u - 0.3 * w, -0.2 * u + 0.8 * w])).astype(np.float32)[None]
    for intensity, want in ((4.0, min(255, round(220 * 4.0 / np.pi))), (2.0, round(220 * 2.0 / np.pi)), (0.0, 0)):
        r = mr.MeshRenderer([[0, 1, 2]], 3, width=64, height=64, camera=front_camera(), light=mr.DirectionalLight(intensity=intensity))
        rgb, face, *_ = r.render(torch.from_numpy(verts).cuda(), return_buffers=True)
        on = (face >= 0).cpu().numpy()
        assert on.sum() > 200 and (rgb.cpu().numpy()[on] == want).all() and (rgb.cpu().numpy()[~on] == 255).all(), (intensity, want)
        r.close()
    assert min(255, round(220 * 4.0 / np.pi)) == 255


def test_chunking_and_repetition_give_the_same_bits():
    v, f = R.octahedron(2, 1.0, (0.0, 0.0, 0.0), (0.5, 0.8, 0.5))
    rs = np.random.RandomState(7)
    verts = torch.from_numpy(np.stack([v + rs.uniform(-0.3, 0.3, 3) for _ in range(5)]).astype(np.float32)).cuda()
    r = mr.MeshRenderer(f, v.shape[0], width=37, height=23, camera=front_camera())
    need = lambda n: int(r.native().lib.mc_render_work_bytes(r.native().handle, n, 37, 23))
    assert need(1) < need(2) < need(5) and need(0) == -1
    base = r.render(verts, work_bytes=need(5), return_buffers=True)
    against_restatement(r, verts.cpu().numpy(), base, 'five frames')
    assert not torch.equal(base[0][0], base[0][1])
    for wb in (need(1), need(2), need(2) + 8, need(5), need(5)):              # 5, 3, 3, 1, 1 chunks; the last repeats on a kept buffer
        again = r.render(verts, work_bytes=wb, return_buffers=True)
        for a, b in zip(again, base):
            assert torch.equal(a, b), wb
    assert torch.equal(r.render(verts[:2]), base[0][:2]) and torch.equal(r.render(verts[3]), base[0][3:4])      # the keys were left clear
    fresh = mr.MeshRenderer(f, v.shape[0], width=37, height=23, camera=front_camera())
    for a, b in zip(fresh.render(verts, return_buffers=True), base):
        assert torch.equal(a, b)
    assert fresh.render(verts[:0]).shape == (0, 23, 37, 3)
    fresh.close(), r.close()


def test_native_object_checks():
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    faces, start, adj = np.array([[0, 1, 2]], np.int32), np.array([0, 1, 2, 3], np.int32), np.array([0, 0, 0], np.int32)
    for bad, msg in ((dict(faces=np.array([[0, 1, 3]], np.int32)), 'is no vertex'), (dict(start=np.array([0, 2, 1, 3], np.int32)), 'decreases'),
                     (dict(adj=np.array([0, 1, 0], np.int32)), 'is no face'), (dict(start=np.array([1, 1, 2, 3], np.int32)), 'expected 0')):
        a = dict(faces=faces, start=start, adj=adj)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r'mc_render_create failed \(code 1\).*' + msg):
            L.NativeObject('render', as_p(a['faces']), 1, 3, as_p(a['start']), as_p(a['adj']))
    o = L.NativeObject('render', as_p(faces), 1, 3, as_p(start), as_p(adj))
    p = mr.MeshRenderer(faces, 3, width=8, height=8).params()
    v, rgb, work = torch.zeros(1, 3, 3, device='cuda'), torch.empty(1, 8, 8, 3, dtype=torch.uint8, device='cuda'), torch.empty(4096, dtype=torch.uint8, device='cuda')
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda wb: o.lib.mc_render_frames(o.handle, ptr(v), 1, ctypes.byref(p), ptr(work), wb, 0, ptr(rgb), None, None, None, None, None)
    assert call(64) == 1 and 'one 8x8 frame needs' in L.last_error()
    p.znear = 0.0
    assert call(4096) == 1 and 'znear' in L.last_error()
    p.znear = 0.05
    assert call(4096) == L.MC_OK, L.last_error()
    torch.cuda.synchronize()
    assert (rgb == 255).all()
    o.close()


def test_through_the_body_model_and_the_tool(tmp_path):
    """poses -> postprocess.smplx_render -> frames on a synthetic model file (random faces: hundreds of layers of large triangles),
    then tools/render_npz.py in a child process on the same two frames."""
    arrays = lbs_ref.synthetic_model(V=1031, shape_space=300, seed=13)
    mpath = str(tmp_path / 'model.npz')
    np.savez(mpath, **arrays)
    body = SMPLXBodyModel.from_npz(mpath)
    rs = np.random.RandomState(17)
    motion = dict(poses=lbs_ref.random_poses(2, 19, scale=0.2), expressions=0.5 * rs.randn(2, 100), trans=np.array([[0.0, 1.0, 0.0], [0.1, 0.9, 0.2]]))
    motion['poses'][:, :3] *= 0.2
    post = {k: torch.from_numpy(a).cuda() for k, a in motion.items()}
    r = mr.MeshRenderer(body.faces, body.num_vertices, width=96, height=64)
    frames = P.smplx_render(post, body, r)
    assert frames.shape == (2, 64, 96, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    verts = P.smplx_vertices(post, body)
    out = r.render(verts, return_buffers=True)
    assert torch.equal(out[0], frames) and (out[1] >= 0).float().mean() > 0.1
    against_restatement(r, verts.cpu().numpy(), out, 'synthetic body')
    npz = str(tmp_path / 'res_two.npz')
    np.savez(npz, betas=np.zeros(300), **motion)
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'render_npz.py'), npz, '--smplx_model', mpath, '--out', str(tmp_path / 'frames'),
           '--render_size', '96x64', '--gt', npz]
    run = subprocess.run(['timeout', '-k', '10', '120'] + cmd, capture_output=True, text=True, timeout=150)
    assert run.returncode == 0, run.stderr[-2000:]
    want = torch.cat([frames, frames], dim=2).cpu().numpy()
    for i in range(2):
        assert np.array_equal(R.read_bmp(str(tmp_path / 'frames' / f'frame_{i}.bmp')), want[i])
    r.close(), body.close()

"""numpy restatement of the rasteriser ``mc_render_*`` (include/motioncraft_amd.h): int64 edge functions and the top-left fill rule,
fp64 depth and shading, the same drop rules.  It is the yardstick of ``test_render_host.py`` (which checks the restatement's own
properties) and ``test_render_gpu.py`` (which holds the kernels to it).

Screen space: x to the right, y DOWN (row 0 on top), coordinates snapped to 1/256 px.  The sample of pixel (x, y) is its centre
P = (256 x + 128, 256 y + 128).  E_ab(P) = (bx - ax)(Py - ay) - (by - ay)(Px - ax); w0 = E_12, w1 = E_20, w2 = E_01; area = E_01(v2) < 0
is counter-clockwise with y up = front.
"""
import struct
from fractions import Fraction

import numpy as np

GUARD = 16384 * 256
OUTSIDE = -2 ** 31


def snap(verts, affine):
    """World vertices [V,3] and the 3x4 screen affine, both taken to fp64 -> snapped int64 [V,2] (``OUTSIDE`` where the coordinate is
    not finite or beyond the guard band) and zcam fp64 [V]."""
    v = np.asarray(verts, np.float64)
    a = np.asarray(affine, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        s = v @ a[:, :3].T + a[:, 3]
        q = np.floor(256.0 * s[:, :2] + 0.5)
        ok = np.isfinite(q) & (np.abs(q) <= GUARD)
    return np.where(ok, np.where(ok, q, 0.0), OUTSIDE).astype(np.int64), s[:, 2]


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _bias(ax, ay, bx, by, sign):
    dx, dy = (bx - ax) * sign, (by - ay) * sign
    return 0 if (dy < 0 or (dy == 0 and dx > 0)) else -1      # a top or a left edge owns the samples on it


def triangle_samples(xy, z, width, height, cull=True):
    """One triangle, ``xy`` int [3,2] and ``z`` [3]: (ys, xs, w1, w2, area) of its covered pixel centres inside the viewport, or None
    when it is dropped (bad vertex, zero area, culled back face, nothing covered)."""
    xy = [[int(c) for c in p] for p in xy]
    if any(abs(c) > GUARD for p in xy for c in p) or not np.all(np.isfinite(np.asarray(z, np.float64))):
        return None
    (x0, y0), (x1, y1), (x2, y2) = xy
    area = edge(x0, y0, x1, y1, x2, y2)
    if area == 0 or (area > 0 and cull):
        return None
    sign = 1 if area > 0 else -1
    bx0, bx1 = max(-((128 - min(x0, x1, x2)) // 256), 0), min((max(x0, x1, x2) - 128) // 256, width - 1)
    by0, by1 = max(-((128 - min(y0, y1, y2)) // 256), 0), min((max(y0, y1, y2) - 128) // 256, height - 1)
    if bx0 > bx1 or by0 > by1:
        return None
    py, px = np.meshgrid(256 * np.arange(by0, by1 + 1, dtype=np.int64) + 128, 256 * np.arange(bx0, bx1 + 1, dtype=np.int64) + 128, indexing='ij')
    w0, w1, w2 = edge(x1, y1, x2, y2, px, py), edge(x2, y2, x0, y0, px, py), edge(x0, y0, x1, y1, px, py)
    inside = ((sign * w0 + _bias(x1, y1, x2, y2, sign) >= 0) & (sign * w1 + _bias(x2, y2, x0, y0, sign) >= 0)
              & (sign * w2 + _bias(x0, y0, x1, y1, sign) >= 0))
    if not inside.any():
        return None
    ys, xs = np.nonzero(inside)
    return ys + by0, xs + bx0, w1[inside], w2[inside], area


def coverage(xy, width, height, cull=False):
    """bool [H,W]: the samples one triangle covers."""
    out = np.zeros((height, width), bool)
    s = triangle_samples(xy, (1.0, 1.0, 1.0), width, height, cull)
    if s is not None:
        out[s[0], s[1]] = True
    return out


def covered_rational(xy, width, height):
    """Brute force with exact rationals: +1 where the pixel centre is strictly inside the triangle, -1 strictly outside, 0 on an edge
    line.  P = v0 + s (v1 - v0) + t (v2 - v0) solved by Cramer's rule; inside <=> s > 0, t > 0, s + t < 1."""
    (x0, y0), (x1, y1), (x2, y2) = [[Fraction(int(c), 256) for c in p] for p in xy]
    det = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    out = np.zeros((height, width), np.int8)
    if det == 0:
        return out - 1
    for y in range(height):
        for x in range(width):
            qx, qy = Fraction(2 * x + 1, 2) - x0, Fraction(2 * y + 1, 2) - y0
            s, t = (qx * (y2 - y0) - (x2 - x0) * qy) / det, ((x1 - x0) * qy - qx * (y1 - y0)) / det
            u = 1 - s - t
            out[y, x] = 1 if (s > 0 and t > 0 and u > 0) else (-1 if (s < 0 or t < 0 or u < 0) else 0)
    return out


def rasterize(xy, zcam, faces, width, height, znear=0.05, zfar=100.0, cull=True):
    """Snapped coordinates int [V,2] + zcam [V] + faces [F,3] -> dict(face int32 [H,W] (-1 background), depth fp64 [H,W] (inf),
    second fp64 [H,W]: the depth of the next nearest sample of ANOTHER face (inf when there is none)).  Equal depths go to the
    lower face id."""
    xy, zc = np.asarray(xy, np.int64), np.asarray(zcam, np.float64)
    face = np.full((height, width), -1, np.int32)
    depth = np.full((height, width), np.inf)
    second = np.full((height, width), np.inf)
    for f, tri in enumerate(np.asarray(faces, np.int64)):
        z0, z1, z2 = zc[tri]
        s = triangle_samples(xy[tri], (z0, z1, z2), width, height, cull)
        if s is None:
            continue
        ys, xs, w1, w2, area = s
        z = z0 + (w1 / area) * (z1 - z0) + (w2 / area) * (z2 - z0)
        keep = (z >= znear) & (z <= zfar)
        ys, xs, z = ys[keep], xs[keep], z[keep]
        old = depth[ys, xs]
        win = z < old                                        # faces come in ascending order: a tie stays with the lower id
        second[ys, xs] = np.where(win, old, np.minimum(second[ys, xs], z))
        depth[ys[win], xs[win]] = z[win]
        face[ys[win], xs[win]] = f
    return dict(face=face, depth=depth, second=second)


def render_world(verts, affine, faces, width, height, **kw):
    xy, zc = snap(verts, affine)
    return rasterize(xy, zc, faces, width, height, **kw)


def vertex_normals(verts, faces):
    """fp64 smooth normals [V,3]: normalise(sum over the vertex's faces of cross(p1 - p0, p2 - p0)), each face once per vertex; zero
    for a vertex without faces (or whose faces cancel)."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    with np.errstate(invalid='ignore'):                       # a non-finite vertex spoils its own faces' vertices only
        fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        n = np.zeros_like(v)
        for f_id, tri in enumerate(f):
            for vid in set(int(t) for t in tri):
                n[vid] += fn[f_id]
        l = np.linalg.norm(n, axis=1, keepdims=True)
        return np.divide(n, l, out=np.zeros_like(n), where=l > 0)


def shade(face, xy, faces, normals, light, color=(220, 220, 220), background=(255, 255, 255), ambient=0.0, gain=4.0 / np.pi):
    """face int [H,W] + snapped coordinates + fp64 vertex normals -> uint8 [H,W,3]:
    c = min(1, color / 255 (ambient + gain max(0, n . light))), u8 = floor(255 c + 0.5), n the normalised barycentric blend."""
    H, W = face.shape
    out = np.empty((H, W, 3), np.uint8)
    out[:] = np.asarray(background, np.uint8)
    ys, xs = np.nonzero(face >= 0)
    if ys.size == 0:
        return out
    tri = np.asarray(faces, np.int64)[face[ys, xs]]
    p = np.asarray(xy, np.int64)
    (x0, y0), (x1, y1), (x2, y2) = [(p[tri[:, k], 0], p[tri[:, k], 1]) for k in range(3)]
    px, py = 256 * xs.astype(np.int64) + 128, 256 * ys.astype(np.int64) + 128
    area = edge(x0, y0, x1, y1, x2, y2).astype(np.float64)
    b1, b2 = edge(x2, y2, x0, y0, px, py) / area, edge(x0, y0, x1, y1, px, py) / area
    n = (1 - b1 - b2)[:, None] * normals[tri[:, 0]] + b1[:, None] * normals[tri[:, 1]] + b2[:, None] * normals[tri[:, 2]]
    l = np.linalg.norm(n, axis=1)
    ndl = np.divide(n @ np.asarray(light, np.float64), l, out=np.zeros_like(l), where=l > 0)
    lit = ambient + gain * np.maximum(0.0, ndl)
    c = np.minimum(1.0, np.asarray(color, np.float64)[None, :] / 255.0 * lit[:, None])
    out[ys, xs] = np.floor(255.0 * c + 0.5).astype(np.uint8)
    return out


def read_bmp(path):
    """24-bit uncompressed BMP -> uint8 [H,W,3] RGB, row 0 on top (the parser of the tests; PIL is used as well where it imports)."""
    b = open(path, 'rb').read()
    magic, size, _, _, off, hdr, W, H, planes, bpp, comp = struct.unpack('<2sIHHIIiiHHI', b[:34])
    assert magic == b'BM' and size == len(b) and hdr == 40 and planes == 1 and bpp == 24 and comp == 0 and H > 0
    row = (3 * W + 3) // 4 * 4
    a = np.frombuffer(b, np.uint8, row * H, off).reshape(H, row)[::-1, :3 * W].reshape(H, W, 3)
    return a[:, :, ::-1].copy()


# ---- meshes of the tests -------------------------------------------------------------------------------------------------------
def octahedron(level=4, radius=0.5, centre=(0.0, 1.0, 0.0), squash=(1.0, 1.0, 1.0)):
    """A closed, outward-oriented subdivided octahedron pushed onto an ellipsoid: 8 * 4^level faces."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.asarray(p, np.float64) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                q = v[a] + v[b]
                v.append(q / np.linalg.norm(q))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    v = np.stack(v) * radius * np.asarray(squash) + np.asarray(centre)
    return v, np.asarray(f, np.int64)

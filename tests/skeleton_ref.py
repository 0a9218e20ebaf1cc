"""numpy / Python-int restatement of the capsule rasteriser ``mc_skeleton_*`` (the header comment of csrc/mc_skeleton.hip): the scene of
``plot_3d_motion``, the fp64 projection and the snap, exact capsule and triangle coverage, the layer maximum and the palette.  It is
the yardstick of ``test_skeleton_host.py`` (which checks the restatement's own properties) and ``test_skeleton_gpu.py`` (which holds
the kernels to it).

Screen space: x to the right, y DOWN (row 0 on top), coordinates snapped to 1/16 px.  The sample of pixel (x, y) is its centre
P = (16 x + 8, 16 y + 8).  Layers: 0 background, 1 plane, 2 trail, 3 + c chain c; a pixel's layer is the maximum that covers it.
"""
import numpy as np

UNIT = 16
GUARD = 1 << 17
INVALID = -2 ** 31
BIG = 1 << 28


# ---- the scene -----------------------------------------------------------------------------------------------------------------
def sequence_stats(joints):
    """fp32 [n,J,3] of ONE sequence -> MINS [3], MAXS [3] (fp32, over the finite values; +inf / -inf when there is none) and traj fp32
    [n,2], the root's (x, z)."""
    j = np.asarray(joints, np.float32)
    mins, maxs = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    for a in range(3):
        v = j[:, :, a][np.isfinite(j[:, :, a])]
        if v.size:
            mins[a], maxs[a] = v.min(), v.max()
    return mins, maxs, j[:, 0, [0, 2]].copy()


def frame_points(joints, i, mins, maxs):
    """Frame i of one sequence -> fp32 p' of its J joints + 4 plane corners [J + 4,3] and of its trail points [i,3] (none for i < 2):
    one fp32 subtraction per axis."""
    j = np.asarray(joints, np.float32)
    off = np.array([j[i, 0, 0], mins[1], j[i, 0, 2]], np.float32)
    corners = np.array([[mins[0], mins[1], mins[2]], [mins[0], mins[1], maxs[2]], [maxs[0], mins[1], maxs[2]], [maxs[0], mins[1], mins[2]]], np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        body = np.concatenate([j[i], corners]) - off
        m = i if i >= 2 else 0
        trail = np.stack([j[:m, 0, 0], np.full(m, mins[1], np.float32), j[:m, 0, 2]], axis=1).astype(np.float32) - off
    return body.astype(np.float32), trail.astype(np.float32)


def project64(points, S):
    """p' [m,3] and the screen matrix, both taken to fp64 -> (sx, sy, h_w) in pixels, no snap."""
    p = np.asarray(points, np.float64)
    s = np.asarray(S, np.float64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        h = p @ s[:, :3].T + s[:, 3]
        return h[:, 0] / h[:, 3], h[:, 1] / h[:, 3], h[:, 3]


def snap(points, S):
    """fp64 projection of the fp32 p' -> int64 [m,2]; both coordinates ``INVALID`` when a component is not finite, h_w <= 0 or the
    snapped value lies beyond the guard band."""
    p = np.asarray(points, np.float64)
    sx, sy, hw = project64(p, S)
    with np.errstate(invalid='ignore', over='ignore'):
        q = np.floor(UNIT * np.stack([sx, sy], axis=1) + 0.5)
        ok = np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1) & np.isfinite(hw) & (hw > 0)
        ok &= (np.abs(np.where(np.isfinite(q), q, 0)) <= GUARD).all(axis=1)
    return np.where(ok[:, None], np.where(ok[:, None], q, 0), INVALID).astype(np.int64)


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def capsule_covers(a, b, R, p):
    """The three rules in Python integers (unbounded): is the sample ``p`` covered by the capsule a -> b of radius R?"""
    (ax, ay), (bx, by), (px, py) = [(int(v[0]), int(v[1])) for v in (a, b, p)]
    dx, dy, ex, ey = bx - ax, by - ay, px - ax, py - ay
    dd, t = dx * dx + dy * dy, ex * dx + ey * dy
    if t <= 0:
        return ex * ex + ey * ey <= R * R
    if t >= dd:
        return (px - bx) ** 2 + (py - by) ** 2 <= R * R
    cross = dx * ey - dy * ex
    return cross * cross <= R * R * dd


def _centres(width, height):
    py, px = np.meshgrid(UNIT * np.arange(height, dtype=np.int64) + UNIT // 2, UNIT * np.arange(width, dtype=np.int64) + UNIT // 2, indexing='ij')
    return px, py


def capsule_mask(a, b, R, width, height):
    """bool [H,W], the same rules in int64: R^2 dd < 2^56, so |cross| >= 2^28 is "not covered" and nothing else overflows
    (``test_skeleton_host`` holds this to ``capsule_covers``)."""
    (ax, ay), (bx, by) = [(int(v[0]), int(v[1])) for v in (a, b)]
    assert max(abs(ax), abs(ay), abs(bx), abs(by)) <= GUARD and 0 < R <= 512
    out = np.zeros((height, width), bool)
    # only the pixels whose centres lie in the segment's box grown by R can be covered: 16 p + 8 in [lo - R, hi + R]
    x0, x1 = max(-((8 - (min(ax, bx) - R)) // 16), 0), min((max(ax, bx) + R - 8) // 16, width - 1)
    y0, y1 = max(-((8 - (min(ay, by) - R)) // 16), 0), min((max(ay, by) + R - 8) // 16, height - 1)
    if x0 > x1 or y0 > y1:
        return out
    py, px = np.meshgrid(UNIT * np.arange(y0, y1 + 1, dtype=np.int64) + 8, UNIT * np.arange(x0, x1 + 1, dtype=np.int64) + 8, indexing='ij')
    dx, dy, ex, ey = bx - ax, by - ay, px - ax, py - ay
    dd, t = dx * dx + dy * dy, ex * dx + ey * dy
    cross = np.abs(dx * ey - dy * ex)
    small = np.where(cross < BIG, cross, 0)
    side = (cross < BIG) & (small * small <= R * R * dd)
    out[y0:y1 + 1, x0:x1 + 1] = np.where(t <= 0, ex * ex + ey * ey <= R * R,
                                         np.where(t >= dd, (px - bx) ** 2 + (py - by) ** 2 <= R * R, side))
    return out


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _bias(ax, ay, bx, by, sign):
    dx, dy = (bx - ax) * sign, (by - ay) * sign
    return 0 if (dy < 0 or (dy == 0 and dx > 0)) else -1      # a top or a left edge owns the samples on it


def triangle_mask(xy, width, height):
    """bool [H,W]: int64 edge functions and the top-left rule, no culling, zero area dropped."""
    (x0, y0), (x1, y1), (x2, y2) = [(int(p[0]), int(p[1])) for p in xy]
    area = edge(x0, y0, x1, y1, x2, y2)
    if area == 0:
        return np.zeros((height, width), bool)
    sign = 1 if area > 0 else -1
    px, py = _centres(width, height)
    w0, w1, w2 = edge(x1, y1, x2, y2, px, py), edge(x2, y2, x0, y0, px, py), edge(x0, y0, x1, y1, px, py)
    return ((sign * w0 + _bias(x1, y1, x2, y2, sign) >= 0) & (sign * w1 + _bias(x2, y2, x0, y0, sign) >= 0)
            & (sign * w2 + _bias(x0, y0, x1, y1, sign) >= 0))


def _valid(*pts):
    return all(int(p[0]) != INVALID and int(p[1]) != INVALID for p in pts)


def frame_layers(screen, trail, segments, trail_radius, width, height):
    """One frame from snapped points: ``screen`` int [J + 4,2] (joints, then the plane's corners), ``trail`` int [m,2] (the frame's
    trail points, m = 0 or i), ``segments`` (joint a, joint b, radius, layer) -> uint8 [H,W].  A primitive with an invalid vertex
    is dropped."""
    screen, trail = np.asarray(screen, np.int64), np.asarray(trail, np.int64).reshape(-1, 2)
    J = screen.shape[0] - 4
    layer = np.zeros((height, width), np.uint8)
    put = lambda mask, l: np.maximum(layer, np.where(mask, l, 0).astype(np.uint8), out=layer)
    c = screen[J:]
    for tri in ((c[0], c[1], c[2]), (c[0], c[2], c[3])):
        if _valid(*tri):
            put(triangle_mask(tri, width, height), 1)
    for k in range(len(trail) - 1):
        if _valid(trail[k], trail[k + 1]):
            put(capsule_mask(trail[k], trail[k + 1], trail_radius, width, height), 2)
    for a, b, R, l in segments:
        if _valid(screen[a], screen[b]):
            put(capsule_mask(screen[a], screen[b], R, width, height), l)
    return layer


def layers_from_buffers(screen, trail_screen, lens, segments, trail_radius, width, height):
    """All frames from the snapped points of every frame (``screen`` [n,J + 4,2], ``trail_screen`` [n,longest,2]; sequences of
    ``lens`` frames one after the other): frame i of a sequence takes its first i trail points when i >= 2."""
    out, g = [], 0
    for n in lens:
        for i in range(n):
            out.append(frame_layers(screen[g], trail_screen[g, :i] if i >= 2 else np.zeros((0, 2), np.int64), segments, trail_radius, width, height))
            g += 1
    return np.stack(out) if out else np.zeros((0, height, width), np.uint8)


def render(joints, lens, S, segments, trail_radius, width, height):
    """The whole restatement from world joints, projected in fp64: dict(layer uint8 [n,H,W], screen int64 [n,J + 4,2], trails: list of
    int64 [m,2], stats fp32 [S,6], traj fp32 [n,2])."""
    j = np.asarray(joints, np.float32)
    layers, screens, trails, stats, trajs, g = [], [], [], [], [], 0
    for n in lens:
        seq = j[g:g + n]
        mins, maxs, traj = sequence_stats(seq)
        stats.append(np.concatenate([mins, maxs]))
        trajs.append(traj)
        for i in range(n):
            body, trail = frame_points(seq, i, mins, maxs)
            sb, st = snap(body, S), snap(trail, S).reshape(-1, 2)
            layers.append(frame_layers(sb, st, segments, trail_radius, width, height))
            screens.append(sb)
            trails.append(st)
        g += n
    return dict(layer=np.stack(layers), screen=np.stack(screens), trails=trails, stats=np.stack(stats), traj=np.concatenate(trajs))


# ---- helpers of the tests ------------------------------------------------------------------------------------------------------
def unproject(S64, sx, sy, y):
    """The world point at height ``y`` that the fp64 screen matrix sends to the pixel position (sx, sy): solves the two linear
    equations (S_0 - sx S_3) . (p, 1) = 0 and (S_1 - sy S_3) . (p, 1) = 0 for (x, z)."""
    s = np.asarray(S64, np.float64)
    r0, r1 = s[0] - sx * s[3], s[1] - sy * s[3]
    a = np.array([[r0[0], r0[2]], [r1[0], r1[2]]])
    rhs = -np.array([r0[1] * y + r0[3], r1[1] * y + r1[3]])
    x, z = np.linalg.solve(a, rhs)
    return np.array([x, y, z])


def eye_world(cam):
    """The eye of an ``Mplot3dCamera`` in data coordinates (where h_w = 0 passes through)."""
    e, a = np.deg2rad(cam.elev), np.deg2rad(cam.azim)
    ps = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    box = 0.5 * cam.box + cam.dist * ps * cam.focal_length
    return cam.limits[:, 0] + box * (cam.limits[:, 1] - cam.limits[:, 0]) / cam.box

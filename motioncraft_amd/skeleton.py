"""Draw HumanML3D / KIT skeleton animations on the device: the picture the reference's text-to-motion tool ends with.

``tools/visualize.py`` (``plot_t2m``, :46-56) recovers the joints, filters them and hands them to ``plot_3d_motion``
(mogen/utils/plot_utils.py:107-204), which draws every frame with matplotlib's ``mplot3d`` inside a ``FuncAnimation``: a grey ground
quad, the root's trail and one polyline per kinematic chain, under ``view_init(elev=120, azim=-90)`` at ``dist = 7.5``.
``SkeletonRenderer`` draws the same scene with the HIP capsule rasteriser ``mc_skeleton_*`` (``csrc/mc_skeleton.hip``, whose header
comment defines every rule) from the joints ``postprocess.recover_joints*`` leaves on the device.

The camera is mplot3d's ``Axes3D.get_proj`` restated in fp64 (``Mplot3dCamera``).  NOT drawn: the title text, anti-aliasing and
mplot3d's projecting line caps -- every segment is a capsule with round caps, which gives round joins.  Pixel parity with
matplotlib's Agg output is not claimed.
"""
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _p, stream as _stream

DEFAULT_WORK_BYTES = 64 << 20
MAX_SIZE = _lib.MC_SKELETON_MAX_SIZE               # the rasteriser's viewport limit, in pixels
MAX_CHAINS = _lib.SKELETON_MAX_LAYERS - 3
MIN_RADIUS, MAX_RADIUS = _lib.MC_SKELETON_MIN_RADIUS, _lib.MC_SKELETON_MAX_RADIUS       # of a capsule, in sixteenths of a pixel
INVALID = -2 ** 31                                 # both coordinates of a point that was dropped

# matplotlib's named colours, as RGB
NAMED_COLORS = dict(red=(255, 0, 0), blue=(0, 0, 255), black=(0, 0, 0), darkblue=(0, 0, 139), darkred=(139, 0, 0), white=(255, 255, 255))
CHAIN_COLORS = ('red', 'blue', 'black', 'red', 'blue') + ('darkblue',) * 5 + ('darkred',) * 5      # plot_utils.py:152-156, cycled here
CHAIN_WIDTHS_PT = (4.0,) * 5                       # chains 0-4; 2.0 pt beyond (plot_utils.py:183-186)
THIN_WIDTH_PT, TRAIL_WIDTH_PT = 2.0, 1.0


def chains_from_parents(parents, leaves):
    """The polylines that draw a skeleton: for every joint of ``leaves``, in this order, walk towards the root and stop at the root or
    at the first joint an earlier chain has already drawn; the chain runs from there down to the leaf."""
    drawn, chains = set(), []
    for leaf in leaves:
        chain, j = [leaf], leaf
        while parents[j] >= 0 and j not in drawn:
            j = parents[j]
            chain.append(j)
            if j in drawn:
                break
        drawn.update(chain)
        chains.append(chain[::-1])
    return chains


# parent of every joint; the leaves in the reference's drawing order: legs, spine and head, arms
T2M_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19)                  # the 22 SMPL body joints
KIT_PARENTS = (-1, 0, 1, 2, 3, 3, 5, 6, 3, 8, 9, 0, 11, 12, 13, 14, 0, 16, 17, 18, 19)                   # the 21 KIT joints
T2M_CHAINS = chains_from_parents(T2M_PARENTS, (11, 10, 15, 21, 20))
KIT_CHAINS = chains_from_parents(KIT_PARENTS, (15, 20, 4, 7, 10))


def _norm_angle(deg):
    a = (deg + 360.0) % 360.0
    return a - 360.0 if a > 180.0 else a


class Mplot3dCamera:
    """``Axes3D.get_proj`` of matplotlib's mplot3d, restated in fp64, with the reference's view as the default.

    The data limits are ``x in +-radius/4`` and ``y, z in [0, radius/2]`` (plot_utils.py:132-135); data z is mplot3d's vertical axis and
    the reference passes the motion's (x, y, z) straight through, so at ``elev = 120, azim = -90`` the motion's height runs up the
    screen.  ``M = persp(-dist, dist, focal_length) . view_uvw(eye_focal) . world(limits, box)`` exactly as ``get_proj`` composes it.

    ``box_aspect`` is scaled to the length ``box_scale`` as ``Axes3D.set_box_aspect`` does.  The default 1.8294640721620434 is the
    constant of matplotlib before 3.9, which the reference used; 3.9 and later multiply it by another 25/24.  ``box_scale=None`` takes
    ``box_aspect`` as it is (what ``ax._box_aspect`` holds).

    ``view`` is the 2-D window (x0, x1, y0, y1) of projected coordinates that fills the axes, the ``viewLim`` that
    ``Axes3D.set_top_view`` leaves.  The reference builds the axes at the initial ``dist = 10`` and only then sets 7.5, so the default
    is the window of 10: (-0.095, 0.09, -0.095, 0.09).  The axes fill the figure and keep a square box, centred, as ``apply_aspect``
    does for a figure that is not square."""

    def __init__(self, elev=120, azim=-90, dist=7.5, focal_length=1, radius=4, box_aspect=(4, 4, 3), box_scale=1.8294640721620434,
                 view=(-0.095, 0.09, -0.095, 0.09), limits=None):
        if limits is None:
            limits = ((-radius / 4, radius / 4), (0, radius / 2), (0, radius / 2))
        lim = np.asarray(limits, np.float64)
        ba = np.asarray(box_aspect, np.float64)
        vw = np.asarray(view, np.float64)
        if lim.shape != (3, 2) or not np.isfinite(lim).all() or not (lim[:, 1] != lim[:, 0]).all():
            raise ValueError(f'limits must be three finite (low, high) pairs with low != high, got {limits!r}')
        if ba.shape != (3,) or not (np.isfinite(ba).all() and (ba > 0).all()):
            raise ValueError(f'box_aspect must be three positive numbers, got {box_aspect!r}')
        if box_scale is not None and not (box_scale > 0 and math.isfinite(box_scale)):
            raise ValueError(f'box_scale must be positive or None, got {box_scale!r}')
        if vw.shape != (4,) or not np.isfinite(vw).all() or not (vw[1] > vw[0] and vw[3] > vw[2]):
            raise ValueError(f'view must be (x0, x1, y0, y1) with x0 < x1 and y0 < y1, got {view!r}')
        if not (dist > 0 and math.isfinite(dist) and focal_length > 0 and math.isfinite(focal_length)):
            raise ValueError(f'dist and focal_length must be positive and finite (perspective only), got {dist} and {focal_length}')
        if not (math.isfinite(elev) and math.isfinite(azim)):
            raise ValueError(f'elev and azim must be finite, got {elev} and {azim}')
        self.elev, self.azim, self.dist, self.focal_length = float(elev), float(azim), float(dist), float(focal_length)
        self.limits, self.view = lim, vw
        self.box = ba * (box_scale / np.linalg.norm(ba)) if box_scale is not None else ba

    def proj_matrix64(self):
        """fp64 [4,4]: what ``ax.get_proj()`` returns."""
        (xmin, xmax), (ymin, ymax), (zmin, zmax) = self.limits
        dx, dy, dz = (xmax - xmin) / self.box[0], (ymax - ymin) / self.box[1], (zmax - zmin) / self.box[2]
        world = np.array([[1 / dx, 0, 0, -xmin / dx], [0, 1 / dy, 0, -ymin / dy], [0, 0, 1 / dz, -zmin / dz], [0, 0, 0, 1]])
        centre = 0.5 * self.box
        e, a = np.deg2rad(self.elev), np.deg2rad(self.azim)
        ps = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
        eye = centre + self.dist * ps
        # past +-90 degrees of elevation the plot is upside down and the vertical axis is reversed
        up = np.array([0.0, 0.0, -1.0 if abs(np.deg2rad(_norm_angle(self.elev))) > np.pi / 2 else 1.0])
        w = eye - centre
        w = w / np.linalg.norm(w)                                  # out of the screen
        u = np.cross(up, w)
        u = u / np.linalg.norm(u)                                  # to the right
        v = np.cross(w, u)                                         # to the top
        rot, shift = np.eye(4), np.eye(4)
        rot[:3, :3] = [u, v, w]
        shift[:3, 3] = -(centre + self.dist * ps * self.focal_length)
        zfront, zback, f = -self.dist, self.dist, self.focal_length
        persp = np.array([[f, 0, 0, 0], [0, f, 0, 0], [0, 0, (zfront + zback) / (zfront - zback), -2 * (zfront * zback) / (zfront - zback)],
                          [0, 0, -1, 0]])
        return np.dot(persp, np.dot(np.dot(rot, shift), world))

    def screen_projective64(self, width, height):
        """fp64 [4,4]: world point (x, y, z, 1) -> (X_num, Y_num, depth, W); the pixel is sx = X_num / W, sy = Y_num / W with row 0 on
        top, and W > 0 in front of the eye."""
        m = self.proj_matrix64()
        x0, x1, y0, y1 = self.view
        side = float(min(width, height))
        ox, oy = (width - side) / 2.0, (height - side) / 2.0
        s = np.empty((4, 4))
        s[0] = ox * m[3] + (side / (x1 - x0)) * (m[0] - x0 * m[3])
        s[1] = (oy + side) * m[3] - (side / (y1 - y0)) * (m[1] - y0 * m[3])
        s[2], s[3] = m[2], m[3]
        return s

    def screen_projective(self, width, height):
        """The fp32 matrix the kernel takes: computed in fp64, rounded once."""
        return self.screen_projective64(width, height).astype(np.float32)


def line_radius(width_px):
    """Radius of a ``width_px`` wide line in sixteenths of a pixel, from the fp32 width the library is given:
    ``max(12, floor(8 width_px + 0.5))``."""
    w = float(np.float32(width_px))
    if not (w > 0 and math.isfinite(w)) or math.floor(8.0 * w + 0.5) > MAX_RADIUS:
        raise ValueError(f'a line width must be positive and at most {MAX_RADIUS // 8} px, got {width_px!r}')
    return max(MIN_RADIUS, int(math.floor(8.0 * w + 0.5)))


def composite(color01, alpha, background):
    """``color01`` (0..1 per channel) at ``alpha`` over the uint8 ``background`` -> one uint8 RGB triple, rounded half up."""
    c, bg = np.asarray(color01, np.float64), np.asarray(background, np.float64) / 255.0
    return tuple(int(v) for v in np.floor(255.0 * (alpha * c + (1.0 - alpha) * bg) + 0.5))


def _colour(c, what):
    if isinstance(c, str):
        if c not in NAMED_COLORS:
            raise ValueError(f'{what}: unknown colour name {c!r} (known: {sorted(NAMED_COLORS)})')
        return NAMED_COLORS[c]
    a = np.asarray(c)
    if a.shape != (3,) or not np.all((a >= 0) & (a <= 255) & (a == np.round(a))):
        raise ValueError(f'{what} must be a colour name or three integers in 0..255, got {c!r}')
    return tuple(int(v) for v in a)


class SkeletonRenderer:
    """``SkeletonRenderer(chains)``; ``.render(joints)`` -> uint8 [n, H, W, 3] on the joints' device and current stream.

    ``chains``: lists of joint indices, one polyline each (``T2M_CHAINS``, ``KIT_CHAINS``, or any other list, e.g. the 52-joint body
    with hand chains).  The defaults are the reference's figure: 1000 x 1000 (``figsize`` 10 x 10 at 100 dpi), chains 4 pt wide for the
    first five and 2 pt beyond in red, blue, black, red, blue, five dark blue and five dark red (cycled), a blue 1 pt trail, the plane
    (0.5, 0.5, 0.5) at alpha 0.5 composited over the white background here, on the host.  A line of ``pt`` points is
    ``pt * dpi / 72`` pixels wide.  The native object is created at the first ``render``; ``close()`` frees it."""

    def __init__(self, chains, width=1000, height=1000, dpi=100, camera=None, num_joints=None, colors=None, widths_pt=None,
                 trail_color='blue', trail_width_pt=TRAIL_WIDTH_PT, plane_color=(0.5, 0.5, 0.5), plane_alpha=0.5, background=(255, 255, 255)):
        try:
            chains = [[int(j) for j in c] for c in chains]
        except (TypeError, ValueError):
            raise ValueError('chains must be lists of joint indices') from None
        if not 1 <= len(chains) <= MAX_CHAINS or any(len(c) < 2 for c in chains) or any(j < 0 for c in chains for j in c):
            raise ValueError(f'chains must be 1..{MAX_CHAINS} lists of at least 2 joint indices >= 0 each')
        J = max(j for c in chains for j in c) + 1 if num_joints is None else int(num_joints)
        if J > 65536 or any(j >= J for c in chains for j in c):
            raise ValueError(f'num_joints={J}: the chains name joints up to {max(j for c in chains for j in c)} (at most 65536 joints)')
        for name, v in (('width', width), ('height', height)):
            if not (isinstance(v, (int, np.integer)) and 1 <= v <= MAX_SIZE):
                raise ValueError(f'{name} must be an integer in 1..{MAX_SIZE}, got {v!r}')
        if not (dpi > 0 and math.isfinite(dpi)):
            raise ValueError(f'dpi must be positive, got {dpi!r}')
        if camera is not None and not isinstance(camera, Mplot3dCamera):
            raise ValueError(f'camera must be an Mplot3dCamera, got {type(camera).__name__}')
        if not 0 <= plane_alpha <= 1 or np.asarray(plane_color).shape != (3,) or not np.all((np.asarray(plane_color) >= 0) & (np.asarray(plane_color) <= 1)):
            raise ValueError('plane_color must be three numbers in 0..1 and plane_alpha in 0..1')
        n = len(chains)
        if colors is None:
            colors = [CHAIN_COLORS[c % len(CHAIN_COLORS)] for c in range(n)]
        if widths_pt is None:
            widths_pt = [CHAIN_WIDTHS_PT[c] if c < len(CHAIN_WIDTHS_PT) else THIN_WIDTH_PT for c in range(n)]
        if len(colors) != n or len(widths_pt) != n:
            raise ValueError(f'colors and widths_pt must have one entry per chain ({n})')
        self.chains, self.num_joints, self.width, self.height, self.dpi = chains, J, int(width), int(height), float(dpi)
        self.camera = camera if camera is not None else Mplot3dCamera()
        self.background = _colour(background, 'background')
        self.chain_width_px = np.array([w * self.dpi / 72.0 for w in widths_pt], np.float32)
        self.trail_width_px = np.float32(trail_width_pt * self.dpi / 72.0)
        self.chain_radius = [line_radius(w) for w in self.chain_width_px]
        self.trail_radius = line_radius(self.trail_width_px)
        # layer -> colour: background, plane, trail, chains
        self.palette = np.array([self.background, composite(plane_color, plane_alpha, self.background), _colour(trail_color, 'trail_color')]
                                + [_colour(c, 'colors') for c in colors], np.uint8)
        self._native = None

    def segments(self):
        """(joint a, joint b, radius, layer) of every chain segment, in drawing order."""
        return [(c[k], c[k + 1], self.chain_radius[i], 3 + i) for i, c in enumerate(self.chains) for k in range(len(c) - 1)]

    def params(self):
        """The ``mc_skeleton_params`` of this scene."""
        p = _lib.SkeletonParams()
        p.screen[:] = [float(v) for v in self.camera.screen_projective(self.width, self.height).reshape(-1)]
        p.width, p.height = self.width, self.height
        return p

    def native(self):
        if self._native is None:
            as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            flat = np.array([j for c in self.chains for j in c], np.int32)
            start = np.cumsum([0] + [len(c) for c in self.chains]).astype(np.int32)
            self._native = _lib.NativeObject('skeleton', as_p(flat), as_p(start), len(self.chains), self.num_joints, as_p(self.chain_width_px),
                                             ctypes.c_float(float(self.trail_width_px)), as_p(np.ascontiguousarray(self.palette)))
        return self._native

    def close(self):
        if self._native is not None:
            self._native.close()
            self._native = None

    def render(self, joints, lengths=None, work_bytes=DEFAULT_WORK_BYTES, return_buffers=False):
        """``joints`` fp32 [n, J, 3] on the device -> uint8 [n, H, W, 3].  ``lengths``: the frame counts of the sequences the rows hold,
        one after the other (default: one sequence); each has its own ground quad, trail and height offset.  With
        ``return_buffers`` a dict: ``rgb``, ``layer`` uint8 [n, H, W], ``screen`` int32 [n, J + 4, 2] (joints, then the plane's corners,
        in sixteenths of a pixel; ``INVALID`` twice for a dropped point), ``trail_screen`` int32 [n, longest, 2], ``stats`` fp32
        [sequences, 6] (MINS, MAXS) and ``traj`` fp32 [n, 2].  Frames run in chunks that fit ``work_bytes`` of scratch (raised to one
        frame's need); the result does not depend on it."""
        if not isinstance(joints, torch.Tensor) or joints.dtype != torch.float32:
            raise ValueError(f'joints must be a float32 tensor, got {getattr(joints, "dtype", type(joints).__name__)}')
        if joints.dim() != 3 or tuple(joints.shape[1:]) != (self.num_joints, 3):
            raise ValueError(f'joints must be [n, {self.num_joints}, 3], got {tuple(joints.shape)}')
        n = joints.shape[0]
        if n > 2 ** 31 - 1:
            raise ValueError(f'joints: {n} frames are more than one call takes')
        lens = [n] if lengths is None else [int(v) for v in torch.as_tensor(lengths).reshape(-1)]
        if any(v < 0 for v in lens) or sum(lens) != n:
            raise ValueError(f'lengths must be non-negative and add up to the {n} frames of joints, got {lens}')
        if not (isinstance(work_bytes, (int, np.integer)) and work_bytes >= 0):
            raise ValueError(f'work_bytes must be a non-negative integer, got {work_bytes!r}')
        if not joints.is_cuda:
            raise ValueError('joints must be in device (HBM) memory: there is no host renderer')
        obj = self.native()
        x = joints.contiguous()
        dev, H, W, J = x.device, self.height, self.width, self.num_joints
        seq_start = np.cumsum([0] + lens).astype(np.int32)
        longest = max(lens) if lens else 0
        rgb = torch.empty(n, H, W, 3, device=dev, dtype=torch.uint8)
        out = dict(rgb=rgb)
        if return_buffers:
            out.update(layer=torch.empty(n, H, W, device=dev, dtype=torch.uint8), screen=torch.empty(n, J + 4, 2, device=dev, dtype=torch.int32),
                       trail_screen=torch.empty(n, longest, 2, device=dev, dtype=torch.int32),
                       stats=torch.empty(len(lens), 6, device=dev, dtype=torch.float32), traj=torch.empty(n, 2, device=dev, dtype=torch.float32))
        if n:
            need = lambda frames: int(obj.lib.mc_skeleton_work_bytes(obj.handle, frames, longest, W, H))
            wb = max(min(int(work_bytes), need(n)), need(1))
            work = torch.empty(wb, device=dev, dtype=torch.uint8)
            p = self.params()
            with torch.cuda.device(dev):
                _lib.check(obj.lib.mc_skeleton_frames(obj.handle, _p(x), seq_start.ctypes.data_as(ctypes.c_void_p), len(lens), ctypes.byref(p),
                                                      _p(work), wb, _p(rgb), _p(out.get('layer')), _p(out.get('screen')),
                                                      _p(out.get('trail_screen')), _p(out.get('stats')), _p(out.get('traj')),
                                                      _stream(dev)), 'mc_skeleton_frames')
        return out if return_buffers else rgb

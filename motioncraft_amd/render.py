"""Render SMPL-X meshes on the device: the frames the reference's tools end with.

``tools/visualize.py``, ``tools/s2g_visualize.py`` and ``tools/m2d_visualize.py`` hand the body model's vertices to
``fast_render.generate_silent_videos*`` (mogen/datasets/EMAGE_2024/utils/fast_render.py:13-81, other_tools.py:695-765): a grey mesh
under ``pyrender.OrthographicCamera(xmag=1.0, ymag=1.0)`` and one ``DirectionalLight(intensity=4.0)``, drawn by pyrender + osmesa in
eight host processes, written as ``frame_%d.<ext>`` and joined by ffmpeg.  ``MeshRenderer`` draws the same scene with the HIP
rasteriser ``mc_render_*`` (``csrc/mc_render.hip``) from the vertices ``body_model.SMPLXBodyModel.vertices`` leaves on the device.

Camera, framing and geometry are the reference's.  The COLOURS are this project's definition -- a clamped Lambert term over smooth
normals (``include/motioncraft_amd.h``) -- not pyrender's physically based shader, whose output could not be pinned.  Orthographic
camera only; no textures, shadows, perspective or anti-aliasing.
"""
import ctypes
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _p

DEFAULT_WORK_BYTES = 256 << 20
MAX_SIZE = _lib.MC_RENDER_MAX_SIZE                 # the rasteriser's guard band, in pixels


def _rot_x_pose(angle_deg, ty, tz):
    a = angle_deg * np.pi / 180
    return np.array([[1.0, 0.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a), ty], [0.0, np.sin(a), np.cos(a), tz], [0.0, 0.0, 0.0, 1.0]])


def reference_camera_pose(angle_deg=-2):
    """``create_pose_camera`` (fast_render.py:16-24): pitched about x, at (0, 1, 5)."""
    return _rot_x_pose(angle_deg, 1.0, 5.0)


def reference_light_pose(angle_deg=-30):
    """``create_pose_light`` (fast_render.py:26-33): pitched about x, at (0, 0, 3)."""
    return _rot_x_pose(angle_deg, 0.0, 3.0)


def _pose(pose, what):
    m = np.asarray(pose, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise ValueError(f'{what}: pose must be a finite 4x4 matrix, got shape {m.shape}')
    return m


class OrthographicCamera:
    """Looks along the pose's -Z with +Y up.  ``ndc_x = x_cam / xmag``, ``ndc_y = y_cam / ymag`` with NO aspect correction, exactly as
    ``pyrender.OrthographicCamera`` with the reference's arguments: the default 1:1 magnification on a 4:3 viewport is the
    reference's framing (the body comes out 4/3 wider than tall in pixels per metre), and it is kept as the default for that
    reason.  ``pose`` must be a rigid transform (the reference's is)."""

    def __init__(self, xmag=1.0, ymag=1.0, znear=0.05, zfar=100.0, pose=None):
        if not (xmag > 0 and ymag > 0):
            raise ValueError(f'xmag and ymag must be positive, got {xmag} and {ymag}')
        if not 0 < znear <= zfar < math.inf:
            raise ValueError(f'znear and zfar must satisfy 0 < znear <= zfar < inf, got {znear} and {zfar}')
        self.xmag, self.ymag, self.znear, self.zfar = float(xmag), float(ymag), float(znear), float(zfar)
        self.pose = reference_camera_pose() if pose is None else _pose(pose, 'camera')

    def screen_affine64(self, width, height):
        """fp64 [3,4]: world point (x, y, z, 1) -> (column in pixels, row in pixels with row 0 on top, distance along the view)."""
        view = np.linalg.inv(self.pose)            # world -> camera
        a = np.empty((3, 4))
        a[0] = view[0] / self.xmag * (width / 2.0)              # xs = (ndc_x + 1) W / 2
        a[0, 3] += width / 2.0
        a[1] = -view[1] / self.ymag * (height / 2.0)            # ys = (1 - ndc_y) H / 2
        a[1, 3] += height / 2.0
        a[2] = -view[2]                                         # the camera looks along -Z
        return a

    def screen_affine(self, width, height):
        """The fp32 3x4 matrix the kernel takes: computed in fp64, rounded once."""
        return self.screen_affine64(width, height).astype(np.float32)


class DirectionalLight:
    """The direction TO the light is the pose's +Z column (pyrender's lights shine along -Z).  ``gain = intensity / pi`` is the Lambert
    term of a unit-albedo diffuse surface; ``ambient`` is added before the clamp."""

    def __init__(self, pose=None, intensity=4.0, ambient=0.0):
        if not (intensity >= 0 and ambient >= 0):
            raise ValueError(f'intensity and ambient must be >= 0, got {intensity} and {ambient}')
        self.pose = reference_light_pose() if pose is None else _pose(pose, 'light')
        self.intensity, self.ambient = float(intensity), float(ambient)
        d = self.pose[:3, 2]
        n = np.linalg.norm(d)
        if not n > 0:
            raise ValueError("light: the pose's Z column is zero")
        self.direction = d / n
        self.gain = self.intensity / math.pi


def vertex_face_adjacency(faces, num_vertices):
    """CSR vertex -> faces with the faces of every vertex in ascending order (a face that names a vertex twice is listed once):
    int32 ``start`` [V + 1] and ``adj`` [start[V]]."""
    f = np.asarray(faces, dtype=np.int64)
    pairs = np.unique(np.stack([f.reshape(-1), np.repeat(np.arange(f.shape[0]), 3)], axis=1), axis=0)     # sorted by vertex, then face
    start = np.zeros(num_vertices + 1, np.int64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=num_vertices), out=start[1:])
    return start.astype(np.int32), np.ascontiguousarray(pairs[:, 1], dtype=np.int32)


def _colour(c, what):
    a = np.asarray(c)
    if a.shape != (3,) or not np.all((a >= 0) & (a <= 255) & (a == np.round(a))):
        raise ValueError(f'{what} must be three integers in 0..255, got {c!r}')
    return [int(v) for v in a]


class MeshRenderer:
    """``MeshRenderer(faces, num_vertices)``; ``.render(vertices)`` -> uint8 [n, H, W, 3] on the vertices' device and current stream.
    The defaults are the reference's scene at ``render_video_width // 2`` x ``render_video_height`` = 960 x 720: its camera and
    light poses, mesh colour 220 and a white background; ``cull_backfaces`` because pyrender's default material is single-sided.
    ``large_threshold``: bounding-box pixels above which a triangle is walked by ``large_slices`` waves instead of one thread (None =
    the library's defaults, 1024 and 32, chosen from the sweep in DESIGN.md section 4g; the result depends on neither).  The native object is created at the first ``render``; ``close()`` frees it."""

    def __init__(self, faces, num_vertices, width=960, height=720, camera=None, light=None, color=(220, 220, 220),
                 background=(255, 255, 255), cull_backfaces=True, large_threshold=None, large_slices=None):
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in 'iu':
            raise ValueError(f'faces must be an integer array [F, 3] with F >= 1, got {f.dtype} {f.shape}')
        V = int(num_vertices)
        if V < 1 or f.min() < 0 or f.max() >= V:
            raise ValueError(f'num_vertices={num_vertices}: faces index vertices {int(f.min())}..{int(f.max())}')
        if f.shape[0] > 2 ** 31 - 1 or 3 * f.shape[0] > 2 ** 31 - 1:
            raise ValueError(f'faces: {f.shape[0]} triangles are more than the int32 tables hold')
        for name, v in (('width', width), ('height', height)):
            if not (isinstance(v, (int, np.integer)) and 1 <= v <= MAX_SIZE):
                raise ValueError(f'{name} must be an integer in 1..{MAX_SIZE}, got {v!r}')
        if camera is not None and not isinstance(camera, OrthographicCamera):
            raise ValueError(f'camera must be an OrthographicCamera (the only kind there is), got {type(camera).__name__}')
        if light is not None and not isinstance(light, DirectionalLight):
            raise ValueError(f'light must be a DirectionalLight, got {type(light).__name__}')
        if large_threshold is not None and not (isinstance(large_threshold, (int, np.integer)) and 1 <= large_threshold <= 2 ** 31 - 1):
            raise ValueError(f'large_threshold must be None or an integer in 1..2^31 - 1, got {large_threshold!r}')
        if large_slices is not None and not (isinstance(large_slices, (int, np.integer)) and 1 <= large_slices <= 1024):
            raise ValueError(f'large_slices must be None or an integer in 1..1024, got {large_slices!r}')
        self.faces = np.ascontiguousarray(f, dtype=np.int32)
        self.num_vertices, self.width, self.height = V, int(width), int(height)
        self.camera = camera if camera is not None else OrthographicCamera()
        self.light = light if light is not None else DirectionalLight()
        self.color, self.background = _colour(color, 'color'), _colour(background, 'background')
        self.cull_backfaces, self.large_threshold, self.large_slices = bool(cull_backfaces), large_threshold, large_slices
        self.adj_start, self.adj_faces = vertex_face_adjacency(self.faces, V)
        self._native, self._work = None, None

    def params(self):
        """The ``mc_render_params`` of this scene."""
        p = _lib.RenderParams()
        p.screen[:] = [float(v) for v in self.camera.screen_affine(self.width, self.height).reshape(-1)]
        p.light[:] = [float(v) for v in self.light.direction.astype(np.float32)]
        p.base[:] = [float(np.float32(c) / np.float32(255)) for c in self.color]
        p.ambient, p.gain = self.light.ambient, self.light.gain
        p.znear, p.zfar = self.camera.znear, self.camera.zfar
        p.background[:] = self.background
        p.width, p.height = self.width, self.height
        p.cull_backfaces, p.large_threshold = int(self.cull_backfaces), int(self.large_threshold or 0)
        p.large_slices = int(self.large_slices or 0)
        return p

    def native(self):
        if self._native is None:
            as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            self._native = _lib.NativeObject('render', as_p(self.faces), self.faces.shape[0], self.num_vertices, as_p(self.adj_start),
                                             as_p(self.adj_faces))
        return self._native

    def close(self):
        self._work = None
        if self._native is not None:
            self._native.close()
            self._native = None

    def render(self, vertices, work_bytes=DEFAULT_WORK_BYTES, return_buffers=False):
        """``vertices`` fp32 [n, V, 3] (or [V, 3]) on the device -> uint8 [n, H, W, 3]; with ``return_buffers`` also ``face`` int32
        [n, H, W] (-1 = background), ``depth`` fp32 [n, H, W] (inf = background), ``screen`` int32 [n, V, 2] (1/256 px) and ``zcam``
        fp32 [n, V].  Frames run in chunks that fit ``work_bytes`` of scratch (raised to one frame's need); the result does not
        depend on it.  The scratch is kept between calls -- its visibility keys are cleared once, every call leaves them clear --
        so one renderer serves one stream at a time."""
        if not isinstance(vertices, torch.Tensor) or vertices.dtype != torch.float32:
            raise ValueError(f'vertices must be a float32 tensor, got {getattr(vertices, "dtype", type(vertices).__name__)}')
        if vertices.dim() not in (2, 3) or tuple(vertices.shape[-2:]) != (self.num_vertices, 3):
            raise ValueError(f'vertices must be [n, {self.num_vertices}, 3], got {tuple(vertices.shape)}')
        if not vertices.is_cuda:
            raise ValueError('vertices must be in device (HBM) memory: there is no host renderer')
        if not (isinstance(work_bytes, (int, np.integer)) and work_bytes >= 0):
            raise ValueError(f'work_bytes must be a non-negative integer, got {work_bytes!r}')
        obj = self.native()
        v = vertices.reshape(-1, self.num_vertices, 3).contiguous()
        n, dev, H, W = v.shape[0], v.device, self.height, self.width
        if n > 2 ** 31 - 1:
            raise ValueError(f'vertices: {n} frames are more than one call takes')
        need = lambda frames: int(obj.lib.mc_render_work_bytes(obj.handle, frames, W, H))
        wb = max(min(int(work_bytes), need(max(n, 1))), need(1))
        stream = torch.cuda.current_stream(dev).cuda_stream
        tag = (dev, wb, stream)
        clean = self._work is not None and self._work[0] == tag
        if not clean:
            self._work = None                                           # a failed call below leaves no buffer that claims to be clean
            work = torch.empty(wb, device=dev, dtype=torch.uint8)
        else:
            work = self._work[1]
        rgb = torch.empty(n, H, W, 3, device=dev, dtype=torch.uint8)
        face = depth = screen = zcam = None
        if return_buffers:
            face, depth = torch.empty(n, H, W, device=dev, dtype=torch.int32), torch.empty(n, H, W, device=dev, dtype=torch.float32)
            screen = torch.empty(n, self.num_vertices, 2, device=dev, dtype=torch.int32)
            zcam = torch.empty(n, self.num_vertices, device=dev, dtype=torch.float32)
        if n == 0:                                                      # nothing to launch (and an empty tensor has no address)
            return (rgb, face, depth, screen, zcam) if return_buffers else rgb
        p = self.params()
        self._work = None
        with torch.cuda.device(dev):
            _lib.check(obj.lib.mc_render_frames(obj.handle, _p(v), n, ctypes.byref(p), _p(work), wb, int(clean), _p(rgb), _p(face), _p(depth),
                                                _p(screen), _p(zcam), ctypes.c_void_p(stream)), 'mc_render_frames')
        self._work = (tag, work)
        return (rgb, face, depth, screen, zcam) if return_buffers else rgb


def write_frames(frames, out_dir, prefix='frame_', filetype='bmp'):
    """uint8 [n, H, W, 3] (tensor or array, RGB, row 0 on top) -> ``out_dir/frame_0.bmp`` ..., the names ``fast_render`` writes before
    ffmpeg (fast_render.py:89): 24-bit uncompressed BMP written with the standard library alone.  Returns the paths."""
    if filetype != 'bmp':
        raise ValueError(f"filetype must be 'bmp' (written without an imaging library), got {filetype!r}")
    a = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f'frames must be uint8 [n, H, W, 3], got {a.dtype} {a.shape}')
    os.makedirs(out_dir, exist_ok=True)
    n, H, W, _ = a.shape
    row = (3 * W + 3) // 4 * 4                                          # rows are padded to 4 bytes and stored bottom-up, BGR
    header = struct.pack('<2sIHHIIiiHHIIiiII', b'BM', 54 + row * H, 0, 0, 54, 40, W, H, 1, 24, 0, row * H, 2835, 2835, 0, 0)
    paths = []
    for i in range(n):
        body = np.zeros((H, row), np.uint8)
        body[:, :3 * W] = a[i, ::-1, :, ::-1].reshape(H, 3 * W)
        path = os.path.join(out_dir, f'{prefix}{i}.{filetype}')
        with open(path, 'wb') as fh:
            fh.write(header)
            fh.write(body.tobytes())
        paths.append(path)
    return paths


def parse_size(text, what='--render_size'):
    """'960x720' -> (960, 720); ValueError naming ``what`` otherwise."""
    parts = str(text).lower().split('x')
    if len(parts) != 2 or not all(q.isdigit() for q in parts) or not all(1 <= int(q) <= MAX_SIZE for q in parts):
        raise ValueError(f'{what} must be WIDTHxHEIGHT with both in 1..{MAX_SIZE}, e.g. 960x720; got {text!r}')
    return int(parts[0]), int(parts[1])


def save_frames(frames, out_dir, fps, video_name='silence_video'):
    """``frames`` -> ``out_dir/frame_%d.bmp`` and, when there is an ffmpeg, ``out_dir/<video_name>.mp4`` at ``fps``
    (fast_render.py:236-237; unlike the reference the frames are kept).  Returns (frame paths, mp4 path or None)."""
    if not fps > 0:
        raise ValueError(f'fps must be positive, got {fps}')
    paths = write_frames(frames, out_dir)
    if shutil.which('ffmpeg') is None:
        return paths, None
    return paths, frames_to_mp4(os.path.join(out_dir, 'frame_%d.bmp'), os.path.join(out_dir, video_name + '.mp4'), fps)


def frames_to_mp4(pattern, out_path, fps):
    """``convert_img_to_mp4`` (mogen/datasets/EMAGE_2024/utils/media.py:24-33): an ``ffmpeg`` found on PATH, in a child process, with
    the reference's arguments.  Without one, RuntimeError: the frames are the result and stay where they are."""
    exe = shutil.which('ffmpeg')
    if exe is None:
        raise RuntimeError(f'no ffmpeg on PATH: keep the frames {pattern} and join them elsewhere '
                           f'(ffmpeg -framerate {fps} -i {pattern} -c:v libx264 -pix_fmt yuv420p {out_path})')
    subprocess.run([exe, '-framerate', str(fps), '-i', pattern, '-c:v', 'libx264', '-pix_fmt', 'yuv420p', out_path, '-y'], check=True)
    return out_path

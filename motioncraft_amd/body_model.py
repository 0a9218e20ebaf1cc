"""The SMPL-X body model on the device: 55 posed joints and the vertices from ``poses / expressions / trans``.

Everything the reference does with a sampled 322-d motion after the ``.npz`` goes through the ``smplx`` package
(``smplx.create`` in ``tools/s2g_test.py:76-85`` and ``tools/visualize.py:71-86``, one forward per frame batch in
``tools/s2g_test.py:364-404``): the 55 joints feed ``L1div`` and the beat alignment, the face vertices the ``l2`` /
``lvel`` errors, the mesh the renderer.  ``SMPLXBodyModel`` reads the published model file and runs the same linear
blend skinning (Loper et al. 2015; SMPL-X 2019) in HIP kernels (``mc_smplx_*``, ``csrc/mc_smplx.hip``) on the arrays
``postprocess.postprocess_smplx[_stitched]`` leaves on the device.  The package itself is not a dependency; parity with
it is pinned to a restatement of the published algorithm.
"""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from .lib import ptr as _p, stream as _stream

NUM_JOINTS, POSE_FEATS, MAX_BETAS, MAX_EXPR = 55, 486, 300, 100
DEFAULT_WORK_BYTES = 256 << 20


class SMPLXBodyModel:
    """``SMPLXBodyModel.from_npz(path)``; ``.joints(...)`` -> fp32 [..., 55, 3], ``.vertices(...)`` -> fp32 [..., V, 3],
    ``.faces`` int64 [F, 3].  The file is checked on the host when the object is made; the native object is created at the
    first device call (``close()`` frees it)."""

    def __init__(self, arrays, num_betas=300, num_expression_coeffs=100, flat_hand_mean=False):
        d = {k: np.asarray(arrays[k]) for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights', 'kintree_table')}
        vt = d['v_template']
        if vt.ndim != 2 or vt.shape[1] != 3:
            raise ValueError(f'v_template must be [V, 3], got {vt.shape}')
        V = vt.shape[0]
        sd, pd = d['shapedirs'], d['posedirs']
        if sd.ndim != 3 or sd.shape[:2] != (V, 3):
            raise ValueError(f'shapedirs must be [{V}, 3, n], got {sd.shape}')
        if pd.shape != (V, 3, POSE_FEATS):
            raise ValueError(f'posedirs must be [{V}, 3, {POSE_FEATS}] (9 entries of R - I for each of 54 joints), got {pd.shape}')
        keys = arrays.keys() if hasattr(arrays, 'keys') else arrays
        if 'expr_dirs' in keys:                                   # separate key, or the last 100 of a 400-wide shapedirs
            ed, shape_space = np.asarray(arrays['expr_dirs']), sd.shape[2]
        else:
            shape_space = sd.shape[2] - MAX_EXPR
            if shape_space < 1:
                raise ValueError(f'shapedirs holds {sd.shape[2]} directions and there is no expr_dirs: the expression directions are '
                                 f'the last {MAX_EXPR} of a wider shapedirs')
            ed = sd[:, :, shape_space:]
        if ed.ndim != 3 or ed.shape[:2] != (V, 3):
            raise ValueError(f'expr_dirs must be [{V}, 3, n], got {ed.shape}')
        nb, ne = int(num_betas), int(num_expression_coeffs)
        if not 1 <= nb <= min(shape_space, MAX_BETAS):
            raise ValueError(f'num_betas={nb}: the file has {shape_space} shape directions (at most {MAX_BETAS} are used)')
        if not 1 <= ne <= min(ed.shape[2], MAX_EXPR):
            raise ValueError(f'num_expression_coeffs={ne}: the file has {ed.shape[2]} expression directions (at most {MAX_EXPR} are used)')
        if d['J_regressor'].shape != (NUM_JOINTS, V) or d['weights'].shape != (V, NUM_JOINTS):
            raise ValueError(f'J_regressor must be [{NUM_JOINTS}, {V}] and weights [{V}, {NUM_JOINTS}], got '
                             f'{d["J_regressor"].shape} and {d["weights"].shape}')
        kt = d['kintree_table']
        if kt.ndim != 2 or kt.shape[1] != NUM_JOINTS:
            raise ValueError(f'kintree_table must be [2, {NUM_JOINTS}], got {kt.shape}')
        parents = kt[0].astype(np.int64)
        parents[0] = -1                                           # the file stores 2^32 - 1 there
        for j in range(1, NUM_JOINTS):
            if not 0 <= parents[j] < j:
                raise ValueError(f'kintree_table: parents[{j}] = {parents[j]}; the tree must be topologically ordered (0 <= parent < joint)')
        self.num_vertices, self.num_betas, self.num_expr = V, nb, ne
        self.parents = parents
        f = np.asarray(arrays['f']) if 'f' in keys else np.zeros((0, 3), np.int64)
        self.faces = f.astype(np.int64)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)       # the package holds its buffers in float32
        self.params = dict(v_template=f32(vt), shapedirs=f32(sd[:, :, :nb]), expr_dirs=f32(ed[:, :, :ne]), posedirs=f32(pd),
                           J_regressor=f32(d['J_regressor']), weights=f32(d['weights']), parents=f32(parents))
        # The package's forward adds the file's mean hand pose to the hand joints before lbs unless flat_hand_mean is set
        # (use_pca=False path; the reference creates the model with the default flat_hand_mean=False, tools/s2g_test.py:76-85).
        self.pose_mean = np.zeros(3 * NUM_JOINTS)
        if not flat_hand_mean and 'hands_meanl' in keys and 'hands_meanr' in keys:
            left, right = (np.asarray(arrays[k], dtype=np.float64).reshape(-1) for k in ('hands_meanl', 'hands_meanr'))
            if left.shape != (45,) or right.shape != (45,):
                raise ValueError(f'hands_meanl / hands_meanr must hold 45 values each, got {left.shape} and {right.shape}')
            self.pose_mean[75:120], self.pose_mean[120:165] = left, right
        self._native = None

    KEYS = ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights', 'kintree_table')
    OPTIONAL_KEYS = ('f', 'expr_dirs', 'hands_meanl', 'hands_meanr')

    @classmethod
    def from_npz(cls, path, num_betas=300, num_expression_coeffs=100, flat_hand_mean=False):
        """``path``: the published ``SMPLX_*.npz``, or a dict with its arrays.  Only the keys the model uses are read
        (v_template, shapedirs, posedirs, J_regressor, weights, kintree_table; f, expr_dirs, hands_meanl, hands_meanr when
        present): the file's other entries -- landmark tables, pickled name maps -- are never touched, so it loads with
        ``allow_pickle=False``.  ``flat_hand_mean=False`` (the package's default, what the reference uses) adds the file's
        mean hand pose to the hand joints of every pose; a file without hands_meanl / hands_meanr has none."""
        if isinstance(path, dict):
            return cls(path, num_betas, num_expression_coeffs, flat_hand_mean)
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in cls.KEYS if k not in z.files]
            if missing:
                raise ValueError(f'{path}: not an SMPL-X model file, missing {missing}')
            return cls({k: z[k] for k in cls.KEYS + cls.OPTIONAL_KEYS if k in z.files}, num_betas, num_expression_coeffs, flat_hand_mean)

    # ---- native object ---------------------------------------------------------------------------------------------
    def native(self):
        if self._native is None:
            cfg = _lib.SMPLXConfig(self.num_vertices, NUM_JOINTS, self.num_betas, self.num_expr, POSE_FEATS)
            self.cfg = cfg
            obj = _lib.NativeObject('smplx', ctypes.byref(cfg))
            obj.upload(self.params.items())
            obj.finalize()
            self._native = obj
        return self._native

    def close(self):
        if self._native is not None:
            self._native.close()
            self._native = None

    def _operands(self, poses, expressions, trans, betas):
        """Inputs as contiguous fp64 device tensors: poses [n,165], expressions [n,ne] | None, trans [n,3] | None,
        betas [nb] | [n,nb]; returns them with the leading shape of ``poses``."""
        first = next((t for t in (poses, expressions, trans, betas) if isinstance(t, torch.Tensor) and t.is_cuda), None)
        dev = first.device if first is not None else torch.device('cuda', torch.cuda.current_device())
        to = lambda a: None if a is None else torch.as_tensor(a).to(device=dev, dtype=torch.float64)
        poses = to(poses)
        if poses.dim() < 1 or poses.shape[-1] != 3 * NUM_JOINTS:
            raise ValueError(f'poses must be [..., {3 * NUM_JOINTS}], got {tuple(poses.shape)}')
        lead = tuple(poses.shape[:-1])
        poses = poses.reshape(-1, 3 * NUM_JOINTS).contiguous()
        if self.pose_mean.any():
            poses = poses + torch.from_numpy(self.pose_mean).to(dev)
        n = poses.shape[0]
        expressions, trans, betas = to(expressions), to(trans), to(betas)
        if expressions is not None:
            if expressions.shape[-1] < self.num_expr or expressions.numel() != n * expressions.shape[-1]:
                raise ValueError(f'expressions must be [..., >= {self.num_expr}] with one row per frame, got {tuple(expressions.shape)}')
            expressions = expressions.reshape(n, expressions.shape[-1])[:, :self.num_expr].contiguous()
        if trans is not None:
            if trans.shape[-1] != 3 or trans.numel() != 3 * n:
                raise ValueError(f'trans must be [..., 3] with one row per frame, got {tuple(trans.shape)}')
            trans = trans.reshape(n, 3).contiguous()
        if betas is None:
            betas = torch.zeros(self.num_betas, device=dev, dtype=torch.float64)        # tools/visualize.py:242 saves zeros
        if betas.shape[-1] < self.num_betas:
            raise ValueError(f'betas must hold at least {self.num_betas} coefficients, got {tuple(betas.shape)}')
        per_frame = betas.numel() != betas.shape[-1]
        if per_frame and betas.numel() != n * betas.shape[-1]:
            raise ValueError(f'betas must be [{self.num_betas}] or one row per frame, got {tuple(betas.shape)}')
        betas = betas.reshape(-1, betas.shape[-1])[:, :self.num_betas].contiguous()
        return dev, lead, n, poses, expressions, trans, betas, int(per_frame)

    def joints(self, poses, expressions=None, trans=None, betas=None):
        """The 55 posed joints, fp32 [..., 55, 3] on the device (fp64 arithmetic, one rounding)."""
        obj = self.native()
        dev, lead, n, poses, expr, trans, betas, per_frame = self._operands(poses, expressions, trans, betas)
        out = torch.empty(n, NUM_JOINTS, 3, device=dev, dtype=torch.float32)
        _lib.check(obj.lib.mc_smplx_joints(obj.handle, _p(poses), _p(expr), _p(trans), _p(betas), per_frame, n, _p(out),
                                           _stream()), 'mc_smplx_joints')
        return out.reshape(lead + (NUM_JOINTS, 3))

    def vertices(self, poses, expressions=None, trans=None, betas=None, return_joints=False, work_bytes=DEFAULT_WORK_BYTES):
        """The skinned vertices, fp32 [..., V, 3] on the device (and the joints with ``return_joints``).  Frames run in
        chunks that fit ``work_bytes`` of scratch (raised to one frame's need); the result does not depend on it."""
        obj = self.native()
        dev, lead, n, poses, expr, trans, betas, per_frame = self._operands(poses, expressions, trans, betas)
        need = lambda frames: int(obj.lib.mc_smplx_work_bytes(obj.handle, frames, per_frame))
        wb = max(min(int(work_bytes), need(max(n, 1))), need(1))
        work = torch.empty(wb, device=dev, dtype=torch.uint8)          # per call: the caching allocator keeps it stream-ordered
        verts = torch.empty(n, self.num_vertices, 3, device=dev, dtype=torch.float32)
        jout = torch.empty(n, NUM_JOINTS, 3, device=dev, dtype=torch.float32) if return_joints else None
        _lib.check(obj.lib.mc_smplx_vertices(obj.handle, _p(poses), _p(expr), _p(trans), _p(betas), per_frame, n, _p(work), wb,
                                             _p(verts), _p(jout), _stream()),
                   'mc_smplx_vertices')
        verts = verts.reshape(lead + (self.num_vertices, 3))
        return (verts, jout.reshape(lead + (NUM_JOINTS, 3))) if return_joints else verts

    def vertex_error_sums(self, poses_a, expr_a, trans_a, poses_b, expr_b, trans_b, betas=None, work_bytes=DEFAULT_WORK_BYTES):
        """The vertices of pose sets a and b (one ``betas`` for both) reduced on the device to the fp64 pair
        ``[sum (a - b)^2, sum |(a[t+1] - b[t]) - (b[t+1] - b[t])|]`` over all frames, vertices and coordinates
        (``mc_smplx_vertex_errors``): a device tensor [2]; the vertices never leave the device, and the result does not depend
        on ``work_bytes``."""
        obj = self.native()
        dev, lead, n, pa, ea, ta, betas_d, per_frame = self._operands(poses_a, expr_a, trans_a, betas)
        _, lead_b, nb_, pb, eb, tb, _, _ = self._operands(poses_b, expr_b, trans_b, betas)
        if nb_ != n:
            raise ValueError(f'the two pose sets hold {n} and {nb_} frames')
        need = lambda frames: int(obj.lib.mc_smplx_vertex_errors_work_bytes(obj.handle, frames, n, per_frame))
        wb = max(min(int(work_bytes), need(max(n, 1))), need(1))
        work = torch.empty(wb, device=dev, dtype=torch.uint8)
        sums = torch.empty(2, device=dev, dtype=torch.float64)
        _lib.check(obj.lib.mc_smplx_vertex_errors(obj.handle, _p(pa), _p(ea), _p(ta), _p(pb), _p(eb), _p(tb), _p(betas_d), per_frame, n, _p(work),
                                                  wb, _p(sums), _stream()),
                   'mc_smplx_vertex_errors')
        return sums

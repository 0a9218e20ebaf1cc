"""Numpy restatement of SMPL-X linear blend skinning as published (Loper et al. 2015; Pavlakos et al. 2019; what
``smplx.lbs.lbs`` computes), the yardstick of ``motioncraft_amd.body_model`` / ``mc_smplx_*``.  Tests import it; the product
does not.  ``lbs(model, ..., dtype)`` runs the six steps in ``dtype`` (float64: the exact side; float32: the package's own
precision, whose distance from float64 is the unit of the joints bound); ``lbs_bound`` evaluates the forward error bound of an
fp32 evaluation of the vertices in float64.  Also the synthetic model files of the tests (the real file's keys, fixed seed).
"""
import numpy as np

NJ = 55
# kintree_table[0] of the published SMPL-X model: pelvis, legs / spine, neck / collars, head, arms, jaw + eyes, the two hands
PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                    20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                    21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53], dtype=np.int64)


def rodrigues(theta, dtype=np.float64):
    """theta [..., 3] -> R [..., 3, 3]: the package's batch_rodrigues (angle = |theta + 1e-8|, direction = theta / angle)."""
    theta = np.asarray(theta, dtype)
    angle = np.sqrt(((theta + dtype(1e-8)) ** 2).sum(-1, dtype=dtype))[..., None]
    d = theta / angle
    s, c = np.sin(angle)[..., None], np.cos(angle)[..., None]
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    zero = np.zeros_like(x)
    K = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(theta.shape[:-1] + (3, 3)).astype(dtype)
    return (np.eye(3, dtype=dtype) + s * K + (dtype(1) - c) * (K @ K)).astype(dtype)


def model_arrays(model, nb, ne):
    """(v_template, shapedirs[:, :, :nb], expr_dirs[:, :, :ne], posedirs, J_regressor, weights, parents) of a model dict, rounded
    to float32 like the package's buffers (and the product's parameter store), returned as float64."""
    sd = np.asarray(model['shapedirs'])
    ed = np.asarray(model['expr_dirs']) if 'expr_dirs' in model else sd[:, :, sd.shape[2] - 100:]
    r = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    parents = np.asarray(model['kintree_table'])[0].astype(np.int64)
    return r(model['v_template']), r(sd[:, :, :nb]), r(ed[:, :, :ne]), r(model['posedirs']), r(model['J_regressor']), r(model['weights']), parents


def lbs(model, poses, expr=None, trans=None, betas=None, nb=None, ne=100, dtype=np.float64, vertices=True, parts=False):
    """poses [n,165], expr [n,ne] | None, trans [n,3] | None, betas [nb] | [n,nb] | None -> (joints [n,55,3], verts [n,V,3] | None),
    every step evaluated in ``dtype``.  parts=True also returns (A [n,55,3,4], v_posed [n,V,3], coef [n,nb+ne], feat [n,486])."""
    dt = dtype
    nb = nb if nb is not None else (np.asarray(betas).shape[-1] if betas is not None else 1)
    vt, sd, ed, pd, jr, wt, parents = (a.astype(dt) if a.dtype != np.int64 else a for a in model_arrays(model, nb, ne))
    poses = np.asarray(poses, dt).reshape(-1, NJ, 3)
    n, V = poses.shape[0], vt.shape[0]
    coef = np.zeros((n, nb + ne), dt)
    if betas is not None:
        coef[:, :nb] = np.asarray(betas, dt).reshape(-1, np.asarray(betas).shape[-1])[:, :nb]
    if expr is not None:
        coef[:, nb:] = np.asarray(expr, dt)[:, :ne]
    tr = np.zeros((n, 3), dt) if trans is None else np.asarray(trans, dt)
    R = rodrigues(poses, dt)                                                        # 1
    dirs = np.concatenate([sd, ed], axis=2).reshape(3 * V, nb + ne)
    v_shaped = vt.reshape(1, 3 * V) + coef @ dirs.T                                 # 2
    J = np.einsum('jv,nvc->njc', jr, v_shaped.reshape(n, V, 3)).astype(dt)          # 3
    feat = (R[:, 1:] - np.eye(3, dtype=dt)).reshape(n, 9 * (NJ - 1))
    v_posed = (v_shaped + feat @ pd.reshape(3 * V, -1).T).reshape(n, V, 3) if vertices else None     # 4
    G = np.zeros((n, NJ, 3, 4), dt)                                                 # 5
    G[:, 0, :, :3], G[:, 0, :, 3] = R[:, 0], J[:, 0]
    for j in range(1, NJ):
        p = parents[j]
        G[:, j, :, :3] = G[:, p, :, :3] @ R[:, j]
        G[:, j, :, 3] = np.einsum('nab,nb->na', G[:, p, :, :3], J[:, j] - J[:, p]) + G[:, p, :, 3]
    A = G.copy()
    A[..., 3] = G[..., 3] - np.einsum('njab,njb->nja', G[..., :3], J)
    joints = (G[..., 3] + tr[:, None]).astype(dt)                                   # 6
    verts = None
    if vertices:
        T = np.einsum('vj,njab->nvab', wt, A).astype(dt)
        verts = (np.einsum('nvab,nvb->nva', T[..., :3], v_posed) + T[..., 3] + tr[:, None]).astype(dt)
    if parts:
        return joints, verts, (A, v_posed, coef, feat)
    return joints, verts


def lbs_bound(model, poses, expr=None, trans=None, betas=None, nb=None, ne=100):
    """Forward error bound of ANY fp32 evaluation of the vertices, per element, evaluated in float64.  A vertex coordinate is a
    nested sum whose leaves are w_j A_j[a,c] x (one term of v_posed[c]: the template entry or one direction entry times its
    coefficient), w_j A_j[a,3] and transl[a].  An fp32 sum of K terms in arbitrary order, each a product of a few rounded
    factors, is within (K + c) u sum |leaf| of the exact value (u = 2^-24, c the multiplications along a leaf; Higham 2002,
    section 4.2); here K = (1 + nb + ne + 486) blend-shape terms + 4 x (the most skin weights of a vertex, at least 8) + 1 skinning
    terms and c is covered by 64.
    Returns (exact vertices, bound), both [n,V,3]."""
    nbv = nb if nb is not None else (np.asarray(betas).shape[-1] if betas is not None else 1)
    _, verts, (A, v_posed, coef, feat) = lbs(model, poses, expr, trans, betas, nbv, ne, np.float64, True, True)
    vt, sd, ed, pd, jr, wt, parents = model_arrays(model, nbv, ne)
    n, V = verts.shape[0], vt.shape[0]
    dirs = np.abs(np.concatenate([sd, ed], axis=2).reshape(3 * V, -1))
    S1 = (np.abs(vt).reshape(1, 3 * V) + np.abs(coef) @ dirs.T + np.abs(feat) @ np.abs(pd).reshape(3 * V, -1).T).reshape(n, V, 3)
    Tabs = np.einsum('vj,njab->nvab', np.abs(wt), np.abs(A))
    tr = np.zeros((n, 3)) if trans is None else np.abs(np.asarray(trans, np.float64))
    leaves = np.einsum('nvab,nvb->nva', Tabs[..., :3], S1) + Tabs[..., 3] + tr[:, None]
    K = 1 + nbv + ne + 486 + 4 * max(8, int((wt != 0).sum(1).max())) + 1
    return verts, (K + 64) * 2.0 ** -24 * leaves


def synthetic_model(V=1031, shape_space=20, seed=0, expr_key=False, max_nz=8):
    """A model dict with the published file's keys: the real 55-joint parent table, sparse regressor rows that sum to 1, skin
    weights with 1..max_nz nonzeros per vertex that sum to 1, body-sized template, small blend-shape directions.
    expr_key=False: shapedirs [V,3,shape_space+100] (expressions last, like the 400-wide file); True: a separate expr_dirs."""
    rs = np.random.RandomState(seed)
    vt = rs.uniform(-1.0, 1.0, (V, 3)) * np.array([0.4, 0.9, 0.2])
    sd = 0.02 * rs.randn(V, 3, shape_space)
    ed = 0.01 * rs.randn(V, 3, 100)
    pd = 0.01 * rs.randn(V, 3, 486)
    jr = np.zeros((NJ, V))
    for j in range(NJ):
        idx = rs.choice(V, 12, replace=False)
        w = rs.uniform(0.1, 1.0, 12)
        jr[j, idx] = w / w.sum()
    wt = np.zeros((V, NJ))
    for v in range(V):
        k = 1 + (v % max_nz)
        idx = rs.choice(NJ, k, replace=False)
        w = rs.uniform(0.1, 1.0, k)
        wt[v, idx] = w / w.sum()
    kt = np.stack([PARENTS, np.arange(NJ)]).astype(np.int64)
    kt[0, 0] = 2 ** 32 - 1
    f = rs.randint(0, V, (2 * V, 3)).astype(np.int64)
    m = dict(v_template=vt, posedirs=pd, J_regressor=jr, weights=wt, kintree_table=kt, f=f)
    if expr_key:
        m.update(shapedirs=sd, expr_dirs=ed)
    else:
        m['shapedirs'] = np.concatenate([sd, ed], axis=2)
    return m


def random_poses(n, seed, scale=0.4):
    """Axis-angle rows [n,165]: moderate joint rotations, a larger global turn."""
    rs = np.random.RandomState(seed)
    p = scale * rs.randn(n, NJ, 3)
    p[:, 0] *= 3.0
    return p.reshape(n, 3 * NJ)

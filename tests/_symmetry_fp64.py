"""numpy float64 referee of the symmetry-aware object errors (--eval_symmetric), by another route than the kernel: the
points are moved by S_k, then by G, and separately by P, and norms of the DIFFERENCES of the moved points are taken -- the kernel's
D_k = P - G S_k form is not used.  NaN is carried by np.max / np.min / np.mean (they do not drop it).  No GPU, no HIP library."""
import numpy as np


def move(rt, pts):
    """(..., 3, 4) rigid transforms applied to (N, 3) points -> (..., N, 3)"""
    return np.einsum('...ij,nj->...ni', rt[..., :3], pts) + rt[..., None, :, 3]


def pair(pd_rt, gt_rt, sym_R, sym_t, bbox3d, verts, diameter):
    """pd_rt (S, 3, 4), gt_rt (3, 4), sym_R (K, 3, 3), sym_t (K, 3), bbox3d (8, 3), verts (P, 3) -> (S, 3): SMCE, MSSD, MSSD < 0.1 d"""
    out = np.zeros((pd_rt.shape[0], 3))
    sym = np.concatenate([sym_R, sym_t[:, :, None]], -1)                       # (K, 3, 4)
    for col, pts, over_points in ((0, np.asarray(bbox3d, np.float64), np.mean), (1, np.asarray(verts, np.float64), np.max)):
        gt_pts = move(gt_rt, move(sym, pts).reshape(-1, 3)).reshape(sym.shape[0], -1, 3)   # (K, N, 3): first S_k, then G
        pd_pts = move(pd_rt, pts)                                              # (S, N, 3)
        d = np.linalg.norm(pd_pts[:, None] - gt_pts[None], axis=-1)            # (S, K, N)
        out[:, col] = np.min(over_points(d, axis=-1), axis=-1)
    bad = ~(np.isfinite(pd_rt).all((-1, -2)) & np.isfinite(gt_rt).all())
    out[bad, :2] = np.nan                                                      # inf - inf etc. give NaN already; an inf alone would not
    with np.errstate(invalid='ignore'):
        out[:, 2] = (out[:, 1] < 0.1 * diameter).astype(np.float64)            # NaN < x is False: the hit of a NaN pose is 0
    return out


def batch(pd_rt, gt_rt, obj_id, sym_R, sym_t, bbox3d, verts, diameter):
    """pd_rt (n, S, 3, 4), gt_rt (n, 3, 4), obj_id (n,), tables indexed by object -> (n, S, 3)"""
    return np.stack([pair(pd_rt[b], gt_rt[b], sym_R[i], sym_t[i], bbox3d[i], verts[i], diameter[i]) for b, i in enumerate(obj_id)])


def mce(pd_rt, gt_rt, bbox3d):
    """the plain mean corner error of one pair (criterion_MCE_OCE, test.py:354-374)"""
    return np.linalg.norm(move(pd_rt, bbox3d) - move(gt_rt, bbox3d), axis=-1).mean(-1)


def table_rule(per):
    """(n, S, 3) -> one, best, mean (n, 3) as vpho_obj_symmetry_table_f64 states it: best starts at hypothesis 0 and takes a later value
    only where v < best (v > best for the hit) holds -- a NaN at 0 stays, a later NaN is passed over; mean is the plain fp64 mean"""
    n, S, _ = per.shape
    best = per[:, 0].copy()
    for s in range(1, S):
        v = per[:, s]
        with np.errstate(invalid='ignore'):
            take = np.concatenate([v[:, :2] < best[:, :2], v[:, 2:] > best[:, 2:]], 1)
        best = np.where(take, v, best)
    total = per[:, 0].copy()
    for s in range(1, S):
        total = total + per[:, s]
    return per[:, 0].copy(), best, total / S

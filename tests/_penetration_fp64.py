"""float64 numpy oracle of the penetration metric, written independently of vpho_amd.physics_eval's tables:

* ``contains(verts, faces, pts)``: the z-ray parity rule of the occupancy-networks ``MeshIntersector`` at resolution 512, every
  (point, triangle) pair tested directly, with the candidate filter of its triangle hash (the point's own int-truncated xy cell must
  lie in the triangle's int-truncated, clamped xy bounding cells) and the same order of operations;
* ``distance(verts, faces, pts)``: the unsigned distance to the nearest triangle, closest point by Voronoi regions (Ericson,
  "Real-Time Collision Detection" 5.1.5), vectorised over pairs;
* ``penetration(...)``: sd and the per-image reduction.
"""
import numpy as np

RES = 512


def _frame(verts, faces):
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)].astype(np.float64)
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    scale = (RES - 1) / (hi - lo)
    return tri, scale, 0.5 - scale * lo


def contains(verts, faces, pts, chunk=256):
    tri, scale, translate = _frame(verts, faces)
    tr = scale * tri + translate
    q = scale * np.asarray(pts, np.float64) + translate
    out = np.zeros(len(q), bool)
    box = np.all((0 <= q) & (q <= RES), axis=1)
    idx = np.nonzero(box)[0]
    cell = q[:, :2].astype(np.int64)                                     # q >= 0 inside the box: truncation
    cmin = np.clip(tr[:, :, :2].min(1).astype(np.int64), 0, RES - 1)
    cmax = np.clip(tr[:, :, :2].max(1).astype(np.int64), 0, RES - 1)
    t1, t2, t3 = tr[:, 0], tr[:, 1], tr[:, 2]
    A00, A01, A10, A11 = t1[:, 0] - t3[:, 0], t2[:, 0] - t3[:, 0], t1[:, 1] - t3[:, 1], t2[:, 1] - t3[:, 1]
    det = A00 * A11 - A01 * A10
    sdet, adet = np.sign(det), np.abs(det)
    n = np.cross(t3 - t1, t2 - t1)
    snz, anz = np.sign(n[:, 2]), np.abs(n[:, 2])
    for s in range(0, len(idx), chunk):
        ii = idx[s:s + chunk]
        qq = q[ii][:, None, :]
        c = cell[ii][:, None, :]
        cand = (c[..., 0] < RES) & (c[..., 1] < RES) & (cmin[None, :, 0] <= c[..., 0]) & (c[..., 0] <= cmax[None, :, 0]) & \
               (cmin[None, :, 1] <= c[..., 1]) & (c[..., 1] <= cmax[None, :, 1])
        y0, y1 = qq[..., 0] - t3[None, :, 0], qq[..., 1] - t3[None, :, 1]
        u = (A11 * y0 - A01 * y1) * sdet
        v = (-A10 * y0 + A00 * y1) * sdet
        suv = u + v
        hit = cand & (adet != 0) & (0 < u) & (u < adet) & (0 < v) & (v < adet) & (0 < suv) & (suv < adet)
        alpha = n[None, :, 0] * (t1[None, :, 0] - qq[..., 0]) + n[None, :, 1] * (t1[None, :, 1] - qq[..., 1])
        with np.errstate(invalid='ignore'):
            depth = np.where(anz != 0, t1[:, 2] * anz, np.nan) + alpha * snz
            zz = qq[..., 2] * anz
            c0 = (hit & (depth >= zz)).sum(1)
            c1 = (hit & (depth < zz)).sum(1)
        out[ii] = (c0 % 2 == 1) & (c1 % 2 == 1)
    return out


def _dist2(p, a, b, c):
    """squared distance of points p (P, 1, 3) to triangles a, b, c (1, T, 3): Voronoi regions, first matching region wins"""
    ab, ac = b - a, c - a
    ap = p - a
    dot = lambda x, y: (x * y).sum(-1)
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = ap - ab
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = ap - ac
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(invalid='ignore', divide='ignore'):
        s_ab = d1 / (d1 - d3)
        s_ac = d2 / (d2 - d6)
        s_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = va + vb + vc
        v, w = vb / den, vc / den
    sq = lambda e: dot(e, e)
    face = sq(ap - v[..., None] * ab - w[..., None] * ac)
    corner = np.minimum(sq(ap), np.minimum(sq(bp), sq(cp)))
    res = np.where(den > 0, face, corner)
    res = np.where((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), sq(bp - s_bc[..., None] * (ac - ab)), res)
    res = np.where((vb <= 0) & (d2 >= 0) & (d6 <= 0), sq(ap - s_ac[..., None] * ac), res)
    res = np.where((d6 >= 0) & (d5 <= d6), sq(cp), res)
    res = np.where((vc <= 0) & (d1 >= 0) & (d3 <= 0), sq(ap - s_ab[..., None] * ab), res)
    res = np.where((d3 >= 0) & (d4 <= d3), sq(bp), res)
    res = np.where((d1 <= 0) & (d2 <= 0), sq(ap), res)
    return res


def distance(verts, faces, pts, chunk=128):
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    p = np.asarray(pts, np.float64)
    out = np.empty(len(p))
    for s in range(0, len(p), chunk):
        out[s:s + chunk] = np.sqrt(_dist2(p[s:s + chunk, None, :], a, b, c).min(1))
    return out


def model_frame(verts_cam, rt):
    """p = R^T (v - t) per image: verts_cam (n, V, 3), rt (n, 3, 4)"""
    v = np.asarray(verts_cam, np.float64)
    R, t = np.asarray(rt, np.float64)[:, :, :3], np.asarray(rt, np.float64)[:, :, 3]
    return np.einsum('nij,nvi->nvj', R, v - t[:, None, :])


def reduce(sd, inside, thresh):
    """(n, 4): PD (max d over the inside vertices, 0 if none), n_inside, min sd, contact"""
    pd = np.where(inside, -sd, 0.0).max(1)
    mn = sd.min(1)
    return np.stack([np.maximum(pd, 0.0), inside.sum(1).astype(np.float64), mn, (mn <= thresh).astype(np.float64)], 1)


def box_sd(lo, hi, pts):
    """closed form signed distance of points to the axis-aligned box [lo, hi] (negative inside)"""
    c, h = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
    q = np.abs(np.asarray(pts, np.float64) - c) - h
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)

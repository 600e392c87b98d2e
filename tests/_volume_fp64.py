"""float64 numpy helpers of the intersection-volume tests:

* ``model_frame(verts_cam, rt)``: q_v = R^T (v - t) in the documented order of operations -- d = (double) v - t per component, then
  R[0][k] d0 + R[1][k] d1 + R[2][k] d2 summed left to right, no fused multiply-add -- so that its bits are the kernel's;
* ``hand_inside(qv, faces, pts)``: the restatement of the kernels -- the 19 parity fields of physics_eval.mesh_tables on the posed mesh,
  then cull, cell test, strict containment and two-bucket parity per (centre, face) pair in the kernel's expressions;
* ``winding_inside(verts, faces, pts)``: an INDEPENDENT formulation, the generalised winding number as the sum of the signed solid
  angles of the faces (Van Oosterom & Strackee 1983), inside iff |w| > 1/2;
* ``edge_band(qv, faces, pts, eps)``: the centres within eps hash units of a projected edge of the mesh, where the parity rule of the
  reference (strict containment: a ray through an edge counts no crossing) and the winding number may disagree.
"""
import numpy as np

RES = 512


def model_frame(verts_cam, rt):
    """verts_cam (V, 3) fp32, rt (3, 4) fp64 -> (V, 3) fp64"""
    v = np.asarray(verts_cam, np.float32).astype(np.float64)
    R = np.asarray(rt, np.float64)
    d0, d1, d2 = v[:, 0] - R[0, 3], v[:, 1] - R[1, 3], v[:, 2] - R[2, 3]
    return np.stack([R[0, k] * d0 + R[1, k] * d1 + R[2, k] * d2 for k in range(3)], 1)


def hand_inside(qv, faces, pts, chunk=512):
    from vpho_amd.physics_eval import mesh_tables
    r, scale, translate = mesh_tables(qv, faces)
    r = r[:, :19]
    f = lambda k: r[None, :, k]
    p = np.asarray(pts, np.float32).astype(np.float64)
    q_all = scale * p + translate
    out = np.zeros(len(p), bool)
    with np.errstate(invalid='ignore'):
        idx = np.nonzero(np.all((0.0 <= q_all) & (q_all <= RES), axis=1))[0]           # the cull: every other centre is outside
    for s in range(0, len(idx), chunk):
        ii = idx[s:s + chunk]
        q = q_all[ii]
        cx, cy = np.trunc(q[:, 0:1]), np.trunc(q[:, 1:2])
        has_cell = (cx < RES) & (cy < RES)
        qx, qy, qz = q[:, 0:1], q[:, 1:2], q[:, 2:3]
        with np.errstate(invalid='ignore', over='ignore'):
            cell = (f(15) <= cx) & (cx <= f(16)) & (f(17) <= cy) & (cy <= f(18))
            y0, y1 = qx - f(0), qy - f(1)
            u = (f(5) * y0 - f(3) * y1) * f(6)
            w = (-f(4) * y0 + f(2) * y1) * f(6)
            suv = u + w
            hit = has_cell & cell & (0.0 < u) & (u < f(7)) & (0.0 < w) & (w < f(7)) & (0.0 < suv) & (suv < f(7))
            alpha = f(10) * (f(8) - qx) + f(11) * (f(9) - qy)
            depth = f(14) + alpha * f(12)
            zz = qz * f(13)
            c0 = (hit & (depth >= zz)).sum(1)
            c1 = (hit & (depth < zz)).sum(1)
        out[ii] = (c0 % 2 == 1) & (c1 % 2 == 1)
    return out


def winding_inside(verts, faces, pts):
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    p = np.asarray(pts, np.float64)[:, None, None, :]
    a, b, c = (tri[None] - p)[:, :, 0], (tri[None] - p)[:, :, 1], (tri[None] - p)[:, :, 2]
    la, lb, lc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
    num = np.einsum('pti,pti->pt', a, np.cross(b, c))
    den = la * lb * lc + (a * b).sum(-1) * lc + (a * c).sum(-1) * lb + (b * c).sum(-1) * la
    w = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)
    return np.abs(w) > 0.5


def edge_band(qv, faces, pts, eps=1e-9):
    """(P,) bool: the centre's xy projection in the mesh's hash frame is within eps of a projected edge (a segment)"""
    tri = np.asarray(qv, np.float64)[np.asarray(faces, np.int64)]
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    scale = (RES - 1) / (hi - lo)
    translate = 0.5 - scale * lo
    t = (scale * tri + translate)[:, :, :2]
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    q = (scale * np.asarray(pts, np.float32).astype(np.float64) + translate)[:, None, :2]
    ab = (b - a)[None]
    s = np.clip(((q - a[None]) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0.0, 1.0)
    d = np.linalg.norm(q - (a[None] + s[..., None] * ab), axis=-1)
    return (d < eps).any(1)

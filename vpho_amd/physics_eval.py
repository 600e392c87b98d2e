"""Hand-object penetration metrics (``--eval_physics``): the object meshes and their per-triangle tables.

``object_meshes`` gives every object of ``assets['ycb']`` a triangle mesh: the real ``object_mesh_info.pkl`` entries (``verts`` +
``faces``, lib/dataset/base.py:221-223) or, for the synthetic table, a closed box from the object's ``bbox3d``.  ``mesh_tables``
turns one mesh into the records of ``vpho_obj_mesh_tables`` (include/vpho_hip.h): the point-independent terms of the z-ray parity
test of the occupancy-networks ``MeshIntersector`` at resolution 512, computed with numpy in that test's order of operations, so
that the device kernel's inside flags are bit-for-bit the host test's.  Importable without the HIP library.
"""
import os
import pickle

import numpy as np

from .assets import AssetError

RESOLUTION = 512              # VPHO_PEN_RESOLUTION
TRI_STRIDE = 28               # VPHO_PEN_TRI_STRIDE
BOX_SUBDIV = 16               # synthetic box meshes: 16 x 16 quads per side, 3 072 triangles
COLUMNS = 64                  # VPHO_PEN_COLUMNS: the 512 x 512 hash cells in 64 x 64 columns of 8 x 8 cells
CLUSTER = 16                  # VPHO_PEN_CLUSTER: triangles per bounding sphere
REACH_GROW = 1.0 + 2.0 ** -20  # the kernel's relative slack on sqrt(best) (csrc/penetration_multi.hip)
RADIUS_GROW = 2.0 ** -30      # the radii's relative slack, and their absolute one in units of the mesh's bounding-box diagonal


def box_mesh(bbox3d, sub=BOX_SUBDIV):
    """Closed, outward-oriented triangle mesh of the axis-aligned box spanned by ``bbox3d`` (8, 3): every side split into sub x sub
    quads of two triangles (12 sub^2 triangles, 6 sub^2 + 2 vertices shared between the sides).  No random numbers."""
    b = np.asarray(bbox3d, np.float64).reshape(-1, 3)
    lo, hi = b.min(0), b.max(0)
    index = {}
    verts = []

    def vid(g):
        if g not in index:
            index[g] = len(verts)
            verts.append(g)
        return index[g]

    faces = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3            # (u, v, axis) is a right-handed frame
        for side in (0, sub):
            for i in range(sub):
                for j in range(sub):
                    def g(a, c):
                        p = [0, 0, 0]
                        p[axis], p[u], p[v] = side, a, c
                        return tuple(p)
                    q = [vid(g(i, j)), vid(g(i + 1, j)), vid(g(i + 1, j + 1)), vid(g(i, j + 1))]   # counter-clockwise about +axis
                    tris = [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
                    if side == 0:                        # outward normal is -axis: reverse the winding
                        tris = [(t[0], t[2], t[1]) for t in tris]
                    faces += tris
    g = np.array(verts, np.int64)
    xyz = lo + (hi - lo) * (g / sub)
    xyz = np.where(g == sub, hi, xyz)                    # the far faces exactly at hi
    return xyz, np.array(faces, np.int64)


def torus_mesh(nu, nv, major=1.0, minor=0.4, drop_quad=None):
    """Closed triangle mesh of a torus about the y axis: nu x nv quads of two triangles (2 nu nv triangles, nu nv vertices), ring radius
    ``major`` and tube radius ``minor``; non-convex, so a z-ray crosses it 0, 2 or 4 times.  ``drop_quad``: index of a quad to leave out
    (an open mesh).  No random numbers."""
    u = np.arange(nu) * (2 * np.pi / nu) + 0.1
    v = np.arange(nv) * (2 * np.pi / nv) + 0.2
    uu, vv = np.meshgrid(u, v, indexing='ij')
    ring = major + minor * np.cos(vv)
    verts = np.stack([ring * np.cos(uu), minor * np.sin(vv), ring * np.sin(uu)], -1).reshape(-1, 3)
    faces = []
    for i in range(nu):
        for j in range(nv):
            if drop_quad is not None and i * nv + j == drop_quad:
                continue
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            faces += [(a, b, c), (a, c, d)]
    return verts, np.array(faces, np.int64)


def mesh_tables(verts, faces):
    """(tri (T, TRI_STRIDE) fp64, scale (3,), translate (3,)) of one mesh; field layout of include/vpho_hip.h."""
    triangles = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)].astype(np.float64)
    n_tri = triangles.shape[0]
    if n_tri == 0:
        raise AssetError('mesh_tables: a mesh without triangles')
    bbox_min = triangles.reshape(3 * n_tri, 3).min(axis=0)
    bbox_max = triangles.reshape(3 * n_tri, 3).max(axis=0)
    scale = (RESOLUTION - 1) / (bbox_max - bbox_min)
    translate = 0.5 - scale * bbox_min
    tr = scale * triangles + translate                                   # the hash frame, [0.5, 511.5]^3
    # 2-D containment terms: A = (t1 - t3, t2 - t3) as columns, det A, its sign and magnitude
    A = (tr[:, :2, :2] - tr[:, 2:, :2]).transpose([0, 2, 1])
    detA = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    # plane terms: n = (t3 - t1) x (t2 - t1); depth = t1.z |n.z| + alpha sign(n.z), NaN where n.z == 0
    t1, t2, t3 = tr[:, 0, :], tr[:, 1, :], tr[:, 2, :]
    normals = np.cross(t3 - t1, t2 - t1)
    n_2 = normals[:, 2]
    abs_n_2 = np.abs(n_2)
    d0 = np.full(n_tri, np.nan)
    m = abs_n_2 != 0
    d0[m] = t1[m, 2] * abs_n_2[m]
    # the triangle hash's cells: int-truncated bbox of the xy projection, clamped to [0, RESOLUTION)
    cmin = np.clip(np.trunc(tr[:, :, :2].min(1)), 0, RESOLUTION - 1)
    cmax = np.clip(np.trunc(tr[:, :, :2].max(1)), 0, RESOLUTION - 1)
    # distance terms in the model frame
    a = triangles[:, 0]
    ab, ac = triangles[:, 1] - a, triangles[:, 2] - a
    tri = np.concatenate([tr[:, 2, :2], A.reshape(n_tri, 4), np.sign(detA)[:, None], np.abs(detA)[:, None], t1[:, :2], normals[:, :2],
                          np.sign(n_2)[:, None], abs_n_2[:, None], d0[:, None], cmin[:, :1], cmax[:, :1], cmin[:, 1:], cmax[:, 1:],
                          a, ab, ac], axis=1)
    assert tri.shape == (n_tri, TRI_STRIDE)
    return np.ascontiguousarray(tri), scale, translate


def mesh_accel(tri):
    """The two conservative filters of ``vpho_obj_mesh_accel`` (include/vpho_hip.h) over the records ``tri`` (T, TRI_STRIDE) of one mesh,
    triangle indices local to the mesh; deterministic (stable sorts, no random numbers):
      col_offset (COLUMNS^2 + 1,), col_tri: per xy column of 512 / COLUMNS hash cells a side (row-major, y first) the triangles whose
        cell rectangle (fields 15-18) touches it, ascending;
      order (C * CLUSTER,): the triangles in Morton order of their centroids, the last cluster padded with copies of its last triangle;
      sphere (C, 4): per cluster of CLUSTER consecutive entries of ``order`` the centre of its corners' bounding box and the largest
        corner distance from it, enlarged by (1 + RADIUS_GROW) and by RADIUS_GROW bounding-box diagonals (the slack the kernel's skip
        test relies on, derived in csrc/penetration_multi.hip);
      geo (C, CLUSTER, 9): bit copies of fields 19-27 in that order."""
    tri = np.ascontiguousarray(tri, np.float64)
    n_tri = tri.shape[0]
    cells = RESOLUTION // COLUMNS
    x0, x1, y0, y1 = (tri[:, 15 + i].astype(np.int64) // cells for i in range(4))
    w = x1 - x0 + 1
    cnt = w * (y1 - y0 + 1)
    t_idx = np.repeat(np.arange(n_tri), cnt)
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    col = (y0[t_idx] + local // w[t_idx]) * COLUMNS + x0[t_idx] + local % w[t_idx]
    by_col = np.lexsort((t_idx, col))                                   # by column, then ascending triangle index
    col_offset = np.searchsorted(col[by_col], np.arange(COLUMNS * COLUMNS + 1)).astype(np.int32)
    col_tri = t_idx[by_col].astype(np.int32)
    # Morton order of the centroids on a 1024^3 lattice over the corners' bounding box
    a, ab, ac = tri[:, 19:22], tri[:, 22:25], tri[:, 25:28]
    corners = np.stack([a, a + ab, a + ac], 1)
    lo, hi = corners.reshape(-1, 3).min(0), corners.reshape(-1, 3).max(0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    g = np.clip(((corners.mean(1) - lo) / ext * 1024.0).astype(np.int64), 0, 1023)
    code = np.zeros(n_tri, np.int64)
    for bit in range(10):
        for k in range(3):
            code |= ((g[:, k] >> bit) & 1) << (3 * bit + k)
    order = np.argsort(code, kind='stable')
    n_clu = (n_tri + CLUSTER - 1) // CLUSTER
    order = np.concatenate([order, np.full(n_clu * CLUSTER - n_tri, order[-1])])
    cc = corners[order].reshape(n_clu, 3 * CLUSTER, 3)
    centre = (cc.min(1) + cc.max(1)) / 2.0
    r0 = np.sqrt(((cc - centre[:, None]) ** 2).sum(-1)).max(1)
    radius = r0 * (1.0 + RADIUS_GROW) + RADIUS_GROW * np.sqrt(((hi - lo) ** 2).sum())
    return dict(col_offset=col_offset, col_tri=col_tri, order=order.astype(np.int32),
                sphere=np.ascontiguousarray(np.concatenate([centre, radius[:, None]], 1)),
                geo=np.ascontiguousarray(tri[order, 19:28].reshape(n_clu, CLUSTER, 9)))


def parity_candidates(acc, scale, translate, pts):
    """Host restatement of the kernel's parity walk: (P, T) bool, the triangles of the column list of every point's own hash cell
    (none for a point outside [0, 512]^3 or on its far faces: no cell).  ``pts`` (P, 3) in the model frame."""
    q = scale * np.asarray(pts, np.float64) + translate
    n_tri = int(acc['order'].max()) + 1
    out = np.zeros((len(q), n_tri), bool)
    ok = np.all((0 <= q) & (q <= RESOLUTION), axis=1)
    cells = RESOLUTION // COLUMNS
    for i in np.nonzero(ok)[0]:
        cx, cy = int(q[i, 0]), int(q[i, 1])
        if cx < RESOLUTION and cy < RESOLUTION:
            col = (cy // cells) * COLUMNS + cx // cells
            out[i, acc['col_tri'][acc['col_offset'][col]:acc['col_offset'][col + 1]]] = True
    return out


def _tri_dist2(p, g):
    """squared distances of points p (P, 1, 3) to the triangles g (1, M, 9) = (a, b - a, c - a): closest point by Voronoi regions
    (Ericson 5.1.5), the first matching region in the kernel's order wins"""
    a, ab, ac = g[..., 0:3], g[..., 3:6], g[..., 6:9]
    dot = lambda x, y: (x * y).sum(-1)
    ap = p - a
    bp, cp = ap - ab, ap - ac
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    sq = lambda e: dot(e, e)
    with np.errstate(invalid='ignore', divide='ignore'):
        den = va + vb + vc
        res = np.where(den > 0, sq(ap - (vb / den)[..., None] * ab - (vc / den)[..., None] * ac), np.minimum(sq(ap), np.minimum(sq(bp), sq(cp))))
        res = np.where((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), sq(bp - ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (ac - ab)), res)
        res = np.where((vb <= 0) & (d2 >= 0) & (d6 <= 0), sq(ap - (d2 / (d2 - d6))[..., None] * ac), res)
        res = np.where((d6 >= 0) & (d5 <= d6), sq(cp), res)
        res = np.where((vc <= 0) & (d1 >= 0) & (d3 <= 0), sq(ap - (d1 / (d1 - d3))[..., None] * ab), res)
        res = np.where((d3 >= 0) & (d4 <= d3), sq(bp), res)
    return np.where((d1 <= 0) & (d2 <= 0), sq(ap), res)


def nearest_candidates(acc, pts):
    """Host restatement of the kernel's nearest-triangle walk: the cluster with the nearest centre first, then the clusters in order,
    skipping those with |p - centre| > sqrt(best) REACH_GROW + radius.  -> (visited (P, T) bool, best (P,) squared distance).
    ``pts`` (P, 3) in the model frame."""
    p = np.asarray(pts, np.float64)
    sphere, geo = acc['sphere'], acc['geo']
    order = acc['order'].reshape(len(sphere), CLUSTER)
    visited = np.zeros((len(p), int(acc['order'].max()) + 1), bool)
    D2 = ((p[:, None, :] - sphere[None, :, :3]) ** 2).sum(-1)
    seed = D2.argmin(1)                                                  # the first minimum, as the kernel's strict compare
    best = _tri_dist2(p[:, None, :], geo[seed]).min(1)
    visited[np.arange(len(p))[:, None], order[seed]] = True
    for k in range(len(sphere)):
        lim = np.sqrt(best) * REACH_GROW + sphere[k, 3]
        go = np.nonzero((seed != k) & ~(D2[:, k] > lim * lim))[0]
        if len(go):
            best[go] = np.minimum(best[go], _tri_dist2(p[go, None, :], geo[k][None]).min(1))
            visited[go[:, None], order[k][None, :]] = True
    return visited, best


def object_meshes(assets, asset_root='asset'):
    """{object name: {'verts': (N, 3) fp64, 'faces': (T, 3) int64}} in the order of ``assets['ycb']``.  The real table re-opens the
    ``object_mesh_info.pkl`` that ``load_assets`` read (``assets['sources']['ycb']``, relative paths resolved against ``asset_root``
    if they do not exist as given) and needs its ``faces``; the synthetic table gets ``box_mesh(bbox3d)`` per object."""
    names = list(assets['ycb'].keys())
    src = assets.get('sources', {}).get('ycb', 'synthetic')
    if src == 'synthetic':
        return {n: dict(zip(('verts', 'faces'), box_mesh(assets['ycb'][n]['bbox3d']))) for n in names}
    path = src if os.path.exists(src) else os.path.join(asset_root, 'ours', 'object_mesh_info.pkl')
    try:
        with open(path, 'rb') as f:
            mesh = pickle.load(f)
    except Exception as e:
        raise AssetError(f'ycb: {path} cannot be re-opened for the object meshes ({type(e).__name__}: {e})') from e
    out = {}
    for n in names:
        entry = mesh.get(n, {})
        if 'faces' not in entry:
            raise AssetError(f"ycb: {path} entry {n!r} lacks the key 'faces' (--eval_physics needs the object meshes' triangles)")
        v = np.asarray(entry['verts'], np.float64).reshape(-1, 3)
        f = np.asarray(entry['faces'], np.int64).reshape(-1, 3)
        if f.size == 0 or f.min() < 0 or f.max() >= v.shape[0]:
            raise AssetError(f"ycb: {path} entry {n!r}: 'faces' index outside its {v.shape[0]} vertices")
        out[n] = dict(verts=v, faces=f)
    return out


# ------------------------------------------------------------------------------------------------ intersection volume (--eval_volume)
def close_mesh(faces):
    """Closes an open triangle mesh: the boundary edges (used by exactly one face) are chained into loops and every loop is
    fan-triangulated from its lowest vertex index, wound so that every edge of the result appears once in each direction.  Deterministic
    (loops in ascending order of their lowest vertex); a closed mesh comes back unchanged.  An edge used more than once in the same
    direction, or a boundary vertex where two loops touch, is non-manifold: AssetError.  (F, 3) int64 -> (F', 3) int64."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    seen = {}
    for a, b in edges.tolist():
        if a == b or (a, b) in seen:
            raise AssetError(f'close_mesh: non-manifold edge ({a}, {b}): used more than once in the same direction')
        seen[(a, b)] = True
    # a boundary edge (a, b) has no twin (b, a); the closing faces run along it backwards: b -> a
    nxt = {}
    for a, b in seen:
        if (b, a) not in seen:
            if b in nxt:
                raise AssetError(f'close_mesh: non-manifold boundary at vertex {b}: two boundary loops touch')
            nxt[b] = a
    if not nxt:
        return f.copy()
    if sorted(nxt) != sorted(nxt.values()):
        raise AssetError('close_mesh: the boundary edges do not chain into loops')
    extra, left = [], set(nxt)
    while left:
        start = min(left)
        loop, v = [], start
        while v in left:
            left.discard(v)
            loop.append(v)
            v = nxt[v]
        if v != start or len(loop) < 3:
            raise AssetError(f'close_mesh: the boundary through vertex {start} does not close into a loop of three or more edges')
        extra += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return np.concatenate([f, np.array(extra, np.int64).reshape(-1, 3)])


def hand_faces(assets):
    """the closed face list of the hand mesh, (F, 3) int64: ``assets['mano']['faces']`` (MANO_RIGHT.pkl's ``f``: 1 538 faces, the wrist
    hole is one boundary loop -> 1 552; the synthetic table: the convex hull of v_template, closed already) through close_mesh"""
    mano = assets['mano']
    if 'faces' not in mano:
        raise AssetError("mano: the table carries no 'faces' (--eval_volume needs the hand mesh's triangles)")
    return close_mesh(mano['faces'])


def solid_lattice(verts, faces, pitch):
    """The cell centres of the lattice of pitch h over a mesh's bbox [lo, hi]: n_a = ceil((hi_a - lo_a) / h) cells per axis, centres
    c = lo + (i + 1/2, j + 1/2, k + 1/2) h computed in fp64 and rounded ONCE to fp32 (the fp32 values are the points: they go through the
    fp32-vertex interface of the kernels unchanged), k fastest.  Which centres are inside the mesh -- the solid -- is the caller's business
    (ops: the single-pose penetration kernel at identity pose).  -> (centres (P, 3) fp32, dims (3,) int64).
    Not a surface voxelisation: trimesh's default ``voxelized()`` marks the cells the surface passes through."""
    h = float(pitch)
    if not h > 0.0:
        raise AssetError(f'solid_lattice: the pitch must be positive ({pitch})')
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)].reshape(-1, 3)
    lo, hi = tri.min(0), tri.max(0)
    dims = np.maximum(np.ceil((hi - lo) / h), 1).astype(np.int64)
    ax = [lo[a] + (np.arange(dims[a], dtype=np.float64) + 0.5) * h for a in range(3)]
    c = np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)
    return np.ascontiguousarray(c.astype(np.float32)), dims


def solid_columns(pts):
    """Run starts of equal (x, y) in a lattice-ordered (P, 3) fp32 point set (the kept centres of ``solid_lattice``: k fastest, so the
    centres of one lattice column (i, j) are one contiguous run with the same fp32 x and y, whatever gaps the solid leaves along k; an
    empty column has no run).  -> col_start (C + 1,) int32: the index of every run's first point, then P.  The runs are what
    ``vpho_obj_solid_columns`` (include/vpho_hip.h) hands to the column-walk kernel; x, y are compared as bits of the fp32 values."""
    p = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))
    n = p.shape[0]
    if n == 0:
        return np.zeros(1, np.int32)
    xy = p[:, :2].copy().view(np.uint32)
    new = np.concatenate([[True], (xy[1:] != xy[:-1]).any(1)])
    return np.concatenate([np.nonzero(new)[0], [n]]).astype(np.int32)

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

"""Golden vectors for the penetration metric (--eval_physics): the inside flags of the reference's own
``MeshIntersector`` (lib/thirdparty/libmesh/inside_mesh.py, the occupancy-networks z-ray parity test at resolution 512).

Run in the build container only.  The reference's ``triangle_hash`` is a Cython extension that is not built there; it is replaced by a
pure-Python module with the same semantics (the triangle's xy bounding cells int-truncated and clamped to [0, res), a query returns
the triangles of the point's own int-truncated cell only, points whose cell is outside the grid get none).  ``check_triangles`` then
filters the candidates exactly, so the flags are the reference's own.

Meshes: two of the synthetic box meshes (vpho_amd.physics_eval.box_mesh of synthetic_assets(0)), a closed non-convex torus, two open
meshes (a box without its top face, a cup: an open cylinder with a bottom).  The last three have their vertices on an integer grid
scaled by powers of two, so that their hash frame is exact and points can be placed exactly on projected edges and vertices.
Query points (float32, as the hand vertices are): random ones in the enlarged bbox, lattice points of the hash frame, points on
projected triangle edges / vertices, and a few outside the box.  ``d`` is the distance of tests/_penetration_fp64.py (ours, not the
reference's: the reference has no distance).  Writes golden_penetration.npz.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import _penetration_fp64 as O  # noqa: E402


class TriangleHash:
    """triangle_hash.pyx, in Python"""

    def __init__(self, triangles, resolution):
        self.res = resolution
        self.cells = {}
        for i, t in enumerate(np.asarray(triangles, np.float64)):
            lo = [min(max(int(min(t[0, j], t[1, j], t[2, j])), 0), resolution - 1) for j in range(2)]
            hi = [min(max(int(max(t[0, j], t[1, j], t[2, j])), 0), resolution - 1) for j in range(2)]
            for x in range(lo[0], hi[0] + 1):
                for y in range(lo[1], hi[1] + 1):
                    self.cells.setdefault(resolution * x + y, []).append(i)

    def query(self, points):
        pi, ti = [], []
        for i, (px, py) in enumerate(np.asarray(points, np.float64)):
            x, y = int(px), int(py)
            if not (0 <= x < self.res and 0 <= y < self.res):
                continue
            for t in self.cells.get(self.res * x + y, ()):
                pi.append(i)
                ti.append(t)
        return np.array(pi, np.int32), np.array(ti, np.int32)


def _reference_intersector():
    pkg = types.ModuleType('libmesh_ref')
    pkg.__path__ = [os.path.join(MG.REF, 'lib', 'thirdparty', 'libmesh')]
    sys.modules['libmesh_ref'] = pkg
    th = types.ModuleType('libmesh_ref.triangle_hash')
    th.TriangleHash = TriangleHash
    sys.modules['libmesh_ref.triangle_hash'] = th
    import importlib
    return importlib.import_module('libmesh_ref.inside_mesh')


# ---------------------------------------------------------------------------------------------------------------- meshes
EXP = np.array([-11, -11, -12])        # model coordinate = (g - 255.5) * 2^EXP per axis, g an integer in [0, 511]


def _grid_to_model(g):
    return (np.asarray(g, np.float64) - 255.5) * np.exp2(EXP)


def _fit_grid(xyz):
    """affine per axis onto [0, 511], rounded: an integer grid mesh whose bbox is exactly [0, 511]^3"""
    lo, hi = xyz.min(0), xyz.max(0)
    return np.rint((xyz - lo) / (hi - lo) * 511)


def torus(nu=48, nv=24, R=1.0, r=0.38):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing='ij')
    xyz = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return _fit_grid(xyz), np.array(faces, np.int64)


def open_box(sub=4):
    from vpho_amd.physics_eval import box_mesh
    g, f = box_mesh(np.array([[0, 0, 0], [511, 511, 511]], np.float64), sub)
    top = np.all(g[f][:, :, 2] == 511, axis=1)
    return g, f[~top]


def cup(n=40, rings=6):
    ang = np.arange(n) * 2 * np.pi / n
    pts = [np.zeros(3)]                                   # bottom centre
    for k in range(rings + 1):                            # ring k at height k / rings
        pts += [np.array([np.cos(a), np.sin(a), k / rings]) for a in ang]
    xyz = np.array(pts)
    ring = lambda k, i: 1 + k * n + (i % n)
    faces = [(0, ring(0, i + 1), ring(0, i)) for i in range(n)]                 # bottom, outward = -z
    for k in range(rings):
        for i in range(n):
            a, b, c, d = ring(k, i), ring(k, i + 1), ring(k + 1, i + 1), ring(k + 1, i)
            faces += [(a, b, c), (a, c, d)]
    return _fit_grid(xyz), np.array(faces, np.int64)


# ---------------------------------------------------------------------------------------------------------------- points
def _points(rng, verts, faces, n_rand, exact):
    lo, hi = verts.min(0), verts.max(0)
    ext = hi - lo
    scale = 511 / ext
    translate = 0.5 - scale * lo
    back = lambda q: (q - translate) / scale
    out = [rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, size=(n_rand, 3))]
    # lattice of the hash frame (integer and half-integer coordinates: cell borders and triangle corners of the grid meshes)
    ax = np.arange(0.0, 512.5, 18.5)
    g = np.stack(np.meshgrid(ax, ax[::3], ax[::4], indexing='ij'), -1).reshape(-1, 3)
    out.append(back(g))
    # projected corners and edge points of random triangles, at random heights inside the box
    tri = (scale * verts[faces] + translate)
    pick = rng.integers(0, len(faces), size=600)
    corner = tri[pick, rng.integers(0, 3, size=600)]
    a, b = tri[pick, 0], tri[pick, 1 + rng.integers(0, 2, size=600)]
    frac = rng.integers(1, 8, size=(600, 1)) / 8.0
    edge = a + frac * (b - a)
    for q in (corner, edge):
        q = q.copy()
        q[:, 2] = rng.uniform(0.5, 511.5, size=len(q)) if not exact else rng.integers(1, 1022, size=len(q)) / 2.0
        out.append(back(q))
    out.append(back(rng.uniform(-40, 552, size=(200, 3))))        # around the box borders, some outside
    p = np.concatenate(out).astype(np.float32)
    if exact:               # grid meshes: every placed point is representable, the float32 rounding must not have moved any
        assert np.array_equal(p[n_rand:-200].astype(np.float64), np.concatenate(out[1:-1]))
    return p


def main():
    from vpho_amd.assets import synthetic_assets
    from vpho_amd.physics_eval import box_mesh
    M = _reference_intersector()
    rng = np.random.default_rng(20261016)
    ycb = synthetic_assets(0)['ycb']
    names = list(ycb)
    meshes = [('box:' + names[0], *box_mesh(ycb[names[0]]['bbox3d']), False),
              ('box:' + names[7], *box_mesh(ycb[names[7]]['bbox3d']), False)]
    for name, (g, f) in (('torus', torus()), ('open_box', open_box()), ('cup', cup())):
        assert g.min() == 0 and g.max() == 511 and (g.min(0) == 0).all() and (g.max(0) == 511).all()
        meshes.append((name, _grid_to_model(g), f, True))
    V, F, P, C, D, VO, FO, PO, names_out = [], [], [], [], [], [0], [0], [0], []
    for name, verts, faces, exact in meshes:
        pts = _points(rng, verts, faces, 2400, exact)
        mesh = types.SimpleNamespace(vertices=verts, faces=faces)
        ref = M.check_mesh_contains(mesh, pts.astype(np.float64), 512)
        ours = O.contains(verts, faces, pts)
        assert np.array_equal(ref, ours), (name, int((ref != ours).sum()))
        d = O.distance(verts, faces, pts)
        print(f'{name}: {len(faces)} triangles, {len(pts)} points, {int(ref.sum())} inside')
        V.append(verts); F.append(faces); P.append(pts); C.append(ref); D.append(d)
        VO.append(VO[-1] + len(verts)); FO.append(FO[-1] + len(faces)); PO.append(PO[-1] + len(pts)); names_out.append(name)
    np.savez_compressed(os.path.join(HERE, 'golden_penetration.npz'), names=np.array(names_out), verts=np.concatenate(V),
                        faces=np.concatenate(F).astype(np.int32), vert_offset=np.array(VO), face_offset=np.array(FO),
                        point_offset=np.array(PO), points=np.concatenate(P), contains_ref=np.concatenate(C), d_ours=np.concatenate(D))


if __name__ == '__main__':
    main()

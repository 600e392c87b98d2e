"""Inputs shared by tests/test_penetration_multi_cpu.py and tests/test_gpu_penetration_multi.py: three meshes with the SAME, exactly
representable hash frame, and per mesh a pool of fp32 points in the model frame -- random ones around the surface and a hand-placed set
on the places where the multi-hypothesis kernel's filters could go wrong.

Every mesh is fitted into the box [LO, LO + EXT] with EXT = 511 * 2^-12 (x, z) / 511 * 2^-13 (y), so scale = (4096, 8192, 4096) and
translate = (256.5, 256.5, 256.5) are exact and q = scale * p + translate is exact for the dyadic p placed here: a point can sit exactly
on a far face (q == 512), on a hash-cell or column boundary (q a multiple of 1 / 8) or on a projected edge.
"""
import functools

import numpy as np

import tests._penetration_fp64 as O

EXT = np.array([511.0 / 4096, 511.0 / 8192, 511.0 / 4096])
LO = np.array([-256.0 / 4096, -256.0 / 8192, -256.0 / 4096])
SCALE = 511.0 / EXT
TRANSLATE = 0.5 - SCALE * LO
N_IMG, S, V = 3, 5, 70                      # none a power of two or a wave multiple
# (mesh of image 0, 1, 2): two objects per launch, one id repeated; every mesh is the repeated one once
ID_CASES = ((0, 1, 0), (1, 2, 1), (2, 0, 2))
MESH_NAMES = ('box', 'torus', 'torus_open')


def _fit(verts):
    """affine map of the vertices' bounding box onto [LO, LO + EXT]: the extreme vertices land exactly on the faces"""
    lo, hi = verts.min(0), verts.max(0)
    out = (verts - lo) / (hi - lo) * EXT + LO
    return out.astype(np.float32).astype(np.float64)


def torus(nu=23, nv=13, drop_quad=None):
    """physics_eval.torus_mesh fitted into the box: 2 nu nv triangles (598: no multiple of a cluster or a tile); z-rays cross it 0, 2 or
    4 times.  ``drop_quad``: index of a quad to leave out (an open mesh)"""
    from vpho_amd.physics_eval import torus_mesh
    verts, faces = torus_mesh(nu, nv, drop_quad=drop_quad)
    return _fit(verts), faces


@functools.lru_cache(maxsize=None)
def meshes():
    from vpho_amd.physics_eval import box_mesh
    corners = np.array([[x, y, z] for x in (LO[0], LO[0] + EXT[0]) for y in (LO[1], LO[1] + EXT[1]) for z in (LO[2], LO[2] + EXT[2])])
    bv, bf = box_mesh(corners)
    tv, tf = torus()
    ov, of = torus(drop_quad=7 * 13 + 3)
    assert len(bf) == 3072 and len(tf) == 598 and len(of) == 596
    return {'box': dict(verts=bv, faces=bf), 'torus': dict(verts=tv, faces=tf), 'torus_open': dict(verts=ov, faces=of)}


def hand_placed(mesh):
    """model-frame fp32 points on the filters' edges; q = SCALE * p + TRANSLATE is exact for the dyadic ones"""
    q_of = lambda q: (np.asarray(q, np.float64) - TRANSLATE) / SCALE
    v = mesh['verts']
    pts = []
    # far outside the bounding box (the cull), on each side
    pts += [np.array(d) for d in ([5.0, 0.0078125, 0], [0.03125, -5.0, 0], [0, 0.015625, 5.0], [-3.0, 4.0, 2.0])]
    # exactly on the far faces: q == 512 has no cell (x, y) / is still inside the cull (z), and q == 0 on the near faces
    pts += [q_of([512.0, 300.25, 200.5]), q_of([130.25, 512.0, 256.5]), q_of([512.0, 512.0, 100.5]), q_of([200.25, 260.5, 512.0]),
            q_of([0.0, 256.25, 256.5]), q_of([256.25, 0.0, 256.5])]
    # exactly on column boundaries (multiples of 8 cells) and on hash-cell boundaries, inside and near the surface
    for qx, qy in ((256.0, 256.0), (248.0, 263.5), (255.5, 264.0), (64.0, 256.25), (448.0, 250.0), (257.0, 255.0), (300.0, 256.5), (301.5, 257.0)):
        for qz in (256.5, 40.25, 505.0):
            pts.append(q_of([qx, qy, qz]))
    # on a projected edge: the xy of an edge midpoint of the first faces (dyadic corners: the midpoint is exact), at several depths
    f = mesh['faces']
    for t in (0, 1, len(f) // 2, len(f) - 1):
        m = (v[f[t, 0]] + v[f[t, 1]]) / 2
        pts += [m, m + [0, 0, 1.0 / 128], m - [0, 0, 1.0 / 64]]
    # at mesh vertices (distance 0) and straight above / below them (the ray passes through a vertex of the projection)
    for i in (0, 1, len(v) // 3, len(v) - 1):
        pts += [v[i], v[i] + [0, 0, 1.0 / 256], v[i] - [0, 0, 1.0 / 256]]
    # the box's corners are dyadic, so everything above is fp32-exact for it; the torus' corners are arbitrary fp32 numbers: an edge
    # midpoint or a shifted z of it may round (its x and y at and above a vertex stay exact)
    pts = np.array(pts, np.float64)
    return pts.astype(np.float32).astype(np.float64)


def _random_points(name, mesh, rng, count):
    if name == 'box':
        return LO + EXT * rng.uniform(-0.2, 1.2, size=(count, 3))
    # around the tube: a surface vertex plus an offset of up to a tube diameter
    v = mesh['verts'][rng.integers(0, len(mesh['verts']), count)]
    return v + rng.normal(size=(count, 3)) * np.array([0.012, 0.008, 0.012])


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


@functools.lru_cache(maxsize=None)
def case(which):
    """One launch: dict(ids, verts (n, S, V, 3) fp32 camera frame, rt (n, S, 3, 4) fp64, p (n, S, V, 3) fp64 the model-frame points the
    kernel sees, inside / dist (n, S, V) by the fp64 restatement).  Hypothesis 0 of every image has the identity pose and carries the
    hand-placed points (exact); the others have random poses and random points."""
    M = meshes()
    ids = ID_CASES[which]
    rng = np.random.default_rng(100 + which)
    verts = np.zeros((N_IMG, S, V, 3), np.float32)
    rt = np.zeros((N_IMG, S, 3, 4))
    for i, o in enumerate(ids):
        name = MESH_NAMES[o]
        hp = hand_placed(M[name])
        for s in range(S):
            pts = _random_points(name, M[name], rng, V).astype(np.float32).astype(np.float64)
            if s == 0:
                rt[i, s, :, :3] = np.eye(3)
                assert len(hp) <= V
                pts[:len(hp)] = hp
            else:
                rt[i, s, :, :3], rt[i, s, :, 3] = _random_rotation(rng), rng.uniform(-0.2, 0.2, 3) + [0, 0, 0.6]
            verts[i, s] = (pts @ rt[i, s, :, :3].T + rt[i, s, :, 3]).astype(np.float32)
    p = O.model_frame(verts.reshape(N_IMG * S, V, 3).astype(np.float64), rt.reshape(N_IMG * S, 3, 4)).reshape(N_IMG, S, V, 3)
    inside = np.zeros((N_IMG, S, V), bool)
    dist = np.zeros((N_IMG, S, V))
    for i, o in enumerate(ids):
        m = M[MESH_NAMES[o]]
        inside[i] = O.contains(m['verts'], m['faces'], p[i].reshape(-1, 3)).reshape(S, V)
        dist[i] = O.distance(m['verts'], m['faces'], p[i].reshape(-1, 3)).reshape(S, V)
    return dict(ids=ids, verts=verts, rt=rt, p=p, inside=inside, dist=dist)


def inside_share():
    """per mesh the share of all test points the fp64 restatement puts inside (the tests assert 10 % .. 90 %)"""
    tot = {n: [0, 0] for n in MESH_NAMES}
    for w in range(len(ID_CASES)):
        c = case(w)
        for i, o in enumerate(c['ids']):
            tot[MESH_NAMES[o]][0] += int(c['inside'][i].sum())
            tot[MESH_NAMES[o]][1] += c['inside'][i].size
    return {n: a / b for n, (a, b) in tot.items()}

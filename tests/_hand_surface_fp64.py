"""numpy float64 restatements for csrc/hand_surface.hip and the contact chain behind it, by another route than the kernel takes:
vertex normals by a loop over the vertices and their incident faces with corner angles from ``arctan2(|u x w|, u . w)`` (the kernel:
face records first, ``acos`` of unit vectors), the fill rule, and the hand -> object contact chain with a brute-force nearest neighbour.
Also the closed test meshes the CPU and the GPU tests share.  No GPU, no package import."""
import numpy as np

GROUP_OF_ANCHOR = np.array([1, 1, 1, 1, 1, 0, 1, 2, 2, 2, 2, 2, 0, 3, 3, 3, 3, 3, 0, 0, 4, 4, 4, 4, 4, 0, 0, 5, 5, 5, 5, 5])
CALL_GATES = dict(normal_thresh=(-0.01, 0.01), vertical_thresh=0.005, decay=(-0.005, 0.005))     # args.py:44-45, base.py:898-905


# ----------------------------------------------------------------------------------------------------------------- normals and fill
def _norm(a):
    return np.sqrt((a * a).sum(-1))


def vertex_sums(verts, faces):
    """verts (n,V,3), faces (F,3) -> (sum (n,V,3) of angle * unit face normal over the incident faces in ascending face index,
    angle_sum (n,V)).  A face whose cross product is exactly zero contributes nothing; a NaN goes through."""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n, V = verts.shape[:2]
    incident = [[] for _ in range(V)]
    for f, tri in enumerate(faces):
        for c in range(3):
            incident[tri[c]].append((f, c))
    total, angles = np.zeros((n, V, 3)), np.zeros((n, V))
    with np.errstate(invalid='ignore', divide='ignore'):
        for v in range(V):
            for f, c in incident[v]:
                tri = faces[f]
                cr = np.cross(verts[:, tri[1]] - verts[:, tri[0]], verts[:, tri[2]] - verts[:, tri[0]])
                area2 = _norm(cr)
                u, w = verts[:, tri[(c + 1) % 3]] - verts[:, tri[c]], verts[:, tri[(c + 2) % 3]] - verts[:, tri[c]]
                ang = np.arctan2(_norm(np.cross(u, w)), (u * w).sum(-1))
                live = area2 != 0
                safe = np.where(live, area2, 1.0)
                total[:, v] += np.where(live[:, None], ang[:, None] * cr / safe[:, None], 0.0)
                angles[:, v] += np.where(live, ang, 0.0)
    return total, angles


def renorm(nrm):
    return nrm / (_norm(nrm)[..., None] + 1e-20)


def vertex_normals(verts, faces):
    """-> (normals (n,V,3) after the first n / (|n| + 1e-20), |sum| (n,V), angle_sum (n,V))"""
    total, angles = vertex_sums(verts, faces)
    length = _norm(total)
    with np.errstate(invalid='ignore', divide='ignore'):
        unit = np.where((length == 0)[..., None], 0.0, total / np.where(length == 0, 1.0, length)[..., None])
    return renorm(unit), length, angles


def fill(x, links, alpha):
    """hand_fn.py:356-384: (..,V,3) -> (..,V+L,3), ``1 - alpha`` formed in float64 as Python does"""
    x = np.asarray(x, np.float64)
    links = np.asarray(links, np.int64).reshape(-1, 2)
    alpha = np.asarray(alpha, np.float64).reshape(-1)
    if len(links) == 0:
        return x.copy()
    al, be = alpha[:, None], (1.0 - alpha)[:, None]
    return np.concatenate([x, al * x[..., links[:, 0], :] + be * x[..., links[:, 1], :]], -2)


def hand_surface(verts, faces, links, alpha):
    """-> verts_filled, normals_filled (float64), |sum|, angle_sum: base.py:887-891 with the normal rule of the kernel's header"""
    nrm, length, angles = vertex_normals(verts, faces)
    return fill(verts, links, alpha), renorm(fill(nrm, links, alpha)), length, angles


def comparable_rows(length, angles, links, V):
    """rows of the filled outputs whose normal is well defined: |sum| >= 1e-6 * angle sum for the vertex itself or, for a filled row, for
    both of its sources"""
    with np.errstate(invalid='ignore'):
        ok = (length >= 1e-6 * angles) & (angles > 0)
    links = np.asarray(links, np.int64).reshape(-1, 2)
    if len(links) == 0:
        return ok
    return np.concatenate([ok, ok[..., links[:, 0]] & ok[..., links[:, 1]]], -1)


# ----------------------------------------------------------------------------------------------------------------- the contact chain
def contact_weight(x, normal_thresh, decay):
    mid1, mid2 = (decay[0] + normal_thresh[0]) / 2, (decay[1] + normal_thresh[1]) / 2

    def fn(x):
        with np.errstate(over='ignore'):
            m1, m2 = 1 + np.exp(-1600 * (x - mid1)), 1 + np.exp(1600 * (x - mid2))
        out = 1 / (m1 * m2 + 1e-10)
        out[~np.isfinite(m1) | ~np.isfinite(m2)] = 0
        return out
    return fn(np.asarray(x, np.float64)) / fn(np.array([0.0]))


def hand_contact(hand_verts, hand_normals, obj_verts, normal_thresh=(-0.015, 0.01), vertical_thresh=0.01, decay=(-0.005, 0.005)):
    """the hand -> object half of detect_hand_and_object_contact (physics_fn.py:68-79,96-110) for ONE sample with a brute-force nearest
    neighbour (ties: the smaller index).  Returns a dict: weight, mask, nd, vd, index, gap (second nearest distance - nearest)."""
    hv, hn, ov = (np.asarray(a, np.float64) for a in (hand_verts, hand_normals, obj_verts))
    d = np.sqrt(((hv[:, None, :] - ov[None, :, :]) ** 2).sum(-1))
    idx = d.argmin(1)
    two = np.partition(d, 1, axis=1)[:, :2] if d.shape[1] > 1 else np.concatenate([d, d + np.inf], 1)
    vec = hv - ov[idx]
    nd = (vec * hn).sum(-1)
    vd = _norm(vec - nd[:, None] * hn)
    mask = (nd > normal_thresh[0]) & (nd < normal_thresh[1]) & (vd < vertical_thresh)
    weight = contact_weight(nd, normal_thresh, decay)
    weight[~mask] = 0
    return dict(weight=weight, mask=mask, nd=nd, vd=vd, index=idx, gap=two[:, 1] - two[:, 0])


def band(chain, normal_thresh, vertical_thresh, near=1e-5, tie=1e-6):
    """vertices a float32 evaluation may decide differently: a gate within ``near`` metres, or two nearest points within ``tie``"""
    nd, vd = chain['nd'], chain['vd']
    return (np.abs(nd - normal_thresh[0]) < near) | (np.abs(nd - normal_thresh[1]) < near) | (np.abs(vd - vertical_thresh) < near) | (chain['gap'] < tie)


def force_contact(hand_contact_map, face_idx, anchor_weight):
    """ForceAnchor.get_force_contact (physics_fn.py:201-208): (..,>=778) -> (..,32)"""
    w = np.concatenate([np.ones((32, 1)), np.asarray(anchor_weight, np.float64).reshape(32, 2)], 1)
    face_idx = np.asarray(face_idx, np.int64).reshape(32, 3)
    return (np.asarray(hand_contact_map, np.float64)[..., face_idx] * (w / w.sum(1, keepdims=True))).sum(-1)


def group_sums(fc):
    return np.stack([fc[..., GROUP_OF_ANCHOR == g].sum(-1) for g in range(6)], -1)


def is_grasped(fc, thresh=0.0):
    """check_is_grasped (physics_fn.py:210-221) per sample"""
    return (group_sums(fc) > thresh).sum(-1) >= 2


# ----------------------------------------------------------------------------------------------------------------- test meshes
def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    return v, _outward(v, f)


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v, _outward(v, f)


def cube(seed=0):
    """the unit cube's 8 corners and 12 triangles, each square face cut along a diagonal chosen by ``seed``"""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    r = np.random.default_rng(seed)
    f = []
    for axis in range(3):
        for side in (-1, 1):
            q = [i for i in range(8) if v[i, axis] == side]
            a, b = [k for k in range(3) if k != axis]
            q.sort(key=lambda i: np.arctan2(v[i, b], v[i, a]))
            if r.random() < 0.5:
                q = q[1:] + q[:1]
            f += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return v, _outward(v, np.array(f))


def _outward(v, f):
    """wind every face of a star-shaped mesh about the origin outwards"""
    f = np.array(f, np.int64)
    tri = v[f]
    flip = (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) * tri.mean(1)).sum(1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return f


def ellipsoid(rings=8, segments=97, axes=(0.09, 0.04, 0.015), bump=0.25):
    """A closed UV ellipsoid with a smooth bump: rings * segments + 2 vertices (778), 2 * rings * segments faces (1552); the two poles have
    valence ``segments``.  Vertex 0 is the north pole, the last vertex the south pole.  Metres."""
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segments) / segments
    T, P = np.meshgrid(th, ph, indexing='ij')
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    d = np.concatenate([[[0, 0, 1.0]], d, [[0, 0, -1.0]]])
    r = 1 + bump * np.exp(-((d - np.array([0.6, 0.0, 0.8])) ** 2).sum(-1) / 0.18)
    v = d * r[:, None] * np.asarray(axes)
    idx = lambda i, j: 1 + i * segments + j % segments
    last = 1 + rings * segments
    f = []
    for j in range(segments):
        f.append([0, idx(0, j), idx(0, j + 1)])
        for i in range(rings - 1):
            f.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            f.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
        f.append([last, idx(rings - 1, j + 1), idx(rings - 1, j)])
    f = _outward(v, f)
    return v, f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def posed(v, seed, scale=1.0):
    """a rigid motion (and a uniform scale) of a mesh, rounded to float32 as the kernel reads it"""
    r = np.random.default_rng(seed)
    q = r.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return ((scale * v) @ R.T + r.uniform(-0.05, 0.05, 3)).astype(np.float32)


def grazing_cloud(hand_filled, normals_filled, seed, n=2048):
    """an object point cloud placed so that part of the hand surface lies inside the contact gates: points next to a patch of the
    surface, pushed along the normals by -6 .. +12 mm, plus points far away"""
    r = np.random.default_rng(seed)
    hv, hn = np.asarray(hand_filled, np.float64), np.asarray(normals_filled, np.float64)
    centre = hv[r.integers(0, len(hv))]
    near = np.argsort(_norm(hv - centre))[:len(hv) // 2]
    pick = r.choice(near, n // 2)
    tang = r.normal(0, 0.0015, (n // 2, 3))
    pts = hv[pick] - hn[pick] * r.uniform(-0.006, 0.012, (n // 2, 1)) + tang
    far = hv.mean(0) + r.normal(0, 0.08, (n - n // 2, 3))
    return np.concatenate([pts, far]).astype(np.float32)

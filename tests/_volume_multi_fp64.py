"""float64 numpy helpers of the multi-hypothesis intersection-volume tests:

* ``column_walk_inside(qv, faces, pts, col_start)``: the restatement of the column-walk kernel -- the 19 parity fields of
  physics_eval.mesh_tables on the posed mesh (as tests/_volume_fp64.hand_inside), then per lattice COLUMN (a run of ``pts`` with one
  fp32 x, y: physics_eval.solid_columns) the cell test, the strict containment and the plane depth ONCE per (column, face) from the
  column's first centre, and only for the faces that hit the z cull and the two-bucket parity per centre.  That it equals
  ``hand_inside`` flag for flag is the CPU proof of the column-sharing argument;
* ``table_rule(per_hyp, pitch)``: the one | best | mean reduction of the kernel on a torch fp64 tensor, with its NaN rule;
* the input generators of the GPU tests and of scripts/volume_multi_bench.py: small rigid perturbations of a posed hand, the fixture's
  three hand meshes as ONE face list, a 1 552-face torus hand, a torus object and a tall box object.
"""
import numpy as np

RES = 512


def column_walk_inside(qv, faces, pts, col_start):
    """(P,) bool.  qv (V, 3) fp64 model-frame hand vertices, faces (F, 3), pts (P, 3) fp32 in lattice order, col_start (C + 1,)"""
    from vpho_amd.physics_eval import mesh_tables
    r, scale, translate = mesh_tables(qv, faces)
    r = r[:, :19]
    p = np.asarray(pts, np.float32).astype(np.float64)
    out = np.zeros(len(p), bool)
    for c in range(len(col_start) - 1):
        s, e = int(col_start[c]), int(col_start[c + 1])
        # ---- the xy part, once per (column, face), from the column's first centre
        qx, qy = scale[0] * p[s, 0] + translate[0], scale[1] * p[s, 1] + translate[1]
        if not (0.0 <= qx <= RES and 0.0 <= qy <= RES):
            continue                                                           # NaN compares false: no cell either
        cx, cy = np.trunc(qx), np.trunc(qy)
        if not (cx < RES and cy < RES):
            continue
        with np.errstate(invalid='ignore', over='ignore'):
            cell = (r[:, 15] <= cx) & (cx <= r[:, 16]) & (r[:, 17] <= cy) & (cy <= r[:, 18])
            y0, y1 = qx - r[:, 0], qy - r[:, 1]
            u = (r[:, 5] * y0 - r[:, 3] * y1) * r[:, 6]
            w = (-r[:, 4] * y0 + r[:, 2] * y1) * r[:, 6]
            suv = u + w
            hit = cell & (0.0 < u) & (u < r[:, 7]) & (0.0 < w) & (w < r[:, 7]) & (0.0 < suv) & (suv < r[:, 7])
            alpha = r[:, 10] * (r[:, 8] - qx) + r[:, 11] * (r[:, 9] - qy)
            depth = r[:, 14] + alpha * r[:, 12]
        h = np.nonzero(hit)[0]
        if len(h) == 0:
            continue
        # ---- the z part, per centre of the column, for the faces that hit
        qz = scale[2] * p[s:e, 2] + translate[2]
        with np.errstate(invalid='ignore', over='ignore'):
            in_box = (0.0 <= qz) & (qz <= RES)
            zz = qz[:, None] * r[h, 13][None]
            c0 = (depth[h][None] >= zz).sum(1)
            c1 = (depth[h][None] < zz).sum(1)
        out[s:e] = in_box & (c0 % 2 == 1) & (c1 % 2 == 1)
    return out


def table_rule(per_hyp, pitch):
    """per_hyp (n, S, 2) torch fp64 = n_cells | IV -> (n, 6) one_IV, one_cells | best_IV, best_cells | mean_IV, mean_cells"""
    import torch
    cells, iv = per_hyp[..., 0], per_hyp[..., 1]
    n, S = cells.shape
    nan = per_hyp.isnan().any(-1).any(-1)
    total = torch.where(cells.isnan(), torch.zeros_like(cells), cells).to(torch.int64).sum(1)       # an exact integer sum
    mean_cells = total.double() / float(S)
    cell_volume = (pitch * pitch) * pitch
    big = torch.full_like(cells, float('inf'))
    tab = torch.stack([iv[:, 0], cells[:, 0], torch.where(iv.isnan(), big, iv).amin(1), torch.where(cells.isnan(), big, cells).amin(1),
                       cell_volume * mean_cells, mean_cells], 1)
    tab[nan, 2:] = float('nan')
    return tab


# ------------------------------------------------------------------------------------------------------------ input generators
def _small_rotation(rng, deg):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(rng.uniform(-deg, deg))
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def perturbed_hypotheses(verts_cam, rt, S, seed, mm=4.0, deg=5.0):
    """hypothesis 0 = (verts_cam, rt) as given; 1 .. S-1: the hand turned by up to ``deg`` degrees about its centroid and moved by up to
    ``mm`` millimetres per axis, the object pose turned and moved by a quarter of that.  -> (S, V, 3) fp32, (S, 3, 4) fp64"""
    rng = np.random.default_rng(seed)
    v0 = np.asarray(verts_cam, np.float32)
    rt = np.asarray(rt, np.float64)
    vs, rts = [v0], [rt]
    c = v0.astype(np.float64).mean(0)
    for _ in range(1, S):
        dR, dt = _small_rotation(rng, deg), rng.uniform(-mm, mm, 3) * 1e-3
        vs.append(((v0.astype(np.float64) - c) @ dR.T + c + dt).astype(np.float32))
        oR, ot = _small_rotation(rng, deg / 4), rng.uniform(-mm, mm, 3) * 0.25e-3
        rts.append(np.concatenate([rt[:, :3] @ oR, (rt[:, 3] + ot)[:, None]], 1))
    return np.stack(vs), np.stack(rts)


def fixture_union(G, pairs=(0, 1, 2)):
    """The fixture's hand meshes as ONE face list (the kernels share one list among all pairs): the vertex arrays concatenated, every face
    list shifted to its own block.  In the image of pair i only block pair_hand[i] holds the hand; the other blocks' vertices all sit on
    the hand's vertex 0, so their faces are points: no area (det A = 0: the strict containment never holds), and a corner of the hand
    itself, so the bbox -- and with it every bit of the hash frame -- is the hand's own.  -> faces (F, 3) int64, [(V, 3) fp32 per pair]"""
    hands = sorted({int(G['pair_hand'][i]) for i in pairs})
    size = {h: int(G[f'hand{h}_faces'].max()) + 1 for h in hands}
    first = {h: sum(size[k] for k in hands if k < h) for h in hands}
    faces = np.concatenate([G[f'hand{h}_faces'].astype(np.int64) + first[h] for h in hands])
    V = sum(size.values())
    verts = []
    for i in pairs:
        h = int(G['pair_hand'][i])
        own = G[f'pair{i}_verts_cam']
        assert own.shape[0] == size[h] and (G[f'hand{h}_faces'] == 0).any()
        v = np.repeat(own[:1], V, 0)
        v[first[h]:first[h] + size[h]] = own
        verts.append(np.ascontiguousarray(v, np.float32))
    return faces, verts


def torus_hand(major=0.035, minor=0.014, extra_verts=2):
    """a closed torus of 1 552 faces (MANO's closed mesh: seven record tiles of 256, the last one partial) on 776 + extra_verts vertices
    (the extra ones, copies of vertex 0, belong to no face) -> verts (778, 3) fp64, faces (1552, 3) int64"""
    from vpho_amd.physics_eval import torus_mesh
    v, f = torus_mesh(97, 8, major, minor)
    assert f.shape == (1552, 3)
    return np.concatenate([v, np.repeat(v[:1], extra_verts, 0)]), f


def torus_object(major=0.045, minor=0.018):
    """a torus about the y axis as an OBJECT: along z a lattice column crosses the ring twice (gaps in k), and the corners of its bbox in
    x, y hold empty columns"""
    from vpho_amd.physics_eval import torus_mesh
    v, f = torus_mesh(24, 12, major, minor)
    return dict(verts=v, faces=f)


def tall_box_object(half=(0.0074, 0.0059, 0.1043)):
    """a box that is long along z: at a 3 mm pitch 5 x 4 lattice columns of 70 centres, more than one 64-centre piece (not square in
    x, y: the centres of a square's diagonal columns would lie on the diagonal edges of box_mesh's end faces, where the parity rule
    counts no crossing)"""
    from vpho_amd.physics_eval import box_mesh
    h = np.asarray(half, np.float64)
    v, f = box_mesh(np.stack([-h, h]), 4)
    return dict(verts=v, faces=f)


def pose_into(rng, hand_verts, centre, tilt_deg=0.0, t_cam=(0.02, -0.03, 0.6)):
    """hand_verts (model frame of the hand) tilted about x by ``tilt_deg``, put at ``centre`` of the object's model frame, then the pair
    moved into the camera frame by a random object pose -> (V, 3) fp32 camera-frame vertices, (3, 4) fp64 object pose"""
    a = np.deg2rad(tilt_deg)
    Rh = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    Ro = q if np.linalg.det(q) > 0 else -q
    hm = np.asarray(hand_verts, np.float64) @ Rh.T + np.asarray(centre, np.float64)
    rt = np.concatenate([Ro, np.asarray(t_cam, np.float64)[:, None]], 1)
    return (hm @ Ro.T + rt[:, 3]).astype(np.float32), rt

"""Golden vectors for the hand-object intersection volume (--eval_volume): the inside flags of the reference's own
``MeshIntersector`` (lib/thirdparty/libmesh/inside_mesh.py, resolution 512) for the cell centres of object lattices against posed
"hand" meshes.

Run in the build container only.  The reference's ``triangle_hash`` is replaced by the pure-Python stand-in of
make_golden_penetration.py (same semantics); ``check_triangles`` filters the candidates exactly, so the flags are the reference's own.

Hands: ``torus_mesh(12, 8)`` scaled to hand size, the same torus with a quad dropped and re-closed by ``close_mesh``, a ``box_mesh(sub=2)``.
Objects: two boxes whose lattices at the 5 mm pitch are 8 x 8 x 8 and 10 x 6 x 7 cells.  Four pairs: torus / box A, re-closed torus /
box B, box hand wholly inside box A (the hand's bbox inside the object), torus far from box B (no overlap).  Every pair is stored twice:
the hand in the object's model frame as fp32 (``verts_model``: with the identity pose p = v exactly) and in the camera frame under a
random pose, fp32(R p + t) (``verts_cam`` with ``rt``); the reference sees the mesh q_v = R^T (v - t) in the documented order of
operations (tests/_volume_fp64.py: model_frame).  Stored per pair and per lattice centre: the reference's flag under both poses and
whether the centre lies within 1e-9 hash units of a projected hand edge; per object: the fp32 centres, the lattice dims and the
reference's inside flag of every centre (the solid).  The generator asserts that the four n_cells differ, that the no-overlap and
bbox-inside pairs are what they claim, and that at most 0.1 % of the (centre, pair) combinations lie in the edge band; otherwise it
moves on to the next seed.  Writes golden_volume.npz.
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
import make_golden_penetration as MP  # noqa: E402
import _volume_fp64 as VO  # noqa: E402

PITCH = 0.005


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def _hands():
    from vpho_amd.physics_eval import box_mesh, close_mesh, torus_mesh
    tv, tf = torus_mesh(12, 8)
    _, of = torus_mesh(12, 8, drop_quad=29)
    bv, bf = box_mesh(np.array([[-0.0093, -0.0081, -0.0102], [0.0093, 0.0081, 0.0102]]), sub=2)
    return [('torus', tv * 0.03, tf), ('torus_reclosed', tv * 0.03, close_mesh(of)), ('box', bv, bf)]


def _objects():
    from vpho_amd.physics_eval import box_mesh
    a = np.array([[-0.0191, -0.0203, -0.0187], [0.0194, 0.0182, 0.0198]])          # 0.0385^3: 8 x 8 x 8 cells
    b = np.array([[-0.0243, -0.0137, -0.0171], [0.0237, 0.0143, 0.0159]])          # 0.048 x 0.028 x 0.033: 10 x 6 x 7
    return [('box_a', *box_mesh(a, sub=4)), ('box_b', *box_mesh(b, sub=4))]


def _attempt(seed, M):
    from vpho_amd.physics_eval import solid_lattice
    rng = np.random.default_rng(seed)
    hands, objects = _hands(), _objects()
    lattices = []
    for name, ov, of in objects:
        c, dims = solid_lattice(ov, of, PITCH)
        solid = M.check_mesh_contains(types.SimpleNamespace(vertices=ov, faces=of), c.astype(np.float64), 512)
        lattices.append((c, dims, solid))
    # (hand, object, where the hand's centre goes in the model frame)
    plan = [(0, 0, rng.uniform(-0.004, 0.004, 3) + np.array([0.03, 0.0, 0.0])),
            (1, 1, rng.uniform(-0.004, 0.004, 3) + np.array([0.0, 0.0, 0.031])),
            (2, 0, rng.uniform(-0.002, 0.002, 3)),
            (0, 1, np.array([0.16, 0.05, -0.11]) + rng.uniform(-0.01, 0.01, 3))]
    pairs = []
    for hi_, oi, centre in plan:
        _, hv, hf = hands[hi_]
        c, dims, solid = lattices[oi]
        Rh = _rotation(rng) if hi_ != 2 else np.eye(3)
        vm = (hv @ Rh.T + centre).astype(np.float32)                         # the hand in the model frame
        rt = np.concatenate([_rotation(rng), (np.array([0.05, -0.03, 0.62]) + rng.uniform(-0.05, 0.05, 3))[:, None]], 1)
        vc = (vm.astype(np.float64) @ rt[:, :3].T + rt[:, 3]).astype(np.float32)
        eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
        rec = dict(hand=hi_, obj=oi, verts_model=vm, verts_cam=vc, rt=rt)
        for key, v, pose in (('eye', vm, eye), ('pose', vc, rt)):
            qv = VO.model_frame(v, pose)
            if key == 'eye':
                assert np.array_equal(qv, vm.astype(np.float64))
            flags = M.check_mesh_contains(types.SimpleNamespace(vertices=qv, faces=hf), c.astype(np.float64), 512)
            ours = VO.hand_inside(qv, hf, c)
            assert np.array_equal(flags, ours), (key, int((flags != ours).sum()))
            rec['flags_' + key] = flags
            rec['band_' + key] = VO.edge_band(qv, hf, c)
            rec['cells_' + key] = int((flags & solid).sum())
            rec['qv_' + key] = qv
        pairs.append(rec)
    cells = [p['cells_pose'] for p in pairs]
    band = sum(int(p['band_eye'].sum()) + int(p['band_pose'].sum()) for p in pairs)
    total = sum(2 * len(p['band_eye']) for p in pairs)
    ok = len(set(cells)) == len(cells) and len(set(p['cells_eye'] for p in pairs)) == len(pairs) and band <= 0.001 * total
    ok = ok and cells[3] == 0 and pairs[3]['cells_eye'] == 0 and min(cells[:3]) > 0
    # pair 2: the hand's bbox lies inside the object's
    olo, ohi = objects[0][1].min(0), objects[0][1].max(0)
    q = pairs[2]['qv_pose']
    ok = ok and bool((q.min(0) > olo).all() and (q.max(0) < ohi).all())
    return ok, hands, objects, lattices, pairs


def main():
    M = MP._reference_intersector()
    seed = 20261018
    while True:
        ok, hands, objects, lattices, pairs = _attempt(seed, M)
        if ok:
            break
        print(f'seed {seed}: rejected (cells {[p["cells_pose"] for p in pairs]})')
        seed += 1
    out = dict(seed=np.array(seed), pitch=np.array(PITCH), hand_names=np.array([h[0] for h in hands]), obj_names=np.array([o[0] for o in objects]),
               pair_hand=np.array([p['hand'] for p in pairs]), pair_obj=np.array([p['obj'] for p in pairs]),
               rt=np.stack([p['rt'] for p in pairs]), cells_eye=np.array([p['cells_eye'] for p in pairs]),
               cells_pose=np.array([p['cells_pose'] for p in pairs]))
    for i, (_, hv, hf) in enumerate(hands):
        out[f'hand{i}_faces'] = hf.astype(np.int32)
    for i, (_, ov, of) in enumerate(objects):
        c, dims, solid = lattices[i]
        out[f'obj{i}_verts'], out[f'obj{i}_faces'] = ov, of.astype(np.int32)
        out[f'obj{i}_centres'], out[f'obj{i}_dims'], out[f'obj{i}_solid'] = c, dims, solid
    for i, p in enumerate(pairs):
        for k in ('verts_model', 'verts_cam', 'flags_eye', 'flags_pose', 'band_eye', 'band_pose'):
            out[f'pair{i}_{k}'] = p[k]
        print(f'pair {i}: hand {hands[p["hand"]][0]} ({len(hands[p["hand"]][2])} faces) / {objects[p["obj"]][0]} {tuple(lattices[p["obj"]][1])}: '
              f'n_cells {p["cells_pose"]} (identity pose {p["cells_eye"]}), band {int(p["band_pose"].sum())}')
    np.savez_compressed(os.path.join(HERE, 'golden_volume.npz'), **out)


if __name__ == '__main__':
    main()

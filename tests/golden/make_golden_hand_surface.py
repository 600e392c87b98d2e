"""Fixtures of the hand surface and the contact-label chain (csrc/hand_surface.hip, vpho_amd/physics_labels.py):
``golden_hand_surface.npz``, data only.

Everything comes from the reference's OWN functions, imported unchanged under the stubs of make_golden.py:

* the gap table: ``lib.utils.hand_fn.fill_finger_gaps_in_mano`` (numpy branch) is run on the one-hot input ``eye(778)``; every filled
  row then shows its two source vertices and their weights.  ``links`` (302, 2) and ``alpha`` (302,) are read off those rows -- the
  function's literal table is never copied.  Which of a row's two vertices is ``links[:, 0]`` matters only where
  ``1 - (1 - alpha) != alpha`` (the thirds); there it is decided exactly (``fl(1 - alpha)`` must be the other weight), elsewhere by the
  rule that a link's weight on its first vertex grows over the rows that repeat it (both orders give the same bits there);
* ``fill_finger_gaps_in_mano`` on 3 random vertex / normal sets (float32 inputs, float64 outputs);
* ``lib.utils.physics_fn.detect_hand_and_object_contact`` (sklearn ball tree), ``np.clip``, ``VERT2ANCHOR.get_force_contact`` and
  ``check_is_grasped`` -- the calls of lib/dataset/dexycb6.py:320-332 with the gates of base.py:898-905 -- on 3 cases of (the filled test
  mesh of tests/_hand_surface_fp64.py, a 2 048-point cloud at a grazing placement).  The anchors are the synthetic CPF table written in
  the reference's on-disk format.  trimesh is not installed: the normals of the test mesh come from the restatement, the reference sees
  them as float32 inputs like the kernel's consumers do.

The generator asserts that at most 1 % of the hand vertices of a case lie in the band the GPU test leaves out.
Run in the build container only (needs /root/reference)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import _hand_surface_fp64 as HS  # noqa: E402

N_CASES = 3


def recover_gap_table(fill_fn):
    rows = fill_fn(np.eye(778), None)[778:]
    pairs, by_pair = [], {}
    for r, row in enumerate(rows):
        nz = np.flatnonzero(row)
        assert len(nz) == 2, (r, nz)
        pairs.append((int(nz[0]), int(nz[1])))
        by_pair.setdefault(pairs[-1], []).append(r)
    links, alpha = np.zeros((len(rows), 2), np.int64), np.zeros(len(rows))
    for (a, b), rr in by_pair.items():
        wa = np.array([rows[r, a] for r in rr])
        first = a if (np.diff(wa) >= 0).all() else b
        assert first == a or (np.diff(wa) <= 0).all(), (a, b, wa)
        for r in rr:
            i0, i1 = (first, b if first == a else a)
            if 1.0 - rows[r, i0] != rows[r, i1]:                      # the exact rule decides
                i0, i1 = i1, i0
            assert 1.0 - rows[r, i0] == rows[r, i1], (r, rows[r, i0], rows[r, i1])
            links[r], alpha[r] = (i0, i1), rows[r, i0]
    return links, alpha


def main():
    from vpho_amd.assets import synthetic_assets
    assets = synthetic_assets(0)
    tmp = tempfile.mkdtemp(prefix='vpho_golden_hs_')
    MG.write_assets(tmp, assets)
    os.chdir(tmp)
    sys.argv = ['main.py']
    sys.path.insert(0, MG.REF)
    MG.install_stubs(assets)
    from lib.utils.hand_fn import fill_finger_gaps_in_mano
    from lib.utils.physics_fn import detect_hand_and_object_contact, VERT2ANCHOR

    links, alpha = recover_gap_table(fill_finger_gaps_in_mano)
    assert links.shape == (302, 2) and 778 + len(links) == 1080
    P = dict(links=links.astype(np.int32), alpha=alpha)
    r = np.random.default_rng(11)
    for k in range(N_CASES):
        v = r.normal(0, 0.05, (778, 3)).astype(np.float32)
        n = r.normal(0, 1, (778, 3)).astype(np.float32)
        vf, nf = fill_finger_gaps_in_mano(v.astype(np.float64), n.astype(np.float64))
        assert np.array_equal(vf, HS.fill(v, links, alpha)) and np.array_equal(nf, HS.fill(n, links, alpha))      # the recovered table IS the function
        P[f'fill{k}_verts'], P[f'fill{k}_norms'], P[f'fill{k}_verts_filled'], P[f'fill{k}_norms_filled'] = v, n, vf, nf

    base, faces = HS.ellipsoid()
    gates = HS.CALL_GATES
    P['faces'] = faces.astype(np.int32)
    for k in range(N_CASES):
        v = HS.posed(base, 100 + k)
        vf64, nf64, _, _ = HS.hand_surface(v[None], faces, links, alpha)
        vf, nf = vf64[0].astype(np.float32), nf64[0].astype(np.float32)
        cloud = HS.grazing_cloud(vf, nf, 200 + k)
        hc, _, _ = detect_hand_and_object_contact(vf.astype(np.float64), nf.astype(np.float64), cloud.astype(np.float64), np.zeros((2048, 3)),
                                                  normal_distance_thresh=gates['normal_thresh'], vertical_distance_thresh=gates['vertical_thresh'])
        hc = np.clip(hc, 0, 1)
        fc = VERT2ANCHOR.get_force_contact(hc)
        grasped = bool(VERT2ANCHOR.check_is_grasped(fc))
        chain = HS.hand_contact(vf, nf, cloud, **gates)
        share = float(HS.band(chain, gates['normal_thresh'], gates['vertical_thresh']).mean())
        print(f'case {k}: {int((hc > 0).sum())} of {len(hc)} hand vertices in contact, band share {share:.4f}, grasped {grasped}')
        assert share <= 0.01 and (hc > 0).sum() >= 30
        P[f'case{k}_verts'], P[f'case{k}_verts_filled'], P[f'case{k}_normals_filled'], P[f'case{k}_cloud'] = v, vf, nf, cloud
        P[f'case{k}_hand_contact'], P[f'case{k}_force_contact'], P[f'case{k}_is_grasped'] = hc, fc, np.array(grasped)
    P['face_vert_idx'] = np.asarray(assets['anchor']['face_vert_idx'], np.int32)
    P['anchor_weight'] = np.loadtxt(os.path.join(tmp, 'asset/2021_CVPR_CPF/anchor/anchor_weight.txt'))    # as the reference read it back
    path = os.path.join(HERE, 'golden_hand_surface.npz')
    np.savez_compressed(path, **P)
    print({k: v.shape for k, v in P.items()}, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()

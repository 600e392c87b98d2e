"""The hand surface and the contact-label chain without a GPU: the restatements of tests/_hand_surface_fp64.py against the reference's own
functions (tests/golden/golden_hand_surface.npz, written by make_golden_hand_surface.py) and against meshes whose normals are known in
closed form, the gap table, the flip to the right-hand frame, the label file beside a frame directory, the flags, the header and the
compiler's report of csrc/hand_surface.hip.

trimesh is not installed here: the normal rule is a restatement of its angle-weighted vertex normals and is held to geometry (cube,
octahedron, tetrahedron), not to trimesh."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hand_surface_fp64 as HS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_hand_surface.npz')))


# ------------------------------------------------------------------------------------------------------------------ fill and table
def test_fill_restatement_equals_the_reference(gold):
    for k in range(3):
        for what in ('verts', 'norms'):
            got = HS.fill(gold[f'fill{k}_{what}'], gold['links'], gold['alpha'])
            assert got.shape == (1080, 3) and np.abs(got - gold[f'fill{k}_{what}_filled']).max() <= 1e-15


def test_gap_table_shape_and_alpha_sequence(gold):
    from vpho_amd import physics_labels as PL
    links, alpha = gold['links'], gold['alpha']
    assert links.shape == (302, 2) and alpha.shape == (302,) and alpha.dtype == np.float64 and 778 + len(links) == 1080
    assert links.min() >= 0 and links.max() < 778 and (links[:, 0] != links[:, 1]).all()
    assert np.array_equal(alpha, PL.gap_alpha())                                  # 1/4 2/4 3/4 | 1/3 2/3 | 1/2, block by block
    counts = {a: int((alpha == a).sum()) for a in (1 / 4, 2 / 4, 3 / 4, 1 / 3, 2 / 3)}
    assert counts == {1 / 4: 51, 2 / 4: 51 + 45, 3 / 4: 51, 1 / 3: 52, 2 / 3: 52}
    row = 0
    for kind, count in PL.GAP_SEGMENTS:                                           # a link keeps its pair over the blocks that repeat it
        nf = PL.GAP_FILL[kind]
        for i in range(1, nf):
            assert np.array_equal(links[row:row + count], links[row + i * count:row + (i + 1) * count])
        row += nf * count
    assert row == 302


def test_gap_table_falls_back_to_synthetic_and_says_so(tmp_path, capsys, gold):
    from vpho_amd import physics_labels as PL
    from vpho_amd.assets import synthetic_assets
    v = synthetic_assets(0)['mano']['v_template']
    t = PL.gap_table(str(tmp_path), v)
    err = capsys.readouterr().err
    assert t['source'] == 'synthetic' and 'SYNTHETIC' in err and 'finger_gap_links.npz' in err
    PL.gap_table(str(tmp_path), v)
    assert capsys.readouterr().err == ''                                          # once
    assert t['links'].shape == (302, 2) and t['links'].dtype == np.int32 and np.array_equal(t['alpha'], gold['alpha'])
    d = np.linalg.norm(v[t['links'][:, 0]].astype(np.float64) - v[t['links'][:, 1]], axis=-1)
    assert (d < 0.02).all() and (t['links'][:, 0] != t['links'][:, 1]).all()
    assert np.array_equal(PL.gap_table(str(tmp_path), v)['links'], t['links'])    # seeded
    # the installed file wins, and a damaged one is an error
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import install_gap_table
    install_gap_table.main([str(tmp_path)])
    real = PL.gap_table(str(tmp_path), v)
    assert real['source'].endswith('finger_gap_links.npz') and np.array_equal(real['links'], gold['links']) and np.array_equal(real['alpha'], gold['alpha'])
    np.savez(str(tmp_path / 'ours' / 'finger_gap_links.npz'), links=gold['links'][:, :1], alpha=gold['alpha'])
    with pytest.raises(ValueError, match='expected'):
        PL.gap_table(str(tmp_path), v)


def test_padded_object_table_repeats_the_last_vertex():
    from vpho_amd import physics_labels as PL
    ycb = {'a': dict(verts=np.arange(12.0).reshape(4, 3)), 'b': dict(verts=np.arange(6.0).reshape(2, 3) + 100)}
    t = PL.padded_object_table(ycb, ('a', 'b'))
    assert t.shape == (2, 4, 3) and t.dtype == np.float64 and np.array_equal(t[0], ycb['a']['verts'])
    assert np.array_equal(t[1, :2], ycb['b']['verts']) and np.array_equal(t[1, 2], t[1, 1]) and np.array_equal(t[1, 3], t[1, 1])


# ------------------------------------------------------------------------------------------------------------------ normals
@pytest.mark.parametrize('seed', range(6))
def test_cube_corner_normals_are_the_diagonals(seed):
    """angle weights make a corner's normal independent of how its three squares are cut: one square gives pi/2 in all (one triangle
    with the right angle, or two with pi/4 each).  Area weights or uniform weights fail this."""
    v, f = HS.cube(seed)
    n, length, angles = HS.vertex_normals(v[None], f)
    assert np.abs(n[0] - v / np.sqrt(3)).max() <= 1e-15 and np.abs(angles[0] - 1.5 * np.pi).max() < 1e-14
    tri = v[f]
    area = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])               # area-weighted and uniform sums are NOT diagonal here
    by_area, uniform = np.zeros((8, 3)), np.zeros((8, 3))
    for k, t in enumerate(f):
        by_area[t] += area[k]
        uniform[t] += area[k] / np.linalg.norm(area[k])
    off = lambda s: np.abs(s / np.linalg.norm(s, axis=1, keepdims=True) - v / np.sqrt(3)).max()
    valence = np.bincount(f.reshape(-1), minlength=8)
    assert seed != 0 or ((valence == 4) | (valence == 5)).any()                  # at least this cut has a corner whose squares are cut unevenly
    if ((valence == 4) | (valence == 5)).any():
        assert off(by_area) > 1e-3 and off(uniform) > 1e-3


@pytest.mark.parametrize('mesh', ['octahedron', 'tetrahedron'])
def test_regular_solids_have_radial_normals(mesh):
    v, f = getattr(HS, mesh)()
    for scale, seed in ((1.0, None), (0.03, 3)):
        p = v * scale if seed is None else HS.posed(v, seed, scale).astype(np.float64)
        n, _, _ = HS.vertex_normals(p[None], f)
        c = p.mean(0)
        want = (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True)
        assert np.abs(n[0] - want).max() <= (1e-15 if seed is None else 2e-6)        # a posed mesh is rounded to float32: 6e-8 / 0.03


def test_degenerate_unreferenced_and_nan_vertices():
    v, f = HS.octahedron()
    v = np.concatenate([v, [[5.0, 5.0, 5.0]]])                                     # vertex 6: unreferenced
    f2 = np.concatenate([f, [[0, 0, 2]], [[0, 2, 4]], [[0, 4, 2]]])                # a repeated index, and a coincident opposite pair
    n, length, angles = HS.vertex_normals(v[None], f2)
    base, _, _ = HS.vertex_normals(v[None], np.concatenate([f, [[0, 2, 4]], [[0, 4, 2]]]))
    assert np.array_equal(n, base) and np.array_equal(n[0, 6], [0, 0, 0]) and np.isfinite(n).all()
    two = np.array([[0, 2, 4], [0, 4, 2]])                                          # only the cancelling pair: every sum is zero
    n0, l0, a0 = HS.vertex_normals(v[None], two)
    assert np.array_equal(n0, np.zeros_like(n0)) and (a0[0, [0, 2, 4]] > 0).all()
    assert not HS.comparable_rows(l0, a0, np.zeros((0, 2)), 7).any()
    bad = v.copy()
    bad[4, 1] = np.nan                                                             # the apex of four faces
    nn, _, _ = HS.vertex_normals(bad[None], f)
    assert np.isnan(nn[0, [0, 1, 2, 3, 4]]).all() and np.isfinite(nn[0, 5]).all() and np.array_equal(nn[0, 6], [0, 0, 0])
    vf, nf, _, _ = HS.hand_surface(bad[None], f, [[5, 6], [4, 5], [5, 5]], [0.25, 0.5, 1 / 3])
    assert np.isfinite(vf[0, 7]).all() and np.isnan(vf[0, 8, 1]) and np.isfinite(nf[0, 7]).all() and np.isnan(nf[0, 8]).all()
    assert np.array_equal(vf[0, 9], bad[5]) and np.abs(nf[0, 9] - nn[0, 5]).max() < 1e-15       # a link with i0 == i1


def test_test_mesh_is_the_closed_ellipsoid_of_the_issue():
    v, f = HS.ellipsoid()
    assert v.shape == (778, 3) and f.shape == (1552, 3)
    val = np.bincount(f.reshape(-1), minlength=778)
    assert val[0] == 97 and val[777] == 97 and (val[1:777] >= 5).all()
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, cnt = np.unique(edges, axis=0, return_counts=True)
    assert (cnt == 2).all()                                                        # closed: every edge has two faces
    n, length, angles = HS.vertex_normals(v[None], f)
    assert ((n[0] * v).sum(-1) > 0).all() and (length[0] >= 0.5 * angles[0]).all()  # outward, and far from cancelling
    assert np.ptp(v, 0).tolist() == pytest.approx([0.18, 0.08, 0.03], rel=0.3)


# ------------------------------------------------------------------------------------------------------------------ chain
def test_chain_restatement_equals_the_reference_outside_the_band(gold):
    g = HS.CALL_GATES
    for k in range(3):
        v, faces = gold[f'case{k}_verts'], gold['faces']
        vf, nf, _, _ = HS.hand_surface(v[None], faces, gold['links'], gold['alpha'])
        assert np.array_equal(vf[0].astype(np.float32), gold[f'case{k}_verts_filled']) and np.array_equal(nf[0].astype(np.float32), gold[f'case{k}_normals_filled'])
        chain = HS.hand_contact(gold[f'case{k}_verts_filled'], gold[f'case{k}_normals_filled'], gold[f'case{k}_cloud'], **g)
        out = HS.band(chain, g['normal_thresh'], g['vertical_thresh'])
        print(f'case {k}: band {int(out.sum())} of {len(out)}, in contact {int(chain["mask"].sum())}')
        assert out.mean() <= 0.01
        ref = gold[f'case{k}_hand_contact']
        assert np.array_equal((ref > 0)[~out], chain['mask'][~out])
        assert np.abs(np.clip(chain['weight'], 0, 1) - ref)[~out].max() <= 1e-12
        if not out.any():
            fc = HS.force_contact(np.clip(chain['weight'], 0, 1), gold['face_vert_idx'], gold['anchor_weight'])
            assert np.abs(fc - gold[f'case{k}_force_contact']).max() <= 1e-12
            assert bool(HS.is_grasped(fc)) == bool(gold[f'case{k}_is_grasped'])


def test_flip_to_the_right_hand_frame_changes_no_value(gold):
    """a left hand: mirrored vertices, faces wound the other way.  Negating x (exact) and taking the right hand's faces gives the
    identical normal distances, vertical distances and weights, bit for bit"""
    mirror = np.array([-1.0, 1.0, 1.0])
    v, faces, cloud = gold['case1_verts'].astype(np.float64), gold['faces'], gold['case1_cloud'].astype(np.float64)
    left_v, left_f, left_cloud = v * mirror, faces[:, [0, 2, 1]], cloud * mirror
    vf_r, nf_r, _, _ = HS.hand_surface(v[None], faces, gold['links'], gold['alpha'])
    vf_l, nf_l, _, _ = HS.hand_surface(left_v[None], left_f, gold['links'], gold['alpha'])
    assert np.array_equal(vf_l * mirror, vf_r) and np.array_equal(nf_l * mirror, nf_r)
    a = HS.hand_contact(vf_r[0], nf_r[0], cloud, **HS.CALL_GATES)
    b = HS.hand_contact(vf_l[0], nf_l[0], left_cloud, **HS.CALL_GATES)
    for k in ('nd', 'vd', 'weight', 'index', 'mask'):
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------ label file
def test_label_file_beside_a_frame_directory(tmp_path):
    from vpho_amd import frames as FR
    from vpho_amd.assets import synthetic_assets
    src = FR.synthetic_frames(3, synthetic_assets(0), seed=2, size=(48, 40))
    d = str(tmp_path / 'd')
    FR.write_frame_directory(d, src)
    plain = FR.FrameDirectory(d)
    assert plain.labels is None and 'force_contact' not in plain[0][1]
    assert bool(plain[1][1]['is_grasped']) == bool(src[1][1]['is_grasped'])
    r = np.random.default_rng(0)
    lab = dict(index=np.arange(3), hand_contact=r.random((3, 1080)).astype(np.float32), force_contact=r.random((3, 32)).astype(np.float32),
               is_grasped=np.array([True, False, True]), force_local=r.normal(size=(3, 32, 3)).astype(np.float32),
               force_global=r.normal(size=(3, 32, 3)).astype(np.float32), meta=np.array('{}'))
    np.savez(os.path.join(d, FR.LABEL_FILE), **lab)
    back = FR.FrameDirectory(d)
    for i in range(3):
        f, rec = back[i]
        assert np.array_equal(f, src[i][0]) and bool(rec['is_grasped']) == bool(lab['is_grasped'][i])
        assert np.array_equal(rec['force_local'], lab['force_local'][i]) and np.array_equal(rec['force_contact'], lab['force_contact'][i])
        for k in FR.RECORD_KEYS + ('hand_vert', 'gravity'):
            assert np.array_equal(np.asarray(rec[k]), np.asarray(src[i][1][k])), k
    np.savez(os.path.join(d, FR.LABEL_FILE), **{k: (v[:2] if v.ndim else v) for k, v in lab.items()})
    with pytest.raises(ValueError, match='physics_labels.npz has 2 rows'):
        FR.FrameDirectory(d)
    assert FR.RECORD_KEYS == ('jt2d', 'joint_3d', 'mano_pose', 'mano_betas', 'is_right', 'obj_id', 'obj_rt', 'cam_intr')
    assert FR.OPTIONAL_KEYS == ('hand_vert', 'gravity', 'force_local', 'is_grasped')


# ------------------------------------------------------------------------------------------------------------------ flags, header, report
def test_flags_and_defaults():
    from vpho_amd.configs import args as A
    p = A._parser()
    d, c = p.parse_args([]), A.Config()
    want = dict(contact_normal_distance_thresh=(-0.01, 0.01), contact_vertical_distance_thresh=0.005, frame_contact=False)
    for k, v in want.items():
        assert getattr(d, k) == v and getattr(c, k) == v, k
    a = p.parse_args(['--frame_contact', '--contact_normal_distance_thresh', '-0.015', '0.01', '--contact_vertical_distance_thresh', '0.01'])
    assert a.frame_contact is True and list(a.contact_normal_distance_thresh) == [-0.015, 0.01] and a.contact_vertical_distance_thresh == 0.01
    assert HS.CALL_GATES['normal_thresh'] == want['contact_normal_distance_thresh'] and HS.CALL_GATES['vertical_thresh'] == 0.005


def test_force_optim_takes_a_frame_source():
    src = open(os.path.join(ROOT, 'force_optim.py')).read()
    for flag in ('--frame_source', '--num_frames', '--out'):
        assert f"'{flag}'" in src
    body = src[src.index('def main'):]
    assert body.index('maybe_spawn(args.gpus)') < body.index('label_frames(args)') < body.index('import torch')


def test_header_declares_the_entry_point_at_abi_13():
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert re.search(r'VPHO_API int vpho_hand_surface_f32\(const vpho_hand_surface_table\* t, const float\* verts, int n, float\* verts_filled, '
                     r'float\* normals_filled,\s*void\* stream\);', hdr)
    assert re.search(r'const int\* faces; const int\* csr_offset; const int\* csr_entry; const int\* links; const double\* alpha;\s*int V, F, L;\s*'
                     r'\} vpho_hand_surface_table;', hdr)
    assert 'base.py:887-891' in hdr and 'hand_fn.py:294-384' in hdr
    src = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'hand_surface.hip')).read()
    assert 'base.py:887-891' in src and 'hand_fn.py:294-384' in src and 'atomic' not in src.replace('no atomics', '')
    from vpho_amd import ops
    assert [f[0] for f in ops.HandSurfaceTable._fields_] == ['faces', 'csr_offset', 'csr_entry', 'links', 'alpha', 'V', 'F', 'L']
    assert hasattr(ops.lib, 'vpho_hand_surface_f32')


def test_hand_surface_kernel_reports_no_spill_and_no_scratch():
    from vpho_amd.build import build_extension
    build_extension()
    seen, name = {}, None
    for line in open(os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'hand_surface.hip.usage.txt')):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (('vgpr', r' VGPRs: (\d+)'), ('spill', r'VGPRs Spill: (\d+)'), ('sspill', r'SGPRs Spill: (\d+)'),
                         ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('lds', r'LDS Size \[bytes/block\]: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    assert len(seen) == 1 and 'hand_surface_kernel' in next(iter(seen)), sorted(seen)
    k = next(iter(seen.values()))
    assert k['spill'] == 0 and k['sspill'] == 0 and k['scratch'] == 0 and k['lds'] == 0 and k['vgpr'] <= 128, k      # the LDS is all dynamic


def test_documents_name_the_feature():
    for doc, words in (('DESIGN.md', ('8f-3m', 'hand_surface')), ('INTEGRATION.md', ('--frame_contact', 'restated', 'physics_labels.npz')),
                       ('README.md', ('--frame_contact', '--contact_normal_distance_thresh'))):
        txt = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in txt, (doc, w)

"""CPU checks of the penetration metric (--eval_physics): the float64 oracle against closed forms and the reference fixture, the
synthetic box meshes, the host tables, the wider metric rows and the physics table, and the ctypes mirror of the new struct."""
import os

import numpy as np
import pytest
import torch

import tests._penetration_fp64 as O

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_penetration.npz'))


def _mesh(i):
    v = G['verts'][G['vert_offset'][i]:G['vert_offset'][i + 1]]
    f = G['faces'][G['face_offset'][i]:G['face_offset'][i + 1]].astype(np.int64)
    p = G['points'][G['point_offset'][i]:G['point_offset'][i + 1]]
    sl = slice(G['point_offset'][i], G['point_offset'][i + 1])
    return v, f, p, G['contains_ref'][sl], G['d_ours'][sl]


def test_oracle_box_signed_distance_equals_closed_form():
    from vpho_amd.physics_eval import box_mesh
    lo, hi = np.array([-0.03, -0.05, -0.02]), np.array([0.04, 0.05, 0.07])
    v, f = box_mesh(np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]))
    rng = np.random.default_rng(3)
    p = rng.uniform(lo - 0.03, hi + 0.03, size=(3000, 3))
    ins = O.contains(v, f, p)
    d = O.distance(v, f, p)
    sd = np.where(ins, -d, d)
    ref = O.box_sd(lo, hi, p)
    np.testing.assert_allclose(sd, ref, atol=1e-12)
    assert 200 < ins.sum() < 2800


def test_synthetic_box_mesh_is_closed_and_oriented_outwards(assets):
    from vpho_amd.physics_eval import box_mesh, object_meshes
    meshes = object_meshes(assets)
    assert list(meshes) == list(assets['ycb'])
    for name, m in meshes.items():
        v, f = m['verts'], m['faces']
        assert f.shape == (3072, 3) and v.shape == (6 * 16 * 16 + 2, 3)
        edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        _, count = np.unique(edges, axis=0, return_counts=True)
        assert (count == 2).all()                                   # every edge shared by exactly two faces
        assert len(v) - len(count) + len(f) == 2                    # Euler characteristic of a sphere
        directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert len(np.unique(directed, axis=0)) == len(directed)    # consistently wound: no directed edge twice
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        n = np.cross(b - a, c - a)
        centre = (a + b + c) / 3 - v.mean(0)
        assert ((n * centre).sum(1) > 0).all()                      # outward
        vol = np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6
        bb = np.asarray(assets['ycb'][name]['bbox3d'], np.float64)
        np.testing.assert_allclose(vol, np.prod(bb.max(0) - bb.min(0)), rtol=1e-9)
        np.testing.assert_array_equal(v.min(0), bb.min(0))
        np.testing.assert_array_equal(v.max(0), bb.max(0))
    v2, f2 = box_mesh(assets['ycb'][name]['bbox3d'])
    assert np.array_equal(v2, v) and np.array_equal(f2, f)          # no random numbers


def test_object_meshes_real_table_needs_faces(tmp_path, assets):
    import pickle
    from vpho_amd.assets import AssetError
    from vpho_amd.physics_eval import object_meshes
    path = tmp_path / 'object_mesh_info.pkl'
    v, f = np.eye(3), np.array([[0, 1, 2]])
    with open(path, 'wb') as fh:
        pickle.dump({n: dict(verts=v) for n in assets['ycb']}, fh)
    real = dict(assets, sources={'ycb': str(path)})
    with pytest.raises(AssetError, match="'faces'"):
        object_meshes(real)
    with open(path, 'wb') as fh:
        pickle.dump({n: dict(verts=v, faces=f) for n in assets['ycb']}, fh)
    m = object_meshes(real)
    assert list(m) == list(assets['ycb']) and np.array_equal(m[next(iter(m))]['faces'], f)


@pytest.mark.parametrize('i', range(5))
def test_oracle_parity_equals_reference_fixture(i):
    v, f, p, ref, d = _mesh(i)
    assert np.array_equal(O.contains(v, f, p), ref), str(G['names'][i])


def test_fixture_covers_inside_outside_and_open_meshes():
    names = [str(n) for n in G['names']]
    assert names[2:] == ['torus', 'open_box', 'cup'] and len(G['points']) >= 20000
    for i in range(3):
        _, _, _, ref, _ = _mesh(i)
        assert 0.2 < ref.mean() < 0.8


def test_host_tables_match_the_oracle_terms():
    """physics_eval.mesh_tables: the reference's scale / translate and the record layout of include/vpho_hip.h"""
    from vpho_amd.physics_eval import mesh_tables, TRI_STRIDE
    v, f, _, _, _ = _mesh(2)
    tri, scale, translate = mesh_tables(v, f)
    assert tri.shape == (len(f), TRI_STRIDE)
    t = v[f]
    lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
    assert np.array_equal(scale, 511 / (hi - lo)) and np.array_equal(translate, 0.5 - scale * lo)
    np.testing.assert_array_equal(tri[:, 19:22], t[:, 0])
    np.testing.assert_array_equal(tri[:, 22:25], t[:, 1] - t[:, 0])
    assert (tri[:, 15] <= tri[:, 16]).all() and (tri[:, 17] <= tri[:, 18]).all() and tri[:, 15:19].min() >= 0 and tri[:, 15:19].max() <= 511


def test_row_width_with_eval_physics():
    from vpho_amd import evaluate as E
    from vpho_amd.ops_names import PHYSICS_COLUMNS
    width = lambda **flags: E.RowLayout.resolve(**flags).width
    assert width() == 28 and width(eval_best=True) == 88
    assert width(eval_physics=True) == 36
    assert width(eval_best=True, eval_physics=True) == 96
    assert len(PHYSICS_COLUMNS) == E.PHYS == 8


def test_summarize_builds_the_physics_table():
    from vpho_amd import evaluate as E
    from vpho_amd.ops_names import PHYSICS_TABLE
    for best in (False, True):
        rows = torch.zeros((4, E.RowLayout.resolve(eval_best=best, eval_physics=True).width))
        rows[:, 7] = torch.tensor([1.0, 0.0, 1.0, 0.0])
        rows[:, -8:] = torch.tensor([[0.004, 12, -0.004, 1, 0.0, 0, 0.002, 1],
                                     [0.0, 0, 0.010, 0, 0.0, 0, 0.006, 0],
                                     [0.002, 3, -0.002, 1, 0.001, 1, -0.001, 1],
                                     [0.0, 0, 0.001, 1, 0.0, 0, 0.020, 0]])
        t = E.summarize(rows)
        assert set(t['physics']) == {'pred', 'gt'} and tuple(t['physics']['pred']) == PHYSICS_TABLE
        p, g = t['physics']['pred'], t['physics']['gt']
        assert p['PD_mm'] == pytest.approx(1.5, rel=1e-6) and p['PD_max_mm'] == pytest.approx(4.0, rel=1e-6)
        assert p['penetration_rate_pct'] == 50.0 and p['inside_verts'] == 3.75 and p['contact_rate_pct'] == 75.0
        assert g['PD_mm'] == pytest.approx(0.25, rel=1e-6) and g['penetration_rate_pct'] == 25.0 and g['contact_rate_pct'] == 50.0
        assert ('best_of_S' in t) == best
    # without the flag: no physics table; gt without object ground truth: NaN
    assert 'physics' not in E.summarize(torch.zeros((2, E.ROW))) and 'physics' not in E.summarize(torch.zeros((2, E.ROW_BEST)))
    rows = torch.zeros((2, E.RowLayout.resolve(eval_best=False, eval_physics=True).width))
    rows[:, -4:] = float('nan')
    g = E.summarize(rows)['physics']['gt']
    assert all(np.isnan(v) for v in g.values())


def test_ctypes_obj_mesh_tables_mirror_the_header():
    import ctypes
    from tests.test_abi import _header_structs
    from vpho_amd import ops
    hs = _header_structs()
    kind = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_double: 'double', ctypes.c_longlong: 'longlong'}
    assert [(f[0], kind[f[1]]) for f in ops.ObjMeshTables._fields_] == hs['vpho_obj_mesh_tables']
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vpho_hip.h')).read()
    from vpho_amd.physics_eval import RESOLUTION, TRI_STRIDE
    assert f'#define VPHO_PEN_TRI_STRIDE {TRI_STRIDE}' in src and f'#define VPHO_PEN_RESOLUTION {RESOLUTION}' in src


def test_config_flags():
    from vpho_amd.configs.args import Config, _parser
    c = Config()
    assert c.eval_physics is False and c.physics_contact_thresh == 0.005
    a = _parser().parse_args(['--eval_physics', '--physics_contact_thresh', '0.01'])
    assert a.eval_physics and a.physics_contact_thresh == 0.01

"""The multi-hypothesis penetration kernel's host-side acceleration tables (physics_eval.mesh_accel), with no kernel involved: for every
test point of tests/_penetration_multi_inputs.py the parity walk's candidates contain every triangle that passes the hash-cell test,
and the nearest-triangle walk visits the brute-force nearest triangle -- plus the tables' layout, the new names and the header."""
import os
import re

import numpy as np
import pytest
import torch

import tests._penetration_fp64 as O
import tests._penetration_multi_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _points_of(mesh_index):
    """all model-frame test points of a mesh over the three launches (the hand-placed set is among them, in hypothesis 0)"""
    out = [I.case(w)['p'][i].reshape(-1, 3) for w in range(len(I.ID_CASES)) for i, o in enumerate(I.ID_CASES[w]) if o == mesh_index]
    return np.concatenate(out)


def test_inputs_hold_inside_and_outside_points_and_an_exact_hash_frame():
    from vpho_amd.physics_eval import mesh_tables
    share = I.inside_share()
    for name, s in share.items():
        assert 0.10 <= s <= 0.90, (name, s)
    for name, m in I.meshes().items():
        _, scale, translate = mesh_tables(m['verts'], m['faces'])
        assert np.array_equal(scale, I.SCALE) and np.array_equal(translate, I.TRANSLATE), name
    # the hand-placed set really sits where it is meant to: far faces, cell and column boundaries
    q = I.SCALE * I.hand_placed(I.meshes()['box']) + I.TRANSLATE
    assert (q == 512.0).any(0).all() and (q[:, :2] == 0.0).any()
    assert ((q[:, 0] % 8 == 0) & (q[:, 0] > 0) & (q[:, 0] < 512)).sum() >= 6 and ((q[:, 1] % 1 == 0) & (q[:, 1] % 8 != 0)).sum() >= 3
    assert (np.abs(q) > 2000).any(1).sum() >= 4


@pytest.mark.parametrize('mesh_index', range(3))
def test_parity_candidates_contain_every_triangle_of_the_cell_test(mesh_index):
    from vpho_amd.physics_eval import RESOLUTION, mesh_accel, mesh_tables, parity_candidates
    m = I.meshes()[I.MESH_NAMES[mesh_index]]
    tri, scale, translate = mesh_tables(m['verts'], m['faces'])
    acc = mesh_accel(tri)
    pts = _points_of(mesh_index)
    cand = parity_candidates(acc, scale, translate, pts)
    # the brute-force kernel's filter, written out: the point's own cell within the triangle's cell rectangle
    q = scale * pts + translate
    box = np.all((0 <= q) & (q <= RESOLUTION), axis=1)
    cx, cy = np.where(box, np.trunc(q[:, 0]), -1.0), np.where(box, np.trunc(q[:, 1]), -1.0)
    has_cell = box & (cx < RESOLUTION) & (cy < RESOLUTION)
    passes = has_cell[:, None] & (tri[None, :, 15] <= cx[:, None]) & (cx[:, None] <= tri[None, :, 16]) & \
        (tri[None, :, 17] <= cy[:, None]) & (cy[:, None] <= tri[None, :, 18])
    assert passes.sum() > 200                                    # the condition is not vacuous
    assert not (passes & ~cand).any()
    assert cand.sum(1).max() < len(tri) / 4                      # and the lists are short
    # lists ascend, and hold exactly the triangles whose rectangle touches the column
    off, lst = acc['col_offset'], acc['col_tri']
    assert off[0] == 0 and off[-1] == len(lst) and (np.diff(off) >= 0).all()
    for col in (0, 17 * 64 + 40, 32 * 64 + 32, 64 * 64 - 1):
        got = lst[off[col]:off[col + 1]]
        X, Y = col % 64, col // 64
        want = np.nonzero((tri[:, 15] // 8 <= X) & (X <= tri[:, 16] // 8) & (tri[:, 17] // 8 <= Y) & (Y <= tri[:, 18] // 8))[0]
        assert np.array_equal(got, want)


@pytest.mark.parametrize('mesh_index', range(3))
def test_nearest_walk_visits_the_brute_force_nearest_triangle(mesh_index):
    from vpho_amd.physics_eval import CLUSTER, mesh_accel, mesh_tables, nearest_candidates
    m = I.meshes()[I.MESH_NAMES[mesh_index]]
    tri, _, _ = mesh_tables(m['verts'], m['faces'])
    acc = mesh_accel(tri)
    pts = _points_of(mesh_index)
    visited, best = nearest_candidates(acc, pts)
    t = m['verts'][m['faces']]
    d2 = np.concatenate([O._dist2(pts[s:s + 64, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2]) for s in range(0, len(pts), 64)])
    nearest = d2.argmin(1)
    assert visited[np.arange(len(pts)), nearest].all()
    # every triangle at the minimum distance is either visited or strictly farther than the one that was: best is the brute-force minimum
    np.testing.assert_allclose(np.sqrt(best), np.sqrt(d2.min(1)), rtol=0, atol=1e-15)
    assert visited.mean() < 0.5                                  # the walk prunes
    # layout: a permutation of the triangles, padded with copies of the last one; spheres contain their triangles' corners
    order = acc['order']
    assert len(order) % CLUSTER == 0 and np.array_equal(np.unique(order), np.arange(len(tri)))
    assert (order[len(tri):] == order[len(tri) - 1]).all()
    assert np.array_equal(acc['geo'].reshape(-1, 9), tri[order, 19:28])
    corners = t[order].reshape(len(acc['sphere']), -1, 3)
    assert (np.linalg.norm(corners - acc['sphere'][:, None, :3], axis=-1) < acc['sphere'][:, None, 3]).all()
    assert np.array_equal(mesh_accel(tri)['order'], order)       # deterministic


def test_names_header_and_row_width():
    from vpho_amd import evaluate as E
    from vpho_amd import physics_eval as P
    from vpho_amd.ops_names import MULTI_TABLES, PHYSICS_METRIC_NAMES, PHYSICS_MULTI_COLUMNS
    assert len(PHYSICS_MULTI_COLUMNS) == E.PHYS_MULTI == 12
    assert PHYSICS_MULTI_COLUMNS[0] == 'physics/one_candidate/PD' and PHYSICS_MULTI_COLUMNS[6] == 'physics/best_of_S/min_sd'
    assert PHYSICS_MULTI_COLUMNS == tuple(f'physics/{t}/{k}' for t in MULTI_TABLES for k in PHYSICS_METRIC_NAMES)
    width = lambda **flags: E.RowLayout.resolve(**flags).width
    assert width(eval_best=True, eval_physics=True, physics_multi=True) == 108 and width(eval_best=True, eval_physics=True) == 96
    assert width(eval_best=True, eval_physics=False, physics_multi=True) == 88 and width(eval_best=False, eval_physics=True) == 36 and width() == 28
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert 'vpho_hand_obj_penetration_multi_f64' in hdr
    assert int(re.search(r'#define VPHO_PEN_COLUMNS (\d+)', hdr).group(1)) == P.COLUMNS
    assert int(re.search(r'#define VPHO_PEN_CLUSTER (\d+)', hdr).group(1)) == P.CLUSTER


def test_ctypes_accel_struct_mirrors_the_header():
    import ctypes
    from tests.test_abi import _header_structs
    from vpho_amd import ops
    kind = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_double: 'double', ctypes.c_longlong: 'longlong'}
    assert [(f[0], kind[f[1]]) for f in ops.ObjMeshAccel._fields_] == _header_structs()['vpho_obj_mesh_accel']
    assert hasattr(ops.HandObjectPenetration, 'multi')


def test_summarize_adds_the_three_multi_hypothesis_physics_tables():
    from vpho_amd import evaluate as E
    from vpho_amd.ops_names import PHYSICS_TABLE
    rows = torch.zeros((4, 108))
    rows[:, 7] = torch.tensor([1.0, 0.0, 1.0, 0.0])
    rows[:, 88:96] = torch.tensor([0.004, 12, -0.004, 1, 0.0, 0, 0.002, 1])
    #                              one: PD n sd contact | best                 | mean (contact: a fraction)
    rows[:, 96:] = torch.tensor([[0.004, 10, -0.004, 1, 0.0, 0, 0.001, 1, 0.002, 2.5, -0.001, 0.75],
                                 [0.0, 0, 0.010, 0, 0.0, 0, 0.010, 0, 0.0, 0.0, 0.012, 0.0],
                                 [0.002, 3, -0.002, 1, 0.001, 1, -0.001, 1, 0.003, 4.0, -0.003, 1.0],
                                 [0.0, 0, 0.001, 1, 0.0, 0, 0.002, 1, 0.001, 0.25, 0.000, 0.25]])
    t = E.summarize(rows)['physics']
    assert set(t) == {'pred', 'gt', 'one_candidate', 'best_of_S', 'mean_of_S'}
    for k in t:
        assert tuple(t[k]) == PHYSICS_TABLE
    assert t['pred']['PD_mm'] == pytest.approx(4.0, rel=1e-6) and t['pred']['inside_verts'] == 12.0
    o, b, m = t['one_candidate'], t['best_of_S'], t['mean_of_S']
    assert o['PD_mm'] == pytest.approx(1.5, rel=1e-6) and o['PD_max_mm'] == pytest.approx(4.0, rel=1e-6)
    assert o['penetration_rate_pct'] == 50.0 and o['inside_verts'] == 3.25 and o['contact_rate_pct'] == 75.0
    assert b['PD_mm'] == pytest.approx(0.25, rel=1e-6) and b['penetration_rate_pct'] == 25.0 and b['contact_rate_pct'] == 75.0
    # mean_of_S: an image penetrates when its MEAN inside count is > 0; contact is 100 x the mean fraction
    assert m['penetration_rate_pct'] == 75.0 and m['inside_verts'] == pytest.approx(1.6875) and m['contact_rate_pct'] == 50.0
    assert m['PD_mm'] == pytest.approx(1.5, rel=1e-6)
    # with one flag only: the tables of today
    assert set(E.summarize(torch.zeros((2, 36)))['physics']) == {'pred', 'gt'}
    assert 'physics' not in E.summarize(torch.zeros((2, 88)))


def test_multi_kernels_have_no_spill_and_no_scratch():
    import __graft_entry__ as g
    g.build()
    txt = open(os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'penetration_multi.hip.usage.txt')).read()
    assert 'penetration_multi_kernel' in txt and 'penetration_table_kernel' in txt
    field = lambda name: [int(v) for v in re.findall(name + r'[^:\n]*: (\d+)', txt)]
    assert field('VGPRs Spill') == [0, 0] and field('SGPRs Spill') == [0, 0] and field('ScratchSize') == [0, 0]
    assert max(field(' VGPRs')) <= 96 and max(field('LDS Size')) <= 8192          # 5 waves per SIMD or more; the reduction arrays only

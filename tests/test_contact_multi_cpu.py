"""--eval_grasp without a GPU: the vertex tables of the pruned kernel and a host emulation of its walk, the flag, the row layout, the
header, the table, and the fp64 restatement (tests/_contact_multi_fp64.py) against the project's own fp32 label chain (oracle/contact.py).

The cross-check's band and tolerance are 4 x the largest difference measured between the two formulations on the CPU over the seeded
scenes below (two fp32 roundings of metre-scale coordinates, through a sigmoid of slope <= 400 / m):
    largest |nd_fp32 - nd_fp64| 4.73e-09 m, largest |vd_fp32 - vd_fp64| 4.91e-09 m   ->  band half-width 4 x 4.91e-09 = 1.964e-08 m
    largest weight difference outside the band 1.79e-06                                ->  weight tolerance 4 x 1.79e-06 = 7.16e-06
    the nearest vertex is the same for all 19 440 hand vertices; at most 1 of 1 080 per pair lies within 1e-6 m of a gate."""
import itertools
import os
import re

import numpy as np
import pytest

import tests._contact_multi_fp64 as CF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 4 * 4.91e-09
W_TOL = 4 * 1.79e-06


@pytest.fixture(scope='module')
def GE():
    from vpho_amd import grasp_eval
    return grasp_eval


def _duplicated(seed=5):
    """300 vertices, every position twice, shuffled: exact ties everywhere"""
    v = CF.ellipsoid(150, seed)
    return np.concatenate([v, v])[np.random.default_rng(seed).permutation(300)]


# --------------------------------------------------------------------------------------------------------------------- the vertex tables
@pytest.mark.parametrize('n_verts', CF.SIZES)
def test_accel_tiles_the_object_and_its_spheres_hold_their_vertices(GE, n_verts):
    v = CF.ellipsoid(n_verts, n_verts)
    acc = GE.vertex_accel(v)
    assert sorted(acc['index'].tolist()) == list(range(n_verts))                        # every original index once
    assert np.array_equal(acc['vert'], v[acc['index']])                                 # bit copies
    start = acc['start']
    assert start[0] == 0 and start[-1] == n_verts and len(start) == -(-n_verts // GE.CLUSTER) + 1
    assert (np.diff(start) >= 1).all() and (np.diff(start)[:-1] == GE.CLUSTER).all() and np.diff(start)[-1] == (n_verts - 1) % GE.CLUSTER + 1
    assert acc['sphere'].shape == (len(start) - 1, 4)
    for k in range(len(start) - 1):
        d = np.sqrt(((acc['vert'][start[k]:start[k + 1]] - acc['sphere'][k, :3]) ** 2).sum(-1))
        assert (d <= acc['sphere'][k, 3]).all()
        assert acc['sphere'][k, 3] <= d.max() * (1 + 2.0 ** -29) + 2.0 ** -29 * np.sqrt(((v.max(0) - v.min(0)) ** 2).sum()) + 1e-300   # exact, not loose
    one = GE.vertex_accel(v, cluster=None)
    assert one['start'].tolist() == [0, n_verts] and np.array_equal(one['index'], acc['index'])


def test_accel_tables_concatenate_without_padding(GE):
    objs = CF.objects(0)
    t = GE.vertex_accel_tables(objs)
    assert t['vert'].shape == (sum(CF.SIZES), 3) and t['index'].shape == (sum(CF.SIZES),)
    assert t['clu_offset'].tolist() == np.concatenate([[0], np.cumsum([-(-k // 32) for k in CF.SIZES])]).tolist()
    row0 = np.concatenate([[0], np.cumsum(CF.SIZES)])
    for o, v in enumerate(objs):
        kb, ke = t['clu_offset'][o], t['clu_offset'][o + 1]
        assert t['clu_start'][kb] == row0[o] and t['clu_start'][ke] == row0[o + 1]
        assert np.array_equal(t['vert'][row0[o]:row0[o + 1]], v[t['index'][row0[o]:row0[o + 1]]])
    assert t['clu_start'].dtype == t['clu_offset'].dtype == t['index'].dtype == np.int32
    from vpho_amd.assets import AssetError
    with pytest.raises(AssetError):
        GE.vertex_accel(np.zeros((0, 3)))
    with pytest.raises(AssetError):
        GE.vertex_accel(np.array([[0.0, np.nan, 0.0]]))


def _brute(v, p):
    d = p[:, None, :] - v[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    return d2.argmin(1), d2.min(1)


@pytest.mark.parametrize('n_verts', CF.SIZES + ('duplicated',))
def test_the_pruned_walk_returns_the_brute_force_index(GE, n_verts):
    v = _duplicated() if n_verts == 'duplicated' else CF.ellipsoid(n_verts, n_verts)
    r = np.random.default_rng(11)
    near = v[r.integers(0, len(v), 400)] + r.normal(size=(400, 3)) * 0.004
    far = r.normal(size=(100, 3)) * 0.2
    on = v[r.integers(0, len(v), 50)]                                                   # distance exactly 0
    p = np.concatenate([near, far, on])
    idx, best, visited = GE.nearest_walk(GE.vertex_accel(v), p)
    want_idx, want_d2 = _brute(v, p)
    assert np.array_equal(idx, want_idx) and np.array_equal(best, want_d2)
    if len(v) >= 300:
        assert visited[:400].mean() < 0.5 * len(v)                                      # ... and it does prune
    if n_verts == 'duplicated':
        assert (idx < 300).all() and len(set(map(tuple, v[idx[-50:]]))) <= 50
        twin = np.array([np.flatnonzero((v == v[i]).all(1)).min() for i in idx])
        assert np.array_equal(idx, twin)                                                # of two equal vertices the smaller index


# ------------------------------------------------------------------------------------------------------------- flag, layout, header
def test_flag_and_config_default():
    from vpho_amd.configs import args as A
    p = A._parser()
    assert p.parse_args([]).eval_grasp is False and p.parse_args(['--eval_grasp']).eval_grasp is True
    assert A.Config().eval_grasp is False


def test_layout_with_the_flag():
    from vpho_amd import ops_names as N
    from vpho_amd.eval_layout import BLOCKS, RowLayout
    assert [b[:3] for b in BLOCKS[-2:]] == [('grasp', 'eval_grasp', 8), ('grasp_multi', 'grasp_multi', 24)] and BLOCKS[-1].needs == 'eval_grasp'
    a = RowLayout.resolve(eval_grasp=True)
    assert a.width == 28 + 8 and a.columns[-8:] == N.GRASP_COLUMNS and a.slice('grasp') == slice(28, 36) and not a.has('grasp_multi')
    assert not RowLayout.resolve(eval_grasp=True, grasp_multi=True).has('grasp_multi')                        # needs eval_best
    assert not RowLayout.resolve(eval_best=True, eval_grasp=False, grasp_multi=True).has('grasp_multi')       # ... and eval_grasp
    b = RowLayout.resolve(eval_best=True, eval_grasp=True, grasp_multi=True)
    assert b.width == 88 + 32 and b.columns[-32:] == N.GRASP_COLUMNS + N.GRASP_MULTI_COLUMNS and b.slice('grasp_multi') == slice(96, 120)
    c = RowLayout.resolve(eval_best=True, eval_symmetric=True, symmetric_multi=True, eval_grasp=True, grasp_multi=True)
    assert c.width == 100 + 32 and c.slice('symmetric') == slice(88, 91) and c.slice('grasp') == slice(100, 108)
    assert N.GRASP_COLUMNS == tuple(f'grasp/pred/{k}' for k in N.GRASP_METRIC_NAMES) and len(N.GRASP_METRIC_NAMES) == 8
    assert N.GRASP_MULTI_COLUMNS[8:10] == ('grasp/best_of_S/IoU', 'grasp/best_of_S/precision')
    assert len(set(c.columns)) == len(c.columns) and BLOCKS[-1][0] == 'grasp_multi'


def test_layouts_without_the_flag_are_todays():
    from vpho_amd.eval_layout import BLOCKS, RowLayout
    old = [b for b in BLOCKS if not b[0].startswith('grasp')]
    assert len(old) == 10
    names = ('eval_best', 'eval_physics', 'physics_multi', 'eval_volume', 'volume_multi', 'eval_hand_bench', 'hand_bench_multi', 'eval_symmetric',
             'symmetric_multi')
    needs = dict(physics_multi='eval_physics', volume_multi='eval_volume', hand_bench_multi='eval_hand_bench', symmetric_multi='eval_symmetric')
    for flags in itertools.product((False, True), repeat=9):
        f = dict(zip(names, flags))
        lay = RowLayout.resolve(**f)
        on = lambda flag: flag is None or (f[flag] and (flag not in needs or (f['eval_best'] and f[needs[flag]])))
        want = tuple(c for b in old if on(b.flag) for c in b.columns)
        assert lay.columns == want and lay.width == len(want) and not lay.has('grasp') and not lay.has('grasp_multi')
        assert lay == RowLayout.resolve(eval_grasp=False, grasp_multi=False, **f) == RowLayout.resolve(eval_grasp=False, grasp_multi=True, **f)
        assert RowLayout.resolve(eval_grasp=True, **f).columns[:lay.width] == lay.columns
    assert RowLayout.resolve().width == 28 and RowLayout.resolve(eval_best=True).width == 88
    assert RowLayout.resolve(eval_best=True, eval_physics=True, physics_multi=True).width == 108
    assert RowLayout.resolve(eval_best=True, eval_symmetric=True, symmetric_multi=True).width == 100
    assert RowLayout.from_width(88) == RowLayout.resolve(eval_best=True)


def test_header_prototypes_count_and_version():
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert re.search(r'VPHO_API int vpho_contact_multi_f32\(const vpho_obj_vertex_accel\* acc, const float\* hand_verts, const float\* hand_normals, '
                     r'int n, int S, int Nh,[^;]*float\* weight, int\* nn_index, double\* nd, double\* vd, void\* stream\);', hdr)
    assert re.search(r'VPHO_API int vpho_contact_agreement_f32\(const float\* weight, const float\* weight_gt,[^;]*int\* counts, double\* values, '
                     r'double\* table, void\* stream\);', hdr)
    count = hdr.count('VPHO_API ') - 1                              # the number itself is pinned in tests/test_abi.py
    for doc in ('README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert (f'{count} entry points' in text or f'exactly the {count} ' in text) and 'contact_multi.hip' in text, doc


def test_ctypes_structure_mirrors_the_header():
    import ctypes
    from vpho_amd import ops
    hdr = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read(), flags=re.S)
    body = re.search(r'typedef\s+struct\s+vpho_obj_vertex_accel\s*\{(.*?)\}\s*vpho_obj_vertex_accel\s*;', hdr, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (' '.join(d.split()) for d in body.split(';'))):
        fields.append((decl.split()[-1].lstrip('*'), 'ptr' if '*' in decl else decl.split()[0]))
    kind = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int'}
    assert [(n, kind[t]) for n, t in ops.ObjVertexAccel._fields_] == fields
    assert fields == [('vert', 'ptr'), ('index', 'ptr'), ('clu_offset', 'ptr'), ('clu_start', 'ptr'), ('clu_sphere', 'ptr'), ('n_obj', 'int')]


# -------------------------------------------------------------------------------------------------------------------------- the table
def test_grasp_table_on_hand_made_rows():
    import torch
    from vpho_amd import evaluate as E
    from vpho_amd.eval_layout import RowLayout
    from vpho_amd.ops_names import GRASP_TABLE
    nan = float('nan')
    pred = torch.tensor([[0.5, 1.0, 0.5, 2 / 3, 0.1, 1.0, 1.0, 1.0],
                         [nan, nan, nan, nan, 0.0, 0.5, 0.0, 1.0],
                         [0.25, 0.5, nan, 0.4, 0.3, 0.0, 1.0, 0.0]])
    t = E.grasp_table(pred)
    assert list(t) == ['pred'] and tuple(t['pred']) == GRASP_TABLE
    assert t['pred']['IoU'] == pytest.approx(0.375) and t['pred']['recall'] == pytest.approx(0.5) and t['pred']['MAE'] == pytest.approx(0.4 / 3)
    assert t['pred']['grasp_agree'] == pytest.approx(2 / 3) and t['pred']['IoU_defined'] == pytest.approx(2 / 3)
    multi = torch.full((3, 24), nan)
    multi[:, 8:16] = pred
    multi[0, 16:24] = 0.25
    t = E.grasp_table(pred, multi)
    assert list(t) == ['pred', 'one_candidate', 'best_of_S', 'mean_of_S']
    assert all(np.isnan(v) for k, v in t['one_candidate'].items() if k != 'IoU_defined') and t['one_candidate']['IoU_defined'] == 0.0   # all-NaN columns
    assert t['best_of_S'] == t['pred'] and t['mean_of_S']['F1'] == 0.25 and t['mean_of_S']['IoU_defined'] == pytest.approx(1 / 3)
    with pytest.raises(ValueError):
        E.grasp_table(torch.zeros(2, 24))
    with pytest.raises(ValueError):
        E.grasp_table(pred, multi[:, :8])
    # summarize finds the blocks by the layout
    lay = RowLayout.resolve(eval_grasp=True)
    rows = torch.zeros(3, lay.width)
    rows[:, lay.slice('grasp')] = pred
    assert E.summarize(rows, lay)['grasp'] == E.grasp_table(pred) and 'grasp' not in E.summarize(torch.zeros(3, 28))


# ------------------------------------------------------------------------------------------------- the restatement vs the fp32 label chain
def test_restatement_against_the_fp32_label_chain():
    from oracle import contact as OC
    objs = CF.objects(0)
    G = CF.GATES
    worst = dict(nd=0.0, vd=0.0, w=0.0, band=0.0)
    for seed, ids in ((1, [2, 4, 5]), (2, [5, 3, 1]), (3, [4, 5, 0])):
        vf, nf, root, right, rt = CF.scene(seed, 3, 2, ids, objs)
        ref = CF.contact_multi(vf, nf, root, right, rt, objs, ids, **G)
        far = CF.gate_distance(ref, G['normal_thresh'], G['vertical_thresh'])
        assert np.isfinite(ref['weight']).all() and 0.3 < ref['contact'].mean() < 0.95      # near-contact scenes: both states are common
        for i, s in itertools.product(range(3), range(2)):
            # the label chain's object vertices (PhysicsLabeler.object_verts): fp64, flipped, root-relative, rounded to fp32 once
            ov = objs[ids[i]] @ rt[i, s, :, :3].T + (rt[i, s, :, 3] - root[i])
            ov[:, 0] *= 1.0 if right[i] else -1.0
            ov = ov.astype(np.float32)
            hw, _, _ = OC.detect(vf[i, s], nf[i, s], ov, np.zeros_like(ov), G['normal_thresh'], G['vertical_thresh'], G['decay'])
            ind = OC._nn(vf[i, s], ov)
            vec = vf[i, s] - ov[ind]
            nd = (vec * nf[i, s]).sum(-1)
            vd = np.linalg.norm(vec - nd[..., None] * nf[i, s], axis=-1)
            assert nd.dtype == vd.dtype == np.float32 and np.array_equal(ind, ref['nearest'][i, s])
            worst['nd'] = max(worst['nd'], float(np.abs(nd - ref['nd'][i, s]).max()))
            worst['vd'] = max(worst['vd'], float(np.abs(vd - ref['vd'][i, s]).max()))
            out = far[i, s] > BAND
            worst['band'] = max(worst['band'], float((~out).mean()))
            assert (~out).mean() <= 0.02                                                    # on the fp64 restatement alone
            assert np.array_equal((hw > 0)[out], ref['contact'][i, s][out])
            dw = np.abs(np.clip(hw, 0.0, 1.0) - ref['weight'][i, s])[out]
            worst['w'] = max(worst['w'], float(dw.max()))
            assert dw.max() <= W_TOL
    print('fp32 label chain vs fp64 restatement:', worst)
    assert worst['nd'] <= BAND and worst['vd'] <= BAND

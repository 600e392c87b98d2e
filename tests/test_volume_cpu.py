"""CPU checks of the hand-object intersection volume (--eval_volume): closing an open mesh, the MANO faces, the
object lattice, the numpy restatement of the kernels and an independent winding-number formulation against the reference fixture
(golden_volume.npz), the row layout, the flags, the header, and the new kernels' register report.  No GPU."""
import glob
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

import tests._penetration_fp64 as O
import tests._volume_fp64 as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_volume.npz'))
N_PAIRS = len(G['pair_hand'])


def _edges(f):
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist()


# ------------------------------------------------------------------------------------------------------------ close_mesh
def test_close_mesh_closes_an_open_torus_with_consistent_winding():
    from vpho_amd.physics_eval import close_mesh, torus_mesh
    _, full = torus_mesh(12, 8)
    _, opened = torus_mesh(12, 8, drop_quad=29)
    assert len(opened) == len(full) - 2
    closed = close_mesh(opened)
    assert len(closed) == len(full) and np.array_equal(closed[:len(opened)], opened)
    e = set(map(tuple, _edges(closed)))
    assert len(e) == 3 * len(closed)                                           # every directed edge once ...
    assert all((b, a) in e for a, b in e)                                      # ... and once in the other direction
    assert np.array_equal(close_mesh(opened), closed)                          # deterministic
    lowest = min(v for a, b in _edges(opened) if (b, a) not in set(map(tuple, _edges(opened))) for v in (a, b))
    assert all(t[0] == lowest for t in closed[len(opened):])                   # the fan starts at the loop's lowest vertex


def test_close_mesh_leaves_a_closed_mesh_alone_and_refuses_non_manifold_edges():
    from vpho_amd.assets import AssetError
    from vpho_amd.physics_eval import box_mesh, close_mesh, torus_mesh
    for f in (torus_mesh(12, 8)[1], box_mesh(np.array([[0, 0, 0], [1, 2, 3]], np.float64), 2)[1]):
        assert np.array_equal(close_mesh(f), f)
    _, f = torus_mesh(6, 4)
    with pytest.raises(AssetError, match='non-manifold'):
        close_mesh(np.concatenate([f, f[:1]]))                                 # a face twice: its edges twice in the same direction
    with pytest.raises(AssetError, match='non-manifold'):
        close_mesh(np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]]))                # three faces on one edge


# ------------------------------------------------------------------------------------------------------------ MANO faces
def _write_mano(root, mano, f):
    d = root / 'mano_v1_2' / 'models'
    d.mkdir(parents=True)
    tab = {k: np.asarray(mano[k], np.float64) for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights')}
    if f is not None:
        tab['f'] = f
    with open(d / 'MANO_RIGHT.pkl', 'wb') as fh:
        pickle.dump(tab, fh, protocol=2)
    return str(root)


def test_load_assets_reads_the_mano_faces(tmp_path, assets):
    from vpho_amd.assets import load_assets
    from vpho_amd.physics_eval import hand_faces, torus_mesh
    _, f = torus_mesh(12, 8, drop_quad=3)
    got = load_assets(_write_mano(tmp_path, assets['mano'], f.astype(np.uint32)))
    m = got['mano']
    assert got['sources']['mano'] != 'synthetic' and m['faces'].dtype == np.int64 and np.array_equal(m['faces'], f)
    assert {k: m[k].shape for k in m if k != 'faces'} == {'v_template': (778, 3), 'shapedirs': (778, 3, 10), 'posedirs': (778, 3, 135),
                                                           'J_regressor': (16, 778), 'weights': (778, 16)}
    closed = hand_faces(got)
    assert len(closed) == len(f) + 2 and np.array_equal(closed[:len(f)], f)


@pytest.mark.parametrize('damage', ['no_f', 'out_of_range', 'negative'])
def test_load_assets_refuses_bad_mano_faces(tmp_path, assets, damage):
    from vpho_amd.assets import AssetError, load_assets
    f = None if damage == 'no_f' else np.array([[0, 1, 778]], np.int64) if damage == 'out_of_range' else np.array([[0, 1, -1]], np.int64)
    with pytest.raises(AssetError, match="lacks the key 'f'" if damage == 'no_f' else 'outside the 778'):
        load_assets(_write_mano(tmp_path, assets['mano'], f))


def test_synthetic_hull_is_closed_outward_sorted_and_reproducible(assets, tmp_path):
    from vpho_amd import assets as A
    from vpho_amd.physics_eval import close_mesh, hand_faces
    f = assets['mano']['faces']
    assert f.dtype == np.int64 and f.ndim == 2 and f.shape[1] == 3 and 0 <= f.min() and f.max() < 778
    assert np.array_equal(f, A.synthetic_assets(0)['mano']['faces']) and np.array_equal(f, A.hull_faces(assets['mano']['v_template']))
    assert f.tolist() == sorted(f.tolist())                                    # lexicographic
    assert np.array_equal(close_mesh(f), f) and np.array_equal(hand_faces(assets), f)
    e = set(map(tuple, _edges(f)))
    assert len(e) == 3 * len(f) and all((b, a) in e for a, b in e)
    v = assets['mano']['v_template'].astype(np.float64)
    t = v[f]
    vol = np.einsum('ij,ij->i', t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0
    assert 1e-4 < vol < 1e-3                                                   # outward (positive), a mitten of some hundred cm^3
    A._reported.clear()
    got = A.load_assets(str(tmp_path / 'nothing_here'))
    assert got['sources']['mano'] == 'synthetic' and np.array_equal(got['mano']['faces'], f)


# ------------------------------------------------------------------------------------------------------------ lattice
def test_solid_lattice_counts_and_ordering():
    from vpho_amd.assets import AssetError
    from vpho_amd.physics_eval import box_mesh, solid_lattice
    lo, hi = np.array([-0.0191, -0.0203, -0.0187]), np.array([0.0297, 0.0082, 0.0148])
    v, f = box_mesh(np.stack([lo, hi]), 2)
    h = 0.005
    c, dims = solid_lattice(v, f, h)
    assert c.dtype == np.float32 and dims.tolist() == np.ceil((hi - lo) / h).astype(int).tolist() == [10, 6, 7]
    assert c.shape == (10 * 6 * 7, 3)
    i, j, k = 3, 4, 5
    want = (lo + (np.array([i, j, k]) + 0.5) * h).astype(np.float32)           # fp64, rounded once
    assert np.array_equal(c[(i * 6 + j) * 7 + k], want)                        # k fastest
    assert np.array_equal(c[1] - c[0] > 0, [False, False, True])
    for o in range(2):
        cc, dd = solid_lattice(G[f'obj{o}_verts'], G[f'obj{o}_faces'], float(G['pitch']))
        assert np.array_equal(cc, G[f'obj{o}_centres']) and np.array_equal(dd, G[f'obj{o}_dims'])
        assert np.array_equal(O.contains(G[f'obj{o}_verts'], G[f'obj{o}_faces'], cc), G[f'obj{o}_solid'])
    assert G['obj0_dims'].tolist() == [8, 8, 8] and G['obj1_dims'].tolist() == [10, 6, 7]
    with pytest.raises(AssetError):
        solid_lattice(v, f, 0.0)


# ------------------------------------------------------------------------------------------------------------ fixture
def _pair(i, key):
    hf = G[f'hand{int(G["pair_hand"][i])}_faces'].astype(np.int64)
    o = int(G['pair_obj'][i])
    if key == 'eye':
        qv = VO.model_frame(G[f'pair{i}_verts_model'], np.concatenate([np.eye(3), np.zeros((3, 1))], 1))
        assert np.array_equal(qv, G[f'pair{i}_verts_model'].astype(np.float64))             # identity pose: p = v exactly
    else:
        qv = VO.model_frame(G[f'pair{i}_verts_cam'], G['rt'][i])
    return qv, hf, G[f'obj{o}_centres'], G[f'obj{o}_solid'], G[f'pair{i}_flags_{key}'], G[f'pair{i}_band_{key}']


def test_fixture_is_what_the_issue_asks_for():
    cells = G['cells_pose'].tolist()
    assert N_PAIRS == 4 and len(set(cells)) == 4 and 0 in cells
    band = sum(int(G[f'pair{i}_band_{k}'].sum()) for i in range(N_PAIRS) for k in ('eye', 'pose'))
    total = sum(G[f'pair{i}_band_{k}'].size for i in range(N_PAIRS) for k in ('eye', 'pose'))
    assert band <= 0.001 * total
    qv, _, _, _, _, _ = _pair(2, 'pose')                                      # the box hand's bbox inside the object's
    ov = G['obj0_verts']
    assert (qv.min(0) > ov.min(0)).all() and (qv.max(0) < ov.max(0)).all()


@pytest.mark.parametrize('key', ['eye', 'pose'])
@pytest.mark.parametrize('i', range(N_PAIRS))
def test_restatement_reproduces_the_reference_flags_and_counts(i, key):
    qv, hf, c, solid, ref, _ = _pair(i, key)
    got = VO.hand_inside(qv, hf, c)
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert int((got & solid).sum()) == int(G[f'cells_{key}'][i])
    assert np.array_equal(got, O.contains(qv, hf, c))                          # and the pairwise oracle of the penetration tests


@pytest.mark.parametrize('key', ['eye', 'pose'])
@pytest.mark.parametrize('i', range(N_PAIRS))
def test_independent_winding_number_agrees_outside_the_edge_band(i, key):
    qv, hf, c, _, ref, band = _pair(i, key)
    w = VO.winding_inside(qv, hf, c.astype(np.float64))
    keep = ~band
    assert keep.sum() >= 0.999 * keep.size
    assert np.array_equal(w[keep], ref[keep]), int((w[keep] != ref[keep]).sum())


# ------------------------------------------------------------------------------------------------------------ layout, flags, header
def test_row_width_and_column_names():
    from vpho_amd import evaluate as E
    from vpho_amd import ops_names as N
    assert N.VOLUME_COLUMNS == ('pred_IV_m3', 'pred_cells', 'gt_IV_m3', 'gt_cells') and E.VOL == len(N.VOLUME_COLUMNS) == 4
    assert N.VOLUME_TABLE == ('IV_cm3', 'IV_max_cm3', 'intersecting_pct')
    old = {(False, False, False): 28, (True, False, False): 88, (False, True, False): 36, (True, True, False): 96, (True, True, True): 108,
           (False, True, True): 36, (True, False, True): 88, (False, False, True): 28}
    width = lambda **flags: E.RowLayout.resolve(**flags).width
    for (b, p, m), w in old.items():
        assert width(eval_best=b, eval_physics=p, physics_multi=m) == w == width(eval_best=b, eval_physics=p, physics_multi=m, eval_volume=False)
        assert width(eval_best=b, eval_physics=p, physics_multi=m, eval_volume=True) == w + 4
    widths = sorted(set(old.values())) + sorted(w + 4 for w in set(old.values()))
    assert len(set(widths)) == len(widths)                                     # summarize tells the layouts apart by their width
    # the flag goes by keyword (tests/test_eval_layout_cpu.py has the whole contract); not named, it is off
    assert E.RowLayout.resolve().eval_volume is False and not E.RowLayout().has('volume')


@pytest.mark.parametrize('width', [28, 88, 36, 96, 108])
def test_summarize_reads_the_volume_block_and_leaves_the_other_tables_alone(width):
    from vpho_amd import evaluate as E
    g = torch.Generator().manual_seed(width)
    rows = torch.rand((6, width), generator=g)
    rows[:, 7] = torch.tensor([1.0, 0, 1, 1, 0, 1])
    before = E.summarize(rows)
    assert 'volume' not in before
    h = 0.005
    cells = torch.tensor([[0.0, 3], [8, 0], [2, 2], [0, 0], [40, 1], [0, 5]])
    vol = torch.stack([cells[:, 0] * h ** 3, cells[:, 0], cells[:, 1] * h ** 3, cells[:, 1]], 1)
    after = E.summarize(torch.cat([rows, vol], 1))
    assert {k: v for k, v in after.items() if k != 'volume'} == before
    v = after['volume']
    assert list(v) == ['pred', 'gt'] and all(tuple(t) == ('IV_cm3', 'IV_max_cm3', 'intersecting_pct') for t in v.values())
    assert v['pred']['IV_cm3'] == pytest.approx(50 / 6 * 0.125, rel=1e-6) and v['pred']['IV_max_cm3'] == pytest.approx(5.0, rel=1e-6)
    assert v['pred']['intersecting_pct'] == pytest.approx(50.0) and v['gt']['intersecting_pct'] == pytest.approx(400 / 6)
    nan = torch.cat([rows, vol], 1)
    nan[:, -2:] = float('nan')                                                 # no object ground truth
    t = E.summarize(nan)['volume']
    assert all(np.isnan(x) for x in t['gt'].values()) and t['pred'] == v['pred']


def test_flags_and_defaults():
    from vpho_amd.configs.args import Config, _parser
    c = Config()
    assert c.eval_volume is False and c.physics_voxel_pitch == 0.005
    a = _parser().parse_args([])
    assert a.eval_volume is False and a.physics_voxel_pitch == 0.005 and a.eval_physics is False
    a = _parser().parse_args(['--eval_volume', '--physics_voxel_pitch', '0.0025'])
    assert a.eval_volume and a.physics_voxel_pitch == 0.0025 and a.eval_physics is False          # independent of --eval_physics


def test_header_declares_the_entry_points_within_abi_13():
    txt = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    m = re.search(r'VPHO_API int vpho_hand_obj_intersection_f64\(([^)]*)\)\s*;', code)
    assert m, 'vpho_hand_obj_intersection_f64 is not declared with VPHO_API'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert len(args) == 15 and args[-1] == 'void* stream' and args[0].startswith('const vpho_obj_mesh_tables*')
    assert [a.split()[-1] for a in args[2:13]] == ['faces', 'F', 'verts', 'n', 'V', 'obj_rt', 'obj_id', 'pitch', 'out', 'flags', 'workspace']
    assert re.search(r'VPHO_API long long vpho_hand_obj_intersection_workspace_bytes\(', code)


# ------------------------------------------------------------------------------------------------------------ kernel resources
def test_volume_kernels_use_no_scratch_and_spill_nothing():
    """from the compiler's own report, kept next to every object by vpho_amd/build.py (as tests/test_kernel_resources.py reads it)"""
    from vpho_amd.build import build_extension
    build_extension()
    path = os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'intersection_volume.hip.usage.txt')
    assert os.path.exists(path), glob.glob(os.path.join(os.path.dirname(path), '*.usage.txt'))
    seen, name = {}, None
    for line in open(path):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = subprocess.run(['c++filt', m.group(1)], capture_output=True, text=True).stdout.strip()
            seen[name] = {}
        for key, pat in (('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('spill', r'VGPRs Spill: (\d+)'), ('sspill', r'SGPRs Spill: (\d+)'),
                         ('lds', r'LDS Size \[bytes/block\]: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    kernels = {k: v for k, v in seen.items() if any(s in k for s in ('hand_mesh_setup_kernel', 'solid_inside_count_kernel', 'volume_finish_kernel'))}
    assert len(kernels) == 3, sorted(seen)
    for k, v in kernels.items():
        assert v['scratch'] == 0 and v['spill'] == 0 and v.get('sspill', 0) == 0, (k, v)
        assert v['lds'] <= 64 * 1024, (k, v)

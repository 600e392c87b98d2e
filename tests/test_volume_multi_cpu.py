"""CPU checks of the multi-hypothesis intersection volume (--eval_best with --eval_volume): the lattice columns of a
solid, the numpy restatement of the column walk against the per-centre restatement and the reference fixture (golden_volume.npz) -- the
proof that the centres of a column may share the x, y part of the parity rule --, the row layout, summarize, the table rule, the header
and the new kernels' register report.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tests._penetration_fp64 as O
import tests._volume_fp64 as VO
import tests._volume_multi_fp64 as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_volume.npz'))
N_PAIRS = len(G['pair_hand'])


# ------------------------------------------------------------------------------------------------------------ solid_columns
def _check_columns(pts, cs):
    assert cs.dtype == np.int32 and cs[0] == 0 and cs[-1] == len(pts) and (np.diff(cs) > 0).all()          # the runs partition pts
    bits = np.ascontiguousarray(pts[:, :2]).view(np.uint32)
    for a, b in zip(cs[:-1], cs[1:]):
        assert (bits[a:b] == bits[a]).all()                                    # x and y are constant along a run ...
    first = bits[cs[:-1]]
    assert (first[1:] != first[:-1]).any(1).all()                              # ... and differ between neighbouring runs
    assert len({tuple(r) for r in first.tolist()}) == len(first)               # a lattice column is ONE run


def test_solid_columns_on_the_fixture_lattices():
    from vpho_amd.physics_eval import solid_columns
    for o in range(2):
        c, solid, dims = G[f'obj{o}_centres'], G[f'obj{o}_solid'], G[f'obj{o}_dims']
        full = solid_columns(c)
        _check_columns(c, full)
        assert len(full) - 1 == dims[0] * dims[1] and (np.diff(full) == dims[2]).all()
        cs = solid_columns(c[solid])
        _check_columns(c[solid], cs)
        assert 0 < len(cs) - 1 <= dims[0] * dims[1]
    assert solid_columns(np.zeros((0, 3), np.float32)).tolist() == [0]
    assert solid_columns(np.array([[1, 2, 3]], np.float32)).tolist() == [0, 1]


def test_solid_columns_on_a_torus_with_empty_columns_and_gaps_in_k():
    from vpho_amd.physics_eval import solid_columns, solid_lattice, torus_mesh
    v, f = torus_mesh(12, 8, 0.045, 0.018)
    c, dims = solid_lattice(v, f, 0.006)
    keep = O.contains(v, f, c)
    pts = c[keep]
    cs = solid_columns(pts)
    _check_columns(pts, cs)
    per_col = keep.reshape(dims[0] * dims[1], dims[2])
    assert len(cs) - 1 == int(per_col.any(1).sum()) < dims[0] * dims[1]        # empty columns have no run
    assert np.array_equal(np.diff(cs), per_col.sum(1)[per_col.any(1)])         # lattice order (i, then j)
    gaps = [(np.diff(np.nonzero(row)[0]) > 1).any() for row in per_col if row.any()]
    assert sum(gaps) >= 5                                                      # the ring is crossed twice: centres not contiguous in k


# ------------------------------------------------------------------------------------------------------------ the column walk
def _pair(i, key):
    hf = G[f'hand{int(G["pair_hand"][i])}_faces'].astype(np.int64)
    o = int(G['pair_obj'][i])
    if key == 'eye':
        qv = VO.model_frame(G[f'pair{i}_verts_model'], np.concatenate([np.eye(3), np.zeros((3, 1))], 1))
    else:
        qv = VO.model_frame(G[f'pair{i}_verts_cam'], G['rt'][i])
    return qv, hf, G[f'obj{o}_centres'], G[f'obj{o}_solid'], G[f'pair{i}_flags_{key}']


@pytest.mark.parametrize('key', ['eye', 'pose'])
@pytest.mark.parametrize('i', range(N_PAIRS))
def test_column_walk_equals_the_per_centre_restatement_and_the_reference(i, key):
    from vpho_amd.physics_eval import solid_columns
    qv, hf, c, solid, ref = _pair(i, key)
    for pts, want_ref in ((c[solid], ref[solid]), (c, ref)):                   # the solid (what the kernel walks) and the full lattice
        got = VM.column_walk_inside(qv, hf, pts, solid_columns(pts))
        assert np.array_equal(got, VO.hand_inside(qv, hf, pts))                # flag for flag
        assert np.array_equal(got, want_ref), int((got != want_ref).sum())     # and the reference's own MeshIntersector
    assert int(got[solid].sum()) == int(G[f'cells_{key}'][i])


def test_column_walk_with_gaps_tall_columns_and_a_partial_cull():
    """a torus object's solid (gaps in k) against a torus hand that covers only part of it: centres of one column on both sides of the
    hand's [0, 512] range in z"""
    from vpho_amd.physics_eval import solid_columns, solid_lattice, torus_mesh
    v, f = torus_mesh(12, 8, 0.045, 0.018)
    c, _ = solid_lattice(v, f, 0.006)
    pts = c[O.contains(v, f, c)]
    hv, hf = torus_mesh(10, 6, 0.03, 0.012)
    qv = hv @ np.array([[1.0, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]]).T + np.array([0.03, 0.004, 0.01])
    got = VM.column_walk_inside(qv, hf, pts, solid_columns(pts))
    want = VO.hand_inside(qv, hf, pts)
    assert np.array_equal(got, want) and 10 < want.sum() < len(pts) / 2
    # the fixture union used on the GPU: the other hands' point faces change no flag
    faces, verts = VM.fixture_union(G)
    for j, i in enumerate((0, 1, 2)):
        o = int(G['pair_obj'][i])
        solid = G[f'obj{o}_centres'][G[f'obj{o}_solid']]
        got = VM.column_walk_inside(VO.model_frame(verts[j], G['rt'][i]), faces, solid, solid_columns(solid))
        assert np.array_equal(got, G[f'pair{i}_flags_pose'][G[f'obj{o}_solid']])


# ------------------------------------------------------------------------------------------------------------ layout
def test_row_width_parameter_order_and_column_names():
    from vpho_amd import evaluate as E
    from vpho_amd import ops_names as N
    assert N.VOLUME_MULTI_COLUMNS == ('one_IV_m3', 'one_cells', 'best_IV_m3', 'best_cells', 'mean_IV_m3', 'mean_cells')
    assert E.VOL_MULTI == len(N.VOLUME_MULTI_COLUMNS) == 6
    old = {(False, False, False): 28, (True, False, False): 88, (False, True, False): 36, (True, True, False): 96, (True, True, True): 108,
           (False, True, True): 36, (True, False, True): 88, (False, False, True): 28}
    widths = set()
    width = lambda **flags: E.RowLayout.resolve(**flags).width
    for (b, p, m), w in old.items():
        for vm in (False, True):
            assert width(eval_best=b, eval_physics=p, physics_multi=m, volume_multi=vm) == w == \
                width(eval_best=b, eval_physics=p, physics_multi=m, volume_multi=vm, eval_volume=False)                  # needs eval_volume
            got = width(eval_best=b, eval_physics=p, physics_multi=m, volume_multi=vm, eval_volume=True)
            assert got == w + 4 + (6 if b and vm else 0)
            widths |= {(w, 'plain'), (w + 4, 'vol'), (got, 'vol+multi' if b and vm else 'vol')}
    assert width(eval_best=True, eval_physics=False, physics_multi=False, volume_multi=True, eval_volume=True) == 98
    assert width(eval_best=True, eval_physics=True, physics_multi=False, volume_multi=True, eval_volume=True) == 106
    assert width(eval_best=True, eval_physics=True, physics_multi=True, volume_multi=True, eval_volume=True) == 118
    assert len({w for w, _ in widths}) == len(widths) == 13                    # summarize tells the layouts apart by their width
    # the flags go by keyword (tests/test_eval_layout_cpu.py has the whole contract); not named, they are off, and None follows cfg
    off = E.RowLayout.resolve()
    assert off.volume_multi is False and off.eval_volume is False and E.RowLayout() == off
    from vpho_amd.configs.args import cfg
    assert not (cfg.eval_best and cfg.eval_volume) and not E.RowLayout.resolve(eval_best=True, eval_volume=True, volume_multi=None).volume_multi


@pytest.mark.parametrize('width', [88, 96, 108])
def test_summarize_reads_the_block_and_leaves_the_other_tables_alone(width):
    from vpho_amd import evaluate as E
    from vpho_amd.ops_names import MULTI_TABLES, VOLUME_TABLE
    g = torch.Generator().manual_seed(width)
    rows = torch.rand((6, width), generator=g)
    rows[:, 7] = torch.tensor([1.0, 0, 1, 1, 0, 1])
    h = 0.005
    cells = torch.tensor([[0.0, 3], [8, 0], [2, 2], [0, 0], [40, 1], [0, 5]])
    vol = torch.stack([cells[:, 0] * h ** 3, cells[:, 0], cells[:, 1] * h ** 3, cells[:, 1]], 1)
    mc = torch.tensor([[4.0, 0, 1.5], [0, 0, 0], [2, 1, 2.25], [0, 0, 0.25], [16, 10, 12], [0, 0, 0]])          # one | best | mean cells
    multi = torch.stack([mc[:, 0] * h ** 3, mc[:, 0], mc[:, 1] * h ** 3, mc[:, 1], mc[:, 2] * h ** 3, mc[:, 2]], 1)
    before = E.summarize(torch.cat([rows, vol], 1))
    wide = torch.cat([rows, multi, vol], 1)
    assert wide.shape[1] == width + 10 and wide.shape[1] in (98, 106, 118)
    after = E.summarize(wide)
    assert {k: v for k, v in after.items() if k != 'volume'} == {k: v for k, v in before.items() if k != 'volume'}
    v = after['volume']
    assert list(v) == ['pred', 'gt'] + list(MULTI_TABLES) and all(tuple(t) == VOLUME_TABLE for t in v.values())
    assert {k: v[k] for k in ('pred', 'gt')} == before['volume']
    for t, name in enumerate(MULTI_TABLES):
        assert v[name]['IV_cm3'] == pytest.approx(float(mc[:, t].mean()) * 0.125, rel=1e-6)
        assert v[name]['IV_max_cm3'] == pytest.approx(float(mc[:, t].max()) * 0.125, rel=1e-6)
        assert v[name]['intersecting_pct'] == pytest.approx(float((mc[:, t] > 0).double().mean() * 100.0))
    assert v['mean_of_S']['intersecting_pct'] == pytest.approx(400 / 6)         # a mean cell count of 0.25 counts as intersecting
    nan = wide.clone()
    nan[2, width + 2:width + 6] = float('nan')                                  # one image with a NaN hypothesis: best and mean
    t = E.summarize(nan)['volume']
    assert t['one_candidate'] == v['one_candidate'] and t['pred'] == v['pred'] and t['gt'] == v['gt']
    assert all(np.isnan(x) for x in t['best_of_S'].values()) and all(np.isnan(x) for x in t['mean_of_S'].values())


def test_table_rule_and_its_nan_rule():
    h = 0.005
    cv = (h * h) * h
    cells = torch.tensor([[3.0, 0, 7, 1], [0, 0, 0, 0], [5, float('nan'), 2, 9], [float('nan'), 4, 4, 4]], dtype=torch.float64)
    per = torch.stack([cells, cv * cells], -1)
    tab = VM.table_rule(per, h)
    assert tab.shape == (4, 6)
    assert tab[0].tolist() == [cv * 3.0, 3.0, cv * 0.0, 0.0, cv * (11.0 / 4.0), 11.0 / 4.0]
    assert tab[1].tolist() == [0.0] * 6
    assert tab[2, :2].tolist() == [cv * 5.0, 5.0] and tab[2, 2:].isnan().all()          # any NaN hypothesis: best and mean NaN, one finite
    assert tab[3].isnan().all()                                                  # hypothesis 0 NaN: one NaN as well
    # an exact integer sum: 3 x 2^53 is not a sum of doubles in any order, but one division of the integer
    big = torch.full((1, 3), 2.0 ** 52 + 1.0, dtype=torch.float64)
    tab = VM.table_rule(torch.stack([big, cv * big], -1), h)
    assert float(tab[0, 5]) == float(3 * (2 ** 52 + 1)) / 3.0 and float(tab[0, 4]) == cv * float(tab[0, 5])
    one = VM.table_rule(per[:1, 2:3], h)                                         # S = 1: the three pairs are equal
    assert one[0, 0:2].tolist() == one[0, 2:4].tolist() == one[0, 4:6].tolist() == [cv * 7.0, 7.0]


# ------------------------------------------------------------------------------------------------------------ header, kernels
def test_header_declares_both_entry_points_within_abi_13():
    txt = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    m = re.search(r'VPHO_API int vpho_hand_obj_intersection_multi_f64\(([^)]*)\)\s*;', code)
    assert m, 'vpho_hand_obj_intersection_multi_f64 is not declared with VPHO_API'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['t', 'solids', 'cols', 'faces', 'F', 'verts', 'n', 'S', 'V', 'obj_rt', 'obj_id', 'pitch', 'per_hyp',
                                                          'table', 'flags', 'workspace', 'workspace_bytes', 'stream']
    assert args[2].startswith('const vpho_obj_solid_columns*')
    assert re.search(r'VPHO_API long long vpho_hand_obj_intersection_multi_workspace_bytes\(int n, int S, int F\)\s*;', code)
    s = re.search(r'typedef struct vpho_obj_solid_columns \{(.*?)\} vpho_obj_solid_columns;', code, flags=re.S)
    assert s and [' '.join(x.split()) for x in s.group(1).split(';') if x.strip()] == ['const int* col_start', 'const int* col_offset', 'int n_obj, max_cols']
    # the split of pen_parity_step lives beside it; the step itself and its three callers are as they were
    common = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'penetration_common.h')).read()
    assert all(f'__device__ inline {sig}' in common for sig in ('void pen_parity_step(', 'bool pen_parity_xy(', 'void pen_parity_z('))
    for name in ('intersection_volume.hip', 'penetration.hip', 'penetration_multi.hip'):
        body = open(os.path.join(ROOT, 'vpho_amd', 'csrc', name)).read()
        assert 'pen_parity_step(' in body and 'pen_parity_xy' not in body


def test_column_walk_kernels_use_no_scratch_and_spill_nothing():
    """from the compiler's own report, kept next to every object by vpho_amd/build.py (as tests/test_volume_cpu.py reads it)"""
    from vpho_amd.build import build_extension
    build_extension()
    path = os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'intersection_volume_multi.hip.usage.txt')
    assert os.path.exists(path), path
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
    kernels = {k: v for k, v in seen.items() if any(s in k for s in ('column_walk_kernel', 'volume_table_kernel'))}
    assert len(kernels) == 2, sorted(seen)
    for k, v in kernels.items():
        assert v['scratch'] == 0 and v['spill'] == 0 and v['sspill'] == 0, (k, v)
        assert v['lds'] <= 64 * 1024, (k, v)

"""CPU side of the symmetry-aware object errors (--eval_symmetric): the symmetry table of vpho_amd/symmetry.py against
the one the reference's own TesterObject.__init__ built (tests/golden/golden_symmetry.npz, made by make_golden_symmetry.py), the float64
referee (tests/_symmetry_fp64.py) against the reference's criterion_SMCE and against closed forms, the row layout, names, flags, the header
and the compiler's report of csrc/obj_symmetry.hip, and that a run without the flag never loads vpho_amd.symmetry.  No GPU."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tests._symmetry_fp64 as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def gold():
    path = os.path.join(GOLD, 'golden_symmetry.npz')
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def ycb():
    from vpho_amd.assets import YCB_NAMES, synthetic_assets
    y = synthetic_assets(0)['ycb']
    names = YCB_NAMES[:3]
    return dict(names=names, bbox3d=np.stack([np.asarray(y[n]['bbox3d'], np.float64) for n in names]),
                verts=np.stack([np.asarray(y[n]['verts_sampled'], np.float64) for n in names]),
                diameter=np.array([float(y[n]['diameter']) for n in names]))


def test_table_equals_the_references(gold, ycb):
    from vpho_amd import symmetry as SY
    infos = json.loads(str(gold['json']))
    R, t = SY.symmetry_table(infos, ycb['names'], 0.01)
    assert R.shape == (3, 628, 3, 3) and t.shape == (3, 628, 3) and R.dtype == t.dtype == np.float64
    assert np.abs(R - gold['R']).max() <= 1e-15 and np.abs(t - gold['t']).max() <= 1e-15
    own = [len(SY.symmetry_transforms(infos[str(i + 1)], 0.01)) for i in range(3)]
    assert own == [1, 3, 628]
    for i in range(3):                                                   # pads are identities
        assert (R[i, own[i]:] == np.eye(3)).all() and (t[i, own[i]:] == 0).all()
    # the continuous loop starts at 1: no identity in the continuous object's own list (its nearest rotation is one step away)
    away = np.abs(R[2] - np.eye(3)).max(axis=(-1, -2))
    assert away.min() > 1e-3
    assert (R[0, 0] == np.eye(3)).all() and (R[1, 0] == np.eye(3)).all()
    # translations: millimetres in the JSON, metres in the table
    assert abs(t[1, 2, 0] - 0.0125) <= 1e-18 and (t[1, 1] == 0).all()
    # every row is a rigid motion
    assert np.abs(np.einsum('okij,oklj->okil', R, R) - np.eye(3)).max() <= 1e-14 and np.abs(np.linalg.det(R) - 1).max() <= 1e-14
    # step 0.05: ceil(pi / 0.05) = 63 steps, 62 rotations, times (identity + one discrete) = 124
    R5, t5 = SY.symmetry_table(infos, ycb['names'][2:], 0.05)
    assert R5.shape == (1, 124, 3, 3) and t5.shape == (1, 124, 3)
    # discrete symmetries are not composed with each other: object 2 has identity + its two entries, not the group of four
    assert own[1] == 3


def test_class_keys_are_the_references_ycb_id():
    from vpho_amd import symmetry as SY
    from vpho_amd.assets import YCB_NAMES
    assert [SY.info_key(n) for n in YCB_NAMES] == [str(i + 1) for i in range(21)]
    assert SY.info_key('002_master_chef_can') == '1' and SY.info_key('061_foam_brick') == '21'


def test_referee_smce_equals_the_references(gold, ycb):
    got = SF.batch(gold['pd_rt'], gold['gt_rt'], gold['obj_idx'], gold['R'], gold['t'], ycb['bbox3d'], ycb['verts'], ycb['diameter'])
    assert got.shape == gold['smce'].shape + (3,)
    assert np.abs(got[..., 0] - gold['smce']).max() <= 1e-12
    plain = np.stack([SF.mce(gold['pd_rt'][b], gold['gt_rt'][b], ycb['bbox3d'][i]) for b, i in enumerate(gold['obj_idx'])])
    assert np.abs(plain - gold['mce']).max() <= 1e-12
    # a table that holds an identity (own or pad) cannot give more than the plain corner error; the continuous object's has none: it is
    # the longest list, so it gets no pad
    assert (got[gold['obj_idx'] != 2, :, 0] <= plain[gold['obj_idx'] != 2] + 1e-15).all()


def test_exact_symmetry_poses_have_zero_error_while_mce_is_centimetres(gold, ycb):
    rng = np.random.default_rng(5)
    # rows well away from the identity (row 0 of the continuous object is a turn by one step, 0.02 rad: millimetres, not centimetres)
    for obj, ks in ((1, (1, 2)), (2, (40, 157, 250, 354, 627))):
        for k in ks:
            G = gold['gt_rt'][int(rng.integers(0, 6))]
            Sk = np.concatenate([np.concatenate([gold['R'][obj, k], gold['t'][obj, k][:, None]], -1), [[0, 0, 0, 1.0]]], 0)
            P = (G @ Sk)[None]
            v = SF.pair(P, G, gold['R'][obj], gold['t'][obj], ycb['bbox3d'][obj], ycb['verts'][obj], ycb['diameter'][obj])[0]
            assert v[0] <= 1e-12 and v[1] <= 1e-12 and v[2] == 1.0, (obj, k, v)
            assert SF.mce(P, G, ycb['bbox3d'][obj])[0] > 0.01, (obj, k)


def test_mssd_is_no_smaller_than_any_single_vertex_and_nan_is_carried(gold, ycb):
    pd, gt, idx = gold['pd_rt'], gold['gt_rt'], gold['obj_idx']
    b = 3
    i = idx[b]
    full = SF.pair(pd[b], gt[b], gold['R'][i], gold['t'][i], ycb['bbox3d'][i], ycb['verts'][i], ycb['diameter'][i])
    for vert in (0, 777, 2047):
        one = SF.pair(pd[b], gt[b], gold['R'][i], gold['t'][i], ycb['bbox3d'][i], ycb['verts'][i][vert:vert + 1], ycb['diameter'][i])
        assert (full[:, 1] >= one[:, 1]).all()
    assert (full[:, 1] >= 0).all() and (full[:, 0] >= 0).all()
    bad = pd[b].copy()
    bad[1, 2, 3] = np.nan
    bad[2, 0, 0] = np.inf
    v = SF.pair(bad, gt[b], gold['R'][i], gold['t'][i], ycb['bbox3d'][i], ycb['verts'][i], ycb['diameter'][i])
    assert np.isnan(v[1:3, :2]).all() and (v[1:3, 2] == 0).all() and np.array_equal(v[[0, 3, 4]], full[[0, 3, 4]])
    per = np.stack([full, v])
    one, best, mean = SF.table_rule(per)
    assert np.array_equal(one, per[:, 0]) and np.isfinite(best).all() and np.isnan(mean[1, :2]).all() and np.isfinite(mean[1, 2])
    nan0 = per.copy()
    nan0[0, 0, :2] = np.nan
    assert np.isnan(SF.table_rule(nan0)[1][0, :2]).all()                       # a NaN hypothesis 0 stays; a later one is passed over
    assert best[0, 0] == full[:, 0].min() and best[0, 2] == full[:, 2].max()


def test_layout_widths_flags_and_the_pinned_blocks():
    from vpho_amd import eval_layout as L
    from vpho_amd import evaluate as E
    from vpho_amd import ops_names as N
    from vpho_amd.eval_layout import RowLayout
    assert N.SYM_METRIC_NAMES == ('SMCE', 'MSSD', 'MSSD01d')
    assert N.SYM_COLUMNS == ('sym/pred/SMCE', 'sym/pred/MSSD', 'sym/pred/MSSD01d') and len(N.SYM_MULTI_COLUMNS) == 9
    assert N.SYM_MULTI_COLUMNS[0] == 'sym/one_candidate/SMCE' and N.SYM_MULTI_COLUMNS[-1] == 'sym/mean_of_S/MSSD01d'
    assert E.SYM == 3 and E.SYM_MULTI == 9
    assert [b[0] for b in L.BLOCKS[:8]] == ['base', 'multi', 'physics', 'physics_multi', 'volume_multi', 'volume', 'hand_bench', 'hand_bench_multi']
    assert [b[:3] for b in L.BLOCKS[8:10]] == [('symmetric', 'eval_symmetric', 3), ('symmetric_multi', 'symmetric_multi', 9)]
    assert L.BLOCKS[9].needs == 'eval_symmetric' and L.BLOCKS[8].needs is None
    older = dict(eval_best=True, eval_physics=True, physics_multi=True, eval_volume=True, volume_multi=True, eval_hand_bench=True, hand_bench_multi=True)
    seven = RowLayout.resolve(**older)
    assert seven.width == 158 and not seven.has('symmetric') and not seven.eval_symmetric
    nine = RowLayout.resolve(eval_symmetric=True, symmetric_multi=True, **older)
    assert nine.width == 170 and nine.slice('symmetric') == slice(158, 161) and nine.slice('symmetric_multi') == slice(161, 170)
    assert nine.columns[:158] == seven.columns and nine.columns[158:] == N.SYM_COLUMNS + N.SYM_MULTI_COLUMNS
    only = RowLayout.resolve(eval_symmetric=True)
    assert only.width == 31 and only.slice('symmetric') == slice(28, 31)
    # symmetric_multi needs both flags
    assert not RowLayout.resolve(eval_symmetric=True, symmetric_multi=True).symmetric_multi
    assert not RowLayout.resolve(eval_best=True, symmetric_multi=True).symmetric_multi
    both = RowLayout.resolve(eval_best=True, eval_symmetric=True, symmetric_multi=True)
    assert both.symmetric_multi and both.width == 28 + 60 + 3 + 9
    # from_width keeps knowing the 13 plain widths only
    five = ('eval_best', 'eval_physics', 'physics_multi', 'eval_volume', 'volume_multi')
    assert sorted(L._BY_WIDTH) == sorted({RowLayout.resolve(**dict(zip(five, f))).width for f in __import__('itertools').product((False, True), repeat=5)})
    assert len(L._BY_WIDTH) == 13 and all(not l.eval_symmetric for l in L._BY_WIDTH.values())
    with pytest.raises(ValueError):
        RowLayout.from_width(31)
    with pytest.raises(ValueError):
        RowLayout.from_width(170)


def test_symmetric_table_and_summarize_on_hand_made_rows():
    import torch
    from vpho_amd import evaluate as E
    from vpho_amd.eval_layout import RowLayout
    from vpho_amd.ops_names import MULTI_TABLES, SYM_METRIC_NAMES
    g = torch.Generator().manual_seed(11)
    blk = torch.rand((5, 12), generator=g)
    t = E.symmetric_table(blk[:, :3])
    assert list(t) == ['pred'] and tuple(t['pred']) == SYM_METRIC_NAMES and t['pred']['MSSD'] == float(blk[:, 1].double().mean())
    t = E.symmetric_table(blk[:, :3], blk[:, 3:])
    assert list(t) == ['pred'] + list(MULTI_TABLES) and t['mean_of_S']['MSSD01d'] == float(blk[:, 11].double().mean())
    with pytest.raises(ValueError):
        E.symmetric_table(blk[:, :9])
    with pytest.raises(ValueError):
        E.symmetric_table(blk[:, :3], blk[:, 3:6])
    layout = RowLayout.resolve(eval_best=True, eval_hand_bench=True, eval_symmetric=True, symmetric_multi=True)
    rows = torch.rand((5, layout.width), generator=g)
    res = E.summarize(rows, layout)
    assert list(res)[-2:] == ['hand_bench', 'symmetric']                          # 'symmetric' comes after 'hand_bench'
    assert layout.slice('symmetric_multi').stop == layout.width
    assert res['symmetric'] == E.symmetric_table(rows[:, layout.slice('symmetric')], rows[:, layout.slice('symmetric').stop:])
    plain = RowLayout.resolve(eval_best=True, eval_hand_bench=True)
    older = E.summarize(rows[:, :plain.width], plain)
    assert {k: v for k, v in res.items() if k != 'symmetric'} == older
    with pytest.raises(ValueError):
        E.summarize(rows)                                                        # no layout: the width names none


def test_flags_defaults_signatures_and_header():
    from vpho_amd import evaluate as E
    from vpho_amd.configs import args as A
    from vpho_amd.trainer import Trainer
    assert A.Config().eval_symmetric is False and A.Config().max_sym_disc_step == 0.01
    a = A._parser().parse_args(['--mode', 'eval', '--eval_symmetric', '--max_sym_disc_step', '0.05'])
    assert a.eval_symmetric is True and a.max_sym_disc_step == 0.05
    a = A._parser().parse_args(['--mode', 'eval'])
    assert a.eval_symmetric is False and a.max_sym_disc_step == 0.01
    # Trainer.eval passes its keywords to RowLayout.resolve, the two symmetric flags among them; not named there, or None, they follow
    # cfg.eval_symmetric (and cfg.eval_best)
    with pytest.raises(TypeError, match='symmetric_mult'):
        Trainer.eval(object(), symmetric_mult=True)                             # the keywords are checked: a misspelt flag is named
    saved = A.cfg.eval_best, A.cfg.eval_symmetric
    try:
        from vpho_amd.eval_layout import RowLayout
        off = dict(eval_physics=False, physics_multi=False, eval_volume=False, volume_multi=False, eval_hand_bench=False, hand_bench_multi=False)
        A.cfg.eval_best, A.cfg.eval_symmetric = True, True
        assert RowLayout.resolve(eval_best=None, eval_symmetric=None, symmetric_multi=None, **off).width == 100
        assert RowLayout.resolve(eval_best=False, eval_symmetric=None, symmetric_multi=None, **off).width == 31
        A.cfg.eval_best, A.cfg.eval_symmetric = True, False
        assert RowLayout.resolve(eval_best=None, eval_symmetric=None, symmetric_multi=None, **off).width == 88
    finally:
        A.cfg.eval_best, A.cfg.eval_symmetric = saved
    for fn in (E.symmetric_block, E.symmetric_multi_block):
        assert list(inspect.signature(fn).parameters) == ['out', 'data', 'meter']
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert re.search(r'VPHO_API int vpho_obj_symmetry_multi_f64\(const vpho_obj_symmetry_tables\* t, const double\* pd_rt, const double\* gt_rt, '
                     r'const int\* obj_id,\s+int n_img, int n_hyp, int prune, double\* per, void\* stream\);', hdr)
    assert re.search(r'VPHO_API int vpho_obj_symmetry_table_f64\(const double\* per, int n_img, int n_hyp, double\* one, double\* best, double\* mean, '
                     r'void\* stream\);', hdr)
    assert 'test.py:377-398' in hdr and ':204-226' in hdr and ':103-150' in hdr
    count = hdr.count('VPHO_API ') - 1
    assert count >= 126
    for doc in ('README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert f'{count} ' in text and '--eval_symmetric' in text, (doc, count)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'obj_symmetry.hip' in design


def test_ctypes_structure_mirrors_the_header():
    import ctypes
    from tests.test_abi import _header_structs
    from vpho_amd import ops
    kind = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int'}
    assert [(f[0], kind[f[1]]) for f in ops.ObjSymmetryTables._fields_] == _header_structs()['vpho_obj_symmetry_tables']
    for name in ('vpho_obj_symmetry_multi_f64', 'vpho_obj_symmetry_table_f64'):
        assert hasattr(ops.lib, name), name
    assert ops.SYMMETRY_MAX_TRANSFORMS == 4096


def test_too_long_a_table_and_cpu_tensors_are_refused_without_a_gpu(ycb):
    """the refusals that need no device: they come before anything is copied or launched"""
    from vpho_amd import ops
    from vpho_amd.assets import synthetic_assets
    y = {n: synthetic_assets(0)['ycb'][n] for n in ycb['names']}
    R = np.tile(np.eye(3), (3, 4097, 1, 1))
    with pytest.raises(ops.VphoError, match='4097'):
        ops.ObjectSymmetry(y, (R, np.zeros((3, 4097, 3))), 'cuda:0')
    with pytest.raises(ops.VphoError):
        ops.ObjectSymmetry(y, (R[:2, :4], np.zeros((2, 4, 3))), 'cuda:0')          # two objects' rows for three objects
    with pytest.raises(ops.VphoError):
        ops.ObjectSymmetry(y, (R[:, :4], np.zeros((3, 4, 3))), 'cpu')


def test_kernels_report_no_scratch_and_no_spill():
    """the compiler's own report (vpho_amd/build.py keeps it next to the object), as tests/test_kernel_resources.py reads it"""
    from vpho_amd.build import build_extension
    build_extension()
    path = os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'obj_symmetry.hip.usage.txt')
    seen, name = {}, None
    for line in open(path):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (('spill', r'VGPRs Spill: (\d+)'), ('sspill', r'SGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds', r'LDS Size \[bytes/block\]: (\d+)'), ('vgpr', r' VGPRs: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    main = [k for k in seen if 'obj_symmetry_multi_kernel' in k]
    table = [k for k in seen if 'obj_symmetry_table_kernel' in k]
    assert len(main) == 1 and len(table) == 1, sorted(seen)
    for k in main + table:
        assert seen[k]['scratch'] == 0 and seen[k]['spill'] == 0 and seen[k]['sspill'] == 0, (k, seen[k])
    # 2048 fp64 vertices + corners + the reduction slots: three workgroups share a CU's 160 KB, each wave within 128 registers
    assert 48 * 1024 <= seen[main[0]]['lds'] <= 160 * 1024 // 3 and seen[main[0]]['vgpr'] <= 128


def test_a_run_without_the_flag_never_loads_the_symmetry_module():
    code = ('import sys\n'
            'import vpho_amd.trainer, vpho_amd.ops, vpho_amd.evaluate, vpho_amd.eval_layout, vpho_amd.configs.args as A\n'
            'assert A.cfg.eval_symmetric is False\n'
            'L = vpho_amd.eval_layout.RowLayout\n'
            'assert not L.resolve(**dict.fromkeys(L.__dataclass_fields__)).has("symmetric")\n'
            "assert 'vpho_amd.symmetry' not in sys.modules, 'vpho_amd.symmetry was imported'\n"
            "print('clean')\n")
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('clean'), r.stdout[-1000:] + r.stderr[-2000:]
    src = open(os.path.join(ROOT, 'vpho_amd', 'evaluate.py')).read()
    assert len(re.findall(r'import .*\bsymmetry\b', src)) == 1 and re.search(r'if key not in _OBJ_SYMMETRY:\n\s+from \. import ops, symmetry', src)
    for mod in ('ops.py', 'trainer.py', 'eval_layout.py', 'ops_names.py', '__init__.py', 'model/engine.py'):
        assert not re.search(r'import symmetry|import .*, symmetry|vpho_amd\.symmetry', open(os.path.join(ROOT, 'vpho_amd', mod)).read()), mod


def test_synthetic_model_info_is_seeded_announced_once_and_a_short_json_raises(tmp_path, capsys):
    from vpho_amd import assets as A
    from vpho_amd import symmetry as SY
    root = str(tmp_path / 'asset')
    capsys.readouterr()
    a = SY.load_symmetries(root)
    b = SY.load_symmetries(root)
    err = capsys.readouterr().err
    assert err.count('SYNTHETIC model-info') <= 1 and a == b == SY.synthetic_model_info(seed=0)
    msg = [m for m in A._reported if 'SYNTHETIC model-info' in m]
    assert len(msg) == 1 and 'not true of a box' in msg[0]
    assert sorted(a, key=int) == [str(i + 1) for i in range(21)]
    cont = [k for k, v in a.items() if 'symmetries_continuous' in v]
    assert cont == [str(i + 1) for i in range(0, 21, 3)]                          # every third object, from the first
    assert [k for k, v in SY.synthetic_model_info(seed=1).items() if 'symmetries_continuous' in v] == [str(i + 1) for i in range(2, 21, 3)]
    R, t = SY.symmetry_table(a, A.YCB_NAMES, 0.01)
    assert R.shape == (21, 4 * 314, 3, 3) and (t == 0).all() and R.shape[1] <= SY.MAX_TRANSFORMS
    # the half-turns are true of the synthetic boxes: they map the corner set onto itself
    box = np.asarray(A.synthetic_assets(0)['ycb'][A.YCB_NAMES[1]]['bbox3d'], np.float64)
    own = SY.symmetry_transforms(a['2'], 0.01)
    assert len(own) == 4
    for Rk, tk in own:
        moved = box @ Rk.T + tk
        assert sorted(map(tuple, np.round(moved, 12))) == sorted(map(tuple, np.round(box, 12)))
    # a file that exists wins; one that lacks a class raises
    d = tmp_path / 'asset' / '2023_NIPS_DeepSimHO'
    d.mkdir(parents=True)
    (d / 'assets_models_info.json').write_text(json.dumps({k: v for k, v in a.items() if k != '7'}))
    with pytest.raises(A.AssetError, match='008_pudding_box'):
        SY.load_symmetries(root)
    assert SY.load_symmetries(root, A.YCB_NAMES[:6]) == {k: v for k, v in a.items() if k != '7'}
    (d / 'assets_models_info.json').write_text('{not json')
    with pytest.raises(A.AssetError):
        SY.load_symmetries(root, A.YCB_NAMES[:6])

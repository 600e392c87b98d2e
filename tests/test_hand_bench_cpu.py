"""CPU side of the hand benchmark metrics (--eval_hand_bench): the float64 restatement (tests/_hand_bench_fp64.py)
against the reference's own alignment and against brute-force forms of the leaderboard definitions; names, widths, the flag, the frozen
signatures, the host-side table and the compiler's report of the new kernels.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tests._hand_bench_fp64 as HB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def fixture():
    z, g = np.load(os.path.join(GOLD, 'golden_multihyp.npz')), np.load(os.path.join(GOLD, 'golden_hand_bench.npz'))
    cam = {k: HB.postprocess(z[f'pd_{k}_model'], z['root_joint'], z['is_right']) for k in ('joint', 'vert')}
    return z, g, cam


def test_restatement_alignment_equals_the_references(fixture):
    """the reference's rigid_align_AtoB runs in float32 numpy on these float32 points; the restatement in float64.  Tolerance: the one
    tests/test_gpu_metrics.py grants PA-MJE against the same reference function, rtol 2e-5 on the mean aligned error of a pair."""
    z, g, cam = fixture
    for k in ('joint', 'vert'):
        gt = z[f'gt_{k}']
        for b in range(gt.shape[0]):
            for s in range(cam[k].shape[1]):
                mine = HB.errors(HB.align(cam[k][b, s], gt[b]), gt[b]).mean()
                ref = HB.errors(g[f'aligned_{k}'][b, s], gt[b]).mean()
                assert abs(mine - ref) <= 2e-5 * ref, (k, b, s, mine, ref)


def test_g_table_is_the_closed_form_and_the_ops_names_constants_are_the_leaderboards():
    from vpho_amd import ops_names as N
    assert N.HAND_BENCH_F_THRESH == HB.F_THRESH == (0.005, 0.015) and N.HAND_BENCH_AUC == HB.AUC == (0.0, 0.05, 100)
    t = HB.thresholds()
    g = HB.g_table(t)
    assert t.shape == (100,) and g.shape == (101,) and g[0] == 0.0
    for c in range(1, 101):
        assert abs(g[c] - (c - 1 + 0.5 * (c < 100)) / 99) <= 1e-15, c


def test_sum_of_g_is_the_trapezoid_of_the_pck_curve_on_every_pair(fixture):
    """FreiHAND EvalUtil.get_measures: PCK(t_j) = share of points with e <= t_j, AUC = trapz(PCK, t) / (t[-1] - t[0])"""
    z, g, cam = fixture
    t = HB.thresholds()
    G = HB.g_table(t)
    trapz = getattr(np, 'trapezoid', None) or np.trapz
    for k in ('joint', 'vert'):
        gt = z[f'gt_{k}']
        P = gt.shape[1]
        for b in range(gt.shape[0]):
            for s in range(cam[k].shape[1]):
                for X in (cam[k][b, s], HB.align(cam[k][b, s], gt[b])):
                    e = HB.errors(X, gt[b])
                    pck = (e[:, None] <= t[None, :]).mean(0)
                    auc = trapz(pck, t) / (t[-1] - t[0])
                    assert abs(auc - G[HB.pck_counts(e, t)].sum() / P) <= 1e-14, (k, b, s)


def test_fixture_holds_what_the_restatement_gives_and_the_band_is_nearly_empty(fixture):
    z, g, cam = fixture
    assert g['aligned_vert'].shape == (6, 8, 778, 3) and g['aligned_vert'].dtype == np.float32 and g['aligned_joint'].shape == (6, 8, 21, 3)
    assert g['counts_vert'].shape == (6, 8, 10) and g['band_mask_vert'].shape == (6, 8, 8, 778)
    # 7 of the 298 752 comparisons lie within 2e-7 m of their threshold; no error lies within 6.5e-10 m of an AUC table entry
    assert int(g['band_mask_vert'].sum()) == 7 and g['band_mask_vert'].size == 298752
    assert float(g['margin_e_vert']) > 6.5e-10 and float(g['margin_e_joint']) > 6.5e-10
    for b, s in ((0, 0), (1, 7), (4, 3)):                               # a right and two left-hand pairs recomputed in full
        values, counts, band, _ = HB.pair(cam['vert'][b, s], z['gt_vert'][b])
        assert (counts == g['counts_vert'][b, s]).all() and (band == g['band_mask_vert'][b, s].sum(-1)).all()
        assert np.array_equal(values, g['values_vert'][b, s])
    values, counts, _, _ = HB.pair(cam['joint'][2, 5], z['gt_joint'][2], with_fscore=False)
    assert (counts == g['counts_joint'][2, 5]).all() and np.isnan(values[2:]).all() and np.array_equal(values[:2], g['values_joint'][2, 5, :2])
    assert os.path.getsize(os.path.join(GOLD, 'golden_hand_bench.npz')) < 1 << 20


def test_restatement_closed_forms():
    """identical sets; the p + r = 0 branch; NaN; the table rule"""
    rng = np.random.default_rng(0)
    B = (rng.normal(size=(40, 3)) * 0.03 + [0, 0, 0.6]).astype(np.float32)
    v, c, _, _ = HB.pair(B.copy(), B)
    assert v[0] == 1.0 and v[2] == v[3] == v[4] == v[5] == 1.0 and v[1] >= 1 - 0.5 / 99 - 1e-12 and c[8] == 40 * 100
    far = (B + np.float32(0.2)).astype(np.float32)
    v, c, _, _ = HB.pair(far, B)
    assert v[0] == 0.0 and v[2] == v[3] == 0.0 and c[:4].sum() == 0
    bad = B.copy()
    bad[3, 1] = np.nan
    assert np.isnan(HB.pair(bad, B)[0]).all()
    per = rng.uniform(size=(3, 4, 8))
    per[1, 2, 5] = np.nan
    one, best, mean = HB.table_rule(per)
    assert np.array_equal(one, per[:, 0]) and np.isnan(best[1, 5]) and np.isnan(mean[1, 5]) and np.isfinite(best).sum() == 23
    assert best[0, 0] == per[0, :, 0].max()


def test_names_widths_flag_and_header():
    from vpho_amd import evaluate as E
    from vpho_amd import ops_names as N
    from vpho_amd.configs import args as A
    assert N.HAND_BENCH_NAMES == ('AUC_J', 'PA_AUC_J', 'AUC_V', 'PA_AUC_V', 'F@5', 'F@15', 'PA_F@5', 'PA_F@15')
    assert len(N.HAND_BENCH_NAMES) == 8 and len(N.HAND_BENCH_COLUMNS) == E.HAND_BENCH == 16 and len(N.HAND_BENCH_MULTI_COLUMNS) == E.HAND_BENCH_MULTI == 24
    assert N.HAND_BENCH_COLUMNS[0] == 'hand_bench/agg/AUC_J' and N.HAND_BENCH_COLUMNS[8] == 'hand_bench/reg/AUC_J'
    assert N.HAND_BENCH_MULTI_COLUMNS[0] == 'hand_bench/one_candidate/AUC_J' and N.HAND_BENCH_MULTI_COLUMNS[-1] == 'hand_bench/mean_of_S/PA_F@15'
    assert N.HAND_BENCH_TABLE == N.HAND_BENCH_NAMES
    assert E.RowLayout.resolve(eval_hand_bench=True, hand_bench_multi=False).width - 28 == 16
    assert E.RowLayout.resolve(eval_best=True, eval_hand_bench=True, hand_bench_multi=True).width - 88 == 40
    assert A.Config().eval_hand_bench is False
    assert A._parser().parse_args(['--mode', 'eval', '--eval_hand_bench']).eval_hand_bench is True
    assert A._parser().parse_args(['--mode', 'eval']).eval_hand_bench is False
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert re.search(r'VPHO_API int vpho_hand_bench_multi_f32\(', hdr) and re.search(r'VPHO_API int vpho_hand_bench_table_f64\(', hdr)
    count = hdr.count('VPHO_API ') - 1                              # the documents say what the header says
    for doc in ('README.md', 'INTEGRATION.md'):
        assert f'{count} ' in open(os.path.join(ROOT, doc)).read(), (doc, count)


def test_signatures_the_new_keywords_and_the_frozen_ones():
    from vpho_amd import evaluate as E
    # the flags go by keyword, eval_hand_bench and hand_bench_multi among them (tests/test_eval_layout_cpu.py has the whole contract)
    lay = E.RowLayout.resolve(eval_best=True, eval_hand_bench=True, hand_bench_multi=True)
    assert lay.eval_hand_bench and lay.hand_bench_multi and not E.RowLayout.resolve().eval_hand_bench
    assert list(inspect.signature(E.summarize).parameters) == ['rows', 'layout'] and inspect.signature(E.summarize).parameters['layout'].default is None
    for fn in (E.hand_bench_block, E.hand_bench_multi_block):
        assert list(inspect.signature(fn).parameters) == ['out', 'data', 'gt_joint', 'gt_vert']


def test_hand_bench_table_on_a_hand_made_block():
    from vpho_amd import evaluate as E
    from vpho_amd.ops_names import HAND_BENCH_TABLE, MULTI_TABLES
    g = torch.Generator().manual_seed(3)
    blk = torch.rand((5, 40), generator=g)
    blk[:, 2] = float('nan')                                             # the aggregated hand's AUC_V in hand mode 2D_pt_joint
    t = E.hand_bench_table(blk[:, :16])
    assert list(t) == ['agg', 'reg'] and all(tuple(v) == HAND_BENCH_TABLE for v in t.values())
    assert np.isnan(t['agg']['AUC_V']) and t['agg']['AUC_J'] == float(blk[:, 0].double().mean()) and t['reg']['PA_F@15'] == float(blk[:, 15].double().mean())
    t = E.hand_bench_table(blk[:, :16], blk[:, 16:])
    assert list(t) == ['agg', 'reg'] + list(MULTI_TABLES)
    assert t['one_candidate']['AUC_J'] == float(blk[:, 16].double().mean()) and t['mean_of_S']['PA_F@15'] == float(blk[:, 39].double().mean())
    assert sum(np.isnan(v) for r in t.values() for v in r.values()) == 1
    assert all(0.0 <= v <= 1.0 for r in t.values() for v in r.values() if not np.isnan(v))
    with pytest.raises(ValueError):
        E.hand_bench_table(blk[:, :24])
    with pytest.raises(ValueError):
        E.hand_bench_table(blk)                                           # both blocks in one tensor: no longer told apart by width
    with pytest.raises(ValueError):
        E.hand_bench_table(blk[:, :16], blk[:, 16:32])


def test_new_kernels_report_no_scratch_and_no_spill():
    """the compiler's own report (vpho_amd/build.py keeps it next to the object), as tests/test_kernel_resources.py reads it"""
    from vpho_amd.build import build_extension
    build_extension()
    path = os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'hand_bench.hip.usage.txt')
    seen, name = {}, None
    for line in open(path):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (('spill', r'VGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('lds', r'LDS Size \[bytes/block\]: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    main = [k for k in seen if 'hand_bench_multi_kernel' in k]
    table = [k for k in seen if 'hand_bench_table_kernel' in k]
    assert len(main) == 1 and len(table) == 1, sorted(seen)
    for k in main + table:
        assert seen[k]['scratch'] == 0 and seen[k]['spill'] == 0, (k, seen[k])
    assert seen[main[0]]['lds'] <= 48 * 1024                             # three workgroups per CU
    # both files call the one similarity_from_cov of the shared header
    for f in ('metrics.hip', 'hand_bench.hip'):
        src = open(os.path.join(ROOT, 'vpho_amd', 'csrc', f)).read()
        assert '#include "procrustes.h"' in src and 'similarity_from_cov(' in src and 'void similarity_from_cov' not in src

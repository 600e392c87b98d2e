"""Hand benchmark metrics on the device (--eval_hand_bench): csrc/hand_bench.hip against the float64 restatement
tests/_hand_bench_fp64.py (another route wherever there is one) and against closed forms that need no restatement.

The comparison rules (fixed by the definitions, not by what the kernel gives):
* the AUC counts sum_p c_p are EQUAL: both sides form the errors in float64 on the same float32 points; no error of any case here lies
  within 6.5e-10 m (fixture) / 1e-9 m (synthetic cases) of a table entry, the two alignment routes differ by about 1e-15 m;
* each of the eight nearest-neighbour counts differs from the restatement's by at most the number of restatement distances of that
  (pair, set, direction, threshold) within 2e-7 m of the threshold -- the rounding of an fp32 point at camera depth; the share of such
  distances is asserted to be <= 1e-4 before the rule is used, so it cannot hide a failure;
* AUC within 1e-12 of the restatement; F = the F rule on the kernel's own counts, to 1e-15."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tests._hand_bench_fp64 as HB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'
# (n, S, P): seed of tests/_hand_bench_fp64.synthetic, found on the CPU by find_seed (margins of seed 0: errors >= 4.2e-8 m from every
# table entry, nearest-neighbour distances >= 1.0e-6 m from both thresholds, in all four shapes)
SEEDS = {(3, 5, 70): 0, (2, 3, 21): 0, (1, 1, 257): 0, (2, 1, 778): 0}
EVAL_ARGS = dict(sample_num=4, sampling_steps=5, topk_hand=8, topk_obj=3, sample_T0=0.2, eval_batch_size=4, num_batches=2, random_seed=7)
_SHARED = {}


def _dev(*arrays):
    return [torch.as_tensor(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _run(pd, gt, root, is_right, **kw):
    from vpho_amd import ops
    pd, gt, root, is_right = _dev(np.asarray(pd, np.float32), np.asarray(gt, np.float32), np.asarray(root, np.float32), np.asarray(is_right, bool))
    return ops.hand_bench_multi(pd, gt, root, is_right, **kw)


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _check(values, counts, ref_values, ref_counts, band, P, with_fscore):
    values, counts = values.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
    assert values.shape == ref_values.shape and counts.shape == ref_counts.shape
    assert np.array_equal(counts[..., 8:], ref_counts[..., 8:]), 'AUC counts'
    assert np.abs(values[..., :2] - ref_values[..., :2]).max() <= 1e-12
    if with_fscore:
        assert band.sum() <= 1e-4 * band.size * P
        assert (np.abs(counts[..., :8] - ref_counts[..., :8]) <= band).all(), (counts[..., :8] - ref_counts[..., :8], band)
        assert np.abs(values - HB.values_from_counts(counts, P, values[..., :2])).max() <= 1e-15
        assert (values[..., 2:] >= 0).all() and (values[..., 2:] <= 1).all()
    else:
        assert np.isnan(values[..., 2:]).all() and (counts[..., :8] == 0).all()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLD, 'golden_multihyp.npz')), np.load(os.path.join(GOLD, 'golden_hand_bench.npz'))


def test_fixture_vertices_counts_and_values(golden):
    z, g = golden
    values, counts = _run(z['pd_vert_model'], z['gt_vert'], z['root_joint'], z['is_right'], counts=True)
    assert values.dtype == torch.float64 and counts.dtype == torch.int32 and values.shape == (6, 8, 6) and counts.shape == (6, 8, 10)
    print('kernel - restatement, nearest-neighbour counts:', (counts.cpu().numpy()[..., :8] - g['counts_vert'][..., :8]).reshape(-1, 8).sum(0))
    _check(values, counts, g['values_vert'], g['counts_vert'].astype(np.int64), g['band_mask_vert'].sum(-1), 778, True)


def test_fixture_joints_auc_only(golden):
    z, g = golden
    values, counts = _run(z['pd_joint_model'], z['gt_joint'], z['root_joint'], z['is_right'], with_fscore=False, counts=True)
    _check(values, counts, g['values_joint'], g['counts_joint'].astype(np.int64), None, 21, False)


@pytest.mark.parametrize('shape', sorted(SEEDS))
def test_small_and_odd_shapes(shape):
    n, S, P = shape
    pd, gt, root, is_right = HB.synthetic(n, S, P, SEEDS[shape])
    ref_values, ref_counts, band, margin = HB.bench_multi(pd, gt, root, is_right)
    assert margin[0] > 1e-9 and margin[1] > HB.BAND and band.sum() == 0          # the recorded seed keeps every comparison off its threshold
    assert 0 < ref_counts[..., :8].sum() < 8 * n * S * P                        # ... and the case is not a trivial one
    values, counts = _run(pd, gt, root, is_right, counts=True)
    _check(values, counts, ref_values, ref_counts, band, P, True)


def test_no_images_and_a_single_hypothesis():
    from vpho_amd import ops
    pd, gt, root, is_right = HB.synthetic(2, 1, 21, 5)
    values, counts = _run(pd[:0], gt[:0], root[:0], is_right[:0], counts=True)
    assert values.shape == (0, 1, 6) and counts.shape == (0, 1, 10)
    one, best, mean = ops.hand_bench_table(torch.zeros((0, 3, 8), device=DEV, dtype=torch.float64))
    assert one.shape == best.shape == mean.shape == (0, 8)
    per = torch.rand((3, 1, 8), device=DEV, dtype=torch.float64)                # S = 1: all three tables are the hypothesis itself
    one, best, mean = ops.hand_bench_table(per)
    assert _bytes_equal(one, per[:, 0].contiguous()) and _bytes_equal(best, one) and _bytes_equal(mean, one)


def test_identical_sets_are_exact():
    """pd bit-equal to gt, right hands: every raw error and distance is 0 -> raw AUC = G[n_t] = 1 and raw F = 1 exactly; the aligned
    points differ from gt by rounding, so their count is at least n_t - 1 (e <= t_0 = 0 may fail): PA AUC >= G[n_t - 1] = 1 - 0.5 / 99"""
    rng = np.random.default_rng(11)
    gt = (rng.normal(size=(2, 778, 3)) * 0.04 + [0, 0, 0.6]).astype(np.float32)
    values, counts = _run(gt[:, None], gt, np.zeros((2, 3)), np.ones(2, bool), counts=True)
    v, c = values.cpu().numpy(), counts.cpu().numpy()
    assert (v[..., 0] == 1.0).all() and (v[..., 2:4] == 1.0).all() and (v[..., 4:6] == 1.0).all()
    assert (v[..., 1] >= 1 - 0.5 / 99 - 1e-12).all() and (v[..., 1] <= 1.0).all()
    assert (c[..., :8] == 778).all() and (c[..., 8] == 778 * 100).all() and (c[..., 9] >= 778 * 99).all()


def test_shifted_lattice_closed_form():
    """a 4 x 4 x 4 lattice of pitch 30 mm, the hypothesis shifted by (6, 8, 0) mm: every nearest neighbour is the point's own copy at
    10 mm (the next one is 22.8 mm away) -> F@5 = 0, F@15 = 1; every raw error is 10 mm -> raw AUC = G[#{t_j >= 0.010}]; a translation is
    aligned away -> the PA values of the identical case"""
    i = np.arange(4) * 0.03
    gt = (np.stack(np.meshgrid(i, i, i, indexing='ij'), -1).reshape(1, 64, 3) + [-0.045, -0.045, 0.6]).astype(np.float32)
    pd = (gt + np.array([0.006, 0.008, 0.0], np.float32)).astype(np.float32)
    for right in (True, False):                                                  # the left hand: x flipped in the model frame
        m = pd.copy()
        if not right:
            m[..., 0] = -m[..., 0]
        values, counts = _run(m[:, None], gt, np.zeros((1, 3)), np.array([right]), counts=True)
        v, c = values.cpu().numpy()[0, 0], counts.cpu().numpy()[0, 0]
        t = HB.thresholds()
        k = int((t >= 0.010).sum())
        assert k == 80 and abs(v[0] - HB.g_table(t)[k]) <= 1e-15 and c[8] == 64 * k
        assert v[2] == 0.0 and v[3] == 1.0 and list(c[:4]) == [0, 64, 0, 64]
        assert v[1] >= 1 - 0.5 / 99 - 1e-12 and v[4] == 1.0 and v[5] == 1.0 and c[9] >= 64 * 99


def test_far_hypothesis_takes_the_zero_branch():
    """every point 0.2 m from every target: no error <= 50 mm, no distance < 15 mm -> raw AUC = 0 and raw F = 0 (p + r = 0), not NaN"""
    pd, gt, root, is_right = HB.synthetic(2, 2, 70, 9)
    pd = pd.copy()
    pd[..., 2] += np.float32(0.2)
    values, counts = _run(pd, gt, root, is_right, counts=True)
    v, c = values.cpu().numpy(), counts.cpu().numpy()
    assert np.isfinite(v).all() and (v[..., 0] == 0.0).all() and (v[..., 2:4] == 0.0).all() and (c[..., :4] == 0).all() and (c[..., 8] == 0).all()


def test_nan_vertex_limits_repeat_runs_and_counts_switch():
    from vpho_amd import ops
    pd, gt, root, is_right = HB.synthetic(3, 5, 70, SEEDS[(3, 5, 70)])
    clean = _run(pd, gt, root, is_right)
    again, counts = _run(pd, gt, root, is_right, counts=True)
    assert _bytes_equal(clean, again) and _bytes_equal(clean, _run(pd, gt, root, is_right))    # counts on / off, two runs
    bad = pd.copy()
    bad[1, 3, 17, 2] = np.nan
    v = _run(bad, gt, root, is_right)
    assert torch.isnan(v[1, 3]).all()
    keep = torch.ones((3, 5), dtype=torch.bool)
    keep[1, 3] = False
    assert _bytes_equal(v[keep], clean[keep])
    bad_gt = gt.copy()
    bad_gt[2, 0, 0] = np.inf                                                    # a ground-truth point: every hypothesis of the image
    v = _run(pd, bad_gt, root, is_right)
    assert torch.isnan(v[2]).all() and _bytes_equal(v[:2], clean[:2])
    with pytest.raises(ops.VphoError, match='1025 points'):
        _run(np.zeros((1, 1, 1025, 3)), np.zeros((1, 1025, 3)), np.zeros((1, 3)), np.ones(1, bool))
    t, g = ops.hand_bench_tables(DEV)
    assert np.array_equal(t.cpu().numpy(), HB.thresholds()) and np.array_equal(g.cpu().numpy(), HB.g_table(HB.thresholds()))


def test_table_kernel_is_the_torch_rule():
    from vpho_amd import ops
    g = torch.Generator().manual_seed(5)
    per = torch.rand((7, 6, 8), generator=g, dtype=torch.float64)
    per[2, 4, 3] = float('nan')
    per[5, 0, 6] = float('nan')                                                 # in hypothesis 0: one, best and mean
    one, best, mean = ops.hand_bench_table(per.to(DEV))
    want_mean = torch.zeros((7, 8), dtype=torch.float64)
    for s in range(6):
        want_mean = want_mean + per[:, s]
    want = (per[:, 0], per.amax(1), want_mean / 6)
    for got, ref in zip((one, best, mean), want):
        assert torch.equal(torch.isnan(got.cpu()), torch.isnan(ref)) and torch.equal(torch.nan_to_num(got.cpu(), nan=-1.0), torch.nan_to_num(ref, nan=-1.0))
    assert torch.isnan(best[2, 3]) and torch.isnan(mean[2, 3]) and not torch.isnan(one[2, 3]) and torch.isnan(one[5, 6])
    ref = HB.table_rule(per.numpy())
    for got, r in zip((one, best, mean), ref):
        np.testing.assert_array_equal(got.cpu().numpy(), r)


def test_blocks_layout_and_the_joint_only_hand_mode():
    """evaluate.hand_bench_block / hand_bench_multi_block on hand-made outputs: agg | reg and one | best | mean in the column order of
    ops_names, against the restatement (fp32 columns: 1e-7); in hand mode 2D_pt_joint the six vertex values of agg are NaN"""
    from vpho_amd import evaluate as E
    from vpho_amd.configs.args import cfg
    pdj, gtj, root, right = HB.synthetic(3, 2, 21, 1)
    pdv, gtv, root_v, right_v = HB.synthetic(3, 2, 70, 1)
    assert np.array_equal(root, root_v) and np.array_equal(right, right_v)       # the same seed draws the same roots first
    vj = HB.bench_multi(pdj, gtj, root, right, with_fscore=False)[0]
    vv, _, band, _ = HB.bench_multi(pdv, gtv, root, right)
    assert band.sum() == 0
    per = np.concatenate([vj[..., :2], vv], -1)                                  # (3, 2, 8)
    pdj, pdv, gtj, gtv, root, right = _dev(pdj, pdv, gtj, gtv, root, right)
    out = {'agg_hand_joint': pdj[:, 0], 'agg_hand_vert': pdv[:, 0], 'reg_hand_joint': pdj[:, 1], 'reg_hand_vert': pdv[:, 1],
           'diff_final_hand_joint': pdj, 'diff_final_hand_vert': pdv}
    data = {'root_joint': root, 'is_right': right}
    want = torch.from_numpy(per.reshape(3, 16)).float()
    saved = cfg.aggregation_mode_hand
    try:
        cfg.aggregation_mode_hand = 'heatmap_cascade'
        blk = E.hand_bench_block(out, data, gtj, gtv)
        cfg.aggregation_mode_hand = '2D_pt_joint'
        joint_only = E.hand_bench_block(out, data, gtj, gtv)
    finally:
        cfg.aggregation_mode_hand = saved
    assert blk.shape == (3, 16) and blk.dtype == torch.float32 and (blk.cpu() - want).abs().max() <= 1e-7
    assert torch.isnan(joint_only[:, 2:8]).all() and torch.equal(joint_only[:, :2], blk[:, :2]) and torch.equal(joint_only[:, 8:], blk[:, 8:])
    multi = E.hand_bench_multi_block(out, data, gtj, gtv)
    want = torch.from_numpy(np.concatenate(HB.table_rule(per), 1)).float()
    assert multi.shape == (3, 24) and multi.dtype == torch.float32 and (multi.cpu() - want).abs().max() <= 1e-7


# ------------------------------------------------------------------------------------------------------------------ end to end
def _eval_cfg():
    from vpho_amd.configs.args import cfg
    keys = tuple(EVAL_ARGS) + ('checkpoint', 'eval_best', 'eval_physics', 'eval_volume', 'eval_hand_bench')
    saved = {k: getattr(cfg, k) for k in keys}
    for k, v in EVAL_ARGS.items():
        setattr(cfg, k, v)
    cfg.checkpoint, cfg.eval_best, cfg.eval_physics, cfg.eval_volume, cfg.eval_hand_bench = None, False, False, False, False
    return cfg, saved


def _table_of(text):
    line = [l for l in text.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, text[-2000:]
    return json.loads(line[0][len('EVAL_JSON '):])['table']


def _by_image(rows):
    idx = rows[:, 0]
    assert len(set(idx.tolist())) == rows.shape[0]
    return rows[idx.argsort()]


def test_trainer_eval_end_to_end(monkeypatch, capsys):
    from vpho_amd import evaluate as E
    from vpho_amd import ops
    from vpho_amd.ops_names import HAND_BENCH_TABLE, MULTI_TABLES
    from vpho_amd.trainer import Trainer
    cfg, saved = _eval_cfg()
    calls = []
    orig = E.hand_bench_multi_block

    def spy(out, data, gt_joint, gt_vert):
        blk = orig(out, data, gt_joint, gt_vert)
        calls.append((out['diff_final_hand_joint'].clone(), out['diff_final_hand_vert'].clone(), data['root_joint'].clone(), data['is_right'].clone(),
                      gt_joint.clone(), gt_vert.clone(), blk.clone()))
        return blk
    try:
        t = Trainer(cfg)
        rng_state = torch.get_rng_state()
        plain = t.eval()
        capsys.readouterr()
        torch.set_rng_state(rng_state)
        wide = t.eval(eval_hand_bench=True)
        text = capsys.readouterr().out
        torch.set_rng_state(rng_state)
        best = t.eval(eval_best=True)
        torch.set_rng_state(rng_state)
        only16 = t.eval(eval_best=True, eval_hand_bench=True)               # the two cfg flags are off: no multi-hypothesis block
        capsys.readouterr()
        monkeypatch.setattr(E, 'hand_bench_multi_block', spy)
        torch.set_rng_state(rng_state)
        multi = t.eval(eval_best=True, eval_hand_bench=True, hand_bench_multi=True)
        text_multi = capsys.readouterr().out
        monkeypatch.undo()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    n = EVAL_ARGS['eval_batch_size'] * EVAL_ARGS['num_batches']
    assert plain.shape == (n, 28) and wide.shape == (n, 44) and best.shape == (n, 88) and only16.shape == (n, 104) and multi.shape == (n, 128)
    plain, wide, best, only16, multi = (_by_image(r) for r in (plain, wide, best, only16, multi))
    i32 = lambda x: x.contiguous().view(torch.int32)
    assert torch.equal(i32(wide[:, :-16]), i32(plain))
    assert torch.equal(i32(only16[:, :-16]), i32(best)) and torch.equal(i32(multi[:, :-40]), i32(best))
    assert torch.equal(i32(only16[:, -16:]), i32(multi[:, -40:-24])) and torch.equal(i32(only16[:, -16:]), i32(wide[:, -16:]))
    blk = wide[:, -16:]
    assert torch.isfinite(blk).all() and (blk >= 0).all() and (blk <= 1).all()
    # batch 0 is its own ground truth: the regression output + root, which is what the postprocess makes of a RIGHT hand
    first = (wide[:, 0] < EVAL_ARGS['eval_batch_size']) & (wide[:, 7] > 0.5)
    assert int(first.sum()) >= 1
    reg = blk[first][:, 8:16]
    assert (reg[:, [0, 2, 4, 5]] == 1.0).all()                              # AUC_J, AUC_V, F@5, F@15 of 'reg'
    table = _table_of(text)
    assert list(table['hand_bench']) == ['agg', 'reg'] and all(tuple(v) == HAND_BENCH_TABLE for v in table['hand_bench'].values())
    assert table['hand_bench'] == E.hand_bench_table(wide[:, -16:].cpu())
    assert {k: v for k, v in table.items() if k != 'hand_bench'} == E.summarize(plain.cpu())
    assert 'hand_bench agg:' in text and 'hand_bench reg:' in text
    # the multi-hypothesis block: one_candidate is the per-pair call on hypothesis 0
    assert len(calls) == EVAL_ARGS['num_batches']
    blocks = []
    for pj, pv, root, right, gj, gv, b in calls:
        assert pv.shape[1] == EVAL_ARGS['sample_num'] and b.shape == (pv.shape[0], 24)
        c = lambda x: x.float().contiguous()
        j0 = ops.hand_bench_multi(c(pj[:, :1]), c(gj), c(root), right, with_fscore=False)
        v0 = ops.hand_bench_multi(c(pv[:, :1]), c(gv), c(root), right)
        assert torch.equal(b[:, :8], torch.cat([j0[:, 0, :2], v0[:, 0]], -1).float())
        assert (b[:, 8:16] >= b[:, :8]).all() and (b[:, 8:16] >= b[:, 16:24]).all()            # best-of-S is the maximum
        blocks.append(b)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    np.testing.assert_array_equal(order(torch.cat(blocks).cpu().numpy()), order(multi[:, -24:].cpu().numpy()))
    table = _table_of(text_multi)
    assert list(table['hand_bench']) == ['agg', 'reg'] + list(MULTI_TABLES)
    assert all(f'hand_bench {s}:' in text_multi for s in ('agg', 'reg') + MULTI_TABLES)
    _SHARED['table'] = table


def test_main_eval_best_eval_hand_bench_prints_five_sources(capsys):
    from vpho_amd.ops_names import HAND_BENCH_TABLE, MULTI_TABLES
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    args = [x for k, v in EVAL_ARGS.items() for x in ('--' + k, str(v))] + ['--eval_best', '--eval_hand_bench']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--mode', 'eval', '--model', 'vpho_net'] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    table = _table_of(r.stdout)
    assert list(table['hand_bench']) == ['agg', 'reg'] + list(MULTI_TABLES) and all(tuple(v) == HAND_BENCH_TABLE for v in table['hand_bench'].values())
    assert all(f'hand_bench {s}:' in r.stdout for s in ('agg', 'reg') + MULTI_TABLES)
    assert all(0.0 <= v <= 1.0 for src in table['hand_bench'].values() for v in src.values())
    if 'table' in _SHARED:                                                     # the same seeds, the same images as the in-process run
        assert table['hand_bench'] == _SHARED['table']['hand_bench']

"""Penetration and contact of every sampled hypothesis on the device (--eval_best with --eval_physics): the pruned multi-hypothesis
kernel against the brute-force single-pose kernel bit for bit, against the float64 restatement (tests/_penetration_fp64.py), its
one | best | mean table, edge cases, and the end-to-end evaluation with both flags.  Inputs: tests/_penetration_multi_inputs.py."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tests._penetration_fp64 as O
import tests._penetration_multi_inputs as I

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = range(len(I.ID_CASES))


@functools.lru_cache(maxsize=None)
def _meter():
    from vpho_amd import ops
    return ops.HandObjectPenetration(I.meshes(), 'cuda')


@functools.lru_cache(maxsize=None)
def _run(which):
    """one launch of each kernel on a case; results on the host"""
    c = I.case(which)
    H = _meter()
    verts, rt = torch.from_numpy(c['verts']).cuda(), torch.from_numpy(c['rt']).cuda()
    n, S, V = verts.shape[:3]
    table, per, sd, inside = H.multi(verts, rt, list(c['ids']), per_vertex=True)
    flat_ids = [i for i in c['ids'] for _ in range(S)]
    per1, sd1, in1 = H(verts.reshape(n * S, V, 3), rt.reshape(n * S, 3, 4), flat_ids, per_vertex=True)
    h = lambda t: t.cpu().numpy()
    return dict(verts=verts, rt=rt, table=h(table), per=h(per), sd=h(sd), inside=h(inside), per1=h(per1), sd1=h(sd1), in1=h(in1))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def table_of(per):
    """the rules of include/vpho_hip.h on per_hyp (n, S, 4): one | best | mean, sums in ascending s"""
    n, S = per.shape[:2]
    out = np.zeros((n, 12))
    out[:, 0:4] = per[:, 0]
    out[:, 4], out[:, 5] = per[:, :, 0].min(1), per[:, :, 1].min(1)
    out[:, 6], out[:, 7] = per[:, :, 2].max(1), per[:, :, 3].max(1)
    acc = np.zeros((n, 4))
    for s in range(S):
        acc = acc + per[:, s]
    out[:, 8:12] = acc / np.float64(S)
    return out


def test_inputs_have_inside_and_outside_points():
    for name, share in I.inside_share().items():
        assert 0.10 <= share <= 0.90, (name, share)


@pytest.mark.parametrize('which', CASES)
def test_bits_of_the_single_pose_kernel(which):
    r = _run(which)
    n, S, V = I.N_IMG, I.S, I.V
    assert r['sd'].shape == (n, S, V) and r['inside'].shape == (n, S, V) and r['per'].shape == (n, S, 4) and r['table'].shape == (n, 12)
    assert np.array_equal(r['inside'].reshape(n * S, V), r['in1'])
    assert np.array_equal(_bits(r['sd']).reshape(n * S, V), _bits(r['sd1']))
    assert np.array_equal(_bits(r['per']).reshape(n * S, 4), _bits(r['per1']))
    assert r['inside'].any() and not r['inside'].all()


@pytest.mark.parametrize('which', CASES)
def test_inside_and_sd_against_the_fp64_restatement(which):
    r, c = _run(which), I.case(which)
    bad = np.nonzero(r['inside'].astype(bool) != c['inside'])
    assert len(bad[0]) == 0, (bad, c['p'][bad][:5])
    np.testing.assert_allclose(r['sd'], np.where(c['inside'], -c['dist'], c['dist']), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(r['per'].reshape(-1, 4), O.reduce(r['sd'].reshape(-1, I.V), r['inside'].reshape(-1, I.V).astype(bool), 0.005))


@pytest.mark.parametrize('which', CASES)
def test_table_is_the_reduction_of_per_hyp_and_runs_repeat(which):
    r = _run(which)
    assert np.array_equal(_bits(r['table']), _bits(table_of(r['per'])))
    # the three reductions differ on these inputs: a table that copied one of them would not pass
    assert not np.array_equal(r['table'][:, 0:4], r['table'][:, 4:8]) and not np.array_equal(r['table'][:, 0:4], r['table'][:, 8:12])
    H = _meter()
    ids = list(I.case(which)['ids'])
    table2, per2 = H.multi(r['verts'], r['rt'], ids)                       # nothing per vertex: the same bits
    assert np.array_equal(_bits(per2.cpu().numpy()), _bits(r['per'])) and np.array_equal(_bits(table2.cpu().numpy()), _bits(r['table']))
    table3, per3, sd3, in3 = H.multi(r['verts'], r['rt'], ids, per_vertex=True)
    assert np.array_equal(_bits(sd3.cpu().numpy()), _bits(r['sd'])) and np.array_equal(in3.cpu().numpy(), r['inside'])
    assert np.array_equal(_bits(per3.cpu().numpy()), _bits(r['per'])) and np.array_equal(_bits(table3.cpu().numpy()), _bits(r['table']))


def test_contact_threshold_and_single_hypothesis():
    r = _run(0)
    H = _meter()
    ids = list(I.case(0)['ids'])
    # S = 1: one, best and mean are the same four values
    v1, rt1 = r['verts'][:, 2:3].contiguous(), r['rt'][:, 2:3].contiguous()
    table, per = H.multi(v1, rt1, ids)
    table, per = table.cpu().numpy(), per.cpu().numpy()
    assert np.array_equal(_bits(per[:, 0]), _bits(r['per'][:, 2]))
    for k in range(3):
        assert np.array_equal(_bits(table[:, 4 * k:4 * k + 4]), _bits(per[:, 0]))
    # the threshold reaches the contact column only
    wide, per_w = H.multi(r['verts'], r['rt'], ids, contact_thresh=10.0)
    assert (per_w[..., 3] == 1).all() and np.array_equal(_bits(per_w[..., :3].cpu().numpy()), _bits(r['per'][..., :3]))
    assert (wide[:, 11] == 1).all()


def test_bad_object_id_empty_batch_and_errors():
    from vpho_amd import ops
    r = _run(1)
    H = _meter()
    ids = I.case(1)['ids']
    dev_bad = torch.tensor([ids[0], 99, ids[2]], dtype=torch.int32, device='cuda')
    table, per, sd, inside = H.multi(r['verts'], r['rt'], dev_bad, per_vertex=True)
    table, per, sd, inside = (t.cpu().numpy() for t in (table, per, sd, inside))
    assert np.isnan(table[1]).all() and np.isnan(per[1]).all() and np.isnan(sd[1]).all() and (inside[1] == 0).all()
    for i in (0, 2):                                                     # the other images: untouched
        assert np.array_equal(_bits(table[i]), _bits(r['table'][i])) and np.array_equal(_bits(per[i]), _bits(r['per'][i]))
        assert np.array_equal(_bits(sd[i]), _bits(r['sd'][i])) and np.array_equal(inside[i], r['inside'][i])
    neg = torch.tensor([-1, ids[1], ids[2]], dtype=torch.int32, device='cuda')
    assert np.isnan(H.multi(r['verts'], r['rt'], neg)[0][0].cpu().numpy()).all()
    with pytest.raises(ops.VphoError, match='outside'):
        H.multi(r['verts'], r['rt'], [0, 1, 3])
    # n = 0 is a no-op
    table, per = H.multi(torch.zeros((0, 5, 70, 3), device='cuda'), torch.zeros((0, 5, 3, 4), dtype=torch.float64, device='cuda'), [])
    assert table.shape == (0, 12) and per.shape == (0, 5, 4)
    with pytest.raises(ops.VphoError, match='GPU'):
        H.multi(r['verts'].cpu(), r['rt'], list(ids))
    bare = ops.HandObjectPenetration({'box': I.meshes()['box']}, 'cuda', accel=False)
    with pytest.raises(ops.VphoError, match='accel'):
        bare.multi(r['verts'][:1], r['rt'][:1], [0])


def test_more_vertices_than_a_workgroup_and_a_nan_vertex():
    """V = 778 (four rounds of a 256-thread workgroup, the last with 10 live lanes) on the box and torus; a NaN vertex is nearest to
    nothing in either kernel (fmin drops the NaN distances: sd = +inf, outside) and no bound may skip on it"""
    H = _meter()
    rng = np.random.default_rng(8)
    n, S, V = 2, 3, 778
    pts = (I.LO + I.EXT * rng.uniform(-0.2, 1.2, size=(n, S, V, 3))).astype(np.float32)
    pts[1, 2, 700] = np.nan
    rt = torch.zeros((n, S, 3, 4), dtype=torch.float64, device='cuda')
    rt[..., :3] = torch.eye(3, dtype=torch.float64)
    verts = torch.from_numpy(pts).cuda()
    table, per, sd, inside = H.multi(verts, rt, [0, 1], per_vertex=True)
    per1, sd1, in1 = H(verts.reshape(n * S, V, 3), rt.reshape(n * S, 3, 4), [0, 0, 0, 1, 1, 1], per_vertex=True)
    assert np.array_equal(_bits(sd.cpu().numpy()).reshape(n * S, V), _bits(sd1.cpu().numpy())) and torch.equal(inside.reshape(n * S, V), in1)
    assert np.array_equal(_bits(per.cpu().numpy()).reshape(n * S, 4), _bits(per1.cpu().numpy()))
    per, table = per.cpu().numpy(), table.cpu().numpy()
    assert np.isposinf(sd.cpu().numpy()[1, 2, 700]) and np.isfinite(per).all()
    assert np.array_equal(_bits(table), _bits(table_of(per)))
    assert inside.sum() > 500


# ------------------------------------------------------------------------------------------------------------ end to end
def _eval_cfg():
    from vpho_amd.configs.args import cfg
    keys = ('sample_num', 'sampling_steps', 'topk_hand', 'topk_obj', 'sample_T0', 'eval_batch_size', 'num_batches', 'random_seed', 'checkpoint',
            'eval_best', 'eval_physics')
    saved = {k: getattr(cfg, k) for k in keys}
    cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 4, 5, 4, 3, 0.2
    cfg.eval_batch_size, cfg.num_batches, cfg.random_seed, cfg.checkpoint, cfg.eval_best, cfg.eval_physics = 2, 2, 7, None, False, False
    return cfg, saved


def test_trainer_eval_with_both_flags(monkeypatch, capsys):
    from vpho_amd import evaluate as E
    from vpho_amd import ops
    from vpho_amd.trainer import Trainer
    cfg, saved = _eval_cfg()
    seen, right = [], []
    orig_rows = E.metric_rows

    def spy(out, data, gt_joint, gt_vert, first, assets=None, *a, **k):
        rows = orig_rows(out, data, gt_joint, gt_vert, first, assets, *a, **k)
        if k['layout'].has('physics_multi'):
            # the same outputs through the row builder with the new block switched off: the rows of this tree before the feature
            without = orig_rows(out, data, gt_joint, gt_vert, first, assets,
                                layout=E.RowLayout.resolve(eval_best=True, eval_physics=True, physics_multi=False))
            meter = E.physics_meter(assets, rows.device)
            S = out['diff_final_hand_vert'].shape[1]
            # hypothesis 0 in the camera frame, written out (postprocess' arithmetic, not the helper the block itself uses):
            # x negated for left hands, then + root joint
            v0 = out['diff_final_hand_vert'][:, 0].float().clone()
            v0[..., 0] = v0[..., 0] * torch.where(data['is_right'].bool(), 1.0, -1.0).to(v0)[:, None]
            v0 = (v0 + data['root_joint'].float()[:, None]).contiguous()
            right.extend(bool(x) for x in data['is_right'].cpu())
            rt0 = ops.obj_9d_to_rt(out['diff_final_obj_6d'][:, 0].double().contiguous(), data['root_joint'].float().contiguous())
            seen.append((rows.clone(), without.clone(), meter(v0, rt0, meter.obj_ids(data['obj_name']), float(cfg.physics_contact_thresh)).clone(), S))
        return rows
    try:
        t = Trainer(cfg)
        monkeypatch.setattr(E, 'metric_rows', spy)
        torch.manual_seed(11)
        both = t.eval(eval_best=True, eval_physics=True, physics_multi=True)
        text_both = capsys.readouterr().out
        monkeypatch.setattr(E, 'metric_rows', orig_rows)

        def boom(*a, **k):
            raise AssertionError('HandObjectPenetration.multi called without both flags')
        monkeypatch.setattr(ops.HandObjectPenetration, 'multi', boom)
        monkeypatch.setattr(ops.HandObjectPenetration, 'build_accel', boom)
        torch.manual_seed(11)
        only_best = t.eval(eval_best=True)
        text_best = capsys.readouterr().out
        torch.manual_seed(11)
        only_phys = t.eval(eval_physics=True)
        text_phys = capsys.readouterr().out
        # a caller that passes the two older flags itself, with neither set on the command line, gets the rows it always got
        torch.manual_seed(11)
        both_args = t.eval(eval_best=True, eval_physics=True)
        text_args = capsys.readouterr().out
        monkeypatch.undo()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    assert both.shape == (4, 108) and only_best.shape == (4, 88) and only_phys.shape == (4, 36)
    assert torch.isfinite(both).all()
    assert len(seen) == 2
    assert not all(right) and any(right), right                                     # the un-flip of a left hand is exercised
    for rows, without, single0, S in seen:
        assert S == 4 and rows.shape == (2, 108) and without.shape == (2, 96)
        assert torch.equal(rows[:, :96].view(torch.int32), without.view(torch.int32))
        assert torch.equal(rows[:, 96:100], single0.float())                       # one_candidate: the single-pose kernel on hypothesis 0
        blk = rows[:, 96:].double()
        assert (blk[:, 4] <= blk[:, 0]).all() and (blk[:, 5] <= blk[:, 1]).all() and (blk[:, 6] >= blk[:, 2]).all() and (blk[:, 7] >= blk[:, 3]).all()
        assert (blk[:, 4] <= blk[:, 8] + 1e-9).all() and (blk[:, 6] >= blk[:, 10] - 1e-9).all() and ((0 <= blk[:, 11]) & (blk[:, 11] <= 1)).all()
    tab = lambda text: json.loads([l for l in text.splitlines() if l.startswith('EVAL_JSON ')][-1][len('EVAL_JSON '):])['table']
    from vpho_amd.ops_names import PHYSICS_TABLE
    phys = tab(text_both)['physics']
    assert set(phys) == {'pred', 'gt', 'one_candidate', 'best_of_S', 'mean_of_S'}
    assert all(tuple(v) == PHYSICS_TABLE for v in phys.values())
    for name in ('one_candidate', 'best_of_S', 'mean_of_S'):
        assert f'physics {name}:' in text_both
    # with one flag only: widths, keys and printed blocks as before
    assert 'physics' not in tab(text_best) and 'best_of_S' in tab(text_best) and 'physics pred:' not in text_best
    assert set(tab(text_phys)['physics']) == {'pred', 'gt'} and 'best_of_S' not in tab(text_phys) and 'physics best_of_S' not in text_phys
    # the shared columns do not depend on the flags (same seed)
    assert both_args.shape == (4, 96) and torch.equal(both_args, both[:, :96]) and set(tab(text_args)['physics']) == {'pred', 'gt'}
    assert torch.equal(both[:, :88], only_best) and torch.equal(both[:, 88:96], only_phys[:, 28:])


def test_main_eval_with_both_flags_prints_the_tables():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    args = ['--sample_num', '4', '--sampling_steps', '5', '--topk_hand', '8', '--topk_obj', '3', '--sample_T0', '0.2',
            '--eval_batch_size', '2', '--num_batches', '2', '--random_seed', '7', '--eval_best', '--eval_physics']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--mode', 'eval', '--model', 'vpho_net'] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, r.stdout[-2000:]
    res = json.loads(line[0][len('EVAL_JSON '):])
    from vpho_amd.ops_names import PHYSICS_TABLE
    assert res['images'] == 4
    assert set(res['table']['physics']) == {'pred', 'gt', 'one_candidate', 'best_of_S', 'mean_of_S'}
    assert all(tuple(v) == PHYSICS_TABLE for v in res['table']['physics'].values())
    assert 'physics best_of_S:' in r.stdout and 'physics mean_of_S:' in r.stdout and 'physics one_candidate:' in r.stdout

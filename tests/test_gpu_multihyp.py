"""Multi-hypothesis evaluation (--eval_best): the per-hypothesis hand / object kernels against the reference's own TesterHand /
TesterObject (golden_multihyp.npz), against a float64 brute force, against the single-hypothesis kernels, and end to end."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_multihyp.npz'))
TH = (0.002, 0.005, 0.010, 0.020, 0.050, 0.100)


def _cols():
    from vpho_amd.ops_names import OBJ_METRIC_NAMES
    return {k: i for i, k in enumerate(OBJ_METRIC_NAMES)}, OBJ_METRIC_NAMES


def _check_obj(got, ref, nn_atol, f_atol):
    """tests/test_gpu_metrics.py::_check_obj's tolerances, on (rows, 16)"""
    col, names = _cols()
    for k in ('MCE', 'OCE', 'REP'):
        np.testing.assert_allclose(got[:, col[k]], ref[:, col[k]], rtol=1e-6, err_msg=k)
    for k in ('MCE2', 'ADD'):
        np.testing.assert_allclose(got[:, col[k]], ref[:, col[k]], rtol=5e-6, err_msg=k)
    for k in ('ADDS', 'CD'):
        np.testing.assert_allclose(got[:, col[k]], ref[:, col[k]], atol=nn_atol, rtol=2e-6, err_msg=k)
    for k in ('ADD01d', 'ADDS01d', 'REP5'):
        np.testing.assert_array_equal(got[:, col[k]], ref[:, col[k]], err_msg=k)
    for k in names[10:]:
        np.testing.assert_allclose(got[:, col[k]], ref[:, col[k]], atol=f_atol, err_msg=k)


def _d(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def test_hand_multi_matches_tester_hand_fixture():
    from vpho_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    root, right = t(G['root_joint']), t(G['is_right'])
    mje, pa = ops.hand_metrics_multi(t(G['pd_joint_model']), t(G['gt_joint']), root, right)
    mve, pav = ops.hand_metrics_multi(t(G['pd_vert_model']), t(G['gt_vert']), root, right)
    got = torch.stack([mje, pa, mve, pav], -1).cpu().numpy()
    np.testing.assert_allclose(got[..., [0, 2]], G['hand'][..., [0, 2]], rtol=1e-5)
    np.testing.assert_allclose(got[..., [1, 3]], G['hand'][..., [1, 3]], rtol=2e-5)


def test_object_multi_matches_tester_object_fixture(assets):
    from vpho_amd import ops
    col, names = _cols()
    M = ops.ObjectMetrics(assets['ycb'], 'cuda')
    N, S = G['pd_rt'].shape[:2]
    per, best, mean = M.multi(_d(G['pd_rt']), _d(G['gt_rt']), _d(G['cam_intr']), _d(G['obj_idx'], torch.int32))
    per, best, mean = per.cpu().numpy(), best.cpu().numpy(), mean.cpu().numpy()
    assert np.isfinite(per).all()
    # the candidate equal to the ground truth (image 0, candidate 3): the reference's torch.cdist expansion leaves sqrt(rounding),
    # ~3e-5 m, in ADD-S / CD at camera-space magnitudes, where the direct form gives 0 (checked below)
    ref = G['obj'].copy()
    assert 0 < ref[0, 3, col['ADDS']] < 1e-4
    ref[0, 3, [col['ADDS'], col['CD']]] = per[0, 3, [col['ADDS'], col['CD']]]
    _check_obj(per.reshape(N * S, 16), ref.reshape(N * S, 16), nn_atol=2e-5, f_atol=3e-3)
    # the reductions are exactly the min / max / mean of the per-candidate values
    is_max = np.array([k in ('ADD01d', 'ADDS01d', 'REP5') or k.startswith('FSCORE@') for k in names])
    np.testing.assert_array_equal(best, np.where(is_max, per.max(1), per.min(1)))
    np.testing.assert_allclose(mean, per.mean(1), rtol=1e-14, atol=1e-300)
    # TesterObject.postprocess (test.py:522-582): mean over images of the best candidate, truncated to 0.01 in its units
    for k, v in zip(G['post_names'], G['post_table']):
        k = str(k)
        scale = 1000.0 if k in ('MCE', 'OCE', 'MCE2', 'ADD', 'ADDS', 'CD') else (1.0 if k == 'REP' else 100.0)
        ours = best[:, col[k]].mean() * scale
        tol = 0.3 if k.startswith('FSCORE@') else 0.02 if k in ('ADDS', 'CD') else 1e-6 * max(1.0, abs(v))   # the NN tolerances above
        assert v - tol <= ours < v + 0.01 + tol, (k, ours, v)
    # the candidate equal to the ground truth
    same = per[0, 3]
    for k in ('MCE', 'OCE', 'MCE2', 'ADD'):
        assert same[col[k]] == 0.0, k
    for k in ('ADDS', 'CD'):
        assert same[col[k]] <= 1e-9, k


def _ragged_tables(assets):
    """ragged vertex counts in one batch: 777 and 300 vertices, and one object of 4500 (more than an LDS tile and a query chunk)"""
    ycb = {k: dict(v) for k, v in assets['ycb'].items()}
    names = list(ycb.keys())
    rng = np.random.default_rng(5)
    ycb[names[1]]['verts'] = ycb[names[1]]['verts'][:777]
    ycb[names[2]]['verts'] = ycb[names[2]]['verts'][:300]
    v = np.asarray(ycb[names[3]]['verts'], np.float64)
    extra = v[rng.integers(0, v.shape[0], 4500 - v.shape[0])] + rng.normal(size=(4500 - v.shape[0], 3)) * 0.003
    ycb[names[3]]['verts'] = np.concatenate([v, extra]).astype(np.float32)
    return ycb


def _poses(n, S, rng, n_obj):
    from oracle import rotations as R
    gR = R.axis_angle_to_matrix(torch.from_numpy(rng.normal(size=(n, 3)))).numpy()
    gt = np.concatenate([gR, (rng.normal(size=(n, 3)) * 0.05 + np.array([0, 0, 0.7]))[:, :, None]], -1)
    sc = rng.uniform(0.0, 0.3, size=(n, S, 1))
    dR = R.axis_angle_to_matrix(torch.from_numpy(rng.normal(size=(n * S, 3)) * sc.reshape(-1, 1))).numpy().reshape(n, S, 3, 3)
    pd = np.zeros((n, S, 3, 4))
    pd[..., :3] = dR @ gt[:, None, :, :3]
    pd[..., 3] = gt[:, None, :, 3] + rng.normal(size=(n, S, 3)) * sc * 0.1
    cam = np.tile(np.array([[500.0, 0, 128], [0, 500.0, 128], [0, 0, 1]]), (n, 1, 1))
    oid = rng.integers(0, n_obj, size=n)
    return pd, gt, cam, oid


def _nn64(q, y):
    """float64 brute-force nearest distances (direct differences)"""
    return torch.cdist(torch.from_numpy(q)[None], torch.from_numpy(y)[None], compute_mode='donot_use_mm_for_euclid_dist')[0].min(-1).values.numpy()


def _check_vs_f64(ycb, names, pd, gt, oid, per, picks):
    col, _ = _cols()
    for b, s in picks:
        e = ycb[names[oid[b]]]
        vs, vf = np.asarray(e['verts_sampled'], np.float64), np.asarray(e['verts'], np.float64)
        tr = lambda rt, v: v @ rt[:, :3].T + rt[:, 3]
        ps, gs, pf, gf = tr(pd[b, s], vs), tr(gt[b], vs), tr(pd[b, s], vf), tr(gt[b], vf)
        adds = _nn64(ps, gs).mean()
        dp, dg = _nn64(pf, gf), _nn64(gf, pf)
        assert abs(per[b, s, col['ADDS']] - adds) <= 1e-6, (b, s)
        assert abs(per[b, s, col['CD']] - 0.5 * (dp.mean() + dg.mean())) <= 1e-6, (b, s)
        for k, th in enumerate(TH):
            if (np.abs(dp - th) <= 1e-6).any() or (np.abs(dg - th) <= 1e-6).any():
                continue                      # a point within 1e-6 m of the threshold may fall on either side in fp32
            prec, rec = np.float32((dp < th).sum() / len(vf)), np.float32((dg < th).sum() / len(vf))
            f = np.float32(np.float32(2.0) * prec * rec) / np.float32(np.float32(prec + rec) + np.float32(1e-6))
            assert per[b, s, 10 + k] == float(f), (b, s, th, per[b, s, 10 + k], float(f))


def test_object_multi_against_float64_brute_force(assets):
    """A seeded 64 x 100 batch over objects of 2048, 777, 300 and 4500 full vertices; ADD-S and CD within 1e-6 m of float64 brute
    force, F-scores equal (points within 1e-6 m of a threshold aside); identity candidates give ADD = 0 and F = 2 / (2 + 1e-6) in fp32."""
    from vpho_amd import ops
    col, _ = _cols()
    ycb = _ragged_tables(assets)
    names = list(ycb.keys())
    M = ops.ObjectMetrics(ycb, 'cuda')
    rng = np.random.default_rng(64)
    n, S = 64, 100
    pd, gt, cam, oid = _poses(n, S, rng, 5)
    oid[:8] = [0, 1, 2, 3, 4, 3, 2, 1]
    pd[np.arange(n), rng.integers(0, S, n)] = gt              # one candidate per image equal to the ground truth
    eq = np.all(pd == gt[:, None], axis=(2, 3))
    per, best, mean = M.multi(_d(pd), _d(gt), _d(cam), _d(oid, torch.int32))
    per = per.cpu().numpy()
    assert np.isfinite(per).all()
    ids = per[eq]
    assert (ids[:, col['ADD']] == 0.0).all() and (ids[:, [col['MCE'], col['OCE'], col['MCE2']]] == 0.0).all()
    assert (ids[:, col['ADDS']] <= 1e-9).all() and (ids[:, col['CD']] <= 1e-9).all()
    f1 = float(np.float32(2.0) / (np.float32(2.0) + np.float32(1e-6)))
    assert (ids[:, 10:] == f1).all() and (ids[:, [col['ADD01d'], col['ADDS01d'], col['REP5']]] == 1.0).all()
    picks = [(b, int(rng.integers(0, S))) for b in range(8)] + [(b, int(np.nonzero(eq[b])[0][0])) for b in range(3)]
    _check_vs_f64(ycb, names, pd, gt, oid, per, picks)


def test_object_multi_small_and_odd_sizes_agree_with_single_hypothesis_kernel(assets):
    """S = 1 and an n_img * S that is no multiple of any tile: every candidate agrees with ObjectMetrics on the same pose (the
    flattened path), within the fixture tolerances; two runs are bitwise identical."""
    from vpho_amd import ops
    ycb = _ragged_tables(assets)
    M = ops.ObjectMetrics(ycb, 'cuda')
    rng = np.random.default_rng(9)
    for n, S in ((5, 1), (3, 7)):
        pd, gt, cam, oid = _poses(n, S, rng, 5)
        oid[:3] = [3, 1, 2]
        args = (_d(pd), _d(gt), _d(cam), _d(oid, torch.int32))
        per, best, mean = M.multi(*args)
        flat = M(_d(pd.reshape(n * S, 3, 4)), _d(np.repeat(gt, S, 0)), _d(np.repeat(cam, S, 0)), _d(np.repeat(oid, S), torch.int32))
        _check_obj(per.cpu().numpy().reshape(n * S, 16), flat.cpu().numpy(), nn_atol=1e-6, f_atol=3e-3)
        again = M.multi(*args)
        for x, y in zip((per, best, mean), again):
            assert torch.equal(x, y)
        if S == 1:
            assert torch.equal(best, per[:, 0]) and torch.equal(mean, per[:, 0])


def test_hand_multi_agrees_with_single_kernel_on_postprocessed_candidates():
    from vpho_amd import ops
    rng = np.random.default_rng(21)
    n, S = 5, 9
    right = torch.tensor([True, False, False, True, False]).cuda()
    root = torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32) * 0.1).cuda()
    for P in (21, 778):
        gt = torch.from_numpy(rng.normal(size=(n, P, 3)).astype(np.float32) * 0.05).cuda() + root[:, None]
        pd = torch.from_numpy(rng.normal(size=(n, S, P, 3)).astype(np.float32) * 0.05).cuda()
        me, pa = ops.hand_metrics_multi(pd, gt, root, right)
        post = pd.clone()
        post[..., 0] = post[..., 0] * torch.where(right, 1.0, -1.0)[:, None, None]
        post = post + root[:, None, None]
        for s in (0, 4, S - 1):
            m1, p1 = ops.hand_metrics(post[:, s].contiguous(), gt)
            torch.testing.assert_close(me[:, s], m1, rtol=2e-5, atol=0)
            torch.testing.assert_close(pa[:, s], p1, rtol=2e-5, atol=0)
        me2, pa2 = ops.hand_metrics_multi(pd, gt, root, right)
        assert torch.equal(me, me2) and torch.equal(pa, pa2)


def test_trainer_eval_best_end_to_end(assets, capsys):
    """Trainer.eval with and without eval_best on the same seeded synthetic batches: columns 0-27 bitwise identical; per image
    best-of-S <= one_candidate and best-of-S <= mean-of-S for every distance; one_candidate MJE = column 2; EVAL_JSON carries
    the three tables."""
    from vpho_amd import evaluate as E
    from vpho_amd.configs.args import cfg
    from vpho_amd.ops_names import OBJ_METRIC_NAMES
    from vpho_amd.trainer import Trainer
    keys = ('sample_num', 'sampling_steps', 'topk_hand', 'topk_obj', 'sample_T0', 'eval_batch_size', 'num_batches', 'random_seed', 'checkpoint',
            'eval_best')
    saved = {k: getattr(cfg, k) for k in keys}
    cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 6, 5, 4, 3, 0.2
    cfg.eval_batch_size, cfg.num_batches, cfg.random_seed, cfg.checkpoint, cfg.eval_best = 3, 2, 7, None, False
    try:
        t = Trainer(cfg)
        torch.manual_seed(11)
        plain = t.eval()
        capsys.readouterr()
        torch.manual_seed(11)
        wide = t.eval(eval_best=True)
        text = capsys.readouterr().out
        cfg.eval_best = True
        torch.manual_seed(11)
        by_cfg = t.eval()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    assert plain.shape == (6, E.ROW) and wide.shape == (6, E.ROW_BEST)
    assert torch.equal(wide[:, :E.ROW], plain) and torch.equal(by_cfg, wide)
    w = wide.cpu().double().numpy()
    assert np.isfinite(w).all()
    hand = w[:, E.ROW:E.ROW + 12].reshape(-1, 3, 4)
    obj = w[:, E.ROW + 12:].reshape(-1, 3, 16)
    np.testing.assert_allclose(hand[:, 0, 0], w[:, 2], rtol=1e-5)
    assert (hand[:, 1] <= hand[:, 0]).all() and (hand[:, 1] <= hand[:, 2] * (1 + 1e-6)).all()
    dist = [i for i, k in enumerate(OBJ_METRIC_NAMES) if k in ('MCE', 'OCE', 'MCE2', 'ADD', 'ADDS', 'REP', 'CD')]
    assert (obj[:, 1, dist] <= obj[:, 0, dist]).all() and (obj[:, 1, dist] <= obj[:, 2, dist] * (1 + 1e-6)).all()
    line = [l for l in text.splitlines() if l.startswith('EVAL_JSON ')][-1]
    table = json.loads(line[len('EVAL_JSON '):])['table']
    for name in ('one_candidate', 'best_of_S', 'mean_of_S'):
        assert set(table[name]) == {'hand', 'object'} and set(table[name]['object']) == set(OBJ_METRIC_NAMES)
    assert table['best_of_S']['hand']['MJE'] <= table['one_candidate']['hand']['MJE']

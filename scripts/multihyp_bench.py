"""Timing of the multi-hypothesis evaluation (--eval_best) at 64 images x S = 100 with the synthetic tables, interleaved on one box:
(a) the flattened path -- the single-hypothesis ObjectMetrics / hand_metrics on bs*S rows, ground truth repeated, candidates
postprocessed into a copy; (b) the multi-hypothesis kernels on the same inputs; the whole metric block of evaluate
(multi_hypothesis_block); Trainer.eval images/s with and without eval_best.  Prints one JSON line.
``python scripts/multihyp_bench.py [--reps 10] [--no-eval]``"""
import argparse
import json
import os
import statistics
import sys
import time

sys.argv, _argv = sys.argv[:1], sys.argv[1:]
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--bs', type=int, default=64)
    p.add_argument('--S', type=int, default=100)
    p.add_argument('--no-eval', action='store_true')
    a = p.parse_args(_argv)
    from vpho_amd import evaluate as E, ops
    from vpho_amd.assets import synthetic_assets
    from oracle import rotations as R
    assets = synthetic_assets(0)
    bs, S, dev = a.bs, a.S, 'cuda'
    rng = np.random.default_rng(0)
    M = ops.ObjectMetrics(assets['ycb'], dev)
    gR = R.axis_angle_to_matrix(torch.from_numpy(rng.normal(size=(bs, 3)))).numpy()
    gt = np.concatenate([gR, (rng.normal(size=(bs, 3)) * 0.05 + np.array([0, 0, 0.7]))[:, :, None]], -1)
    dR = R.axis_angle_to_matrix(torch.from_numpy(rng.normal(size=(bs * S, 3)) * 0.1)).numpy().reshape(bs, S, 3, 3)
    pd = np.zeros((bs, S, 3, 4))
    pd[..., :3] = dR @ gt[:, None, :, :3]
    pd[..., 3] = gt[:, None, :, 3] + rng.normal(size=(bs, S, 3)) * 0.01
    d = lambda x, t=torch.float64: torch.from_numpy(np.ascontiguousarray(x)).to(t).to(dev)
    pd_rt, gt_rt = d(pd), d(gt)
    cam = d(np.tile(np.array([[500.0, 0, 128], [0, 500.0, 128], [0, 0, 1]]), (bs, 1, 1)))
    oid = d(rng.integers(0, len(M.names), bs), torch.int32)
    root = d(rng.normal(size=(bs, 3)) * 0.05, torch.float32)
    right = torch.from_numpy(rng.random(bs) < 0.5).to(dev)
    hj = d(rng.normal(size=(bs, S, 21, 3)) * 0.05, torch.float32)
    hv = d(rng.normal(size=(bs, S, 778, 3)) * 0.05, torch.float32)
    gj = d(rng.normal(size=(bs, 21, 3)) * 0.05, torch.float32)
    gv = d(rng.normal(size=(bs, 778, 3)) * 0.05, torch.float32)

    def flat_obj():
        M(pd_rt.view(bs * S, 3, 4), gt_rt.repeat_interleave(S, 0), cam.repeat_interleave(S, 0), oid.repeat_interleave(S, 0))

    def multi_obj():
        M.multi(pd_rt, gt_rt, cam, oid)

    def post(x):
        y = x.clone()
        y[..., 0] = y[..., 0] * torch.where(right, 1.0, -1.0)[:, None, None]
        return (y + root[:, None, None]).reshape(bs * S, x.shape[2], 3)

    def flat_hand():
        ops.hand_metrics(post(hj), gj.repeat_interleave(S, 0))
        ops.hand_metrics(post(hv), gv.repeat_interleave(S, 0))

    def multi_hand():
        ops.hand_metrics_multi(hj, gj, root, right)
        ops.hand_metrics_multi(hv, gv, root, right)

    x9 = torch.cat([pd_rt[..., :2, :3].reshape(bs, S, 6), (pd_rt[..., 3] - root[:, None].double())], -1).float()
    out = {'diff_final_hand_joint': hj, 'diff_final_hand_vert': hv, 'diff_final_obj_6d': x9}
    data = {'root_joint': root, 'is_right': right, 'gt_obj_rt': gt_rt, 'cam_intr': cam, 'obj_name': [M.names[i] for i in oid.tolist()]}

    def block():
        E.multi_hypothesis_block(out, data, gj, gv, assets)

    legs = dict(flat_obj=flat_obj, multi_obj=multi_obj, flat_hand=flat_hand, multi_hand=multi_hand, eval_best_block=block)
    for f in legs.values():                         # warm-up: tables, allocator
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(a.reps):                         # interleaved
        for k, f in legs.items():
            ts[k] += _ms(f, 1)
    res = {k: round(statistics.median(v), 3) for k, v in ts.items()}
    res['obj_speedup'] = round(res['flat_obj'] / res['multi_obj'], 2)
    res['hand_speedup'] = round(res['flat_hand'] / res['multi_hand'], 2)
    nf = int(M.vert_offset[1] - M.vert_offset[0])
    pairs = bs * S * (M.verts_sampled.shape[1] ** 2 + 2 * nf * nf)
    res['obj_nn_pairs'] = pairs
    res['obj_multi_gpairs_per_s'] = round(pairs / res['multi_obj'] / 1e6, 1)
    if not a.no_eval:
        from vpho_amd.configs.args import cfg
        from vpho_amd.trainer import Trainer
        cfg.sample_num, cfg.eval_batch_size, cfg.num_batches, cfg.checkpoint = S, bs, 3, None
        t = Trainer(cfg)
        t.eval(eval_best=False)                     # warm-up
        for flag in (False, True, False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = t.eval(eval_best=flag)
            torch.cuda.synchronize()
            res.setdefault('eval_images_per_s_' + ('best' if flag else 'plain'), []).append(round(rows.shape[0] / (time.perf_counter() - t0), 1))
    res.update(bs=bs, S=S, reps=a.reps)
    print('MULTIHYP_BENCH ' + json.dumps(res))


if __name__ == '__main__':
    main()

"""Timing of the symmetry-aware object errors (--eval_best with --eval_symmetric) at the README configuration: the two launches of
``ops.ObjectSymmetry.multi`` (vpho_obj_symmetry_multi_f64 + vpho_obj_symmetry_table_f64) on 64 images x 50 hypotheses with a table of
K = 628 transforms (a continuous axis at step 0.01 and one discrete symmetry) and 2048 sampled vertices, pruned and unpruned.  One process,
the two forms interleaved, HIP events around the launch pair: 5 warm-ups, then the median of ``--reps`` passes with min and max.  The poses
are ground truths turned by a random angle about the symmetry axis (which the metric must forgive) plus pose noise of three sizes, so the
pruning bound is small for some hypotheses and large for others.  Both forms must return the same bits.  Prints one OBJ_SYMMETRY_BENCH
JSON line.
``python scripts/obj_symmetry_bench.py [--reps 50] [--bs 64] [--samples 50] [--step 0.01] [--verts 2048]``"""
import argparse
import json
import os
import statistics
import sys

sys.argv, _argv = sys.argv[:1], sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _rot(axis, angle):
    from vpho_amd.symmetry import axis_rotation
    return axis_rotation(angle, axis)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--bs', type=int, default=64)
    ap.add_argument('--samples', type=int, default=50)
    ap.add_argument('--step', type=float, default=0.01)
    ap.add_argument('--verts', type=int, default=2048)
    a = ap.parse_args(_argv)
    from vpho_amd import ops, symmetry as SY
    from vpho_amd.assets import YCB_NAMES, synthetic_assets
    n, S = a.bs, a.samples
    y = synthetic_assets(0)['ycb']
    ycb = {k: dict(bbox3d=v['bbox3d'], verts_sampled=np.asarray(v['verts_sampled'])[:a.verts], diameter=v['diameter']) for k, v in y.items()}
    half_y = [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
    infos = {str(i + 1): {'symmetries_continuous': [{'axis': [0, 0, 1], 'offset': [0, 0, 0]}], 'symmetries_discrete': [half_y]} for i in range(len(YCB_NAMES))}
    table = SY.symmetry_table(infos, YCB_NAMES, a.step)
    rng = np.random.default_rng(0)
    ids = rng.integers(0, len(YCB_NAMES), size=n)
    gt = np.zeros((n, 3, 4))
    pd = np.zeros((n, S, 3, 4))
    noise = np.array([0.002, 0.02, 0.2])
    for b in range(n):
        v = rng.normal(size=3)
        gt[b, :, :3] = _rot(v, rng.uniform(0, np.pi))
        gt[b, :, 3] = rng.normal(size=3) * 0.05 + [0, 0, 0.7]
        for s in range(S):
            w = rng.normal(size=3)
            pd[b, s, :, :3] = _rot(w, noise[s % 3] * rng.uniform(0.5, 1.5)) @ gt[b, :, :3] @ _rot([0, 0, 1], rng.uniform(0, 2 * np.pi))
            pd[b, s, :, 3] = gt[b, :, 3] + rng.normal(size=3) * noise[s % 3] * 0.1
    dev = 'cuda'
    pd_d, gt_d = torch.from_numpy(pd).to(dev), torch.from_numpy(gt).to(dev)
    ids_d = torch.from_numpy(ids.astype(np.int32)).to(dev)
    m = ops.ObjectSymmetry(ycb, table, dev)
    legs = dict(pruned=lambda: m.multi(pd_d, gt_d, ids_d, prune=True), unpruned=lambda: m.multi(pd_d, gt_d, ids_d, prune=False))
    outs = {k: fn() for k, fn in legs.items()}
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int64), z.view(torch.int64)) for x, z in zip(outs['pruned'], outs['unpruned']))
    for _ in range(5):
        for fn in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            ts[k].append(_ms(fn))
    per = outs['pruned'][0]
    pairs = float(n) * S * m.K * a.verts
    res = dict(n=n, S=S, K=m.K, verts=a.verts, reps=a.reps, point_evaluations=pairs, same_bits=bool(same),
               mean_SMCE_m=float(per[..., 0].mean()), mean_MSSD_m=float(per[..., 1].mean()), hit_share=float(per[..., 2].mean()))
    for k, v in ts.items():
        med = statistics.median(v)
        res[k] = dict(median_ms=round(med, 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), gpoints_per_s=round(pairs / med / 1e6, 1))
    res['unpruned_over_pruned'] = round(res['unpruned']['median_ms'] / res['pruned']['median_ms'], 2)
    print('OBJ_SYMMETRY_BENCH ' + json.dumps(res))
    if not same:
        sys.exit('obj_symmetry_bench: the pruned and the unpruned form differ')


if __name__ == '__main__':
    main()

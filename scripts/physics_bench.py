"""Timing of the penetration metric (--eval_physics) at 64 images with HIP events, interleaved: the kernel pair on the synthetic box
meshes (3 072 triangles) and on a 20 480-triangle icosphere, with 778 hand vertices per image; the whole physics block of evaluate
(two calls: predicted and ground-truth pairs); Trainer.eval images/s with and without eval_physics.  Prints one JSON line.
``python scripts/physics_bench.py [--reps 10] [--no-eval]``"""
import argparse
import json
import os
import statistics
import sys
import time

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


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--bs', type=int, default=64)
    p.add_argument('--no-eval', action='store_true')
    a = p.parse_args(_argv)
    from vpho_amd import evaluate as E, ops
    from vpho_amd.assets import synthetic_assets
    from vpho_amd.physics_eval import object_meshes
    from tests.test_gpu_penetration import icosphere
    assets = synthetic_assets(0)
    bs, dev = a.bs, 'cuda'
    rng = np.random.default_rng(0)
    boxes = ops.HandObjectPenetration(object_meshes(assets), dev)
    v, f = icosphere(5)
    ico = ops.HandObjectPenetration({n: dict(verts=v * 0.06, faces=f) for n in assets['ycb']}, dev)
    rt = torch.zeros((bs, 3, 4), dtype=torch.float64, device=dev)
    rt[:, :, :3] = torch.eye(3, dtype=torch.float64)
    rt[:, 2, 3] = 0.6
    # hands around the object: a third of the vertices inside, the rest within 5 cm
    hand = torch.from_numpy((rng.normal(size=(bs, 778, 3)) * 0.04 + np.array([0, 0, 0.6])).astype(np.float32)).to(dev)
    oid = boxes.obj_ids([boxes.names[i] for i in rng.integers(0, len(boxes.names), bs)])
    legs = dict(kernels_3072=lambda: boxes(hand, rt, oid), kernels_20480=lambda: ico(hand, rt, oid))
    pp = {'agg_hand_vert': hand}
    x9 = torch.cat([rt[:, :2, :3].reshape(bs, 6), rt[:, :, 3]], -1).float()
    out = {'agg_obj_6d': x9}
    data = {'root_joint': torch.zeros((bs, 3), device=dev), 'gt_obj_rt': rt, 'obj_name': [boxes.names[i] for i in oid.tolist()]}
    legs['physics_block'] = lambda: E.physics_block(pp, out, data, hand, boxes)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            ts[k].append(_ms(fn))
    res = {k: round(statistics.median(t), 3) for k, t in ts.items()}
    for k, n_tri in (('kernels_3072', 3072), ('kernels_20480', 20480)):
        res[k + '_gpairs_per_s'] = round(bs * 778 * n_tri / res[k] / 1e6, 1)
    if not a.no_eval:
        from vpho_amd.configs.args import cfg
        from vpho_amd.trainer import Trainer
        # the README eval config (bench.py): 100 hypotheses, 50 sampling steps, top-k 30 / 10, T0 0.65
        cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 100, 50, 30, 10, 0.65
        cfg.eval_batch_size, cfg.num_batches, cfg.checkpoint = bs, 4, None
        t = Trainer(cfg)
        t.eval(eval_physics=True)                   # warm-up, tables built
        for flag in (False, True, False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = t.eval(eval_physics=flag)
            torch.cuda.synchronize()
            res.setdefault('eval_images_per_s_' + ('physics' if flag else 'plain'), []).append(round(rows.shape[0] / (time.perf_counter() - t0), 1))
    res.update(bs=bs, reps=a.reps)
    print('PHYSICS_BENCH ' + json.dumps(res))


if __name__ == '__main__':
    main()

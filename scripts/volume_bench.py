"""Timing of the hand-object intersection volume (--eval_volume) at 64 pairs with HIP events, median of --reps, interleaved: the synthetic
hand (778 vertices, the faces of its convex hull) pushed into one side of the synthetic box objects, solids at the 5 mm pitch.
``setup`` is the entry point with the count launch left out (a solids table whose largest object has no centre: hand_mesh_setup_kernel and
the one-thread-per-pair finish), ``total`` all three launches, ``count`` their difference; Trainer.eval images/s at the README config with
and without eval_volume, interleaved in one process.  Prints one JSON line.
``python scripts/volume_bench.py [--reps 10] [--no-eval]``"""
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
    p.add_argument('--pitch', type=float, default=0.005)
    p.add_argument('--no-eval', action='store_true')
    a = p.parse_args(_argv)
    from vpho_amd import ops
    from vpho_amd.assets import synthetic_assets
    from vpho_amd.physics_eval import hand_faces, object_meshes
    assets = synthetic_assets(0)
    bs, dev, C = a.bs, 'cuda', ops.C
    rng = np.random.default_rng(0)
    faces = hand_faces(assets)
    meter = ops.HandObjectPenetration(object_meshes(assets), dev, accel=False, hand_faces=faces)
    t0 = time.perf_counter()
    sol = meter.build_solids(a.pitch)
    build_s = time.perf_counter() - t0
    names = [meter.names[i] for i in rng.integers(0, len(meter.names), bs)]
    oid = meter.obj_ids(names)
    rt = torch.zeros((bs, 3, 4), dtype=torch.float64, device=dev)
    rt[:, :, :3] = torch.eye(3, dtype=torch.float64)
    rt[:, 2, 3] = 0.6
    vt = assets['mano']['v_template'].astype(np.float64)
    hands = []
    for n in names:                                           # the hand's centroid on the object's +x side, fingers along -x into it
        half = np.asarray(assets['ycb'][n]['bbox3d'], np.float64).max(0)
        hands.append((vt - vt.mean(0)) * np.array([-1.0, 1.0, -1.0]) + np.array([half[0], 0.0, 0.0]) + rng.normal(size=3) * 0.004 + np.array([0, 0, 0.6]))
    hand = torch.from_numpy(np.stack(hands).astype(np.float32)).to(dev)
    out = torch.empty((bs, 2), dtype=torch.float64, device=dev)
    F_ = int(meter.hand_faces.shape[0])
    ws = torch.empty(ops.abi.query('vpho_hand_obj_intersection_workspace_bytes', bs, F_), dtype=torch.uint8, device=dev)
    empty = ops.ObjSolids(sol['pts'].data_ptr(), sol['pt_offset'].data_ptr(), len(meter.names), 0)

    def run(solids):
        ops._call('vpho_hand_obj_intersection_f64', C.byref(meter.c), C.byref(solids), meter.hand_faces, F_, hand, bs,
                  778, rt, oid, a.pitch, out, None, ws, ws.numel())
    legs = dict(setup=lambda: run(empty), total=lambda: run(sol['c']), wrapper=lambda: meter.volume(hand, rt, oid, a.pitch))
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    cells = meter.volume(hand, rt, oid, a.pitch)[:, 0]
    ts = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            ts[k].append(_ms(fn))
    res = {k + '_ms': round(statistics.median(t), 4) for k, t in ts.items()}
    res['count_ms'] = round(res['total_ms'] - res['setup_ms'], 4)
    res.update(faces=F_, solid_centres=int(sum(sol['counts'])), largest_solid=int(sol['max_pts']), build_solids_s=round(build_s, 2),
               mean_cells=round(float(cells.mean()), 1), intersecting=int((cells > 0).sum()))
    if not a.no_eval:
        from vpho_amd.configs.args import cfg
        from vpho_amd.trainer import Trainer
        # the README eval config (bench.py): 100 hypotheses, 50 sampling steps, top-k 30 / 10, T0 0.65
        cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 100, 50, 30, 10, 0.65
        cfg.eval_batch_size, cfg.num_batches, cfg.checkpoint, cfg.physics_voxel_pitch = bs, 4, None, a.pitch
        t = Trainer(cfg)
        t.eval(eval_volume=True)                    # warm-up, solids built
        for flag in (False, True, False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = t.eval(eval_volume=flag)
            torch.cuda.synchronize()
            res.setdefault('eval_images_per_s_' + ('volume' if flag else 'plain'), []).append(round(rows.shape[0] / (time.perf_counter() - t0), 1))
    res.update(bs=bs, reps=a.reps, pitch=a.pitch)
    print('VOLUME_BENCH ' + json.dumps(res))


if __name__ == '__main__':
    main()

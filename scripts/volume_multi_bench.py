"""Timing of the intersection volume of every sampled hypothesis (--eval_best with --eval_volume) at 64 images x 100 hypotheses with HIP
events, median of --reps, the two sides interleaved in one process: a closed torus "hand" of 1 552 faces on 778 vertices (MANO's closed
mesh sizes; the synthetic hull has 224 faces) pushed into one side of the synthetic box objects, solids at the 5 mm pitch.
``baseline``: HandObjectPenetration.volume on the 6 400 flattened pairs (the only way before the column walk; --chunk pairs per call, the
entry point takes at most 65 535), ``candidate``: HandObjectPenetration.volume_multi.  The per-hypothesis results must be byte-equal
(exit status 1 otherwise), and the candidate faster than the baseline by more than the baseline's own spread (exit status 2 otherwise).
Then Trainer.eval images/s at the README config with both flags, with and without the block, interleaved.  Prints one JSON line.
``python scripts/volume_multi_bench.py [--reps 7] [--no-eval] [--eval-batches 4]``"""
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
    p.add_argument('--reps', type=int, default=7)
    p.add_argument('--bs', type=int, default=64)
    p.add_argument('--S', type=int, default=100)
    p.add_argument('--pitch', type=float, default=0.005)
    p.add_argument('--chunk', type=int, default=6400)
    p.add_argument('--no-eval', action='store_true')
    p.add_argument('--eval-batches', type=int, default=4)
    a = p.parse_args(_argv)
    from vpho_amd import ops
    from vpho_amd.assets import synthetic_assets
    from vpho_amd.physics_eval import object_meshes, torus_mesh
    assets = synthetic_assets(0)
    bs, S, dev = a.bs, a.S, 'cuda'
    rng = np.random.default_rng(0)
    tv, tf = torus_mesh(97, 8, 0.035, 0.014)
    tv = np.concatenate([tv, np.repeat(tv[:1], 2, 0)])                       # 778 vertices, 1 552 faces
    meter = ops.HandObjectPenetration(object_meshes(assets), dev, accel=False, hand_faces=tf)
    sol = meter.build_solids(a.pitch)
    cols = meter.build_solid_columns(a.pitch)
    pick = rng.integers(0, len(meter.names), bs)
    oid = meter.obj_ids([meter.names[i] for i in pick])
    half = np.stack([np.asarray(assets['ycb'][meter.names[i]]['bbox3d'], np.float64).max(0) for i in pick])
    # the ring's centre on the object's +x side (the tube reaches into it), tilted about x and moved by a few mm per hypothesis
    ang = rng.uniform(-0.5, 0.5, (bs, S))
    Rx = np.zeros((bs, S, 3, 3))
    Rx[..., 0, 0] = 1.0
    Rx[..., 1, 1], Rx[..., 1, 2], Rx[..., 2, 1], Rx[..., 2, 2] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
    centre = np.stack([half[:, 0], np.zeros(bs), np.zeros(bs)], 1)[:, None] + rng.normal(size=(bs, S, 3)) * 0.004
    t_cam = np.array([0.0, 0.0, 0.6]) + rng.normal(size=(bs, S, 3)) * 0.002
    hand = np.einsum('bsij,vj->bsvi', Rx, tv) + centre[:, :, None] + t_cam[:, :, None]
    verts = torch.from_numpy(hand.astype(np.float32)).to(dev)
    rt = torch.zeros((bs, S, 3, 4), dtype=torch.float64, device=dev)
    rt[..., :3] = torch.eye(3, dtype=torch.float64)
    rt[..., 3] = torch.from_numpy(t_cam).to(dev)
    fv, frt, fid = verts.view(bs * S, 778, 3), rt.view(bs * S, 3, 4), oid.repeat_interleave(S).contiguous()

    def baseline():
        return torch.cat([meter.volume(fv[i:i + a.chunk], frt[i:i + a.chunk], fid[i:i + a.chunk], a.pitch) for i in range(0, bs * S, a.chunk)])

    def candidate():
        return meter.volume_multi(verts, rt, oid, a.pitch)

    t0 = time.perf_counter()
    ref = baseline()
    torch.cuda.synchronize()
    first_baseline_s = time.perf_counter() - t0
    table, per = candidate()
    torch.cuda.synchronize()
    same = torch.equal(per.view(bs * S, 2).view(torch.uint8), ref.view(torch.uint8))
    res = dict(bs=bs, S=S, pitch=a.pitch, reps=a.reps, faces=int(tf.shape[0]), equal=bool(same), first_baseline_s=round(first_baseline_s, 3),
               solid_centres_per_object=round(float(np.mean(sol['counts'])), 1), columns_per_object=round(float(np.mean(cols['counts'])), 1),
               centres_per_column=round(sum(sol['counts']) / max(sum(cols['counts']), 1), 2),
               mean_cells=round(float(per[..., 0].mean()), 1), intersecting_pairs=int((per[..., 0] > 0).sum()))
    if not same:
        print('VOLUME_MULTI_BENCH ' + json.dumps(res))
        print('per-hypothesis results differ from the per-pair kernel', file=sys.stderr)
        sys.exit(1)
    ts = dict(baseline=[], candidate=[])
    for _ in range(a.reps):
        ts['baseline'].append(_ms(baseline))
        ts['candidate'].append(_ms(candidate))
    for k, t in ts.items():
        res[k + '_ms'] = round(statistics.median(t), 4)
        res[k + '_spread_ms'] = round(max(t) - min(t), 4)
    res['speedup'] = round(res['baseline_ms'] / res['candidate_ms'], 2)
    gate = res['baseline_ms'] - res['candidate_ms'] > res['baseline_spread_ms']
    res['gate'] = bool(gate)
    if not a.no_eval:
        from vpho_amd.configs.args import cfg
        from vpho_amd.trainer import Trainer
        # the README eval config (bench.py): 100 hypotheses, 50 sampling steps, top-k 30 / 10, T0 0.65
        cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 100, 50, 30, 10, 0.65
        cfg.eval_batch_size, cfg.num_batches, cfg.checkpoint, cfg.physics_voxel_pitch = bs, a.eval_batches, None, a.pitch
        cfg.eval_best = cfg.eval_volume = True
        t = Trainer(cfg)
        t.eval()                                     # warm-up, solids and columns built
        for flag in (False, True, False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = t.eval(volume_multi=flag)
            torch.cuda.synchronize()
            res.setdefault('eval_images_per_s_' + ('with_block' if flag else 'without_block'), []).append(round(rows.shape[0] / (time.perf_counter() - t0), 1))
    print('VOLUME_MULTI_BENCH ' + json.dumps(res))
    if not gate:
        print('the column walk is not faster than the per-pair kernel by more than its spread', file=sys.stderr)
        sys.exit(2)


if __name__ == '__main__':
    main()

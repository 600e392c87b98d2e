"""Timing of the multi-hypothesis penetration metric (--eval_best with --eval_physics) at the README config -- 64 images x 100 hypotheses
x 778 hand vertices -- against the brute-force single-pose kernel on the same n * S pairs flattened, in one process, interleaved, with
HIP events: median of ``--reps`` passes, the baseline's max - min spread, the ratio, on the synthetic box (3 072 triangles) and on a
16 000-triangle torus standing in for a real YCB mesh; the mean share of a mesh's triangles a point visits (host restatement of the two
walks on a sample of the points); Trainer.eval images/s with both flags against --eval_best alone.  Prints one JSON line and exits
non-zero unless the new kernel beats the baseline on both meshes by more than the baseline's own spread.
``python scripts/physics_multi_bench.py [--reps 10] [--no-eval]``"""
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


def _visit_share(mesh, pts):
    """mean share of the mesh's triangles a point visits: nearest-walk clusters + its column's parity list"""
    from vpho_amd.physics_eval import mesh_accel, mesh_tables, nearest_candidates, parity_candidates
    tri, scale, translate = mesh_tables(mesh['verts'], mesh['faces'])
    acc = mesh_accel(tri)
    near = nearest_candidates(acc, pts)[0].sum(1).mean()
    par = parity_candidates(acc, scale, translate, pts).sum(1).mean()
    return dict(nearest=round(float(near) / len(tri), 5), parity=round(float(par) / len(tri), 5))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--bs', type=int, default=64)
    p.add_argument('--samples', type=int, default=100)
    p.add_argument('--no-eval', action='store_true')
    a = p.parse_args(_argv)
    from vpho_amd import ops
    from vpho_amd.physics_eval import box_mesh, torus_mesh
    n, S, V, dev = a.bs, a.samples, 778, 'cuda'
    rng = np.random.default_rng(0)
    half = np.array([0.05, 0.03, 0.04])
    corners = np.array([[x, y, z] for x in (-half[0], half[0]) for y in (-half[1], half[1]) for z in (-half[2], half[2])])
    tv, tf = torus_mesh(125, 64, major=0.045, minor=0.02)      # about the box's size: 13 x 4 x 13 cm
    meshes = {'box_3072': dict(zip(('verts', 'faces'), box_mesh(corners))), 'torus_16000': dict(verts=tv, faces=tf)}
    assert len(meshes['box_3072']['faces']) == 3072 and len(tf) == 16000
    rt = torch.zeros((n, S, 3, 4), dtype=torch.float64, device=dev)
    rt[..., :3] = torch.eye(3, dtype=torch.float64)
    rt[..., 2, 3] = 0.6
    # hands around the object: a good share of the vertices inside, the rest within a few centimetres
    model_pts = rng.normal(size=(n, S, V, 3)) * 0.04
    hand = torch.from_numpy((model_pts + np.array([0, 0, 0.6])).astype(np.float32)).to(dev)
    res = dict(n=n, S=S, V=V, reps=a.reps)
    for name, mesh in meshes.items():
        H = ops.HandObjectPenetration({name: mesh}, dev)
        ids = H.obj_ids([name] * n)
        ids_flat = H.obj_ids([name] * (n * S))
        flat_v, flat_rt = hand.view(n * S, V, 3), rt.view(n * S, 3, 4)
        legs = dict(single=lambda: H(flat_v, flat_rt, ids_flat), multi=lambda: H.multi(hand, rt, ids))
        per1 = legs['single']()
        table, per = legs['multi']()
        torch.cuda.synchronize()
        assert torch.equal(per.view(n * S, 4).view(torch.int64), per1.view(torch.int64)), 'the two kernels disagree'
        ts = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, fn in legs.items():
                ts[k].append(_ms(fn))
        single, multi = statistics.median(ts['single']), statistics.median(ts['multi'])
        spread = max(ts['single']) - min(ts['single'])
        res[name] = dict(single_ms=round(single, 3), multi_ms=round(multi, 3), single_spread_ms=round(spread, 3),
                         multi_spread_ms=round(max(ts['multi']) - min(ts['multi']), 3), ratio=round(single / multi, 2),
                         faster_by_more_than_the_spread=bool(single - multi > spread),
                         inside_share=round(float(per[..., 1].sum() / (n * S * V)), 3),
                         visit_share=_visit_share(mesh, model_pts.reshape(-1, 3)[::max(1, n * S * V // 2000)].astype(np.float32).astype(np.float64)))
    if not a.no_eval:
        from vpho_amd.configs.args import cfg
        from vpho_amd.trainer import Trainer
        # the README eval config (bench.py): 100 hypotheses, 50 sampling steps, top-k 30 / 10, T0 0.65
        cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = S, 50, 30, 10, 0.65
        cfg.eval_batch_size, cfg.num_batches, cfg.checkpoint = n, 4, None
        t = Trainer(cfg)
        t.eval(eval_best=True, eval_physics=True, physics_multi=True)     # warm-up, tables built
        for flag in (False, True, False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = t.eval(eval_best=True, eval_physics=flag, physics_multi=flag)
            torch.cuda.synchronize()
            res.setdefault('eval_images_per_s_' + ('best_physics' if flag else 'best'), []).append(round(rows.shape[0] / (time.perf_counter() - t0), 1))
    print('PHYSICS_MULTI_BENCH ' + json.dumps(res))
    slow = [name for name in meshes if not res[name]['faster_by_more_than_the_spread']]
    if slow:
        sys.exit(f'physics_multi_bench: the multi-hypothesis kernel does not beat the single-pose kernel by more than its spread on {slow}')


if __name__ == '__main__':
    main()

"""Same entry point as the reference's force_optim.py:7-9 (ForceOptimizer(cfg).optimize_batch()): pseudo-force label
optimisation over hand-object pairs.  No data set in this build -> synthetic pairs (seeded MANO poses through the HIP FK,
random contact maps); pairs are sharded over the ranks of one node (one process per GPU), no collective on the data path.

    python force_optim.py --pairs 10000 [--batch_size 64]            # or torch.distributed.run --nproc-per-node N ...
Prints one JSON line per run (rank 0): pairs/s over all ranks, final mean losses.

    python force_optim.py --frame_source synthetic|DIR [--num_frames N] [--out PATH]
labels a frame source from its annotations instead (contact, grasp and pseudo-forces: label_frames) and writes physics_labels.npz."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pairs', type=int, default=10000)
    p.add_argument('--batch_size', type=int, default=64)
    p.add_argument('--iters', type=int, default=3000)
    p.add_argument('--phase1', type=int, default=300)
    p.add_argument('--gpus', type=int, default=int(os.environ.get('WORLD_SIZE', '1')))
    # labels for a frame source instead of the synthetic pairs (label_frames below): 'synthetic' or a FrameDirectory path
    p.add_argument('--frame_source', type=str, default='none')
    p.add_argument('--num_frames', type=int, default=None)
    p.add_argument('--out', type=str, default=None)
    args = p.parse_args()
    if args.frame_source != 'none':
        if args.gpus != 1:
            p.error('--frame_source labels one source on one GPU: run it with --gpus 1')
        if args.frame_source == 'synthetic' and not args.out:
            p.error('--frame_source synthetic has no directory to write into: give --out PATH')
        if not 1 <= args.batch_size <= 64:
            p.error('--batch_size: the force optimiser takes batches of 1 .. 64 pairs')
    from vpho_amd.launch import maybe_spawn, world_from_env
    maybe_spawn(args.gpus)             # N > 1 from a bare shell: start the N rank processes (before any GPU call)
    sys.argv = sys.argv[:1]
    if args.frame_source != 'none':
        return label_frames(args)
    import torch
    import torch.distributed as dist
    from vpho_amd import ops
    from vpho_amd.assets import load_assets, ANCHOR_SKELETON
    from vpho_amd.evaluate import shard_range

    world, rank, local = world_from_env(args.gpus)
    rehearse = os.environ.get('VPHO_REHEARSE_ONE_GPU') == '1'    # every rank on cuda:0 over gloo (1-GPU box; timings meaningless)
    if rehearse:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    from vpho_amd.launch import init_process_group
    init_process_group(dev)                               # loud on failure: bounded timeout, expected vs observed world, first collective
    assets = load_assets('asset')
    n_batches = (args.pairs + args.batch_size - 1) // args.batch_size
    lo, hi = shard_range(n_batches, rank, world)
    n = (hi - lo) * args.batch_size
    g = torch.Generator().manual_seed(1000 + rank)
    mano = ops.Mano(assets['mano'], dev)
    agg = ops.Aggregation(assets, ANCHOR_SKELETON, dev)
    pose = (torch.randn(n, 48, generator=g) * 0.3).to(dev)
    ctx = mano.shape((torch.randn(n, 10, generator=g) * 0.5).to(dev))
    verts, _ = mano.fk(pose, ctx, 1, True)
    verts = (verts + torch.tensor([0.0, 0.0, 0.7], device=dev)).contiguous()
    grav = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).to(dev)
    com = (torch.tensor([0.05, 0.0, 0.7]) + torch.randn(n, 3, generator=g) * 0.02).to(dev)
    fc = torch.rand(n, 32, generator=g).to(dev)
    grasped = (torch.rand(n, generator=g) < 0.8).to(torch.uint8).to(dev)
    agg.force_optimize(verts[:args.batch_size], grav[:args.batch_size], com[:args.batch_size], fc[:args.batch_size], grasped[:args.batch_size],
                       args.batch_size, iters=10, phase1=5)                       # warm-up
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    ops.prof_enable('force_optim', True)                  # HIP events around the persistent kernel (one launch)
    t0 = time.perf_counter()
    out = agg.force_optimize(verts, grav, com, fc, grasped, args.batch_size, iters=args.iters, phase1=args.phase1)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
    tot = torch.tensor([float(n)], device=dev, dtype=torch.float64)
    if world > 1:
        if rehearse:
            dt, tot = dt.cpu(), tot.cpu()
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        dist.all_reduce(tot)
    kprof = ops.prof_collect('force_optim')
    ops.prof_enable('force_optim', False)
    if rank == 0:
        losses = out['losses'].mean(0).tolist()
        # ALU-bound, not HBM / MFMA: 480 fp32 operations per (pair, anchor) item and iteration (counted on the reference's arithmetic in
        # csrc/force_optim.hip) against the fp32 vector peak (packed FMA).  One 1024-thread workgroup per batch of 64 pairs: a sample's 32
        # anchors in one DPP row, two per lane in packed registers; ~640 issued instructions per thread and iteration (two items), of
        # which ~70 are quarter-rate transcendentals (v_exp / v_rcp / v_sqrt / v_log); 157 workgroups leave 99 of the 256 CUs idle at the
        # default 10 048 pairs.  VPHO_FORCE_EXACT=1: IEEE divisions / square roots and libm exp / log instead (2.8 x slower)
        tf = kprof['flops'] / kprof['total_ms'] / 1e9 if kprof['total_ms'] else None
        exact = os.environ.get('VPHO_FORCE_EXACT') == '1'
        traffic, source = pmc_traffic('force_optim_kernel') if (args.pairs, args.batch_size, args.iters, exact) == (10048, 64, 3000, False) else (None, None)
        roof = {'bound': 'valu', 'kernel': f'force_optim_kernel<{"true" if exact else "false"}> (3000 AdamW iterations per batch in one persistent workgroup)', 'achieved': tf, 'peak': 157.3,
                'unit': 'TFLOP/s', 'frac': tf / 157.3 if tf else None, 'traffic': traffic, 'traffic_source': source, 'flop_per_pair_per_iteration': 480 * 32,
                'algorithmic_bytes_per_launch': int(tot.item()) * (32 * (3 + 9 + 1 + 3 + 3 + 1 + 8) * 4 + 6 * 4 + 1),     # per pair: anchor points, frames, contact map in; two force labels, scale, cone weights out; gravity, centre of mass, flag
                'kernel_ms': kprof['total_ms'], 'workgroups': (hi - lo), 'timing': 'HIP events around the launch on the launch stream',
                'limited_by': 'vector-ALU issue: ~640 instructions per thread (two items) and iteration for the 2 x 480 counted operations, ~70 of them '
                              'quarter-rate transcendentals; 4 waves per SIMD; no scratch and no HBM traffic inside the loops; 157 workgroups for 256 CUs at 10 048 pairs'}
        print(json.dumps({'roofline': roof, 'metric': 'pseudo-force optimisation pairs/s (3000 AdamW iterations per pair)', 'value': float(tot.item() / dt.item()),
                          'unit': 'pairs/s', 'n_gpus': world, 'pairs': int(tot.item()), 'batch_size': args.batch_size, 'iters': args.iters,
                          'seconds': float(dt.item()), 'mean_losses_force_gravity_moment_dist': losses, 'data': 'synthetic'}))
    if world > 1:
        dist.destroy_process_group()


CHAIN_BATCH = 256


def label_frames(args):
    """--frame_source synthetic|DIR: the physics labels of every frame of the source, from its annotations alone
    (vpho_amd/physics_labels.py).  The pipeline runs in evaluation mode (no draws: the reference sets ``trainset.is_train = False`` for this
    pass), the contact chain per loader batch, the pseudo-force optimisation over all pairs at the end: the full batches of --batch_size
    in one call, a remainder as a second one.  Writes DIR/physics_labels.npz (or --out) and prints one JSON line."""
    import numpy as np
    import torch
    from vpho_amd.configs.args import cfg
    from vpho_amd.assets import load_assets
    from vpho_amd import frames as FR
    from vpho_amd.physics_labels import PhysicsLabeler

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    assets = load_assets(cfg.asset_root)
    if args.frame_source == 'synthetic':
        source = FR.synthetic_frames(args.num_frames if args.num_frames is not None else 4 * args.batch_size, assets, seed=int(cfg.random_seed))
        path = args.out
    else:
        source = FR.FrameDirectory(args.frame_source)
        path = args.out or os.path.join(args.frame_source, FR.LABEL_FILE)
    n = len(source) if args.num_frames is None else min(int(args.num_frames), len(source))
    if n < 1:
        raise SystemExit(f'force_optim.py: {args.frame_source} holds no frame to label')

    class Head:                                            # the first n frames of the source
        def __len__(self):
            return n

        def __getitem__(self, i):
            return source[i]

    labeler = PhysicsLabeler(cfg, assets, dev)
    # the contact chain is per sample: it runs on loader batches of up to CHAIN_BATCH frames, whatever the optimiser's batch size is
    loader = FR.FrameLoader(Head(), min(n, max(args.batch_size, CHAIN_BATCH)), FR.FramePipeline(cfg, assets, dev, train=False, seed=int(cfg.random_seed)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = {k: [] for k in ('index', 'hv', 'gravity', 'com', 'hand_contact', 'force_contact', 'is_grasped')}
    for batch in loader:
        lab = labeler(batch)
        sign = torch.where(batch['is_right'].bool(), 1.0, -1.0)[:, None] * torch.tensor([1.0, 0.0, 0.0], device=dev) + torch.tensor([0.0, 1.0, 1.0], device=dev)
        for k, v in (('index', batch['index']), ('hv', batch['gt_hand_vert_flip']), ('gravity', batch['gravity'].reshape(-1, 3) * sign),
                     ('com', batch['obj_CoM'].reshape(-1, 3) * sign), ('hand_contact', lab['hand_contact']), ('force_contact', lab['force_contact']),
                     ('is_grasped', lab['is_grasped'])):
            keep[k].append(v)
    keep = {k: torch.cat(v) for k, v in keep.items()}
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    opt = labeler.optimize(keep['hv'].contiguous(), keep['gravity'].contiguous(), keep['com'].contiguous(), keep['force_contact'],
                           keep['is_grasped'].to(torch.uint8), args.batch_size, iters=args.iters, phase1=args.phase1)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    meta = dict(labeler.meta(), iters=args.iters, phase1=args.phase1, batch_size=args.batch_size, frame_source=args.frame_source)
    host = lambda t: t.detach().cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, index=host(keep['index']).astype(np.int64), hand_contact=host(keep['hand_contact']), force_contact=host(keep['force_contact']),
             is_grasped=host(keep['is_grasped']).astype(bool), force_local=host(opt['force_local']), force_global=host(opt['force_global']),
             meta=np.array(json.dumps(meta)))
    print(json.dumps({'metric': f'physics labels from annotations, pairs/s ({args.iters} AdamW iterations per pair)', 'value': n / (t2 - t0), 'unit': 'pairs/s',
                      'pairs': n, 'batch_size': args.batch_size, 'iters': args.iters, 'seconds': t2 - t0, 'seconds_contact_chain_with_frames': t1 - t0,
                      'seconds_force_optimize': t2 - t1, 'grasped_share': float(keep['is_grasped'].float().mean()),
                      'mean_losses_force_gravity_moment_dist': opt['losses'].mean(0).tolist(), 'out': path, 'gap_table': meta['gap_table'],
                      'data': args.frame_source}))


def pmc_traffic(kernel):
    """(HBM bytes per launch, file) of `kernel` from the newest committed counter pass of THIS workload (profiles/rNN_force_pmc_hbm_traffic.json:
    10 048 pairs, batches of 64, 3000 iterations; 2 x FETCH_SIZE + WRITE_SIZE), (None, None) when there is none."""
    root = os.path.dirname(os.path.abspath(__file__))
    for rnd in ('r06', 'r05'):
        path = os.path.join(root, 'profiles', f'{rnd}_force_pmc_hbm_traffic.json')
        try:
            with open(path) as f:
                tab = json.load(f)
        except Exception:
            continue
        hit = [v for k, v in tab.items() if k.startswith(kernel)]
        if hit:
            # the pass holds the 10-iteration, one-batch warm-up launch too (a few hundred KB): the sum over launches IS the timed launch
            return sum(v['hbm_bytes_per_launch'] * v['launches'] for v in hit), os.path.relpath(path, root)
    return None, None


if __name__ == '__main__':
    main()

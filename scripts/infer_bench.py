"""What does writing predictions cost the evaluation pipeline?  ``Trainer.eval`` of the PARENT commit against this tree's ``Trainer.eval``
and ``Trainer.infer`` at the README config (bs 64, S 100, 50 sampling steps, 50 synthetic batches), interleaved on one box.

    python scripts/infer_bench.py --parent <root of a built checkout of the parent commit> [--reps 10] [--steps 50] [--visits 2]

The orchestrating process never opens the GPU: it starts ONE child at a time, alternating parent / branch ``--visits`` times; every child
builds a Trainer, runs one warm-up pass and then its share of the ``--reps`` timed passes (the branch child interleaves eval and infer
pass by pass).  Legs:
  (a) parent  Trainer.eval images/s          (the parent's own python + library: the child runs with the parent root first on sys.path)
  (b) branch  Trainer.eval images/s          -- must sit inside (a)'s own min..max spread
  (c) branch  Trainer.infer images/s up to the last record collected in host memory (no file work)
              -- judged against (a): not below (a)'s minimum by more than the copy time, record bytes per batch / measured pinned D2H rate
  (d) branch  Trainer.infer images/s with the files written (reported, not gated: JSON encoding is host work)
and, from the last branch child, the record kernel alone (HIP events, median over the last child's passes) next to the time its bytes would take at
the measured HBM copy rate of MI355X_MICROARCH.md (6.29 TB/s), and the pinned D2H rate.  Prints one ``INFER_BENCH`` JSON line.
A leg that could not be taken is reported as null with the reason, never estimated.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

_argv = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.29e12


def _args():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', type=str, default='')
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--steps', type=int, default=50)
    p.add_argument('--bs', type=int, default=64)
    p.add_argument('--visits', type=int, default=2)
    p.add_argument('--child', type=str, default='', choices=['', 'eval', 'branch'])
    p.add_argument('--root', type=str, default=ROOT)
    p.add_argument('--kernel', action='store_true')
    return p.parse_args(_argv)


def _trainer(a):
    sys.argv = sys.argv[:1]
    sys.path.insert(0, a.root)
    import torch
    from vpho_amd.configs.args import cfg
    from vpho_amd.trainer import Trainer
    # the README eval config (bench.py): 100 hypotheses, 50 sampling steps, top-k 30 / 10, T0 0.65
    cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 100, 50, 30, 10, 0.65
    cfg.eval_batch_size, cfg.num_batches, cfg.checkpoint = a.bs, a.steps, None
    return torch, cfg, Trainer(cfg)


def _quiet(fn):
    """run fn with stdout parked in a file (the tables of 3 200 images are not the measurement)"""
    sys.stdout.flush()
    keep = os.dup(1)
    with open(os.devnull, 'w') as null:
        os.dup2(null.fileno(), 1)
        try:
            return fn()
        finally:
            sys.stdout.flush()
            os.dup2(keep, 1)
            os.close(keep)


def _eval_rate(torch, t):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = _quiet(t.eval)
    torch.cuda.synchronize()
    return rows.shape[0] / (time.perf_counter() - t0)


def child_eval(a):
    torch, cfg, t = _trainer(a)
    _quiet(t.eval)
    print('CHILD ' + json.dumps({'eval': [_eval_rate(torch, t) for _ in range(a.reps)]}), flush=True)


def _kernel_legs(torch, a):
    from vpho_amd import ops
    n = a.bs
    packer = ops.InferPacker('cuda', max_batch=n, slots=1)
    g = torch.Generator().manual_seed(0)
    out = {'reg_hand_joint': torch.randn(n, 21, 3, generator=g).cuda(), 'reg_hand_vert': torch.randn(n, 778, 3, generator=g).cuda(),
           'agg_hand_joint': torch.randn(n, 21, 3, generator=g).cuda(), 'agg_hand_vert': torch.randn(n, 778, 3, generator=g).cuda(),
           'agg_obj_6d': torch.randn(n, 9, generator=g, dtype=torch.float64).cuda()}
    batch = {'root_joint': torch.randn(n, 3, generator=g).cuda(), 'is_right': (torch.rand(n, generator=g) < 0.5).cuda()}
    stage, host = packer.stage[0], packer.host[0]
    rj, rv, aj, av = (out[k] for k in ('reg_hand_joint', 'reg_hand_vert', 'agg_hand_joint', 'agg_hand_vert'))
    o9, root, flag = out['agg_obj_6d'], batch['root_joint'], batch['is_right'].view(torch.uint8)

    def ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    kernel = lambda: ops._call('vpho_infer_pack_f32', rj, rv, aj, av, o9, root, flag, n, 21, 778, stage, None)                 # records_host NULL: the kernel alone
    copy = lambda: host.copy_(stage, non_blocking=True)
    both = lambda: packer.pack(out, batch)
    for fn in (kernel, copy, both):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {'kernel': [], 'copy': [], 'pack': []}
    for _ in range(a.reps):                                                          # interleaved
        ts['kernel'].append(ms(kernel))
        ts['copy'].append(ms(copy))
        ts['pack'].append(ms(both))
    rec = packer.record_bytes
    moved = n * (4 * 4794 + 72 + 12 + 1) + n * rec                                   # operands read once + records written once
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {'record_bytes': rec, 'batch_bytes': n * rec, 'kernel_ms': med['kernel'], 'kernel_ms_all': ts['kernel'], 'kernel_bytes_moved': moved,
            'hbm_time_ms_at_6.29TBps': moved / HBM_BYTES_PER_S * 1e3, 'copy_ms': med['copy'], 'pinned_d2h_GBps': n * rec / med['copy'] / 1e6,
            'pack_ms': med['pack']}


def child_branch(a):
    torch, cfg, t = _trainer(a)
    _quiet(t.eval)
    tmp = tempfile.mkdtemp(prefix='vpho_infer_bench_')
    _quiet(lambda: t.infer(save_dir=os.path.join(tmp, 'warm')))
    res = {'eval': [], 'infer_collected': [], 'infer_files': []}
    for i in range(a.reps):
        res['eval'].append(_eval_rate(torch, t))
        r = _quiet(lambda: t.infer(save_dir=os.path.join(tmp, f'run{i}')))
        res['infer_collected'].append(r['images_per_s'])
        res['infer_files'].append(r['images_per_s_with_files'])
    if a.kernel:
        res['kernel'] = _kernel_legs(torch, a)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    print('CHILD ' + json.dumps(res), flush=True)


def _spawn(a, mode, root, reps, kernel=False):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', mode, '--root', root, '--reps', str(reps), '--steps', str(a.steps), '--bs', str(a.bs)]
    r = subprocess.run(cmd + (['--kernel'] if kernel else []), cwd=root, capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith('CHILD ')]
    if r.returncode != 0 or len(line) != 1:
        raise RuntimeError(f'{mode} child in {root} failed ({r.returncode}):\n' + r.stdout[-1500:] + r.stderr[-3000:])
    return json.loads(line[0][len('CHILD '):])


def main():
    a = _args()
    if a.child:
        return child_eval(a) if a.child == 'eval' else child_branch(a)
    per = -(-a.reps // a.visits)
    legs = {'a_parent_eval': [], 'b_branch_eval': [], 'c_infer_collected': [], 'd_infer_files': []}
    kernel, why_no_parent = None, None
    if not a.parent or not os.path.exists(os.path.join(a.parent, 'vpho_amd', 'libvpho_hip.so')):
        why_no_parent = f'no built parent checkout at --parent {a.parent!r}'
    for v in range(a.visits):
        if why_no_parent is None:
            legs['a_parent_eval'] += _spawn(a, 'eval', os.path.abspath(a.parent), per)['eval']
        r = _spawn(a, 'branch', ROOT, per, kernel=v == a.visits - 1)
        legs['b_branch_eval'] += r['eval']
        legs['c_infer_collected'] += r['infer_collected']
        legs['d_infer_files'] += r['infer_files']
        kernel = r.get('kernel', kernel)
    med = lambda v: round(statistics.median(v), 1) if v else None
    out = {'config': dict(bs=a.bs, steps=a.steps, reps=a.reps, visits=a.visits, S=100, sampling_steps=50), 'images_per_s': {}, 'kernel': kernel}
    for k, v in legs.items():
        out['images_per_s'][k] = dict(median=med(v), min=round(min(v), 1), max=round(max(v), 1), all=[round(x, 1) for x in v]) if v else None
    if why_no_parent is not None:
        out['not_taken'] = {'a_parent_eval': why_no_parent}
    else:
        A, B, Cc = legs['a_parent_eval'], legs['b_branch_eval'], legs['c_infer_collected']
        copy_s = kernel['copy_ms'] * 1e-3                     # per batch, at the pinned D2H rate measured above
        batch_s_at_a_min = a.bs / min(A)
        floor_c = a.bs / (batch_s_at_a_min + copy_s)          # (a)'s slowest pass plus one exposed copy per batch
        out['verdict'] = {'b_inside_a_spread': bool(min(A) <= statistics.median(B) <= max(A)), 'b_not_below_a_min': bool(statistics.median(B) >= min(A)),
                          'c_floor_images_per_s': round(floor_c, 1), 'c_not_below_floor': bool(statistics.median(Cc) >= floor_c)}
    print('INFER_BENCH ' + json.dumps(out))


if __name__ == '__main__':
    main()

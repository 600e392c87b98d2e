"""The front of the physics-label chain at the size of a batch: 64 samples, 778 hand vertices, 1 080 filled rows
(csrc/hand_surface.hip, vpho_amd/physics_labels.py).  The real MANO faces when the assets are present, else the closed 1 552-face test
mesh of tests/_hand_surface_fp64.py (the synthetic MANO's hull faces leave most vertices without a face).

HIP events, median of 10 (min .. max), the forms interleaved:
  * ``HandSurface.fill`` alone
  * the five-launch contact chain of ``PhysicsLabeler`` (fill, object vertices posed, hand_contact, clamp, force_contact)
By wall clock:
  * labels/s of the label pass at 3 000 iterations over 1 024 pairs as ``force_optim.py --frame_source`` runs it -- the chain on batches of
    256, then ``force_optimize`` in batches of 64 -- against the same pass with the chain's outputs precomputed (``force_optimize`` alone)
  * the numpy float64 restatement of the normals and the fill per sample on this host: the CPU yardstick (the reference calls trimesh
    per sample; trimesh is not installed)

    python scripts/hand_surface_bench.py [--out profiles/hand_surface_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
N, CHAIN, REPS, PAIRS, ITERS, PHASE1 = 64, 256, 10, 1024, 3000, 300


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                                                   # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    args, _ = ap.parse_known_args()
    sys.argv = [sys.argv[0]]
    import _hand_surface_fp64 as HS
    from vpho_amd import frames as FR
    from vpho_amd.assets import load_assets
    from vpho_amd.configs.args import cfg
    from vpho_amd.physics_labels import PhysicsLabeler
    assets = load_assets(cfg.asset_root)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    real = assets['sources']['mano'] != 'synthetic'
    if not real:
        assets = dict(assets, mano=dict(assets['mano'], faces=HS.ellipsoid()[1]))
    lab = PhysicsLabeler(cfg, assets, 'cuda')
    src = FR.synthetic_frames(PAIRS, assets, seed=0, size=(160, 120))
    batches = list(FR.FrameLoader(src, CHAIN, FR.FramePipeline(cfg, assets, 'cuda', train=False, seed=0)))
    torch.cuda.synchronize()
    b256 = batches[0]
    b0 = {k: (v[:N].contiguous() if torch.is_tensor(v) else v[:N]) for k, v in b256.items()}
    hv = b0['gt_hand_vert_flip'].contiguous()
    out = lab.surface.fill(hv)
    forms = {'fill': lambda: lab.surface.fill(hv, out=out), 'chain': lambda: lab(b0), 'chain256': lambda: lab(b256)}
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(REPS):
        for k, f in forms.items():
            t[k].append(timed(f))
    say(f'hand_surface_bench: {N} samples, V 778, F {lab.surface.F} ({"MANO faces" if real else "the closed test mesh"}), L {lab.surface.L} '
        f'(gap table: {lab.gap["source"]}), object table {tuple(lab.obj_verts.shape)}')
    for k, name in (('fill', 'HandSurface.fill'), ('chain', 'contact chain, five launches (fill, pose, hand_contact, clamp, force_contact)'),
                    ('chain256', f'the same chain on {CHAIN} samples')):
        say(f'  {name}: {statistics.median(t[k]):9.1f} us  ({min(t[k]):.1f} .. {max(t[k]):.1f})')
    sign = lambda b: torch.where(b['is_right'].bool(), 1.0, -1.0)[:, None] * torch.tensor([1.0, 0.0, 0.0], device='cuda') + torch.tensor([0.0, 1.0, 1.0], device='cuda')
    allhv = torch.cat([b['gt_hand_vert_flip'] for b in batches]).contiguous()
    grav = torch.cat([b['gravity'].reshape(-1, 3) * sign(b) for b in batches]).contiguous()
    com = torch.cat([b['obj_CoM'].reshape(-1, 3) * sign(b) for b in batches]).contiguous()

    def chain_all():
        labs = [lab(b) for b in batches]
        return torch.cat([l['force_contact'] for l in labs]), torch.cat([l['is_grasped'] for l in labs]).to(torch.uint8)

    fc, gr = chain_all()
    lab.optimize(allhv[:N], grav[:N], com[:N], fc[:N].contiguous(), gr[:N].contiguous(), N, iters=10, phase1=5)
    torch.cuda.synchronize()
    rates = {'with': [], 'pre': []}
    for _ in range(3):
        for k in ('with', 'pre'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f, g = chain_all() if k == 'with' else (fc, gr)
            lab.optimize(allhv, grav, com, f, g, N, iters=ITERS, phase1=PHASE1)
            torch.cuda.synchronize()
            rates[k].append(PAIRS / (time.perf_counter() - t0))
    say(f'  label pass, {PAIRS} pairs in batches of {N}, {ITERS} iterations: {statistics.median(rates["with"]):.0f} labels/s with the chain on batches of {CHAIN}, '
        f'{statistics.median(rates["pre"]):.0f} labels/s with its outputs precomputed (wall clock, median of 3, interleaved)')
    v = hv[:8].cpu().numpy()
    t0 = time.perf_counter()
    HS.hand_surface(v, np.asarray(assets['mano']['faces']), lab.gap['links'], lab.gap['alpha'])
    cpu_ms = (time.perf_counter() - t0) * 1e3 / 8
    say(f'  numpy float64 restatement of the normals and the fill on this host: {cpu_ms:.1f} ms per sample (8 samples vectorised)')
    say('HAND_SURFACE_BENCH ' + json.dumps(dict(fill_us=statistics.median(t['fill']), chain_us=statistics.median(t['chain']), samples=N,
                                                chain256_us=statistics.median(t['chain256']),
                                                labels_per_s=statistics.median(rates['with']), labels_per_s_chain_precomputed=statistics.median(rates['pre']),
                                                pairs=PAIRS, iters=ITERS, numpy_ms_per_sample=cpu_ms, faces='mano' if real else 'test mesh')))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""The photometric augmentation at the size of a camera batch: 64 frames of 640 x 480 -> 256 (vpho_amd/photo.py, csrc/photo.hip).

HIP events, warm-ups, median of 10 (min .. max), the forms interleaved.  Every new gate is ON for every sample (clip limit 4, contrast,
hue, a 7 x 7 blur and a 7 x 7 motion line), which is the most any batch can cost:
  * each ``ops.photo_*`` launch on its own (the zero fill of the grey sums counts towards ``photo_grey_sum``), and their sum
  * ``ops.frame_patch`` alone (training form), the launch all of this replaces, measured in the same run
  * the host-to-device copy of the 59 MB of frames from pinned memory
  * one ``photo.photo_patch`` call (all launches back to back, uploads of the parameters included)

    python scripts/photo_bench.py [--out profiles/photo_bench.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, H, W, P, REPS = 64, 480, 640, 256, 10


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
    sys.argv = [sys.argv[0], '--mode', 'train', '--photo_aug', 'reference']
    from vpho_amd import frames as FR, ops, photo as PH
    from vpho_amd.assets import load_assets
    from vpho_amd.configs.args import cfg
    assets = load_assets(cfg.asset_root)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    src = FR.synthetic_frames(N, assets, seed=0, size=(W, H))
    items = [src[i] for i in range(N)]
    host = torch.from_numpy(np.stack([f for f, _ in items])).pin_memory()
    rec = FR._stack_records([r for _, r in items])
    dev = host.cuda()
    K, rt = np.asarray(rec['cam_intr'], np.float64), np.asarray(rec['obj_rt'], np.float64)
    names = [FR.YCB_NAMES[int(i)] for i in rec['obj_id']]
    kp = np.stack([np.asarray(assets['ycb'][n]['kpt3d'], np.float64) for n in names]) @ np.swapaxes(rt[:, :, :3], -1, -2) + rt[:, None, :, 3]
    right = np.asarray(rec['is_right'], bool)
    per = [FR.sample_draws(cfg, 0, 0, i, True, P) for i in range(N)]
    draws = {k: np.stack([np.asarray(d[k]) for d in per]) for k in per[0]}
    plan = FR.crop_plan(rec['jt2d'], FR.project(kp, K), K, draws, P, cfg.bbox_scale_factor, is_right=right)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    minv, flip, colour = c(plan['minv']), c((~right).astype(np.uint8)), c(draws['colour'].astype(np.float32))
    erase, key = c(draws['erase'].astype(np.int32)), c(draws['key'].astype(np.uint32).view(np.int32))
    # every gate on, the largest kernels
    r = np.random.default_rng(0)
    params = dict(clip_limit=np.full(N, 4.0), contrast=r.uniform(0.6, 1.3, N).astype(np.float32), hue=r.uniform(0.05, 0.15, N).astype(np.float32),
                  k1=np.stack([PH.blur_kernel(7, r.uniform(0.2, 2), r.uniform(0.2, 2), r.uniform(-90, 90), r.uniform(0.5, 8), r.uniform(0.9, 1.1, 49)) for _ in range(N)]),
                  K1=np.full(N, 7), k2=np.stack([PH.motion_kernel(7, int(r.integers(0, 48))) for _ in range(N)]), K2=np.full(N, 7))
    clip = [PH.clahe_clip(4.0, P // 8)] * N
    contrast, hue, k1, k2 = c(params['contrast']), c(params['hue']), c(params['k1']), c(params['k2'])
    K7 = [7] * N
    out = torch.empty((N, 3, P, P), device='cuda')
    levels = ops.photo_levels(dev, minv, P)
    l8, lut, clipd = ops.photo_clahe_lut(levels, clip)
    after = ops.photo_clahe_apply(levels, clipd, l8, lut)
    sums = ops.photo_grey_sum(after, colour)
    final = ops.photo_colour(after, colour, contrast, hue, sums)
    stage = torch.empty_like(levels)
    new = {
        'photo_levels (warp -> uint8 levels)': lambda: ops.photo_levels(dev, minv, P, out=stage),
        'photo_clahe_lut (L8 plane, 64 histograms and LUTs per image)': lambda: ops.photo_clahe_lut(levels, clip),
        'photo_clahe_apply (interpolation, Lab round trip)': lambda: ops.photo_clahe_apply(levels, clipd, l8, lut, out=stage),
        'photo_grey_sum (zero fill + integer sum)': lambda: ops.photo_grey_sum(after, colour),
        'photo_colour (shift, brightness, contrast, saturation, hue)': lambda: ops.photo_colour(after, colour, contrast, hue, sums, out=stage),
        'photo_filter (7 x 7 + 7 x 7, mirror, normalise, erase)': lambda: ops.photo_filter(final, k1, K7, k2, K7, flip=flip, erase=erase, key=key, out=out),
    }
    forms = dict(new)
    forms['frame_patch (training: colour, flip, erasing), the launch this replaces'] = lambda: ops.frame_patch(dev, minv, P, colour=colour, flip=flip, erase=erase, key=key, out=out)
    forms['host-to-device copy of the frames (pinned, 59.0 MB)'] = lambda: dev.copy_(host, non_blocking=True)
    forms['photo_patch (all of the above back to back, parameter uploads included)'] = lambda: PH.photo_patch(ops, dev, minv, P, colour, params, flip=flip, erase=erase, key=key)
    say(f'photo_bench: {N} frames {W} x {H} -> {P}, every new gate on for every sample (clip limit 4, contrast, hue, 7 x 7 blur, 7 x 7 motion line)')
    for _ in range(3):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(REPS):
        for k, f in forms.items():
            t[k].append(timed(f))
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, v in t.items():
        say(f'  {k}: {med[k]:9.1f} us  ({min(v):.1f} .. {max(v):.1f})')
    total = sum(med[k] for k in new)
    patch = med['frame_patch (training: colour, flip, erasing), the launch this replaces']
    copy = med['host-to-device copy of the frames (pinned, 59.0 MB)']
    top = max(new, key=lambda k: med[k])
    say(f'  sum of the six launches: {total:.1f} us = frame_patch {patch:.1f} us + {total - patch:.1f} us added; the copy takes {copy:.1f} us')
    say(f'  added device time / copy = {(total - patch) / copy:.2f}: the front end {"stays" if total - patch < copy else "is no longer"} copy-bound; '
        f'the largest launch is {top.split(" (")[0]} ({med[top]:.1f} us)')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

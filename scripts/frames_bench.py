"""The data front end at the size of a camera batch: 64 frames of 640 x 480 -> 256 (vpho_amd/frames.py, csrc/frames.hip).

HIP events, median of 10 (min .. max), the forms interleaved:
  * ``ops.frame_patch`` alone (evaluation form; training form with colour, flip and erasing)
  * the two ``ops.heatmap_targets`` launches (adaptive hand maps, square object maps)
  * the host-to-device copy of the 59 MB of frames from pinned memory, on its own
  * the yardstick: torch on the device, ``affine_grid`` + ``grid_sample(mode='bicubic')`` on the float frames, flip, normalise
  * the host side of one ``FramePipeline`` call (plan, labels, uploads) by wall clock
``--eval``: ``Trainer.eval`` images/s at the README configuration on a ``FrameLoader`` of synthetic frames (generated before the clock
starts) against the default synthetic batch dicts.

    python scripts/frames_bench.py [--eval] [--out profiles/frames_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, H, W, P, S, REPS = 64, 480, 640, 256, 64, 10


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                                                   # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--eval', action='store_true')
    ap.add_argument('--out', default='')
    args, _ = ap.parse_known_args()
    sys.argv = [sys.argv[0], '--mode', 'eval']
    from vpho_amd import frames as FR, ops
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
    recs = [r for _, r in items]
    dev = host.cuda()
    pipe_eval = FR.FramePipeline(cfg, assets, 'cuda', train=False, seed=0)
    pipe_train = FR.FramePipeline(cfg, assets, 'cuda', train=True, seed=0)
    rec = FR._stack_records(recs)
    K = np.asarray(rec['cam_intr'], np.float64)
    rt = np.asarray(rec['obj_rt'], np.float64)
    names = [FR.YCB_NAMES[int(i)] for i in rec['obj_id']]
    kp = np.stack([np.asarray(assets['ycb'][n]['kpt3d'], np.float64) for n in names]) @ np.swapaxes(rt[:, :, :3], -1, -2) + rt[:, None, :, 3]
    right = np.asarray(rec['is_right'], bool)
    per = [FR.sample_draws(cfg, 0, 0, i, True, P) for i in range(N)]
    draws = {k: np.stack([np.asarray(d[k]) for d in per]) for k in per[0]}
    plan = FR.crop_plan(rec['jt2d'], FR.project(kp, K), K, draws, P, cfg.bbox_scale_factor, is_right=right)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    minv, flip, colour = c(plan['minv']), c((~right).astype(np.uint8)), c(draws['colour'].astype(np.float32))
    erase, key = c(draws['erase'].astype(np.int32)), c(draws['key'].astype(np.uint32).view(np.int32))
    res, wh = FR.adaptive_res(plan['bbox_hand'], S)
    g, sigma, gmin = pipe_eval.tables['hand']
    jt, ob = c(plan['gt_jt2d']), c(plan['gt_obj2d'])
    bh, resd = c(np.concatenate([plan['bbox_hand'][:, :2], wh], -1)), c(res)
    bor = plan['bbox_obj_rect']
    mw = (bor[:, 2:] - bor[:, :2]).max(1)
    bo = c(np.concatenate([bor[:, :2], mw[:, None], mw[:, None]], -1))
    out = torch.empty((N, 3, P, P), device='cuda')
    hh, ho = torch.empty((N, 21, S, S), device='cuda'), torch.empty((N, 27, S, S), device='cuda')
    # the yardstick's grid: patch pixel centres -> normalised frame coordinates (align_corners=False), from the same inverse matrices
    Mi = plan['minv'].reshape(N, 2, 3)
    sx, sy = 2.0 / W, 2.0 / H
    A = np.zeros((N, 2, 3))
    A[:, 0, 0], A[:, 0, 1] = Mi[:, 0, 0] * P / 2 * sx, Mi[:, 0, 1] * P / 2 * sx
    A[:, 1, 0], A[:, 1, 1] = Mi[:, 1, 0] * P / 2 * sy, Mi[:, 1, 1] * P / 2 * sy
    ctr = (P - 1) / 2
    A[:, 0, 2] = (Mi[:, 0, 0] * ctr + Mi[:, 0, 1] * ctr + Mi[:, 0, 2] + 0.5) * sx - 1
    A[:, 1, 2] = (Mi[:, 1, 0] * ctr + Mi[:, 1, 1] * ctr + Mi[:, 1, 2] + 0.5) * sy - 1
    A = c(A.astype(np.float32))
    mean, std = torch.tensor(FR.IMG_MEAN, device='cuda').view(1, 3, 1, 1), torch.tensor(FR.IMG_STD, device='cuda').view(1, 3, 1, 1)
    left = c(~right)

    def torch_form():
        x = dev.permute(0, 3, 1, 2).float()
        grid = torch.nn.functional.affine_grid(A, (N, 3, P, P), align_corners=False)
        y = torch.nn.functional.grid_sample(x, grid, mode='bicubic', padding_mode='zeros', align_corners=False).round().clamp(0, 255)
        y = torch.where(left.view(N, 1, 1, 1), y.flip(-1), y)
        return (y / 255.0 - mean) / std

    forms = {
        'frame_patch (evaluation: warp, flip, normalise)': lambda: ops.frame_patch(dev, minv, P, flip=flip, out=out),
        'frame_patch (training: + colour, erasing)': lambda: ops.frame_patch(dev, minv, P, colour=colour, flip=flip, erase=erase, key=key, out=out),
        'heatmap_targets x 2 (hand adaptive + object square)': lambda: (ops.heatmap_targets(jt, bh, g, sigma, gmin, S, res=resd, out=hh),
                                                                        ops.heatmap_targets(ob, bo, g, sigma, gmin, S, left=flip, out=ho)),
        'host-to-device copy of the frames (pinned, 59.0 MB)': lambda: dev.copy_(host, non_blocking=True),
        'torch on the device: affine_grid + grid_sample(bicubic), flip, normalise': torch_form,
    }
    # the yardstick computes the same crop: levels agree with the kernel's up to rounding near half-integers and grid_sample's fp32 coordinates
    ours = ops.frame_patch(dev, minv, P, flip=flip)
    theirs = torch_form()
    lv = lambda t: ((t * std + mean) * 255).round()
    d = (lv(ours) - lv(theirs)).abs()
    say(f'frames_bench: {N} frames {W} x {H} -> {P}; levels of the kernel against the torch form: {float((d == 0).float().mean()) * 100:.2f} % equal, '
        f'{float((d > 1).float().mean()) * 100:.3f} % differ by more than 1, largest {int(d.max())}')
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(REPS):
        for k, f in forms.items():
            t[k].append(timed(f))
    for k, v in t.items():
        say(f'  {k}: {statistics.median(v):9.1f} us  ({min(v):.1f} .. {max(v):.1f})')
    px = N * P * P
    say(f'  by count: frame_patch writes {px * 12 / 1e6:.1f} MB and reads at most {N * H * W * 3 / 1e6:.1f} MB; the two heat-map launches write {N * 48 * S * S * 4 / 1e6:.1f} MB')
    for name, pipe in (('evaluation', pipe_eval), ('training', pipe_train)):
        pipe(host, recs)
        torch.cuda.synchronize()
        w = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            pipe(host, recs)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            w.append(((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3))
        say(f'  FramePipeline call, {name}: host returns after {statistics.median([a for a, _ in w]):.2f} ms, batch complete after '
            f'{statistics.median([b for _, b in w]):.2f} ms (wall clock, {N} frames from pinned memory)')
    if args.eval:
        from vpho_amd.trainer import Trainer
        tr = Trainer(cfg)
        cfg.num_batches = max(int(cfg.num_batches), 16)                              # 512 images: a pass of 128 is mostly warm-up
        bs, nb = cfg.eval_batch_size, cfg.num_batches
        big = FR.synthetic_frames(bs * nb, tr.assets, seed=0, size=(W, H))
        cached = [big[i] for i in range(len(big))]
        loader = FR.FrameLoader(cached, bs, FR.FramePipeline(cfg, tr.assets, tr.device, train=False, seed=0))
        rates = {'frames': [], 'synthetic batches': []}
        for _ in range(3):
            for k, ld in (('frames', loader), ('synthetic batches', None)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows = tr.eval(ld)
                torch.cuda.synchronize()
                rates[k].append(rows.shape[0] / (time.perf_counter() - t0))
        for k, v in rates.items():
            say(f'  Trainer.eval, {bs * nb} images in batches of {bs}, {k}: {statistics.median(v):.1f} images/s ({min(v):.1f} .. {max(v):.1f}; the first pass includes warm-up)')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""Photometric augmentation on the device: the host side of csrc/photo.hip (``ops.photo_*``).

The reference's ``ImageAugmentor`` (lib/dataset/base.py:349-397) composes A.CLAHE, A.RGBShift, A.ColorJitter, A.AdvancedBlur and
A.MotionBlur.  ``frames.hip`` has the RGB shift, brightness and saturation; this module adds CLAHE, contrast, hue and the two blurs as
this project's own rules -- neither albumentations nor OpenCV is reproduced bit for bit, and none is claimed to be.
It is imported only when one of the new gates can fire (``frames.photo_can_fire``); with the default flags nothing here runs.

Random draws: sample ``index`` of epoch ``epoch`` takes its numbers from a SECOND generator, ``np.random.default_rng((seed, epoch,
index, 1))``, so the 15 draws of ``frames.sample_draws`` keep their positions.  All are U(0,1)-based and all are always taken, whatever
the gates say, in this order (``photo_draws``):
  1 CLAHE gate, 2 clip limit U(clahe_clip_limit), 3 contrast factor U(jitter_contrast), 4 hue shift U(jitter_hue),
  5 blur gate, 6 blur size (u -> the odd sizes of blur_limit), 7 sigma x, 8 sigma y U(sigma_limit), 9 angle U(-90, 90) degrees,
  10 beta U(0.5, 8), 11-59 the 7 x 7 noise matrix U(0.9, 1.1) row-major,
  60 motion gate, 61 motion size (u -> the odd sizes of motion_blur_limit), 62 motion cell (u -> a cell of the K x K grid but the centre).
Contrast and hue apply when draw 10 of stream 1 (the colour-jitter gate) fired: the reference's ColorJitter is one transform with one p.
"""
import math

import numpy as np
import torch

TILES = 8                 # CLAHE: an 8 x 8 grid of tiles
KMAX = 7                  # the largest filter the kernel's halo holds
IDENTITY = np.zeros(KMAX * KMAX, np.float32)
IDENTITY[0] = 1.0         # a gate that is off: the 1 x 1 kernel [1]


def photo_can_fire(cfg):
    """True when a flag lets one of the new stages fire (the same rule as ``frames.photo_can_fire``)"""
    return bool(cfg.clahe_p > 0 or tuple(cfg.jitter_contrast) != (1, 1) or tuple(cfg.jitter_hue) != (0, 0) or cfg.blur_p > 0 or cfg.motion_blur_p > 0)


# ------------------------------------------------------------------------------------------------------------------ CLAHE, host rules
def clahe_clip(clip_limit, tw):
    """the clip COUNT of a tile of tw x tw pixels: max(1, int(clip_limit * tw * tw / 256)); a limit below 1 or not finite is refused"""
    if not (math.isfinite(clip_limit) and clip_limit >= 1):
        raise ValueError(f'CLAHE: clip_limit {clip_limit} must be finite and >= 1')
    return max(1, int(float(clip_limit) * tw * tw / 256))


def clahe_lut(hist, clip):
    """The LUT of one tile from its 256-bin histogram, in integers only (the rule of OpenCV's CLAHE_CalcLut_Body): counts above ``clip``
    are cut off, excess // 256 goes to every bin, the residual one count each to bins 0, step, 2 step, ... (step = max(256 // residual,
    1)); lut[i] = 255 * cumsum[i] / area rounded half to even.  The kernel does the same; this is the rule written down on the host."""
    h = np.asarray(hist, np.int64).copy()
    if h.shape != (256,) or (h < 0).any() or clip < 1:
        raise ValueError('clahe_lut: a 256-bin histogram of counts and a clip count >= 1')
    area = int(h.sum())
    excess = int(np.maximum(h - clip, 0).sum())
    h = np.minimum(h, clip)
    batch, resid = divmod(excess, 256)
    h += batch
    if resid:
        step = max(256 // resid, 1)
        h[np.arange(resid) * step] += 1
    num = 255 * np.cumsum(h)
    q, r = num // area, num % area
    q += (2 * r > area) | ((2 * r == area) & (q % 2 == 1))
    return q.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ filter kernels
def _odd_sizes(limit, name):
    lo, hi = int(limit[0]), int(limit[1])
    sizes = [k for k in range(lo, hi + 1) if k % 2 == 1]
    if not sizes or sizes[0] < 1 or sizes[-1] > KMAX:
        raise ValueError(f'--{name} {lo} {hi}: needs an odd size in 1..{KMAX} and none beyond')
    return sizes


def blur_kernel(K, sigma_x, sigma_y, angle_deg, beta, noise):
    """A.AdvancedBlur's generalised normal as a (49,) fp32 row (K * K weights row-major in front): exp(-0.5 * (g^T Sigma^-1 g) ** beta)
    on the grid -(K // 2) .. K // 2 with Sigma = U diag(sx^2, sy^2) U^T, U the rotation by the angle, times the K x K top-left corner
    of the 7 x 7 ``noise`` matrix, normalised to sum 1 in fp64 and rounded to fp32 once."""
    check_size(K)
    noise = np.asarray(noise, np.float64).reshape(KMAX, KMAX)
    if not (all(math.isfinite(v) for v in (sigma_x, sigma_y, angle_deg, beta)) and sigma_x > 0 and sigma_y > 0 and beta > 0 and np.isfinite(noise).all()):
        raise ValueError(f'blur_kernel: sigma ({sigma_x}, {sigma_y}), angle {angle_deg}, beta {beta} or the noise is not finite and positive')
    a = math.radians(angle_deg)
    U = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    inv = np.linalg.inv(U @ np.diag([sigma_x ** 2, sigma_y ** 2]) @ U.T)
    c = np.arange(K, dtype=np.float64) - K // 2
    g = np.stack(np.meshgrid(c, c, indexing='xy'), -1)                             # [row][col] = (x, y)
    k = np.exp(-0.5 * np.einsum('yxi,ij,yxj->yx', g, inv, g) ** beta) * noise[:K, :K]
    out = np.zeros(KMAX * KMAX, np.float32)
    out[:K * K] = (k / k.sum()).astype(np.float32).reshape(-1)
    return out


def motion_cells(K, cell):
    """the cells (row, col) of our centred motion line: the 8-connected line from the centre to ``cell`` (index into the K * K - 1 cells
    that are not the centre, row-major), its mirror image through the centre, and the centre.  Step i of m = max(|dx|, |dy|) lies at
    round-half-away(i * d / m) in each coordinate, in integers."""
    check_size(K)
    if K == 1:
        return [(0, 0)]
    if not 0 <= cell < K * K - 1:
        raise ValueError(f'motion_cells: cell {cell} outside the {K * K - 1} cells of a {K} x {K} grid without its centre')
    c = K // 2
    flat = cell if cell < c * K + c else cell + 1
    dy, dx = flat // K - c, flat % K - c
    m = max(abs(dx), abs(dy))
    rnd = lambda q: (1 if q >= 0 else -1) * ((2 * abs(q) + m) // (2 * m))
    cells = set()
    for i in range(m + 1):
        oy, ox = rnd(i * dy), rnd(i * dx)
        cells.add((c + oy, c + ox))
        cells.add((c - oy, c - ox))
    return sorted(cells)


def motion_kernel(K, cell):
    """(49,) fp32: 1 / count on every cell of ``motion_cells``"""
    cells = motion_cells(K, cell)
    k = np.zeros((K, K), np.float32)
    for y, x in cells:
        k[y, x] = np.float32(1.0 / len(cells))
    out = np.zeros(KMAX * KMAX, np.float32)
    out[:K * K] = k.reshape(-1)
    return out


def check_size(K):
    if not (isinstance(K, (int, np.integer)) and 1 <= K <= KMAX and K % 2 == 1):
        raise ValueError(f'filter size {K}: must be an odd integer in 1..{KMAX}')


def check_kernel(k, K):
    """refuses what the device must not get: a size that is not odd in 1..7, a weight that is not finite, a sum off 1 by more than 1e-6"""
    check_size(K)
    k = np.asarray(k)
    if k.shape != (KMAX * KMAX,) or k.dtype != np.float32:
        raise ValueError(f'filter kernel: a ({KMAX * KMAX},) float32 row, got {k.dtype} {k.shape}')
    w = k[:K * K].astype(np.float64)
    if not np.isfinite(w).all() or abs(w.sum() - 1.0) > 1e-6:
        raise ValueError(f'filter kernel {K} x {K}: weights must be finite and sum to 1 within 1e-6 (sum {w.sum()!r})')


# ------------------------------------------------------------------------------------------------------------------ draws
def photo_draws(cfg, seed, epoch, index, jitter_gate):
    """Stream 2 of ONE training sample (module docstring) -> dict: clip_limit (0.0 = CLAHE off), contrast (1.0 = none), hue (0.0 = none),
    k1 / K1 the blur kernel, k2 / K2 the motion kernel (the 1 x 1 kernel [1] when the gate is off).  ``jitter_gate``: whether the
    colour-jitter gate of stream 1 fired."""
    blur_sizes, motion_sizes = _odd_sizes(cfg.blur_limit, 'blur_limit'), _odd_sizes(cfg.motion_blur_limit, 'motion_blur_limit')
    r = np.random.default_rng((int(seed), int(epoch), int(index), 1))
    pick = lambda u, items: items[min(int(u * len(items)), len(items) - 1)]
    out = dict(clip_limit=0.0, contrast=np.float32(1), hue=np.float32(0), k1=IDENTITY.copy(), K1=1, k2=IDENTITY.copy(), K2=1)
    gate, limit = r.uniform(0, 1), r.uniform(*cfg.clahe_clip_limit)
    if gate < cfg.clahe_p:
        clahe_clip(limit, 1)                                                       # refuses a limit below 1
        out['clip_limit'] = float(limit)
    contrast, hue = r.uniform(*cfg.jitter_contrast), r.uniform(*cfg.jitter_hue)
    if jitter_gate:
        if not (math.isfinite(contrast) and contrast >= 0 and math.isfinite(hue) and abs(hue) <= 0.5):
            raise ValueError(f'--jitter_contrast / --jitter_hue: factor {contrast} must be >= 0 and shift {hue} within [-0.5, 0.5]')
        out['contrast'], out['hue'] = np.float32(contrast), np.float32(hue)
    gate, K = r.uniform(0, 1), pick(r.uniform(0, 1), blur_sizes)
    sx, sy, angle, beta, noise = r.uniform(*cfg.sigma_limit), r.uniform(*cfg.sigma_limit), r.uniform(-90, 90), r.uniform(0.5, 8), r.uniform(0.9, 1.1, 49)
    if gate < cfg.blur_p:
        out['k1'], out['K1'] = blur_kernel(K, sx, sy, angle, beta, noise), K
    gate, K, u = r.uniform(0, 1), pick(r.uniform(0, 1), motion_sizes), r.uniform(0, 1)
    if gate < cfg.motion_blur_p and K > 1:
        out['k2'], out['K2'] = motion_kernel(K, min(int(u * (K * K - 1)), K * K - 2)), K
    return out


# ------------------------------------------------------------------------------------------------------------------ the launches
def photo_patch(ops, frames, minv, patch, colour, params, flip=None, erase=None, key=None):
    """The training crop with every stage: levels, CLAHE, colour, the two filters, mirror, normalisation, erasing -> (n,3,P,P) fp32.

    frames (n,H,W,3) uint8 and minv (n,6) fp64 on the device; colour (n,5) fp32 device tensor or None; ``params``: dict of host arrays
    clip_limit (n), contrast (n), hue (n), k1 (n,49), K1 (n), k2 (n,49), K2 (n) (stacked ``photo_draws``); flip / erase / key as
    ``ops.frame_patch`` takes them.  Everything is checked here, on the host, before the first launch.  Stages nobody in the batch
    takes are not launched."""
    n, P, dev = int(frames.shape[0]), int(patch), frames.device
    limits = np.asarray(params['clip_limit'], np.float64).reshape(n)
    if (limits != 0).any() and P % TILES:
        raise ValueError(f'CLAHE: the {TILES} x {TILES} tile grid needs a patch size that is a multiple of {TILES}, got {P}')
    clip = np.array([clahe_clip(c, P // TILES) if c != 0 else 0 for c in limits], np.int32)
    contrast, hue = np.asarray(params['contrast'], np.float32).reshape(n), np.asarray(params['hue'], np.float32).reshape(n)
    if not (np.isfinite(contrast).all() and (contrast >= 0).all() and np.isfinite(hue).all() and (np.abs(hue) <= 0.5).all()):
        raise ValueError('photo_patch: contrast factors must be finite and >= 0, hue shifts within [-0.5, 0.5]')
    k1, k2 = np.ascontiguousarray(params['k1'], np.float32).reshape(n, KMAX * KMAX), np.ascontiguousarray(params['k2'], np.float32).reshape(n, KMAX * KMAX)
    K1, K2 = np.asarray(params['K1']).reshape(n), np.asarray(params['K2']).reshape(n)
    for i in range(n):
        check_kernel(k1[i], int(K1[i]))
        check_kernel(k2[i], int(K2[i]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
    levels = ops.photo_levels(frames, minv, P)
    if clip.any():
        l8, lut, clipd = ops.photo_clahe_lut(levels, clip)
        ops.photo_clahe_apply(levels, clipd, l8, lut, out=levels)
    cdev = up(contrast) if (contrast != 1).any() else None
    hdev = up(hue) if (hue != 0).any() else None
    if colour is not None or cdev is not None or hdev is not None:
        sums = ops.photo_grey_sum(levels, colour) if cdev is not None else None
        ops.photo_colour(levels, colour, cdev, hdev, sums, out=levels)
    return ops.photo_filter(levels, up(k1), K1.astype(np.int32), up(k2), K2.astype(np.int32), flip=flip, erase=erase, key=key)

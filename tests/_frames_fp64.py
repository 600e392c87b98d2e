"""float64 numpy restatements of what csrc/frames.hip computes (tests/test_frames_cpu.py, tests/test_gpu_frames.py).  Written from the
header's description, not from the kernel: the warp, the colour stages, the normalisation, the half-pixel-centre bilinear resize,
Philox4x32-10 and Box-Muller."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def cubic_weights(t, A=-0.75):
    """Keys' cubic convolution weights of the taps at floor - 1 .. floor + 2, t = the fraction: (..., 4)"""
    def near(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def far(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], -1)


def warp_levels(frame, minv, P):
    """frame (H,W,3) uint8, minv (6,) -> (P,P,3) float64 UNROUNDED bicubic values of the inverse mapping, constant border 0"""
    H, W, _ = frame.shape
    y, x = np.mgrid[0:P, 0:P].astype(np.float64)
    sx = minv[0] * x + minv[1] * y + minv[2]
    sy = minv[3] * x + minv[4] * y + minv[5]
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = cubic_weights(sx - fx), cubic_weights(sy - fy)
    pad = np.zeros((H + 8, W + 8, 3))
    pad[4:-4, 4:-4] = frame
    ix, iy = np.clip(fx, -3, W + 1).astype(np.int64), np.clip(fy, -3, H + 1).astype(np.int64)
    inside = (fx == ix) & (fy == iy)                                                      # beyond the clip every tap is outside anyway
    out = np.zeros((P, P, 3))
    for j in range(4):
        for i in range(4):
            out += (wy[..., j] * wx[..., i])[..., None] * pad[iy + j - 1 + 4, ix + i - 1 + 4]
    return np.where(inside[..., None], out, 0.0)


def to_level(v):
    return np.clip(np.rint(v), 0, 255)


def colour_stages(levels, colour):
    """integer levels (...,3) float64, colour = (dr, dg, db, b, s) as the fp32 values the kernel gets -> list of the UNROUNDED values of
    the stages (shift, brightness, gray (...,1), saturation), each computed from the rounded result of the one before"""
    c = np.asarray(colour, np.float32).astype(np.float64)
    raw = []
    v = levels + c[:3]
    raw.append(v)
    v = to_level(v) * c[3]
    raw.append(v)
    v = to_level(v)
    gray = (0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])[..., None]
    raw.append(gray)
    v = c[4] * v + (1 - c[4]) * to_level(gray)
    raw.append(v)
    return raw


def near_half(v, eps=1e-3):
    """True where a value lies within eps of a half-integer (where rounding may fall either way)"""
    return np.abs(v - np.floor(v) - 0.5) <= eps


def normalise_f32(levels):
    """the reference's three fp32 operations on integer levels (...,3)"""
    return (levels.astype(np.float32) / np.float32(255.0) - MEAN) / STD


def denormalise(rgb):
    """(...,3) normalised fp32 -> the integer level it came from (exact: neighbouring levels are 0.017 apart)"""
    return np.rint((rgb.astype(np.float64) * STD.astype(np.float64) + MEAN.astype(np.float64)) * 255.0)


def resize_linear(src, S):
    """(J, h, w) -> (J, S, S): bilinear, source of cell d = (d + 0.5) * size / S - 0.5, taps clamped to the edge"""
    J, h, w = src.shape

    def taps(n):
        f = (np.arange(S) + 0.5) * n / S - 0.5
        fl = np.floor(f)
        return np.clip(fl, 0, n - 1).astype(int), np.clip(fl + 1, 0, n - 1).astype(int), f - fl
    x0, x1, tx = taps(w)
    y0, y1, ty = taps(h)
    s = src.astype(np.float64)
    top = s[:, y0][:, :, x0] * (1 - tx) + s[:, y0][:, :, x1] * tx
    bot = s[:, y1][:, :, x0] * (1 - tx) + s[:, y1][:, :, x1] * tx
    return top * (1 - ty)[None, :, None] + bot * ty[None, :, None]


def philox4x32_10(counter, key):
    """counter: 4 ints, key: 2 ints -> 4 ints (python integers: no overflow to think about)"""
    c, k = [int(v) & 0xFFFFFFFF for v in counter], [int(v) & 0xFFFFFFFF for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def unit23(w):
    return ((int(w) >> 9) + 0.5) / 8388608.0


def box_muller(a, b):
    r = np.sqrt(-2.0 * np.log(unit23(a)))
    return r * np.cos(2 * np.pi * unit23(b)), r * np.sin(2 * np.pi * unit23(b))


def erase_normals(x, y, P, key):
    """the three channel values of an erased output pixel"""
    w = philox4x32_10((y * P + x, 0, 0, 0), key)
    z0, z1 = box_muller(w[0], w[1])
    z2, _ = box_muller(w[2], w[3])
    return np.array([z0, z1, z2])

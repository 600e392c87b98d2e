"""NumPy referee of csrc/photo.hip (tests/test_photo_cpu.py, tests/test_gpu_photo.py), written from the header's description and
independently of vpho_amd/photo.py: CLAHE with per-tile Python loops and Lab in float64, the fp32 colour stages and the two filters
emulated with np.float32 one operation at a time (numpy rounds every float32 operation once, as the kernel's uncontracted code does)."""
import numpy as np

F = np.float32


def level(v):
    """round half to even, clamp to 0..255; keeps the dtype"""
    return np.clip(np.rint(v), 0, 255)


# ---------------------------------------------------------------------------------------------------------------------- Lab
M_RGB2XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
M_XYZ2RGB = np.array([[3.240479, -1.53715, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])
WHITE = np.array([0.950456, 1.0, 1.088754])


def _f(t):
    return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)


def _finv(f):
    c = f * f * f
    return np.where(c > 0.008856, c, (f - 16.0 / 116.0) / 7.787)


def rgb_to_fxyz(levels):
    """(...,3) integer levels -> f(X/Xn), f(Y), f(Z/Zn) in float64, sums in the kernel's order ((a + b) + c)"""
    c = np.asarray(levels, np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4))
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    xyz = [(M_RGB2XYZ[i, 0] * r + M_RGB2XYZ[i, 1] * g) + M_RGB2XYZ[i, 2] * b for i in range(3)]
    return _f(xyz[0] / WHITE[0]), _f(xyz[1]), _f(xyz[2] / WHITE[2])


def l8_raw(levels):
    """the UNROUNDED L * 255 / 100 in float64"""
    _, fY, _ = rgb_to_fxyz(levels)
    return (116.0 * fY - 16.0) * 255.0 / 100.0


def lab_return(levels, l8_new):
    """levels with L replaced by l8_new * 100 / 255, the pixel's own a and b kept: the UNROUNDED 255 * sRGB values, float64"""
    fX, fY, fZ = rgb_to_fxyz(levels)
    a, b = 500.0 * (fX - fY), 200.0 * (fY - fZ)
    L = np.asarray(l8_new, np.float64) * 100.0 / 255.0
    gY = (L + 16.0) / 116.0
    gX, gZ = gY + a / 500.0, gY - b / 200.0
    X, Y, Z = _finv(gX) * WHITE[0], _finv(gY), _finv(gZ) * WHITE[2]
    out = []
    for i in range(3):
        c = (M_XYZ2RGB[i, 0] * X + M_XYZ2RGB[i, 1] * Y) + M_XYZ2RGB[i, 2] * Z
        with np.errstate(invalid='ignore'):
            s = np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 0.0), 1.0 / 2.4) - 0.055)
        out.append(255.0 * s)
    return np.stack(out, -1)


# ---------------------------------------------------------------------------------------------------------------------- CLAHE
def clip_count(clip_limit, tw):
    return max(1, int(clip_limit * tw * tw / 256))


def round_half_even_div(num, den):
    """integers: num / den rounded half to even"""
    q, r = divmod(int(num), int(den))
    if 2 * r > den or (2 * r == den and q % 2 == 1):
        q += 1
    return q


def tile_lut(tile, clip):
    """one tile (any shape) of L8 values -> its 256-entry LUT, plain Python integers, a loop per step of the rule"""
    vals = [int(v) for v in np.asarray(tile).reshape(-1)]
    area = len(vals)
    hist = [0] * 256
    for v in vals:
        hist[v] += 1
    excess = 0
    for i in range(256):
        if hist[i] > clip:
            excess += hist[i] - clip
            hist[i] = clip
    batch = excess // 256
    residual = excess - batch * 256
    for i in range(256):
        hist[i] += batch
    if residual:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            hist[i] += 1
            i += step
            residual -= 1
    lut, run = [], 0
    for i in range(256):
        run += hist[i]
        lut.append(round_half_even_div(255 * run, area))
    return np.array(lut, np.int64)


def clahe_luts(l8, clip):
    """(P,P) L8 plane -> (64,256) LUTs of the 8 x 8 tiles, tile ty * 8 + tx"""
    P = l8.shape[0]
    tw = P // 8
    return np.stack([tile_lut(l8[ty * tw:(ty + 1) * tw, tx * tw:(tx + 1) * tw], clip) for ty in range(8) for tx in range(8)])


def clahe_interpolate(l8, luts):
    """(P,P) L8 and (64,256) LUTs -> (P,P) interpolated L8', a Python loop per pixel, integers only"""
    P = l8.shape[0]
    tw = P // 8
    out = np.zeros((P, P), np.int64)
    for y in range(P):
        ay = 2 * y + 1 - tw
        fy = ay // (2 * tw)                                  # Python's floor division
        ya = ay - fy * 2 * tw
        ty1, ty2 = min(max(fy, 0), 7), min(max(fy + 1, 0), 7)
        for x in range(P):
            ax = 2 * x + 1 - tw
            fx = ax // (2 * tw)
            xa = ax - fx * 2 * tw
            tx1, tx2 = min(max(fx, 0), 7), min(max(fx + 1, 0), 7)
            v = int(l8[y, x])
            num = (2 * tw - xa) * (2 * tw - ya) * int(luts[ty1 * 8 + tx1, v]) + xa * (2 * tw - ya) * int(luts[ty1 * 8 + tx2, v]) + \
                (2 * tw - xa) * ya * int(luts[ty2 * 8 + tx1, v]) + xa * ya * int(luts[ty2 * 8 + tx2, v])
            out[y, x] = round_half_even_div(num, 4 * tw * tw)
    return out


# ---------------------------------------------------------------------------------------------------------------------- colour (fp32)
def shift_brightness(levels, colour):
    """(...,3) integer levels -> float32 levels after v + d and v * b"""
    c = np.asarray(colour, F)
    v = level(np.asarray(levels, F) + c[:3])
    return level(v * c[3])


def grey(v):
    return level((F(0.299) * v[..., 0] + F(0.587) * v[..., 1]) + F(0.114) * v[..., 2])


def grey_mean(v):
    """the integer mean (2 sum + N) // (2 N) of the grey levels of a float32 image (P,P,3), and the sum"""
    g = grey(v)
    total, N = int(g.astype(np.int64).sum()), g.size
    return (2 * total + N) // (2 * N), total


def contrast(v, f, m):
    f = F(f)
    g1 = (F(1) - f) * F(m)
    return level(f * v + g1)


def saturation(v, s):
    s = F(s)
    g1 = ((F(1) - s) * grey(v))[..., None]
    return level(s * v + g1)


def hue(v, delta):
    """torchvision's _rgb2hsv / _hsv2rgb in float32 on v / 255, h + delta - floor(h + delta) between them"""
    delta = F(delta)
    if delta == 0:
        return v
    r, g, b = (v[..., k] / F(255) for k in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    eq = maxc == minc
    cr = maxc - minc
    sat = cr / np.where(eq, F(1), maxc)
    div = np.where(eq, F(1), cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, (F(2) + rc) - bc, (F(4) + gc) - rc)).astype(F)
    h = np.fmod(h / F(6) + F(1), F(1))
    hs = h + delta
    h = hs - np.floor(hs)
    h6 = h * F(6)
    fl = np.floor(h6)
    f = h6 - fl
    i = fl.astype(np.int64) % 6
    one = F(1)
    clamp = lambda a: np.clip(a, F(0), F(1))
    p = clamp(maxc * (one - sat))
    q = clamp(maxc * (one - sat * f))
    t = clamp(maxc * (one - sat * (one - f)))
    R = np.choose(i, [maxc, q, p, p, t, maxc])
    G = np.choose(i, [t, maxc, maxc, q, p, p])
    B = np.choose(i, [p, p, t, maxc, maxc, q])
    out = np.stack([level(R * F(255)), level(G * F(255)), level(B * F(255))], -1)
    assert out.dtype == F
    return out


def colour_chain(levels, colour=None, f=None, delta=None):
    """the kernel's chain on one image (P,P,3) of integer levels -> (float32 levels, grey sum or None)"""
    v = np.asarray(levels, F)
    total = None
    if colour is not None:
        v = shift_brightness(v, colour)
    if f is not None:
        m, total = grey_mean(v)
        v = contrast(v, f, m)
    if colour is not None:
        v = saturation(v, np.asarray(colour, F)[4])
    if delta is not None:
        v = hue(v, delta)
    assert v.dtype == F
    return v, total


# ---------------------------------------------------------------------------------------------------------------------- filters (fp32)
def filter2d(img, k):
    """(P,P,C) float32 integer levels, k (K,K) float32: correlation with reflect-101 borders, accumulated from 0 in row-major tap order,
    one float32 multiply and one float32 add per tap, then rounded and clamped"""
    K = k.shape[0]
    h = K // 2
    P = img.shape[0]
    pad = np.pad(img, ((h, h), (h, h), (0, 0)), mode='reflect') if h else img
    acc = np.zeros_like(img, dtype=F)
    for ky in range(K):
        for kx in range(K):
            acc = acc + F(k[ky, kx]) * pad[ky:ky + P, kx:kx + P]
    assert acc.dtype == F
    return level(acc)


def finish(v, flip):
    """mirror, then the three float32 operations of the normalisation -> (3,P,P)"""
    mean, std = np.array([0.485, 0.456, 0.406], F), np.array([0.229, 0.224, 0.225], F)
    if flip:
        v = v[:, ::-1]
    return np.ascontiguousarray(((v / F(255) - mean) / std).transpose(2, 0, 1))

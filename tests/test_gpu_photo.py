"""csrc/photo.hip through ``ops.photo_*`` and the front end built on it (vpho_amd/photo.py, FramePipeline).

Levels: equal to the de-normalised ``ops.frame_patch`` everywhere.  CLAHE: the L8 plane equals the referee's (tests/_photo_fp64.py)
wherever float64 L * 255 / 100 is farther than 1e-9 from a half-integer -- the cases are chosen so that the referee alone finds no such
pixel; given equal L8 the 64 LUTs and the interpolated plane are bit-equal; after the return trip through Lab the levels are equal outside
a 1e-3 band about half-integers, which holds at most 1 % of the values.  Contrast and hue: the integer mean exact, the levels bit-equal
to the np.float32 restatement.  Filters: bit-equal to the np.float32 referee, tap order and reflect-101 corners included.  A sample with
every new gate off equals ``ops.frame_patch`` bit for bit; the mirror comes after the directional filter; runs and batch compositions
repeat; refusals come before any launch.  End to end: the pipeline's dict, one ``Trainer.fit`` epoch, ``main.py`` in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _frames_fp64 as RF  # noqa: E402
import _photo_fp64 as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _ops():
    from vpho_amd import ops
    return ops


def _photo():
    from vpho_amd import photo
    return photo


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frames(n, H, W, seed):
    """textured frames: per channel a product of two sinusoids plus noise, as frames.synthetic_frames draws them"""
    r = np.random.default_rng(seed)
    out = np.zeros((n, H, W, 3), np.uint8)
    for s in range(n):
        ph = r.uniform(0, 2 * np.pi, (3, 2))
        f = np.stack([128 + 70 * np.outer(np.cos(np.arange(H) / r.uniform(5, 20) + ph[c, 1]), np.sin(np.arange(W) / r.uniform(5, 20) + ph[c, 0])) for c in range(3)], -1)
        out[s] = np.clip(np.rint(f) + r.integers(-24, 25, f.shape), 0, 255).astype(np.uint8)
    return out


def _minv(n, H, W, P, seed):
    """patch -> frame: a rotation and a scale about the frame centre, so that most of the frame shows and a corner lies outside it"""
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        ang, sc = r.uniform(-0.5, 0.5), P / H * r.uniform(0.8, 1.1)
        c, s = np.cos(ang) * sc, np.sin(ang) * sc
        A = np.array([[c, -s], [s, c]])
        t = np.array([P / 2, P / 2]) - A @ np.array([W / 2 + r.uniform(-3, 3), H / 2 + r.uniform(-3, 3)])
        rows.append(np.linalg.inv(np.concatenate([np.concatenate([A, t[:, None]], 1), [[0, 0, 1]]]))[:2].reshape(6))
    return np.stack(rows)


_LEVELS = {}


def _levels(n, H, W, P, seed=0):
    """levels (n,P,P,3) uint8 of ops.photo_levels on textured frames, on the host; computed once per case and never changed"""
    key = (n, H, W, P, seed)
    if key not in _LEVELS:
        frames, minv = _frames(n, H, W, seed), _minv(n, H, W, P, seed + 100)
        lev = _ops().photo_levels(_cuda(frames), _cuda(minv), P)
        torch.cuda.synchronize()
        _LEVELS[key] = (frames, minv, lev.cpu().numpy())
    return _LEVELS[key]


# ---------------------------------------------------------------------------------------------------------------------- levels
@pytest.mark.parametrize('n,H,W,P', [(1, 40, 56, 16), (3, 40, 56, 32), (3, 96, 128, 16), (1, 96, 128, 32)])
def test_levels_are_the_levels_of_frame_patch(n, H, W, P):
    ops = _ops()
    frames, minv, lev = _levels(n, H, W, P)
    rgb = ops.frame_patch(_cuda(frames), _cuda(minv), P).cpu().numpy().transpose(0, 2, 3, 1)          # no colour, no flip, no erase
    want = np.rint((rgb.astype(np.float64) * RF.STD.astype(np.float64) + RF.MEAN.astype(np.float64)) * 255)
    assert lev.dtype == np.uint8 and lev.shape == (n, P, P, 3)
    assert np.array_equal(lev.astype(np.float64), want), int((lev != want).sum())
    assert (lev == 0).all(-1).any() and lev.max() > 200                                    # a corner outside the frame, and texture
    # other transforms: a translation over the edge, an identity
    for m in (np.array([1.0, 0, -P / 2 + 0.3, 0, 1, 2.6]), np.array([1.0, 0, 0, 0, 1, 0])):
        mm = _cuda(np.repeat(m[None], n, 0))
        got = ops.photo_levels(_cuda(frames), mm, P).cpu().numpy()
        rgb = ops.frame_patch(_cuda(frames), mm, P).cpu().numpy().transpose(0, 2, 3, 1)
        assert np.array_equal(got.astype(np.float64), RF.denormalise(rgb))
    assert np.array_equal(ops.photo_levels(_cuda(frames), _cuda(np.repeat(np.array([[1.0, 0, 0, 0, 1, 0]]), n, 0)), P).cpu().numpy(), frames[:, :P, :P])
    assert tuple(ops.photo_levels(_cuda(frames[:0]), _cuda(minv[:0]), P).shape) == (0, P, P, 3)     # n == 0: no launch


# ---------------------------------------------------------------------------------------------------------------------- CLAHE
def _clahe_check(name, lev, limits):
    """lev (n,P,P,3) uint8 on the host, limits: the clip limit of every sample"""
    ops = _ops()
    n, P = lev.shape[:2]
    clip = [R.clip_count(c, P // 8) for c in limits]
    assert clip == [_photo().clahe_clip(c, P // 8) for c in limits]
    l8, lut, clipd = ops.photo_clahe_lut(_cuda(lev), clip)
    out, l8n = ops.photo_clahe_apply(_cuda(lev), clipd, l8, lut, want_l8=True)
    torch.cuda.synchronize()
    l8, lut, out, l8n = l8.cpu().numpy(), lut.cpu().numpy(), out.cpu().numpy(), l8n.cpu().numpy()
    for s in range(n):
        raw = R.l8_raw(lev[s])
        close = np.abs(raw - np.floor(raw) - 0.5) <= 1e-9
        assert int(close.sum()) == 0, f'{name}[{s}]: the referee alone finds {int(close.sum())} pixels within 1e-9 of a half-integer L8: choose another case'
        want8 = np.clip(np.rint(raw), 0, 255).astype(np.int64)
        assert np.array_equal(l8[s].astype(np.int64), want8), f'{name}[{s}]: {int((l8[s] != want8).sum())} L8 values differ'
        luts = R.clahe_luts(want8, clip[s])
        assert np.array_equal(lut[s].astype(np.int64), luts), f'{name}[{s}]: LUT entries differ in tiles {sorted(set(np.nonzero(lut[s] != luts)[0]))}'
        new8 = R.clahe_interpolate(want8, luts)
        assert np.array_equal(l8n[s].astype(np.int64), new8), f'{name}[{s}]: {int((l8n[s] != new8).sum())} interpolated values differ'
        back = R.lab_return(lev[s], new8)
        unsure = RF.near_half(back)
        share = float(unsure.mean())
        diff = np.abs(out[s].astype(np.float64) - R.level(back))
        print(f'PHOTO clahe {name}[{s}] P {P} clip {clip[s]}: L8 range {want8.min()}..{want8.max()} -> {new8.min()}..{new8.max()}, excluded share {share:.5f}, '
              f'mismatches outside the band {int((diff[~unsure] != 0).sum())}, largest inside {diff[unsure].max() if unsure.any() else 0:.0f}')
        assert share <= 0.01, f'{name}[{s}]: the referee alone puts {share:.4f} of the values within 1e-3 of a half-integer'
        assert not diff[~unsure].any() and diff.max() <= 1, f'{name}[{s}]: {int((diff[~unsure] != 0).sum())} levels differ outside the band, largest {diff.max()}'
    return out


@pytest.mark.parametrize('P,n,H,W', [(8, 3, 40, 56), (16, 3, 40, 56), (16, 1, 96, 128), (24, 3, 96, 128), (64, 3, 96, 128), (128, 3, 96, 128)])
def test_clahe_against_the_referee(P, n, H, W):
    """one launch holds the three clip limits (sample s takes limit s); up to P = 64 a tile has at most 64 pixels and the clip count is 1
    for every limit, at P = 128 it is 1, 2 and 4"""
    _, _, lev = _levels(n, H, W, P, seed=P)
    limits = (1.0, 2.5, 4.0)[:n] if n == 3 else (2.5,)
    out = _clahe_check(f'textured {H}x{W}', lev, limits)
    assert not np.array_equal(out, lev)


def test_clahe_at_256_on_a_ramp_and_on_a_constant_image():
    # the camera patch: tiles of 32 x 32, clip limit 4 -> clip 16
    _, _, lev = _levels(1, 96, 128, 256, seed=5)
    _clahe_check('textured 256', lev, (4.0,))
    # a grey ramp along the diagonal and a constant image, P = 64, clip limits 1 and 4.  (A ramp along x alone repeats each of its 64
    # values down a column, so one value near a half-integer is 1.6 % of the image; the colour (90, 140, 60) comes back with G =
    # 147.4998.  Both were set aside on the referee's figures alone.)
    y, x = np.mgrid[0:64, 0:64]
    ramp = np.repeat(np.rint(255 * (x + y) / 126).astype(np.uint8)[..., None], 3, 2)
    const = np.full((64, 64, 3), (120, 80, 200), np.uint8)
    out = _clahe_check('ramp, constant', np.stack([ramp, const]), (1.0, 4.0))
    assert (out[1] == out[1][0, 0]).all() and not np.array_equal(out[1][0, 0], const[0, 0])           # a constant image stays constant
    assert np.abs(out[0].astype(int) - out[0][..., 1:2].astype(int)).max() <= 1                         # grey stays grey, to a level


def test_clahe_leaves_a_sample_whose_gate_is_off_untouched():
    ops = _ops()
    _, _, lev = _levels(3, 40, 56, 16, seed=16)
    l8, lut, clipd = ops.photo_clahe_lut(_cuda(lev), [1, 0, 1])
    out = ops.photo_clahe_apply(_cuda(lev), clipd, l8, lut).cpu().numpy()
    alone = _clahe_check('gate on', lev[[0, 2]], (4.0, 4.0))
    assert np.array_equal(out[1], lev[1]) and np.array_equal(out[[0, 2]], alone)
    # in place: out may be the levels
    t = _cuda(lev)
    assert ops.photo_clahe_apply(t, clipd, l8, lut, out=t) is t and np.array_equal(t.cpu().numpy(), out)


# ---------------------------------------------------------------------------------------------------------------------- contrast and hue
@pytest.mark.parametrize('f', [0.6, 1.0, 1.3])
@pytest.mark.parametrize('delta', [-0.15, 0.0, 0.15])
def test_contrast_and_hue_are_bit_equal_to_the_float32_restatement(f, delta):
    ops = _ops()
    n, P = 3, 24
    _, _, lev = _levels(n, 96, 128, P, seed=24)
    colour = np.array([[17, -20, 6, 1.2514, 0.7301], [0, 0, 0, 0.6207, 1.2993], [-9, 3, 20, 1.0, 1.0]], F)      # shift, brightness, saturation
    fs, ds = np.full(n, f, F), np.full(n, delta, F)
    sums = ops.photo_grey_sum(_cuda(lev), _cuda(colour))
    out = ops.photo_colour(_cuda(lev), _cuda(colour), _cuda(fs), _cuda(ds), sums).cpu().numpy()
    bare_sums = ops.photo_grey_sum(_cuda(lev))
    bare = ops.photo_colour(_cuda(lev), None, _cuda(fs), _cuda(ds), bare_sums).cpu().numpy()         # contrast and hue alone
    only = ops.photo_colour(_cuda(lev), _cuda(colour)).cpu().numpy()                                   # today's chain
    for s in range(n):
        want, total = R.colour_chain(lev[s], colour[s], f, delta)
        assert int(sums[s]) == total, (s, int(sums[s]), total)                          # the integer sum, hence the integer mean, is exact
        assert np.array_equal(out[s].astype(F), want), f'sample {s}: {int((out[s] != want).sum())} levels differ, f {f}, delta {delta}'
        want, total = R.colour_chain(lev[s], None, f, delta)
        assert int(bare_sums[s]) == total and np.array_equal(bare[s].astype(F), want), s
        assert np.array_equal(only[s].astype(F), R.colour_chain(lev[s], colour[s])[0]), s
    if f == 1.0 and delta == 0.0:
        assert np.array_equal(out, only)                                                # factor 1 and shift 0 change nothing
    else:
        assert not np.array_equal(out, only)


def test_the_colour_stages_equal_frame_patch_when_nothing_new_is_on():
    ops = _ops()
    frames, minv, lev = _levels(3, 40, 56, 32)
    colour = np.array([[17, -20, 6, 1.2514, 0.7301], [0, 0, 0, 0.6207, 1.2993], [-9, 3, 20, 1.0, 1.0]], F)
    rgb = ops.frame_patch(_cuda(frames), _cuda(minv), 32, colour=_cuda(colour)).cpu().numpy().transpose(0, 2, 3, 1)
    got = ops.photo_colour(_cuda(lev), _cuda(colour)).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), RF.denormalise(rgb))


# ---------------------------------------------------------------------------------------------------------------------- filters
def _kernels(K, seed):
    """three K x K kernels: random positive weights (not symmetric), a delta in the top right corner, one-sided (the left column)"""
    r = np.random.default_rng(seed)
    rnd = r.uniform(0.1, 1.0, (K, K))
    rnd = (rnd / rnd.sum()).astype(F)
    delta = np.zeros((K, K), F)
    delta[0, K - 1] = 1
    side = np.zeros((K, K), F)
    side[:, 0] = F(1.0 / K)
    return [rnd, delta, side]


def _row(k):
    out = np.zeros(49, F)
    out[:k.size] = k.reshape(-1)
    return out


ONE = np.ones((1, 1), F)


@pytest.mark.parametrize('P', [8, 16, 32, 40])
def test_filters_are_bit_equal_to_the_float32_referee(P):
    """every pair of the batch is one sample: each K alone as the first and as the second filter (three kernel shapes), chained pairs,
    and the identity.  P = 8, 16: the halo exceeds the image; 32: one full tile; 40: four tiles, three of them cut"""
    ops = _ops()
    pairs = [(ONE, ONE)]
    for K in (3, 5, 7):
        for k in _kernels(K, K):
            pairs += [(k, ONE), (ONE, k)]
    a3, a5, a7 = _kernels(3, 13), _kernels(5, 15), _kernels(7, 17)
    pairs += [(a3[0], a5[0]), (a7[0], a7[0].T.copy()), (a5[1], a3[2]), (a7[2], a3[1]), (a7[1], a7[1]), (a5[0], a7[2])]
    n = len(pairs)
    r = np.random.default_rng(P)
    y, x = np.mgrid[0:P, 0:P]
    lev = np.clip(128 + 90 * np.sin(x[None, :, :, None] / 3.0 + r.uniform(0, 6, (n, 1, 1, 3))) * np.cos(y / 2.5)[None, :, :, None] + r.integers(-40, 41, (n, P, P, 3)), 0, 255).astype(np.uint8)
    flip = (np.arange(n) % 3 == 1).astype(np.uint8)
    k1, k2 = np.stack([_row(a) for a, _ in pairs]), np.stack([_row(b) for _, b in pairs])
    K1, K2 = [a.shape[0] for a, _ in pairs], [b.shape[0] for _, b in pairs]
    out = ops.photo_filter(_cuda(lev), _cuda(k1), K1, _cuda(k2), K2, flip=_cuda(flip))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == (n, 3, P, P)
    for s, (a, b) in enumerate(pairs):
        mid = R.filter2d(lev[s].astype(F), a)
        want = R.finish(R.filter2d(mid, b), bool(flip[s]))
        bad = _bits(out[s]) != _bits(want)
        assert not bad.any(), f'P {P} sample {s} (K {K1[s]}, {K2[s]}, flip {flip[s]}): {int(bad.sum())} values differ, first at {tuple(np.argwhere(bad)[0])}'
        for cy in (0, P - 1):
            for cx in (0, P - 1):                                                     # the reflect-101 corners, spelt out
                assert np.array_equal(_bits(out[s][:, cy, cx]), _bits(want[:, cy, cx])), (P, s, cy, cx)
    # a delta in the top right corner of the first filter reads the pixel K // 2 up and K // 2 to the right, reflected at the border
    s = 1 + 2                                                                          # K 3: (rnd, 1), (1, rnd), (delta, 1)
    assert K1[s] == 3 and pairs[s][0][0, 2] == 1 and not flip[s]
    got = RF.denormalise(out[s].transpose(1, 2, 0))
    assert np.array_equal(got[1:, :P - 1], lev[s][:P - 1, 1:]) and np.array_equal(got[0, :P - 1], lev[s][1, 1:]) and np.array_equal(got[1:, P - 1], lev[s][:P - 1, P - 2])


def test_the_filter_finish_is_the_finish_of_frame_patch():
    """identity kernels: mirror, normalisation and erasing equal ``ops.frame_patch`` bit for bit, the Philox normals included"""
    ops = _ops()
    n, P = 3, 40
    frames, minv, lev = _levels(n, 96, 128, P, seed=40)
    flip = np.array([0, 1, 1], np.uint8)
    erase = np.zeros((n, 4, 4), np.int32)
    erase[0, 0], erase[1, 0], erase[1, 1], erase[2, 3] = (3, 5, 30, 22), (0, 0, 9, 40), (33, 10, 40, 12), (10, 35, 25, 40)
    key = np.array([[1, 2], [0x7fffffff, -5], [123456789, 42]], np.int32)
    ident = np.repeat(_row(ONE)[None], n, 0)
    want = ops.frame_patch(_cuda(frames), _cuda(minv), P, flip=_cuda(flip), erase=_cuda(erase), key=_cuda(key)).cpu().numpy()
    got = ops.photo_filter(_cuda(lev), _cuda(ident), [1] * n, _cuda(ident), [1] * n, flip=_cuda(flip), erase=_cuda(erase), key=_cuda(key)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    plain = ops.photo_filter(_cuda(lev), _cuda(ident), [1] * n, _cuda(ident), [1] * n).cpu().numpy()
    assert (_bits(plain) != _bits(got)).any() and np.array_equal(_bits(plain), _bits(ops.frame_patch(_cuda(frames), _cuda(minv), P).cpu().numpy()))


# ---------------------------------------------------------------------------------------------------------------------- the whole path
def _params(n, **kw):
    PH = _photo()
    p = dict(clip_limit=np.zeros(n), contrast=np.ones(n, F), hue=np.zeros(n, F), k1=np.repeat(PH.IDENTITY[None], n, 0), K1=np.ones(n, np.int64),
             k2=np.repeat(PH.IDENTITY[None], n, 0), K2=np.ones(n, np.int64))
    for k, v in kw.items():
        for s, item in v.items():
            p[k][s] = item
    return p


def _full_case(P=32):
    PH = _photo()
    n = 4
    frames, minv, _ = _levels(n, 40, 56, P, seed=77)
    colour = np.array([[17, -20, 6, 1.2514, 0.7301], [0, 0, 0, 1, 1], [-9, 3, 20, 0.8, 1.1], [5, 5, -5, 1.1, 0.9]], F)
    flip = np.array([1, 0, 1, 0], np.uint8)
    erase = np.zeros((n, 4, 4), np.int32)
    erase[0, 0], erase[1, 1], erase[2, 0] = (2, 3, 20, 17), (10, 0, 31, 6), (0, 20, 12, 32)
    key = np.array([[11, 22], [33, 44], [55, 66], [77, 88]], np.int32)
    blur = PH.blur_kernel(5, 1.4, 0.5, 30.0, 1.7, np.random.default_rng(1).uniform(0.9, 1.1, 49))
    # samples 0 and 1: every new gate off (0 is a left hand with erasing); 2 and 3: everything on
    params = _params(n, clip_limit={2: 2.5, 3: 4.0}, contrast={2: F(0.7), 3: F(1.25)}, hue={2: F(0.1), 3: F(-0.12)}, k1={2: blur, 3: blur}, K1={2: 5, 3: 5},
                     k2={2: PH.motion_kernel(7, 3), 3: PH.motion_kernel(3, 0)}, K2={2: 7, 3: 3})
    return frames, minv, colour, flip, erase, key, params


def _run(frames, minv, P, colour, params, flip=None, erase=None, key=None, pick=None):
    pick = slice(None) if pick is None else pick
    dev = lambda a: None if a is None else _cuda(a[pick])
    out = _photo().photo_patch(_ops(), dev(frames), dev(minv), P, dev(colour), {k: np.asarray(v)[pick] for k, v in params.items()}, flip=dev(flip), erase=dev(erase),
                               key=dev(key))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_gates_off_in_a_mixed_batch_equal_frame_patch_bit_for_bit():
    ops, P = _ops(), 32
    frames, minv, colour, flip, erase, key, params = _full_case(P)
    out = _run(frames, minv, P, colour, params, flip, erase, key)
    today = ops.frame_patch(_cuda(frames), _cuda(minv), P, colour=_cuda(colour), flip=_cuda(flip), erase=_cuda(erase), key=_cuda(key)).cpu().numpy()
    assert np.array_equal(_bits(out[:2]), _bits(today[:2]))
    assert (_bits(out[2]) != _bits(today[2])).any() and (_bits(out[3]) != _bits(today[3])).any() and np.isfinite(out).all()
    # where a rectangle was erased both hold the same normals, whatever the colour stages did
    assert np.array_equal(_bits(out[2][:, 20:32, 0:12]), _bits(today[2][:, 20:32, 0:12]))
    # the samples that took every stage are the referee's chain on the device's own levels, outside the CLAHE band
    lev = ops.photo_levels(_cuda(frames), _cuda(minv), P).cpu().numpy()
    PH = _photo()
    s = 3                                                                              # no erasing, a right hand
    raw8 = R.l8_raw(lev[s])
    l8 = np.clip(np.rint(raw8), 0, 255).astype(np.int64)
    back = R.lab_return(lev[s], R.clahe_interpolate(l8, R.clahe_luts(l8, PH.clahe_clip(4.0, P // 8))))
    if not RF.near_half(back).any():                                                  # else a level may legitimately differ by one before the later stages
        v, _ = R.colour_chain(R.level(back), colour[s], params['contrast'][s], params['hue'][s])
        v = R.filter2d(R.filter2d(v, params['k1'][s][:25].reshape(5, 5)), params['k2'][s][:9].reshape(3, 3))
        assert np.array_equal(_bits(out[s]), _bits(R.finish(v, False)))


def test_the_mirror_comes_after_the_directional_filter():
    PH = _photo()
    P = 32
    frames, minv, _ = _levels(4, 40, 56, P, seed=77)
    two = lambda a: np.repeat(a[:1], 2, 0)
    diag = PH.motion_kernel(5, 0)                                                      # top left to bottom right
    params = _params(2, k2={0: diag, 1: diag}, K2={0: 5, 1: 5}, contrast={0: F(0.8), 1: F(0.8)})
    out = _run(two(frames), two(minv), P, None, params, flip=np.array([0, 1], np.uint8))
    assert np.array_equal(_bits(out[1]), _bits(out[0][:, :, ::-1]))
    # ... which is NOT the filter applied to the mirrored patch: that one blurs along the other diagonal
    anti = diag[:25].reshape(5, 5)[:, ::-1].reshape(-1)
    other = _run(two(frames), two(minv), P, None, _params(2, k2={0: _row(anti), 1: _row(anti)}, K2={0: 5, 1: 5}, contrast={0: F(0.8), 1: F(0.8)}),
                 flip=np.array([0, 1], np.uint8))
    assert not np.array_equal(_bits(other[1]), _bits(out[1]))


def test_runs_and_batch_compositions_repeat():
    P = 32
    frames, minv, colour, flip, erase, key, params = _full_case(P)
    a = _run(frames, minv, P, colour, params, flip, erase, key)
    b = _run(frames, minv, P, colour, params, flip, erase, key)
    assert np.array_equal(_bits(a), _bits(b))
    for pick in ([2], [3, 0], [1, 2, 3]):
        part = _run(frames, minv, P, colour, params, flip, erase, key, pick=pick)
        assert np.array_equal(_bits(part), _bits(a[pick])), pick
    # the grey sum at a size with many workgroups per image: 65 536 pixels, 64 adds per sample, the same bits every time
    _, _, lev = _levels(1, 96, 128, 256, seed=5)
    sums = [int(_ops().photo_grey_sum(_cuda(lev))[0]) for _ in range(3)]
    assert sums[0] == sums[1] == sums[2] == int(R.grey(lev[0].astype(F)).astype(np.int64).sum())


def test_refusals_come_before_any_launch():
    ops, PH = _ops(), _photo()
    VE = ops.VphoError
    _, _, lev = _levels(3, 40, 56, 16, seed=16)
    t = _cuda(lev)
    ident = _cuda(np.repeat(PH.IDENTITY[None], 3, 0))
    sentinel = torch.full((3, 3, 16, 16), 12345.0, device='cuda')
    lev20 = torch.zeros((3, 20, 20, 3), dtype=torch.uint8, device='cuda')
    calls = [lambda: ops.photo_clahe_lut(lev20, [1, 1, 1]),                            # P % 8
             lambda: ops.photo_clahe_lut(t, [1, -1, 1]), lambda: ops.photo_clahe_lut(t, [1, 1]), lambda: ops.photo_clahe_lut(t, [1.0, 1.0, 1.0]),
             lambda: ops.photo_clahe_lut(t.float(), [1, 1, 1]), lambda: ops.photo_clahe_lut(t[:, :, :8], [1, 1, 1]),
             lambda: ops.photo_filter(t, ident, [1, 2, 1], ident, [1, 1, 1], out=sentinel),           # an even size
             lambda: ops.photo_filter(t, ident, [1, 1, 1], ident, [9, 1, 1], out=sentinel),           # beyond the halo
             lambda: ops.photo_filter(t, ident, [1, 1, 1], ident, [1, 1, 0], out=sentinel),
             lambda: ops.photo_filter(t, ident[:, :9], [1, 1, 1], ident, [1, 1, 1], out=sentinel),
             lambda: ops.photo_filter(t, ident, [1, 1, 1], ident, [1, 1, 1], erase=torch.zeros((3, 4, 4), dtype=torch.int32, device='cuda'), out=sentinel),
             lambda: ops.photo_filter(t, ident, [1, 1, 1], ident, [1, 1, 1], out=sentinel[:2]),
             lambda: ops.photo_colour(t, contrast=torch.ones(3, device='cuda')),                      # contrast without the sums
             lambda: ops.photo_colour(t, colour=torch.ones((3, 4), device='cuda')),
             lambda: ops.photo_grey_sum(torch.from_numpy(lev.copy())),                                      # host memory
             lambda: ops.photo_levels(t, torch.zeros((3, 5), dtype=torch.float64, device='cuda'), 16)]
    for i, call in enumerate(calls):
        with pytest.raises(VE):
            call()
            pytest.fail(f'call {i} was not refused')
    torch.cuda.synchronize()
    assert bool((sentinel == 12345.0).all())
    # the host side of the whole path: nothing is launched when a parameter is out of range
    frames, minv, colour, flip, erase, key, params = _full_case(32)
    seen = []

    class Spy:
        VphoError = VE

        def __getattr__(self, name):
            seen.append(name)
            return getattr(ops, name)
    half = PH.IDENTITY.copy()
    half[0] = 0.5
    for bad in (dict(K1={2: 4}), dict(K2={3: 9}), dict(clip_limit={2: 0.5}), dict(clip_limit={2: np.nan}), dict(k1={2: half}), dict(hue={3: F(np.inf)}),
                dict(contrast={2: F(-1)}), dict(k2={3: np.full(49, np.nan, F)})):
        p = {k: np.array(v) for k, v in params.items()}
        for k, v in bad.items():
            for s, item in v.items():
                p[k][s] = item
        with pytest.raises(ValueError):
            PH.photo_patch(Spy(), _cuda(frames), _cuda(minv), 32, _cuda(colour), p)
    with pytest.raises(ValueError, match='multiple of 8'):
        PH.photo_patch(Spy(), _cuda(frames), _cuda(minv), 20, _cuda(colour), params)
    assert seen == [], seen


def test_a_refusal_of_the_c_side_is_read_from_the_one_error_slot():
    """past the Python-side checks, straight at the entry point: P = 0 fails photo.hip's first VPHO_REQUIRE, before any launch, and the
    text comes back through vpho_last_error; a frames.hip call refused right after reports its own text, so the slot is one and not stale"""
    ops = _ops()
    frames = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device='cuda')
    minv = torch.zeros((1, 6), dtype=torch.float64, device='cuda')
    lev = torch.full((1, 4, 4, 3), 77, dtype=torch.uint8, device='cuda')
    out = torch.full((1, 3, 4, 4), 12345.0, device='cuda')
    with pytest.raises(ops.VphoError, match=r'vpho_photo_levels_u8: bad size \(n 1, H 4, W 4, P 0\)'):
        ops._call('vpho_photo_levels_u8', frames, 1, 4, 4, minv, 0, lev)
    with pytest.raises(ops.VphoError, match=r'vpho_frame_patch_f32: bad size \(n 1, H 4, W 4, P 0\)') as e:
        ops._call('vpho_frame_patch_f32', frames, 1, 4, 4, minv, None, None, None, None, 0, out)
    assert 'photo' not in str(e.value)
    torch.cuda.synchronize()
    assert bool((lev == 77).all()) and bool((out == 12345.0).all())


# ---------------------------------------------------------------------------------------------------------------------- end to end
class _Cfg:
    """context: set fields of the module-global cfg, restore them afterwards"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from vpho_amd.configs.args import cfg
        self.saved = {k: getattr(cfg, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(cfg, k, v)
        return cfg

    def __exit__(self, *exc):
        from vpho_amd.configs.args import cfg
        for k, v in self.saved.items():
            setattr(cfg, k, v)


SMALL = dict(sample_num=4, sampling_steps=5, topk_hand=8, topk_obj=3, sample_T0=0.2, eval_batch_size=4, batch_size=4, num_batches=2, repeat_num=4,
             random_seed=7, checkpoint='')
REFERENCE = dict(clahe_p=0.5, jitter_contrast=(0.6, 1.3), jitter_hue=(-0.15, 0.15), blur_p=0.5, motion_blur_p=0.5)


def test_pipeline_with_the_reference_augmentation(assets):
    from vpho_amd import frames as FR
    from vpho_amd.synth import synth_batch
    src = FR.synthetic_frames(6, assets, seed=3, size=(160, 120))
    items = [src[i] for i in range(6)]
    frames, recs = torch.from_numpy(np.stack([f for f, _ in items])), [r for _, r in items]
    with _Cfg(**SMALL) as cfg:
        plain = FR.FramePipeline(cfg, assets, 'cuda', train=True, seed=11)
        assert plain.photo is None
        base = plain(frames, recs, epoch=2)
        # without the new flags rgb is what the path before this module gave: ops.frame_patch on the same plan and draws
        per = [FR.sample_draws(cfg, 11, 2, i, True, 256) for i in range(6)]
        draws = {k: np.stack([np.asarray(d[k]) for d in per]) for k in per[0]}
        assert set(per[0]) == {'jitter', 'scale', 'rot', 'colour', 'erase', 'key', 'jitter_gate'}
        K = np.stack([r['cam_intr'] for r in recs])
        rt = np.stack([r['obj_rt'] for r in recs])
        kp = np.stack([assets['ycb'][n]['kpt3d'] for n in base['obj_name']]).astype(np.float64) @ rt[:, :, :3].transpose(0, 2, 1) + rt[:, None, :, 3]
        right = np.array([r['is_right'] for r in recs], bool)
        plan = FR.crop_plan(np.stack([r['jt2d'] for r in recs]), FR.project(kp, K), K, draws, 256, cfg.bbox_scale_factor, is_right=right)
        some = (draws['erase'][:, :, 2] > draws['erase'][:, :, 0]).any()
        want = _ops().frame_patch(frames.cuda(), _cuda(plan['minv']), 256, colour=_cuda(draws['colour'].astype(F)), flip=_cuda((~right).astype(np.uint8)),
                                  erase=_cuda(draws['erase'].astype(np.int32)) if some else None,
                                  key=_cuda(draws['key'].astype(np.uint32).view(np.int32)) if some else None)
        assert torch.equal(base['rgb'], want)
    with _Cfg(**SMALL, **REFERENCE) as cfg:
        pipe = FR.FramePipeline(cfg, assets, 'cuda', train=True, seed=11)
        assert pipe.photo is not None
        b = pipe(frames, recs, epoch=2)
        again = pipe(frames.cuda(), recs, epoch=2)
        other = pipe(frames, recs, epoch=3)
        ev = FR.FramePipeline(cfg, assets, 'cuda', train=False, seed=11)
        assert ev.photo is None                                                        # evaluation draws nothing and launches nothing new
        evb = ev(frames, recs)
    with _Cfg(**SMALL) as cfg:
        assert torch.equal(evb['rgb'], FR.FramePipeline(cfg, assets, 'cuda', train=False, seed=11)(frames, recs)['rgb'])
    torch.cuda.synchronize()
    for k, v in synth_batch(6, assets, seed=1).items():                               # the Appendix-A keys
        assert k in b, k
        if torch.is_tensor(v):
            assert tuple(b[k].shape) == tuple(v.shape) and b[k].dtype == v.dtype and b[k].is_cuda, (k, b[k].shape, v.shape)
    assert set(b) == set(base) and tuple(b['rgb'].shape) == (6, 3, 256, 256) and bool(torch.isfinite(b['rgb']).all())
    assert torch.equal(b['rgb'], again['rgb']) and not torch.equal(b['rgb'], other['rgb'])
    for k in ('hm_hand', 'hm_obj', 'bbox_hand', 'gt_mano', 'gt_jt2d'):                # nothing but the image changes
        assert torch.equal(b[k], base[k]), k
    # the samples whose new gates all stayed shut are today's crops, the others are not
    PH = _photo()
    with _Cfg(**SMALL, **REFERENCE) as cfg:
        pd = [PH.photo_draws(cfg, 11, 2, i, bool(per[i]['jitter_gate'])) for i in range(6)]
    shut = [d['clip_limit'] == 0 and d['contrast'] == 1 and d['hue'] == 0 and d['K1'] == 1 and d['K2'] == 1 for d in pd]
    print('PHOTO pipeline: samples with every new gate shut', shut)
    # (a gate that fired need not change a level: a blur drawn with sigma 0.2 is the 1 x 1 kernel to eight digits)
    same = [torch.equal(b['rgb'][s], base['rgb'][s]) for s in range(6)]
    assert all(same[s] for s in range(6) if shut[s]) and not all(same) and not all(shut), (same, shut)
    assert any(d['clip_limit'] > 0 for d in pd) and all(not same[s] for s in range(6) if pd[s]['clip_limit'] > 0), (same, [d['clip_limit'] for d in pd])


def test_one_fit_epoch_with_the_reference_augmentation(tmp_path):
    from vpho_amd import frames as FR
    from vpho_amd.trainer import Trainer
    with _Cfg(max_epochs=1, train_scope='full', gradient_clip=5.0, print_freq=1, **SMALL, **REFERENCE) as cfg:
        tr = Trainer(cfg)
        src = FR.synthetic_frames(8, tr.assets, seed=1)
        pipe = FR.FramePipeline(cfg, tr.assets, tr.device, train=True, seed=7)
        assert pipe.photo is not None
        train = FR.FrameLoader(src, 4, pipe, shuffle=True, drop_last=True)
        out = tr.fit(train, save_dir=str(tmp_path / 'run'))
        assert out['epochs'] == 1 and len(out['losses']) == 1 and all(np.isfinite(v) for v in out['losses'][0].values()), out['losses']
        assert {'hm_hand_loss', 'hm_obj_loss', 'diff_hand_loss'} <= set(out['losses'][0]) and train.epoch == 1


def test_main_train_on_synthetic_frames_with_photo_aug_reference_in_a_child_process():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    args = ['--mode', 'train', '--model', 'vpho_net', '--frame_source', 'synthetic', '--photo_aug', 'reference', '--batch_size', '4', '--num_batches', '2',
            '--random_seed', '7', '--sample_num', '4', '--sampling_steps', '5', '--repeat_num', '4']
    script = ("import sys; sys.argv = ['main.py'] + %r\nimport main\nmain.main()\nfrom vpho_amd.configs.args import cfg\n"
              "print('PHOTO_CHILD', 'vpho_amd.photo' in sys.modules, cfg.clahe_p, cfg.blur_p, cfg.motion_blur_p, tuple(cfg.jitter_hue))\n" % (args,))
    r = subprocess.run([sys.executable, '-c', script], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert '[0000] ' in r.stdout and 'PHOTO_CHILD True 0.5 0.5 0.5 (-0.15, 0.15)' in r.stdout, r.stdout[-2000:]
    assert 'nan' not in r.stdout.split('PHOTO_CHILD')[0].lower(), r.stdout[-2000:]

"""The host side of the photometric augmentation (vpho_amd/photo.py, the flags, csrc/photo.hip's report) without a GPU: the new flags
and ``--photo_aug reference``, the draw order of the second generator, stream 1 untouched, the CLAHE LUT rule worked by hand (on the
host function AND on the referee of tests/_photo_fp64.py, which share no code), the host-built filter kernels, the refusals, the
compiler's report, the header, and that a defaults run never imports vpho_amd.photo."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _photo_fp64 as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = dict(photo_aug='none', clahe_p=0.0, clahe_clip_limit=(1.0, 4.0), jitter_contrast=(1.0, 1.0), jitter_hue=(0.0, 0.0), blur_p=0.0, blur_limit=(3, 7),
           sigma_limit=(0.2, 2.0), motion_blur_p=0.0, motion_blur_limit=(3, 7))
REFERENCE = dict(clahe_p=0.5, jitter_contrast=(0.6, 1.3), jitter_hue=(-0.15, 0.15), blur_p=0.5, motion_blur_p=0.5)


@pytest.fixture(scope='module')
def PH():
    from vpho_amd import photo
    return photo


def _cfg(**kw):
    from vpho_amd.configs import args as A
    c = A.Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ---------------------------------------------------------------------------------------------------------------------- flags
def test_new_flags_defaults_and_photo_aug_reference():
    from vpho_amd.configs import args as A
    p = A._parser()
    d, c = p.parse_args([]), A.Config()
    for k, v in NEW.items():
        assert tuple(np.atleast_1d(getattr(d, k))) == tuple(np.atleast_1d(v)) and tuple(np.atleast_1d(getattr(c, k))) == tuple(np.atleast_1d(v)), k
    ref = p.parse_args(['--photo_aug', 'reference'])
    for k, v in REFERENCE.items():
        assert tuple(np.atleast_1d(getattr(ref, k))) == tuple(np.atleast_1d(v)), k
    assert tuple(ref.clahe_clip_limit) == (1.0, 4.0) and tuple(ref.blur_limit) == (3, 7) and tuple(ref.sigma_limit) == (0.2, 2.0)
    # explicit flags win over --photo_aug, wherever they stand on the line, also when they spell a default
    mix = p.parse_args(['--blur_p', '0', '--photo_aug', 'reference', '--jitter_hue', '-0.05', '0.05', '--clahe_clip_limit', '2', '3'])
    assert mix.blur_p == 0 and list(mix.jitter_hue) == [-0.05, 0.05] and mix.clahe_p == 0.5 and mix.motion_blur_p == 0.5 and list(mix.clahe_clip_limit) == [2, 3]
    assert tuple(mix.jitter_contrast) == (0.6, 1.3) and not hasattr(mix, '_explicit')
    assert A.PHOTO_REFERENCE == REFERENCE
    with pytest.raises(SystemExit):
        p.parse_args(['--photo_aug', 'albumentations'])


def test_can_fire_only_when_a_flag_lets_it(PH):
    from vpho_amd import frames as FR
    assert not FR.photo_can_fire(_cfg()) and not PH.photo_can_fire(_cfg())
    for kw in (dict(clahe_p=0.1), dict(jitter_contrast=(0.9, 1.0)), dict(jitter_hue=(0.0, 0.1)), dict(blur_p=1.0), dict(motion_blur_p=0.5), REFERENCE):
        assert FR.photo_can_fire(_cfg(**kw)) and PH.photo_can_fire(_cfg(**kw)), kw
    # the other knobs alone fire nothing
    assert not FR.photo_can_fire(_cfg(clahe_clip_limit=(2.0, 3.0), blur_limit=(3, 5), sigma_limit=(1.0, 1.5), motion_blur_limit=(5, 7)))


# ---------------------------------------------------------------------------------------------------------------------- draws
def test_stream_one_is_unchanged_by_the_new_flags():
    from vpho_amd import frames as FR
    base = dict(random_erasing_max_count=2, random_erasing_prob=1.0, RGB_shift_prob=1.0, color_jitter_prob=1.0)
    for index in (0, 7, 123):
        a = FR.sample_draws(_cfg(**base), 3, 1, index, True, 256)
        b = FR.sample_draws(_cfg(**base, **REFERENCE), 3, 1, index, True, 256)
        for k in ('jitter', 'scale', 'rot', 'colour', 'erase', 'key'):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (index, k)
        # ... and they are the numbers of the documented order, drawn by hand from generator 1
        r = np.random.default_rng((3, 1, index))
        assert np.array_equal(a['jitter'], 0.2 * r.uniform(-1, 1, 2)) and a['scale'] == 0.2 * r.uniform(0, 1) + 1
        r.uniform(0, 1), r.uniform(-1, 1), r.uniform(0, 1)
        assert np.array_equal(a['colour'][:3], np.rint(r.uniform(-20, 20, 3)).astype(np.float32))
        r.uniform(0, 1)
        assert np.array_equal(a['colour'][3:], np.array([r.uniform(0.6, 1.3), r.uniform(0.6, 1.3)], np.float32)) and a['jitter_gate'] is True
    assert FR.sample_draws(_cfg(color_jitter_prob=0.0), 3, 1, 7, True, 256)['jitter_gate'] is False
    assert FR.sample_draws(_cfg(), 3, 1, 7, False, 256)['jitter_gate'] is False


def test_the_draw_order_of_stream_two(PH):
    on = dict(clahe_p=1.0, jitter_contrast=(0.6, 1.3), jitter_hue=(-0.15, 0.15), blur_p=1.0, motion_blur_p=1.0)
    for index in (0, 5, 31):
        d = PH.photo_draws(_cfg(**on), 9, 2, index, True)
        r = np.random.default_rng((9, 2, index, 1))
        u = [r.uniform(0, 1), r.uniform(1.0, 4.0), r.uniform(0.6, 1.3), r.uniform(-0.15, 0.15), r.uniform(0, 1), r.uniform(0, 1), r.uniform(0.2, 2.0),
             r.uniform(0.2, 2.0), r.uniform(-90, 90), r.uniform(0.5, 8)]
        noise = r.uniform(0.9, 1.1, 49)
        tail = [r.uniform(0, 1), r.uniform(0, 1), r.uniform(0, 1)]
        assert d['clip_limit'] == u[1] and d['contrast'] == np.float32(u[2]) and d['hue'] == np.float32(u[3])
        K1 = (3, 5, 7)[min(int(u[5] * 3), 2)]
        assert d['K1'] == K1 and np.array_equal(d['k1'], PH.blur_kernel(K1, u[6], u[7], u[8], u[9], noise))
        K2 = (3, 5, 7)[min(int(tail[1] * 3), 2)]
        assert d['K2'] == K2 and np.array_equal(d['k2'], PH.motion_kernel(K2, min(int(tail[2] * (K2 * K2 - 1)), K2 * K2 - 2)))
        # every draw is taken whether or not its gate fires: with the gates shut the values that remain are the same numbers
        half = PH.photo_draws(_cfg(**dict(on, clahe_p=0.0, blur_p=0.0)), 9, 2, index, True)
        assert half['clip_limit'] == 0.0 and half['K1'] == 1 and np.array_equal(half['k1'], PH.IDENTITY)
        assert half['contrast'] == d['contrast'] and half['K2'] == d['K2'] and np.array_equal(half['k2'], d['k2'])
        # contrast and hue ride under the colour-jitter gate of stream 1
        shut = PH.photo_draws(_cfg(**on), 9, 2, index, False)
        assert shut['contrast'] == 1 and shut['hue'] == 0 and shut['clip_limit'] == d['clip_limit'] and np.array_equal(shut['k1'], d['k1'])
    off = PH.photo_draws(_cfg(), 9, 2, 5, True)
    assert off['clip_limit'] == 0 and off['contrast'] == 1 and off['hue'] == 0 and off['K1'] == 1 and off['K2'] == 1
    # the gates fire at about their probability
    fired = [PH.photo_draws(_cfg(**REFERENCE), 0, 0, i, True) for i in range(400)]
    for share in (np.mean([f['clip_limit'] > 0 for f in fired]), np.mean([f['K1'] > 1 for f in fired]), np.mean([f['K2'] > 1 for f in fired])):
        assert 0.4 < share < 0.6, share
    with pytest.raises(ValueError, match='blur_limit'):
        PH.photo_draws(_cfg(blur_limit=(3, 9)), 0, 0, 0, True)
    with pytest.raises(ValueError, match='motion_blur_limit'):
        PH.photo_draws(_cfg(motion_blur_limit=(4, 4)), 0, 0, 0, True)
    with pytest.raises(ValueError, match='clip_limit'):
        PH.photo_draws(_cfg(clahe_p=1.0, clahe_clip_limit=(0.2, 0.5)), 0, 0, 0, True)


# ---------------------------------------------------------------------------------------------------------------------- the LUT rule, by hand
def _both(PH, tile, clip):
    """the LUT of a tile by the referee's loops and by the host function: they must agree, and the caller holds them to the hand-made answer"""
    a = R.tile_lut(tile, clip)
    b = PH.clahe_lut(np.bincount(np.asarray(tile).reshape(-1), minlength=256), clip)
    assert np.array_equal(a, b.astype(np.int64))
    return a


def _rhe(num, den):
    """round half to even of a fraction, by Python's own exact rounding of Fractions"""
    from fractions import Fraction
    return round(Fraction(num, den))


def test_lut_of_a_constant_tile(PH):
    # 8 x 8 pixels of level 10, clip limit 4: clip = max(1, int(4 * 64 / 256)) = 1.  63 counts are cut off: none per bin (63 // 256), the
    # residual 63 to bins 0, 4, 8, ..., 248 (step 256 // 63 = 4).  cumsum[i] = i // 4 + 1 (at most 63) + 1 from level 10 on
    assert R.clip_count(4.0, 8) == 1 and PH.clahe_clip(4.0, 8) == 1
    lut = _both(PH, np.full((8, 8), 10), 1)
    want = [_rhe(255 * (min(i // 4, 62) + 1 + (i >= 10)), 64) for i in range(256)]
    assert list(lut) == want and lut[0] == 4 and lut[10] == 16 and lut[255] == 255


def test_lut_of_a_two_level_tile(PH):
    # 32 x 32 pixels, half at 50, half at 200, clip limit 4: clip = 16.  2 * (512 - 16) = 992 counts cut off: 3 to every bin, the
    # residual 224 one each to bins 0 .. 223 (step 1)
    assert R.clip_count(4.0, 32) == 16 and PH.clahe_clip(4.0, 32) == 16 and PH.clahe_clip(1.0, 32) == 4 and PH.clahe_clip(2.5, 32) == 10
    tile = np.concatenate([np.full(512, 50), np.full(512, 200)])
    lut = _both(PH, tile, 16)
    want = [_rhe(255 * (3 * (i + 1) + min(i + 1, 224) + 16 * (i >= 50) + 16 * (i >= 200)), 1024) for i in range(256)]
    assert list(lut) == want and lut[255] == 255
    # no clipping at all when the clip count is the tile: the plain equalisation
    assert list(_both(PH, tile, 1024)) == [0 if i < 50 else (_rhe(255 * 512, 1024) if i < 200 else 255) for i in range(256)]
    assert _rhe(255 * 512, 1024) == 128                     # 127.5 goes to the even neighbour


def test_lut_of_a_tile_of_one_pixel_and_of_four(PH):
    # P = 8: a tile is one pixel, clip = max(1, int(c / 256)) = 1, nothing is cut off: a step from 0 to 255 at the pixel's level
    assert R.clip_count(4.0, 1) == 1 and PH.clahe_clip(4.0, 1) == 1
    lut = _both(PH, np.array([37]), 1)
    assert list(lut) == [0] * 37 + [255] * 219
    # P = 16: four pixels, clip = 1 whatever the limit.  Levels 3, 3, 3, 200: two counts cut off, one each to bins 0 and 128 (step 128);
    # cumsum = 1 | 2 from 3 | 3 from 128 | 4 from 200 -> 63.75 -> 64, 127.5 -> 128 (half to even), 191.25 -> 191, 255
    for c in (1.0, 2.5, 4.0):
        assert R.clip_count(c, 2) == 1 and PH.clahe_clip(c, 2) == 1
    lut = _both(PH, np.array([[3, 3], [3, 200]]), 1)
    assert list(lut) == [64] * 3 + [128] * 125 + [191] * 72 + [255] * 56
    with pytest.raises(ValueError, match='clip_limit'):
        PH.clahe_clip(0.5, 8)
    with pytest.raises(ValueError, match='clip_limit'):
        PH.clahe_clip(float('nan'), 8)


def test_interpolation_is_exact_at_tile_centres_and_blends_between():
    # P = 16, tiles of 2: LUT of tile (ty, tx) maps every level to 10 * ty + tx
    luts = np.stack([np.full(256, 10 * ty + tx) for ty in range(8) for tx in range(8)])
    out = R.clahe_interpolate(np.zeros((16, 16), np.int64), luts)
    # pixel x = 0 has tile coordinate (1 - 2) / 4 = -0.25: clamped to tile 0 on both sides; x = 1: 0.25 -> 0.75 * 0 + 0.25 * 1 = 0.25 -> 0;
    # x = 2: 0.75 -> 0.75 -> 1; x = 15: 7.25 -> tile 7 on both sides
    assert list(out[0, :4]) == [0, 0, 1, 1] and out[0, 15] == 7 and out[15, 15] == 77 and out[15, 0] == 70
    assert out[1, 0] == _rhe(10, 4) == 2 and out[2, 0] == _rhe(30, 4) == 8       # 2.5 -> 2 and 7.5 -> 8: half to even
    assert R.round_half_even_div(5, 2) == 2 and R.round_half_even_div(7, 2) == 4 and R.round_half_even_div(9, 4) == 2


# ---------------------------------------------------------------------------------------------------------------------- host kernels
def test_blur_kernels_sum_to_one(PH):
    r = np.random.default_rng(0)
    for K in (1, 3, 5, 7):
        for _ in range(8):
            k = PH.blur_kernel(K, r.uniform(0.2, 2), r.uniform(0.2, 2), r.uniform(-90, 90), r.uniform(0.5, 8), r.uniform(0.9, 1.1, 49))
            assert k.dtype == np.float32 and k.shape == (49,) and abs(k[:K * K].astype(np.float64).sum() - 1) <= 1e-6 and not k[K * K:].any() and (k >= 0).all()
            PH.check_kernel(k, K)
    # without noise an isotropic kernel is symmetric under transposition and both flips; an elongated one at 0 degrees is wider than tall
    k = PH.blur_kernel(5, 1.0, 1.0, 30.0, 1.0, np.ones(49))[:25].reshape(5, 5)
    assert np.array_equal(k, k.T) and np.array_equal(k, k[::-1]) and k.argmax() == 12
    assert abs(k[2, 3] / k[2, 2] - np.exp(-0.5)) < 1e-6                              # beta 1: the Gaussian exp(-x^2 / (2 sigma^2))
    wide = PH.blur_kernel(5, 2.0, 0.3, 0.0, 1.0, np.ones(49))[:25].reshape(5, 5)
    assert wide[2, 4] > 100 * wide[4, 2]
    turned = PH.blur_kernel(5, 2.0, 0.3, 90.0, 1.0, np.ones(49))[:25].reshape(5, 5)
    assert np.allclose(turned, wide.T, atol=1e-7)
    for bad in (dict(sigma_x=0.0), dict(beta=float('nan')), dict(noise=np.full(49, np.inf))):
        kw = dict(K=3, sigma_x=1.0, sigma_y=1.0, angle_deg=0.0, beta=1.0, noise=np.ones(49))
        kw.update(bad)
        with pytest.raises(ValueError):
            PH.blur_kernel(**kw)


def test_motion_kernels_are_centred_symmetric_connected_lines(PH):
    for K in (3, 5, 7):
        c = K // 2
        seen = set()
        for cell in range(K * K - 1):
            cells = PH.motion_cells(K, cell)
            k = PH.motion_kernel(K, cell)[:K * K].reshape(K, K)
            on = {(int(y), int(x)) for y, x in zip(*np.nonzero(k))}
            assert on == set(cells) and (c, c) in on and len(on) >= 3
            assert np.array_equal(k, k[::-1, ::-1])                                   # central symmetry
            assert np.all(k[k > 0] == np.float32(1.0 / len(on))) and abs(float(k.astype(np.float64).sum()) - 1) <= 1e-6
            flat = cell if cell < c * K + c else cell + 1
            assert (flat // K, flat % K) in on                                        # the drawn cell lies on the line
            # 8-connected: a flood fill from the centre reaches every cell
            reach, todo = {(c, c)}, [(c, c)]
            while todo:
                y, x = todo.pop()
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        q = (y + dy, x + dx)
                        if q in on and q not in reach:
                            reach.add(q)
                            todo.append(q)
            assert reach == on, (K, cell)
            # a line, not a blob: at most one cell per step of the longer axis, on both sides of the centre
            assert len(on) <= 2 * c + 1
            seen.add(frozenset(on))
            PH.check_kernel(PH.motion_kernel(K, cell), K)
        assert len(seen) == (K * K - 1) // 2 if K == 3 else len(seen) > K     # a cell and its mirror image give the same line
    assert np.array_equal(PH.motion_kernel(1, 0), PH.IDENTITY)
    # the diagonal of a 3 x 3 grid: cell 0 is the top-left corner
    assert PH.motion_cells(3, 0) == [(0, 0), (1, 1), (2, 2)] and PH.motion_cells(3, 1) == [(0, 1), (1, 1), (2, 1)]
    assert PH.motion_cells(5, 0) == [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]
    with pytest.raises(ValueError):
        PH.motion_cells(3, 8)
    with pytest.raises(ValueError):
        PH.motion_cells(4, 0)


def test_kernels_the_device_must_not_get_are_refused(PH):
    good = PH.IDENTITY.copy()
    PH.check_kernel(good, 1)
    for K in (0, 2, 4, 9, -1, 3.0):
        with pytest.raises(ValueError, match='odd integer'):
            PH.check_kernel(good, K)
    k = np.zeros(49, np.float32)
    k[:9] = 1 / 9
    PH.check_kernel(k, 3)
    k[4] += 1e-4
    with pytest.raises(ValueError, match='sum to 1'):
        PH.check_kernel(k, 3)
    k[4] = np.nan
    with pytest.raises(ValueError, match='finite'):
        PH.check_kernel(k, 3)
    with pytest.raises(ValueError, match='float32'):
        PH.check_kernel(np.zeros(49), 3)


# ---------------------------------------------------------------------------------------------------------------------- referee against itself
def test_referee_known_answers():
    # Lab: white is L = 100 -> 255, black 0, and mid grey 119 is L = 50.03 (sRGB 119 -> Y = 0.1845)
    assert np.rint(R.l8_raw(np.array([[255, 255, 255], [0, 0, 0]]))).tolist() == [255, 0]
    assert abs(R.l8_raw(np.array([119, 119, 119])) * 100 / 255 - 50.03) < 0.02
    # the return trip with L unchanged gives the levels back where L8 happens to be exact: white, black
    assert np.rint(R.lab_return(np.array([[255, 255, 255], [0, 0, 0]]), np.array([255, 0]))).tolist() == [[255, 255, 255], [0, 0, 0]]
    # hue: a shift of 1/3 turns red into green, of -1/3 into blue; grey stays grey; a shift of 0 is skipped
    red = np.array([[[200, 0, 0]]], np.float32)
    assert R.hue(red, 1 / 3).tolist() == [[[0, 200, 0]]] and R.hue(red, -1 / 3).tolist() == [[[0, 0, 200]]]
    assert R.hue(np.full((1, 1, 3), 77, np.float32), 0.15).tolist() == [[[77, 77, 77]]] and R.hue(red, 0) is red
    # contrast about the integer mean, saturation about the pixel's grey
    img = np.array([[[10, 10, 10], [30, 30, 30]]], np.float32)
    assert R.grey_mean(img) == (20, 40) and R.contrast(img, 0.5, 20).tolist() == [[[15, 15, 15], [25, 25, 25]]]
    assert R.grey_mean(np.array([[[10, 10, 10], [11, 11, 11]]], np.float32))[0] == 11       # 10.5 rounds up: (2 * 21 + 2) // 4
    # filters: a delta kernel off the centre shifts the image, reflect-101 at the border (no edge pixel is doubled)
    r = np.random.default_rng(1)
    img = r.integers(0, 256, (8, 8, 3)).astype(np.float32)
    k = np.zeros((3, 3), np.float32)
    k[1, 2] = 1                                              # tap (ky 1, kx 2): out[y][x] = in[y][x + 1]
    out = R.filter2d(img, k)
    assert np.array_equal(out[:, :7], img[:, 1:]) and np.array_equal(out[:, 7], img[:, 6])
    k = np.zeros((7, 7), np.float32)
    k[0, 3] = 1                                              # out[y][x] = in[y - 3][x]; rows 0..2 read rows 3, 2, 1
    out = R.filter2d(img, k)
    assert np.array_equal(out[3:], img[:5]) and np.array_equal(out[0], img[3]) and np.array_equal(out[2], img[1])
    assert np.array_equal(R.filter2d(img, np.ones((1, 1), np.float32)), img)
    assert np.array_equal(R.finish(img, True)[:, :, 0], R.finish(img, False)[:, :, 7])


# ---------------------------------------------------------------------------------------------------------------------- build
def test_photo_kernels_report_no_spill_and_no_scratch():
    from vpho_amd.build import build_extension
    build_extension()
    seen, name = {}, None
    for line in open(os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'photo.hip.usage.txt')):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (('spill', r'VGPRs Spill: (\d+)'), ('sspill', r'SGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds', r'LDS Size \[bytes/block\]: (\d+)'), ('vgpr', r' VGPRs: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    want = ('photo_levels_kernel', 'photo_clahe_lut_kernel', 'photo_clahe_apply_kernel', 'photo_grey_sum_kernel', 'photo_colour_kernel', 'photo_filter_kernel')
    assert len(seen) == len(want) and all(any(w in k for k in seen) for w in want), sorted(seen)
    for k, v in seen.items():
        print('PHOTO', k, v)
        assert v['spill'] == 0 and v['sspill'] == 0 and v['scratch'] == 0 and v['vgpr'] <= 64, (k, v)
    lds = {w: next(v['lds'] for k, v in seen.items() if w in k) for w in want}
    # the filter's two tiles: (32 + 12)^2 and (32 + 6)^2 pixels of one word, and two 49-tap kernels
    assert lds['photo_filter_kernel'] >= 44 * 44 * 4 + 38 * 38 * 4 + 2 * 49 * 4 and lds['photo_filter_kernel'] <= 16384
    assert lds['photo_levels_kernel'] == 0 and lds['photo_colour_kernel'] == 0 and 0 < lds['photo_clahe_lut_kernel'] <= 8192


def test_the_photo_entry_points_are_declared_in_the_one_header_and_exported_by_the_one_library():
    """csrc/photo.hip links into libvpho_hip.so like every other kernel file: its six entry points are declared in include/vpho_hip.h with
    VPHO_API and exported by the library.  How many entry points there are, the ABI version, that the exports equal the header and that
    every `_call` in ops.py passes what the prototype declares are tests/test_abi.py's business"""
    from vpho_amd import build as B
    B.build_extension()
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    for proto in (r'VPHO_API int vpho_photo_levels_u8\(const unsigned char\* frames, int n, int H, int W, const double\* minv, int P, unsigned char\* out, void\* stream\);',
                  r'VPHO_API int vpho_photo_clahe_lut_u8\(const unsigned char\* levels, const int\* clip, int n, int P, unsigned char\* l8, unsigned char\* lut, void\* stream\);',
                  r'VPHO_API int vpho_photo_clahe_apply_u8\(const unsigned char\* levels, const int\* clip,[^;]*unsigned char\* l8_out, void\* stream\);',
                  r'VPHO_API int vpho_photo_grey_sum_u8\(const unsigned char\* levels, const float\* colour, int n, int P, long long\* sums, void\* stream\);',
                  r'VPHO_API int vpho_photo_colour_u8\(const unsigned char\* levels, const float\* colour, const float\* contrast, const float\* hue,[^;]*void\* stream\);',
                  r'VPHO_API int vpho_photo_filter_f32\(const unsigned char\* levels, const float\* k1, const int\* K1, const float\* k2, const int\* K2,[^;]*float\* out, void\* stream\);'):
        assert re.search(proto, hdr), proto
    assert 'base.py:349-397' in hdr
    declared = sorted(set(re.findall(r'\b(vpho_photo_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))))
    assert len(declared) == 6
    nm = subprocess.run(['nm', '-D', '--defined-only', B.LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if l.strip())
    assert [n for n in exported if 'photo' in n] == declared
    # every photo op of ops.py goes through the one `_call`, once each
    src = open(os.path.join(ROOT, 'vpho_amd', 'ops.py')).read()
    assert sorted(re.findall(r"\b_call\('(vpho_photo_[a-z0-9_]+)'", src)) == declared
    for doc in ('README.md', 'INTEGRATION.md'):
        assert 'photo.hip' in open(os.path.join(ROOT, doc)).read(), doc
    # frames.hip keeps its two kernels; what photo.hip shares with it is one copy, in frames_common.h
    src = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'frames.hip')).read()
    assert src.count('__global__') == 2 and 'photo' not in src
    photo = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'photo.hip')).read()
    common = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'frames_common.h')).read()
    for shared in ('philox4x32_10', 'unit23', 'box_muller', 'cubic_weights', 'level', 'bicubic_crop', 'normalise_erase'):
        assert len(re.findall(r'__device__ __forceinline__ \w+ ' + shared + r'\(', common)) == 1, shared
        assert not re.search(r'__device__[^;{]*\b' + shared + r'\(', src + photo), shared
    assert '__global__' not in common and '#include "frames_common.h"' in src and '#include "frames_common.h"' in photo


_DEFAULTS_SCRIPT = '''
import sys
sys.argv = ['x'] + {flags!r}
from vpho_amd.configs.args import cfg
from vpho_amd import frames as FR
from vpho_amd.assets import synthetic_assets
for train in (True, False):
    pipe = FR.FramePipeline(cfg, synthetic_assets(0), 'cpu', train=train, seed=0)
    print('PHOTO', train, pipe.photo is not None, 'vpho_amd.photo' in sys.modules)
'''


def test_a_defaults_run_never_imports_the_module():
    """with the default flags a training pipeline is built without vpho_amd.photo; with --photo_aug reference the training pipeline has
    it and the evaluation pipeline (built first here) does not ask for it"""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    run = lambda flags: subprocess.run([sys.executable, '-c', _DEFAULTS_SCRIPT.format(flags=flags)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    r = run([])
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'PHOTO True False False' in r.stdout and 'PHOTO False False False' in r.stdout, r.stdout
    r = run(['--photo_aug', 'reference'])
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'PHOTO True True True' in r.stdout, r.stdout
    script = _DEFAULTS_SCRIPT.replace('for train in (True, False)', 'for train in (False,)')
    r = subprocess.run([sys.executable, '-c', script.format(flags=['--photo_aug', 'reference'])], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'PHOTO False False False' in r.stdout, r.stdout + r.stderr[-2000:]
    with pytest.raises(ValueError, match='multiple of 8'):
        from vpho_amd import frames as FR
        from vpho_amd.assets import synthetic_assets
        FR.FramePipeline(_cfg(clahe_p=0.5, patch_size=20), synthetic_assets(0), 'cpu', train=True)

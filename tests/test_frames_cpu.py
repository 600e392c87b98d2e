"""The host side of the data front end (vpho_amd/frames.py) without a GPU: the crop plan against the reference's own
``get_augmentation_rotmat`` (tests/golden/golden_frames.npz, written by make_golden_frames.py from the real lib/dataset/base.py), the box
helpers against the reference's, the fit loop, left-hand mirroring, the label algebra, the seeding rule, the flags, the header and the
compiler's report of csrc/frames.hip, the restatements of tests/_frames_fp64.py held to their known answers, and FrameDirectory."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _frames_fp64 as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_frames.npz')))


@pytest.fixture(scope='module')
def FR():
    from vpho_amd import frames
    return frames


@pytest.fixture(scope='module')
def syn_assets():
    from vpho_amd.assets import synthetic_assets
    return synthetic_assets(0)


def _cfg(**kw):
    from vpho_amd.configs import args as A
    c = A.Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ---------------------------------------------------------------------------------------------------------------------- plan
def test_crop_matrices_equal_the_reference_to_1e12(gold, FR):
    n = len(gold['crop_rot'])
    for i in range(n):
        R3, M, Kc = FR._crop_matrices(gold['crop_jt2d'][i:i + 1], gold['crop_obj2d'][i:i + 1], gold['crop_K'][i:i + 1], gold['crop_jitter'][i:i + 1],
                                      gold['crop_scale'][i:i + 1], gold['crop_rot'][i:i + 1], int(gold['crop_patch'][i]), float(gold['crop_bsf'][i]))
        for name, got, want in (('rotmat_3d', R3, gold['crop_R3'][i]), ('rotmat_2d', M, gold['crop_M'][i]), ('cam_intr_crop', Kc, gold['crop_Kc'][i])):
            err = np.abs(got[0] - want).max() / max(1.0, np.abs(want).max())
            print(f'crop {i} {name}: max relative error {err:.2e}')
            assert err <= 1e-12, (i, name, err)
    # the whole batch at once equals sample by sample (six samples share one patch size)
    R3, M, Kc = FR._crop_matrices(gold['crop_jt2d'][:6], gold['crop_obj2d'][:6], gold['crop_K'][:6], gold['crop_jitter'][:6], gold['crop_scale'][:6],
                                  gold['crop_rot'][:6], 256, 1.2)
    assert np.abs(M - gold['crop_M'][:6]).max() <= 1e-12 * np.abs(gold['crop_M']).max() and np.abs(Kc - gold['crop_Kc'][:6]).max() <= 1e-9


def test_plan_with_a_fit_on_the_first_try_is_the_fixture(gold, FR):
    """a sample whose boxes fit at once keeps the reference's matrices; its points are the reference's affine map of the inputs"""
    draws = dict(jitter=gold['crop_jitter'][:6], scale=gold['crop_scale'][:6], rot=gold['crop_rot'][:6])
    plan = FR.crop_plan(gold['crop_jt2d'][:6], gold['crop_obj2d'][:6], gold['crop_K'][:6], draws, 256, 1.2)
    first = plan['tries'] == 0
    assert first.any()
    assert np.abs(plan['rotmat_2d'][first] - gold['crop_M'][:6][first]).max() <= 1e-12 * np.abs(gold['crop_M']).max()
    assert np.abs(plan['cam_intr_crop'][first] - gold['crop_Kc'][:6][first]).max() <= 1e-9
    for i in range(6):
        M = plan['rotmat_2d'][i]
        want = gold['crop_jt2d'][i] @ M[:2, :2].T + M[:2, 2]
        assert np.abs(plan['gt_jt2d'][i] - want).max() <= 1e-10
        full = np.concatenate([plan['minv'][i].reshape(2, 3), [[0, 0, 1]]])
        assert np.abs(full @ M - np.eye(3)).max() <= 1e-9
        assert np.array_equal(plan['cam_intr_crop_flip'][i], plan['cam_intr_crop'][i])             # no is_right given: nothing mirrored


def test_box_helpers_equal_the_reference(gold, FR):
    b = FR.pt2d_to_bbox2d(gold['box_pts'])
    e = FR.expand_bbox2d(b, 1.15)
    rect, m = FR.rect_bbox2d(e)
    for got, want in ((b, gold['box_bbox']), (e, gold['box_expand']), (rect, gold['box_rect']), (m, gold['box_max_wh'])):
        assert np.abs(got - want).max() <= 1e-12 * 300
    assert np.array_equal(FR.check_bbox2d(rect, 256), gold['box_ok']) and gold['box_ok'].any() and not gold['box_ok'].all()


def _scene(spread_obj=25.0, offset=(0.0, 0.0)):
    r = np.random.default_rng(3)
    c = np.array([300.0, 220.0])
    jt = c + r.normal(0, 30, (1, 21, 2))
    ob = c + np.asarray(offset) + r.normal(0, spread_obj, (1, 27, 2))
    K = np.array([[[600.0, 0, 320], [0, 600, 240], [0, 0, 1]]])
    return jt, ob, K


def test_fit_loop_zero_tries_several_tries_and_failure(FR):
    jt, ob, K = _scene()
    plan = FR.crop_plan(jt, ob, K, FR.eval_draws(1), 256, 1.2)
    assert plan['tries'][0] == 0 and plan['scale_factor'][0] == 1.0
    # a tight crop (bbox_scale_factor 1.0) leaves the expanded, squared boxes outside: the scale factor grows by 1.01 per try
    tight = FR.crop_plan(jt, ob, K, FR.eval_draws(1), 256, 0.9)
    k = int(tight['tries'][0])
    print('tries with bbox_scale_factor 0.9:', k)
    assert 1 < k < 99 and abs(tight['scale_factor'][0] - 1.01 ** k) < 1e-12
    for key in ('bbox_hand_rect', 'bbox_obj_rect'):
        assert FR.check_bbox2d(tight[key], 256).all()
    # one try fewer does not fit: the loop stopped at the first scale factor that does
    R3, M, Kc = FR._crop_matrices(jt, ob, K, np.zeros((1, 2)), np.array([1.01 ** (k - 1)]), np.zeros(1), 256, 0.9)
    j2, o2 = jt @ np.swapaxes(M[:, :2, :2], -1, -2) + M[:, None, :2, 2], ob @ np.swapaxes(M[:, :2, :2], -1, -2) + M[:, None, :2, 2]
    ok = FR.check_bbox2d(FR.rect_bbox2d(FR.expand_bbox2d(FR.pt2d_to_bbox2d(j2), 1.15))[0], 256) & \
        FR.check_bbox2d(FR.rect_bbox2d(FR.expand_bbox2d(FR.pt2d_to_bbox2d(o2), 1.10))[0], 256)
    assert not ok.any()
    # in a batch the samples keep their own counts
    both = FR.crop_plan(np.concatenate([jt, jt]), np.concatenate([ob, ob]), np.concatenate([K, K]), FR.eval_draws(2), 256, 0.9)
    assert list(both['tries']) == [k, k]
    # 1.01 ** 99 = 2.68 cannot rescue a crop that is ten times too tight: ValueError naming the sample
    with pytest.raises(ValueError, match='index 1 bbox out of image'):
        FR.crop_plan(np.concatenate([jt, jt]), np.concatenate([ob, ob]), np.concatenate([K, K]), dict(jitter=np.zeros((2, 2)), scale=np.array([1.0, 0.1]),
                                                                                                   rot=np.zeros(2)), 256, 1.2)
    bad = jt.copy()
    bad[0, 3, 1] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        FR.crop_plan(bad, ob, K, FR.eval_draws(1), 256, 1.2)


def test_eval_draws_are_the_identity(FR):
    d = FR.eval_draws(3)
    assert not d['jitter'].any() and (d['scale'] == 1).all() and not d['rot'].any()
    s = FR.sample_draws(_cfg(), 5, 2, 9, False, 256)
    assert not s['jitter'].any() and s['scale'] == 1.0 and s['rot'] == 0.0 and list(s['colour']) == [0, 0, 0, 1, 1] and not s['erase'].any()
    jt, ob, K = _scene()
    plan = FR.crop_plan(jt, ob, K, FR.eval_draws(1), 256, 1.2)
    assert np.array_equal(plan['rotmat_3d'][0], np.eye(3)) and plan['rotmat_2d'][0, 0, 1] == 0 and plan['rotmat_2d'][0, 0, 0] == plan['rotmat_2d'][0, 1, 1]


def test_left_hands_mirror_every_2d_key(FR):
    jt, ob, K = _scene()
    two = lambda a: np.concatenate([a, a])
    draws = dict(jitter=np.full((2, 2), 0.05), scale=np.full(2, 1.1), rot=np.full(2, 0.3))
    plan = FR.crop_plan(two(jt), two(ob), two(K), draws, 256, 1.2, is_right=np.array([True, False]))
    r, l = 0, 1
    for k in ('gt_jt2d', 'gt_obj2d'):
        assert np.array_equal(plan[k][l, :, 0], 256 - plan[k][r, :, 0]) and np.array_equal(plan[k][l, :, 1], plan[k][r, :, 1])
    for k in ('bbox_hand', 'bbox_obj', 'bbox_hand_rect', 'bbox_obj_rect'):
        b, m = plan[k][r], plan[k][l]
        assert m[0] == 256 - b[2] and m[2] == 256 - b[0] and m[1] == b[1] and m[3] == b[3] and m[0] < m[2]
    assert plan['cam_intr_crop_flip'][l, 0, 2] == 256 - plan['cam_intr_crop'][l, 0, 2]
    assert np.array_equal(plan['cam_intr_crop_flip'][r], plan['cam_intr_crop'][r])
    assert np.array_equal(plan['cam_intr_crop'][l], plan['cam_intr_crop'][r]) and np.array_equal(plan['minv'][l], plan['minv'][r])


# ---------------------------------------------------------------------------------------------------------------------- labels
def _records(FR, syn_assets, n=6, seed=4):
    src = FR.synthetic_frames(n, syn_assets, seed=seed, size=(160, 120))
    return FR._stack_records([src[i][1] for i in range(n)])


def test_label_algebra(FR, syn_assets):
    rec = _records(FR, syn_assets)
    rec['is_right'] = np.array([True, False, True, False, True, True])
    n = 6
    rot = np.linspace(-0.5, 0.5, n)
    lab = FR.rigid_labels(rec, rot, syn_assets)
    c, s = np.cos(rot), np.sin(rot)
    Rz = np.zeros((n, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1
    Rz = torch.from_numpy(Rz)
    # global rotation: Rz . R, then mirrored for left hands (components 1 and 2 of the axis-angle negated = conjugation by diag(1,-1,-1)... of
    # the vector, i.e. the rotation matrix F R F with F = diag(-1, 1, 1))
    R0 = FR.aa_to_matrix(torch.from_numpy(rec['mano_pose'][:, :3]))
    got = FR.aa_to_matrix(lab['gt_mano'][:, :3])
    want = Rz @ R0
    F = torch.diag(torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64))
    want = torch.where(torch.from_numpy(rec['is_right'])[:, None, None], want, F @ want @ F)
    assert (got - want).abs().max() <= 1e-12
    fingers = torch.from_numpy(rec['mano_pose'][:, 3:]).reshape(n, 15, 3).clone()
    fingers[~torch.from_numpy(rec['is_right']), :, 1:] *= -1
    assert torch.equal(lab['gt_mano'][:, 3:48], fingers.reshape(n, 45)) and torch.equal(lab['gt_mano'][:, 48:], torch.from_numpy(rec['mano_betas']))
    assert lab['gt_mano'].shape == (n, 58)
    # matrix_to_aa inverts aa_to_matrix also near pi and near 0
    aa = torch.tensor([[3.1, 0.2, -0.1], [1e-9, 0, 0], [0, 0, 0], [0.0, 3.14159, 0.0], [1.0, -2.0, 0.5]], dtype=torch.float64)
    assert (FR.aa_to_matrix(FR.matrix_to_aa(FR.aa_to_matrix(aa))) - FR.aa_to_matrix(aa)).abs().max() <= 1e-12
    # object: 9-D pose round trip through obj_9d_to_rt's host formula (Gram-Schmidt of the two rows, third = cross; t + root)
    a1, a2 = lab['gt_obj'][:, :3], lab['gt_obj'][:, 3:6]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=-1, keepdim=True)
    rt = torch.cat([torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], 1), (lab['gt_obj'][:, 6:] + lab['root_joint'])[..., None]], -1)
    assert (rt - lab['gt_obj_rt']).abs().max() <= 1e-12
    assert (lab['gt_obj_rt'][:, :, :3] - Rz @ torch.from_numpy(rec['obj_rt'][:, :, :3])).abs().max() <= 1e-15
    # root-relative keys
    assert torch.equal(lab['root_joint'], lab['gt_joint'][:, 0]) and not lab['gt_hand_jt3d_flip'][:, 0].any()
    left = ~torch.from_numpy(rec['is_right'])
    assert torch.equal(lab['root_joint_flip'][left, 0], -lab['root_joint'][left, 0]) and torch.equal(lab['root_joint_flip'][~left], lab['root_joint'][~left])
    assert (lab['gt_hand_jt3d_flip'][left][..., 0] + (lab['gt_joint'][left] - lab['root_joint'][left][:, None])[..., 0]).abs().max() <= 1e-15
    assert (lab['gt_hand_vert_flip'] + lab['root_joint_flip'][:, None])[~left].sub(lab['gt_hand_vert'][~left]).abs().max() <= 1e-15
    assert (lab['gt_joint'] - torch.from_numpy(rec['joint_3d']) @ Rz.transpose(1, 2)).abs().max() <= 1e-15
    assert lab['gravity'].shape == (n, 1, 3) and lab['obj_CoM'].shape == (n, 1, 3)
    assert (lab['gravity'][:, 0] - (Rz @ torch.from_numpy(rec['gravity'])[..., None])[..., 0]).abs().max() <= 1e-15
    del rec['hand_vert']
    assert 'gt_hand_vert' not in FR.rigid_labels(rec, rot, syn_assets)


# ---------------------------------------------------------------------------------------------------------------------- seeding
def test_the_seeding_rule(FR):
    cfg = _cfg(random_erasing_max_count=2, random_erasing_prob=1.0)
    a = {i: FR.sample_draws(cfg, 3, 1, i, True, 256) for i in (7, 2, 11)}
    b = {i: FR.sample_draws(cfg, 3, 1, i, True, 256) for i in (11, 7, 2)}              # another batch order
    for i in a:
        for k in a[i]:
            assert np.array_equal(np.asarray(a[i][k]), np.asarray(b[i][k])), (i, k)
    other = FR.sample_draws(cfg, 3, 2, 7, True, 256)
    assert not np.array_equal(other['jitter'], a[7]['jitter']) and other['scale'] != a[7]['scale'] and other['rot'] != a[7]['rot']
    assert not np.array_equal(FR.sample_draws(cfg, 4, 1, 7, True, 256)['key'], a[7]['key'])
    d = a[7]
    assert np.abs(d['jitter']).max() <= cfg.center_jittering and 1 <= d['scale'] <= 1 + cfg.scale_factor and abs(d['rot']) <= cfg.max_rot / 180 * np.pi
    e = d['erase']
    assert ((e[:2, 2] > e[:2, 0]) & (e[:2, 3] > e[:2, 1]) & (e[:2, :2] >= 0).all(1) & (e[:2, 2:] <= 256).all(1)).all() and not e[2:].any()
    area = (e[:2, 2] - e[:2, 0]) * (e[:2, 3] - e[:2, 1]) / 256.0 ** 2 * 2
    assert (area > 0.015).all() and (area < 0.21).all()
    # the gates: with all probabilities 0 nothing but jitter and scale is applied, and those are the SAME numbers (fixed stream positions)
    off = FR.sample_draws(_cfg(rot_prob=0.0, RGB_shift_prob=0.0, color_jitter_prob=0.0, random_erasing_prob=0.0), 3, 1, 7, True, 256)
    assert off['rot'] == 0.0 and list(off['colour']) == [0, 0, 0, 1, 1] and not off['erase'].any()
    assert np.array_equal(off['jitter'], d['jitter']) and off['scale'] == d['scale'] and np.array_equal(off['key'], d['key'])
    on = FR.sample_draws(_cfg(RGB_shift_prob=1.0, color_jitter_prob=1.0), 3, 1, 7, True, 256)
    c = on['colour']
    assert (c[:3] == np.rint(c[:3])).all() and np.abs(c[:3]).max() <= 20 and 0.6 <= c[3] <= 1.3 and 0.6 <= c[4] <= 1.3
    with pytest.raises(ValueError, match='at most 4'):
        FR.sample_draws(_cfg(random_erasing_max_count=5), 0, 0, 0, True, 256)


def test_loader_order_and_length(FR, tmp_path):
    # a resumed fit starts the loader at the checkpoint's epoch; a model file or nothing starts it at 0
    state = tmp_path / 'checkpoint' / 'epoch_3.state'
    state.mkdir(parents=True)
    assert FR.resume_epoch(_cfg(checkpoint=str(state))) == 0                          # no optimiser in it: not a training state
    (state / 'optimizer.bin').write_bytes(b'')
    assert FR.resume_epoch(_cfg(checkpoint=str(state))) == 3 and FR.resume_epoch(_cfg(checkpoint='')) == 0
    pipe = types.SimpleNamespace(seed=5, device='cpu')
    src = list(range(10))
    L = FR.FrameLoader(src, 4, pipe, shuffle=True, drop_last=True)
    assert len(L) == 2 and len(FR.FrameLoader(src, 4, pipe)) == 3
    o0, o0b, o1 = L._order(0), L._order(0), L._order(1)
    assert all(np.array_equal(a, b) for a, b in zip(o0, o0b)) and not all(np.array_equal(a, b) for a, b in zip(o0, o1))
    assert sorted(np.concatenate(FR.FrameLoader(src, 4, pipe, shuffle=True)._order(3))) == src
    assert [list(b) for b in FR.FrameLoader(src, 4, pipe)._order(0)] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]


# ---------------------------------------------------------------------------------------------------------------------- flags, header, report
def test_flags_defaults_and_config_attributes():
    from vpho_amd.configs import args as A
    p = A._parser()
    d = p.parse_args([])
    want = dict(frame_source='none', bbox_scale_factor=1.2, center_jittering=0.2, scale_factor=0.2, max_rot=30.0, rot_prob=1.0, RGB_shift_prob=0.5,
                shift_limit=(-20.0, 20.0), color_jitter_prob=0.5, brightness=(0.6, 1.3), saturation=(0.6, 1.3), random_erasing_prob=0.5,
                random_erasing_min_area=0.02, random_erasing_max_area=0.2, random_erasing_max_count=1, heatmap_hand_sigma=2.0, heatmap_obj_sigma=2.0)
    c = A.Config()
    for k, v in want.items():
        assert getattr(d, k) == v and getattr(c, k) == v, k
    a = p.parse_args(['--mode', 'eval', '--frame_source', 'synthetic', '--shift_limit', '-5', '5', '--heatmap_obj_sigma', '1.5'])
    assert a.frame_source == 'synthetic' and list(a.shift_limit) == [-5.0, 5.0] and a.heatmap_obj_sigma == 1.5
    for gone in ('contrast', 'hue', 'clahe_prob', 'gaussian_blur_prob', 'motion_blur_prob'):
        assert not hasattr(d, gone)
    assert 'no dataset in this build' not in open(os.path.join(ROOT, 'vpho_amd', 'configs', 'args.py')).read()


def test_header_declares_the_two_entry_points_at_abi_13():
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert re.search(r'VPHO_API int vpho_frame_patch_f32\(const unsigned char\* frames, int n, int H, int W, const double\* minv,[^;]*void\* stream\);', hdr)
    assert re.search(r'VPHO_API int vpho_heatmap_targets_f32\(const double\* pts, const double\* box,[^;]*void\* stream\);', hdr)
    assert 'dexycb6.py:339-469' in hdr and 'misc_fn.py:285-385' in hdr
    count = hdr.count('VPHO_API ') - 1
    assert count >= 120
    for doc in ('README.md', 'INTEGRATION.md'):
        assert f'{count} ' in open(os.path.join(ROOT, doc)).read(), (doc, count)


def test_frames_kernels_report_no_spill_and_no_scratch():
    from vpho_amd.build import build_extension
    build_extension()
    seen, name = {}, None
    for line in open(os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'frames.hip.usage.txt')):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (('spill', r'VGPRs Spill: (\d+)'), ('sspill', r'SGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds', r'LDS Size \[bytes/block\]: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    assert len(seen) == 2 and any('frame_patch_kernel' in k for k in seen) and any('heatmap_targets_kernel' in k for k in seen), sorted(seen)
    for k, v in seen.items():
        assert v == dict(spill=0, sspill=0, scratch=0, lds=0), (k, v)


# ---------------------------------------------------------------------------------------------------------------------- restatements
def test_philox_known_answers():
    kat = (((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'))
    for ctr, key, want in kat:
        assert ' '.join(f'{w:08x}' for w in R.philox4x32_10(ctr, key)) == want


def test_restatements_of_the_warp_and_the_resize():
    w = R.cubic_weights(np.array([0.0, 0.25, 0.5, 0.999]))
    assert np.abs(w.sum(-1) - 1).max() < 1e-14 and np.array_equal(w[0], [0, 1, 0, 0]) and np.allclose(w[2], [-0.09375, 0.59375, 0.59375, -0.09375])
    r = np.random.default_rng(0)
    f = r.integers(0, 256, (12, 14, 3), dtype=np.uint8)
    ident = R.warp_levels(f, np.array([1.0, 0, 0, 0, 1, 0]), 10)
    assert np.array_equal(ident, f[:10, :10].astype(np.float64))
    shifted = R.warp_levels(f, np.array([1.0, 0, 3, 0, 1, -2]), 10)                 # patch (x, y) <- frame (x + 3, y - 2)
    assert np.array_equal(shifted[2:, :], f[:8, 3:13].astype(np.float64)) and not shifted[:2].any()
    lv = r.integers(0, 256, (5, 5, 3)).astype(np.float64)
    assert np.array_equal(R.denormalise(R.normalise_f32(lv)), lv)
    assert np.array_equal(R.to_level(R.colour_stages(lv, (0, 0, 0, 1, 1))[-1]), lv)
    src = r.random((2, 5, 7))
    same = R.resize_linear(np.repeat(src[:, :1], 5, 1), 7)                           # constant columns, width 7 -> 7: identity along x
    assert np.allclose(same[:, 0], src[:, 0]) and np.allclose(same[:, 6], src[:, 0])
    up = R.resize_linear(np.arange(4.0).reshape(1, 1, 4), 8)[0, 0]                    # 4 -> 8: sources -0.25, 0.25, ..., edge clamped
    assert np.allclose(up, [0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3])
    z0, z1 = R.box_muller(0x80000000, 0)
    assert abs(z0 - np.sqrt(-2 * np.log((2 ** 22 + 0.5) / 2 ** 23)) * np.cos(2 * np.pi * 0.5 / 2 ** 23)) < 1e-15


def test_adaptive_exclusion_cap_holds_on_the_fixture(gold, FR):
    """the GPU test leaves out pixels whose float64 value lies within 1e-6 of g.min(); that share stays below 0.5 % on every fixture case"""
    for ci, (S, sigma, n) in enumerate(gold['hm_cases']):
        gmin = float(gold[f'hm{ci}_g'].min())
        assert gmin == FR.gauss_table(float(sigma))[1] and np.array_equal(FR.gauss_table(float(sigma))[0], gold[f'hm{ci}_g'].astype(np.float32))
        for si in range(int(n)):
            want = R.resize_linear(gold[f'hm{ci}_{si}_tight'], int(S))
            share = float((np.abs(want - gmin) <= 1e-6).mean())
            print(f'adaptive case {ci}.{si}: excluded share {share:.5f}, tight map {gold[f"hm{ci}_{si}_tight"].shape[1:]}')
            assert share <= 0.005
            res, wh = FR.adaptive_res(gold[f'hm{ci}_{si}_box'][None], int(S))
            assert (int(res[0, 1]), int(res[0, 0])) == gold[f'hm{ci}_{si}_tight'].shape[1:]
    with pytest.raises(ValueError, match='degenerate'):
        FR.adaptive_res(np.array([[10.0, 10.0, 200.0, 11.0]]), 64)
    with pytest.raises(ValueError, match='degenerate'):
        FR.adaptive_res(np.array([[10.0, 10.0, 10.0, 50.0]]), 64)


# ---------------------------------------------------------------------------------------------------------------------- sources
def test_frame_directory_round_trips_npy_frames(tmp_path, FR, syn_assets):
    src = FR.synthetic_frames(3, syn_assets, seed=2, size=(48, 40))
    f0, r0 = src[1]
    assert f0.shape == (40, 48, 3) and f0.dtype == np.uint8 and np.array_equal(src[1][0], f0) and not np.array_equal(src[2][0], f0)
    assert r0['jt2d'].shape == (21, 2) and r0['hand_vert'].shape == (778, 3) and r0['obj_rt'].shape == (3, 4)
    assert np.abs(FR.project(r0['joint_3d'], r0['cam_intr']) - r0['jt2d']).max() < 1e-9
    FR.write_frame_directory(str(tmp_path / 'd'), src)
    back = FR.FrameDirectory(str(tmp_path / 'd'))
    assert len(back) == 3
    for i in range(3):
        f, r = back[i]
        assert np.array_equal(f, src[i][0]) and r['index'] == i
        for k in FR.RECORD_KEYS + FR.OPTIONAL_KEYS:
            assert np.array_equal(np.asarray(r[k]), np.asarray(src[i][1][k])), k
    with pytest.raises(FileNotFoundError, match='annotations.npz'):
        FR.FrameDirectory(str(tmp_path / 'nothing'))
    a = dict(np.load(str(tmp_path / 'd' / 'annotations.npz')))
    del a['obj_rt']
    os.makedirs(str(tmp_path / 'e'))
    np.savez(str(tmp_path / 'e' / 'annotations.npz'), **a)
    with pytest.raises(KeyError, match='obj_rt'):
        FR.FrameDirectory(str(tmp_path / 'e'))

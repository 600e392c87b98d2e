"""The two kernels of csrc/frames.hip through ``ops.frame_patch`` / ``ops.heatmap_targets`` and the front end built on them.

Warp and colour: the integer grey level recovered from the output equals the float64 restatement's (tests/_frames_fp64.py) wherever every
float64 value that gets rounded lies farther than 1e-3 from a half-integer; the remaining pixels may differ by one level and are at most
1 % of a case; the normalised value is bit-equal to numpy's fp32 expression of the level.  Erasing: untouched pixels bit-identical, the
normals within 1e-5 of the restatement's.  Heat-maps: square mode bit-equal to the reference's own maps (tests/golden/golden_frames.npz),
adaptive mode within 1e-6 of the restatement's resize of the reference's tight map.  End to end: the pipeline's dict, Trainer.eval / fit
on a FrameLoader, main.py in child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _frames_fp64 as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 12345.0


def _ops():
    from vpho_amd import ops
    return ops


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_frames.npz')))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frames(n, H, W, seed):
    """frame 0 uint8 noise, frame 1 a smooth ramp, further frames noise"""
    r = np.random.default_rng(seed)
    f = r.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    f[1] = np.stack([np.rint(255 * x / (W - 1)), np.rint(255 * y / (H - 1)), np.rint(255 * (x + y) / (W + H - 2))], -1).astype(np.uint8)
    return f


def _inverse(M):
    return np.linalg.inv(np.concatenate([M, [[0, 0, 1]]]))[:2].reshape(6)


def _similarity(angle, scale, H, W, P):
    """patch <- frame: rotate by ``angle`` and scale by ``scale`` about the frame centre, which lands on the patch centre"""
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    A = np.array([[c, -s], [s, c]])
    t = np.array([P / 2, P / 2]) - A @ np.array([W / 2, H / 2])
    return _inverse(np.concatenate([A, t[:, None]], 1))


def _transforms(H, W, P):
    return {'identity': np.array([1.0, 0, 0, 0, 1, 0]),
            'integer translation': np.array([1.0, 0, 5, 0, 1, 3]),
            'rotation 0.4 scale 0.8': _similarity(0.4, 0.8, H, W, P),
            'rotation -0.5 scale 2.3': _similarity(-0.5, 2.3, H, W, P),
            'over the left edge': np.array([1.0, 0, -P / 2 + 0.3, 0, 1, 2.6]),
            'over the right edge': np.array([1.0, 0, W - P / 2 + 0.3, 0, 1, 2.6]),
            'over the top edge': np.array([1.0, 0, 2.6, 0, 1, -P / 2 + 0.7]),
            'over the bottom edge': np.array([1.0, 0, 2.6, 0, 1, H - P / 2 + 0.7])}


def _patch(frames, minv, P, **kw):
    ops = _ops()
    n = frames.shape[0]
    dev = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in kw.items()}
    m = torch.from_numpy(np.repeat(np.asarray(minv, np.float64).reshape(1, 6), n, 0)).cuda()
    out = ops.frame_patch(torch.from_numpy(frames).cuda(), m, P, **dev)
    torch.cuda.synchronize()
    return out.cpu().numpy().transpose(0, 2, 3, 1)                                   # (n, P, P, 3)


def _unsure(raws, shape):
    """per VALUE: True where one of the float64 values rounded on the way lies within 1e-3 of a half-integer (a (..., 1) stage counts
    for the three channels)"""
    unsure = np.zeros(shape, bool)
    for v in raws:
        unsure |= R.near_half(v)
    return unsure


def _judge(name, out, raws, want_level):
    """out (P,P,3) normalised; raws: the float64 values that were rounded on the way; want_level: the float64 route's final level"""
    got = R.denormalise(out)
    assert np.array_equal(_bits(out), _bits(R.normalise_f32(got))), f'{name}: the output is not numpy\'s fp32 expression of an integer level'
    unsure = _unsure(raws, out.shape)
    share = float(unsure.mean())
    diff = np.abs(got - want_level)
    print(f'FRAMES {name}: excluded share {share:.5f}, mismatches outside the band {int((diff[~unsure] != 0).sum())}, '
          f'largest difference inside {diff[unsure].max() if unsure.any() else 0:.0f}')
    assert share <= 0.01, f'{name}: {share:.4f} of the values lie within 1e-3 of a half-integer'
    assert not diff[~unsure].any(), f'{name}: {int((diff[~unsure] != 0).sum())} levels differ outside the band'
    assert diff.max() <= 1, f'{name}: a level differs by {diff.max()}'


# ---------------------------------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize('n,H,W,P', [(3, 40, 56, 16), (3, 40, 56, 32), (2, 96, 128, 16), (2, 96, 128, 32)])
def test_warp_against_the_float64_restatement(n, H, W, P):
    frames = _frames(n, H, W, seed=H + P)
    for name, minv in _transforms(H, W, P).items():
        out = _patch(frames, minv, P)
        for s in range(n):
            raw = R.warp_levels(frames[s], minv, P)
            _judge(f'{(n, H, W)} -> {P} {name} frame {s}', out[s], [raw], R.to_level(raw))
        if name == 'integer translation':                                            # the source pixels themselves
            assert np.array_equal(R.denormalise(out), frames[:, 3:3 + P, 5:5 + P].astype(np.float64))
        if name == 'over the left edge':
            assert (R.denormalise(out)[:, :, :P // 2 - 2] == 0).all() and R.denormalise(out)[:, :, P // 2 + 2:].any()


def test_warp_of_a_camera_frame_to_256():
    frames = _frames(2, 480, 640, seed=1)[1:]                                        # the ramp alone: (1, 480, 640)
    frames = np.ascontiguousarray(frames)
    frames[0, ::2, ::3] = np.random.default_rng(2).integers(0, 256, frames[0, ::2, ::3].shape, dtype=np.uint8)
    minv = _similarity(0.3, 0.55, 480, 640, 256)
    out = _patch(frames, minv, 256)
    raw = R.warp_levels(frames[0], minv, 256)
    _judge('(1, 480, 640) -> 256 rotation 0.3 scale 0.55', out[0], [raw], R.to_level(raw))


def test_flip_writes_the_mirrored_row_and_only_where_asked():
    frames = _frames(3, 40, 56, seed=9)
    minv = _similarity(0.4, 0.8, 40, 56, 32)
    plain = _patch(frames, minv, 32)
    flipped = _patch(frames, minv, 32, flip=np.array([0, 1, 0], np.uint8))
    assert np.array_equal(_bits(flipped[1]), _bits(plain[1][:, ::-1])) and not np.array_equal(flipped[1], plain[1])
    assert np.array_equal(_bits(flipped[0]), _bits(plain[0])) and np.array_equal(_bits(flipped[2]), _bits(plain[2]))


# A stage multiplies INTEGER levels by its factor, so its values take a few hundred distinct fractions; with an arbitrary factor one common
# difference can sit on a half-integer (29 * 0.2931 = 8.4999) and push the excluded share over the cap.  The factors below keep every
# product of an integer in [-255, 255] at least 2e-3 away from a half-integer (0.6 and 1.12 cannot reach one at all); what is left in
# the band are the exact half-integers of the gray value, about 0.3 % of a noise frame.
@pytest.mark.parametrize('name,colour', [('shift', (17, -20, 6, 1, 1)), ('brightness', (0, 0, 0, 1.2514, 1)), ('darker', (0, 0, 0, 0.6207, 1)),
                                         ('saturation up', (0, 0, 0, 1, 1.2514)), ('saturation down', (0, 0, 0, 1, 0.6)),
                                         ('together', (-13, 9, 20, 1.12, 0.752))])
def test_colour_stages(name, colour):
    frames = _frames(3, 40, 56, seed=5)
    col = np.tile(np.asarray(colour, np.float32), (3, 1))
    col[2] = (0, 0, 0, 1, 1)                                                          # per sample: the third frame is left alone
    for tname, minv in (('identity', np.array([1.0, 0, 0, 0, 1, 0])), ('rotation 0.4 scale 0.8', _similarity(0.4, 0.8, 40, 56, 32))):
        out = _patch(frames, minv, 32, colour=col)
        for s in range(3):
            raw = R.warp_levels(frames[s], minv, 32)
            stages = R.colour_stages(R.to_level(raw), col[s])
            _judge(f'colour {name} {tname} frame {s}', out[s], [raw] + stages, R.to_level(stages[-1]))
        assert np.array_equal(_bits(out[2]), _bits(_patch(frames, minv, 32)[2]))
    assert not np.array_equal(out[0], _patch(frames, minv, 32)[0])


def test_no_frames_sentinels_and_a_repeat_run():
    ops = _ops()
    empty = ops.frame_patch(torch.zeros((0, 40, 56, 3), dtype=torch.uint8, device='cuda'), torch.zeros((0, 6), dtype=torch.float64, device='cuda'), 16)
    assert tuple(empty.shape) == (0, 3, 16, 16)
    frames = torch.from_numpy(_frames(2, 40, 56, seed=3)).cuda()
    minv = torch.from_numpy(np.tile(_similarity(-0.5, 2.3, 40, 56, 23), (2, 1))).cuda()
    size = 2 * 3 * 23 * 23                                                            # an odd patch size: the last block is partial
    buf = torch.full((size + 512,), SENT, device='cuda')
    out = buf[256:256 + size].view(2, 3, 23, 23)
    ops.frame_patch(frames, minv, 23, out=out)
    first = out.clone()
    ops.frame_patch(frames, minv, 23, out=out)
    torch.cuda.synchronize()
    assert bool((buf[:256] == SENT).all()) and bool((buf[256 + size:] == SENT).all()) and not bool((out == SENT).any())
    assert torch.equal(first.view(torch.int32), out.view(torch.int32))
    raw = R.warp_levels(frames[0].cpu().numpy(), minv[0].cpu().numpy(), 23)
    _judge('(2, 40, 56) -> 23', out[0].cpu().numpy().transpose(1, 2, 0), [raw], R.to_level(raw))
    with pytest.raises(ops.VphoError, match='expected'):
        ops.frame_patch(frames, minv[:1], 23)
    with pytest.raises(ops.VphoError, match='Philox key'):
        ops.frame_patch(frames, minv, 23, erase=torch.zeros((2, 4, 4), dtype=torch.int32, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------------- erasing
def test_random_erasing():
    """Tolerance 1e-5 as the issue states it (fp32 log, sincospi and sqrt against float64 on values of magnitude <= 5.77); the uniforms are
    23-bit values that fp32 holds exactly, so no input rounding adds to it.  The measured worst case is printed."""
    P = 32
    frames = _frames(2, 40, 56, seed=6)
    minv = _similarity(0.4, 0.8, 40, 56, P)
    erase = np.zeros((2, 4, 4), np.int32)
    erase[0, 0] = (0, 0, 10, 7)                                                       # touches the top-left corner
    erase[1] = [(20, 25, 32, 32), (0, 30, 5, 32), (12, 3, 19, 9), (17, 7, 26, 11)]    # four, two at the borders, two overlapping
    key = np.array([[0x12345678, 0x9abcdef0], [0xffffffff, 0x00000001]], np.uint32)
    plain = _patch(frames, minv, P)
    got = _patch(frames, minv, P, erase=erase, key=key.view(np.int32), flip=np.array([0, 1], np.uint8))
    ref = plain.copy()
    ref[1] = ref[1][:, ::-1]
    inside = np.zeros((2, P, P), bool)
    for s in range(2):
        for x0, y0, x1, y1 in erase[s]:
            inside[s, y0:y1, x0:x1] = True
    assert inside[0].sum() == 70 and inside[1].sum() > 150
    assert np.array_equal(_bits(got)[~inside], _bits(ref)[~inside])
    worst = 0.0
    for s, y, x in zip(*np.nonzero(inside)):
        worst = max(worst, float(np.abs(got[s, y, x] - R.erase_normals(int(x), int(y), P, key[s])).max()))
    print(f'FRAMES erasing: {int(inside.sum())} pixels, worst difference {worst:.3e}')
    assert worst <= 1e-5
    z = got[inside]
    assert abs(float(z.mean())) < 0.15 and 0.85 < float(z.std()) < 1.15               # N(0, 1)


# ---------------------------------------------------------------------------------------------------------------------- heat-maps
def _square_inputs(gold, ci, n):
    pts = np.stack([gold[f'hm{ci}_{si}_obj'] for si in range(n)])
    rect = np.stack([gold[f'hm{ci}_{si}_rect'] for si in range(n)])
    mw = (rect[:, 2:] - rect[:, :2]).max(1)
    box = np.concatenate([rect[:, :2], mw[:, None], mw[:, None]], 1)
    left = np.array([not bool(gold[f'hm{ci}_{si}_is_right']) for si in range(n)], np.uint8)
    want = np.stack([gold[f'hm{ci}_{si}_square'] for si in range(n)])
    return pts, box, left, want


@pytest.mark.parametrize('ci', [0, 1, 2])
def test_square_heatmaps_are_the_reference_bit_for_bit(gold, ci):
    ops = _ops()
    from vpho_amd.frames import gauss_table
    S, sigma, n = int(gold['hm_cases'][ci][0]), float(gold['hm_cases'][ci][1]), int(gold['hm_cases'][ci][2])
    g, gmin = gauss_table(sigma)
    gd = torch.from_numpy(g).cuda()
    pts, box, left, want = _square_inputs(gold, ci, n)
    assert want.dtype == np.float32 and left[0] == 1 and (want.reshape(n, 27, -1).max(-1) == 0).any() and (want.reshape(n, 27, -1).max(-1) > 0.8).any()
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for J, m in ((27, n), (21, n), (27, 1)):
        got = ops.heatmap_targets(c(pts[:m, :J]), c(box[:m]), gd, sigma, gmin, S, left=c(left[:m]))
        torch.cuda.synchronize()
        assert tuple(got.shape) == (m, J, S, S)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[:m, :J])), (ci, J, m)
    # without the side flag a left hand's map differs (the + 1 of misc_fn.py:328)
    assert not torch.equal(ops.heatmap_targets(c(pts[:1]), c(box[:1]), gd, sigma, gmin, S), got)
    with pytest.raises(ops.VphoError, match='expected'):
        ops.heatmap_targets(c(pts), c(box[:1].repeat(n + 1, 0)), gd, sigma, gmin, S)
    assert tuple(ops.heatmap_targets(c(pts[:0]), c(box[:0]), gd, sigma, gmin, S).shape) == (0, 27, S, S)


@pytest.mark.parametrize('ci', [0, 1, 2])
def test_adaptive_heatmaps_against_the_resized_reference_map(gold, ci):
    ops = _ops()
    from vpho_amd.frames import adaptive_res, gauss_table
    S, sigma, n = int(gold['hm_cases'][ci][0]), float(gold['hm_cases'][ci][1]), int(gold['hm_cases'][ci][2])
    g, gmin = gauss_table(sigma)
    pts = np.stack([gold[f'hm{ci}_{si}_hand'] for si in range(n)])
    bb = np.stack([gold[f'hm{ci}_{si}_box'] for si in range(n)])
    res, wh = adaptive_res(bb, S)
    c = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for m in sorted({1, n}):
        got = ops.heatmap_targets(c(pts[:m]), c(np.concatenate([bb[:m, :2], wh[:m]], 1)), torch.from_numpy(g).cuda(), sigma, gmin, S, res=c(res[:m]))
        torch.cuda.synchronize()
        got = got.cpu().numpy().astype(np.float64)
        for si in range(m):
            tight = gold[f'hm{ci}_{si}_tight']
            assert tight.shape == (21, res[si, 1], res[si, 0])
            want = R.resize_linear(tight, S)
            band = np.abs(want - gmin) <= 1e-6
            want = np.where(want < gmin, 0.0, want)
            err = float(np.abs(got[si] - want)[~band].max())
            print(f'FRAMES adaptive case {ci}.{si} (n = {m}): tight map {tight.shape[1:]}, excluded share {band.mean():.5f}, worst error {err:.2e}, peak {want.max():.3f}')
            assert band.mean() <= 0.005 and err <= 1e-6 and want.max() > 0.5
            assert np.abs(got[si] - want)[band].max(initial=0.0) <= gmin + 1e-6        # in the band: either the value or 0
    with pytest.raises(ValueError, match='degenerate'):
        adaptive_res(np.array([[10.0, 10.0, 200.0, 11.0]]), 64)


# ---------------------------------------------------------------------------------------------------------------------- end to end
class _Cfg:
    """the global cfg with a few attributes set for the length of a test"""
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


def test_pipeline_gives_the_batch_dict_of_the_schema(assets):
    from vpho_amd import frames as FR
    from vpho_amd.synth import synth_batch
    with _Cfg(**SMALL) as cfg:
        src = FR.synthetic_frames(5, assets, seed=3, size=(160, 120))
        items = [src[i] for i in range(5)]
        frames = torch.from_numpy(np.stack([f for f, _ in items]))
        recs = [r for _, r in items]
        train = FR.FramePipeline(cfg, assets, 'cuda', train=True, seed=11)
        b = train(frames, recs, epoch=2)
        again = train(frames.cuda(), recs, epoch=2)
        other = train(frames, recs, epoch=3)
        ev = FR.FramePipeline(cfg, assets, 'cuda', train=False, seed=11)(frames, recs)
    torch.cuda.synchronize()
    ref = synth_batch(5, assets, seed=1)
    for k, v in ref.items():
        assert k in b, k
        if torch.is_tensor(v):
            assert tuple(b[k].shape) == tuple(v.shape) and b[k].dtype == v.dtype and b[k].is_cuda, (k, b[k].shape, v.shape, b[k].dtype)
        else:
            assert isinstance(b[k], list) and len(b[k]) == len(v) and all(isinstance(s, str) for s in b[k])
    shapes = dict(hm_hand=(5, 21, 64, 64), hm_obj=(5, 27, 64, 64), gt_jt2d=(5, 21, 2), gt_obj2d=(5, 27, 2), gt_joint=(5, 21, 3), gt_hand_vert=(5, 778, 3),
                  gt_obj=(5, 9), gt_mano=(5, 58), gt_hand_jt3d_flip=(5, 21, 3), gt_hand_vert_flip=(5, 778, 3), cam_intr_crop=(5, 3, 3),
                  force_local=(5, 32, 3), obj_id=(5,), index=(5,))
    for k, s in shapes.items():
        assert tuple(b[k].shape) == s and (b[k].dtype == torch.float32 or k in ('obj_id', 'index')), (k, b[k].shape, b[k].dtype)
    # the same (seed, epoch, index) repeats bit for bit, wherever the frames lie; another epoch draws anew; evaluation does not augment
    for k in ('rgb', 'hm_hand', 'hm_obj', 'bbox_hand', 'gt_mano'):
        assert torch.equal(b[k], again[k]), k
    assert not torch.equal(b['rgb'], other['rgb']) and not torch.equal(b['bbox_hand'], other['bbox_hand'])
    assert torch.equal(ev['gt_joint'], torch.from_numpy(np.stack([r['joint_3d'] for r in recs])).float().cuda())
    # the maps peak where the points are: the arg-max of every object map whose point lies well inside the box is within a cell of it
    rect, pts, left = ev['bbox_obj_rect'].double().cpu(), ev['gt_obj2d'].double().cpu(), ~ev['is_right'].cpu()
    cell = (pts - rect[:, None, :2]) / (rect[:, 2] - rect[:, 0])[:, None, None] * 63
    cell[..., 0] += left[:, None].double()
    hm = ev['hm_obj'].cpu()
    am = hm.reshape(5, 27, -1).argmax(-1)
    peak = torch.stack([am % 64, am // 64], -1).double()
    inside = ((cell > 8) & (cell < 55)).all(-1)
    assert inside.sum() > 20 and float((peak - cell.trunc())[inside].abs().max()) <= 1.0 and float(hm.max()) == 1.0
    assert float(ev['hm_hand'].max()) > 0.6 and float(ev['hm_hand'].min()) == 0.0
    # the crop shows the frame: an evaluation crop of a right hand is the float64 warp of its frame
    s = int(torch.nonzero(ev['is_right'])[0])
    K = np.stack([r['cam_intr'] for r in recs])
    rt = np.stack([r['obj_rt'] for r in recs])
    kp = np.stack([assets['ycb'][n]['kpt3d'] for n in ev['obj_name']]).astype(np.float64) @ rt[:, :, :3].transpose(0, 2, 1) + rt[:, None, :, 3]
    plan = FR.crop_plan(np.stack([r['jt2d'] for r in recs]), FR.project(kp, K), K, FR.eval_draws(5), 256, cfg.bbox_scale_factor)
    raw = R.warp_levels(items[s][0], plan['minv'][s], 256)
    _judge('pipeline crop', ev['rgb'][s].cpu().numpy().transpose(1, 2, 0), [raw], R.to_level(raw))


def test_trainer_eval_and_one_fit_epoch_on_a_frame_loader(assets, tmp_path):
    from vpho_amd import frames as FR
    from vpho_amd.trainer import Trainer
    with _Cfg(max_epochs=1, train_scope='full', gradient_clip=5.0, print_freq=1, **SMALL) as cfg:
        tr = Trainer(cfg)
        src = FR.synthetic_frames(8, tr.assets, seed=1)
        loader = FR.FrameLoader(src, 4, FR.FramePipeline(cfg, tr.assets, tr.device, train=False, seed=7))
        assert len(loader) == 2
        rows = tr.eval(loader)
        assert rows.shape[0] == 8 and bool(torch.isfinite(rows).all()) and rows[:, 0].tolist() == list(range(8))
        again = tr.eval(loader)                                                       # a second pass: the same rows (evaluation draws nothing)
        assert torch.equal(rows[:, [0, 1, 7]], again[:, [0, 1, 7]])                      # index, MJE of the regression hand, is_right
        train = FR.FrameLoader(src, 4, FR.FramePipeline(cfg, tr.assets, tr.device, train=True, seed=7), shuffle=True, drop_last=True)
        out = tr.fit(train, save_dir=str(tmp_path / 'run'))
        assert out['epochs'] == 1 and len(out['losses']) == 1 and all(np.isfinite(v) for v in out['losses'][0].values()), out['losses']
        assert {'hm_hand_loss', 'hm_obj_loss', 'diff_hand_loss'} <= set(out['losses'][0]) and train.epoch == 1
        assert os.path.exists(str(tmp_path / 'run' / 'final_model.pt'))


def _child(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


ARGS = ['--sample_num', '4', '--sampling_steps', '5', '--topk_hand', '8', '--topk_obj', '3', '--sample_T0', '0.2', '--eval_batch_size', '4', '--num_batches', '2',
        '--random_seed', '7']


def test_main_eval_on_synthetic_frames_in_a_child_process():
    r = _child([os.path.join(ROOT, 'main.py'), '--mode', 'eval', '--model', 'vpho_net', '--frame_source', 'synthetic'] + ARGS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'evaluated 8 images on 1 GPU(s)' in r.stdout and 'EVAL_JSON ' in r.stdout, r.stdout[-2000:]


_NONE_SCRIPT = '''
import sys, numpy as np
sys.argv = ['main.py', '--mode', 'eval', '--model', 'vpho_net', '--frame_source', 'none'] + {args!r}
import main
from vpho_amd import trainer as T
kept = []
plain = T.Trainer.eval
def keep(self, *a, **k):
    rows = plain(self, *a, **k)
    kept.append(rows.cpu().numpy())
    return rows
T.Trainer.eval = keep
main.main()
assert 'vpho_amd.frames' not in sys.modules, 'the front end was imported without --frame_source'
np.save({out!r}, kept[0])
'''


def test_without_a_frame_source_nothing_changes(tmp_path):
    """main.py --frame_source none never imports the front end, and its rows are those of Trainer.eval() in this process, byte for byte"""
    out = str(tmp_path / 'rows.npy')
    r = _child(['-c', _NONE_SCRIPT.format(args=ARGS, out=out)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    from vpho_amd.trainer import Trainer
    with _Cfg(mode='eval', frame_source='none', **{k: v for k, v in SMALL.items() if k not in ('batch_size', 'repeat_num')}) as cfg:
        rows = Trainer(cfg).eval().cpu().numpy()
    child = np.load(out)
    assert child.shape == rows.shape == (8, rows.shape[1]) and child.tobytes() == rows.tobytes()

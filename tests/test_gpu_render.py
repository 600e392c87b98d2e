"""csrc/raster.hip on the GPU: ``ops.MeshRaster.raster`` against the numpy referee of tests/_raster_fp64.py -- bit for bit on exact (dyadic)
scenes, ids and depths on generic ones outside the referee's `tie` pixels --, run-to-run and batch-composition identity, ``overlay``
against a float64 restatement on the kernel's own maps, the refusals, and ``Trainer.infer`` with ``--infer_render 3`` end to end."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raster_fp64 as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = ('depth_front', 'depth_back', 'face_front', 'face_back')


def _ops():
    from vpho_amd import ops
    return ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _raster(mr, verts, mesh_id, K, H, W, **kw):
    out = mr.raster(_dev(verts, torch.float32), list(mesh_id), _dev(K, torch.float64), H, W, **kw)
    torch.cuda.synchronize()
    return out, {k: out[k].cpu().numpy() for k in MAPS if k in out}


def _assert_bit_equal(got, ref, what):
    for k in MAPS:
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.argwhere(a.view(np.int32) != b.view(np.int32))
        assert bad.size == 0, (what, k, len(bad), [(tuple(i), a[tuple(i)], b[tuple(i)]) for i in bad[:5]])


# ---------------------------------------------------------------------------------------------------------------------- exact scenes
EXACT = {'quad': R.quad_scene, 'fan': R.fan_scene, 'tetra': R.tetra_scene, 'border': R.border_scene}


@pytest.mark.parametrize('size', [(24, 32), (1, 1)])
@pytest.mark.parametrize('name', sorted(EXACT))
def test_exact_scenes_equal_the_referee_bit_for_bit(name, size):
    """dyadic vertices and a dyadic K: projection, snapping and coverage are exact; at 1 x 1 the principal point is moved so that the one
    pixel is the 24 x 32 scene's pixel (8, 8) -- the fan's hub"""
    ops = _ops()
    H, W = size
    v, f, K = EXACT[name]()
    if size == (1, 1):
        K = R.dyadic_K(32.0, 8.0, 4.0)                           # the same vertices seen 8 pixels further left and up
    mr = ops.MeshRaster([(len(v), f)], 'cuda')
    _, got = _raster(mr, v[None], [0], K[None], H, W)
    ref = R.raster(v[None], [0], K[None], [(len(v), f)], H, W)
    print(f'{name} {H}x{W}: {int((ref["face_front"] >= 0).sum())} covered pixels, faces seen {sorted(set(np.unique(ref["face_front"])) - {-1})}')
    _assert_bit_equal(got, ref, name)
    if name != 'border' and size == (1, 1):
        assert got['face_front'][0, 0, 0] >= 0


def test_a_mixed_batch_of_three_meshes_is_one_launch_and_exact():
    ops = _ops()
    scenes = [R.quad_scene(), R.fan_scene(), R.tetra_scene()]
    meshes = [(len(v), f) for v, f, _ in scenes]
    mr = ops.MeshRaster(meshes, 'cuda')
    verts, K = R.pad_verts([v for v, _, _ in scenes]), np.stack([k for _, _, k in scenes])
    order = [2, 0, 1]                                            # images in another order than the table
    _, got = _raster(mr, verts[order], order, K[order], 24, 32)
    _assert_bit_equal(got, R.raster(verts[order], order, K[order], meshes, 24, 32), 'mixed')
    # without the back maps the front maps are the same
    out, front = _raster(mr, verts[order], order, K[order], 24, 32, back=False)
    assert 'depth_back' not in out and np.array_equal(front['face_front'], got['face_front']) and np.array_equal(front['depth_front'], got['depth_front'])
    # n == 0: empty maps, no launch
    out, empty = _raster(mr, verts[:0], [], K[:0], 24, 32)
    assert empty['face_front'].shape == (0, 24, 32)


# ---------------------------------------------------------------------------------------------------------------------- generic scenes
@pytest.fixture(scope='module')
def generic_raster():
    ops = _ops()
    meshes, _ = R.generic_meshes()
    return ops.MeshRaster(meshes, 'cuda')


@pytest.mark.parametrize('name', sorted(R.GENERIC))
def test_generic_scenes_ids_and_depths(name, generic_raster):
    s = R.generic_scene(name)
    ref = s['ref']
    _, got = _raster(generic_raster, s['verts'], s['mesh_id'], s['K'], s['H'], s['W'])
    covered = ref['face_front'] >= 0
    tie = ref['tie']
    share = float(tie.sum()) / int(covered.sum())
    print(f'{name}: {int(covered.sum())} covered pixels, tie share {share:.5f}')
    assert share <= R.TIE_CAP
    for side in ('front', 'back'):
        gf, rf = got['face_' + side], ref['face_' + side]
        bad = np.argwhere((gf != rf) & ~tie)
        assert bad.size == 0, (name, side, len(bad), [(tuple(i), gf[tuple(i)], rf[tuple(i)]) for i in bad[:5]])
        gd, rd = got['depth_' + side], ref['depth_' + side]
        assert not gd[~covered].any() and (gf[~covered] == -1).all()
        check = covered & ~tie
        whole = check & (ref['area_' + side] >= R.FULL_PIXEL_AREA)
        ulp = R.ulp_distance(gd[whole], rd[whole])
        sliver = check & ~whole
        lo, hi = np.zeros_like(gd), np.zeros_like(gd)
        for i, m in enumerate(s['mesh_id']):
            lo[i], hi[i] = R.face_z_range(s['verts'][i], s['meshes'][m][1], gf[i])
        inside = (gd >= lo) & (gd <= hi)
        print(f'  {side}: {int(whole.sum())} pixels on faces of a pixel or more, worst {int(ulp.max()) if ulp.size else 0} ulp; {int(sliver.sum())} on smaller '
              f'faces, {int((~inside & sliver).sum())} outside their face\'s depth range')
        assert ulp.size and ulp.max() <= 2, (name, side, int(ulp.max()))
        assert inside[check].all(), (name, side)


def test_two_runs_and_two_batch_compositions_give_identical_bytes(generic_raster):
    s = R.generic_scene('mixed_40x56')
    many = R.generic_scene('many_images_20x24')
    _, a = _raster(generic_raster, s['verts'], s['mesh_id'], s['K'], s['H'], s['W'])
    _, b = _raster(generic_raster, s['verts'], s['mesh_id'], s['K'], s['H'], s['W'])
    _, alone = _raster(generic_raster, s['verts'][1:], s['mesh_id'][1:], s['K'][1:], s['H'], s['W'])
    _, swapped = _raster(generic_raster, s['verts'][::-1], s['mesh_id'][::-1], s['K'][::-1], s['H'], s['W'])
    _, m1 = _raster(generic_raster, many['verts'], many['mesh_id'], many['K'], many['H'], many['W'])
    _, m2 = _raster(generic_raster, many['verts'][3:5], many['mesh_id'][3:5], many['K'][3:5], many['H'], many['W'])
    for k in MAPS:
        assert a[k].tobytes() == b[k].tobytes(), k
        assert a[k][1:].tobytes() == alone[k].tobytes() and a[k][::-1].tobytes() == swapped[k].tobytes(), k
        assert m1[k][3:5].tobytes() == m2[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------------- overlay
def _overlay_scene():
    """hand: three quads (z = 2, 8, 2); object: the tetrahedron (2 < z < 4 in front, 4 behind) and a quad at z = 2 under the hand's third"""
    K = R.dyadic_K()
    q1, f2, _ = R.quad_scene(3.5, 11.5, 2.5, 10.5, 2.0)
    q2 = R.quad_scene(14.5, 26.5, 4.5, 12.5, 8.0)[0]
    q3 = R.quad_scene(3.5, 6.5, 13.5, 16.5, 2.0)[0]
    hand_v, hand_f = np.concatenate([q1, q2, q3]), np.concatenate([f2, f2 + 4, f2 + 8])
    tv, tf, _ = R.tetra_scene()
    obj_v, obj_f = np.concatenate([tv, q3]), np.concatenate([tf, f2 + 4])
    return K, (hand_v, hand_f), (obj_v, obj_f)


@pytest.mark.parametrize('exact', [True, False])
def test_overlay_against_the_float64_restatement(exact):
    ops = _ops()
    K, (hv, hf), (ov, of) = _overlay_scene()
    H, W = 24, 32
    meshes = [(len(hv), hf), (len(ov), of)]
    mr = ops.MeshRaster(meshes, 'cuda')
    Kd = _dev(K[None], torch.float64)
    hand = mr.raster(_dev(hv[None]), [0], Kd, H, W, back=False)
    obj = mr.raster(_dev(ov[None]), [1], Kd, H, W, back=False)
    r = np.random.default_rng(9)
    if exact:        # dyadic image, mean, std and colours, opacity 0 or 1, ambient 1 (shade == 1): every product and sum is exact
        image = (r.integers(-8, 9, (1, 3, H, W)) / 16.0).astype(np.float32)
        mean, std, ambient = (0.5, 0.25, 0.375), (0.25, 0.5, 0.125), 1.0
        hand_par, obj_par = dict(colour=(200.0, 64.5, 16.0), opacity=1.0), dict(colour=(32.0, 96.0, 255.0), opacity=0.0)
    else:
        image = r.normal(0, 1.2, (1, 3, H, W)).astype(np.float32)
        mean, std, ambient = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 0.3
        hand_par, obj_par = dict(colour=(224.0, 160.0, 128.0), opacity=0.75), dict(colour=(96.0, 160.0, 224.0), opacity=0.6)
    img = _dev(image)
    np_layer = lambda L, par: dict(depth_front=L['depth_front'].cpu().numpy(), face_front=L['face_front'].cpu().numpy(), verts=L['verts'].cpu().numpy(),
                                   mesh_id=L['mesh_id'].cpu().numpy(), **par)
    hd, od, hfm, ofm = (x[0] for x in (np_layer(hand, {})['depth_front'], np_layer(obj, {})['depth_front'], np_layer(hand, {})['face_front'], np_layer(obj, {})['face_front']))
    both = (hfm >= 0) & (ofm >= 0)
    kinds = {'hand only': (hfm >= 0) & (ofm < 0), 'object only': (hfm < 0) & (ofm >= 0), 'hand over object': both & (hd < od), 'object over hand': both & (od < hd),
             'exact tie': both & (hd == od), 'uncovered': (hfm < 0) & (ofm < 0)}
    print({k: int(v.sum()) for k, v in kinds.items()})
    assert all(v.any() for v in kinds.values()), {k: int(v.sum()) for k, v in kinds.items()}
    worst = 0
    for use_hand, use_obj in ((True, True), (True, False), (False, True), (False, False)):
        got = mr.overlay(img, Kd, hand=dict(hand, **hand_par) if use_hand else None, obj=dict(obj, **obj_par) if use_obj else None, mean=mean, std=std,
                         ambient=ambient)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (1, H, W, 3) and got.dtype == np.uint8
        _, want = R.overlay(image, mean, std, K[None], np_layer(hand, hand_par) if use_hand else None, np_layer(obj, obj_par) if use_obj else None, meshes, ambient)
        diff = int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max())
        worst = max(worst, diff)
        if use_hand and use_obj and exact:
            assert (got[0][kinds['exact tie']] == [200, 64, 16]).all()              # the hand wins the tie (64.5 rounds to even)
            assert (got[0][kinds['object over hand']] == want[0][kinds['object over hand']]).all()
    print(f'overlay exact={exact}: worst byte difference {worst}')
    assert worst <= (0 if exact else 1)


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(monkeypatch):
    ops = _ops()
    v, f, K = R.quad_scene()
    mr = ops.MeshRaster([(4, f)], 'cuda')
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, '_call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    with pytest.raises(ops.VphoError, match='2049'):
        mr.raster(_dev(v[None]), [0], _dev(K[None]), 2049, 32)
    with pytest.raises(ops.VphoError, match='2049'):
        mr.raster(_dev(v[None]), [0], _dev(K[None]), 32, 2049)
    with pytest.raises(ops.VphoError, match='outside the 4 vertices'):
        ops.MeshRaster([(4, np.array([[0, 1, 4]]))], 'cuda')
    with pytest.raises(ops.VphoError, match='integer'):
        ops.MeshRaster([(4, np.array([[0.0, 1.0, 2.0]]))], 'cuda')
    with pytest.raises(ops.VphoError, match='mesh_id 1 lies outside'):
        mr.raster(_dev(v[None]), [1], _dev(K[None]), 24, 32)
    with pytest.raises(ops.VphoError, match='mesh_id -1 lies outside'):
        mr.raster(_dev(v[None]), torch.tensor([-1]), _dev(K[None]), 24, 32)
    with pytest.raises(ops.VphoError, match='2049'):
        mr.overlay(torch.zeros(1, 3, 2049, 8, device='cuda'), _dev(K[None]))
    assert calls == []
    # the library refuses the size too, should a caller get past the wrapper
    with pytest.raises(ops.VphoError, match='bad size'):
        real('vpho_mesh_raster_f32', ops.C.byref(mr.table), _dev(v[None]), 4, _dev(np.zeros(1, np.int32)), _dev(K[None]),
             1, 2049, 8, 2, 0.01, None, None, None, None, None)
    mr.raster(_dev(v[None]), [0], _dev(K[None]), 2048, 3)                         # the largest side is served
    torch.cuda.synchronize()
    assert calls == ['vpho_mesh_raster_f32']


# ---------------------------------------------------------------------------------------------------------------------- end to end
KEYS = ('sample_num', 'sampling_steps', 'topk_hand', 'topk_obj', 'sample_T0', 'eval_batch_size', 'num_batches', 'random_seed', 'checkpoint',
        'clean_data_mode', 'infer_render')
INDEX = [[41, 3], [17, 0], [8]]


@pytest.fixture()
def small_cfg():
    from vpho_amd.configs.args import cfg
    saved = {k: getattr(cfg, k) for k in KEYS}
    cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 4, 5, 8, 3, 0.2
    cfg.eval_batch_size, cfg.num_batches, cfg.random_seed, cfg.checkpoint, cfg.clean_data_mode = 2, 3, 7, None, '2023_CVPR_HFL'
    yield cfg
    for k, v in saved.items():
        setattr(cfg, k, v)


def _batches(t):
    from vpho_amd.synth import synth_batch
    res = []
    for i, idx in enumerate(INDEX):
        b = synth_batch(2, t.assets, seed=7 + i, rank=0)
        b = {k: v[:len(idx)] for k, v in b.items()}
        b['index'] = torch.tensor(idx)
        b['rgb_path'] = [f'img/{j:05d}.jpg' for j in idx]
        res.append(b)
    return res


def test_infer_render_end_to_end(small_cfg, tmp_path):
    from vpho_amd import infer as INF
    from vpho_amd.model.engine import Engine
    from vpho_amd.trainer import Trainer
    t = Trainer(small_cfg)
    batches = _batches(t)
    runs = {}
    for n_render in (3, 0):
        small_cfg.infer_render = n_render
        torch.manual_seed(11)
        res = t.infer(loader=iter(batches), save_dir=str(tmp_path / f'run{n_render}'))
        files = res['files']
        runs[n_render] = (res, INF.read_submission_zip(files['hand_reg'])[1], INF.read_submission_zip(files['hand_diff'])[1],
                          open(files['prediction'], 'rb').read())
    res, res0 = runs[3][0], runs[0][0]
    assert 'render' not in res0 and not os.path.exists(tmp_path / 'run0' / 'render')
    assert set(res) - set(res0) == {'render'} and res['render']['images'] == 3 and res['render']['dir'] == str(tmp_path / 'run3' / 'render')
    assert runs[3][1:3] == runs[0][1:3]                                          # the submissions: identical bytes
    a, b = pickle.loads(runs[3][3]), pickle.loads(runs[0][3])
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert x['path'] == y['path'] and all(x[k].tobytes() == y[k].tobytes() for k in ('index', 'pd_obj_rt', 'pd_hand_vert', 'pd_hand_joint'))
    assert sorted(os.listdir(tmp_path / 'run3' / 'render')) == ['00000003.png', '00000017.png', '00000041.png']       # the first three images seen
    # what MeshRenderer.overlay returns for those images, from the same predictions made sequentially
    from vpho_amd import render
    rnd = render.MeshRenderer(t.assets, 'cuda')
    eng = Engine(t.model)
    torch.manual_seed(11)
    want = {}
    for bt, idx in zip(batches, INDEX):
        gb = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in bt.items()}
        n = gb['rgb'].shape[0]
        nh, no = torch.randn(n * small_cfg.sample_num, 96), torch.randn(n * small_cfg.sample_num, 9)
        out = eng.predict(gb, noise_hand=nh, noise_obj=no)
        img = rnd.overlay(gb, out).cpu().numpy()
        bare = rnd.raster.overlay(gb['rgb'], gb['cam_intr_crop_flip'], mean=render.IMG_MEAN, std=render.IMG_STD).cpu().numpy()      # no layer: the crop itself
        assert img.shape == (n, 256, 256, 3)
        want.update({j: (img[i], int((img[i] != bare[i]).any(-1).sum())) for i, j in enumerate(idx)})
    for j in (41, 3, 17):
        png = render.read_png(str(tmp_path / 'run3' / 'render' / f'{j:08d}.png'))
        print(f'image {j}: the meshes changed {want[j][1]} pixels of the crop')
        assert png.shape == (256, 256, 3) and np.array_equal(png, want[j][0]), j
        assert want[j][1] > 100, j                                                  # something was drawn

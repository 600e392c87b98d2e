"""Hand-object penetration on the device (--eval_physics): the kernel's inside flags against the reference's own MeshIntersector
(golden_penetration.npz), its signed distances against the float64 oracle (tests/_penetration_fp64.py) and closed forms, edge
cases, and the end-to-end evaluation with the flag."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tests._penetration_fp64 as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_penetration.npz'))


def _fixture_meshes():
    out = {}
    for i, name in enumerate(G['names']):
        out[str(name)] = dict(verts=G['verts'][G['vert_offset'][i]:G['vert_offset'][i + 1]],
                              faces=G['faces'][G['face_offset'][i]:G['face_offset'][i + 1]].astype(np.int64))
    return out


def _eye_rt(n):
    rt = torch.zeros((n, 3, 4), dtype=torch.float64, device='cuda')
    rt[:, :, :3] = torch.eye(3, dtype=torch.float64)
    return rt


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def icosphere(levels=5):
    """unit icosphere of 20 * 4^levels triangles, built with + - * / sqrt only (bit-reproducible)"""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.sqrt(np.dot(p, p)) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid = {}

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = (v[a] + v[b]) / 2.0
                v.append(p / np.sqrt(np.dot(p, p)))
                mid[k] = len(v) - 1
            return mid[k]
        f = [g for a, b, c in f for g in ((a, m(a, b), m(c, a)), (b, m(b, c), m(a, b)), (c, m(c, a), m(b, c)), (m(a, b), m(b, c), m(c, a)))]
    return np.array(v), np.array(f, np.int64)


def test_inside_flags_equal_reference_fixture_and_sd_matches_oracle():
    from vpho_amd import ops
    meshes = _fixture_meshes()
    H = ops.HandObjectPenetration(meshes, 'cuda')
    po = G['point_offset']
    P = int(po[1] - po[0])
    assert all(int(po[i + 1] - po[i]) == P for i in range(len(meshes)))
    verts = torch.from_numpy(G['points'].reshape(len(meshes), P, 3)).cuda()
    per, sd, inside = H(verts, _eye_rt(len(meshes)), list(range(len(meshes))), per_vertex=True)
    inside, sd = inside.cpu().numpy().astype(bool).reshape(-1), sd.cpu().numpy().reshape(-1)
    ref = G['contains_ref']
    for i, name in enumerate(meshes):
        sl = slice(po[i], po[i + 1])
        bad = np.nonzero(inside[sl] != ref[sl])[0]
        assert len(bad) == 0, (name, len(bad), G['points'][sl][bad[:5]])
    want = np.where(ref, -G['d_ours'], G['d_ours'])
    np.testing.assert_allclose(sd, want, rtol=0, atol=1e-10)


def test_box_grid_against_closed_form(assets):
    from vpho_amd import ops
    from vpho_amd.physics_eval import object_meshes
    meshes = object_meshes(assets)
    H = ops.HandObjectPenetration(meshes, 'cuda')
    names = list(meshes)[:3]
    rows = []
    for n in names:
        bb = np.asarray(assets['ycb'][n]['bbox3d'], np.float64)
        lo, hi = bb.min(0), bb.max(0)
        # a grid off the mesh's own grid lines: a point whose xy projection lies ON a projected edge is strictly inside neither
        # triangle, the parity rule then misses a crossing (the reference's behaviour, pinned by the fixture test above)
        ax = [np.linspace(lo[k] - 0.02, hi[k] + 0.02, 17) + 0.00131 * (k + 1) for k in range(3)]
        rows.append(np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3).astype(np.float32))
    pts = np.stack(rows)
    per, sd, inside = H(torch.from_numpy(pts).cuda(), _eye_rt(3), H.obj_ids(names), per_vertex=True)
    sd = sd.cpu().numpy()
    for i, n in enumerate(names):
        bb = np.asarray(assets['ycb'][n]['bbox3d'], np.float64)
        ref = O.box_sd(bb.min(0), bb.max(0), pts[i].astype(np.float64))
        np.testing.assert_allclose(sd[i], ref, rtol=0, atol=1e-12)
        assert (ref < -1e-9).sum() > 100


def test_icosphere_spans_many_lds_tiles():
    from vpho_amd import ops
    v, f = icosphere(5)
    assert len(f) == 20480
    v = v * 0.06
    H = ops.HandObjectPenetration({'ico': dict(verts=v, faces=f)}, 'cuda')
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(300, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pts = (dirs * rng.uniform(0.02, 0.09, size=(300, 1))).astype(np.float32)
    per, sd, inside = H(torch.from_numpy(pts[None]).cuda(), _eye_rt(1), [0], per_vertex=True)
    ins = O.contains(v, f, pts, chunk=32)
    d = O.distance(v, f, pts, chunk=16)
    assert np.array_equal(inside.cpu().numpy()[0].astype(bool), ins)
    np.testing.assert_allclose(sd.cpu().numpy()[0], np.where(ins, -d, d), rtol=0, atol=1e-10)
    assert 50 < ins.sum() < 250


def test_rigid_camera_motion_leaves_sd_unchanged():
    from vpho_amd import ops
    meshes = _fixture_meshes()
    H = ops.HandObjectPenetration(meshes, 'cuda')
    rng = np.random.default_rng(9)
    n, V = 5, 778
    pts = np.stack([G['points'][G['point_offset'][i]:G['point_offset'][i] + V] for i in range(n)]).astype(np.float64)
    obj = np.zeros((n, 3, 4))
    cam = np.zeros((n, 3, 4))
    for i in range(n):
        obj[i, :, :3], obj[i, :, 3] = _random_rotation(rng), rng.uniform(-0.2, 0.2, 3) + [0, 0, 0.6]
        cam[i, :, :3], cam[i, :, 3] = _random_rotation(rng), rng.uniform(-0.3, 0.3, 3)
    # hand vertices in the camera frame: v = R p + t, rounded to fp32 once; the moved copy: R' v + t' in fp64, rounded likewise
    v1 = np.einsum('nij,nvj->nvi', obj[:, :, :3], pts) + obj[:, None, :, 3]
    v1 = v1.astype(np.float32).astype(np.float64)
    per1, sd1, in1 = H(torch.from_numpy(v1.astype(np.float32)).cuda(), torch.from_numpy(obj).cuda(), list(range(n)), per_vertex=True)
    # motion applied to the fp64 model frame points of v1 so the fp32 rounding does not enter: compare via the oracle frame
    p1 = O.model_frame(v1, obj)
    obj2 = np.zeros_like(obj)
    obj2[:, :, :3] = np.einsum('nij,njk->nik', cam[:, :, :3], obj[:, :, :3])
    obj2[:, :, 3] = np.einsum('nij,nj->ni', cam[:, :, :3], obj[:, :, 3]) + cam[:, :, 3]
    v2 = (np.einsum('nij,nvj->nvi', obj2[:, :, :3], p1) + obj2[:, None, :, 3]).astype(np.float32)
    p2 = O.model_frame(v2.astype(np.float64), obj2)
    assert np.abs(p2 - p1).max() < 1e-6                      # same points up to the fp32 rounding of the moved copy
    per2, sd2, in2 = H(torch.from_numpy(v2).cuda(), torch.from_numpy(obj2).cuda(), list(range(n)), per_vertex=True)
    # the kernel's sd at the points it actually saw: equal to the fp64 oracle at p1 / p2, and p1 vs p2 differ by the fp32 rounding only
    for p, sd, ins in ((p1, sd1, in1), (p2, sd2, in2)):
        for i, name in enumerate(meshes):
            m = meshes[name]
            d = O.distance(m['verts'], m['faces'], p[i])
            c = O.contains(m['verts'], m['faces'], p[i])
            assert np.array_equal(ins.cpu().numpy()[i].astype(bool), c)
            np.testing.assert_allclose(sd.cpu().numpy()[i], np.where(c, -d, d), rtol=0, atol=1e-12)
    # a camera motion that fp32 represents exactly (a rotation by a signed permutation): the same points, sd to 1e-12 m
    Pm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    obj3 = obj.copy()
    obj3[:, :, :3] = np.einsum('ij,njk->nik', Pm, obj[:, :, :3])
    obj3[:, :, 3] = np.einsum('ij,nj->ni', Pm, obj[:, :, 3])
    v3 = np.einsum('ij,nvj->nvi', Pm, v1).astype(np.float32)
    assert np.array_equal(v3.astype(np.float64), np.einsum('ij,nvj->nvi', Pm, v1))
    per3, sd3, in3 = H(torch.from_numpy(v3).cuda(), torch.from_numpy(obj3).cuda(), list(range(n)), per_vertex=True)
    np.testing.assert_allclose(sd3.cpu().numpy(), sd1.cpu().numpy(), rtol=0, atol=1e-12)


def test_far_hand_odd_sizes_and_errors(assets):
    from vpho_amd import ops
    from vpho_amd.physics_eval import object_meshes
    H = ops.HandObjectPenetration(object_meshes(assets), 'cuda')
    rng = np.random.default_rng(2)
    rt = _eye_rt(3)
    for V in (1, 255, 257, 778):
        far = torch.from_numpy(rng.uniform(-0.05, 0.05, size=(3, V, 3)).astype(np.float32) + np.float32(5.0)).cuda()
        per = H(far, rt, [0, 4, 20]).cpu().numpy()
        assert per.shape == (3, 4) and (per[:, 0] == 0).all() and (per[:, 1] == 0).all() and (per[:, 3] == 0).all()
        assert (per[:, 2] > 4.5).all()
        near = torch.from_numpy(rng.uniform(-0.02, 0.02, size=(3, V, 3)).astype(np.float32)).cuda()
        per, sd, inside = H(near, rt, [1, 2, 3], per_vertex=True)
        s, ins = sd.cpu().numpy(), inside.cpu().numpy().astype(bool)
        assert sd.shape == (3, V) and inside.shape == (3, V)
        np.testing.assert_array_equal(per.cpu().numpy(), O.reduce(s, ins, 0.005))           # per_image = reduction of the kernel's own sd
        assert ins.all()                                                                    # every synthetic box is >= 25 mm per side
    per = H(torch.zeros((0, 778, 3), device='cuda'), _eye_rt(0), [])
    assert per.shape == (0, 4)
    with pytest.raises(ops.VphoError, match='outside'):
        H(near, rt, [0, 1, 21])
    with pytest.raises(ops.VphoError):
        H.obj_ids(['no_such_object'])
    dev_bad = torch.tensor([0, 99, 1], dtype=torch.int32, device='cuda')
    per = H(near, rt, dev_bad).cpu().numpy()
    assert np.isnan(per[1]).all() and np.isfinite(per[[0, 2]]).all()
    with pytest.raises(ops.VphoError, match='GPU'):
        H(near.cpu(), rt, [0, 1, 2])
    with pytest.raises(ops.VphoError, match='GPU'):
        H(near, rt.cpu(), [0, 1, 2])
    # sd / inside may be NULL in the C ABI: the per-image result is the same
    per_ref = H(near, rt, [1, 2, 3])
    per2 = torch.empty_like(per_ref)
    ops._call('vpho_hand_obj_penetration_f64', ops.C.byref(H.c), near, 3, near.shape[1], rt,
              H.obj_ids(list(H.names[1:4])), 0.005, None, None, per2)
    assert torch.equal(per2, per_ref)


def _eval_cfg():
    from vpho_amd.configs.args import cfg
    keys = ('sample_num', 'sampling_steps', 'topk_hand', 'topk_obj', 'sample_T0', 'eval_batch_size', 'num_batches', 'random_seed', 'checkpoint',
            'eval_best', 'eval_physics')
    saved = {k: getattr(cfg, k) for k in keys}
    cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 6, 5, 4, 3, 0.2
    cfg.eval_batch_size, cfg.num_batches, cfg.random_seed, cfg.checkpoint, cfg.eval_best, cfg.eval_physics = 3, 2, 7, None, False, False
    return cfg, saved


def test_trainer_eval_physics_end_to_end(monkeypatch, capsys):
    from vpho_amd import evaluate as E
    from vpho_amd import ops
    from vpho_amd.trainer import Trainer
    cfg, saved = _eval_cfg()
    calls = []
    orig_block = E.physics_block

    def spy(pp, out, data, gt_vert, meshes):
        blk = orig_block(pp, out, data, gt_vert, meshes)
        calls.append((pp['agg_hand_vert'].clone(), out['agg_obj_6d'].clone(), data['root_joint'].clone(), list(data['obj_name']),
                      gt_vert.clone(), data['gt_obj_rt'].clone(), blk.clone(), meshes))
        return blk
    try:
        t = Trainer(cfg)
        res = {}
        for best in (False, True):
            torch.manual_seed(11)
            res[best, False] = t.eval(eval_best=best)
            monkeypatch.setattr(E, 'physics_block', spy)
            torch.manual_seed(11)
            res[best, True] = t.eval(eval_best=best, eval_physics=True)
            monkeypatch.setattr(E, 'physics_block', orig_block)
        text = capsys.readouterr().out
        # without the flag the penetration code is never called
        def boom(*a, **k):
            raise AssertionError('HandObjectPenetration called without eval_physics')
        monkeypatch.setattr(ops.HandObjectPenetration, '__call__', boom)
        torch.manual_seed(11)
        again = t.eval()
        monkeypatch.undo()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    assert torch.equal(again, res[False, False])
    for best in (False, True):
        plain, wide = res[best, False], res[best, True]
        w = E.RowLayout.resolve(eval_best=best).width
        assert plain.shape == (6, w) and wide.shape == (6, E.RowLayout.resolve(eval_best=best, eval_physics=True).width)
        assert torch.equal(wide[:, :w], plain)
        assert torch.isfinite(wide).all()
    # the physics columns are a direct HandObjectPenetration call on the same outputs
    blocks = []
    for hv, o6, root, names, gv, grt, blk, meter in calls:
        pd_rt = ops.obj_9d_to_rt(o6.double().contiguous(), root.float().contiguous())
        ids = meter.obj_ids(names)
        direct = torch.cat([meter(hv.float().contiguous(), pd_rt, ids, 0.005), meter(gv.float().contiguous(), grt.double().contiguous(), ids, 0.005)], 1)
        assert torch.equal(direct.float(), blk)
        blocks.append(blk)
    got = torch.cat(blocks[:len(blocks) // 2]).cpu().numpy()
    phys = res[False, True][:, -E.PHYS:].cpu().numpy()
    order = lambda a: a[np.lexsort(a.T[::-1])]
    np.testing.assert_array_equal(order(got), order(phys))
    line = [l for l in text.splitlines() if l.startswith('EVAL_JSON ')][-1]
    table = json.loads(line[len('EVAL_JSON '):])['table']
    assert set(table['physics']) == {'pred', 'gt'} and 'best_of_S' in table
    assert 'physics pred:' in text and not [l for l in text.splitlines() if l.lstrip().startswith('physics:')]


def test_main_eval_physics_prints_the_table():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    args = ['--sample_num', '4', '--sampling_steps', '5', '--topk_hand', '8', '--topk_obj', '3', '--sample_T0', '0.2',
            '--eval_batch_size', '2', '--num_batches', '2', '--random_seed', '7', '--eval_physics']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--mode', 'eval', '--model', 'vpho_net'] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, r.stdout[-2000:]
    table = json.loads(line[0][len('EVAL_JSON '):])['table']
    from vpho_amd.ops_names import PHYSICS_TABLE
    assert tuple(table['physics']['pred']) == PHYSICS_TABLE and tuple(table['physics']['gt']) == PHYSICS_TABLE
    assert 'physics pred:' in r.stdout and 'physics gt:' in r.stdout

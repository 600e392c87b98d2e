"""Hand-object intersection volume on the device (--eval_volume): the kernels' per-centre flags and counts against the reference's own
MeshIntersector (golden_volume.npz) and the numpy restatement in the documented order of operations (tests/_volume_fp64.py), a closed
form, edge cases, the object solids, the row layout with the flag off, and the end-to-end evaluation with the flag."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tests._penetration_fp64 as O
import tests._volume_fp64 as VO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_volume.npz'))
N_PAIRS = len(G['pair_hand'])
H_PITCH = float(G['pitch'])
EVAL_ARGS = dict(sample_num=4, sampling_steps=5, topk_hand=8, topk_obj=3, sample_T0=0.2, eval_batch_size=2, num_batches=2, random_seed=7)
_SHARED = {}


def _eye_rt(n):
    rt = torch.zeros((n, 3, 4), dtype=torch.float64, device='cuda')
    rt[:, :, :3] = torch.eye(3, dtype=torch.float64)
    return rt


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


@pytest.fixture(scope='module')
def meter():
    """the two fixture objects, their solids at the fixture's pitch"""
    from vpho_amd import ops
    meshes = {str(n): dict(verts=G[f'obj{i}_verts'], faces=G[f'obj{i}_faces'].astype(np.int64)) for i, n in enumerate(G['obj_names'])}
    m = ops.HandObjectPenetration(meshes, 'cuda', accel=False)
    m.build_solids(H_PITCH)
    return m


def _fixture_run(meter, hand, key):
    """all pairs of one hand mesh in ONE call -> [(pair index, n_cells, IV, flags of the object's solid centres)]"""
    pairs = [i for i in range(N_PAIRS) if int(G['pair_hand'][i]) == hand]
    meter.set_hand_faces(G[f'hand{hand}_faces'])
    verts = torch.from_numpy(np.stack([G[f'pair{i}_verts_model' if key == 'eye' else f'pair{i}_verts_cam'] for i in pairs])).cuda()
    rt = _eye_rt(len(pairs)) if key == 'eye' else torch.from_numpy(G['rt'][pairs]).cuda()
    out, flags = meter.volume(verts, rt, [int(G['pair_obj'][i]) for i in pairs], H_PITCH, flags=True)
    out, flags = out.cpu().numpy(), flags.cpu().numpy()
    return [(i, out[j, 0], out[j, 1], flags[j]) for j, i in enumerate(pairs)]


@pytest.mark.parametrize('key', ['eye', 'pose'])
@pytest.mark.parametrize('hand', range(3))
def test_flags_and_counts_equal_the_reference_fixture(meter, hand, key):
    sol = meter.build_solids(H_PITCH)
    for i, cells, iv, flags in _fixture_run(meter, hand, key):
        o = int(G['pair_obj'][i])
        solid = G[f'obj{o}_solid']
        assert sol['counts'][o] == int(solid.sum())
        ref = G[f'pair{i}_flags_{key}'][solid]                                  # the reference's flag of every solid centre, in lattice order
        got = flags[:len(ref)].astype(bool)
        bad = np.nonzero(got != ref)[0]
        assert len(bad) == 0, (i, key, len(bad), G[f'obj{o}_centres'][solid][bad[:5]])
        assert not flags[len(ref):].any()                                       # nothing behind the object's last centre
        assert cells == int(G[f'cells_{key}'][i]) == int(ref.sum())
        assert iv == (H_PITCH * H_PITCH) * H_PITCH * cells                      # IV = ((h h) h) n_cells, to the bit
        # ... and the restatement in the documented order of operations (the real poses: q_v = R^T (v - t) with the kernel's bits)
        pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1) if key == 'eye' else G['rt'][i]
        qv = VO.model_frame(G[f'pair{i}_verts_model' if key == 'eye' else f'pair{i}_verts_cam'], pose)
        again = VO.hand_inside(qv, G[f'hand{hand}_faces'].astype(np.int64), G[f'obj{o}_centres'][solid])
        assert np.array_equal(got, again)


def test_object_solids_equal_the_fp64_restatement(meter, assets):
    from vpho_amd import ops
    from vpho_amd.physics_eval import box_mesh, solid_lattice
    sol = meter.build_solids(H_PITCH)
    assert meter.build_solids(H_PITCH) is sol                                   # once per pitch
    off = sol['pt_offset'].cpu().numpy()
    pts = sol['pts'].cpu().numpy()
    for o in range(2):
        c = G[f'obj{o}_centres']
        want = c[O.contains(G[f'obj{o}_verts'], G[f'obj{o}_faces'], c)]
        assert np.array_equal(pts[off[o]:off[o + 1]], want) and np.array_equal(want, c[G[f'obj{o}_solid']])
        assert sol['dims'][o] == tuple(G[f'obj{o}_dims'])
    assert sol['max_pts'] == max(sol['counts']) and off[-1] == sum(sol['counts'])
    # a synthetic box (3 072 triangles) at a coarser pitch, more than one block of centres: the count of a box is a product of three
    name = list(assets['ycb'])[3]
    v, f = box_mesh(assets['ycb'][name]['bbox3d'])
    m = ops.HandObjectPenetration({name: dict(verts=v, faces=f)}, 'cuda', accel=False)
    s2 = m.build_solids(0.0075)
    c, dims = solid_lattice(v, f, 0.0075)
    want = c[O.contains(v, f, c)]
    assert len(c) > 256 and np.array_equal(s2['pts'].cpu().numpy(), want)
    lo, hi = v.min(0), v.max(0)
    per_axis = [np.unique(c[:, a]).astype(np.float64) for a in range(3)]
    assert len(want) == int(np.prod([((lo[a] < x) & (x < hi[a])).sum() for a, x in enumerate(per_axis)]))


def _count_in_box(centres, lo, hi):
    c = centres.astype(np.float64)
    return int(np.all((lo < c) & (c < hi), axis=1).sum())


@pytest.mark.parametrize('posed', [False, True])
def test_box_hand_in_box_object_gives_the_closed_form_count(meter, posed):
    """a box "hand" overlapping box A: n_cells is the number of the object's solid centres inside the intersection box.  The hand's faces lie
    at least 0.3 mm from every centre coordinate, far above the 1e-9 m the pose round trip can move them."""
    from vpho_amd.physics_eval import box_mesh
    o = 0
    solid = G[f'obj{o}_centres'][G[f'obj{o}_solid']]
    lo, hi = np.array([-0.0139, -0.0302, 0.0011]), np.array([0.0312, 0.0068, 0.0402])          # sticks out of the object on three sides
    for a in range(3):
        assert np.abs(solid[:, a].astype(np.float64)[:, None] - np.array([lo[a], hi[a]])[None]).min() > 3e-4
    hv, hf = box_mesh(np.stack([lo, hi]), sub=3)
    meter.set_hand_faces(hf)
    rng = np.random.default_rng(5)
    rt = np.concatenate([_rotation(rng), np.array([[0.04], [-0.02], [0.61]])], 1) if posed else np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    verts = (hv @ rt[:, :3].T + rt[:, 3]).astype(np.float32)
    out, flags = meter.volume(torch.from_numpy(verts[None]).cuda(), torch.from_numpy(rt[None]).cuda(), [o], H_PITCH, flags=True)
    want = np.all((lo < solid.astype(np.float64)) & (solid < hi), axis=1)
    ov = G[f'obj{o}_verts']
    assert int(want.sum()) == _count_in_box(solid, np.maximum(lo, ov.min(0)), np.minimum(hi, ov.max(0))) > 50
    assert np.array_equal(flags[0, :len(solid)].cpu().numpy().astype(bool), want)
    assert float(out[0, 0]) == want.sum() and float(out[0, 1]) == (H_PITCH * H_PITCH) * H_PITCH * float(want.sum())


def _uv_sphere(rings=8, segs=97):
    """closed, outward mesh of 2 + rings * segs vertices and 2 * rings * segs faces: 778 vertices and 1 552 faces, MANO's sizes"""
    th = (np.arange(rings) + 1) * np.pi / (rings + 1)
    ph = np.arange(segs) * 2 * np.pi / segs
    v = [[0.0, 0.0, 1.0]] + [[np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)] for t in th for p in ph] + [[0.0, 0.0, -1.0]]
    idx = lambda r, s: 1 + r * segs + s % segs
    last = 1 + rings * segs
    f = [(0, idx(0, s), idx(0, s + 1)) for s in range(segs)]
    for r in range(rings - 1):
        for s in range(segs):
            f += [(idx(r, s), idx(r + 1, s), idx(r + 1, s + 1)), (idx(r, s), idx(r + 1, s + 1), idx(r, s + 1))]
    f += [(last, idx(rings - 1, s + 1), idx(rings - 1, s)) for s in range(segs)]
    return np.array(v), np.array(f, np.int64)


def test_mano_sized_mesh_repeat_runs_and_flags_on_off(assets):
    """V = 778, F = 1 552 (seven LDS tiles, the last one partial), three images with three objects of different solid sizes at 5 mm, several
    blocks of centres each: the count equals the restatement's, twice, and with and without the per-centre flags"""
    from vpho_amd import ops
    from vpho_amd.physics_eval import box_mesh, close_mesh
    sv, sf = _uv_sphere()
    assert sv.shape == (778, 3) and sf.shape == (1552, 3) and np.array_equal(close_mesh(sf), sf)
    names = list(assets['ycb'])[:3]
    meshes = {n: dict(zip(('verts', 'faces'), box_mesh(assets['ycb'][n]['bbox3d'], 4))) for n in names}
    m = ops.HandObjectPenetration(meshes, 'cuda', accel=False, hand_faces=sf)
    sol = m.build_solids(0.005)
    assert min(sol['counts']) > 256 and len(set(sol['counts'])) == 3
    rng = np.random.default_rng(9)
    verts, rts = [], []
    for i, n in enumerate(names):
        half = np.asarray(assets['ycb'][n]['bbox3d'], np.float64).max(0)
        centre = half * np.array([0.9, 0.2, -0.5])                              # an ellipsoid through one side of the box
        hm = (sv * np.array([0.034, 0.013, 0.027])) @ _rotation(rng).T + centre
        rt = np.concatenate([_rotation(rng), rng.uniform(-0.1, 0.1, (3, 1)) + np.array([[0.0], [0.0], [0.6]])], 1)
        verts.append((hm @ rt[:, :3].T + rt[:, 3]).astype(np.float32))
        rts.append(rt)
    tv, trt = torch.from_numpy(np.stack(verts)).cuda(), torch.from_numpy(np.stack(rts)).cuda()
    ids = m.obj_ids(names)
    out, flags = m.volume(tv, trt, ids, 0.005, flags=True)
    off, pts = sol['pt_offset'].cpu().numpy(), sol['pts'].cpu().numpy()
    for i in range(3):
        want = VO.hand_inside(VO.model_frame(verts[i], rts[i]), sf, pts[off[i]:off[i + 1]])
        assert want.sum() > 20
        assert np.array_equal(flags[i, :sol['counts'][i]].cpu().numpy().astype(bool), want) and not flags[i, sol['counts'][i]:].any()
        assert float(out[i, 0]) == want.sum()
    assert torch.equal(out[:, 1], out[:, 0] * ((0.005 * 0.005) * 0.005))
    for _ in range(2):
        assert torch.equal(m.volume(tv, trt, ids, 0.005), out)
    out2, flags2 = m.volume(tv, trt, ids, 0.005, flags=True)
    assert torch.equal(out2, out) and torch.equal(flags2, flags)
    # another pitch: its own solids, and IV stays near the 5 mm value (the same solid, sampled more finely)
    fine = m.volume(tv, trt, ids, 0.0025)
    assert (fine[:, 0] > 4 * out[:, 0]).all() and torch.allclose(fine[:, 1], out[:, 1], rtol=0.25)


def test_edge_cases(meter):
    from vpho_amd import ops
    meter.set_hand_faces(G['hand0_faces'])
    verts = torch.from_numpy(G['pair0_verts_cam'][None]).cuda()
    rt = torch.from_numpy(G['rt'][:1]).cuda()
    empty = meter.volume(verts[:0], rt[:0], [], H_PITCH)
    assert empty.shape == (0, 2) and empty.dtype == torch.float64
    e2, f2 = meter.volume(verts[:0], rt[:0], [], H_PITCH, flags=True)
    assert e2.shape == (0, 2) and f2.shape[0] == 0
    for bad in ([2], [-1], [0, 1]):
        with pytest.raises(ops.VphoError, match='object ids'):
            meter.volume(verts, rt, bad, H_PITCH)
    for pitch in (0.0, -0.005):
        with pytest.raises(ops.VphoError, match='pitch'):
            meter.volume(verts, rt, [0], pitch)
    with pytest.raises(ops.VphoError):
        meter.set_hand_faces(np.zeros((0, 3), np.int64))
    with pytest.raises(ops.VphoError, match='index vertex'):
        meter.volume(verts[:, :50].contiguous(), rt, [0], H_PITCH)            # the faces index vertices the hands do not have
    # the C entry point refuses F = 0 and pitch <= 0 before any launch
    sol = meter.build_solids(H_PITCH)
    out = torch.zeros((1, 2), dtype=torch.float64, device='cuda')
    ws = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    ids = meter.obj_ids([meter.names[0]])
    call = lambda F_, pitch: ops._call('vpho_hand_obj_intersection_f64', ops.C.byref(meter.c), ops.C.byref(sol['c']), meter.hand_faces, F_,
                                      verts, 1, verts.shape[1], rt, ids, pitch, out,
                                      None, ws, ws.numel())
    with pytest.raises(ops.VphoError, match='without faces'):
        call(0, H_PITCH)
    with pytest.raises(ops.VphoError, match='pitch'):
        call(int(meter.hand_faces.shape[0]), 0.0)
    assert ops.lib.vpho_hand_obj_intersection_workspace_bytes(1, 0) == -1
    # a device id the host cannot check, and a hand vertex that is not a number: NaN rows, the other image untouched
    two_v = torch.from_numpy(np.stack([G['pair0_verts_cam'], G['pair0_verts_cam']])).cuda()
    two_rt = torch.from_numpy(G['rt'][[0, 0]]).cuda()
    got = meter.volume(two_v, two_rt, torch.tensor([0, 7], dtype=torch.int32, device='cuda'), H_PITCH)
    assert float(got[0, 0]) == int(G['cells_pose'][0]) and got[1].isnan().all()
    two_v[1, 5, 1] = float('nan')
    got, fl = meter.volume(two_v, two_rt, [0, 0], H_PITCH, flags=True)
    assert float(got[0, 0]) == int(G['cells_pose'][0]) and got[1].isnan().all() and not fl[1].any()


def _eval_cfg():
    from vpho_amd.configs.args import cfg
    keys = tuple(EVAL_ARGS) + ('checkpoint', 'eval_best', 'eval_physics', 'eval_volume', 'physics_voxel_pitch')
    saved = {k: getattr(cfg, k) for k in keys}
    for k, v in EVAL_ARGS.items():
        setattr(cfg, k, v)
    cfg.checkpoint, cfg.eval_best, cfg.eval_physics, cfg.eval_volume, cfg.physics_voxel_pitch = None, False, False, False, 0.005
    return cfg, saved


def _volume_table_of(text):
    line = [l for l in text.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, text[-2000:]
    return json.loads(line[0][len('EVAL_JSON '):])['table']


def test_trainer_eval_volume_end_to_end_and_rows_without_the_flag(monkeypatch, capsys):
    from vpho_amd import evaluate as E
    from vpho_amd import ops
    from vpho_amd.ops_names import VOLUME_TABLE
    from vpho_amd.trainer import Trainer
    cfg, saved = _eval_cfg()
    calls, first = [], []
    orig_block, orig_rows = E.volume_block, E.metric_rows

    def spy_block(pp, out, data, gt_vert, meshes):
        blk = orig_block(pp, out, data, gt_vert, meshes)
        calls.append((pp['agg_hand_vert'].clone(), out['agg_obj_6d'].clone(), data['root_joint'].clone(), list(data['obj_name']), gt_vert.clone(),
                      data['gt_obj_rt'].clone(), blk.clone(), meshes))
        return blk

    def spy_rows(out, data, gt_joint, gt_vert, first_index, assets=None, *a, **k):
        if not first:
            first.append((out, data, gt_joint, gt_vert, first_index, assets))
        return orig_rows(out, data, gt_joint, gt_vert, first_index, assets, *a, **k)
    try:
        t = Trainer(cfg)                                   # seeds torch with cfg.random_seed, as `main.py --random_seed` does: the child's run
        monkeypatch.setattr(E, 'volume_block', spy_block)
        monkeypatch.setattr(E, 'metric_rows', spy_rows)
        wide = t.eval(eval_volume=True)
        text = capsys.readouterr().out
        monkeypatch.setattr(E, 'volume_block', orig_block)
        monkeypatch.setattr(E, 'metric_rows', orig_rows)
        # the rows of every older flag combination: same width and bits with the keyword off, left out or on (the block comes last)
        out, data, gj, gv, fi, assets = first[0]
        combos = {}
        for best in (False, True):
            for phys in (False, True):
                lay = lambda **more: E.RowLayout.resolve(eval_best=best, eval_physics=phys, **more)
                base = orig_rows(out, data, gj, gv, fi, assets, layout=lay())
                off = orig_rows(out, data, gj, gv, fi, assets, layout=lay(physics_multi=False, eval_volume=False))
                on = orig_rows(out, data, gj, gv, fi, assets, layout=lay(physics_multi=False, eval_volume=True))
                combos[best, phys] = (base, off, on)
        # without the flag the new code is never called
        def boom(*a, **k):
            raise AssertionError('HandObjectPenetration.volume called without eval_volume')
        monkeypatch.setattr(ops.HandObjectPenetration, 'volume', boom)
        torch.manual_seed(int(cfg.random_seed))
        plain = t.eval()
        monkeypatch.undo()
        capsys.readouterr()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    n = EVAL_ARGS['eval_batch_size'] * EVAL_ARGS['num_batches']
    assert plain.shape == (n, 28) and wide.shape == (n, 32)
    for (best, phys), (base, off, on) in combos.items():
        w = {(False, False): 28, (True, False): 88, (False, True): 36, (True, True): 96}[best, phys]
        assert base.shape[1] == off.shape[1] == w and on.shape[1] == w + 4
        assert torch.equal(base.view(torch.int32), off.view(torch.int32)) and torch.equal(on[:, :w].view(torch.int32), base.view(torch.int32))
        assert torch.equal(on[:, w:].view(torch.int32), combos[False, False][2][:, 28:].view(torch.int32))
    # the volume columns are a direct HandObjectPenetration.volume call on the same outputs
    assert len(calls) == EVAL_ARGS['num_batches']
    blocks = []
    for hv, o6, root, names, gv, grt, blk, m in calls:
        pd_rt = ops.obj_9d_to_rt(o6.double().contiguous(), root.float().contiguous())
        ids = m.obj_ids(names)
        direct = torch.cat([m.volume(hv.float().contiguous(), pd_rt, ids, 0.005).flip(1), m.volume(gv.float().contiguous(), grt.double().contiguous(), ids, 0.005).flip(1)], 1)
        assert torch.equal(direct.float(), blk) and torch.isfinite(blk).all()
        assert torch.equal(direct[:, 0], direct[:, 1] * ((0.005 * 0.005) * 0.005))
        blocks.append(blk)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    np.testing.assert_array_equal(order(torch.cat(blocks).cpu().numpy()), order(wide[:, -E.VOL:].cpu().numpy()))
    table = _volume_table_of(text)
    assert set(table['volume']) == {'pred', 'gt'} and all(tuple(v) == VOLUME_TABLE for v in table['volume'].values())
    assert table['volume'] == E.summarize(wide.cpu())['volume'] and 'physics' not in table
    assert 'volume pred (pitch 5 mm):' in text and 'volume gt (pitch 5 mm):' in text
    allb = torch.cat(blocks).double()
    for s, src in enumerate(('pred', 'gt')):
        assert table['volume'][src]['IV_cm3'] == pytest.approx(float(allb[:, 2 * s].mean() * 1e6), rel=1e-12, abs=0)
        assert table['volume'][src]['intersecting_pct'] == float((allb[:, 2 * s + 1] > 0).double().mean() * 100.0)
    _SHARED['table'] = table


def test_main_eval_volume_prints_the_table_of_the_in_process_run(capsys):
    if 'table' not in _SHARED:                             # run on its own: the in-process run of the test above, without its checks
        from vpho_amd.trainer import Trainer
        cfg, saved = _eval_cfg()
        try:
            Trainer(cfg).eval(eval_volume=True)
        finally:
            for k, v in saved.items():
                setattr(cfg, k, v)
        _SHARED['table'] = _volume_table_of(capsys.readouterr().out)
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    args = [x for k, v in EVAL_ARGS.items() for x in ('--' + k, str(v))] + ['--eval_volume']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--mode', 'eval', '--model', 'vpho_net'] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    table = _volume_table_of(r.stdout)
    assert 'physics' not in table and 'volume pred (pitch 5 mm):' in r.stdout and 'volume gt (pitch 5 mm):' in r.stdout
    # the same seeds, the same images: the table of the in-process run, which is checked against direct volume() calls there
    assert table['volume'] == _SHARED['table']['volume']

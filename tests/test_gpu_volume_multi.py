"""The intersection volume of every sampled hypothesis on the device (--eval_best with --eval_volume): the column-walk kernel against the
per-pair kernel (byte for byte) and the reference's own flags (golden_volume.npz), the shapes where a column walk can go wrong, the
one | best | mean table, edge cases, and the end-to-end evaluation with both flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tests._volume_multi_fp64 as VM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_volume.npz'))
H_PITCH = float(G['pitch'])
PAIRS = (0, 1, 2)                                      # objects 0, 1, 0; the fixture's three hand meshes
EVAL_ARGS = dict(sample_num=4, sampling_steps=5, topk_hand=8, topk_obj=3, sample_T0=0.2, eval_batch_size=2, num_batches=2, random_seed=7)
_SHARED = {}


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _flat_volume(m, verts, rt, ids, pitch):
    """the per-pair kernel on the n * S flattened pairs -> per_hyp (n, S, 2), flags (n, S, max_pts)"""
    n, S = verts.shape[:2]
    ids = torch.as_tensor(ids, dtype=torch.int32).to(verts.device) if not torch.is_tensor(ids) else ids
    out, fl = m.volume(verts.reshape(n * S, -1, 3).contiguous(), rt.reshape(n * S, 3, 4).contiguous(), ids.repeat_interleave(S).contiguous(), pitch, flags=True)
    return out.view(n, S, 2), fl.view(n, S, -1)


@pytest.fixture(scope='module')
def fix():
    """n = 3 fixture images x S = 5 (hypothesis 0: the fixture's own pose), one volume_multi call and the 15 per-pair results"""
    from vpho_amd import ops
    meshes = {str(n): dict(verts=G[f'obj{i}_verts'], faces=G[f'obj{i}_faces'].astype(np.int64)) for i, n in enumerate(G['obj_names'])}
    faces, hands = VM.fixture_union(G, PAIRS)
    m = ops.HandObjectPenetration(meshes, 'cuda', accel=False, hand_faces=faces)
    hyp = [VM.perturbed_hypotheses(hands[j], G['rt'][i], 5, seed=40 + i) for j, i in enumerate(PAIRS)]
    verts = torch.from_numpy(np.stack([h[0] for h in hyp])).cuda()
    rt = torch.from_numpy(np.stack([h[1] for h in hyp])).cuda()
    ids = [int(G['pair_obj'][i]) for i in PAIRS]
    table, per, flags = m.volume_multi(verts, rt, ids, H_PITCH, flags=True)
    ref_per, ref_flags = _flat_volume(m, verts, rt, ids, H_PITCH)
    return dict(m=m, verts=verts, rt=rt, ids=ids, table=table, per=per, flags=flags, ref_per=ref_per, ref_flags=ref_flags)


def test_fixture_hands_equal_the_per_pair_kernel_and_the_reference_flags(fix):
    assert fix['per'].shape == (3, 5, 2) and fix['per'].dtype == torch.float64 and fix['flags'].dtype == torch.uint8
    assert _bytes_equal(fix['per'], fix['ref_per']) and _bytes_equal(fix['flags'], fix['ref_flags'])
    cells = fix['per'][..., 0].cpu().numpy()
    assert len(set(cells.reshape(-1).tolist())) >= 6                            # the perturbations move the count
    for j, i in enumerate(PAIRS):
        solid = G[f'obj{int(G["pair_obj"][i])}_solid']
        ref = G[f'pair{i}_flags_pose'][solid]                                   # the reference's flag of every solid centre, lattice order
        got = fix['flags'][j, 0].cpu().numpy()
        assert np.array_equal(got[:len(ref)].astype(bool), ref) and not got[len(ref):].any()
        assert cells[j, 0] == int(G['cells_pose'][i]) == int(ref.sum())
    assert torch.equal(fix['per'][..., 1], ((H_PITCH * H_PITCH) * H_PITCH) * fix['per'][..., 0])          # IV = ((h h) h) cells, to the bit


@pytest.fixture(scope='module')
def shapes():
    """a torus object (more than 256 columns, empty ones, gaps in k), a tall box (70 centres per column) and a 1 552-face torus hand"""
    from vpho_amd import ops
    hv, hf = VM.torus_hand()
    m = ops.HandObjectPenetration(dict(torus=VM.torus_object(), tall=VM.tall_box_object()), 'cuda', accel=False, hand_faces=hf)
    pitch = 0.003
    rng = np.random.default_rng(11)
    where = {0: [((0.045, 0.0, 0.01), 0.0), ((-0.03, 0.005, 0.03), 25.0), ((0.0, 0.0, -0.045), 70.0)],
             1: [((0.0, 0.0, 0.055), 0.0), ((0.002, 0.0, 0.0), 10.0), ((0.0, 0.003, -0.07), -20.0)]}
    posed = [[VM.pose_into(rng, hv, c, tilt) for c, tilt in where[i]] for i in range(2)]
    verts = torch.from_numpy(np.stack([np.stack([p[0] for p in row]) for row in posed])).cuda()
    rt = torch.from_numpy(np.stack([np.stack([p[1] for p in row]) for row in posed])).cuda()
    return dict(m=m, pitch=pitch, verts=verts, rt=rt, ids=[0, 1])


def test_many_columns_gaps_tall_columns_and_a_partial_record_tile(shapes):
    m, pitch = shapes['m'], shapes['pitch']
    sol, cols = m.build_solids(pitch), m.build_solid_columns(pitch)
    assert m.build_solid_columns(pitch) is cols and m.build_solids(pitch) is sol                           # once per pitch, the solids untouched
    assert set(sol) == {'pts', 'pt_offset', 'counts', 'dims', 'max_pts', 'pitch', 'c'}
    cs, co = cols['col_start'].cpu().numpy(), cols['col_offset'].cpu().numpy()
    off = sol['pt_offset'].cpu().numpy()
    assert co.tolist() == [0, cols['counts'][0], sum(cols['counts'])] and cs[-1] == off[-1] and len(cs) == co[-1] + 1
    assert cs[co[1]] == off[1]                                                  # the second object's columns start at its first centre
    d = sol['dims'][0]
    assert 300 <= cols['counts'][0] < d[0] * d[1]                               # more columns than threads; empty columns
    pts = sol['pts'].cpu().numpy()
    k = np.rint((pts[:off[1], 2] - pts[:off[1], 2].min()) / pitch).astype(int)
    runs = [k[a:b] for a, b in zip(cs[:co[1]], cs[1:co[1] + 1])]
    assert sum((np.diff(r) > 1).any() for r in runs) >= 20                      # columns whose centres are not contiguous in k
    assert np.diff(cs[co[1]:]).max() > 64                                       # a column of more than one 64-centre piece
    assert int(m.hand_faces.shape[0]) == 1552 and 1552 % 256 != 0
    table, per, flags = m.volume_multi(shapes['verts'], shapes['rt'], shapes['ids'], pitch, flags=True)
    ref_per, ref_flags = _flat_volume(m, shapes['verts'], shapes['rt'], shapes['ids'], pitch)
    assert _bytes_equal(per, ref_per) and _bytes_equal(flags, ref_flags)
    assert (per[..., 0] > 30).all(), per[..., 0]                                # every pair intersects
    # centres behind the 64th of a tall column are inside the hand in the pair at the box's far end
    assert sol['dims'][1] == (5, 4, 70) and sol['counts'][1] == 5 * 4 * 70
    tall = flags[1, 0, :sol['counts'][1]].cpu().numpy().reshape(20, 70)
    assert tall[:, 64:].any() and tall[:, :64].any()
    for i in range(2):
        assert not flags[i, :, sol['counts'][i]:].any()                         # the max_pts padding stays zero
    _SHARED['shapes'] = (table, per, flags)


def test_without_flags_and_twice(fix, shapes):
    for d, pitch in ((fix, H_PITCH), (shapes, shapes['pitch'])):
        a = d['m'].volume_multi(d['verts'], d['rt'], d['ids'], pitch)
        b = d['m'].volume_multi(d['verts'], d['rt'], d['ids'], pitch, flags=True)
        c = d['m'].volume_multi(d['verts'], d['rt'], d['ids'], pitch, flags=True)
        assert len(a) == 2 and len(b) == 3
        assert _bytes_equal(a[0], b[0]) and _bytes_equal(a[1], b[1])            # flags=False: the same table and per_hyp
        assert all(_bytes_equal(x, y) for x, y in zip(b, c))                    # two calls: equal bytes
    assert _bytes_equal(fix['m'].volume_multi(fix['verts'], fix['rt'], fix['ids'], H_PITCH)[1], fix['per'])


def test_table_is_the_stated_rule(fix, shapes):
    assert fix['table'].shape == (3, 6) and fix['table'].dtype == torch.float64
    assert torch.equal(fix['table'].cpu(), VM.table_rule(fix['per'].cpu(), H_PITCH))
    t2, p2 = shapes['m'].volume_multi(shapes['verts'], shapes['rt'], shapes['ids'], shapes['pitch'])
    assert torch.equal(t2.cpu(), VM.table_rule(p2.cpu(), shapes['pitch']))
    assert (t2[:, 2] <= t2[:, 0]).all() and (t2[:, 3] <= t2[:, 5]).all()
    # hypothesis 0 far from the object, the others in it: one = best = 0, mean > 0
    verts, rt = fix['verts'][:1].clone(), fix['rt'][:1].clone()
    verts[0, 0] += 0.5
    table, per = fix['m'].volume_multi(verts, rt, fix['ids'][:1], H_PITCH)
    assert per[0, 0].tolist() == [0.0, 0.0] and (per[0, 1:, 0] > 0).all()
    assert table[0, :4].tolist() == [0.0] * 4 and float(table[0, 5]) == float(per[0, :, 0].sum()) / 5.0 > 0
    assert torch.equal(table.cpu(), VM.table_rule(per.cpu(), H_PITCH))


def test_edge_cases(fix):
    from vpho_amd import ops
    m, verts, rt = fix['m'], fix['verts'], fix['rt']
    # a device id the host cannot check: that image all NaN, the others untouched
    ids = torch.tensor([0, 9, 0], dtype=torch.int32, device='cuda')
    table, per, flags = m.volume_multi(verts, rt, ids, H_PITCH, flags=True)
    assert table[1].isnan().all() and per[1].isnan().all() and not flags[1].any()
    for i in (0, 2):
        assert _bytes_equal(table[i], fix['table'][i]) and _bytes_equal(per[i], fix['per'][i]) and _bytes_equal(flags[i], fix['flags'][i])
    for bad in ([0, 2, 0], [0, -1, 0], [0, 1]):
        with pytest.raises(ops.VphoError, match='object ids'):
            m.volume_multi(verts, rt, bad, H_PITCH)
    # a NaN vertex in hypothesis 2: that hypothesis NaN, flags 0, best / mean NaN, one finite
    v = verts.clone()
    first_face_vertex = int(m.hand_faces[0, 0])
    v[1, 2, first_face_vertex, 1] = float('nan')
    table, per, flags = m.volume_multi(v, rt, fix['ids'], H_PITCH, flags=True)
    assert per[1, 2].isnan().all() and not flags[1, 2].any()
    assert table[1, 2:].isnan().all() and _bytes_equal(table[1, :2], fix['table'][1, :2]) and torch.isfinite(table[1, :2]).all()
    keep = [s for s in range(5) if s != 2]
    assert _bytes_equal(per[1, keep], fix['per'][1, keep]) and _bytes_equal(flags[1, keep], fix['flags'][1, keep])
    assert _bytes_equal(table[[0, 2]], fix['table'][[0, 2]])
    # no overlap at all: zeros
    far = verts + 0.5
    table, per, flags = m.volume_multi(far, rt, fix['ids'], H_PITCH, flags=True)
    assert not table.any() and not per.any() and not flags.any()
    # n = 0 is a no-op; S = 1: the table's three pairs are equal
    t0, p0 = m.volume_multi(verts[:0], rt[:0], [], H_PITCH)
    assert t0.shape == (0, 6) and p0.shape == (0, 5, 2)
    assert len(m.volume_multi(verts[:0], rt[:0], [], H_PITCH, flags=True)) == 3
    t1, p1 = m.volume_multi(verts[:, :1].contiguous(), rt[:, :1].contiguous(), fix['ids'], H_PITCH)
    assert _bytes_equal(p1, fix['per'][:, :1]) and torch.equal(t1[:, 0:2], t1[:, 2:4]) and torch.equal(t1[:, 0:2], t1[:, 4:6])
    assert torch.equal(t1[:, 0:2], p1[:, 0].flip(1)) and (t1[:, 1] > 0).all()
    # argument checks: the pitch, faces beyond V, no hand mesh, and the C entry point's own
    for pitch in (0.0, -0.005):
        with pytest.raises(ops.VphoError, match='pitch'):
            m.volume_multi(verts, rt, fix['ids'], pitch)
    with pytest.raises(ops.VphoError, match='index vertex'):
        m.volume_multi(verts[:, :, :50].contiguous(), rt, fix['ids'], H_PITCH)
    bare = ops.HandObjectPenetration({'box_a': dict(verts=G['obj0_verts'], faces=G['obj0_faces'].astype(np.int64))}, 'cuda', accel=False)
    with pytest.raises(ops.VphoError, match='no hand mesh'):
        bare.volume_multi(verts[:1], rt[:1], [0], H_PITCH)
    sol, cols = m.build_solids(H_PITCH), m.build_solid_columns(H_PITCH)
    per, table = torch.zeros((3, 5, 2), dtype=torch.float64, device='cuda'), torch.zeros((3, 6), dtype=torch.float64, device='cuda')
    dev_ids = m.obj_ids([m.names[i] for i in fix['ids']])
    call = lambda n, S, F_, pitch: ops._call('vpho_hand_obj_intersection_multi_f64', ops.C.byref(m.c), ops.C.byref(sol['c']), ops.C.byref(cols['c']),
                                             m.hand_faces, F_, verts, n, S, verts.shape[2], rt,
                                             dev_ids, pitch, per, table, None, None, 0)
    F_ = int(m.hand_faces.shape[0])
    with pytest.raises(ops.VphoError, match='hypotheses'):
        call(3, 0, F_, H_PITCH)
    with pytest.raises(ops.VphoError, match='without faces'):
        call(3, 5, 0, H_PITCH)
    with pytest.raises(ops.VphoError, match='pitch'):
        call(3, 5, F_, 0.0)
    with pytest.raises(ops.VphoError, match='at most 2147483647'):
        call(70000, 70000, F_, H_PITCH)
    call(0, 5, F_, H_PITCH)                                                     # n == 0: nothing is launched
    assert not per.any() and not table.any()
    call(3, 5, F_, H_PITCH)                                                     # and the raw call with a NULL workspace is the wrapper's
    assert _bytes_equal(per, fix['per']) and _bytes_equal(table, fix['table'])
    wb = ops.lib.vpho_hand_obj_intersection_multi_workspace_bytes
    assert wb(64, 100, 1552) == 0 and wb(1, 0, 4) == -1 and wb(1, 1, 0) == -1
    assert wb(70000, 70000, 4) == -1
    with pytest.raises(ops.VphoError, match='at most'):
        m.volume_multi(verts[:1, :1].expand(50000, 50000, -1, -1), rt[:1, :1].expand(50000, 50000, -1, -1), fix['ids'], H_PITCH)       # views: no memory


# ------------------------------------------------------------------------------------------------------------ end to end
def _eval_cfg():
    from vpho_amd.configs.args import cfg
    keys = tuple(EVAL_ARGS) + ('checkpoint', 'eval_best', 'eval_physics', 'eval_volume', 'physics_voxel_pitch')
    saved = {k: getattr(cfg, k) for k in keys}
    for k, v in EVAL_ARGS.items():
        setattr(cfg, k, v)
    cfg.checkpoint, cfg.eval_best, cfg.eval_physics, cfg.eval_volume, cfg.physics_voxel_pitch = None, True, False, True, 0.005
    return cfg, saved


def _table_of(text):
    line = [l for l in text.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, text[-2000:]
    return json.loads(line[0][len('EVAL_JSON '):])['table']


def _by_image(rows):
    idx = rows[:, 0]
    assert len(set(idx.tolist())) == rows.shape[0]
    return rows[idx.argsort()]


def test_trainer_eval_with_both_flags_end_to_end(monkeypatch, capsys):
    from vpho_amd import evaluate as E
    from vpho_amd import ops
    from vpho_amd.ops_names import MULTI_TABLES, VOLUME_TABLE
    from vpho_amd.trainer import Trainer
    cfg, saved = _eval_cfg()
    calls = []
    orig_block = E.volume_multi_block

    def spy_block(out, data, meshes):
        blk = orig_block(out, data, meshes)
        calls.append((out['diff_final_hand_vert'].clone(), out['diff_final_obj_6d'].clone(), data['root_joint'].clone(), data['is_right'].clone(),
                      list(data['obj_name']), blk.clone(), meshes))
        return blk
    try:
        t = Trainer(cfg)                                   # seeds torch with cfg.random_seed, as `main.py --random_seed` does: the child's run
        rng_state = torch.get_rng_state()                  # behind the model's construction: where the prior draws of an evaluation start
        monkeypatch.setattr(E, 'volume_multi_block', spy_block)
        wide = t.eval(eval_best=True, eval_volume=True)    # volume_multi=None: follows the two configuration flags
        text = capsys.readouterr().out
        monkeypatch.setattr(E, 'volume_multi_block', orig_block)

        def boom(*a, **k):
            raise AssertionError('HandObjectPenetration.volume_multi called with volume_multi=False')
        monkeypatch.setattr(ops.HandObjectPenetration, 'volume_multi', boom)
        torch.set_rng_state(rng_state)                     # the same prior draws as the run above
        narrow = t.eval(eval_best=True, eval_volume=True, volume_multi=False)
        monkeypatch.undo()
        capsys.readouterr()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    n = EVAL_ARGS['eval_batch_size'] * EVAL_ARGS['num_batches']
    assert wide.shape == (n, 98) and narrow.shape == (n, 92)
    wide, narrow = _by_image(wide), _by_image(narrow)
    i32 = lambda x: x.contiguous().view(torch.int32)
    assert torch.equal(i32(wide[:, :88]), i32(narrow[:, :88])) and torch.equal(i32(wide[:, -4:]), i32(narrow[:, -4:]))
    # the six new columns are a direct volume_multi call on the same outputs, whose per_hyp is the per-pair kernel's
    assert len(calls) == EVAL_ARGS['num_batches']
    blocks = []
    for hv, o6, root, right, names, blk, m in calls:
        bs, S = hv.shape[:2]
        assert S == EVAL_ARGS['sample_num']
        rootf = root.float().contiguous()
        verts = E.hypotheses_to_camera(hv.float(), rootf, right).contiguous()
        pd_rt = ops.obj_9d_to_rt(o6.reshape(bs * S, 9).double().contiguous(), rootf.repeat_interleave(S, 0).contiguous()).view(bs, S, 3, 4)
        ids = m.obj_ids(names)
        table, per = m.volume_multi(verts, pd_rt, ids, 0.005)
        assert torch.equal(table.float(), blk) and torch.isfinite(blk).all()
        assert _bytes_equal(per, _flat_volume(m, verts, pd_rt, ids, 0.005)[0])
        assert torch.equal(table.cpu(), VM.table_rule(per.cpu(), 0.005))
        blocks.append(blk)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    np.testing.assert_array_equal(order(torch.cat(blocks).cpu().numpy()), order(wide[:, 88:94].cpu().numpy()))
    table = _table_of(text)
    assert list(table['volume']) == ['pred', 'gt'] + list(MULTI_TABLES) and all(tuple(v) == VOLUME_TABLE for v in table['volume'].values())
    assert table['volume'] == E.summarize(wide.cpu())['volume'] and 'physics' not in table
    for name in ('pred', 'gt') + MULTI_TABLES:
        assert f'volume {name} (pitch 5 mm):' in text
    allb = torch.cat(blocks).double()
    for s, src in enumerate(MULTI_TABLES):
        assert table['volume'][src]['IV_cm3'] == pytest.approx(float(allb[:, 2 * s].mean() * 1e6), rel=1e-12, abs=0)
        assert table['volume'][src]['intersecting_pct'] == float((allb[:, 2 * s + 1] > 0).double().mean() * 100.0)
    _SHARED['table'] = table


def test_main_eval_best_eval_volume_prints_the_table_of_the_in_process_run(capsys):
    if 'table' not in _SHARED:                             # run on its own: the in-process run of the test above, without its checks
        from vpho_amd.trainer import Trainer
        cfg, saved = _eval_cfg()
        try:
            Trainer(cfg).eval(eval_best=True, eval_volume=True)
        finally:
            for k, v in saved.items():
                setattr(cfg, k, v)
        _SHARED['table'] = _table_of(capsys.readouterr().out)
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    args = [x for k, v in EVAL_ARGS.items() for x in ('--' + k, str(v))] + ['--eval_best', '--eval_volume']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--mode', 'eval', '--model', 'vpho_net'] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    table = _table_of(r.stdout)
    assert 'physics' not in table and all(f'volume {name} (pitch 5 mm):' in r.stdout for name in ('pred', 'gt', 'one_candidate', 'best_of_S', 'mean_of_S'))
    # the same seeds, the same images: the table of the in-process run, which is checked against direct calls there
    assert table['volume'] == _SHARED['table']['volume']

"""The symmetry-aware object errors on the device (--eval_symmetric, csrc/obj_symmetry.hip) against the float64 referee of
tests/_symmetry_fp64.py, which goes by another route (points moved by S_k, G and P separately; no D_k form).

Shapes: n = 3 images of three different classes, S in {1, 5}; tables of K = 1 (identity only), 4 (half-turns), 124 (no multiple of 64 or
256) and 628 (three rounds of 256: the production step 0.01); n_sampled in {1, 70, 2048}: one point, a tail that is no multiple of the
wave, the real size -- and once 2500, more than the kernel stages in LDS.  Poses: tests/golden/golden_symmetry.npz (numpy seed 2024 in
make_golden_symmetry.py): hypothesis 0 of every image is the ground truth moved by one of the object's own symmetries exactly, hypotheses
1 .. 4 go from near to far off.

Tolerance: each distance is at most 20 fp64 roundings of magnitudes below 2 m, about 1e-14 m; 1e-12 m leaves 100 x for contraction and
ordering differences and lies six orders below a millimetre.  The hit MSSD < 0.1 d is compared for equality: the referee's MSSD of every
pose used lies at least 1e-6 m from the threshold, which each test checks on the CPU first."""
import json
import os

import numpy as np
import pytest
import torch

import tests._symmetry_fp64 as SF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
MARGIN = 1e-6
IMAGES = (0, 1, 2)                       # rows of the fixture: classes 0, 1, 2


@pytest.fixture(scope='module')
def world():
    from vpho_amd import symmetry as SY
    from vpho_amd.assets import YCB_NAMES, synthetic_assets
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_symmetry.npz'))
    names = YCB_NAMES[:3]
    y = synthetic_assets(0)['ycb']
    # 4096 surface points per object: the 2048 sampled ones, then the object's 2048 full vertices (for a table longer than the LDS stage)
    ycb = {n: dict(bbox3d=np.asarray(y[n]['bbox3d'], np.float64),
                   verts_sampled=np.concatenate([np.asarray(y[n]['verts_sampled'], np.float64), np.asarray(y[n]['verts'], np.float64)]),
                   diameter=float(y[n]['diameter'])) for n in names}
    infos = json.loads(str(z['json']))
    half = {k: {'symmetries_discrete': v['symmetries_discrete']} for k, v in SY.synthetic_model_info(names).items()}
    tables = {1: (np.tile(np.eye(3), (3, 1, 1, 1)), np.zeros((3, 1, 3))), 4: SY.symmetry_table(half, names, 0.01),
              124: SY.symmetry_table(infos, names, 0.05), 628: (z['R'], z['t'])}
    assert [tables[k][0].shape[1] for k in (1, 4, 124, 628)] == [1, 4, 124, 628]
    idx = list(IMAGES)
    assert list(z['obj_idx'][idx]) == [0, 1, 2]
    return dict(names=names, ycb=ycb, tables=tables, pd=np.ascontiguousarray(z['pd_rt'][idx]), gt=np.ascontiguousarray(z['gt_rt'][idx]),
                ids=[0, 1, 2], ref={}, meters={})


def _ycb(world, P):
    return {n: dict(v, verts_sampled=v['verts_sampled'][:P]) for n, v in world['ycb'].items()}


def _meter(world, K, P):
    from vpho_amd import ops
    if (K, P) not in world['meters']:
        world['meters'][K, P] = ops.ObjectSymmetry(_ycb(world, P), world['tables'][K], 'cuda:0')
    return world['meters'][K, P]


def _referee(world, K, P, pd=None, gt=None, ids=None):
    """(n, S, 3) of the fixture's poses, computed once per (table, vertex count) and left unchanged; other poses are computed afresh"""
    R, t = world['tables'][K]
    y = _ycb(world, P)
    tabs = (R, t, [y[n]['bbox3d'] for n in world['names']], [y[n]['verts_sampled'] for n in world['names']], [y[n]['diameter'] for n in world['names']])
    if pd is not None:
        return SF.batch(pd, gt, ids, *tabs)
    if (K, P) not in world['ref']:
        world['ref'][K, P] = SF.batch(world['pd'], world['gt'], world['ids'], *tabs)
        world['ref'][K, P].setflags(write=False)
    return world['ref'][K, P]


def _margin_ok(world, ref, ids):
    thr = np.array([0.1 * world['ycb'][world['names'][i]]['diameter'] for i in ids])[:, None]
    return bool((np.abs(ref[..., 1] - thr) >= MARGIN).all())


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to('cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


@pytest.mark.parametrize('P', [1, 70, 2048])
@pytest.mark.parametrize('K', [1, 4, 124, 628])
def test_against_the_referee_pruned_and_unpruned(world, K, P):
    ref = _referee(world, K, P)
    assert _margin_ok(world, ref, world['ids'])
    m = _meter(world, K, P)
    pd, gt = _dev(world['pd']), _dev(world['gt'])
    for S in (1, 5):
        per, best, mean = m.multi(pd[:, :S].contiguous(), gt, world['ids'])
        full, bfull, mfull = m.multi(pd[:, :S].contiguous(), gt, world['ids'], prune=False)
        torch.cuda.synchronize()
        assert per.shape == (3, S, 3) and best.shape == mean.shape == (3, 3)
        got = per.cpu().numpy()
        d = np.abs(got[..., :2] - ref[:, :S, :2])
        print(f'K={K} P={P} S={S}: max |SMCE - ref| {d[..., 0].max():.3e}  max |MSSD - ref| {d[..., 1].max():.3e}')
        assert d.max() <= TOL, (K, P, S, d.max())
        assert np.array_equal(got[..., 2], ref[:, :S, 2])
        # pruning changes no bit, of the per-hypothesis values or of the tables
        for a, b in ((per, full), (best, bfull), (mean, mfull)):
            assert torch.equal(_bits(a), _bits(b))
        # the reduction: the stated rule applied to the device's own per-hypothesis values, bit for bit, and the referee's reduction
        one, rb, rm = SF.table_rule(got)
        assert np.array_equal(best.cpu().numpy(), rb) and np.array_equal(mean.cpu().numpy(), rm)
        _, refb, refm = SF.table_rule(np.ascontiguousarray(ref[:, :S]))
        assert np.abs(best.cpu().numpy()[:, :2] - refb[:, :2]).max() <= TOL and np.abs(mean.cpu().numpy()[:, :2] - refm[:, :2]).max() <= TOL
        assert np.array_equal(best.cpu().numpy()[:, 2], refb[:, 2]) and np.abs(mean.cpu().numpy()[:, 2] - refm[:, 2]).max() <= 1e-15
        # per[:, 0] is __call__ on hypothesis 0, bit for bit
        single = m(pd[:, 0].contiguous(), gt, world['ids'])
        assert single.shape == (3, 3) and torch.equal(_bits(single), _bits(per[:, 0]))
    if K == 628:
        # hypothesis 0 is an exact symmetric copy of the ground truth for every class (for class 0 and 1 through their own short lists)
        assert got[:, 0, :2].max() <= TOL and (got[:, 0, 2] == 1.0).all()


def test_more_vertices_than_the_lds_stage_holds(world):
    """n_sampled = 2500: vertices 2048 .. 2499 are read from memory behind the staged ones (K = 628: with the pruning bound in that loop
    too; K = 4: one round, no bound)"""
    pd, gt = _dev(world['pd']), _dev(world['gt'])
    for K in (4, 628):
        ref = _referee(world, K, 2500)
        assert _margin_ok(world, ref, world['ids']) and not np.array_equal(ref[..., 1], _referee(world, K, 2048)[..., 1])
        m = _meter(world, K, 2500)
        a, b = (m.per_hypothesis(pd, gt, world['ids'], prune=p) for p in (True, False))
        torch.cuda.synchronize()
        got = a.cpu().numpy()
        d = np.abs(got[..., :2] - ref[..., :2])
        print(f'K={K} P=2500: max |SMCE - ref| {d[..., 0].max():.3e}  max |MSSD - ref| {d[..., 1].max():.3e}')
        assert torch.equal(_bits(a), _bits(b)) and d.max() <= TOL and np.array_equal(got[..., 2], ref[..., 2])


def test_exact_symmetry_rows_where_pruning_must_fire_and_where_it_cannot(world):
    """P = G S_k for rows of the 628-table of the continuous object.  k = 40 lies in the first round of 256: its completed maximum (about
    0) is the bound of rounds two and three, every symmetry of which is abandoned after its first vertices; k = 627 lies in the last
    round, whose minimum no earlier bound can remove; with K = 1 there is no second round at all.  Same bits with and without pruning."""
    R, t = world['tables'][628]
    G = world['gt'][2]
    ks = (40, 300, 627)
    P = np.stack([G @ np.concatenate([np.concatenate([R[2, k], t[2, k][:, None]], -1), [[0, 0, 0, 1.0]]], 0) for k in ks])[None]   # (1, 3, 3, 4)
    # a far-off hypothesis after the near ones: each (image, hypothesis) pair has a bound of its own
    far = world['pd'][2, 4][None, None]
    P = np.concatenate([P, far], 1)
    ref = _referee(world, 628, 2048, P, G[None], [2])
    assert _margin_ok(world, ref, [2]) and ref[0, :3, :2].max() <= TOL and ref[0, 3, 1] > 0.05
    assert SF.mce(P[0, :3], G, world['ycb'][world['names'][2]]['bbox3d']).min() > 0.01          # centimetres by the plain corner error
    m = _meter(world, 628, 2048)
    a = m.per_hypothesis(_dev(P), _dev(G[None]), [2], prune=True)
    b = m.per_hypothesis(_dev(P), _dev(G[None]), [2], prune=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))
    got = a.cpu().numpy()
    assert got[0, :3, :2].max() <= TOL and (got[0, :3, 2] == 1.0).all()
    assert np.abs(got[..., :2] - ref[..., :2]).max() <= TOL and np.array_equal(got[..., 2], ref[..., 2])
    m1 = _meter(world, 1, 2048)
    a1, b1 = (m1.per_hypothesis(_dev(P), _dev(G[None]), [2], prune=p) for p in (True, False))
    torch.cuda.synchronize()
    assert torch.equal(_bits(a1), _bits(b1))
    ref1 = _referee(world, 1, 2048, P, G[None], [2])
    assert np.abs(a1.cpu().numpy()[..., :2] - ref1[..., :2]).max() <= TOL and ref1[0, :3, 1].min() > 0.001


def test_same_bits_across_runs_and_alone_or_in_the_batch(world):
    m = _meter(world, 628, 2048)
    pd, gt = _dev(world['pd']), _dev(world['gt'])
    first = m.per_hypothesis(pd, gt, world['ids'])
    again = m.per_hypothesis(pd, gt, world['ids'])
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(again))
    for b in range(3):
        alone = m.per_hypothesis(pd[b:b + 1].contiguous(), gt[b:b + 1].contiguous(), [world['ids'][b]])
        assert torch.equal(_bits(alone[0]), _bits(first[b])), b
    # a device tensor of ids (obj_ids) gives what host ints give
    dev_ids = m.obj_ids([world['names'][i] for i in world['ids']])
    assert torch.equal(_bits(m.per_hypothesis(pd, gt, dev_ids)), _bits(first))


def test_non_finite_poses(world):
    """a hypothesis or ground truth with a non-finite entry: NaN, NaN, 0; best passes a later NaN hypothesis over and keeps a NaN
    hypothesis 0; mean is NaN (the hit's mean counts the hypothesis as a miss)"""
    K, P = 124, 70
    m = _meter(world, K, P)
    pd, gt = world['pd'].copy(), world['gt'].copy()
    pd[0, 2, 1, 3] = np.nan
    pd[0, 3, 0, 0] = np.inf
    pd[1, 0, 2, 2] = -np.inf
    gt[2, 0, 1] = np.nan
    ref = _referee(world, K, P, pd, gt, world['ids'])
    clean = _referee(world, K, P)
    assert _margin_ok(world, clean, world['ids'])
    per, best, mean = m.multi(_dev(pd), _dev(gt), world['ids'])
    torch.cuda.synchronize()
    got = per.cpu().numpy()
    bad = np.zeros((3, 5), bool)
    bad[0, 2] = bad[0, 3] = bad[1, 0] = bad[2, :] = True
    assert np.isnan(got[bad][:, :2]).all() and (got[bad][:, 2] == 0).all() and np.isnan(ref[bad][:, :2]).all() and (ref[bad][:, 2] == 0).all()
    assert np.abs(got[~bad][:, :2] - ref[~bad][:, :2]).max() <= TOL and np.array_equal(got[~bad][:, 2], ref[~bad][:, 2])
    one, rb, rm = SF.table_rule(got)
    assert np.array_equal(best.cpu().numpy(), rb, equal_nan=True) and np.array_equal(mean.cpu().numpy(), rm, equal_nan=True)
    b, mn = best.cpu().numpy(), mean.cpu().numpy()
    assert np.isfinite(b[0]).all() and np.isnan(b[1, :2]).all() and np.isnan(b[2, :2]).all() and b[2, 2] == 0
    assert np.isnan(mn[:, :2]).all() and np.isfinite(mn[:, 2]).all() and mn[2, 2] == 0
    pruned_off = m.per_hypothesis(_dev(pd), _dev(gt), world['ids'], prune=False)
    assert np.array_equal(pruned_off.cpu().numpy(), got, equal_nan=True)


def test_refusals(world):
    from vpho_amd import ops
    y = _ycb(world, 70)
    with pytest.raises(ops.VphoError, match='4097'):
        ops.ObjectSymmetry(y, (np.tile(np.eye(3), (3, 4097, 1, 1)), np.zeros((3, 4097, 3))), 'cuda:0')
    m = ops.ObjectSymmetry(y, world['tables'][4], 'cuda:0')
    pd, gt = _dev(world['pd']), _dev(world['gt'])
    with pytest.raises(ops.VphoError):
        m.multi(pd.cpu(), gt.cpu(), world['ids'])
    for ids in ([0, 1, 3], [0, -1, 2], [0, 1]):
        with pytest.raises(ops.VphoError):
            m.per_hypothesis(pd, gt, ids)
    with pytest.raises(ops.VphoError):
        m.per_hypothesis(pd.cpu(), gt.cpu(), world['ids'])
    with pytest.raises(ops.VphoError):
        m.per_hypothesis(pd.float(), gt, world['ids'])
    with pytest.raises(ops.VphoError):
        m(pd, gt, world['ids'])                                                   # (n, S, 3, 4) into the single-pose call
    # an id outside the table in a DEVICE tensor cannot be refused without a host sync: the kernel answers NaN, NaN, 0 and reads nothing
    out = m.per_hypothesis(pd, gt, torch.tensor([0, 7, -2], dtype=torch.int32, device='cuda:0'))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isfinite(o[0]).all() and np.isnan(o[1:, :, :2]).all() and (o[1:, :, 2] == 0).all()


EVAL_ARGS = dict(sample_num=4, sampling_steps=5, topk_hand=8, topk_obj=3, sample_T0=0.2, eval_batch_size=2, num_batches=2, random_seed=7)


def test_trainer_eval_end_to_end(capsys, monkeypatch):
    """Trainer.eval with eval_best, eval_symmetric and symmetric_multi, by keyword and once through cfg (what --eval_best --eval_symmetric set): the new blocks hold what ObjectSymmetry gives on the poses of each batch, every older block keeps its
    bits, and the EVAL_JSON table is summarize(rows, layout)"""
    from vpho_amd import evaluate as E
    from vpho_amd.configs.args import cfg
    from vpho_amd.eval_layout import RowLayout
    from vpho_amd.trainer import Trainer
    keys = tuple(EVAL_ARGS) + ('checkpoint', 'eval_best', 'eval_physics', 'eval_volume', 'eval_hand_bench', 'eval_symmetric', 'max_sym_disc_step')
    saved = {k: getattr(cfg, k) for k in keys}
    for k, v in EVAL_ARGS.items():
        setattr(cfg, k, v)
    cfg.checkpoint, cfg.eval_best, cfg.eval_physics, cfg.eval_volume, cfg.eval_hand_bench, cfg.eval_symmetric = None, False, False, False, False, False
    cfg.max_sym_disc_step = 0.01
    seen = []
    inner = E.metric_rows

    def spy(out, data, *a, **kw):
        rows = inner(out, data, *a, **kw)
        seen.append((out, data, rows))
        return rows

    monkeypatch.setattr(E, 'metric_rows', spy)
    try:
        t = Trainer(cfg)
        rng_state = torch.get_rng_state()
        capsys.readouterr()
        rows_sym = t.eval(eval_best=True, eval_symmetric=True, symmetric_multi=True)
        text = capsys.readouterr().out
        torch.set_rng_state(rng_state)
        batches = list(seen)
        rows_old = t.eval(eval_best=True)
        assert len(seen) == 2 * len(batches)
        cfg.eval_best = cfg.eval_symmetric = True           # not named, the symmetric blocks follow cfg, as after --eval_best --eval_symmetric
        torch.set_rng_state(rng_state)
        rows_cfg = t.eval()
        cfg.eval_best = cfg.eval_symmetric = False
        capsys.readouterr()
        meter = E.symmetry_meter(t.assets, t.device)
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    torch.cuda.synchronize()
    n = EVAL_ARGS['eval_batch_size'] * EVAL_ARGS['num_batches']
    layout = RowLayout.resolve(eval_best=True, eval_symmetric=True, symmetric_multi=True)
    assert rows_sym.shape == (n, 100) == (n, layout.width) and rows_old.shape == (n, 88)
    order = lambda r: r[r[:, 0].argsort()]
    i32 = lambda x: x.contiguous().view(torch.int32)
    assert torch.equal(i32(order(rows_sym)[:, :88]), i32(order(rows_old)))               # every older block keeps its bits
    assert torch.equal(i32(order(rows_cfg)), i32(order(rows_sym)))                       # the flags of cfg give the rows of the keywords
    blk = rows_sym[:, layout.slice('symmetric').start:]
    assert blk.shape == (n, 12) and torch.isfinite(blk).all()
    assert meter.K == 4 * 314 and len(batches) == EVAL_ARGS['num_batches']
    for out, data, rows in batches:
        root = data['root_joint'].float().contiguous()
        ids = meter.obj_ids(data['obj_name'])
        gt = data['gt_obj_rt'].double().contiguous()
        single = meter(E._agg_obj_rt(out, data), gt, ids, prune=False)
        per, best, mean = meter.multi(E._hypothesis_obj_rt(out, root), gt, ids, prune=False)
        want = torch.cat([single, per[:, 0], best, mean], 1).float()
        assert torch.equal(i32(rows[:, 88:]), i32(want))
    line = [l for l in text.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, text[-2000:]
    table = json.loads(line[0][len('EVAL_JSON '):])['table']
    assert json.dumps(table) == json.dumps(E.summarize(rows_sym.cpu(), layout))
    assert list(table['symmetric']) == ['pred', 'one_candidate', 'best_of_S', 'mean_of_S'] and list(table)[-1] == 'symmetric'
    assert sum(l.startswith('symmetric ') for l in text.splitlines()) == 4

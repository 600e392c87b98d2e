"""csrc/contact_multi.hip on the device against tests/_contact_multi_fp64.py (NumPy fp64, brute force over all object vertices): the
contact kernel at n in {1, 3}, S in {1, 3, 7}, Nh = 1 080 over objects of 1, 31, 32, 33, 300 and 4 500 vertices mixed in one table, left
and right hands in one batch; exact ties; pruned against unpruned; prediction = annotation; the agreement kernel and its S-reduction;
degenerate pairs; Trainer.eval with --eval_best --eval_grasp end to end."""
import json

import numpy as np
import pytest
import torch

import tests._contact_multi_fp64 as CF

pytestmark = pytest.mark.gpu
G = CF.GATES
NH = 1080


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


@pytest.fixture(scope='module')
def world():
    from vpho_amd import grasp_eval as GE
    from vpho_amd import ops
    objs = CF.objects(0)
    return dict(objs=objs, pruned=ops.ContactMulti(GE.vertex_accel_tables(objs), 'cuda'),
                whole=ops.ContactMulti(GE.vertex_accel_tables(objs, cluster=None), 'cuda'))


def _launch(kernel, vf, nf, root, right, rt, ids, gates=G):
    out = kernel(_dev(vf, torch.float32), _dev(nf, torch.float32), _dev(root, torch.float64), _dev(right, torch.uint8), _dev(rt, torch.float64),
                 _dev(np.asarray(ids), torch.int32), gates['normal_thresh'], gates['vertical_thresh'], gates['decay'], per_vertex=True)
    torch.cuda.synchronize()
    return out


CASES = {'n1_S1_4500': (1, 1, [5]), 'n1_S3_33': (1, 3, [3]), 'n3_S3_1_32_300': (3, 3, [0, 2, 4]), 'n3_S7_31_33_4500': (3, 7, [1, 3, 5]),
         'n3_S1_4500_1_300': (3, 1, [5, 0, 4])}


@pytest.fixture(scope='module')
def scenes(world):
    """every case's inputs and its fp64 reference, computed once and left unchanged"""
    out = {}
    for seed, (name, (n, S, ids)) in enumerate(CASES.items()):
        inp = CF.scene(100 + seed, n, S, ids, world['objs'], NH)
        out[name] = (inp, ids, CF.contact_multi(*inp, world['objs'], ids, **G))
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_against_the_fp64_brute_force(world, scenes, name):
    inp, ids, ref = scenes[name]
    if inp[3].shape[0] > 1:
        assert 0 < inp[3].sum() < inp[3].shape[0]                                          # left and right hands in one batch
    w, nn, nd, vd = (t.cpu().numpy() for t in _launch(world['pruned'], *inp, ids))
    # judged: the two smallest reference d2 differ by more than 1e-12 relative and nd, vd are more than 1e-12 m from a gate
    judged = (ref['gap'] > 1e-12) & (CF.gate_distance(ref, G['normal_thresh'], G['vertical_thresh']) > 1e-12)
    assert (~judged).mean() <= 0.001                                                       # on the reference alone
    assert 0.2 < ref['contact'].mean() < 0.98                                              # both states are common
    assert np.array_equal(nn[judged], ref['nn'][judged]) and np.array_equal((w > 0)[judged], ref['contact'][judged])
    print(name, 'excluded', int((~judged).sum()), 'nd', np.abs(nd - ref['nd'])[judged].max(), 'vd', np.abs(vd - ref['vd'])[judged].max(),
          'weight', np.abs(w - ref['weight'])[judged].max())
    assert np.abs(nd - ref['nd'])[judged].max() <= 1e-12 and np.abs(vd - ref['vd'])[judged].max() <= 1e-12
    assert np.abs(w - ref['weight'])[judged].max() <= 1e-6 and (w >= 0).all() and (w <= 1).all()


def test_exact_ties_go_to_the_smaller_original_index(world):
    """dyadic coordinates, identity / axis-permutation rotations: every product and sum below is exact, so equidistant is equal bits"""
    from vpho_amd import grasp_eval as GE
    from vpho_amd import ops
    r = np.random.default_rng(3)
    grid = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing='ij'), -1).reshape(-1, 3) / 64.0           # 343 lattice points
    v = np.concatenate([grid, grid[r.permutation(len(grid))[:157]]])[r.permutation(500)]                     # 157 of them twice
    objs = [v, v[::-1].copy()]
    n, S = 3, 3
    perms = [np.eye(3), np.eye(3)[[1, 2, 0]], np.eye(3)[[2, 0, 1]] * np.array([[1.0], [-1.0], [1.0]])]
    root = np.array([[0.5, -0.25, 0.75], [0.125, 0.5, 0.5], [-0.25, 0.25, 1.0]])
    right = np.array([1, 0, 1], np.uint8)
    ids = [0, 1, 0]
    rt = np.zeros((n, S, 3, 4))
    vf, nf = np.zeros((n, S, NH, 3), np.float32), np.zeros((n, S, NH, 3), np.float32)
    for i in range(n):
        for s in range(S):
            R, t = perms[(i + s) % 3], root[i] + np.array([1, -2, 3]) / 32.0
            rt[i, s, :, :3], rt[i, s, :, 3] = R, t
            p = r.integers(-8, 9, (NH, 3)) / 128.0                           # half-lattice queries: equidistant from 2, 4 or 8 lattice points
            c = p @ R.T + t - root[i]
            c[:, 0] *= 1.0 if right[i] else -1.0
            vf[i, s] = c
            assert np.array_equal(vf[i, s].astype(np.float64), c)            # exact in fp32
            nf[i, s, :, (i + s) % 3] = 1.0
    wide = dict(normal_thresh=(-8.0, 8.0), vertical_thresh=8.0, decay=(-0.005, 0.005))         # everything is in contact: the index shows
    ref = CF.contact_multi(vf, nf, root, right, rt, objs, ids, **wide)
    assert ref['contact'].all() and (ref['gap'] == 0).mean() > 0.5                              # most queries have an exact tie
    for cluster in (GE.CLUSTER, None):
        k = ops.ContactMulti(GE.vertex_accel_tables(objs, cluster), 'cuda')
        w, nn, nd, vd = (t.cpu().numpy() for t in _launch(k, vf, nf, root, right, rt, ids, wide))
        assert np.array_equal(nn, ref['nearest'])                                               # everywhere, no band
        assert np.array_equal(nd, ref['nd']) and np.abs(vd - ref['vd']).max() <= 1e-12


@pytest.mark.parametrize('name', ['n3_S7_31_33_4500', 'n3_S3_1_32_300'])
def test_pruned_and_unpruned_walks_return_the_same_bits(world, scenes, name):
    inp, ids, _ = scenes[name]
    a, b = _launch(world['pruned'], *inp, ids), _launch(world['whole'], *inp, ids)
    assert world['whole'].sphere.shape[0] == len(CF.SIZES) and world['pruned'].sphere.shape[0] > 100
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


@pytest.fixture(scope='module')
def glove():
    """GraspMeter over the synthetic assets with object 0 replaced by a 'glove': the hand template's vertices moved by ~1 mm, so a hand at
    the template pose is in contact nearly everywhere"""
    from vpho_amd import grasp_eval as GE
    from vpho_amd.assets import synthetic_assets
    from vpho_amd.configs.args import cfg
    assets = synthetic_assets(0)
    assets = dict(assets, ycb={k: dict(v) for k, v in assets['ycb'].items()})
    first = next(iter(assets['ycb']))
    tmpl = np.asarray(assets['mano']['v_template'], np.float64).reshape(-1, 3)
    assets['ycb'][first]['verts'] = tmpl + np.random.default_rng(0).normal(size=tmpl.shape) * 0.001
    return GE.GraspMeter(cfg, assets, 'cuda'), tmpl


def _glove_batch(tmpl, n, S, seed):
    r = np.random.default_rng(seed)
    hand = (tmpl[None, None] + r.normal(size=(n, S, 778, 3)) * 0.0005).astype(np.float32)       # flipped, root-relative frame
    root = r.normal(size=(n, 3)) * 0.05 + np.array([0.0, 0.0, 0.6])
    right = (np.arange(n) % 2).astype(np.uint8)
    rt = np.zeros((n, S, 3, 4))
    for i in range(n):
        for s in range(S):
            # the object frame = the un-flipped hand frame moved by a few millimetres: R = diag(sg, 1, 1) maps the glove onto the hand
            rt[i, s, :, :3] = np.diag([1.0 if right[i] else -1.0, 1.0, 1.0])
            rt[i, s, :, 3] = root[i] + r.normal(size=3) * 0.0005
    return hand, root, right, rt


def test_a_prediction_equal_to_its_annotation_scores_exactly_one(glove):
    meter, tmpl = glove
    n, S = 3, 3
    hand, root, right, rt = _glove_batch(tmpl, n, S, 1)
    hand[:, 1:], rt[:, 1:] = hand[:, :1], rt[:, :1]                                              # every hypothesis IS hypothesis 0 ...
    ids = torch.zeros(n, dtype=torch.int32, device='cuda')
    args = (_dev(root, torch.float64), _dev(right, torch.uint8))
    counts, values, table = meter.score(_dev(hand, torch.float32), _dev(rt, torch.float64), _dev(hand[:, 0], torch.float32),   # ... and the annotation
                                        _dev(rt[:, 0], torch.float64), *args, ids)
    torch.cuda.synchronize()
    counts, values, table = counts.cpu().numpy(), values.cpu().numpy(), table.cpu().numpy()
    assert (counts[..., 2] > 0).all()                                                            # G > 0: the glove touches
    assert (counts[..., 0] == counts[..., 1]).all() and (counts[..., 1] == counts[..., 2]).all()
    assert (values[..., [0, 1, 2, 3, 5, 7]] == 1.0).all() and (values[..., 4] == 0.0).all()
    assert (table[:, [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19]] == 1.0).all() and (table[:, [4, 12, 20]] == 0.0).all()
    # a pair without any contact on either side: IoU, precision, recall, F1 undefined, MAE 0
    rt_far = rt.copy()
    rt_far[..., 3] += 1.0
    _, v, _ = meter.score(_dev(hand, torch.float32), _dev(rt_far, torch.float64), _dev(hand[:, 0], torch.float32), _dev(rt_far[:, 0], torch.float64), *args, ids)
    v = v.cpu().numpy()
    assert np.isnan(v[..., :4]).all() and (v[..., 4] == 0.0).all() and (v[..., 5] == 1.0).all() and (v[..., 6] == 0.0).all() and (v[..., 7] == 1.0).all()


def test_graspmeter_against_the_restatement_through_the_whole_chain(glove):
    """fill -> contact -> pooling -> agreement on moved hypotheses: the maps against the restatement fed the device's filled surface, the
    counts and values against the restatement fed the device's maps and pooled contacts"""
    meter, tmpl = glove
    n, S = 3, 3
    hand, root, right, rt = _glove_batch(tmpl, n, S, 2)
    hand[:, 1] += 0.004                                                                          # partly out of reach
    vf, nf = meter.fill(_dev(hand, torch.float32))
    ids = torch.zeros(n, dtype=torch.int32, device='cuda')
    w = meter.contact(vf, nf, _dev(root, torch.float64), _dev(right, torch.uint8), _dev(rt, torch.float64), ids)
    objs = [np.asarray(meter.tables['vert'], np.float64)[np.argsort(meter.tables['index'][:778])]]   # object 0 in its original order
    ref = CF.contact_multi(vf.cpu().numpy(), nf.cpu().numpy(), root, right, rt, objs, [0] * n, meter.normal_thresh, meter.vertical_thresh, meter.decay)
    judged = (ref['gap'] > 1e-12) & (CF.gate_distance(ref, meter.normal_thresh, meter.vertical_thresh) > 1e-12)
    assert (~judged).mean() <= 0.001 and vf.shape == (n, S, NH, 3)
    assert np.abs(w.cpu().numpy() - ref['weight'])[judged].max() <= 1e-6 and np.array_equal((w.cpu().numpy() > 0)[judged], ref['contact'][judged])
    w_gt = w[:, 0].contiguous()
    counts, values, table = meter.agreement(w, w_gt)
    (fc, gr), (fc_gt, gr_gt) = meter.pooled(w), meter.pooled(w_gt)
    c_ref, v_ref = CF.agreement(w.cpu().numpy(), w_gt.cpu().numpy(), fc.cpu().numpy(), gr.cpu().numpy(), fc_gt.cpu().numpy(), gr_gt.cpu().numpy())
    assert np.array_equal(counts.cpu().numpy(), c_ref) and (c_ref[..., 2] > 0).all() and (c_ref[:, 1] != c_ref[:, 0]).any()
    np.testing.assert_allclose(values.cpu().numpy(), v_ref, rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(table.cpu().numpy(), CF.table(v_ref), rtol=0, atol=1e-12, equal_nan=True)
    assert (values[:, 0, :4] == 1.0).all()


@pytest.mark.parametrize('n,S', [(1, 1), (3, 3), (3, 7)])
def test_agreement_kernel_and_its_reduction(n, S):
    from vpho_amd import ops
    r = np.random.default_rng(10 * n + S)
    w = (r.uniform(0, 1, (n, S, NH)) * (r.uniform(size=(n, S, NH)) < 0.4)).astype(np.float32)
    w_gt = (r.uniform(0, 1, (n, NH)) * (r.uniform(size=(n, NH)) < 0.4)).astype(np.float32)
    fc = (r.uniform(0, 1, (n, S, 32)) * (r.uniform(size=(n, S, 32)) < 0.5)).astype(np.float32)
    fc_gt = (r.uniform(0, 1, (n, 32)) * (r.uniform(size=(n, 32)) < 0.5)).astype(np.float32)
    gr, gr_gt = r.integers(0, 2, (n, S)).astype(np.uint8), r.integers(0, 2, (n,)).astype(np.uint8)
    if S > 1:
        w[0, 1] = 0.0                                   # P = 0: precision undefined, recall 0
        w[0, 2, 7] = np.nan                             # a NaN hypothesis among defined ones
    if n > 1:
        w[1, :, 3] = np.nan                             # an image whose every hypothesis is NaN
        w_gt[2] = 0.0                                   # G = 0: recall undefined
        w[2, 0] = 0.0                                   # ... and P = 0 too: IoU and F1 undefined, MAE 0
    counts, values, table = ops.contact_agreement(_dev(w, torch.float32), _dev(w_gt, torch.float32), _dev(fc, torch.float32), _dev(gr, torch.uint8),
                                                  _dev(fc_gt, torch.float32), _dev(gr_gt, torch.uint8))
    torch.cuda.synchronize()
    c_ref, v_ref = CF.agreement(w, w_gt, fc, gr, fc_gt, gr_gt)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), c_ref)
    np.testing.assert_allclose(values.cpu().numpy(), v_ref, rtol=0, atol=1e-12, equal_nan=True)
    t_ref = CF.table(v_ref)
    np.testing.assert_allclose(table.cpu().numpy(), t_ref, rtol=0, atol=1e-12, equal_nan=True)
    if n > 1:
        assert np.isnan(t_ref[1]).all() and (c_ref[1] == 0).all()                                 # all-NaN image: NaN row, zero counts
        assert np.isnan(v_ref[2, 0, :4]).all() and v_ref[2, 0, 4] == 0.0 and np.isnan(t_ref[2, [2, 10, 18]]).all()
    if S > 1:
        assert np.isnan(v_ref[0, 2]).all() and np.isfinite(t_ref[0, 8:]).all() and np.isnan(v_ref[0, 1, 1]) and v_ref[0, 1, 2] == 0.0
        assert t_ref[0, 12] == np.nanmin(v_ref[0, :, 4]) and t_ref[0, 8] == np.nanmax(v_ref[0, :, 0])


def test_degenerate_pairs_give_nan_rows_and_leave_their_neighbours_alone(world, scenes):
    from vpho_amd import ops
    (vf, nf, root, right, rt), ids, _ = scenes['n3_S3_1_32_300']
    clean = _launch(world['pruned'], vf, nf, root, right, rt, ids)
    n_obj = len(CF.SIZES)

    def check(out, dead):
        """dead (n, S) bool: NaN / -1 there, the clean launch's bits elsewhere"""
        w, nn, nd, vd = out
        d = torch.as_tensor(dead, device='cuda')
        assert w[d].isnan().all() and nd[d].isnan().all() and vd[d].isnan().all() and (nn[d] == -1).all()
        for x, y in zip(out, clean):
            assert torch.equal(_bits(x[~d]), _bits(y[~d]))
        # ... and the agreement kernel: NaN values and zero counts for those pairs, the S-reduction leaves them out
        w_gt = clean[0][:, 0].contiguous()
        fc = torch.rand(3, 3, 32, device='cuda')
        gr = torch.ones(3, 3, dtype=torch.uint8, device='cuda')
        counts, values, table = ops.contact_agreement(w, w_gt, fc, gr, fc[:, 0].contiguous(), gr[:, 0].contiguous())
        assert values[d].isnan().all() and (counts[d] == 0).all() and values[~d][:, 4:].isfinite().all()
        c_ref, v_ref = CF.agreement(w.cpu().numpy(), w_gt.cpu().numpy(), fc.cpu().numpy(), gr.cpu().numpy(), fc[:, 0].cpu().numpy(), gr[:, 0].cpu().numpy())
        assert np.array_equal(counts.cpu().numpy(), c_ref)
        np.testing.assert_allclose(table.cpu().numpy(), CF.table(v_ref), rtol=0, atol=1e-12, equal_nan=True)

    dead = np.zeros((3, 3), bool)
    bad_rt = rt.copy()
    bad_rt[1, 1, 2, 0] = np.nan                                                                   # one pose
    dead[1, 1] = True
    check(_launch(world['pruned'], vf, nf, root, right, bad_rt, ids), dead)
    bad_vf = vf.copy()
    bad_vf[0, 2, 1079, 1] = np.inf                                                                # one coordinate of one hand vertex
    dead[:] = False
    dead[0, 2] = True
    check(_launch(world['pruned'], bad_vf, nf, root, right, rt, ids), dead)
    bad_root = root.copy()
    bad_root[2, 0] = -np.inf                                                                      # a root joint: the whole image
    dead[:] = False
    dead[2] = True
    check(_launch(world['pruned'], vf, nf, bad_root, right, rt, ids), dead)
    for bad_id in (-1, n_obj):                                                                    # object ids outside the table
        dead[:] = False
        dead[1] = True
        check(_launch(world['pruned'], vf, nf, root, right, rt, [ids[0], bad_id, ids[2]]), dead)


def test_refusals(world, scenes):
    from vpho_amd import ops
    (vf, nf, root, right, rt), ids, _ = scenes['n1_S1_4500']
    with pytest.raises(ops.VphoError, match='normal_lo < decay_lo < decay_hi < normal_hi'):
        _launch(world['pruned'], vf, nf, root, right, rt, ids, dict(normal_thresh=(-0.004, 0.01), vertical_thresh=0.005, decay=(-0.005, 0.005)))
    with pytest.raises(ops.VphoError, match='ContactMulti'):
        _launch(world['pruned'], vf, nf[:, :, :5], root, right, rt, ids)


EVAL_ARGS = dict(sample_num=4, sampling_steps=5, topk_hand=8, topk_obj=3, sample_T0=0.2, eval_batch_size=2, num_batches=2, random_seed=7)


def test_trainer_eval_end_to_end(capsys, monkeypatch):
    """Trainer.eval with eval_best, eval_grasp and grasp_multi, by keyword and once through cfg (what --eval_best --eval_grasp set): the new blocks hold what a direct GraspMeter
    call gives on the outputs of each batch, every older block keeps its bits, and the EVAL_JSON table is summarize(rows, layout)"""
    from vpho_amd import evaluate as E
    from vpho_amd.configs.args import cfg
    from vpho_amd.eval_layout import RowLayout
    from vpho_amd.trainer import Trainer
    keys = tuple(EVAL_ARGS) + ('checkpoint', 'eval_best', 'eval_physics', 'eval_volume', 'eval_hand_bench', 'eval_symmetric', 'eval_grasp')
    saved = {k: getattr(cfg, k) for k in keys}
    for k, v in EVAL_ARGS.items():
        setattr(cfg, k, v)
    cfg.checkpoint, cfg.eval_best, cfg.eval_physics, cfg.eval_volume, cfg.eval_hand_bench, cfg.eval_symmetric, cfg.eval_grasp = (None,) + (False,) * 6
    seen = []
    inner = E.metric_rows

    def spy(out, data, *a, **kw):
        rows = inner(out, data, *a, **kw)
        seen.append((out, data, a[1], rows))
        return rows

    monkeypatch.setattr(E, 'metric_rows', spy)
    try:
        t = Trainer(cfg)
        rng_state = torch.get_rng_state()
        capsys.readouterr()
        rows_new = t.eval(eval_best=True, eval_grasp=True, grasp_multi=True)
        text = capsys.readouterr().out
        torch.set_rng_state(rng_state)
        batches = list(seen)
        rows_old = t.eval(eval_best=True)
        assert len(seen) == 2 * len(batches)
        cfg.eval_best = cfg.eval_grasp = True               # not named, the grasp blocks follow cfg, as after --eval_best --eval_grasp
        torch.set_rng_state(rng_state)
        rows_cfg = t.eval()
        cfg.eval_best = cfg.eval_grasp = False
        capsys.readouterr()
        meter = E.grasp_meter(t.assets, t.device)
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    torch.cuda.synchronize()
    n = EVAL_ARGS['eval_batch_size'] * EVAL_ARGS['num_batches']
    layout = RowLayout.resolve(eval_best=True, eval_grasp=True, grasp_multi=True)
    assert rows_new.shape == (n, 120) == (n, layout.width) and rows_old.shape == (n, 88)
    order = lambda r: r[r[:, 0].argsort()]
    i32 = lambda x: x.contiguous().view(torch.int32)
    assert torch.equal(i32(order(rows_new)[:, :88]), i32(order(rows_old)))               # every older block keeps its bits
    assert torch.equal(i32(order(rows_cfg)), i32(order(rows_new)))                       # the flags of cfg give the rows of the keywords
    assert len(batches) == EVAL_ARGS['num_batches'] and meter.Nh == NH
    for out, data, gt_vert, rows in batches:
        root, right = data['root_joint'], data['is_right']
        ids = meter.obj_ids(data['obj_name'])
        gt = (gt_vert.float() - root.float()[:, None]) * torch.stack([torch.where(right.bool(), 1.0, -1.0), torch.ones_like(root[:, 0]),
                                                                      torch.ones_like(root[:, 0])], -1)[:, None]
        assert data.get('gt_hand_vert_flip') is None
        w_gt = meter.contact(*meter.fill(gt[:, None]), root, right, data['gt_obj_rt'].double()[:, None].contiguous(), ids)[:, 0].contiguous()
        w_one = meter.contact(*meter.fill(out['agg_hand_vert'][:, None]), root, right, E._agg_obj_rt(out, data)[:, None].contiguous(), ids)
        w_all = meter.contact(*meter.fill(out['diff_final_hand_vert']), root, right, E._hypothesis_obj_rt(out, root.float().contiguous()), ids)
        want = torch.cat([meter.agreement(w_one, w_gt)[1][:, 0], meter.agreement(w_all, w_gt)[2]], 1).float()
        assert torch.equal(i32(rows[:, 88:]), i32(want)) and rows[:, 88 + 4].isfinite().all()   # MAE is always defined
    line = [l for l in text.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, text[-2000:]
    table = json.loads(line[0][len('EVAL_JSON '):])['table']
    assert json.dumps(table) == json.dumps(E.summarize(rows_new.cpu(), layout))
    assert list(table['grasp']) == ['pred', 'one_candidate', 'best_of_S', 'mean_of_S'] and list(table)[-1] == 'grasp'
    assert sum(l.startswith('grasp ') for l in text.splitlines()) == 4

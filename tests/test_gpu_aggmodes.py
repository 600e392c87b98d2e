"""The ablation aggregators on the device (--aggregation_mode_hand / --aggregation_mode_obj other than heatmap_cascade).

Selection: top-k indices and heat-map peaks identical to the reference's (tests/golden/golden_aggmodes.npz) on every image, mode and
side.  Values: fused hand pose, joints, vertices and object 6-D against the float64 restatement (tests/_agg_modes_fp64.py) on the
fixture's inputs, allowance per quantity = 2 x (the reference's own fp32 error against that float64 result, stored in the fixture) + 1e-6,
and the project's 1e-3 gate.  Then bit-level properties of the whole predict path: determinism, graph replay = plain launches, the
default untouched (same bits, same launches), a side left at the cascade unchanged by the other side's mode; limits; end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tests._agg_modes_fp64 as O
from tests.test_aggmodes_cpu import G, BS, S, K, fixture_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-3                     # the project's headline gate on joints, vertices and the 6-DoF pose

# what one default aggregation launches, entry by entry, at the commit before the modes existed (Engine.aggregate, plain launches)
CASCADE_CENSUS = (['vpho_hand_candidates_f32'] + ['vpho_mano_fk_f32', 'vpho_hand_heat_f32', 'vpho_hand_fuse_level_f32'] * 4
                  + ['vpho_mano_fk_f32', 'vpho_force_anchor_f32', 'vpho_obj_heat_score', 'vpho_topk_f32', 'vpho_topk_weights_f32', 'vpho_obj_fuse_f64',
                     'vpho_obj_heat_score', 'vpho_topk_f32', 'vpho_obj_cross_candidates', 'vpho_obj_physics_score', 'vpho_topk_f32',
                     'vpho_obj_heat_score', 'vpho_topk_f32', 'vpho_topk_weights_f32', 'vpho_obj_fuse_f64', 'vpho_obj_verts_f32',
                     'vpho_hand_phys_candidates_f32', 'vpho_mano_fk_f32', 'vpho_force_anchor_f32', 'vpho_hand_phys_score_f32', 'vpho_topk_f32',
                     'vpho_hand_phys_fuse_f32', 'vpho_mano_fk_f32'])
CASCADE_ONLY = {'vpho_hand_candidates_f32', 'vpho_force_anchor_f32', 'vpho_obj_physics_score', 'vpho_obj_cross_candidates', 'vpho_obj_verts_f32',
                'vpho_hand_phys_candidates_f32', 'vpho_hand_phys_score_f32', 'vpho_hand_phys_fuse_f32'}


def _engine(model_cpu, graphs):
    import copy
    from vpho_amd.model.engine import Engine
    old = os.environ.get('VPHO_GRAPHS')
    os.environ['VPHO_GRAPHS'] = '1' if graphs else '0'
    try:
        return Engine(copy.deepcopy(model_cpu).cuda().eval())
    finally:
        if old is None:
            del os.environ['VPHO_GRAPHS']
        else:
            os.environ['VPHO_GRAPHS'] = old


@pytest.fixture(scope='module')
def eng(model_cpu):
    return _engine(model_cpu, graphs=False)


@pytest.fixture(scope='module')
def eng_graphs(model_cpu):
    return _engine(model_cpu, graphs=True)


def _fixture_call(eng, mode_hand, mode_obj, weighted=False, k=K):
    """Engine.aggregate on the fixture's inputs: what HOI_Aggregator.__call__ hands the two aggregators"""
    I = fixture_inputs()
    c = lambda t: t.cuda()
    betas = c(I['betas'])
    f = dict(mano_ctx=eng.mano.shape(betas), mano_shape=betas, hand_heatmap=c(I['hm_hand']).contiguous(), obj_heatmap=c(I['hm_obj']).contiguous())
    data = dict(root_joint_flip=c(I['root_flip']), root_joint=c(I['root']), cam_intr_crop_flip=c(I['K']), bbox_hand=c(I['bbox_hand']),
                bbox_obj_rect=c(I['bbox_obj_rect']), is_right=c(I['is_right']), obj_name=I['obj_name'])
    final58 = torch.cat([c(I['pose']), betas[:, None].expand(BS, S, 10)], -1).reshape(BS * S, 58).contiguous()
    res, dbg = eng.aggregate(f, data, final58, c(I['obj_pose']).contiguous(), S, k, k, mode_hand=mode_hand, mode_obj=mode_obj, weighted=weighted)
    torch.cuda.synchronize()
    return res, dbg


def _maxerr(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


@pytest.mark.parametrize('mode,weighted', [('heatmap', False), ('heatmap', True), ('2D_pt_pose', False), ('2D_pt_joint', False),
                                           ('average_all', False), ('random', False)])
def test_hand_modes_on_the_reference_fixture(eng, assets, mode, weighted):
    res, dbg = _fixture_call(eng, mode, 'random', weighted)
    info = dbg['hand_mode']
    assert dbg['mode_hand'] == mode and dbg['mode_obj'] == 'random'
    if mode in ('heatmap', '2D_pt_pose', '2D_pt_joint'):
        got, want = info['topk'].cpu().numpy(), G[f'hand_{mode}_topk']
        if mode == '2D_pt_joint':                # kernel layout (bs,21,k); joint 0 is an exact S-way tie, see the fixture's maker
            got, want = got.transpose(0, 2, 1)[..., 1:], want[..., 1:]
        for b in range(BS):
            assert np.array_equal(got[b], want[b]), (mode, b, got[b], want[b])
    if mode.startswith('2D_pt'):
        assert np.array_equal(info['peak_index'].cpu().numpy(), G['hand_peak_index'])
        assert np.array_equal(info['peak'].cpu().numpy(), G['hand_peak'])
    I = fixture_inputs(torch.float64)
    r = O.hand_mode(assets['mano'], mode, I['pose'], I['betas'], I['root_flip'], I['K'], I['hm_hand'], I['bbox_hand'], K, is_weight=weighted)
    ref_err = G['hand_heatmap_weighted_err' if weighted else f'hand_{mode}_err']
    for (q, key), e in zip((('mano', 'hand_agg_mano'), ('joint', 'hand_agg_joint'), ('vert', 'hand_agg_vert')), ref_err):
        err, allow = _maxerr(res[key], r[q]), 2 * float(e) + 1e-6
        print(f'AGGMODES hand {mode}{" weighted" if weighted else ""} {q}: max |kernel - fp64| {err:.3e}  allowance {allow:.3e}  (reference fp32 {float(e):.3e})')
        assert err <= allow and err < GATE, (mode, q, err, allow)
    assert res['hand_agg_mano'].shape == (BS, 58) and res['hand_agg_vert'].shape == (BS, 778, 3) and res['hand_agg_joint'].shape == (BS, 21, 3)
    if mode == '2D_pt_joint':
        assert not res['hand_agg_vert'].any() and not res['hand_agg_mano'].any()
    if mode == 'random':                         # candidate 0 as it stands
        assert torch.equal(res['hand_agg_mano'][:, :48].cpu(), torch.from_numpy(G['in_pose'][:, 0]))
        assert torch.equal(res['hand_agg_mano'][:, 48:].cpu(), torch.from_numpy(G['in_betas']))


@pytest.mark.parametrize('mode', ['heatmap', '2D_pt_pose', 'average_all', 'random'])
def test_object_modes_on_the_reference_fixture(eng, assets, mode):
    from vpho_amd import ops
    res, dbg = _fixture_call(eng, 'random', mode)
    info = dbg['obj_mode']
    got = info['topk'].cpu().numpy()
    for b in range(BS):
        assert np.array_equal(got[b], G[f'obj_{mode}_topk'][b]), (mode, b)
    if mode == '2D_pt_pose':
        assert np.array_equal(info['peak_index'].cpu().numpy(), G['obj_peak_index'])
        assert np.array_equal(info['peak'].cpu().numpy(), G['obj_peak'])
    I = fixture_inputs()
    r = O.obj_mode(assets['ycb'], mode, I['obj_pose'], I['root'], I['obj_name'], I['is_right'], I['K'], I['hm_obj'], I['bbox_obj_rect'], K)
    e = float(G[f'obj_{mode}_err'])
    err, allow = _maxerr(res['obj_agg_6d'], r['fused']), 2 * e + 1e-6
    print(f'AGGMODES obj {mode} 6d: max |kernel - fp64| {err:.3e}  allowance {allow:.3e}  (reference fp32 {e:.3e})')
    assert err <= allow and err < GATE
    assert res['obj_agg_6d'].dtype == torch.float64 and res['obj_agg_6d'].shape == (BS, 9)
    pose = torch.from_numpy(G['in_obj_pose']).cuda()
    if mode == 'average_all':                    # the FIRST k candidates: vpho_obj_fuse_f64 on arange(k), unweighted
        idx = torch.arange(K, dtype=torch.int32, device='cuda').repeat(BS, 1)
        assert torch.equal(res['obj_agg_6d'], eng.agg.obj_fuse(pose, idx, None))
    if mode == 'random':                         # candidate 0 through the reference's fuse_topk: its translation bit for bit
        assert torch.equal(res['obj_agg_6d'][:, 6:], pose[:, 0, 6:])
        assert torch.equal(res['obj_agg_6d'], eng.agg.obj_fuse(pose, torch.zeros((BS, 1), dtype=torch.int32, device='cuda'), None))


def test_modes_without_a_cascade_side_launch_no_cascade_kernel(eng, monkeypatch):
    from vpho_amd import ops
    names = []
    orig = ops._call
    # (vpho_mano_shape_f32 is _fixture_call's own preparation of the shape context, not part of the aggregation)
    monkeypatch.setattr(ops, '_call', lambda name, *a: (names.append(name) if name != 'vpho_mano_shape_f32' else None, orig(name, *a))[1])
    _fixture_call(eng, '2D_pt_pose', '2D_pt_pose')
    assert not CASCADE_ONLY & set(names), names
    assert names.count('vpho_mano_fk_f32') == 2          # one pass over the candidates (joints only), one for the answer
    del names[:]
    _fixture_call(eng, 'random', 'average_all')
    assert names == ['vpho_mano_fk_f32', 'vpho_obj_fuse_f64'], names


# ------------------------------------------------------------------------------------------------ the whole predict path
CFG = dict(sample_num=6, sampling_steps=5, topk_hand=4, topk_obj=3, sample_T0=0.2)
OUT_KEYS = ('agg_obj_6d', 'agg_hand_mano', 'agg_hand_vert', 'agg_hand_joint')


class _Cfg:
    def __init__(self, **kw):
        from vpho_amd.configs.args import cfg
        self.cfg, self.kw = cfg, {**CFG, 'aggregation_mode_hand': 'heatmap_cascade', 'aggregation_mode_obj': 'heatmap_cascade', 'do_weighted_average': True, **kw}

    def __enter__(self):
        self.saved = {k: getattr(self.cfg, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.cfg, k, v)
        return self.cfg

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.cfg, k, v)


@pytest.fixture(scope='module')
def batch(assets):
    from vpho_amd.synth import synth_batch
    bs = 3
    data = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth_batch(bs, assets, seed=206).items()}
    g = torch.Generator().manual_seed(5)
    return data, torch.randn(bs * CFG['sample_num'], 96, generator=g), torch.randn(bs * CFG['sample_num'], 9, generator=g)


def _predict(e, batch, **kw):
    data, nh, no = batch
    out = e.predict(data, noise_hand=nh, noise_obj=no, **kw)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


ALL_PAIRS = [(h, o) for h in ('heatmap', '2D_pt_pose', '2D_pt_joint', 'average_all', 'random') for o in ('heatmap', '2D_pt_pose', 'average_all', 'random')]


def test_default_modes_are_todays_path_bit_for_bit_with_todays_launches(eng, eng_graphs, batch, monkeypatch):
    from vpho_amd import ops
    with _Cfg():
        plain = _predict(eng, batch)                                               # mode arguments omitted
        named = _predict(eng, batch, mode_hand='heatmap_cascade', mode_obj='heatmap_cascade')
        graphed = _predict(eng_graphs, batch, mode_hand='heatmap_cascade', mode_obj='heatmap_cascade')
        assert set(plain) == set(named) == set(graphed)
        for k in plain:
            assert torch.equal(plain[k], named[k]) and torch.equal(plain[k], graphed[k]), k
        assert 'hand_mode' not in eng.last_info['agg'] and 'obj_mode' not in eng.last_info['agg']
        # the launch census of the aggregation: exactly the cascade's, in its order
        names, live = [], []
        orig_call, orig_agg = ops._call, eng.aggregate
        monkeypatch.setattr(ops, '_call', lambda name, *a: (names.append(name) if live else None, orig_call(name, *a))[1])

        def agg(*a, **kw):
            live.append(1)
            try:
                return orig_agg(*a, **kw)
            finally:
                live.pop()
        monkeypatch.setattr(eng, 'aggregate', agg)
        _predict(eng, batch)
        assert names == CASCADE_CENSUS, names


def test_a_side_left_at_the_cascade_keeps_its_bits(eng, batch):
    with _Cfg():
        base = _predict(eng, batch)
        for mode in ('heatmap', '2D_pt_pose', '2D_pt_joint', 'average_all', 'random'):
            out = _predict(eng, batch, mode_hand=mode)
            assert torch.equal(out['agg_obj_6d'], base['agg_obj_6d']), mode
            assert set(out) == set(base) and all(out[k].shape == base[k].shape and out[k].dtype == base[k].dtype for k in base)
            assert not torch.equal(out['agg_hand_joint'], base['agg_hand_joint'])
        for mode in ('heatmap', '2D_pt_pose', 'average_all', 'random'):
            out = _predict(eng, batch, mode_obj=mode)
            for k in ('agg_hand_mano', 'agg_hand_vert', 'agg_hand_joint'):
                assert torch.equal(out[k], base[k]), (mode, k)
            assert not torch.equal(out['agg_obj_6d'], base['agg_obj_6d'])
        for k in base:                                        # everything before the aggregation is the same run
            if k not in OUT_KEYS:
                assert torch.equal(out[k], base[k]), k


@pytest.mark.parametrize('weighted', [True, False])
def test_every_mode_is_deterministic_and_graph_replay_equals_plain_launches(eng, eng_graphs, batch, weighted):
    with _Cfg(do_weighted_average=weighted):
        seen = {}
        for h, o in ALL_PAIRS if weighted else [('heatmap', 'heatmap')]:
            a = _predict(eng, batch, mode_hand=h, mode_obj=o)
            b = _predict(eng, batch, mode_hand=h, mode_obj=o)
            g1 = _predict(eng_graphs, batch, mode_hand=h, mode_obj=o)          # first call of the pair: capture
            g2 = _predict(eng_graphs, batch, mode_hand=h, mode_obj=o)          # replay
            for k in a:
                assert torch.equal(a[k], b[k]) and torch.equal(a[k], g1[k]) and torch.equal(a[k], g2[k]), (h, o, k)
                assert torch.isfinite(a[k]).all(), (h, o, k)
            seen[h, o] = a
        if weighted:
            # a mode change re-captures: different modes give different answers from the same engine
            assert not torch.equal(seen['heatmap', 'heatmap']['agg_hand_mano'], seen['average_all', 'heatmap']['agg_hand_mano'])
            assert torch.equal(seen['random', 'random']['agg_hand_mano'], seen['random', 'random']['diff_final_hand_mano'][:, 0])
        else:
            with _Cfg(do_weighted_average=True):
                w = _predict(eng_graphs, batch, mode_hand='heatmap', mode_obj='heatmap')
            assert not torch.equal(w['agg_hand_mano'], seen['heatmap', 'heatmap']['agg_hand_mano'])      # the flag is part of the graph key
            assert torch.equal(w['agg_obj_6d'], seen['heatmap', 'heatmap']['agg_obj_6d'])                # ... and touches the hand only


def test_documented_limits_raise(eng, eng_graphs, batch):
    from vpho_amd import ops
    with _Cfg(topk_hand=7):                                   # fine for the cascade (2 S candidates), not without the regression copies
        _predict(eng, batch)
        for e in (eng, eng_graphs):
            with pytest.raises(ops.VphoError, match='topk_hand'):
                _predict(e, batch, mode_hand='heatmap')
    with _Cfg(topk_obj=7):
        with pytest.raises(ops.VphoError, match='topk_obj'):
            _predict(eng, batch, mode_obj='average_all')
    with _Cfg():
        with pytest.raises(ops.VphoError, match='aggregation_mode_obj'):
            _predict(eng, batch, mode_obj='2D_pt_joint')
    with pytest.raises(ops.VphoError, match='square'):
        eng.agg.heatmap_peak(torch.zeros((2, 3, 8, 16), device='cuda'))
    f = dict(hand_heatmap=torch.zeros((1, 21, 8, 16)), obj_heatmap=torch.zeros((1, 27, 8, 8)))
    with pytest.raises(ops.VphoError, match='square'):
        eng._check_modes(f, 6, 4, 3, '2D_pt_joint', 'heatmap_cascade')
    eng._check_modes(f, 6, 4, 3, 'heatmap', '2D_pt_pose')


def test_peak_kernel_tie_and_nan_rules(eng):
    hm = torch.zeros((1, 4, 8, 8), device='cuda')
    hm[0, 0, 2, 5] = hm[0, 0, 6, 1] = 3.0                     # two equal maxima: the first in row-major order
    hm[0, 1, 7, 7] = 1.0
    hm[0, 2, 3, 3], hm[0, 2, 1, 2] = float('nan'), 9.0        # a NaN is a maximum (torch.argmax)
    peak, ind = eng.agg.heatmap_peak(hm)                      # channel 3: all equal -> index 0
    want_peak, want_ind = O.heatmap_peak(hm.cpu())
    assert ind.cpu().tolist() == [[2 * 8 + 5, 63, 3 * 8 + 3, 0]] and torch.equal(ind.cpu().long(), want_ind)
    assert torch.equal(peak.cpu(), want_peak)


def _main_eval(extra):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    args = ['--sample_num', '4', '--sampling_steps', '5', '--topk_hand', '4', '--topk_obj', '3', '--sample_T0', '0.2',
            '--eval_batch_size', '2', '--num_batches', '2', '--random_seed', '7'] + extra
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--mode', 'eval', '--model', 'vpho_net'] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][len('EVAL_JSON '):]), r.stdout


def test_object_random_scores_exactly_like_candidate_0(eng, batch, assets):
    """the aggregated object pose of `random` IS candidate 0: through the SAME metric kernel both give the same row, no tolerance"""
    from vpho_amd import evaluate as E
    with _Cfg():
        out = _predict(eng, batch, mode_hand='average_all', mode_obj='random')
    data = batch[0]
    agg = E.object_metric_block(out, data, assets).float()
    first = E.object_metric_block({'agg_obj_6d': out['diff_final_obj_6d'][:, 0].contiguous()}, data, assets).float()
    assert torch.equal(agg, first), (agg - first).abs().max()


def test_main_eval_average_all_random_end_to_end():
    """the one_candidate object row and the aggregated object row are both candidate 0.  They come from two different metric kernels
    (the per-pose one and the multi-hypothesis one, which searches nearest neighbours in the object frame): equal where both are exact
    fp64 criteria, within the bounds tests/test_gpu_multihyp.py sets between those kernels elsewhere (1e-6 m on the nearest-neighbour
    distances = 1e-3 in the table's mm, 3e-3 on the F-scores = 0.3 in its percent).  test_object_random_scores_exactly_like_candidate_0
    is the check without a tolerance."""
    js, text = _main_eval(['--aggregation_mode_hand', 'average_all', '--aggregation_mode_obj', 'random', '--eval_best'])
    assert js['aggregation_mode_hand'] == 'average_all' and js['aggregation_mode_obj'] == 'random'
    assert 'aggregation_mode_hand average_all  aggregation_mode_obj random' in text
    table = js['table']
    agg, one = table['object'], table['one_candidate']['object']
    assert list(agg) == list(one)
    for k in agg:
        print(f'AGGMODES e2e object {k}: aggregated {agg[k]!r} one_candidate {one[k]!r}')
        atol = 0.3 if k.startswith('F') else 1e-3 if k in ('ADDS', 'CD') else 0.0
        assert abs(agg[k] - one[k]) <= atol + 5e-6 * abs(one[k]), (k, agg[k], one[k])
    assert all(np.isfinite(v) for v in table['both'].values())


def test_main_eval_2d_pt_joint_reports_no_vertex_error():
    js, _ = _main_eval(['--aggregation_mode_hand', '2D_pt_joint', '--do_weighted_average'])
    both = js['table']['both']
    assert np.isnan(both['MVE_agg']) and np.isnan(both['PA_MVE_agg'])
    assert np.isfinite(both['MJE_agg']) and np.isfinite(both['PA_MJE_agg']) and js['aggregation_mode_obj'] == 'heatmap_cascade'

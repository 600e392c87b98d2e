"""The ablation aggregators (--aggregation_mode_hand / --aggregation_mode_obj) without a GPU: the float64 restatement
(tests/_agg_modes_fp64.py) selects what the reference selected (tests/golden/golden_aggmodes.npz, made by the reference's own
HandAggregator / ObjectAggregator), the command line takes the reference's spellings, the transposed heat-map peak."""
import os

import numpy as np
import pytest
import torch

import tests._agg_modes_fp64 as O

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'golden_aggmodes.npz'))
BS, S, K, HM = (int(v) for v in G['cfg'])


def fixture_inputs(dtype=torch.float32):
    t = lambda k: torch.from_numpy(G['in_' + k])
    d = lambda k: t(k).to(dtype)
    return dict(pose=d('pose'), betas=d('betas'), root_flip=d('root_flip'), root=t('root'), K=d('K'), bbox_hand=d('bbox_hand'),
                bbox_obj_rect=t('bbox_obj_rect'), is_right=t('is_right'), obj_name=[str(n) for n in G['obj_name']], obj_pose=t('obj_pose'),
                hm_hand=O.decode_heatmap(G['in_hm_hand_u8']).to(dtype), hm_obj=O.decode_heatmap(G['in_hm_obj_u8']))


def test_fixture_holds_its_own_condition():
    """>= 6 images, a left hand among them, and every k | k+1 gap at least 100 x the reference's largest fp32 score error"""
    assert BS >= 6 and S == 16 and K == 4 and HM == 64 and not G['in_is_right'].all()
    scored = ('hand_heatmap', 'hand_2D_pt_pose', 'hand_2D_pt_joint', 'obj_heatmap', 'obj_2D_pt_pose')
    worst = max(float(G[m + '_score_err'].max()) for m in scored)
    for m in scored:
        assert G[m + '_gap'].shape[0] == BS
        assert float(G[m + '_gap'].min()) >= 100 * worst, (m, float(G[m + '_gap'].min()), worst)
        assert float(G[m + '_gap_inside'].min()) >= 100 * float(G[m + '_score_err'].max()), m


@pytest.mark.parametrize('mode', ['heatmap', '2D_pt_pose', '2D_pt_joint'])
def test_fp64_restatement_selects_the_references_hand_candidates(assets, mode):
    I = fixture_inputs(torch.float64)
    r = O.hand_mode(assets['mano'], mode, I['pose'], I['betas'], I['root_flip'], I['K'], I['hm_hand'], I['bbox_hand'], K, is_weight=False)
    got, want = r['topk'].numpy(), G[f'hand_{mode}_topk']
    if mode == '2D_pt_joint':                       # joint 0 is an exact S-way tie (every candidate's joint 0 is the origin): no claim
        got, want = got[..., 1:], want[..., 1:]
    for b in range(BS):
        assert np.array_equal(got[b], want[b]), (mode, b)


@pytest.mark.parametrize('mode', ['heatmap', '2D_pt_pose', 'average_all', 'random'])
def test_fp64_restatement_selects_the_references_object_candidates(assets, mode):
    I = fixture_inputs()
    r = O.obj_mode(assets['ycb'], mode, I['obj_pose'], I['root'], I['obj_name'], I['is_right'], I['K'], I['hm_obj'], I['bbox_obj_rect'], K)
    assert np.array_equal(r['topk'].numpy(), G[f'obj_{mode}_topk'])
    if mode in ('heatmap', '2D_pt_pose'):           # ... and they are what the reference's own fp32 scores rank first
        assert np.array_equal(torch.from_numpy(G[f'obj_{mode}_score_ref']).topk(K, dim=1)[1].numpy(), G[f'obj_{mode}_topk'])
    assert np.abs(r['fused'].numpy() - G[f'obj_{mode}_6d']).max() <= 2 * float(G[f'obj_{mode}_err']) + 1e-6
    if mode == 'average_all':
        assert np.array_equal(r['topk'].numpy(), np.tile(np.arange(K), (BS, 1)))           # the FIRST k candidates, not all S
    if mode == 'random':
        assert r['topk'].shape == (BS, 1) and not r['topk'].any()


@pytest.mark.parametrize('mode', O.HAND_MODES)
def test_fp64_restatement_reproduces_the_references_hand_outputs(assets, mode):
    I = fixture_inputs(torch.float64)
    r = O.hand_mode(assets['mano'], mode, I['pose'], I['betas'], I['root_flip'], I['K'], I['hm_hand'], I['bbox_hand'], K, is_weight=False)
    err = G[f'hand_{mode}_err']
    for q, e in zip(('mano', 'joint', 'vert'), err):
        assert np.abs(r[q].numpy() - G[f'hand_{mode}_{q}']).max() <= 2 * float(e) + 1e-6, (mode, q)
    if mode == '2D_pt_joint':
        assert not G['hand_2D_pt_joint_vert'].any() and not G['hand_2D_pt_joint_mano'].any()
    if mode == 'random':
        assert np.array_equal(G['hand_random_mano'][:, :48], G['in_pose'][:, 0])


@pytest.mark.parametrize('side', ['hand', 'obj'])
def test_peak_is_read_through_the_transposed_grid(side):
    hm = O.decode_heatmap(G[f'in_hm_{side}_u8'])
    peak, ind = O.heatmap_peak(hm)
    assert np.array_equal(ind.numpy(), G[f'{side}_peak_index'])
    assert np.array_equal(peak.numpy(), G[f'{side}_peak'])
    # quirk (1): x comes from the ROW of the arg-max, y from its column
    rows, cols = G[f'{side}_peak_index'] // HM, G[f'{side}_peak_index'] % HM
    lin = (np.arange(HM, dtype=np.float32) / np.float32(HM - 1) * np.float32(2) - np.float32(1)).astype(np.float32)
    assert np.array_equal(G[f'{side}_peak'][..., 0], lin[rows]) and np.array_equal(G[f'{side}_peak'][..., 1], lin[cols])
    assert (rows != cols).any()                      # the transposition is visible in the fixture


def test_command_line_takes_the_references_spellings():
    from vpho_amd.configs import args as A
    p = A._parser()
    d = p.parse_args([])
    assert d.aggregation_mode_hand == 'heatmap_cascade' and d.aggregation_mode_obj == 'heatmap_cascade' and d.do_weighted_average is True
    assert A.cfg.aggregation_mode_hand == 'heatmap_cascade' and A.cfg.aggregation_mode_obj == 'heatmap_cascade' and A.cfg.do_weighted_average is True
    for m in ('heatmap_cascade', 'heatmap', '2D_pt_pose', '2D_pt_joint', 'average_all', 'random'):
        assert p.parse_args(['--aggregation_mode_hand', m]).aggregation_mode_hand == m
    for m in ('heatmap_cascade', 'heatmap', '2D_pt_pose', 'average_all', 'random'):
        assert p.parse_args(['--aggregation_mode_obj', m]).aggregation_mode_obj == m
    assert p.parse_args(['--do_weighted_average']).do_weighted_average is False              # store_false, as in the reference
    for bad in (['--aggregation_mode_obj', '2D_pt_joint'], ['--aggregation_mode_hand', 'physics'], ['--aggregation_mode_obj', 'heatmap_cascade_n_level']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)

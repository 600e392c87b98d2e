"""Generate ``golden_aggmodes.npz``: the reference's own ``HandAggregator`` / ``ObjectAggregator`` (lib/model/aggregation.py) called in
every mode other than the cascade, on seeded inputs.  Run in the build container only (needs the reference checkout); same stubs
as ``make_golden.py``.  Only data goes into the file.

Inputs: 6 images (at least one left hand), S = 16 candidates, k = 4, 64 x 64 heat maps with one clear peak per channel (a Gaussian at
the projection of a ground-truth pose's joints / key-points) plus uniform noise, synthetic assets.  Candidates are the ground-truth
pose plus noise, so the scores of the candidates differ.

The maker also evaluates every mode in float64 (tests/_agg_modes_fp64.py) and stores, per image and scored mode,
  (a) gap:  the gap between the k-th and the (k+1)-th float64 score (per joint for 2D_pt_joint),
  (b) err:  the largest difference between the reference's fp32 scores and the float64 scores.
CONDITION (asserted): every (a) is at least 100 x the largest (b) of all modes, and -- so that the ORDER of the selected indices is
pinned as well -- every gap between neighbours inside the top k is at least 100 x its own mode's (b).  The seed is searched upwards from
0 until the condition holds and is recorded in the file: no image is excused.

2D_pt_joint, joint 0: MANO's joints are relative to joint 0, so every candidate's joint 0 is exactly (0, 0, 0) and all S scores of that
joint are the same number, in fp32 and in float64 alike.  Its top-k is a k-way exact tie whose order torch.topk leaves open, and the fused
joint is (0, 0, 0) whichever candidates are listed: joint 0 has no gap and its index row is not part of the fixture's claims (the 20 other
joints of every image are).

Findings recorded here: the reference's hand `heatmap` mode with is_weight=True (the default of --do_weighted_average) does not run:
select_topk_hand_by_observed_heatmap_and_fuse_by_index hands average_quaternion 16 rotations with a (bs, 1, K) weight
(aggregation.py:228), whose shape assert (transform_fn.py:115) fails.  The fixture holds the reference's unweighted run; the weighted
variant (the weights broadcast over the 16 rotations, the evident intent) is pinned by the float64 restatement, its "reference fp32
error" by the restatement run in float32.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
REF = '/root/reference'
BS, S, K, HM = 6, 16, 4, 64


def make_inputs(assets, seed):
    """seeded inputs in float32 (poses of the object in float64, as the sampler returns them)"""
    from vpho_amd.synth import synth_batch
    from oracle import aggregation as OA
    from oracle.mano import get_hand_verts
    rng = np.random.default_rng(1000 + seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    b = synth_batch(BS, assets, seed=300 + seed)
    if bool(b['is_right'].all()):
        return None
    Kmat, root_flip, root = b['cam_intr_crop_flip'], b['root_joint_flip'], b['root_joint']
    # hand: a ground-truth pose per image, candidates around it
    gt_pose = f32(rng.normal(size=(BS, 48)) * 0.25)
    betas = f32(rng.normal(size=(BS, 10)) * 0.5)
    pose = gt_pose[:, None] + f32(rng.normal(size=(BS, S, 48)) * 0.3)
    _, gj = get_hand_verts(assets['mano'], gt_pose, betas)
    pt_h = OA._norm_to_bbox(OA.project((gj + root_flip[:, None])[:, None], Kmat), b['bbox_hand'])[:, 0]          # (bs,21,2)
    # object: a ground-truth 9-D pose per image (translation relative to the root), candidates around it, a box around its projection
    q = rng.normal(size=(BS, 3, 3))
    rot = np.linalg.qr(q)[0]
    gt6 = np.concatenate([rot[:, :2].reshape(BS, 6), rng.normal(size=(BS, 3)) * 0.02], -1)
    obj_pose = torch.from_numpy(gt6[:, None] + np.concatenate([rng.normal(size=(BS, S, 6)) * 0.15, rng.normal(size=(BS, S, 3)) * 0.015], -1))
    p = torch.from_numpy(gt6).float().clone()[:, None]
    p[..., 6:] = p[..., 6:] + root[:, None]
    kp = OA.flip_x(OA.object_points(assets['ycb'], p, b['obj_name'], 'kpt3d'), b['is_right'])                        # (bs,1,27,3)
    uv = OA.project(kp, Kmat)[:, 0]                                                                                # (bs,27,2) pixels
    c = uv.mean(1)
    half = (uv - c[:, None]).abs().amax(dim=(1, 2))[:, None] * 1.25
    bbox_obj_rect = torch.cat([c - half, c + half], -1)
    pt_o = OA._norm_to_bbox(uv[:, None], bbox_obj_rect)[:, 0]

    def maps(pt, sigma):
        """one Gaussian per channel at the normalised point (pixel centre convention of grid_sample, align_corners=False) + noise"""
        J = pt.shape[1]
        px = ((pt + 1) * HM - 1) / 2
        yy, xx = torch.meshgrid(torch.arange(HM, dtype=torch.float32), torch.arange(HM, dtype=torch.float32), indexing='ij')
        d2 = (xx[None, None] - px[..., 0, None, None]) ** 2 + (yy[None, None] - px[..., 1, None, None]) ** 2
        # 8-bit levels (the file stays small, value / 255 is exact in fp32): the Gaussian up to 240, the noise 0 .. 7
        u8 = torch.round(240 * torch.exp(-d2 / (2 * sigma ** 2))).to(torch.uint8) + torch.from_numpy(rng.integers(0, 8, size=(BS, J, HM, HM), dtype=np.uint8))
        return u8

    from tests._agg_modes_fp64 import decode_heatmap
    u8_hand, u8_obj = maps(pt_h, 8.0), maps(pt_o, 8.0)
    return dict(pose=pose, betas=betas, root_flip=root_flip, root=root, K=Kmat, bbox_hand=b['bbox_hand'], bbox_obj_rect=bbox_obj_rect,
                is_right=b['is_right'], obj_name=list(b['obj_name']), obj_pose=obj_pose, hm_hand_u8=u8_hand, hm_obj_u8=u8_obj,
                hm_hand=decode_heatmap(u8_hand), hm_obj=decode_heatmap(u8_obj))


def run_reference(ha, oa, I):
    """the reference's aggregators, every mode, fresh copies of the inputs per call (they write into their arguments)"""
    out = {}
    shape = I['betas'][:, None].expand(BS, S, 10).reshape(-1, 10)
    for mode in ('heatmap', '2D_pt_pose', '2D_pt_joint', 'average_all', 'random'):
        r = ha(mode=mode, pose=I['pose'].reshape(-1, 48).clone(), shape=shape.clone(), root_joint=I['root_flip'].clone(),
               cam_intrinsic=I['K'].clone(), heatmap=I['hm_hand'].clone(), bbox=I['bbox_hand'].clone(), k=K, is_weight=False)
        out[f'hand_{mode}'] = r
    try:
        ha(mode='heatmap', pose=I['pose'].reshape(-1, 48).clone(), shape=shape.clone(), root_joint=I['root_flip'].clone(),
           cam_intrinsic=I['K'].clone(), heatmap=I['hm_hand'].clone(), bbox=I['bbox_hand'].clone(), k=K, is_weight=True)
        out['hand_heatmap_weighted_runs'] = True
    except AssertionError:
        out['hand_heatmap_weighted_runs'] = False
    for mode in ('heatmap', '2D_pt_pose', 'average_all', 'random'):
        r = oa(mode=mode, pose6d=I['obj_pose'].clone(), root_joint=I['root'].clone(), cam_intrinsic=I['K'].clone(), obj_name=I['obj_name'],
               is_right=I['is_right'].clone(), heatmap=I['hm_obj'].clone(), bbox=I['bbox_obj_rect'].clone(), k=K)
        out[f'obj_{mode}'] = r
    return out


def ref_scores(ha, oa, I):
    """the reference's fp32 SCORES, which its aggregators do not return: the same calls with torch.Tensor.topk spied on"""
    rec = {}
    orig, orig_argmax = torch.Tensor.topk, torch.argmax

    def spy_argmax(*a, **kw):
        r = orig_argmax(*a, **kw)
        rec.setdefault('argmax', r.detach().clone())                        # the first call of an aggregator call: the heat-map peak
        return r

    def spy(self, *a, **kw):
        rec['score'] = self.detach().clone()
        return orig(self, *a, **kw)
    shape = I['betas'][:, None].expand(BS, S, 10).reshape(-1, 10)
    out = {}
    torch.Tensor.topk, torch.argmax = spy, spy_argmax
    try:
        for mode in ('heatmap', '2D_pt_pose', '2D_pt_joint'):
            rec.pop('argmax', None)
            ha(mode=mode, pose=I['pose'].reshape(-1, 48).clone(), shape=shape.clone(), root_joint=I['root_flip'].clone(),
               cam_intrinsic=I['K'].clone(), heatmap=I['hm_hand'].clone(), bbox=I['bbox_hand'].clone(), k=K, is_weight=False)
            out[f'hand_{mode}'] = rec['score']
            if mode == '2D_pt_pose':
                out['hand_peak_index'] = rec['argmax']
        for mode in ('heatmap', '2D_pt_pose'):
            rec.pop('argmax', None)
            oa(mode=mode, pose6d=I['obj_pose'].clone(), root_joint=I['root'].clone(), cam_intrinsic=I['K'].clone(), obj_name=I['obj_name'],
               is_right=I['is_right'].clone(), heatmap=I['hm_obj'].clone(), bbox=I['bbox_obj_rect'].clone(), k=K)
            out[f'obj_{mode}'] = rec['score']
            if mode == '2D_pt_pose':
                out['obj_peak_index'] = rec['argmax']
    finally:
        torch.Tensor.topk, torch.argmax = orig, orig_argmax
    return out


def run_fp64(assets, I, dtype):
    import tests._agg_modes_fp64 as O
    d = lambda t: t.to(dtype)
    out = {}
    for mode in O.HAND_MODES:
        for weighted in ((False, True) if mode == 'heatmap' else (False,)):
            out[f'hand_{mode}' + ('_weighted' if weighted else '')] = O.hand_mode(
                assets['mano'], mode, d(I['pose']), d(I['betas']), d(I['root_flip']), d(I['K']), d(I['hm_hand']), d(I['bbox_hand']), K, is_weight=weighted)
    for mode in O.OBJ_MODES:
        out[f'obj_{mode}'] = O.obj_mode(assets['ycb'], mode, I['obj_pose'], I['root'], I['obj_name'], I['is_right'], I['K'], I['hm_obj'],
                                        I['bbox_obj_rect'], K, dtype=dtype)
    return out


def gaps(score64):
    """score (bs,S) or (bs,S,F) -> sorted descending along dim 1: gap k|k+1 (bs[,F]) and the smallest neighbour gap inside the top k"""
    if score64.dim() == 3:
        score64 = score64[:, :, 1:]                # 2D_pt_joint, joint 0: see the module docstring
    s = torch.sort(score64, dim=1, descending=True)[0]
    d = s[:, :-1] - s[:, 1:]
    return d[:, K - 1], d[:, :K - 1].amin(dim=1)


def main():
    from vpho_amd.assets import synthetic_assets
    from make_golden import install_stubs, write_assets
    assets = synthetic_assets(0)
    tmp = tempfile.mkdtemp(prefix='vpho_golden_')
    write_assets(tmp, assets)
    os.chdir(tmp)
    sys.argv = ['main.py', '--mode', 'eval']
    sys.path.insert(0, REF)
    install_stubs(assets)
    from lib.model.aggregation import HandAggregator, ObjectAggregator
    from lib.model.head_mano import HeadMano
    from lib.model.head_object import HeadObject
    sys.argv = ['x']
    ha, oa = HandAggregator(HeadMano(in_dim=1024, is_output_contact=False).get_hand_verts), ObjectAggregator(HeadObject())

    scored = ('hand_heatmap', 'hand_2D_pt_pose', 'hand_2D_pt_joint', 'obj_heatmap', 'obj_2D_pt_pose')
    with torch.no_grad():
        for seed in range(400):
            I = make_inputs(assets, seed)
            if I is None:
                continue
            sc32 = ref_scores(ha, oa, I)
            f64 = run_fp64(assets, I, torch.float64)
            err = {m: (sc32[m].double() - f64[m]['score']).abs().reshape(BS, -1).amax(1) for m in scored}
            gk = {m: gaps(f64[m]['score']) for m in scored}
            worst = max(float(e.max()) for e in err.values())
            ok = all(float(gk[m][0].min()) >= 100 * worst and float(gk[m][1].min()) >= 100 * float(err[m].max()) for m in scored)
            print(f'seed {seed}: ' + '  '.join(f'{m} err {float(err[m].max()):.1e} gap {float(gk[m][0].min()):.1e}/{float(gk[m][1].min()):.1e}' for m in scored)
                  + f' -> {"ok" if ok else "next"}')
            if ok:
                break
        else:
            raise AssertionError('no seed below 400 satisfies the gap condition')
        assert all(float(gk[m][0].min()) >= 100 * worst for m in scored)                    # the condition, once more, on what is stored
        ref = run_reference(ha, oa, I)
        f32 = run_fp64(assets, I, torch.float32)
    assert not bool(I['is_right'].all()) and not ref['hand_heatmap_weighted_runs'], 'see the module docstring'
    G = dict(seed=np.array(seed), cfg=np.array([BS, S, K, HM]), obj_name=np.array(I['obj_name']))
    for k_, v in I.items():
        if torch.is_tensor(v) and k_ not in ('hm_hand', 'hm_obj'):          # the maps travel as their 8-bit levels
            G['in_' + k_] = v.numpy()
    n = lambda t: t.detach().numpy()
    for m in scored:
        G[f'{m}_score_ref'] = n(sc32[m])
        G[f'{m}_gap'], G[f'{m}_gap_inside'] = n(gk[m][0]), n(gk[m][1])
        G[f'{m}_score_err'] = n(err[m])
    for mode in ('heatmap', '2D_pt_pose', '2D_pt_joint', 'average_all', 'random'):
        r, o = ref[f'hand_{mode}'], f64[f'hand_{mode}']
        if r['topk'] is not None:
            G[f'hand_{mode}_topk'] = n(r['topk'])
            assert torch.equal(r['topk'][..., 1:], o['topk'][..., 1:]) if mode == '2D_pt_joint' else torch.equal(r['topk'], o['topk']), mode
        G[f'hand_{mode}_mano'], G[f'hand_{mode}_vert'], G[f'hand_{mode}_joint'] = n(r['agg_hand_mano']), n(r['agg_vert']), n(r['agg_joint'])
        # the reference's own fp32 error against float64, per quantity: what the GPU test's allowance is made of
        G[f'hand_{mode}_err'] = np.array([float((r['agg_hand_mano'].double() - o['mano']).abs().max()), float((r['agg_joint'].double() - o['joint']).abs().max()),
                                          float((r['agg_vert'].double() - o['vert']).abs().max())])
    o32, o64 = f32['hand_heatmap_weighted'], f64['hand_heatmap_weighted']
    assert torch.equal(o32['topk'], o64['topk'])
    G['hand_heatmap_weighted_err'] = np.array([float((o32[q].double() - o64[q]).abs().max()) for q in ('mano', 'joint', 'vert')])
    for mode in ('heatmap', '2D_pt_pose', 'average_all', 'random'):
        r, o = ref[f'obj_{mode}'], f64[f'obj_{mode}']
        G[f'obj_{mode}_6d'] = n(r['agg_6d'])
        G[f'obj_{mode}_topk'] = n(o['topk'])
        G[f'obj_{mode}_err'] = np.array(float((r['agg_6d'].double() - o['fused']).abs().max()))
    for m in ('hand_2D_pt_pose', 'obj_2D_pt_pose'):
        side = m.split('_')[0]
        # the arg-max is the reference's own (spied); the coordinate pair is its expression X[ind // W], Y[ind % W] evaluated in fp32
        assert torch.equal(sc32[f'{side}_peak_index'], f32[m]['peak_index'])
        G[f'{side}_peak'], G[f'{side}_peak_index'] = n(f32[m]['peak']), n(sc32[f'{side}_peak_index'])
    # the reference's top-k of the object modes is internal: its scores (spied) give it
    for mode in ('heatmap', '2D_pt_pose'):
        assert torch.equal(sc32[f'obj_{mode}'].topk(K, dim=1)[1], f64[f'obj_{mode}']['topk']), mode
    path = os.path.join(HERE, 'golden_aggmodes.npz')
    np.savez_compressed(path, **G)
    print('golden_aggmodes.npz', os.path.getsize(path) // 1024, 'KiB, seed', seed)


if __name__ == '__main__':
    main()

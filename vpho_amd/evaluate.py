"""Evaluation loop of the hot path: per-rank batches, per-image metric rows, ONE fixed-layout all-gather.

Counterpart of the reference's ``Trainer.evaluate`` / ``postprocess`` (lib/engine/train_diff_hand_obj.py:202-357,578-602)
for synthetic batches.  The reference gathers pickled nested dicts with ``gather_for_metrics(use_gather_object=True)``
(:333-335); here every rank fills a ``(n_images, ROW)`` fp32 tensor on its GPU and the ranks exchange it with a single
``torch.distributed.all_gather_into_tensor`` (RCCL over xGMI with backend 'nccl', gloo on CPU for tests).
The forward pass itself needs no collective: the image batch is the only sharded dimension.
"""
import torch
import torch.distributed as dist

from .eval_layout import BLOCKS, RowLayout
from .ops_names import (GRASP_METRIC_NAMES, HAND_BENCH_SOURCES, HAND_BENCH_TABLE, HAND_METRIC_NAMES, MULTI_TABLES, OBJ_METRIC_NAMES,
                        PHYSICS_SOURCES, SYM_METRIC_NAMES)

# the row layout -- which blocks there are, their order and widths -- is eval_layout.BLOCKS; these are its widths, by block name
_W = {b.name: b.width for b in BLOCKS}
ROW, MULTI = _W['base'], _W['multi']
PHYS, PHYS_MULTI = _W['physics'], _W['physics_multi']
VOL, VOL_MULTI = _W['volume'], _W['volume_multi']
HAND_BENCH, HAND_BENCH_MULTI = _W['hand_bench'], _W['hand_bench_multi']
SYM, SYM_MULTI = _W['symmetric'], _W['symmetric_multi']
GRASP, GRASP_MULTI = _W['grasp'], _W['grasp_multi']
ROW_BEST = ROW + MULTI
OBJ_COL = 12                 # first of the 16 object metrics of the aggregated pose within the base block


def mje_mm(pd, gt):
    """TesterHand MJE (test.py:657-668): mean over joints of the L2 distance, millimetres."""
    return (pd - gt).norm(dim=-1).mean(dim=-1) * 1000.0


def postprocess(out, root_joint, is_right):
    """train_diff_hand_obj.py:578-602: un-flip left hands along x and add the root joint (hand outputs only)."""
    sgn = torch.where(is_right.bool(), 1.0, -1.0).to(out['agg_hand_joint'].dtype)[:, None, None]
    res = {}
    for k in ('reg_hand_joint', 'agg_hand_joint', 'reg_hand_vert', 'agg_hand_vert'):
        v = out[k].clone()
        v[..., 0] = v[..., 0] * sgn[..., 0]
        res[k] = v + root_joint[:, None]
    first = out['diff_final_hand_joint'][:, 0].clone()
    first[..., 0] = first[..., 0] * sgn[..., 0]
    res['first_hand_joint'] = first + root_joint[:, None]
    return res


_OBJ_METRICS = {}


def _object_metrics(assets, device):
    """the ops.ObjectMetrics of an asset set on a device, built once"""
    key = (id(assets), str(device))
    if key not in _OBJ_METRICS:
        from . import ops
        _OBJ_METRICS[key] = ops.ObjectMetrics(assets['ycb'], device)
    return _OBJ_METRICS[key]


def _agg_obj_rt(out, data):
    """(bs, 3, 4) fp64: the aggregated object pose in the camera frame, obj_9D_to_mat + root joint"""
    from . import ops
    return ops.obj_9d_to_rt(out['agg_obj_6d'].double().contiguous(), data['root_joint'].float().contiguous())


def _hypothesis_obj_rt(out, root):
    """(bs, S, 3, 4) fp64: every object candidate in the camera frame, obj_9D_to_mat + its image's root joint (``root``: fp32, contiguous)"""
    from . import ops
    x = out['diff_final_obj_6d']
    bs, S = x.shape[:2]
    return ops.obj_9d_to_rt(x.reshape(bs * S, 9).double().contiguous(), root.repeat_interleave(S, 0).contiguous()).view(bs, S, 3, 4)


def object_metric_block(out, data, assets):
    """(bs,16) fp64: TesterObject on the aggregated object pose ('mean_candidate_pose', train_diff_hand_obj.py:249-258,
    498-501) -- obj_9D_to_mat + root joint, then the device metric kernels.  Needs data['gt_obj_rt'], data['cam_intr']."""
    M = _object_metrics(assets, out['agg_obj_6d'].device)
    return M(_agg_obj_rt(out, data), data['gt_obj_rt'].double().contiguous(), data['cam_intr'].double().contiguous(), M.obj_ids(data['obj_name']))


def multi_hypothesis_block(out, data, gt_joint, gt_vert, assets=None):
    """(bs, MULTI) fp32: every sampled hypothesis scored (test_diff_hand / test_diff_object with is_eval_best,
    train_diff_hand_obj.py:454-523) and reduced per image to hypothesis 0, best-of-S and mean-of-S.  Hand by the multi-hypothesis
    Procrustes kernel on the model-frame candidates (postprocess on load), object by ObjectMetrics.multi on obj_9D_to_mat + root of
    every candidate; object columns stay 0 without object tables or data['gt_obj_rt'], as in the 28-column block."""
    from . import ops
    if not gt_joint.is_cuda:
        raise RuntimeError('multi_hypothesis_block: the multi-hypothesis metrics run on the GPU only (no CPU path)')
    blk = torch.zeros((gt_joint.shape[0], MULTI), device=gt_joint.device, dtype=torch.float32)
    root = data['root_joint'].float().contiguous()
    c = lambda t: t.float().contiguous()
    mje, pa_mje = ops.hand_metrics_multi(c(out['diff_final_hand_joint']), c(gt_joint), root, data['is_right'])
    mve, pa_mve = ops.hand_metrics_multi(c(out['diff_final_hand_vert']), c(gt_vert), root, data['is_right'])
    hand = torch.stack([mje, pa_mje, mve, pa_mve], -1) * 1000.0                 # (bs, S, 4) mm
    blk[:, 0:4] = hand[:, 0]
    blk[:, 4:8] = hand.amin(1)
    blk[:, 8:12] = hand.mean(1)
    if assets is not None and 'gt_obj_rt' in data:
        M = _object_metrics(assets, gt_joint.device)
        per, best, mean = M.multi(_hypothesis_obj_rt(out, root), data['gt_obj_rt'].double().contiguous(), data['cam_intr'].double().contiguous(),
                                  M.obj_ids(data['obj_name']))
        blk[:, 12:28] = per[:, 0].float()
        blk[:, 28:44] = best.float()
        blk[:, 44:60] = mean.float()
    return blk


_PHYSICS = {}


def physics_meter(assets, device, multi=False, volume=False, volume_multi=False):
    """the HandObjectPenetration of an asset set on a device, built once (object meshes: physics_eval.object_meshes); its acceleration
    tables for the multi-hypothesis kernel only with ``multi`` (eval_best and eval_physics together), once as well; with ``volume``
    (eval_volume) the closed hand mesh (physics_eval.hand_faces) and the objects' solids at cfg.physics_voxel_pitch, once per pitch;
    with ``volume_multi`` (eval_best and eval_volume together) also the solids' lattice columns, once per pitch"""
    from .configs.args import cfg
    key = (id(assets), str(device))
    if key not in _PHYSICS:
        from . import ops
        from .physics_eval import object_meshes
        _PHYSICS[key] = ops.HandObjectPenetration(object_meshes(assets, cfg.asset_root), device, accel=False)
    meter = _PHYSICS[key]
    if multi:
        meter.build_accel()
    if volume or volume_multi:
        if meter.hand_faces is None:
            from .physics_eval import hand_faces
            meter.set_hand_faces(hand_faces(assets))
        (meter.build_solid_columns if volume_multi else meter.build_solids)(float(cfg.physics_voxel_pitch))
    return meter


def physics_block(pp, out, data, gt_vert, meshes):
    """(bs, PHYS) fp32: hand-object penetration and contact of the aggregated hand vertices (pp['agg_hand_vert'],
    postprocessed: camera frame) with the aggregated object pose (obj_9D_to_mat + root, as object_metric_block), then of the ground-truth
    vertices gt_vert with data['gt_obj_rt'] (NaN without it).  ``meshes``: an ops.HandObjectPenetration (physics_meter)."""
    from .configs.args import cfg
    if not gt_vert.is_cuda:
        raise RuntimeError('physics_block: the penetration metrics run on the GPU only (no CPU path)')
    blk = torch.full((gt_vert.shape[0], PHYS), float('nan'), device=gt_vert.device, dtype=torch.float32)
    ids = meshes.obj_ids(data['obj_name'])
    th = float(cfg.physics_contact_thresh)
    blk[:, 0:4] = meshes(pp['agg_hand_vert'].float().contiguous(), _agg_obj_rt(out, data), ids, th).float()
    if 'gt_obj_rt' in data:
        blk[:, 4:8] = meshes(gt_vert.float().contiguous(), data['gt_obj_rt'].double().contiguous(), ids, th).float()
    return blk


def volume_block(pp, out, data, gt_vert, meshes):
    """(bs, VOL) fp32: the hand-object intersection volume of the pairs of physics_block -- the aggregated hand
    vertices (pp['agg_hand_vert'], camera frame) with the aggregated object pose, then the ground-truth vertices with data['gt_obj_rt']
    (NaN without it) -- as IV (m^3) | solid-cell count each.  ``meshes``: physics_meter(..., volume=True)."""
    from .configs.args import cfg
    if not gt_vert.is_cuda:
        raise RuntimeError('volume_block: the intersection volume runs on the GPU only (no CPU path)')
    blk = torch.full((gt_vert.shape[0], VOL), float('nan'), device=gt_vert.device, dtype=torch.float32)
    ids = meshes.obj_ids(data['obj_name'])
    h = float(cfg.physics_voxel_pitch)
    blk[:, 0:2] = meshes.volume(pp['agg_hand_vert'].float().contiguous(), _agg_obj_rt(out, data), ids, h).flip(1).float()
    if 'gt_obj_rt' in data:
        blk[:, 2:4] = meshes.volume(gt_vert.float().contiguous(), data['gt_obj_rt'].double().contiguous(), ids, h).flip(1).float()
    return blk


def hypotheses_to_camera(x, root_joint, is_right):
    """(bs, S, N, 3) model-frame hand candidates -> camera frame: postprocess' un-flip of left hands along x + root joint, per hypothesis"""
    sgn = torch.where(is_right.bool(), 1.0, -1.0).to(x.dtype)[:, None, None]
    v = x.clone()
    v[..., 0] = v[..., 0] * sgn
    return v + root_joint[:, None, None]


def _hypothesis_pairs(out, data):
    """(verts (bs, S, V, 3) fp32, pd_rt (bs, S, 3, 4) fp64), both in the camera frame: hand candidate s (out['diff_final_hand_vert'][:, s],
    un-flipped + root as the multi-hypothesis hand metrics) and object candidate s (obj_9D_to_mat + root of out['diff_final_obj_6d'][:, s])"""
    root = data['root_joint'].float().contiguous()
    return hypotheses_to_camera(out['diff_final_hand_vert'].float(), root, data['is_right']).contiguous(), _hypothesis_obj_rt(out, root)


def physics_multi_block(out, data, meshes):
    """(bs, PHYS_MULTI) fp32: penetration and contact of every sampled hypothesis -- the pairs of _hypothesis_pairs --
    reduced per image to hypothesis 0 | best-of-S | mean-of-S by ONE HandObjectPenetration.multi launch pair.
    ``meshes``: physics_meter(..., multi=True)."""
    from .configs.args import cfg
    if not out['diff_final_hand_vert'].is_cuda:
        raise RuntimeError('physics_multi_block: the penetration metrics run on the GPU only (no CPU path)')
    verts, pd_rt = _hypothesis_pairs(out, data)
    table, _ = meshes.multi(verts, pd_rt, meshes.obj_ids(data['obj_name']), contact_thresh=float(cfg.physics_contact_thresh))
    return table.float()


def volume_multi_block(out, data, meshes):
    """(bs, VOL_MULTI) fp32: the intersection volume of every sampled hypothesis -- the pairs of _hypothesis_pairs --
    reduced per image to hypothesis 0 | best-of-S | mean-of-S by ONE HandObjectPenetration.volume_multi launch pair.
    ``meshes``: physics_meter(..., volume_multi=True)."""
    from .configs.args import cfg
    if not out['diff_final_hand_vert'].is_cuda:
        raise RuntimeError('volume_multi_block: the intersection volume runs on the GPU only (no CPU path)')
    verts, pd_rt = _hypothesis_pairs(out, data)
    table, _ = meshes.volume_multi(verts, pd_rt, meshes.obj_ids(data['obj_name']), float(cfg.physics_voxel_pitch))
    return table.float()


def _hand_bench_pair(pd_joint, pd_vert, data, gt_joint, gt_vert):
    """(bs, S, 8) fp64 in the order of ops_names.HAND_BENCH_NAMES from model-frame candidates (bs, S, 21 | V, 3): one joint call (AUC
    only) and one vertex call of ops.hand_bench_multi"""
    from . import ops
    root = data['root_joint'].float().contiguous()
    c = lambda t: t.float().contiguous()
    j = ops.hand_bench_multi(c(pd_joint), c(gt_joint), root, data['is_right'], with_fscore=False)
    v = ops.hand_bench_multi(c(pd_vert), c(gt_vert), root, data['is_right'])
    return torch.cat([j[..., :2], v], -1)


def hand_bench_block(out, data, gt_joint, gt_vert):
    """(bs, HAND_BENCH) fp32 in the order of ops_names.HAND_BENCH_COLUMNS: AUC_J, PA_AUC_J, AUC_V, PA_AUC_V, F@5, F@15, PA_F@5, PA_F@15
     of the aggregated hand, then of the regression hand, each as one hypothesis (S = 1) of the multi-hypothesis
    kernel: the model-frame outputs go in, the postprocess happens on load.  In hand mode 2D_pt_joint the six vertex values of the
    aggregated hand are NaN, as MVE is there."""
    if not gt_joint.is_cuda:
        raise RuntimeError('hand_bench_block: the hand benchmark metrics run on the GPU only (no CPU path)')
    agg = _hand_bench_pair(out['agg_hand_joint'][:, None], out['agg_hand_vert'][:, None], data, gt_joint, gt_vert)[:, 0]
    reg = _hand_bench_pair(out['reg_hand_joint'][:, None], out['reg_hand_vert'][:, None], data, gt_joint, gt_vert)[:, 0]
    blk = torch.cat([agg, reg], 1).float()
    from .configs.args import cfg
    if cfg.aggregation_mode_hand == '2D_pt_joint':
        blk[:, 2:8] = float('nan')
    return blk


def hand_bench_multi_block(out, data, gt_joint, gt_vert):
    """(bs, HAND_BENCH_MULTI) fp32 in the order of ops_names.HAND_BENCH_MULTI_COLUMNS: the eight values of every sampled hypothesis
    (out['diff_final_hand_joint'] / _vert, model frame) reduced per image to hypothesis 0 | best-of-S (each value's maximum on its
    own) | mean-of-S by ops.hand_bench_table"""
    from . import ops
    if not gt_joint.is_cuda:
        raise RuntimeError('hand_bench_multi_block: the hand benchmark metrics run on the GPU only (no CPU path)')
    per = _hand_bench_pair(out['diff_final_hand_joint'], out['diff_final_hand_vert'], data, gt_joint, gt_vert).contiguous()
    return torch.cat(ops.hand_bench_table(per), 1).float()


def _with_multi(what, block, multi, sources):
    """for the three tables below: the single-pose block ``block`` of ``what`` and, where the caller has it, the block ``multi`` of every
    sampled hypothesis, side by side, with the table's source names; a block of the wrong width is a ValueError"""
    for name, b in ((what, block), (what + '_multi', multi)):
        if b is not None and b.shape[1] != _W[name]:
            raise ValueError(f'{what}_table: a {name} block of {b.shape[1]} columns, expected {_W[name]}')
    return (block, sources) if multi is None else (torch.cat([block, multi], 1), sources + MULTI_TABLES)


def hand_bench_table(block, multi=None):
    """the table 'hand_bench' of Trainer.eval / EVAL_JSON from the (n, 16) columns hand_bench_block [and the (n, 24) hand_bench_multi_block] made:
    {'agg': {...}, 'reg': {...}[, 'one_candidate': ..., 'best_of_S': ..., 'mean_of_S': ...]}, each the ops_names.HAND_BENCH_TABLE keys as
    fp64 means over the images, in [0, 1] (NaN where a column holds one)"""
    block, names = _with_multi('hand_bench', block, multi, HAND_BENCH_SOURCES)
    mean = block.double().mean(0)
    return {src: {k: float(mean[8 * s + i]) for i, k in enumerate(HAND_BENCH_TABLE)} for s, src in enumerate(names)}


_OBJ_SYMMETRY = {}


def symmetry_meter(assets, device):
    """the ops.ObjectSymmetry of an asset set on a device, built once per cfg.max_sym_disc_step: the model-info of
    symmetry.load_symmetries(cfg.asset_root) (the synthetic one without the file), its padded table, the objects' corners, sampled vertices
    and diameters.  vpho_amd.symmetry is imported here and nowhere else on the evaluation path."""
    from .configs.args import cfg
    key = (id(assets), str(device), float(cfg.max_sym_disc_step))
    if key not in _OBJ_SYMMETRY:
        from . import ops, symmetry
        names = list(assets['ycb'].keys())
        table = symmetry.symmetry_table(symmetry.load_symmetries(cfg.asset_root, names), names, float(cfg.max_sym_disc_step))
        _OBJ_SYMMETRY[key] = ops.ObjectSymmetry(assets['ycb'], table, device)
    return _OBJ_SYMMETRY[key]


def symmetric_block(out, data, meter):
    """(bs, SYM) fp32 in the order of ops_names.SYM_COLUMNS: SMCE (m), MSSD (m) and MSSD < 0.1 * diameter of the
    aggregated object pose (obj_9D_to_mat + root, as object_metric_block) against data['gt_obj_rt']; NaN without it.
    ``meter``: an ops.ObjectSymmetry (symmetry_meter)."""
    dev = out['agg_obj_6d'].device
    if dev.type != 'cuda':
        raise RuntimeError('symmetric_block: the symmetric object errors run on the GPU only (no CPU path)')
    if 'gt_obj_rt' not in data:
        return torch.full((out['agg_obj_6d'].shape[0], SYM), float('nan'), device=dev, dtype=torch.float32)
    return meter(_agg_obj_rt(out, data), data['gt_obj_rt'].double().contiguous(), meter.obj_ids(data['obj_name'])).float()


def symmetric_multi_block(out, data, meter):
    """(bs, SYM_MULTI) fp32 in the order of ops_names.SYM_MULTI_COLUMNS: the three values of every sampled object hypothesis (the poses of
    multi_hypothesis_block) reduced per image to hypothesis 0 | best-of-S (min SMCE, min MSSD, max hit) | mean-of-S by ONE
    ObjectSymmetry.multi launch pair; NaN without data['gt_obj_rt']"""
    dev = out['diff_final_obj_6d'].device
    if dev.type != 'cuda':
        raise RuntimeError('symmetric_multi_block: the symmetric object errors run on the GPU only (no CPU path)')
    if 'gt_obj_rt' not in data:
        return torch.full((out['diff_final_obj_6d'].shape[0], SYM_MULTI), float('nan'), device=dev, dtype=torch.float32)
    per, best, mean = meter.multi(_hypothesis_obj_rt(out, data['root_joint'].float().contiguous()), data['gt_obj_rt'].double().contiguous(),
                                  meter.obj_ids(data['obj_name']))
    return torch.cat([per[:, 0], best, mean], 1).float()


def symmetric_table(block, multi=None):
    """the table 'symmetric' of Trainer.eval / EVAL_JSON from the (n, 3) columns symmetric_block [and the (n, 9) symmetric_multi_block] made:
    {'pred': {...}[, 'one_candidate': ..., 'best_of_S': ..., 'mean_of_S': ...]}, each the ops_names.SYM_METRIC_NAMES keys as fp64 means
    over the images (SMCE and MSSD in metres, MSSD01d in [0, 1]; NaN where a column holds one)"""
    block, names = _with_multi('symmetric', block, multi, ('pred',))
    mean = block.double().mean(0)
    return {src: {k: float(mean[3 * s + i]) for i, k in enumerate(SYM_METRIC_NAMES)} for s, src in enumerate(names)}


_GRASP = {}


def grasp_meter(assets, device):
    """the grasp_eval.GraspMeter of an asset set on a device, built once per set of contact gates: the hand surface fill, the anchor tables
    and the objects' vertex tables.  vpho_amd.grasp_eval is imported here and nowhere else on the evaluation path."""
    from .configs.args import cfg
    key = (id(assets), str(device), tuple(float(x) for x in cfg.contact_normal_distance_thresh), float(cfg.contact_vertical_distance_thresh))
    if key not in _GRASP:
        from .grasp_eval import GraspMeter
        _GRASP[key] = GraspMeter(cfg, assets, device)
    return _GRASP[key]


def _gt_hand_vert_flip(data, gt_vert):
    """(bs, 778, 3) fp32: the annotated hand in the flipped, root-relative frame of the fill: data['gt_hand_vert_flip'] where the batch
    carries it, else the camera-frame gt_vert minus the root joint with a left hand's x negated"""
    if data.get('gt_hand_vert_flip') is not None:
        return data['gt_hand_vert_flip'].to(gt_vert.device, torch.float32)
    v = gt_vert.float() - data['root_joint'].float()[:, None]
    v[..., 0] = v[..., 0] * torch.where(data['is_right'].bool(), 1.0, -1.0).to(v.dtype)[:, None]
    return v


def _grasp_against_gt(hand_vert_flip, pd_rt, data, gt_vert, meter):
    """GraspMeter.score of (bs, S, 778, 3) model-frame hands with (bs, S, 3, 4) camera-frame object poses against the annotated pair
    (the annotation's map comes from the same kernel, S = 1) -> counts, values (bs, S, 8), table (bs, 24)"""
    return meter.score(hand_vert_flip.float(), pd_rt, _gt_hand_vert_flip(data, gt_vert), data['gt_obj_rt'].double().contiguous(),
                       data['root_joint'], data['is_right'], meter.obj_ids(data['obj_name']))


def grasp_block(out, data, gt_vert, meter):
    """(bs, GRASP) fp32 in the order of ops_names.GRASP_COLUMNS: contact-map and grasp agreement of the aggregated
    hand (out['agg_hand_vert']: flipped and root-relative, the frame of the fill) with the aggregated object pose, the pair of
    physics_block, against the annotated pair; NaN without data['gt_obj_rt'].  ``meter``: a grasp_eval.GraspMeter (grasp_meter)."""
    if not gt_vert.is_cuda:
        raise RuntimeError('grasp_block: the contact agreement runs on the GPU only (no CPU path)')
    if 'gt_obj_rt' not in data:
        return torch.full((gt_vert.shape[0], GRASP), float('nan'), device=gt_vert.device, dtype=torch.float32)
    _, values, _ = _grasp_against_gt(out['agg_hand_vert'][:, None], _agg_obj_rt(out, data)[:, None].contiguous(), data, gt_vert, meter)
    return values[:, 0].float()


def grasp_multi_block(out, data, gt_vert, meter):
    """(bs, GRASP_MULTI) fp32 in the order of ops_names.GRASP_MULTI_COLUMNS: the eight values of every sampled hypothesis -- the pairs of
    _hypothesis_pairs, the fill run on out['diff_final_hand_vert'] as it is (flipped and root-relative already) -- reduced per image to
    hypothesis 0 | best-of-S | mean-of-S by the agreement kernel; NaN without data['gt_obj_rt']"""
    if not gt_vert.is_cuda:
        raise RuntimeError('grasp_multi_block: the contact agreement runs on the GPU only (no CPU path)')
    if 'gt_obj_rt' not in data:
        return torch.full((gt_vert.shape[0], GRASP_MULTI), float('nan'), device=gt_vert.device, dtype=torch.float32)
    pd_rt = _hypothesis_obj_rt(out, data['root_joint'].float().contiguous())
    return _grasp_against_gt(out['diff_final_hand_vert'], pd_rt, data, gt_vert, meter)[2].float()


def grasp_table(block, multi=None):
    """the table 'grasp' of Trainer.eval / EVAL_JSON from the (n, 8) columns grasp_block [and the (n, 24) grasp_multi_block] made:
    {'pred': {...}[, 'one_candidate': ..., 'best_of_S': ..., 'mean_of_S': ...]}, each the ops_names.GRASP_TABLE keys: the fp64 mean of
    every value over the images where it is defined (NaN where it never is), then IoU_defined, the share of images with an IoU"""
    block, names = _with_multi('grasp', block, multi, ('pred',))
    blk = block.double()
    ok = ~blk.isnan()
    mean = torch.where(ok, blk, torch.zeros_like(blk)).sum(0) / ok.sum(0)                # 0 / 0 = NaN: never defined
    share = ok.double().mean(0)
    return {src: dict({k: float(mean[8 * s + i]) for i, k in enumerate(GRASP_METRIC_NAMES)}, IoU_defined=float(share[8 * s]))
            for s, src in enumerate(names)}


def build_meters(layout, assets, device):
    """what the blocks of ``layout`` need built, once, before a timed loop: the object meshes, acceleration tables, closed hand mesh, solids
    and columns (physics_meter), the symmetry table (symmetry_meter, which refuses one that is too long) and the hand surface, anchor and
    object vertex tables (grasp_meter); nothing, and no import, for a block the layout lacks"""
    if layout.has('physics') or layout.has('volume'):
        physics_meter(assets, device, multi=layout.has('physics_multi'), volume=layout.has('volume'), volume_multi=layout.has('volume_multi'))
    if layout.has('symmetric'):
        symmetry_meter(assets, device)
    if layout.has('grasp'):
        grasp_meter(assets, device)


def metric_rows(out, data, gt_joint, gt_vert, first_index, assets=None, *, layout=None):
    """(bs, layout.width) fp32 on the model's device: the blocks of ``layout`` (an eval_layout.RowLayout, as RowLayout.resolve makes it of
    the flags; default: the base block alone), each filled by its block function; a block that the layout does not have costs no launch."""
    if layout is None:
        layout = RowLayout()
    for name, tables in (('physics', 'object meshes'), ('volume', 'object meshes, hand faces'),
                         ('symmetric', 'object corners, sampled vertices, diameters'), ('grasp', 'hand faces, anchors, object vertices')):
        if assets is None and layout.has(name):
            raise ValueError(f'metric_rows: eval_{name} needs the asset tables ({tables})')
    pp = postprocess(out, data['root_joint'], data['is_right'])
    bs, dev = gt_joint.shape[0], gt_joint.device
    rows = torch.empty((bs, layout.width), device=dev, dtype=torch.float32)
    if torch.is_tensor(first_index):                 # per-image ids (a loader batch that is not a run of the data set)
        rows[:, 0] = first_index.to(device=rows.device, dtype=torch.float32).reshape(bs)
    else:
        rows[:, 0] = torch.arange(first_index, first_index + bs, device=rows.device, dtype=torch.float32)
    rows[:, 1] = mje_mm(pp['reg_hand_joint'], gt_joint)
    rows[:, 2] = mje_mm(pp['first_hand_joint'], gt_joint)
    rows[:, 3] = mje_mm(pp['agg_hand_joint'], gt_joint)
    rows[:, 4] = mje_mm(pp['agg_hand_vert'], gt_vert)
    rows[:, 5] = mje_mm(pp['agg_hand_joint'], pp['reg_hand_joint'])
    rows[:, 6] = out['agg_obj_6d'][:, 6:].float().norm(dim=-1)
    rows[:, 7] = data['is_right'].float()
    rows[:, 8:ROW] = 0.0
    if gt_joint.is_cuda:                 # Procrustes-aligned metrics by the HIP kernel (test.py:657-680 on the device)
        from . import ops
        c = lambda t: t.float().contiguous()
        rows[:, 8] = ops.hand_metrics(c(pp['reg_hand_joint']), c(gt_joint))[1] * 1000.0
        rows[:, 9] = ops.hand_metrics(c(pp['agg_hand_joint']), c(gt_joint))[1] * 1000.0
        rows[:, 10] = ops.hand_metrics(c(pp['agg_hand_vert']), c(gt_vert))[1] * 1000.0
        if assets is not None and 'gt_obj_rt' in data:
            rows[:, OBJ_COL:OBJ_COL + 16] = object_metric_block(out, data, assets).float()
    # in the order the blocks always ran; each lambda finds its block function in this module when it is called (tests put spies there)
    for name, block in (('multi', lambda: multi_hypothesis_block(out, data, gt_joint, gt_vert, assets)),
                        ('physics', lambda: physics_block(pp, out, data, gt_vert, physics_meter(assets, dev))),
                        ('physics_multi', lambda: physics_multi_block(out, data, physics_meter(assets, dev, multi=True))),
                        ('volume', lambda: volume_block(pp, out, data, gt_vert, physics_meter(assets, dev, volume=True))),
                        ('volume_multi', lambda: volume_multi_block(out, data, physics_meter(assets, dev, volume_multi=True))),
                        ('hand_bench', lambda: hand_bench_block(out, data, gt_joint, gt_vert)),
                        ('hand_bench_multi', lambda: hand_bench_multi_block(out, data, gt_joint, gt_vert)),
                        ('symmetric', lambda: symmetric_block(out, data, symmetry_meter(assets, dev))),
                        ('symmetric_multi', lambda: symmetric_multi_block(out, data, symmetry_meter(assets, dev))),
                        ('grasp', lambda: grasp_block(out, data, gt_vert, grasp_meter(assets, dev))),
                        ('grasp_multi', lambda: grasp_multi_block(out, data, gt_vert, grasp_meter(assets, dev)))):
        if layout.has(name):
            rows[:, layout.slice(name)] = block()
    from .configs.args import cfg
    if cfg.aggregation_mode_hand == '2D_pt_joint':
        # that mode fuses joints only; its vertices are the reference's all-zero mesh (aggregation.py:364-366): no vertex metric of it
        rows[:, 4] = float('nan')
        rows[:, 10] = float('nan')
        if layout.has('physics'):
            rows[:, layout.slice('physics')][:, 0:4] = float('nan')
        if layout.has('volume'):
            rows[:, layout.slice('volume')][:, 0:2] = float('nan')
        if layout.has('grasp'):
            rows[:, layout.slice('grasp')] = float('nan')
    return rows


class _Pending:
    """Future of one pipelined batch: the worker's future + the HIP event behind the batch's last kernel"""

    def __init__(self, fut):
        self._fut = fut

    def result(self, timeout=None):
        res, done = self._fut.result(timeout)
        done.synchronize()
        return res

    def done(self):
        return self._fut.done() and self._fut.result()[1].query()


class PipelinedPredictor:
    """Evaluation batches are independent, so `depth` of them are kept in flight: each on its own HIP stream, driven by its own
    host thread and execution plan (packed weights are per plan).  One batch alone leaves the GPU idle at the sampler's
    per-attempt host syncs and at the tails of its small launches; a second batch fills those gaps.
    The CPU prior draws are made by the submitting thread, in submission order (hand then object per batch), so a seeded
    run draws exactly what the sequential loop of the reference would (sde.py:26-28)."""

    def __init__(self, model, depth=3):
        import threading
        from concurrent.futures import ThreadPoolExecutor
        from .model.engine import Engine
        self.model, self.depth = model, depth
        self.engines = [Engine(model) for _ in range(depth)]
        self.dev = self.engines[0].dev
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(depth)]
        self.locks = [threading.Lock() for _ in range(depth)]
        # ONE worker thread and queue per slot: with a shared pool a thread that has finished its slot's batch takes the next task in line,
        # which may belong to ANOTHER slot, and sleeps on that slot's lock while its own slot sits idle
        self.pools = [ThreadPoolExecutor(max_workers=1, thread_name_prefix=f'vpho-predict-{i}') for i in range(depth)]
        self.n = 0
        import os
        self.sync_in_worker = os.environ.get('VPHO_PIPE_SYNC_IN_WORKER', '0') == '1'      # A/B aid: the round-1 behaviour

    def submit(self, batch, post=None):
        """Returns a future of post(out, batch, engine) (or of the output dict).  The worker thread only ENQUEUES the batch and
        moves on to its next one; ``.result()`` waits (in the caller's thread, sleeping) for the event recorded behind the batch's
        last kernel, so the result can be consumed from any stream."""
        from .configs.args import cfg
        bs = batch['rgb'].shape[0]
        noise_h = torch.randn(bs * cfg.sample_num, 96)
        noise_o = torch.randn(bs * cfg.sample_num, 9)
        slot = self.n % self.depth
        self.n += 1
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.dev))

        def work():
            with self.locks[slot], torch.cuda.device(self.dev), torch.cuda.stream(self.streams[slot]), torch.no_grad():
                self.streams[slot].wait_event(ready)
                eng = self.engines[slot]
                out = eng.predict(batch, noise_hand=noise_h, noise_obj=noise_o)
                res = post(out, batch, eng) if post is not None else out
                done = torch.cuda.Event(blocking=True)      # sleep, do not spin: the slot threads share the rank's CPU quota
                done.record(self.streams[slot])
                if self.sync_in_worker:
                    done.synchronize()
                return res, done

        return _Pending(self.pools[slot].submit(work))

    def close(self):
        for p in self.pools:
            p.shutdown(wait=True)


def gather_rows(rows):
    """All ranks' rows, concatenated in rank order.  Ranks may hold different numbers of rows (a data loader's ragged last batches, like
    accelerate's ``gather_for_metrics``, train_diff_hand_obj.py:333-335): the counts travel first (one all-gather of a single integer per
    rank), the rows padded to the largest count, the padding dropped again.  No-op without a process group."""
    from .launch import group_active
    if not group_active():
        return rows
    world = dist.get_world_size()
    try:
        host_stage = dist.get_backend() == 'gloo' and rows.is_cuda       # CPU rehearsal backend: stage through host memory
        dev = torch.device('cpu') if host_stage else rows.device
        counts = torch.zeros(world, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(counts, torch.tensor([rows.shape[0]], dtype=torch.int64, device=dev))
        counts = counts.tolist()
        cap = max(counts)
        mine = torch.zeros((cap, rows.shape[1]), device=dev, dtype=rows.dtype)
        mine[:rows.shape[0]] = rows.to(dev)
        out = torch.empty((world * cap, rows.shape[1]), device=dev, dtype=rows.dtype)
        dist.all_gather_into_tensor(out, mine)
        if rows.is_cuda and not host_stage:
            torch.cuda.current_stream(rows.device).synchronize()          # an RCCL failure surfaces HERE, with the context below
        out = torch.cat([out[r * cap:r * cap + counts[r]] for r in range(world)], 0) if any(c != cap for c in counts) else out
        return out.to(rows.device)
    except Exception as e:
        raise RuntimeError(f'gather_rows: the all-gather of the metric rows failed on rank {dist.get_rank()} of {world} (backend '
                           f'{dist.get_backend()}, {tuple(rows.shape)} rows on {rows.device}): {type(e).__name__}: {e}') from e


def shard_range(n_items, rank, world):
    """Contiguous shard [lo, hi) of n_items for strong-scaling splits of one global batch."""
    per = (n_items + world - 1) // world
    lo = min(rank * per, n_items)
    return lo, min(lo + per, n_items)


def summarize(rows, layout=None):
    """Table like train_diff_hand_obj.py:336-357 for right / left / both hands, then one table per block of ``layout`` (default:
    RowLayout.from_width, for rows without hand-benchmark blocks; a width it does not know is a ValueError)."""
    if layout is None:
        layout = RowLayout.from_width(rows.shape[1])
    elif rows.shape[1] != layout.width:
        raise ValueError(f'summarize: rows of {rows.shape[1]} columns with a layout of {layout.width}')
    block = lambda name: rows[:, layout.slice(name)]
    res = {}
    for name, mask in (('right', rows[:, 7] > 0.5), ('left', rows[:, 7] < 0.5), ('both', torch.ones_like(rows[:, 7], dtype=torch.bool))):
        sel = rows[mask]
        if sel.shape[0] == 0:
            continue
        res[name] = dict(n=int(sel.shape[0]), MJE_reg=float(sel[:, 1].mean()), MJE_first=float(sel[:, 2].mean()),
                         MJE_agg=float(sel[:, 3].mean()), MVE_agg=float(sel[:, 4].mean()), PA_MJE_reg=float(sel[:, 8].mean()),
                         PA_MJE_agg=float(sel[:, 9].mean()), PA_MVE_agg=float(sel[:, 10].mean()))
    # object table (test.py:521-584 'average_instance' column: distances in mm, hit rates / F-scores in percent, REP in pixels)
    res['object'] = _object_table(rows[:, OBJ_COL:OBJ_COL + 16].double().mean(0))
    if layout.has('volume'):
        res['volume'] = _volume_table(block('volume'))
        if layout.has('volume_multi'):
            # every hypothesis' volume reduced per image: for mean_of_S an image counts as intersecting when its mean cell count is > 0
            res['volume'].update(_volume_table(block('volume_multi'), MULTI_TABLES))
    if layout.has('physics'):
        res['physics'] = _physics_table(block('physics'), PHYSICS_SOURCES)
        if layout.has('physics_multi'):
            # every hypothesis' penetration reduced per image (physics_multi_block): for mean_of_S an image counts as penetrating when
            # its mean inside-vertex count is > 0, and its contact is the fraction of its hypotheses in contact
            res['physics'].update(_physics_table(block('physics_multi'), MULTI_TABLES))
    if layout.has('multi'):
        # multi-hypothesis tables (train_diff_hand_obj.py:466-469,494-496 one_candidate; TesterObject.postprocess best_candidate_pose),
        # over all images: hand in mm, object in the units of the object table
        blk = block('multi').double().mean(0)
        for t, name in enumerate(MULTI_TABLES):
            res[name] = dict(hand={k: float(blk[4 * t + i]) for i, k in enumerate(HAND_METRIC_NAMES)},
                             object=_object_table(blk[12 + 16 * t:28 + 16 * t]))
    for name, table in (('hand_bench', hand_bench_table), ('symmetric', symmetric_table), ('grasp', grasp_table)):
        if layout.has(name):
            res[name] = table(block(name), block(name + '_multi') if layout.has(name + '_multi') else None)
    return res


def _object_table(obj):
    return {k: float(obj[i] * (1000.0 if k in ('MCE', 'OCE', 'MCE2', 'ADD', 'ADDS', 'CD') else (1.0 if k == 'REP' else 100.0)))
            for i, k in enumerate(OBJ_METRIC_NAMES)}


def _volume_table(blk, names=None):
    """volume table over all images, per source (pred / gt; one_candidate / best_of_S / mean_of_S): mean and largest intersection volume
    (cm^3) and the share of images with at least one solid cell of the object inside the hand (%); NaN for a source without values"""
    blk = blk.double()
    res = {}
    for s, name in enumerate(PHYSICS_SOURCES if names is None else names):
        iv, cells = blk[:, 2 * s], blk[:, 2 * s + 1]
        res[name] = dict(IV_cm3=float(iv.mean() * 1e6), IV_max_cm3=float(iv.max() * 1e6) if iv.shape[0] else float('nan'),
                         intersecting_pct=float((cells > 0).double().mean() * 100.0) if not cells.isnan().any() else float('nan'))
    return res


def _physics_table(blk, names):
    """physics table over all images, per source (pred / gt; one_candidate / best_of_S / mean_of_S): mean and largest PD (mm), % of images
    with a hand vertex inside the object, mean inside-vertex count, % of images in contact (NaN for a source without values, e.g. gt
    without object ground truth)"""
    blk = blk.double()
    res = {}
    for s, name in enumerate(names):
        b = blk[:, 4 * s:4 * s + 4]
        res[name] = dict(PD_mm=float(b[:, 0].mean() * 1000.0), PD_max_mm=float(b[:, 0].max() * 1000.0) if b.shape[0] else float('nan'),
                         penetration_rate_pct=float((b[:, 1] > 0).double().mean() * 100.0) if not b[:, 1].isnan().any() else float('nan'),
                         inside_verts=float(b[:, 1].mean()), contact_rate_pct=float(b[:, 3].mean() * 100.0))
    return res

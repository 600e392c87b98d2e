"""Evaluation loop of the hot path: per-rank batches, per-image metric rows, ONE fixed-layout all-gather.

Counterpart of the reference's ``Trainer.evaluate`` / ``postprocess`` (lib/engine/train_diff_hand_obj.py:202-357,578-602)
for synthetic batches.  The reference gathers pickled nested dicts with ``gather_for_metrics(use_gather_object=True)``
(:333-335); here every rank fills a ``(n_images, ROW)`` fp32 tensor on its GPU and the ranks exchange it with a single
``torch.distributed.all_gather_into_tensor`` (RCCL over xGMI with backend 'nccl', gloo on CPU for tests).
The forward pass itself needs no collective: the image batch is the only sharded dimension.
"""
import torch
import torch.distributed as dist

from .ops_names import MULTI_TABLES  # noqa: F401  (table names of summarize with eval_best)

# row layout: [global image index, MJE(regression), MJE(first hypothesis), MJE(aggregated), MVE(aggregated),
#              |agg - regression| mean joint distance (mm), object translation norm (m), is_right,
#              PA-MJE(regression), PA-MJE(aggregated), PA-MVE(aggregated), 0,
#              then the 16 object metrics of the aggregated pose in the order of ops.OBJ_METRIC_NAMES (TesterObject,
#              test.py:240-503: MCE, OCE, MCE2, ADD, ADD-S, ADD<0.1d, ADD-S<0.1d, REP, REP<5px, CD, F-score x6)]
ROW = 28
OBJ_COL = 12
# with eval_best (cfg.eval_best, the reference's is_eval_best) every row carries MULTI more columns from ROW on, in the order of
# ops_names.MULTI_COLUMNS: hand one_candidate / best_of_S / mean_of_S (MJE, PA-MJE, MVE, PA-MVE in mm, 4 each), then object
# one_candidate / best_of_S / mean_of_S (the 16 OBJ_METRIC_NAMES each).  Columns 0-27 are the same with and without the flag.
MULTI = 60
ROW_BEST = ROW + MULTI
# with eval_physics (cfg.eval_physics) every row carries PHYS more columns, last (after the eval_best block if there is one), in the
# order of ops_names.PHYSICS_COLUMNS: PD (m), n_inside, min sd (m), contact of (aggregated hand, aggregated object), then of (ground-truth
# hand, ground-truth object).  The columns before them are the same with and without the flag.
PHYS = 8
# with physics_multi (both command-line flags, cfg.eval_best AND cfg.eval_physics; an explicit argument of Trainer.eval / metric_rows
# otherwise, so that callers who pass the two older flags themselves get the rows they always got) every row carries PHYS_MULTI more
# columns, last (after the PHYS block), in the order of
# ops_names.PHYSICS_MULTI_COLUMNS: PD (m), n_inside, min sd (m), contact of (hand hypothesis s, object hypothesis s) reduced per image to
# hypothesis 0, best-of-S and mean-of-S.  The 96 columns before them are the same with and without the block.
PHYS_MULTI = 12
# with eval_volume (cfg.eval_volume; independent of the flags above) every row carries VOL more columns, last of all, in the order of
# ops_names.VOLUME_COLUMNS: IV (m^3) and the solid-cell count of (aggregated hand, aggregated object), then of the ground-truth pair.
# Every column before them is the same with and without the flag.
VOL = 4
# with volume_multi (both command-line flags, cfg.eval_best AND cfg.eval_volume; an explicit argument of Trainer.eval / metric_rows
# otherwise, as physics_multi) every row carries VOL_MULTI more columns IMMEDIATELY BEFORE the VOL block -- rows[:, -VOL:] is the volume
# block in every layout --, in the order of ops_names.VOLUME_MULTI_COLUMNS: IV (m^3) and the solid-cell count of (hand hypothesis s,
# object hypothesis s) reduced per image to hypothesis 0, best-of-S and mean-of-S.  Widths 98, 106 and 118: no other layout has them.
VOL_MULTI = 6
# with eval_hand_bench (cfg.eval_hand_bench; Trainer.eval, not metric_rows: its signature and summarize's width table are frozen) the
# pipeline callback appends HAND_BENCH more columns AFTER everything metric_rows returns, in the order of ops_names.HAND_BENCH_COLUMNS:
# the eight leaderboard values of the aggregated hand, then of the regression hand; with hand_bench_multi (both
# command-line flags, cfg.eval_best AND cfg.eval_hand_bench; an explicit argument of Trainer.eval otherwise) HAND_BENCH_MULTI more after
# those (ops_names.HAND_BENCH_MULTI_COLUMNS).  summarize never sees them: Trainer.eval cuts them off and tabulates them by
# hand_bench_table.  In these layouts rows[:, -VOL:] is NOT the volume block.
HAND_BENCH = 16
HAND_BENCH_MULTI = 24


def row_width(eval_best=False, eval_physics=False, physics_multi=False, volume_multi=False, eval_volume=False):
    return (ROW_BEST if eval_best else ROW) + (PHYS if eval_physics else 0) + (PHYS_MULTI if eval_best and eval_physics and physics_multi else 0) + \
        (VOL_MULTI if eval_best and eval_volume and volume_multi else 0) + (VOL if eval_volume else 0)


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


def object_metric_block(out, data, assets):
    """(bs,16) fp64: TesterObject on the aggregated object pose ('mean_candidate_pose', train_diff_hand_obj.py:249-258,
    498-501) -- obj_9D_to_mat + root joint, then the device metric kernels.  Needs data['gt_obj_rt'], data['cam_intr']."""
    from . import ops
    dev = out['agg_obj_6d'].device
    key = (id(assets), str(dev))
    if key not in _OBJ_METRICS:
        _OBJ_METRICS[key] = ops.ObjectMetrics(assets['ycb'], dev)
    M = _OBJ_METRICS[key]
    pd_rt = ops.obj_9d_to_rt(out['agg_obj_6d'].double().contiguous(), data['root_joint'].float().contiguous())
    return M(pd_rt, data['gt_obj_rt'].double().contiguous(), data['cam_intr'].double().contiguous(), M.obj_ids(data['obj_name']))


def multi_hypothesis_block(out, data, gt_joint, gt_vert, assets=None):
    """(bs, MULTI) fp32: every sampled hypothesis scored (test_diff_hand / test_diff_object with is_eval_best,
    train_diff_hand_obj.py:454-523) and reduced per image to hypothesis 0, best-of-S and mean-of-S.  Hand by the multi-hypothesis
    Procrustes kernel on the model-frame candidates (postprocess on load), object by ObjectMetrics.multi on obj_9D_to_mat + root of
    every candidate; object columns stay 0 without object tables or data['gt_obj_rt'], as in the 28-column block."""
    from . import ops
    if not gt_joint.is_cuda:
        raise RuntimeError('multi_hypothesis_block: the multi-hypothesis metrics run on the GPU only (no CPU path)')
    bs = gt_joint.shape[0]
    blk = torch.zeros((bs, MULTI), device=gt_joint.device, dtype=torch.float32)
    root = data['root_joint'].float().contiguous()
    c = lambda t: t.float().contiguous()
    mje, pa_mje = ops.hand_metrics_multi(c(out['diff_final_hand_joint']), c(gt_joint), root, data['is_right'])
    mve, pa_mve = ops.hand_metrics_multi(c(out['diff_final_hand_vert']), c(gt_vert), root, data['is_right'])
    hand = torch.stack([mje, pa_mje, mve, pa_mve], -1) * 1000.0                 # (bs, S, 4) mm
    blk[:, 0:4] = hand[:, 0]
    blk[:, 4:8] = hand.amin(1)
    blk[:, 8:12] = hand.mean(1)
    if assets is not None and 'gt_obj_rt' in data:
        key = (id(assets), str(gt_joint.device))
        if key not in _OBJ_METRICS:
            _OBJ_METRICS[key] = ops.ObjectMetrics(assets['ycb'], gt_joint.device)
        M = _OBJ_METRICS[key]
        x = out['diff_final_obj_6d']
        S = x.shape[1]
        pd_rt = ops.obj_9d_to_rt(x.reshape(bs * S, 9).double().contiguous(), root.repeat_interleave(S, 0).contiguous()).view(bs, S, 3, 4)
        per, best, mean = M.multi(pd_rt, data['gt_obj_rt'].double().contiguous(), data['cam_intr'].double().contiguous(),
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
    key = (id(assets), str(device))
    if key not in _PHYSICS:
        from . import ops
        from .configs.args import cfg
        from .physics_eval import object_meshes
        _PHYSICS[key] = ops.HandObjectPenetration(object_meshes(assets, cfg.asset_root), device, accel=False)
    if multi:
        _PHYSICS[key].build_accel()
    if volume or volume_multi:
        from .configs.args import cfg
        if _PHYSICS[key].hand_faces is None:
            from .physics_eval import hand_faces
            _PHYSICS[key].set_hand_faces(hand_faces(assets))
        _PHYSICS[key].build_solids(float(cfg.physics_voxel_pitch))
        if volume_multi:
            _PHYSICS[key].build_solid_columns(float(cfg.physics_voxel_pitch))
    return _PHYSICS[key]


def physics_block(pp, out, data, gt_vert, meshes):
    """(bs, PHYS) fp32: hand-object penetration and contact of the aggregated hand vertices (pp['agg_hand_vert'],
    postprocessed: camera frame) with the aggregated object pose (obj_9D_to_mat + root, as object_metric_block), then of the ground-truth
    vertices gt_vert with data['gt_obj_rt'] (NaN without it).  ``meshes``: an ops.HandObjectPenetration (physics_meter)."""
    from . import ops
    from .configs.args import cfg
    if not gt_vert.is_cuda:
        raise RuntimeError('physics_block: the penetration metrics run on the GPU only (no CPU path)')
    bs = gt_vert.shape[0]
    blk = torch.full((bs, PHYS), float('nan'), device=gt_vert.device, dtype=torch.float32)
    ids = meshes.obj_ids(data['obj_name'])
    th = float(cfg.physics_contact_thresh)
    pd_rt = ops.obj_9d_to_rt(out['agg_obj_6d'].double().contiguous(), data['root_joint'].float().contiguous())
    blk[:, 0:4] = meshes(pp['agg_hand_vert'].float().contiguous(), pd_rt, ids, th).float()
    if 'gt_obj_rt' in data:
        blk[:, 4:8] = meshes(gt_vert.float().contiguous(), data['gt_obj_rt'].double().contiguous(), ids, th).float()
    return blk


def volume_block(pp, out, data, gt_vert, meshes):
    """(bs, VOL) fp32: the hand-object intersection volume of the pairs of physics_block -- the aggregated hand
    vertices (pp['agg_hand_vert'], camera frame) with the aggregated object pose, then the ground-truth vertices with data['gt_obj_rt']
    (NaN without it) -- as IV (m^3) | solid-cell count each.  ``meshes``: physics_meter(..., volume=True)."""
    from . import ops
    from .configs.args import cfg
    if not gt_vert.is_cuda:
        raise RuntimeError('volume_block: the intersection volume runs on the GPU only (no CPU path)')
    bs = gt_vert.shape[0]
    blk = torch.full((bs, VOL), float('nan'), device=gt_vert.device, dtype=torch.float32)
    ids = meshes.obj_ids(data['obj_name'])
    h = float(cfg.physics_voxel_pitch)
    pd_rt = ops.obj_9d_to_rt(out['agg_obj_6d'].double().contiguous(), data['root_joint'].float().contiguous())
    blk[:, 0:2] = meshes.volume(pp['agg_hand_vert'].float().contiguous(), pd_rt, ids, h).flip(1).float()
    if 'gt_obj_rt' in data:
        blk[:, 2:4] = meshes.volume(gt_vert.float().contiguous(), data['gt_obj_rt'].double().contiguous(), ids, h).flip(1).float()
    return blk


def hypotheses_to_camera(x, root_joint, is_right):
    """(bs, S, N, 3) model-frame hand candidates -> camera frame: postprocess' un-flip of left hands along x + root joint, per hypothesis"""
    sgn = torch.where(is_right.bool(), 1.0, -1.0).to(x.dtype)[:, None, None]
    v = x.clone()
    v[..., 0] = v[..., 0] * sgn
    return v + root_joint[:, None, None]


def physics_multi_block(out, data, meshes):
    """(bs, PHYS_MULTI) fp32: penetration and contact of every sampled hypothesis -- hand candidate s
    (out['diff_final_hand_vert'][:, s], un-flipped + root as the multi-hypothesis hand metrics) against object candidate s
    (obj_9D_to_mat + root of out['diff_final_obj_6d'][:, s]) -- reduced per image to hypothesis 0 | best-of-S | mean-of-S by ONE
    HandObjectPenetration.multi launch pair.  ``meshes``: physics_meter(..., multi=True)."""
    from . import ops
    from .configs.args import cfg
    hv = out['diff_final_hand_vert']
    if not hv.is_cuda:
        raise RuntimeError('physics_multi_block: the penetration metrics run on the GPU only (no CPU path)')
    bs, S = hv.shape[:2]
    root = data['root_joint'].float().contiguous()
    verts = hypotheses_to_camera(hv.float(), root, data['is_right']).contiguous()
    pd_rt = ops.obj_9d_to_rt(out['diff_final_obj_6d'].reshape(bs * S, 9).double().contiguous(), root.repeat_interleave(S, 0).contiguous()).view(bs, S, 3, 4)
    table, _ = meshes.multi(verts, pd_rt, meshes.obj_ids(data['obj_name']), contact_thresh=float(cfg.physics_contact_thresh))
    return table.float()


def volume_multi_block(out, data, meshes):
    """(bs, VOL_MULTI) fp32: the intersection volume of every sampled hypothesis, the pairing of
    physics_multi_block -- hand candidate s (out['diff_final_hand_vert'][:, s], un-flipped + root) against object candidate s
    (obj_9D_to_mat + root of out['diff_final_obj_6d'][:, s]) -- reduced per image to hypothesis 0 | best-of-S | mean-of-S by ONE
    HandObjectPenetration.volume_multi launch pair.  ``meshes``: physics_meter(..., volume_multi=True)."""
    from . import ops
    from .configs.args import cfg
    hv = out['diff_final_hand_vert']
    if not hv.is_cuda:
        raise RuntimeError('volume_multi_block: the intersection volume runs on the GPU only (no CPU path)')
    bs, S = hv.shape[:2]
    root = data['root_joint'].float().contiguous()
    verts = hypotheses_to_camera(hv.float(), root, data['is_right']).contiguous()
    pd_rt = ops.obj_9d_to_rt(out['diff_final_obj_6d'].reshape(bs * S, 9).double().contiguous(), root.repeat_interleave(S, 0).contiguous()).view(bs, S, 3, 4)
    table, _ = meshes.volume_multi(verts, pd_rt, meshes.obj_ids(data['obj_name']), float(cfg.physics_voxel_pitch))
    return table.float()


def hand_bench_width(multi=False):
    """columns that Trainer.eval appends after metric_rows' with eval_hand_bench: 16, or 40 with the multi-hypothesis block"""
    return HAND_BENCH + (HAND_BENCH_MULTI if multi else 0)


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


def hand_bench_table(block):
    """the table 'hand_bench' of Trainer.eval / EVAL_JSON from the (n, 16 | 40) columns hand_bench_block [+ hand_bench_multi_block] made:
    {'agg': {...}, 'reg': {...}[, 'one_candidate': ..., 'best_of_S': ..., 'mean_of_S': ...]}, each the ops_names.HAND_BENCH_TABLE keys as
    fp64 means over the images, in [0, 1] (NaN where a column holds one)"""
    from .ops_names import HAND_BENCH_SOURCES, HAND_BENCH_TABLE, MULTI_TABLES
    if block.shape[1] not in (HAND_BENCH, HAND_BENCH + HAND_BENCH_MULTI):
        raise ValueError(f'hand_bench_table: {block.shape[1]} columns, expected {HAND_BENCH} or {HAND_BENCH + HAND_BENCH_MULTI}')
    mean = block.double().mean(0)
    names = HAND_BENCH_SOURCES + (MULTI_TABLES if block.shape[1] > HAND_BENCH else ())
    return {src: {k: float(mean[8 * s + i]) for i, k in enumerate(HAND_BENCH_TABLE)} for s, src in enumerate(names)}


def metric_rows(out, data, gt_joint, gt_vert, first_index, assets=None, eval_best=False, eval_physics=False, physics_multi=False, volume_multi=False,
                eval_volume=False):
    """(bs, ROW) fp32 on the model's device; (bs, ROW_BEST) with eval_best (multi_hypothesis_block appended); PHYS more columns with
    eval_physics (physics_block), and with both and ``physics_multi`` PHYS_MULTI more (physics_multi_block; without it that block
    and its launch are left out: the rows of the two flags as they always were); VOL more with ``eval_volume`` (volume_block), last of
    all, whatever the other flags are; with eval_best, eval_volume and ``volume_multi`` VOL_MULTI more immediately before them
    (volume_multi_block; without it that block and its launches are left out)."""
    pp = postprocess(out, data['root_joint'], data['is_right'])
    bs = gt_joint.shape[0]
    rows = torch.empty((bs, row_width(eval_best, eval_physics, physics_multi, volume_multi, eval_volume)), device=gt_joint.device, dtype=torch.float32)
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
    if eval_best:
        rows[:, ROW:ROW_BEST] = multi_hypothesis_block(out, data, gt_joint, gt_vert, assets)
    if eval_physics:
        if assets is None:
            raise ValueError('metric_rows: eval_physics needs the asset tables (object meshes)')
        p0 = ROW_BEST if eval_best else ROW
        rows[:, p0:p0 + PHYS] = physics_block(pp, out, data, gt_vert, physics_meter(assets, gt_joint.device))
        if eval_best and physics_multi:
            rows[:, p0 + PHYS:p0 + PHYS + PHYS_MULTI] = physics_multi_block(out, data, physics_meter(assets, gt_joint.device, multi=True))
    if eval_volume:
        if assets is None:
            raise ValueError('metric_rows: eval_volume needs the asset tables (object meshes, hand faces)')
        v0 = rows.shape[1] - VOL
        rows[:, v0:] = volume_block(pp, out, data, gt_vert, physics_meter(assets, gt_joint.device, volume=True))
        if eval_best and volume_multi:
            rows[:, v0 - VOL_MULTI:v0] = volume_multi_block(out, data, physics_meter(assets, gt_joint.device, volume_multi=True))
    from .configs.args import cfg
    if cfg.aggregation_mode_hand == '2D_pt_joint':
        # that mode fuses joints only; its vertices are the reference's all-zero mesh (aggregation.py:364-366): no vertex metric of it
        rows[:, 4] = float('nan')
        rows[:, 10] = float('nan')
        if eval_physics:
            rows[:, p0:p0 + 4] = float('nan')
        if eval_volume:
            rows[:, v0:v0 + 2] = float('nan')
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


def summarize(rows):
    """Table like train_diff_hand_obj.py:336-357 for right / left / both hands."""
    res = {}
    for name, mask in (('right', rows[:, 7] > 0.5), ('left', rows[:, 7] < 0.5), ('both', torch.ones_like(rows[:, 7], dtype=torch.bool))):
        sel = rows[mask]
        if sel.shape[0] == 0:
            continue
        res[name] = dict(n=int(sel.shape[0]), MJE_reg=float(sel[:, 1].mean()), MJE_first=float(sel[:, 2].mean()),
                         MJE_agg=float(sel[:, 3].mean()), MVE_agg=float(sel[:, 4].mean()), PA_MJE_reg=float(sel[:, 8].mean()),
                         PA_MJE_agg=float(sel[:, 9].mean()), PA_MVE_agg=float(sel[:, 10].mean()))
    # object table (test.py:521-584 'average_instance' column: distances in mm, hit rates / F-scores in percent, REP in pixels)
    from .ops_names import OBJ_METRIC_NAMES
    obj = rows[:, OBJ_COL:OBJ_COL + 16].double().mean(0)
    res['object'] = _object_table(obj)
    # the widths without the volume block are 28, 88, 36, 96 and 108; with it each is 4 wider, and the three with the eval_best block
    # another 6 wider with the volume_multi block (98, 106, 118): no two layouts share a width
    if rows.shape[1] in tuple(w + VOL_MULTI + VOL for w in (ROW_BEST, ROW_BEST + PHYS, ROW_BEST + PHYS + PHYS_MULTI)):
        from .ops_names import MULTI_TABLES
        res['volume'] = _volume_table(rows[:, -VOL:])
        # every hypothesis' volume reduced per image (volume_multi_block): for mean_of_S an image counts as intersecting when its mean
        # cell count is > 0
        res['volume'].update(_volume_table(rows[:, -VOL - VOL_MULTI:-VOL], MULTI_TABLES))
        rows = rows[:, :-VOL - VOL_MULTI]
    elif rows.shape[1] in tuple(w + VOL for w in (ROW, ROW_BEST, ROW + PHYS, ROW_BEST + PHYS, ROW_BEST + PHYS + PHYS_MULTI)):
        res['volume'] = _volume_table(rows[:, -VOL:])
        rows = rows[:, :-VOL]
    p0 = {ROW + PHYS: ROW, ROW_BEST + PHYS: ROW_BEST, ROW_BEST + PHYS + PHYS_MULTI: ROW_BEST}.get(rows.shape[1])
    if p0 is not None:
        from .ops_names import MULTI_TABLES, PHYSICS_SOURCES
        res['physics'] = _physics_table(rows[:, p0:p0 + PHYS], PHYSICS_SOURCES)
        if rows.shape[1] > p0 + PHYS:
            # every hypothesis' penetration reduced per image (physics_multi_block): for mean_of_S an image counts as penetrating when
            # its mean inside-vertex count is > 0, and its contact is the fraction of its hypotheses in contact
            res['physics'].update(_physics_table(rows[:, p0 + PHYS:], MULTI_TABLES))
    if rows.shape[1] >= ROW_BEST:
        # multi-hypothesis tables (train_diff_hand_obj.py:466-469,494-496 one_candidate; TesterObject.postprocess best_candidate_pose),
        # over all images: hand in mm, object in the units of the object table
        from .ops_names import HAND_METRIC_NAMES, MULTI_TABLES
        blk = rows[:, ROW:ROW_BEST].double().mean(0)
        for t, name in enumerate(MULTI_TABLES):
            res[name] = dict(hand={k: float(blk[4 * t + i]) for i, k in enumerate(HAND_METRIC_NAMES)},
                             object=_object_table(blk[12 + 16 * t:28 + 16 * t]))
    return res


def _object_table(obj):
    from .ops_names import OBJ_METRIC_NAMES
    return {k: float(obj[i] * (1000.0 if k in ('MCE', 'OCE', 'MCE2', 'ADD', 'ADDS', 'CD') else (1.0 if k == 'REP' else 100.0)))
            for i, k in enumerate(OBJ_METRIC_NAMES)}


def _volume_table(blk, names=None):
    """volume table over all images, per source (pred / gt; one_candidate / best_of_S / mean_of_S): mean and largest intersection volume
    (cm^3) and the share of images with at least one solid cell of the object inside the hand (%); NaN for a source without values"""
    from .ops_names import PHYSICS_SOURCES
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

"""Contact-map and grasp agreement (``--eval_grasp``): does a predicted hand touch a predicted object where the
annotated hand touches the annotated object?

``vertex_accel`` / ``vertex_accel_tables`` build ``vpho_obj_vertex_accel`` (include/vpho_hip.h) from the objects' full vertices, with
numpy alone; ``nearest_walk`` restates the kernel's pruned walk on the host.  ``GraspMeter`` owns everything the device side needs --
the hand surface fill, the anchor tables, the vertex tables -- and is the one place where a contact map of a (hand, object pose) pair is
made for this metric: the annotation goes through the SAME kernel as the predictions (S = 1), so both sides share one arithmetic and a
prediction equal to its annotation scores IoU = F1 = 1, MAE = 0 exactly.  Dataset-supplied ``hand_contact`` labels are not used.

Imported only when a caller asks for it (evaluate.grasp_meter); the HIP library is loaded by GraspMeter, not by the import."""
import numpy as np

from .assets import AssetError

CLUSTER = 32                       # vertices per bounding sphere
REACH_GROW = 1.0 + 2.0 ** -20      # the kernel's relative slack on sqrt(best) (csrc/contact_multi.hip)
RADIUS_GROW = 2.0 ** -30           # the radii's relative slack, and their absolute one in units of the object's bounding-box diagonal


def vertex_accel(verts, cluster=CLUSTER):
    """``vpho_obj_vertex_accel`` of ONE object over its vertices ``verts`` (N, 3), N >= 1; deterministic (a stable sort, no random numbers):
      vert (N, 3) fp64: the vertices in Morton order of a 1024^3 lattice over their bounding box;  index (N,): their original indices;
      start (C + 1,): cluster k holds rows start[k] .. start[k + 1]: ``cluster`` rows, fewer in the last one (``cluster=None``: one
        cluster of all rows, the walk then visits every vertex);
      sphere (C, 4): the centre of the rows' bounding box and their largest distance from it, enlarged by (1 + RADIUS_GROW) and by
        RADIUS_GROW bounding-box diagonals (the slack the kernel's skip test relies on, derived in csrc/contact_multi.hip)."""
    v = np.ascontiguousarray(np.asarray(verts, np.float64).reshape(-1, 3))
    n = v.shape[0]
    if n == 0:
        raise AssetError('vertex_accel: an object without vertices')
    if not np.isfinite(v).all():
        raise AssetError('vertex_accel: a vertex is not a finite number')
    lo, hi = v.min(0), v.max(0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    g = np.clip(((v - lo) / ext * 1024.0).astype(np.int64), 0, 1023)
    code = np.zeros(n, np.int64)
    for bit in range(10):
        for k in range(3):
            code |= ((g[:, k] >> bit) & 1) << (3 * bit + k)
    order = np.argsort(code, kind='stable')
    step = n if cluster is None else int(cluster)
    if step < 1:
        raise AssetError(f'vertex_accel: clusters of {cluster} vertices')
    start = np.concatenate([np.arange(0, n, step), [n]]).astype(np.int64)
    vs = v[order]
    centre = (np.minimum.reduceat(vs, start[:-1], axis=0) + np.maximum.reduceat(vs, start[:-1], axis=0)) / 2.0
    owner = np.repeat(np.arange(len(start) - 1), np.diff(start))
    r0 = np.maximum.reduceat(np.sqrt(((vs - centre[owner]) ** 2).sum(-1)), start[:-1])
    radius = r0 * (1.0 + RADIUS_GROW) + RADIUS_GROW * np.sqrt(((hi - lo) ** 2).sum())
    return dict(vert=vs, index=order.astype(np.int32), start=start.astype(np.int32),
                sphere=np.ascontiguousarray(np.concatenate([centre, radius[:, None]], 1)))


def vertex_accel_tables(verts_per_object, cluster=CLUSTER):
    """the tables of all objects concatenated, none padded, in the order given (the order of the object ids): vert, index, clu_offset
    (n_obj + 1,), clu_start (C + 1,) with rows counted over all objects, clu_sphere (C, 4) -- the fields of vpho_obj_vertex_accel"""
    acc = [vertex_accel(v, cluster) for v in verts_per_object]
    if not acc:
        raise AssetError('vertex_accel_tables: no object')
    row0 = np.concatenate([[0], np.cumsum([len(a['vert']) for a in acc])])
    if row0[-1] > 0x7fffffff:
        raise AssetError(f'vertex_accel_tables: {row0[-1]} vertices in all, the tables index rows with 32 bits')
    return dict(vert=np.concatenate([a['vert'] for a in acc]), index=np.concatenate([a['index'] for a in acc]),
                clu_offset=np.concatenate([[0], np.cumsum([len(a['sphere']) for a in acc])]).astype(np.int32),
                clu_start=np.concatenate([a['start'][:-1].astype(np.int64) + row0[i] for i, a in enumerate(acc)] + [row0[-1:]]).astype(np.int32),
                clu_sphere=np.concatenate([a['sphere'] for a in acc]))


def _d2(p, v):
    """the kernel's squared distance: three differences, three squares, added left to right"""
    d = p[:, None, :] - v[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def nearest_walk(acc, pts):
    """Host restatement of the kernel's pruned walk over ONE object's ``vertex_accel``: the cluster with the nearest centre first (the
    first of equally near ones), then the clusters in order, skipping those with |p - centre| > sqrt(best) REACH_GROW + radius; the
    lexicographic minimum of (squared distance, original index) over the visited vertices.  ``pts`` (P, 3) in the model frame.
    -> (index (P,) original index of the nearest vertex, best (P,) squared distance, visited (P,) how many vertices were looked at)"""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    P, start, sphere = len(p), acc['start'].astype(np.int64), acc['sphere']
    D2 = _d2(p, sphere[:, :3])
    seed = D2.argmin(1)
    best, bi, visited = np.full(P, np.inf), np.full(P, np.iinfo(np.int64).max), np.zeros(P, np.int64)

    def scan(rows, k):
        if len(rows) == 0:
            return
        d2 = _d2(p[rows], acc['vert'][start[k]:start[k + 1]])
        idx = acc['index'][start[k]:start[k + 1]].astype(np.int64)
        for j in range(d2.shape[1]):                                    # in row order, with the kernel's compare
            better = (d2[:, j] < best[rows]) | ((d2[:, j] == best[rows]) & (idx[j] < bi[rows]))
            best[rows[better]], bi[rows[better]] = d2[better, j], idx[j]
        visited[rows] += d2.shape[1]

    for k in range(len(sphere)):
        scan(np.nonzero(seed == k)[0], k)
    for k in range(len(sphere)):
        lim = np.sqrt(best) * REACH_GROW + sphere[k, 3]
        scan(np.nonzero((seed != k) & ~(D2[:, k] > lim * lim))[0], k)
    return bi, best, visited


class GraspMeter:
    """``GraspMeter(cfg, assets, device)``: contact maps of (hand, object pose) pairs and their agreement, on the device.
    Gates: cfg.contact_normal_distance_thresh, cfg.contact_vertical_distance_thresh and PhysicsLabeler.DECAY, those of the label chain."""

    def __init__(self, cfg, assets, device, cluster=CLUSTER):
        import torch
        from . import ops
        from .assets import ANCHOR_SKELETON
        from .physics_labels import PhysicsLabeler, gap_table
        self.device = torch.device(device)
        self.agg = ops.Aggregation(assets, ANCHOR_SKELETON, self.device)
        self.gap = gap_table(cfg.asset_root, assets['mano']['v_template'])
        self.surface = ops.HandSurface(np.asarray(assets['mano']['faces']), self.gap['links'], self.gap['alpha'], self.device, n_verts=778)
        self.names = list(assets['ycb'].keys())
        self.name_to_id = {n: i for i, n in enumerate(self.names)}
        self.tables = vertex_accel_tables([assets['ycb'][n]['verts'] for n in self.names], cluster)
        self.kernel = ops.ContactMulti(self.tables, self.device)
        self.normal_thresh = tuple(float(x) for x in cfg.contact_normal_distance_thresh)
        self.vertical_thresh = float(cfg.contact_vertical_distance_thresh)
        self.decay = PhysicsLabeler.DECAY
        self.Nh = self.surface.V + self.surface.L

    def obj_ids(self, names):
        """class indices of a batch as a device tensor (ObjectMetrics.obj_ids)"""
        from . import ops
        return ops._ids_to_device([self.name_to_id[n] for n in names], self.device)

    def fill(self, hand_vert_flip):
        """(n, S, 778, 3) hand vertices in the flipped, root-relative frame -> filled vertices and normals (n, S, Nh, 3) fp32"""
        n, S = hand_vert_flip.shape[:2]
        vf, nf = self.surface.fill(hand_vert_flip.float().reshape(n * S, self.surface.V, 3).contiguous())
        return vf.view(n, S, self.Nh, 3), nf.view(n, S, self.Nh, 3)

    def contact(self, filled_v, filled_n, root, is_right, rt, obj_id, per_vertex=False):
        """ops.ContactMulti with this meter's gates: filled_v, filled_n (n,S,Nh,3), root (n,3), is_right (n,), rt (n,S,3,4) camera frame,
        obj_id (n,) int32 -> weight (n,S,Nh) in [0, 1] (with per_vertex: + nn_index, nd, vd)"""
        import torch
        return self.kernel(filled_v.contiguous(), filled_n.contiguous(), root.to(self.device, torch.float64).contiguous(),
                           is_right.to(self.device).bool().to(torch.uint8).contiguous(), rt.to(self.device, torch.float64).contiguous(), obj_id,
                           self.normal_thresh, self.vertical_thresh, self.decay, per_vertex)

    def pooled(self, weight):
        """weight (..., Nh) -> force_contact (..., 32) fp32, is_grasped (...) uint8: vpho_force_contact_f32 over all maps"""
        fc, gr = self.agg.force_contact(weight.reshape(-1, weight.shape[-1]).contiguous())
        return fc.view(*weight.shape[:-1], 32), gr.view(*weight.shape[:-1])

    def agreement(self, weight, weight_gt):
        """weight (n,S,Nh) of the predictions, weight_gt (n,Nh) of the annotation -> counts (n,S,3) int32 = TP, P, G; values (n,S,8)
        fp64 in the order of ops_names.GRASP_METRIC_NAMES; table (n,24) fp64 = hypothesis 0 | best-of-S | mean-of-S"""
        from . import ops
        fc, gr = self.pooled(weight)
        fc_gt, gr_gt = self.pooled(weight_gt)
        return ops.contact_agreement(weight.contiguous(), weight_gt.contiguous(), fc, gr, fc_gt, gr_gt)

    def score(self, hand_vert_flip, rt, gt_hand_vert_flip, gt_rt, root, is_right, obj_id):
        """predictions (n,S,778,3) / (n,S,3,4) against the annotation (n,778,3) / (n,3,4): both sides through fill and contact, then
        agreement -> counts, values, table"""
        w = self.contact(*self.fill(hand_vert_flip), root, is_right, rt, obj_id)
        w_gt = self.contact(*self.fill(gt_hand_vert_flip[:, None]), root, is_right, gt_rt[:, None], obj_id)[:, 0]
        return self.agreement(w, w_gt.contiguous())

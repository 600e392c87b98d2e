"""Physics labels from annotations: hand_contact, force_contact, is_grasped and (on request) the pseudo-forces, all on the device.

The reference derives them per sample on the CPU: ``get_hand_contact`` (lib/dataset/base.py:841-911: trimesh vertex normals,
``fill_finger_gaps_in_mano``, ``detect_hand_and_object_contact`` against the posed object vertices), then ``np.clip(., 0, 1)``,
``get_force_contact`` and ``check_is_grasped`` (dexycb6.py:320-332), and ``ForceOptimizer.optimize_batch``
(lib/engine/force_optimization.py:110-207) for ``force_local``.  Here the chain is five launches per batch -- ``ops.HandSurface.fill``,
``Aggregation.hand_contact``, a clamp, ``Aggregation.force_contact`` -- and ``Aggregation.force_optimize`` behind them.

Everything runs in the flipped (right-hand), root-relative frame of ``gt_hand_vert_flip``, as the force optimiser does
(force_optimization.py:132-136): a left hand's vertices, the object's vertices, gravity and obj_CoM have x negated, so MANO's right-hand
faces are wound outwards for both sides; negation is exact, so distances and dot products are those of the unflipped left-hand mesh.

Imported only when a caller asks for labels (``force_optim.py --frame_source``, ``--frame_contact``)."""
import os

import numpy as np
import torch

from . import ops
from .assets import ANCHOR_SKELETON, YCB_NAMES, _report

GAP_FILE = os.path.join('ours', 'finger_gap_links.npz')
# rows of the fill per finger segment, in the order the reference emits them: a segment of kind M / P / D with c links gives 3 / 2 / 1
# blocks of c rows with alpha = 1/4 2/4 3/4 | 1/3 2/3 | 1/2 (hand_fn.py:294, NUM_FILL)
GAP_SEGMENTS = (('M', 11), ('P', 10), ('D', 12), ('M', 10), ('P', 10), ('D', 11), ('M', 10), ('P', 10), ('D', 12), ('M', 10), ('P', 10), ('D', 10),
                ('M', 10), ('P', 12))
GAP_FILL = {'M': 3, 'P': 2, 'D': 1}


def gap_alpha():
    """the (302,) weights of the fill in row order"""
    out = []
    for kind, count in GAP_SEGMENTS:
        nf = GAP_FILL[kind]
        for i in range(nf):
            out += [(i + 1) / (nf + 1)] * count
    return np.array(out, np.float64)


def synthetic_gap_table(v_template, seed=0):
    """a seeded table of the real one's shape and weights: every link joins two template vertices less than 2 cm apart; a link keeps its
    pair over the blocks that repeat it, as the real table does"""
    v = np.asarray(v_template, np.float64).reshape(-1, 3)
    r = np.random.default_rng(seed)
    d = np.linalg.norm(v[:, None] - v[None], axis=-1)
    links = []
    for kind, count in GAP_SEGMENTS:
        pairs = []
        while len(pairs) < count:
            a = int(r.integers(0, len(v)))
            near = np.flatnonzero((d[a] < 0.02) & (np.arange(len(v)) != a))
            if len(near):
                pairs.append((a, int(r.choice(near))))
        links += pairs * GAP_FILL[kind]
    return np.array(links, np.int32), gap_alpha()


def gap_table(asset_root, v_template=None, seed=0):
    """``{'links' (L,2) int32, 'alpha' (L,) float64, 'source'}``: ``<asset_root>/ours/finger_gap_links.npz`` (written by
    scripts/install_gap_table.py) when it exists, else the seeded synthetic table over ``v_template`` (default: the synthetic MANO
    template), said once on stderr.  A file that exists but cannot be used raises."""
    path = os.path.join(asset_root, GAP_FILE)
    if os.path.exists(path):
        with np.load(path, allow_pickle=False) as z:
            links, alpha = np.asarray(z['links']), np.asarray(z['alpha'], np.float64)
        if links.ndim != 2 or links.shape[1] != 2 or alpha.shape != (len(links),) or links.dtype.kind not in 'iu':
            raise ValueError(f'gap_table: {path} holds links {links.shape} {links.dtype} and alpha {alpha.shape}, expected (L, 2) integers and (L,)')
        return dict(links=links.astype(np.int32), alpha=alpha, source=path)
    if v_template is None:
        from .assets import synthetic_assets
        v_template = synthetic_assets(seed)['mano']['v_template']
    _report(f'finger gap table: no file {os.path.abspath(path)!r} -> seeded SYNTHETIC links (seed {seed}) of the same shape and weights; '
            f'contact labels are not those of the real table (scripts/install_gap_table.py writes it)')
    links, alpha = synthetic_gap_table(v_template, seed)
    return dict(links=links, alpha=alpha, source='synthetic')


def padded_object_table(ycb, names=YCB_NAMES):
    """(n_obj, N, 3) float64: the FULL vertices of every object, padded to the longest by repeating the object's last vertex.  The contact
    kernel keeps the smaller index among equally near points, so a repeated point changes neither a distance nor an index."""
    verts = [np.asarray(ycb[n]['verts'], np.float64).reshape(-1, 3) for n in names]
    top = max(len(v) for v in verts)
    return np.stack([np.concatenate([v, np.repeat(v[-1:], top - len(v), 0)]) for v in verts])


class PhysicsLabeler:
    """``PhysicsLabeler(cfg, assets, device)``; ``labeler(batch, optimize=False, ...)`` with a FramePipeline batch dict (or any dict with
    gt_hand_vert_flip, gt_obj_rt, root_joint, obj_id, is_right and, to optimise, gravity and obj_CoM) -> dict of device tensors:
    hand_contact (n, 778 + L), force_contact (n, 32), is_grasped (n,) bool, and with ``optimize`` force_local / force_global (n, 32, 3)
    and losses (batches, 4)."""
    DECAY = (-0.005, 0.005)                  # detect_hand_and_object_contact's default decay points: the reference never passes others

    def __init__(self, cfg, assets, device):
        self.cfg, self.device = cfg, torch.device(device)
        self.agg = ops.Aggregation(assets, ANCHOR_SKELETON, self.device)
        self.gap = gap_table(cfg.asset_root, assets['mano']['v_template'])
        self.surface = ops.HandSurface(np.asarray(assets['mano']['faces']), self.gap['links'], self.gap['alpha'], self.device, n_verts=778)
        self.obj_verts = torch.from_numpy(padded_object_table(assets['ycb'])).to(self.device)
        self.normal_thresh = tuple(float(x) for x in cfg.contact_normal_distance_thresh)
        self.vertical_thresh = float(cfg.contact_vertical_distance_thresh)

    def meta(self):
        return dict(contact_normal_distance_thresh=list(self.normal_thresh), contact_vertical_distance_thresh=self.vertical_thresh,
                    decay_points=list(self.DECAY), gap_table=self.gap['source'], filled_vertices=self.surface.V + self.surface.L)

    def object_verts(self, obj_rt, root, obj_id, is_right):
        """the padded full vertices of each sample's object in the flipped, root-relative frame: float64 torch ops, rounded to float32 once"""
        rt = obj_rt.to(self.device, torch.float64)
        v = self.obj_verts[obj_id.to(self.device).long()]
        p = v @ rt[:, :, :3].transpose(1, 2) + (rt[:, :, 3] - root.to(self.device, torch.float64))[:, None]
        sign = torch.where(is_right.to(self.device).bool(), 1.0, -1.0).to(torch.float64)
        p[..., 0] = p[..., 0] * sign[:, None]
        return p.float().contiguous()

    def contact(self, hand_vert_flip, obj_verts_flip):
        """steps 1 and 3-5: (n,778,3), (n,No,3) in the flipped frame -> hand_contact (n, 778 + L) in [0, 1], force_contact (n,32),
        is_grasped (n,) uint8"""
        vf, nf = self.surface.fill(hand_vert_flip.contiguous())
        hc = self.agg.hand_contact(vf, nf, obj_verts_flip, self.normal_thresh, self.vertical_thresh, self.DECAY).clamp_(0, 1)
        fc, grasped = self.agg.force_contact(hc)
        return hc, fc, grasped

    def __call__(self, batch, optimize=False, batch_size=64, iters=3000, phase1=300):
        if batch.get('gt_hand_vert_flip') is None:
            raise ValueError('PhysicsLabeler: the records carry no hand_vert, so there is no hand surface to label; vertices are not rebuilt '
                             'from MANO parameters here')
        hv = batch['gt_hand_vert_flip'].to(self.device, torch.float32).contiguous()
        right = batch['is_right'].to(self.device).bool()
        ov = self.object_verts(batch['gt_obj_rt'], batch['root_joint'], batch['obj_id'], right)
        hc, fc, grasped = self.contact(hv, ov)
        out = dict(hand_contact=hc, force_contact=fc, is_grasped=grasped.bool())
        if optimize:
            sign = torch.where(right, 1.0, -1.0).to(torch.float32)
            flip = lambda a: (a.to(self.device, torch.float32).reshape(-1, 3) * torch.stack([sign, torch.ones_like(sign), torch.ones_like(sign)], -1)).contiguous()
            out.update(self.optimize(hv, flip(batch['gravity']), flip(batch['obj_CoM']), fc, grasped, batch_size, iters, phase1))
        return out

    def optimize(self, hv, gravity, com, fc, grasped, batch_size=64, iters=3000, phase1=300):
        """ForceOptimizer.optimize_batch over n samples: the full batches in one call, a remainder as a second call with B = remainder
        (the reference's ``bs = len(rgb_path)`` of its last batch)"""
        n, B = hv.shape[0], int(batch_size)
        full = n // B * B
        parts = []
        for lo, hi, b in ((0, full, B), (full, n, n - full)):
            if hi > lo:
                parts.append(self.agg.force_optimize(hv[lo:hi].contiguous(), gravity[lo:hi].contiguous(), com[lo:hi].contiguous(), fc[lo:hi].contiguous(),
                                                     grasped[lo:hi].contiguous(), b, iters=iters, phase1=phase1))
        return {k: torch.cat([p[k] for p in parts]) for k in ('force_local', 'force_global', 'losses')}

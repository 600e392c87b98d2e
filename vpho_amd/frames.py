"""Frames in: raw uint8 camera frames + per-sample annotations -> the reference's batch dict on the device.

What lib/dataset/dexycb6.py:339-469 does per image on CPU workers, as a host-side crop plan (numpy float64, vectorised over the batch)
and two launches per batch (vpho_amd/csrc/frames.hip through ``ops.frame_patch`` / ``ops.heatmap_targets``).  Nothing here is imported
unless ``--frame_source`` is set or a caller builds a ``FramePipeline`` itself.

A *source* is anything with ``len(source)`` and ``source[i] -> (frame (H, W, 3) uint8 ndarray, record dict)``.  A record holds
``jt2d`` (21,2) pixel joints, ``joint_3d`` (21,3) m, ``mano_pose`` (48) axis-angle (global rotation + 15 joints, hands_mean added),
``mano_betas`` (10), ``is_right``, ``obj_id`` (index into assets.YCB_NAMES), ``obj_rt`` (3,4) [R | t], ``cam_intr`` (3,3) and optionally
``hand_vert`` (778,3), ``gravity`` (3), ``force_local`` (32,3), ``is_grasped``, ``index``.

Random draws: sample ``index`` of epoch ``epoch`` draws from ``np.random.default_rng((seed, epoch, index))`` in the order of
``sample_draws`` -- so an augmentation depends neither on the batch a sample falls into nor on rank or worker count, and a resumed
``Trainer.fit`` repeats it.
"""
import math
import os

import numpy as np
import torch

from .assets import YCB_NAMES

IMG_MEAN = (0.485, 0.456, 0.406)
IMG_STD = (0.229, 0.224, 0.225)
MAX_ERASE = 4            # rectangles the kernel takes per sample
FIT_TRIES = 99           # dexycb6.py:341-342: `n = 100; while n := n - 1`


# ------------------------------------------------------------------------------------------------------------------ boxes (misc_fn.py:87-170)
def pt2d_to_bbox2d(p):
    return np.stack([p[..., 0].min(-1), p[..., 1].min(-1), p[..., 0].max(-1), p[..., 1].max(-1)], -1)


def expand_bbox2d(b, scale_factor=1):
    c = (b[..., :2] + b[..., 2:]) / 2
    wh = (b[..., 2:] - b[..., :2]) * scale_factor
    return np.concatenate([c - wh / 2, c + wh / 2], -1)


def rect_bbox2d(b):
    ct = (b[..., :2] + b[..., 2:]) / 2
    m = (b[..., 2:] - b[..., :2]).max(-1)
    return np.concatenate([ct - m[..., None] / 2, ct + m[..., None] / 2], -1), m


def check_bbox2d(b, size):
    return (b[..., 0] >= 0) & (b[..., 1] >= 0) & (b[..., 2] <= size) & (b[..., 3] <= size) & (b[..., 0] < b[..., 2]) & (b[..., 1] < b[..., 3])


def project(p3d, K):
    """(..., N, 3) camera points, (..., 3, 3) -> (..., N, 2) pixels (project_pt3d_to_pt2d)"""
    q = p3d @ np.swapaxes(K, -1, -2)
    return q[..., :2] / q[..., 2:3]


# ------------------------------------------------------------------------------------------------------------------ draws
def eval_draws(n):
    """get_spatial_aug_params(is_train=False), base.py:515-518: zeros, 1 and 0"""
    return dict(jitter=np.zeros((n, 2)), scale=np.ones(n), rot=np.zeros(n))


def sample_draws(cfg, seed, epoch, index, train, patch):
    """All random numbers of ONE sample, from ``default_rng((seed, epoch, index))`` in this fixed order: 1-2 centre jitter U(-1,1)^2,
    3 scale U(0,1), 4 rotation gate U(0,1), 5 rotation U(-1,1), 6 RGB-shift gate, 7-9 dr dg db U(shift_limit), 10 colour-jitter gate,
    11 brightness, 12 saturation, 13 erasing gate, 14-15 the two words of the Philox key, then per rectangle and attempt area,
    log-aspect and -- when the rectangle fits -- top, left.  Draws 1-15 are always taken, whatever the gates say, so the position of each
    in the stream is fixed.  Evaluation (``train`` False) draws nothing: zeros, 1 and 0, no colour change, no erasing.  ``jitter_gate``
    tells whether draw 10 fired: the contrast and hue of vpho_amd/photo.py (a second generator, its own order) ride under that gate."""
    out = dict(jitter=np.zeros(2), scale=1.0, rot=0.0, colour=np.array([0, 0, 0, 1, 1], np.float32), erase=np.zeros((MAX_ERASE, 4), np.int32),
               key=np.zeros(2, np.uint32), jitter_gate=False)
    if not train:
        return out
    r = np.random.default_rng((int(seed), int(epoch), int(index)))
    out['jitter'] = cfg.center_jittering * r.uniform(-1, 1, 2)
    out['scale'] = cfg.scale_factor * r.uniform(0, 1) + 1
    gate, rot = r.uniform(0, 1), r.uniform(-1, 1)
    out['rot'] = rot * cfg.max_rot / 180 * np.pi if gate < cfg.rot_prob else 0.0
    gate, d = r.uniform(0, 1), r.uniform(cfg.shift_limit[0], cfg.shift_limit[1], 3)
    if gate < cfg.RGB_shift_prob:
        out['colour'][:3] = np.rint(d)
    gate, b, s = r.uniform(0, 1), r.uniform(*cfg.brightness), r.uniform(*cfg.saturation)
    if gate < cfg.color_jitter_prob:
        out['colour'][3:] = (b, s)
        out['jitter_gate'] = True
    gate = r.uniform(0, 1)
    out['key'] = r.integers(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
    count = int(cfg.random_erasing_max_count)
    if count > MAX_ERASE:
        raise ValueError(f'--random_erasing_max_count {count}: the kernel takes at most {MAX_ERASE} rectangles per image')
    if gate < cfg.random_erasing_prob:
        # timm RandomErasing._erase: min_count == max_count == count; each rectangle aims at area / count
        lo, hi = math.log(0.3), math.log(1 / 0.3)
        for k in range(count):
            for _ in range(10):
                target = r.uniform(cfg.random_erasing_min_area, cfg.random_erasing_max_area) * patch * patch / count
                aspect = math.exp(r.uniform(lo, hi))
                h, w = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
                if w < patch and h < patch:
                    top, left = int(r.integers(0, patch - h + 1)), int(r.integers(0, patch - w + 1))
                    out['erase'][k] = (left, top, left + w, top + h)
                    break
    return out


# ------------------------------------------------------------------------------------------------------------------ crop plan
def _crop_matrices(jt2d, obj2d, K, jitter, scale_factor, rot, patch, bbox_scale_factor):
    """BaseDataset.get_augmentation_rotmat (base.py:522-574), operation for operation, over a batch"""
    bh, _ = rect_bbox2d(expand_bbox2d(pt2d_to_bbox2d(jt2d)))
    bo, _ = rect_bbox2d(expand_bbox2d(pt2d_to_bbox2d(obj2d)))
    center = np.concatenate([bh, bo], -1).reshape(-1, 4, 2).mean(1)
    c, s = np.cos(rot), np.sin(rot)
    z, o = np.zeros_like(c), np.ones_like(c)
    R3 = np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)
    allp = np.concatenate([jt2d, obj2d], 1)
    radius = np.linalg.norm(allp - center[:, None], axis=-1).max(-1)
    center = center + jitter * radius[:, None]
    radius = radius * bbox_scale_factor * scale_factor
    scale = patch / (radius * 2)
    R2T = np.swapaxes(R3[:, :2, :2], -1, -2)
    half = np.array([patch // 2, patch // 2]) + .5
    t = half - np.einsum('ni,nij->nj', center, R2T) * scale[:, None]
    St = np.zeros_like(R3)
    St[:, 0, 0] = St[:, 1, 1] = scale
    St[:, 2, 2] = 1
    St[:, :2, 2] = t
    M = St @ R3
    t_ = half - np.einsum('ni,nij->nj', center - K[:, :2, 2], R2T) * scale[:, None]
    Kc = K.copy()
    Kc[:, :2] *= scale[:, None, None]
    Kc[:, :2, 2] = t_
    return R3, M, Kc


def crop_plan(jt2d, obj_kpt2d, cam_intr, draws, patch, bbox_scale_factor, is_right=None):
    """The crop of every sample of a batch (base.py:522-574 and the fit loop of dexycb6.py:340-363) in numpy float64.

    jt2d (n,21,2), obj_kpt2d (n,27,2), cam_intr (n,3,3); draws: dict with jitter (n,2), scale (n), rot (n) (``eval_draws`` or stacked
    ``sample_draws``).  While the squared hand box (expansion 1.15) or the squared object box (1.10) of the transformed points fails
    check_bbox2d against the patch, the sample's scale factor is multiplied by 1.01; after 99 tries ValueError names the sample.
    ``is_right`` (n) bool mirrors the 2-D keys of left hands as dexycb6.py:398-420 does (x -> patch - x, box x swapped and mirrored,
    cam_intr_crop_flip[0,2] = patch - cx).  Returns a dict of arrays: rotmat_3d, rotmat_2d, minv (n,6: rows 0-1 of the inverse of
    rotmat_2d), cam_intr_crop, cam_intr_crop_flip, gt_jt2d, gt_obj2d, bbox_hand, bbox_obj, bbox_hand_rect, bbox_obj_rect, scale_factor
    (as it ended) and tries (multiplications taken)."""
    jt2d, obj2d, K = (np.asarray(a, np.float64) for a in (jt2d, obj_kpt2d, cam_intr))
    n = jt2d.shape[0]
    for name, a in (('jt2d', jt2d), ('obj_kpt2d', obj2d)):
        bad = ~np.isfinite(a).reshape(n, -1).all(1)
        if bad.any():
            raise ValueError(f'crop_plan: sample {int(np.flatnonzero(bad)[0])} has a non-finite point in {name}')
    jitter, sf, rot = np.asarray(draws['jitter'], np.float64).reshape(n, 2), np.array(draws['scale'], np.float64).reshape(n).copy(), \
        np.asarray(draws['rot'], np.float64).reshape(n)
    keys = ('rotmat_3d', 'rotmat_2d', 'cam_intr_crop', 'gt_jt2d', 'gt_obj2d', 'bbox_hand', 'bbox_obj', 'bbox_hand_rect', 'bbox_obj_rect')
    out = {k: None for k in keys}
    tries = np.zeros(n, np.int64)
    todo = np.arange(n)
    for attempt in range(FIT_TRIES):
        R3, M, Kc = _crop_matrices(jt2d[todo], obj2d[todo], K[todo], jitter[todo], sf[todo], rot[todo], patch, bbox_scale_factor)
        A, b = np.swapaxes(M[:, :2, :2], -1, -2), M[:, None, :2, 2]
        j2, o2 = jt2d[todo] @ A + b, obj2d[todo] @ A + b
        bh, bo = expand_bbox2d(pt2d_to_bbox2d(j2), 1.15), expand_bbox2d(pt2d_to_bbox2d(o2), 1.10)
        bhr, bor = rect_bbox2d(bh)[0], rect_bbox2d(bo)[0]
        ok = check_bbox2d(bhr, patch) & check_bbox2d(bor, patch)
        for k, v in zip(keys, (R3, M, Kc, j2, o2, bh, bo, bhr, bor)):
            if out[k] is None:
                out[k] = np.zeros((n,) + v.shape[1:])
            out[k][todo[ok]] = v[ok]
        sf[todo[~ok]] *= 1.01
        tries[todo[~ok]] += 1
        todo = todo[~ok]
        if todo.size == 0:
            break
    if todo.size:
        raise ValueError(f'index {int(todo[0])} bbox out of image')                 # dexycb6.py:361-362
    det = out['rotmat_2d'][:, 0, 0] * out['rotmat_2d'][:, 1, 1] - out['rotmat_2d'][:, 0, 1] * out['rotmat_2d'][:, 1, 0]
    if not (np.isfinite(det) & (np.abs(det) > 0)).all():
        raise ValueError(f'crop_plan: sample {int(np.flatnonzero(~(np.isfinite(det) & (np.abs(det) > 0)))[0])} has a non-invertible crop matrix')
    out['minv'] = np.ascontiguousarray(np.linalg.inv(out['rotmat_2d'])[:, :2, :].reshape(n, 6))
    out['cam_intr_crop_flip'] = out['cam_intr_crop'].copy()
    if is_right is not None:
        left = ~np.asarray(is_right, bool).reshape(n)
        for k in ('gt_jt2d', 'gt_obj2d'):
            out[k][left, :, 0] = patch - out[k][left, :, 0]
        for k in ('bbox_hand', 'bbox_obj', 'bbox_hand_rect', 'bbox_obj_rect'):
            b = out[k]
            b[left, 0], b[left, 2] = patch - b[left, 2], patch - b[left, 0]
        out['cam_intr_crop_flip'][left, 0, 2] = patch - out['cam_intr_crop_flip'][left, 0, 2]
    out['scale_factor'], out['tries'] = sf, tries
    return out


# ------------------------------------------------------------------------------------------------------------------ rigid 3-D labels
def aa_to_matrix(aa):
    """(...,3) axis-angle -> (...,3,3), Rodrigues in the dtype of ``aa``"""
    th = aa.norm(dim=-1, keepdim=True)
    small = th < 1e-8
    k = aa / torch.where(small, torch.ones_like(th), th)
    x, y, z = k.unbind(-1)
    o = torch.zeros_like(x)
    Kx = torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(aa.shape[:-1] + (3, 3))
    s, c = torch.sin(th)[..., None], torch.cos(th)[..., None]
    eye = torch.eye(3, dtype=aa.dtype, device=aa.device).expand(Kx.shape)
    return eye + s * Kx + (1 - c) * (Kx @ Kx)


def matrix_to_aa(R):
    """(...,3,3) -> (...,3) axis-angle with angle in [0, pi], through the best-conditioned quaternion candidate"""
    m = R.reshape(-1, 9)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(-1)
    q2 = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1).clamp_min(0)
    cand = torch.stack([torch.stack([q2[:, 0], m21 - m12, m02 - m20, m10 - m01], -1),
                        torch.stack([m21 - m12, q2[:, 1], m10 + m01, m02 + m20], -1),
                        torch.stack([m02 - m20, m10 + m01, q2[:, 2], m12 + m21], -1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q2[:, 3]], -1)], 1)
    best = q2.argmax(-1)
    q = cand[torch.arange(m.shape[0]), best] / (2 * q2.gather(1, best[:, None]).sqrt())
    q = torch.where(q[:, :1] < 0, -q, q)
    vn = q[:, 1:].norm(dim=-1, keepdim=True)
    ang = 2 * torch.atan2(vn, q[:, :1])
    k = torch.where(vn < 1e-12, 2 * torch.ones_like(vn), ang / vn.clamp_min(1e-300))
    return (q[:, 1:] * k).reshape(R.shape[:-2] + (3,))


def rigid_labels(rec, rot, assets):
    """The 3-D labels of dexycb6.py:368-469 that are a rigid motion of the annotations, torch float64 on the host.  ``rec``: dict of stacked
    arrays (joint_3d, mano_pose, mano_betas, is_right, obj_id, obj_rt, optional hand_vert, gravity), ``rot`` (n) the crop's rotation.
    root_joint_flip is the flipped ANNOTATED root (the reference takes it from a MANO evaluation that was translated onto it)."""
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    rot = t64(rot)
    n = rot.shape[0]
    Rz = aa_to_matrix(torch.stack([torch.zeros_like(rot), torch.zeros_like(rot), rot], -1))
    right = torch.as_tensor(np.asarray(rec['is_right'], bool).reshape(n))
    sign = torch.where(right, 1.0, -1.0).double()[:, None]
    out = {}
    jt = t64(rec['joint_3d']) @ Rz.transpose(1, 2)
    root = jt[:, 0]
    out['gt_joint'], out['root_joint'] = jt, root

    def flipped(p):                                     # x negated for left hands, relative to the flipped root
        f = p.clone()
        f[..., 0] = f[..., 0] * sign
        return f
    jf = flipped(jt)
    out['root_joint_flip'] = jf[:, 0].clone()
    out['gt_hand_jt3d_flip'] = jf - jf[:, :1]
    if rec.get('hand_vert') is not None:
        hv = t64(rec['hand_vert']) @ Rz.transpose(1, 2)
        out['gt_hand_vert'] = hv
        out['gt_hand_vert_flip'] = flipped(hv) - jf[:, :1]
    rt = t64(rec['obj_rt'])
    Ro, to = Rz @ rt[:, :, :3], (Rz @ rt[:, :, 3:])[..., 0]
    out['gt_obj_rt'] = torch.cat([Ro, to[..., None]], -1)
    out['gt_obj'] = torch.cat([Ro[:, :2, :].reshape(n, 6), to - root], -1)            # matrix_to_rotation_6d: the first two rows
    com = np.stack([np.asarray(assets['ycb'][YCB_NAMES[int(i)]]['CoM'], np.float64) for i in np.asarray(rec['obj_id']).reshape(n)])
    out['obj_CoM'] = ((Ro @ t64(com)[..., None])[..., 0] + to - root)[:, None]
    g = t64(rec['gravity']) if rec.get('gravity') is not None else torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).expand(n, 3)
    out['gravity'] = (Rz @ g[..., None])[..., 0][:, None]
    pose = t64(rec['mano_pose']).reshape(n, 16, 3).clone()
    pose[:, 0] = matrix_to_aa(Rz @ aa_to_matrix(pose[:, 0]))
    pose[:, :, 1:] = pose[:, :, 1:] * sign[:, None]
    out['gt_mano'] = torch.cat([pose.reshape(n, 48), t64(rec['mano_betas'])], -1)
    return out


# ------------------------------------------------------------------------------------------------------------------ heat-map tables
def gauss_table(sigma):
    """HeatmapGenerator.__init__ (misc_fn.py:291-295): the reference's numpy expression; returns (g fp32 as its fp32 maps store it,
    g.min() of the float64 table)"""
    size = 6 * sigma + 3
    x = np.arange(0, size, 1, float)
    y = x[:, np.newaxis]
    x0, y0 = 3 * sigma + 1, 3 * sigma + 1
    g = np.exp(- ((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma ** 2))
    return g.astype(np.float32), float(g.min())


def adaptive_res(bbox, size):
    """AdaptiveHeatmapGenerator.__call__ (misc_fn.py:373-375): (n,4) boxes -> (res (n,2) int32, wh (n,2)); a res component < 1 raises"""
    bbox = np.asarray(bbox, np.float64)
    wh = bbox[:, 2:] - bbox[:, :2]
    if not (np.isfinite(wh).all() and (wh > 0).all()):
        raise ValueError(f'heat-map box {int(np.flatnonzero(~(np.isfinite(wh) & (wh > 0)).all(1))[0])} is degenerate: {bbox}')
    max_l = wh.max(1)
    res = np.stack([np.trunc(size * wh[:, 0] / max_l), np.trunc(size * wh[:, 1] / max_l)], -1).astype(np.int32)
    if (res < 1).any():
        raise ValueError(f'heat-map box {int(np.flatnonzero((res < 1).any(1))[0])} is degenerate: a tight map of {res[(res < 1).any(1)][0]} cells')
    return res, wh


# ------------------------------------------------------------------------------------------------------------------ pipeline
def photo_can_fire(cfg):
    """True when a flag lets CLAHE, contrast, hue or one of the two blurs fire (vpho_amd/photo.py, csrc/photo.hip): the training crop
    then takes the ``ops.photo_*`` launches for the whole batch.  With the default flags it is False and photo.py is never imported."""
    g = lambda k, d: getattr(cfg, k, d)
    return bool(g('clahe_p', 0) > 0 or tuple(g('jitter_contrast', (1, 1))) != (1, 1) or tuple(g('jitter_hue', (0, 0))) != (0, 0) or g('blur_p', 0) > 0
                or g('motion_blur_p', 0) > 0)


def _stack_records(records):
    if isinstance(records, dict):
        return records
    keys = [k for k in records[0] if all(k in r and r[k] is not None for r in records)]
    return {k: np.stack([np.asarray(r[k]) for r in records]) for k in keys}


class FramePipeline:
    """``FramePipeline(cfg, assets, device, train, seed)``; ``pipe(frames_u8, records, epoch=0)`` -> the Appendix-A batch dict on the device.

    frames_u8: (n,H,W,3) uint8 tensor (pinned host memory or already on the device); records: list of record dicts (module docstring) or
    a dict of stacked arrays.  Everything runs on the current stream: the host does the crop plan and the rigid labels, the device the
    crops (``ops.frame_patch``; in training with ``--clahe_p``, ``--jitter_contrast``, ``--jitter_hue``, ``--blur_p`` or ``--motion_blur_p``
    able to fire, the ``ops.photo_*`` launches of vpho_amd/photo.py for the whole batch), the adaptive hand maps on ``bbox_hand`` and the square object maps on ``bbox_obj_rect`` with is_right
    (``ops.heatmap_targets``; dexycb6.py:435-437)."""
    def __init__(self, cfg, assets, device, train=False, seed=0):
        from . import ops                               # the HIP library: a missing kernel is an error, there is no host path
        self.ops, self.cfg, self.assets, self.device, self.train, self.seed = ops, cfg, assets, torch.device(device), bool(train), int(seed)
        self.patch, self.size = int(cfg.patch_size), int(cfg.heatmap_size)
        self.tables = {}
        for who in ('hand', 'obj'):
            sigma = float(getattr(cfg, f'heatmap_{who}_sigma'))
            g, gmin = gauss_table(sigma)
            self.tables[who] = (torch.from_numpy(g).to(self.device), sigma, gmin)
        self.photo = None
        if self.train and photo_can_fire(cfg):          # CLAHE, contrast, hue, blurs: the training crop goes through ops.photo_*
            from . import photo
            if cfg.clahe_p > 0 and self.patch % photo.TILES:
                raise ValueError(f'--clahe_p {cfg.clahe_p}: the {photo.TILES} x {photo.TILES} tile grid needs a patch size that is a multiple of {photo.TILES}, '
                                 f'got {self.patch}')
            self.photo = photo
        self.labeler = None
        if getattr(cfg, 'frame_contact', False):        # --frame_contact: contact labels from the annotations, on the device
            from .physics_labels import PhysicsLabeler
            self.labeler = PhysicsLabeler(cfg, assets, self.device)

    def _dev(self, a, dtype=None):
        t = torch.as_tensor(np.ascontiguousarray(a))
        return (t if dtype is None else t.to(dtype)).to(self.device, non_blocking=True)

    def __call__(self, frames_u8, records, epoch=0):
        ops, cfg, P, S = self.ops, self.cfg, self.patch, self.size
        rec = _stack_records(records)
        n = int(np.asarray(rec['is_right']).shape[0])
        if tuple(frames_u8.shape[:1]) != (n,) or frames_u8.dtype != torch.uint8:
            raise ValueError(f'FramePipeline: {n} records with frames of shape {tuple(frames_u8.shape)} and dtype {frames_u8.dtype}')
        index = np.asarray(rec['index'] if 'index' in rec else np.arange(n)).reshape(n).astype(np.int64)
        right = np.asarray(rec['is_right'], bool).reshape(n)
        K = np.asarray(rec['cam_intr'], np.float64)
        names = [YCB_NAMES[int(i)] for i in np.asarray(rec['obj_id']).reshape(n)]
        rt = np.asarray(rec['obj_rt'], np.float64)
        kpt3d = np.stack([np.asarray(self.assets['ycb'][nm]['kpt3d'], np.float64) for nm in names]) @ np.swapaxes(rt[:, :, :3], -1, -2) + rt[:, None, :, 3]
        obj2d = project(kpt3d, K)
        per = [sample_draws(cfg, self.seed, epoch, i, self.train, P) for i in index]
        draws = {k: np.stack([np.asarray(d[k]) for d in per]) for k in per[0]}
        plan = crop_plan(rec['jt2d'], obj2d, K, draws, P, float(cfg.bbox_scale_factor), is_right=right)
        res, wh = adaptive_res(plan['bbox_hand'], S)
        labels = rigid_labels(rec, draws['rot'], self.assets)
        frames = frames_u8.to(self.device, non_blocking=True).contiguous()
        flip = self._dev((~right).astype(np.uint8))
        erase = key = colour = None
        if self.train:
            colour = self._dev(draws['colour'].astype(np.float32))
            if (draws['erase'][:, :, 2] > draws['erase'][:, :, 0]).any():
                erase, key = self._dev(draws['erase'].astype(np.int32)), self._dev(draws['key'].astype(np.uint32).view(np.int32))
        if self.photo is not None:
            pd = [self.photo.photo_draws(cfg, self.seed, epoch, i, bool(d['jitter_gate'])) for i, d in zip(index, per)]
            params = {k: np.stack([np.asarray(d[k]) for d in pd]) for k in pd[0]}
            out = {'rgb': self.photo.photo_patch(ops, frames, self._dev(plan['minv']), P, colour, params, flip=flip, erase=erase, key=key)}
        else:
            out = {'rgb': ops.frame_patch(frames, self._dev(plan['minv']), P, colour=colour, flip=flip, erase=erase, key=key)}
        g, sigma, gmin = self.tables['hand']
        out['hm_hand'] = ops.heatmap_targets(self._dev(plan['gt_jt2d']), self._dev(np.concatenate([plan['bbox_hand'][:, :2], wh], -1)), g, sigma, gmin, S,
                                             res=self._dev(res))
        g, sigma, gmin = self.tables['obj']
        bor = plan['bbox_obj_rect']
        mw = (bor[:, 2:] - bor[:, :2]).max(1)
        out['hm_obj'] = ops.heatmap_targets(self._dev(plan['gt_obj2d']), self._dev(np.concatenate([bor[:, :2], mw[:, None], mw[:, None]], -1)), g, sigma,
                                            gmin, S, left=flip)
        f32 = lambda a: self._dev(a, torch.float32)
        for k in ('bbox_hand', 'bbox_obj', 'bbox_hand_rect', 'bbox_obj_rect', 'gt_jt2d', 'gt_obj2d', 'cam_intr_crop', 'cam_intr_crop_flip'):
            out[k] = f32(plan[k])
        out['cam_intr'] = f32(K)
        for k, v in labels.items():
            out[k] = v.float().to(self.device, non_blocking=True)
        out['is_right'] = self._dev(right)
        out['is_ho3d'] = torch.zeros(n, dtype=torch.bool, device=self.device)
        # the engine's physics stage reads is_grasped: a record without it counts as grasped
        out['is_grasped'] = self._dev(np.asarray(rec['is_grasped'], bool).reshape(n) if 'is_grasped' in rec else np.ones(n, bool))
        if 'force_local' in rec:
            out['force_local'] = f32(rec['force_local'])
        out['obj_name'], out['obj_id'] = names, self._dev(np.asarray(rec['obj_id']).reshape(n).astype(np.int64))
        out['index'] = torch.from_numpy(index)
        if self.labeler is not None:
            # get_hand_contact .. check_is_grasped (dexycb6.py:320-332) on the labels as they stand after the augmentation: the in-plane
            # rotation moves hand and object alike.  A record's own is_grasped is not used then.
            lab = self.labeler(out)
            out['hand_contact'], out['force_contact'], out['is_grasped'] = lab['hand_contact'], lab['force_contact'], lab['is_grasped']
        return out


class FrameLoader:
    """Iterable of device batch dicts for ``Trainer.fit / run / eval / infer``: ``FrameLoader(source, batch_size, pipeline, shuffle, drop_last)``.

    Frames are gathered into pinned host memory in this process; the copy and the two launches of batch k + 1 run on a side stream while
    batch k is consumed (one batch ahead).  The consumer's stream waits on the batch's event and every tensor is handed over with
    ``record_stream``.  Every pass over the loader is one epoch (``set_epoch`` for a resumed run): the shuffle is seeded by
    (pipeline.seed, epoch) and the augmentation by (pipeline.seed, epoch, index)."""
    def __init__(self, source, batch_size, pipeline, shuffle=False, drop_last=False):
        self.source, self.batch_size, self.pipeline, self.shuffle, self.drop_last = source, int(batch_size), pipeline, bool(shuffle), bool(drop_last)
        if self.batch_size < 1:
            raise ValueError(f'FrameLoader: batch_size {batch_size}')
        self.epoch = 0
        self._pinned = [None, None]

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        n = len(self.source)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _order(self, epoch):
        n = len(self.source)
        order = np.random.default_rng((self.pipeline.seed, int(epoch))).permutation(n) if self.shuffle else np.arange(n)
        return [order[i * self.batch_size:(i + 1) * self.batch_size] for i in range(len(self))]

    def _stage(self, slot, ids, epoch, side):
        items = [self.source[int(i)] for i in ids]
        shape = (len(items),) + tuple(items[0][0].shape)
        if any(f.shape != items[0][0].shape or f.dtype != np.uint8 for f, _ in items) or len(shape) != 4 or shape[3] != 3:
            raise ValueError('FrameLoader: the frames of one batch must be uint8 (H, W, 3) arrays of one size')
        buf, ev = self._pinned[slot] or (None, None)
        if ev is not None:
            ev.synchronize()                             # the copy that last read this pinned buffer is done
        if buf is None or buf.shape[0] < shape[0] or tuple(buf.shape[1:]) != shape[1:]:
            buf = torch.empty((self.batch_size,) + shape[1:], dtype=torch.uint8).pin_memory()
        host = buf[:shape[0]]
        for k, (f, _) in enumerate(items):
            host[k] = torch.from_numpy(np.ascontiguousarray(f))
        records = [dict(r, index=r.get('index', int(i))) for (_, r), i in zip(items, ids)]
        with torch.cuda.stream(side):
            batch = self.pipeline(host, records, epoch=epoch)
            ev = torch.cuda.Event()
            ev.record(side)
        self._pinned[slot] = (buf, ev)
        return batch, ev

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        side = torch.cuda.Stream(device=self.pipeline.device)
        ahead = None
        for k, ids in enumerate(self._order(epoch)):
            staged = self._stage(k % 2, ids, epoch, side)
            if ahead is not None:
                yield self._hand_over(*ahead)
            ahead = staged
        if ahead is not None:
            yield self._hand_over(*ahead)

    def _hand_over(self, batch, ev):
        cur = torch.cuda.current_stream(self.pipeline.device)
        cur.wait_event(ev)
        for v in batch.values():
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(cur)
        return batch


# ------------------------------------------------------------------------------------------------------------------ sources
class synthetic_frames:
    """``synthetic_frames(n, assets, seed, size=(640, 480))``: a source of n textured frames of ``size`` (width, height).  The 2-D points come
    from projecting a rigidly posed MANO template (random global rotation, zero finger pose and shape) and a posed object, so the crop
    geometry is not trivial; about a third of the hands are left ones.  Records carry every optional key."""
    def __init__(self, n, assets, seed=0, size=(640, 480)):
        self.n, self.assets, self.seed, self.size = int(n), assets, int(seed), (int(size[0]), int(size[1]))
        self.v = np.asarray(assets['mano']['v_template'], np.float64)
        self.v2j = np.asarray(assets['anchor']['vert2joint'], np.float64)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        W, H = self.size
        r = np.random.default_rng((self.seed, 7, int(i)))
        foc = r.uniform(0.85, 1.1) * W
        K = np.array([[foc, 0, W / 2 + r.uniform(-8, 8)], [0, foc, H / 2 + r.uniform(-8, 8)], [0, 0, 1]])
        aa = r.normal(size=3)
        aa *= r.uniform(0, 1.2) / np.linalg.norm(aa)
        R = aa_to_matrix(torch.from_numpy(aa)).numpy()
        root = np.array([r.uniform(-0.08, 0.08), r.uniform(-0.05, 0.05), r.uniform(0.65, 0.9)])
        verts = self.v @ R.T
        joints = self.v2j @ verts
        shift = root - joints[0]
        verts, joints = verts + shift, joints + shift
        oid = int(r.integers(0, len(YCB_NAMES)))
        q = r.normal(size=3)
        q *= r.uniform(0, np.pi) / np.linalg.norm(q)
        Ro = aa_to_matrix(torch.from_numpy(q)).numpy()
        to = joints.mean(0) + r.normal(0, 0.02, 3)
        g = r.normal(size=3)
        rec = dict(jt2d=project(joints, K), joint_3d=joints, mano_pose=np.concatenate([aa, np.zeros(45)]), mano_betas=np.zeros(10),
                   is_right=bool(r.random() < 0.67), obj_id=oid, obj_rt=np.concatenate([Ro, to[:, None]], 1), cam_intr=K, hand_vert=verts,
                   gravity=g / np.linalg.norm(g), force_local=r.normal(0, 0.1, (32, 3)), is_grasped=bool(r.random() < 0.8), index=int(i))
        ph = r.uniform(0, 2 * np.pi, (3, 2))
        frame = np.stack([128 + 70 * np.outer(np.cos(np.arange(H) / r.uniform(9, 40) + ph[c, 1]), np.sin(np.arange(W) / r.uniform(9, 40) + ph[c, 0]))
                          for c in range(3)], -1)
        frame = np.clip(np.rint(frame) + r.integers(-24, 25, frame.shape, dtype=np.int16), 0, 255).astype(np.uint8)
        return frame, rec


RECORD_KEYS = ('jt2d', 'joint_3d', 'mano_pose', 'mano_betas', 'is_right', 'obj_id', 'obj_rt', 'cam_intr')
OPTIONAL_KEYS = ('hand_vert', 'gravity', 'force_local', 'is_grasped')
LABEL_FILE = 'physics_labels.npz'                        # beside annotations.npz, one row per frame
LABEL_KEYS = ('is_grasped', 'force_local', 'force_contact')


class FrameDirectory:
    """A source read from a directory: ``annotations.npz`` with the stacked arrays ``image`` (file names relative to the directory),
    jt2d, joint_3d, mano_pose (48), mano_betas, is_right, obj_id, obj_rt, cam_intr and optionally hand_vert, gravity, force_local,
    is_grasped.  A frame is a ``.npy`` (H,W,3) uint8 array, or an image file read with PIL when PIL can be imported.  When the directory
    also holds ``physics_labels.npz`` (force_optim.py --frame_source DIR), is_grasped and force_local are read from it and the records
    carry force_contact too; a file with another number of rows raises ValueError."""
    def __init__(self, path):
        self.path = str(path)
        ann = os.path.join(self.path, 'annotations.npz')
        if not os.path.exists(ann):
            raise FileNotFoundError(f'FrameDirectory: {ann} is missing')
        with np.load(ann, allow_pickle=False) as z:
            self.a = {k: z[k] for k in z.files}
        missing = [k for k in ('image',) + RECORD_KEYS if k not in self.a]
        if missing:
            raise KeyError(f'FrameDirectory: {ann} lacks {missing}')
        n = len(self.a['image'])
        bad = [k for k, v in self.a.items() if len(v) != n]
        if bad:
            raise ValueError(f'FrameDirectory: {bad} do not have the {n} rows of image')
        # physics_labels.npz (force_optim.py --frame_source DIR): is_grasped and force_local come from it, force_contact rides along
        self.labels = None
        side = os.path.join(self.path, LABEL_FILE)
        if os.path.exists(side):
            with np.load(side, allow_pickle=False) as z:
                self.labels = {k: z[k] for k in LABEL_KEYS}
            bad = [k for k, v in self.labels.items() if len(v) != n]
            if bad:
                raise ValueError(f'FrameDirectory: {side} has {len(self.labels[bad[0]])} rows of {bad[0]}, annotations.npz has {n} frames')

    def __len__(self):
        return len(self.a['image'])

    def __getitem__(self, i):
        name = os.path.join(self.path, str(self.a['image'][i]))
        if name.endswith('.npy'):
            frame = np.load(name, allow_pickle=False)
        else:
            try:
                from PIL import Image
            except ImportError as e:
                raise ImportError(f'FrameDirectory: {name} is an image file and PIL is not importable; store the frame as a .npy uint8 array') from e
            frame = np.asarray(Image.open(name).convert('RGB'))
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError(f'FrameDirectory: {name} holds {frame.dtype} {frame.shape}, expected uint8 (H, W, 3)')
        rec = {k: self.a[k][i] for k in RECORD_KEYS + OPTIONAL_KEYS if k in self.a}
        if self.labels is not None:
            rec.update({k: self.labels[k][i] for k in LABEL_KEYS})
        rec['index'] = int(i)
        return frame, rec


def write_frame_directory(path, source):
    """write a source in FrameDirectory's layout (frames as .npy)"""
    os.makedirs(path, exist_ok=True)
    rows, images = [], []
    for i in range(len(source)):
        frame, rec = source[i]
        images.append(f'{i:08d}.npy')
        np.save(os.path.join(path, images[-1]), frame)
        rows.append(rec)
    keys = [k for k in RECORD_KEYS + OPTIONAL_KEYS if all(k in r for r in rows)]
    np.savez(os.path.join(path, 'annotations.npz'), image=np.array(images), **{k: np.stack([np.asarray(r[k]) for r in rows]) for k in keys})


def make_loader(cfg, assets, device, train):
    """the loader of ``main.py --frame_source synthetic|DIR``: cfg.num_batches batches of synthetic frames, or the directory as it is"""
    bs = int(cfg.batch_size if train else cfg.eval_batch_size)
    if cfg.frame_source == 'synthetic':
        source = synthetic_frames(bs * int(cfg.num_batches), assets, seed=int(cfg.random_seed))
    else:
        source = FrameDirectory(cfg.frame_source)
    pipe = FramePipeline(cfg, assets, device, train=train, seed=int(cfg.random_seed))
    loader = FrameLoader(source, bs, pipe, shuffle=train, drop_last=train)
    loader.set_epoch(resume_epoch(cfg) if train else 0)
    return loader


def resume_epoch(cfg):
    """the epoch a resumed ``Trainer.fit`` starts at (``--checkpoint .../epoch_N.state`` with an optimiser in it), else 0: the loader of a
    resumed run must draw the order and the augmentations of epoch N, not of epoch 0"""
    from . import checkpoint as CK
    return CK.epoch_of(cfg.checkpoint) if CK.is_training_state(cfg.checkpoint) else 0

"""Restatement of the reference's ablation aggregators (lib/model/aggregation.py, HandAggregator :82-113,286-467, ObjectAggregator
:646-659,1001-1112) on the oracle's building blocks, in the dtype of its inputs: float64 is the yardstick of
tests/test_gpu_aggmodes.py, float32 repeats the reference's own arithmetic.  TEST INFRASTRUCTURE (like tests/_penetration_fp64.py).

Top-k ties are broken as everywhere in this project (larger value first, then the smaller index); the fixture's seed keeps every
compared gap far from a tie."""
import torch

from oracle import aggregation as OA
from oracle import rotations as R
from oracle.mano import get_hand_verts

HAND_MODES = ('heatmap', '2D_pt_pose', '2D_pt_joint', 'average_all', 'random')
OBJ_MODES = ('heatmap', '2D_pt_pose', 'average_all', 'random')


def decode_heatmap(u8):
    """the fixture stores its heat maps as 8-bit levels; value = level / 255 (exact in fp32)"""
    return torch.as_tensor(u8).float() / 255


def heatmap_peak(heatmap, dtype=None):
    """aggregation.py:313-323 with its transposition: torch.meshgrid(X, Y) in `ij` order flattened against the row-major map, so the
    value used as x is X[ind // W] and y is Y[ind % W].  -> peak (bs,J,2), flat arg-max index (bs,J)"""
    bs, J, H, W = heatmap.shape
    assert H == W, 'only defined for square maps'
    dtype = heatmap.dtype if dtype is None else dtype
    ind = torch.argmax(heatmap.reshape(bs, J, -1), dim=-1)
    X = torch.arange(W).to(dtype) / (W - 1) * 2 - 1
    Y = torch.arange(H).to(dtype) / (H - 1) * 2 - 1
    return torch.stack([X[ind // H], Y[ind % H]], dim=-1), ind


def _fuse_whole_pose(pose, idx, weight):
    """pose (bs,S,48), idx (bs,n) -> (bs,48): average_quaternion of all 16 rotations over the listed candidates"""
    bs, n = idx.shape
    sel = torch.gather(pose, 1, idx[:, :, None].expand(bs, n, 48)).reshape(bs, n, 16, 3)
    q = R.axis_angle_to_quaternion(sel).permute(0, 2, 1, 3)                              # (bs,16,n,4)
    w = None if weight is None else weight[:, None].expand(bs, 16, n)
    return R.quaternion_to_axis_angle(OA.average_quaternion(q, w)).reshape(bs, 48)


def hand_mode(mano, mode, pose, betas, root_flip, K, heatmap, bbox, k, is_weight=True):
    """pose (bs,S,48), betas (bs,10) (one shape row per image), K (bs,3,3).  -> dict: score, topk, val, peak (where the mode has them),
    pose48 (None for 2D_pt_joint), mano (bs,58), vert, joint"""
    bs, S = pose.shape[:2]
    out = {}
    if mode in ('heatmap', '2D_pt_pose', '2D_pt_joint'):
        _, joint = get_hand_verts(mano, pose.reshape(-1, 48), betas[:, None].expand(bs, S, 10).reshape(-1, 10))
        joint = joint.reshape(bs, S, 21, 3)
        pt2d = OA._norm_to_bbox(OA.project(joint + root_flip[:, None, None], K), bbox)   # (bs,S,21,2)
    if mode == 'heatmap':
        score = OA._bicubic_lookup(heatmap, pt2d, list(range(21))).sum(-1)
        val, idx = OA.topk_stable(score, k, dim=1)
        w = (val + 1e-8) / (val.sum(dim=1, keepdim=True) + 1e-8)
        pose48 = _fuse_whole_pose(pose, idx, w if is_weight else None)
        out.update(score=score, topk=idx, val=val)
    elif mode in ('2D_pt_pose', '2D_pt_joint'):
        peak, ind = heatmap_peak(heatmap)
        score = -torch.norm(pt2d - peak[:, None], dim=-1)                                # (bs,S,21)
        out.update(peak=peak, peak_index=ind)
        if mode == '2D_pt_pose':
            score = score.sum(-1)
            val, idx = OA.topk_stable(score, k, dim=1)
            pose48 = _fuse_whole_pose(pose, idx, None)
            out.update(score=score, topk=idx, val=val)
        else:
            val, idx = OA.topk_stable(score, k, dim=1)                                   # (bs,k,21)
            sel = torch.gather(joint, 1, idx[..., None].expand(bs, k, 21, 3))
            out.update(score=score, topk=idx, val=val, pose48=None, mano=torch.zeros(bs, 58, dtype=pose.dtype),
                       vert=torch.zeros(bs, 778, 3, dtype=pose.dtype), joint=sel.mean(dim=1))
            return out
    elif mode == 'average_all':
        pose48 = _fuse_whole_pose(pose, torch.arange(S)[None].expand(bs, S), None)
    elif mode == 'random':
        pose48 = pose[:, 0].clone()
    else:
        raise ValueError(mode)
    vert, joint = get_hand_verts(mano, pose48, betas)
    out.update(pose48=pose48, mano=torch.cat([pose48, betas], -1), vert=vert, joint=joint)
    return out


def obj_scores_2d(ycb, pose6d, root, names, is_right, K, heatmap, bbox, dtype):
    """aggregation.py:1015-1039: minus the summed distance of the projected key-points to their maps' peaks"""
    p = pose6d.clone().to(dtype)
    p[..., 6:] = p[..., 6:] + root.to(dtype).unsqueeze(1)
    pt = OA.flip_x(OA.object_points(ycb, p, names, 'kpt3d'), is_right)
    pt2d = OA._norm_to_bbox(OA.project(pt, K.to(dtype)), bbox.to(dtype))
    peak, ind = heatmap_peak(heatmap, dtype)
    return -torch.norm(pt2d - peak[:, None], dim=-1).sum(-1), peak, ind


def obj_mode(ycb, mode, pose6d, root, names, is_right, K, heatmap, bbox, k, dtype=torch.float64):
    """pose6d (bs,S,9) in its own dtype (float64: the sampler's); the SCORES in ``dtype`` (the reference casts with .float(), :753).
    -> dict: score / topk / val / peak where the mode has them, fused (bs,9) in pose6d's dtype"""
    bs = pose6d.shape[0]
    out = {}
    if mode == 'heatmap':
        score = OA.obj_heat_scores(ycb, pose6d, root.to(dtype), names, is_right, K.to(dtype), heatmap.to(dtype), bbox.to(dtype), dtype=dtype)
    elif mode == '2D_pt_pose':
        score, out['peak'], out['peak_index'] = obj_scores_2d(ycb, pose6d, root, names, is_right, K, heatmap, bbox, dtype)
    elif mode == 'average_all':
        score, idx = None, torch.arange(k)[None].expand(bs, k)                           # the FIRST k candidates, not all S (:1069)
    elif mode == 'random':
        score, idx = None, torch.zeros(bs, 1, dtype=torch.long)
    else:
        raise ValueError(mode)
    if score is not None:
        val, idx = OA.topk_stable(score, k, dim=1)
        out.update(score=score, val=val)
    n = idx.shape[1]
    out.update(topk=idx, fused=OA.fuse_topk(pose6d, idx, torch.ones(bs, n, dtype=pose6d.dtype) / n))
    return out

"""Plain torch restatements of the sixteen aggregation-cascade kernels (csrc/aggregate.hip, csrc/aggregate_modes.hip), written from the
kernel comments and the reference lines they cite, independently of oracle/aggregation.py: the bicubic look-up is a direct 16-tap
cubic-convolution sum (A = -0.75, zeros padding, align_corners=False -- no grid_sample), the nearest vertex an explicit arg-min with the
rule "smaller squared distance, then smaller index", the rotation conversions are spelled out here.  TEST INFRASTRUCTURE ONLY: nothing
here imports ``vpho_amd.ops``.

As in tests/_leaf_fp64.py every function computes in the dtype of its tensor arguments: ``f(*to64(args))`` is the float64 reference,
``f(*args)`` torch's own float32 evaluation, from which ``bound`` derives the tolerance of the fp32 kernels.  The input generators live
here too, so that tests/test_cascade_fp64_cpu.py (which asserts their conditions) and tests/test_gpu_cascade_leaves.py see the same tensors."""
import math

import numpy as np
import torch

from tests._leaf_fp64 import SENT, ULP, bits_equal, bound, check, gen, ruled, to64  # noqa: F401  (re-exported for the two test files)

JOINT_LEVEL = {1: [1, 5, 9, 13, 17], 2: [2, 6, 10, 14, 18], 3: [3, 7, 11, 15, 19], 4: [4, 8, 12, 16, 20]}
LVL2_JOINT, LVL3_JOINT = [14, 2, 5, 11, 8], [15, 3, 6, 12, 9]                                     # MANO rotations of the T, I, M, R, P fingers
FINGER_ANCHOR = [[1, 2, 3, 4], [8, 9, 10, 11], [14, 15, 16, 17], [21, 22, 23, 24], [28, 29, 30, 31]]
H_MAP, W_MAP = 12, 20                                                                            # never square: an H / W swap must show


def observe_list(level):
    """the joints a cascade level scores: every joint of the deeper levels (20, 15, 10, 5); level -1: all 21"""
    return list(range(21)) if level < 0 else [j for l in range(level + 1, 5) for j in JOINT_LEVEL[l]]


def check_each(name, got, ref64, tol):
    """elementwise |got - ref64| <= tol (a tensor): every element is asserted, the one closest to its bound is printed through ``check``"""
    got, ref64, tol = got.detach().cpu().double().reshape(-1), ref64.double().reshape(-1), tol.double().reshape(-1)
    assert got.shape == ref64.shape == tol.shape, (name, got.shape, ref64.shape, tol.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref64).abs()
    i = int(torch.argmax(err / tol.clamp_min(1e-300)))
    check(name, got[i:i + 1], ref64[i:i + 1], float(tol[i]))
    bad = torch.nonzero(err > tol).reshape(-1)
    assert bad.numel() == 0, (name, bad[:8].tolist())


# ------------------------------------------------------------------------------------------------ rotations
def _unit(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def rot6d_to_matrix(d6):
    """Gram-Schmidt of the two 3-vectors; the matrix' ROWS are b1, b2, b1 x b2"""
    b1 = _unit(d6[..., :3])
    b2 = _unit(d6[..., 3:6] - (b1 * d6[..., 3:6]).sum(-1, keepdim=True) * b1)
    return torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], -2)


def axis_angle_to_quaternion(aa):
    ang = aa.norm(dim=-1, keepdim=True)
    small = ang.abs() < 1e-6
    s = torch.where(small, 0.5 - ang * ang / 48, torch.sin(ang * 0.5) / torch.where(small, torch.ones_like(ang), ang))
    return torch.cat([torch.cos(ang * 0.5), aa * s], -1)


def quaternion_to_axis_angle(q):
    n = q[..., 1:].norm(dim=-1, keepdim=True)
    half = torch.atan2(n, q[..., :1])
    ang = 2 * half
    small = ang.abs() < 1e-6
    s = torch.where(small, 0.5 - ang * ang / 48, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    return q[..., 1:] / s


def quaternion_to_matrix(q):
    r, i, j, k = q.unbind(-1)
    s = 2 / (q * q).sum(-1)
    m = torch.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                     s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                     s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def matrix_to_quaternion(m):
    """the best-conditioned of the four candidates (largest |component|), real part >= 0"""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.reshape(m.shape[:-2] + (9,)).unbind(-1)
    qa = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1).clamp_min(0).sqrt()
    cand = torch.stack([torch.stack([qa[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
                        torch.stack([m21 - m12, qa[..., 1] ** 2, m10 + m01, m02 + m20], -1),
                        torch.stack([m02 - m20, m10 + m01, qa[..., 2] ** 2, m12 + m21], -1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, qa[..., 3] ** 2], -1)], -2)
    cand = cand / (2 * qa.clamp_min(0.1))[..., None]
    best = qa.argmax(-1)
    q = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    return torch.where(q[..., :1] < 0, -q, q)


def _pos_real(q):
    """q if its real part is > 0, else -q (a real part of exactly 0 flips, as the kernels' ``q0 > 0 ? 1 : -1``)"""
    return torch.where(q[..., :1] > 0, q, -q)


def moment_matrix(Q, W, wsum=None):
    Q = _pos_real(Q)
    A = (Q[..., :, None] * Q[..., None, :] * W[..., None, None]).sum(-3)
    return A / (W.sum(-1) if wsum is None else wsum)[..., None, None]


def average_quaternion(Q, W=None, wsum=None):
    """Markley's mean: the top eigenvector of sum_r w_r q_r q_r^T / sum_r w_r over the members (..., n, 4), real part made positive"""
    W = torch.ones_like(Q[..., 0]) if W is None else W
    return _pos_real(torch.linalg.eigh(moment_matrix(Q, W, wsum))[1][..., -1])


def eigen_gap(Q, W=None):
    """lambda_1 - lambda_2 of the moment matrix: the conditioning of the mean"""
    W = torch.ones_like(Q[..., 0]) if W is None else W
    ev = torch.linalg.eigvalsh(moment_matrix(Q.double(), W.double()))
    return ev[..., -1] - ev[..., -2]


def aa_to_matrix(aa):
    return quaternion_to_matrix(axis_angle_to_quaternion(aa))


def geodesic(Ra, Rb):
    """the angle of Ra Rb^T from the chord: ||Ra - Rb||_F = 2 sqrt(2) sin(angle / 2), accurate down to angle 0"""
    d = (Ra.double() - Rb.double()).flatten(-2).norm(dim=-1)
    return 2 * torch.asin((d / (2 * math.sqrt(2))).clamp(max=1.0))


def check_rotation(name, got_R, ref_R, f32_R, out_scale):
    """rotations compared as rotations: geodesic angle to the float64 reference, bound = the rule applied to the angle of the float32
    restatement (4 x its worst angle, floor 4 ulp of the largest output component `out_scale`)"""
    ang = geodesic(got_R.detach().cpu(), ref_R)
    tol = max(4.0 * float(geodesic(f32_R, ref_R).max()), 4.0 * ULP * float(out_scale))
    check(name, ang, torch.zeros_like(ang), tol)


def _quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def clustered_quaternions(prefix, n, g, spread=0.35, identical=False):
    """float64 unit quaternions (*prefix, n, 4): n members within `spread` rad of one random rotation per prefix entry"""
    common = _unit(torch.randn(*prefix, 1, 4, generator=g, dtype=torch.float64))
    axis = _unit(torch.randn(*prefix, n, 3, generator=g, dtype=torch.float64))
    ang = torch.rand(*prefix, n, 1, generator=g, dtype=torch.float64) * spread * (0.0 if identical else 1.0)
    return _quat_mul(common.expand(*prefix, n, 4), torch.cat([torch.cos(ang / 2), axis * torch.sin(ang / 2)], -1))


def clustered_axis_angles(prefix, n, g, identical=False):
    """float32 axis-angle members (*prefix, n, 3) within 0.4 rad of a common rotation; every third member is written with its rotation
    angle in (pi, 2 pi) (the same rotation, the quaternion's real part negative: the q0 > 0 sign fix has to act)"""
    q = _pos_real(clustered_quaternions(prefix, n, g, identical=identical))
    aa = quaternion_to_axis_angle(q)                                                                  # angle in [0, pi]
    ang = aa.norm(dim=-1, keepdim=True).clamp_min(1e-3)
    long_way = aa * (ang - 2 * math.pi) / ang                                                         # same axis, angle - 2 pi
    pick = (torch.arange(n) % 3 == 1).reshape((1,) * len(prefix) + (n, 1)) & (ang > 0.05) & (not identical)
    return torch.where(pick, long_way, aa).float()


# ------------------------------------------------------------------------------------------------ projection, bicubic look-up
def project_norm(P, K, bbox):
    """pinhole projection of P (bs, ..., 3) with K (bs,3,3), then normalisation of the pixel to the box (bs,4) -> gx, gy in (-1, 1) inside"""
    sh = (-1,) + (1,) * (P.dim() - 2)
    k = lambda r, c: K[:, r, c].reshape(sh)
    u = P[..., 0] * k(0, 0) + P[..., 1] * k(0, 1) + P[..., 2] * k(0, 2)
    v = P[..., 0] * k(1, 0) + P[..., 1] * k(1, 1) + P[..., 2] * k(1, 2)
    w = P[..., 0] * k(2, 0) + P[..., 1] * k(2, 1) + P[..., 2] * k(2, 2)
    bb = lambda c: bbox[:, c].reshape(sh)
    return 2 * (u / w - bb(0)) / (bb(2) - bb(0)) - 1, 2 * (v / w - bb(1)) / (bb(3) - bb(1)) - 1


def grid_index(g, size):
    return ((g + 1) * size - 1) / 2


def cubic_weight(d):
    """Keys' cubic convolution kernel with A = -0.75 at distance d >= 0"""
    A = -0.75
    return torch.where(d <= 1, (A + 2) * d ** 3 - (A + 3) * d ** 2 + 1, A * d ** 3 - 5 * A * d ** 2 + 8 * A * d - 4 * A)


def bicubic16(planes, gx, gy):
    """planes (bs,m,H,W); gx, gy (bs,C,m): plane i sampled at point i.  -> value (bs,C,m) and S = sum |tap * weight| of that look-up"""
    bs, m, H, W = planes.shape
    ix, iy = grid_index(gx, W), grid_index(gy, H)
    fx, fy = torch.floor(ix), torch.floor(iy)
    tx, ty = ix - fx, iy - fy
    bi, mi = torch.arange(bs)[:, None, None], torch.arange(m)[None, None, :]
    val, S = torch.zeros_like(gx), torch.zeros_like(gx)
    for i in (-1, 0, 1, 2):
        yy, wy = fy + i, cubic_weight((ty - i).abs())
        for j in (-1, 0, 1, 2):
            xx, wx = fx + j, cubic_weight((tx - j).abs())
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            tap = planes[bi, mi, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()] * ok.to(planes.dtype)
            term = tap * wx * wy
            val, S = val + term, S + term.abs()
    return val, S


def hand_heat(joints, root, K, bbox, heatmap, observe, want_S=False):
    """hv[b,c,i] = bicubic(heatmap[b, observe[i]], project(joints[b,c,observe[i]] + root[b]))"""
    P = joints[:, :, observe] + root[:, None, None]
    gx, gy = project_norm(P, K, bbox)
    val, S = bicubic16(heatmap[:, observe], gx, gy)
    return (val, S) if want_S else val


# ------------------------------------------------------------------------------------------------ object transforms
def obj_points(pose, root, table, obj_id, is_right):
    """flip(R(pose) p + t + root): pose (bs,n,9), table (n_obj,P,3) -> (bs,n,P,3); the flip negates x of a LEFT hand's image"""
    R = rot6d_to_matrix(pose[..., :6])
    t = pose[..., 6:] + root[:, None]
    p = (table[obj_id.long()][:, None, :, None, :] * R[:, :, None, :, :]).sum(-1) + t[:, :, None]
    sgn = torch.where(is_right.bool(), 1.0, -1.0).to(p.dtype)[:, None, None]
    return torch.cat([p[..., :1] * sgn[..., None], p[..., 1:]], -1)


def with_translation(pose, transl):
    return pose if transl is None else torch.cat([pose[..., :6], transl[:, None].expand(pose.shape[0], pose.shape[1], 3)], -1)


def obj_heat_score(pose, transl_override, root, kpt, obj_id, is_right, K, bbox, heatmap, want_S=False):
    """score[b,c] = sum_j bicubic(heatmap[b,j], project(key-point j of candidate c)); an override replaces the pose's translation"""
    gx, gy = project_norm(obj_points(with_translation(pose, transl_override), root, kpt, obj_id, is_right), K, bbox)
    val, S = bicubic16(heatmap, gx, gy)
    return (val.sum(-1), S.sum(-1)) if want_S else val.sum(-1)


def obj_verts(pose, root, vert, obj_id, is_right):
    return obj_points(pose[:, None], root, vert, obj_id, is_right)[:, 0]


def squared_distances(x, y):
    return ((x[..., :, None, :] - y[..., None, :, :]) ** 2).sum(-1)


def argmin_first(d2):
    """smaller value, then smaller index -- explicit, not torch's"""
    m = d2.min(dim=-1, keepdim=True)[0]
    n = d2.shape[-1]
    return torch.where(d2 == m, torch.arange(n), torch.full((), n, dtype=torch.long)).min(dim=-1)[0]


def obj_physics_score(cand, root, vert, com, obj_id, is_right, force_point, force_global, pick=None):
    """-(sum_a w_a d_a) * |sum_a u_a x (fp_a - nearest_a - CoM)|, w = |f| / sum |f|, u = f / |f|, d = the distance to the nearest transformed
    vertex.  pick (bs,n,32): use these vertices instead of the arg-min (the tie test's counter-example)"""
    verts = obj_points(cand, root, vert, obj_id, is_right)                                           # (bs,n,nv,3)
    c = obj_points(cand, root, com[:, None], obj_id, is_right)                                       # (bs,n,1,3)
    idx = argmin_first(squared_distances(force_point[:, None], verts)) if pick is None else pick     # (bs,n,32)
    nn = torch.gather(verts, 2, idx[..., None].expand(idx.shape + (3,)))
    d = (force_point[:, None] - nn).norm(dim=-1)
    nrm = force_global.norm(dim=-1)
    sc = (d * (nrm / nrm.sum(-1, keepdim=True))[:, None]).sum(-1)
    u = (force_global / nrm[..., None])[:, None].expand_as(nn)
    L = torch.cross(u, force_point[:, None] - nn - c, dim=-1).sum(-2).norm(dim=-1)
    return -(sc * L)


def nearest_separation(cand, root, vert, obj_id, is_right, force_point):
    """the smallest relative gap (d2_second - d2_first) / d2_second over every (candidate, force point), in float64"""
    verts = obj_points(cand.double(), root.double(), vert.double(), obj_id, is_right)
    two = torch.topk(squared_distances(force_point.double()[:, None], verts), 2, dim=-1, largest=False)[0]
    return float(((two[..., 1] - two[..., 0]) / two[..., 1]).min())


def obj_pt2d_score(pose, root, kpt, obj_id, is_right, K, bbox, peak):
    gx, gy = project_norm(obj_points(pose, root, kpt, obj_id, is_right), K, bbox)
    return -torch.sqrt((gx - peak[:, None, :, 0]) ** 2 + (gy - peak[:, None, :, 1]) ** 2).sum(-1)


def hand_pt2d_score(joints, root, K, bbox, peak, per_joint):
    gx, gy = project_norm(joints + root[:, None, None], K, bbox)
    s = -torch.sqrt((gx - peak[:, None, :, 0]) ** 2 + (gy - peak[:, None, :, 1]) ** 2)
    return s if per_joint else s.sum(-1)


# ------------------------------------------------------------------------------------------------ gathers
def hand_candidates(diff, reg):
    """(bs,S,ld>=48), (bs,48) -> (bs,2S,48): [the S diffusion poses | S regression poses with the wrist of diffusion pose c - S]"""
    bs, S = diff.shape[:2]
    second = reg[:, None].expand(bs, S, 48).clone()
    second[..., :3] = diff[..., :3]
    return torch.cat([diff[..., :48], second], 1)


def obj_cross(pose, transl_idx, rot_idx):
    bs, ko = rot_idx.shape
    b = torch.arange(bs)[:, None, None]
    rot = pose[b, rot_idx.long()[:, None, :].expand(bs, ko, ko)][..., :6]                            # candidate i*ko + j: rotation j
    tr = pose[b, transl_idx.long()[:, :, None].expand(bs, ko, ko)][..., 6:]                          # translation i
    return torch.cat([rot, tr], -1).reshape(bs, ko * ko, 9)


def hand_phys_candidates(agg_pose, betas, topk_pose):
    """(bs,ld>=48), (bs,10), (bs,k,5,3) -> (bs,k+1,58): candidate c < k = the aggregated pose with rotations 15, 3, 6, 12, 9 taken from
    columns 0..4 of topk_pose[b,c]; candidate k = the aggregated pose; columns 48..57 the betas"""
    bs, k = topk_pose.shape[:2]
    out = torch.cat([agg_pose[:, None, :48].expand(bs, k + 1, 48), betas[:, None].expand(bs, k + 1, 10)], -1).clone()
    for f, joint in enumerate(LVL3_JOINT):
        out[:, :k, joint * 3:joint * 3 + 3] = topk_pose[:, :, f]
    return out


def hand_joint_gather_mean(joints, idx):
    """joints (bs,C,21,3), idx (bs,21,k): joint j = the mean over the k candidates listed FOR THAT JOINT"""
    bs, _, k = idx.shape
    b, j = torch.arange(bs)[:, None, None], torch.arange(21)[None, :, None]
    return joints[b, idx.long(), j].sum(2) / k


def topk_weights(val):
    return (val + 1e-8) / (val.sum(-1, keepdim=True) + 1e-8)


# ------------------------------------------------------------------------------------------------ anchors, hand physics, fuses
def force_anchor(verts, root, force_local, hands_per_image, face, aw, v2j, skel):
    """hand h belongs to image h // hands_per_image: its root and its force_local row.  -> the 32 anchor points (barycentric in their
    face) and force_local turned into the anchor frame (x, y, z) = (y x z, z x x normalised, face normal), y along the bone"""
    img = torch.arange(verts.shape[0]) // hands_per_image
    V = verts + root[img][:, None]
    J = torch.einsum('jv,nvc->njc', v2j, V)
    p0, p1, p2 = V[:, face[:, 0]], V[:, face[:, 1]], V[:, face[:, 2]]
    b1, b2 = p1 - p0, p2 - p0
    unit8 = lambda v: v / (v.norm(dim=-1, keepdim=True) + 1e-8)
    dz = unit8(torch.cross(b1, b2, dim=-1))
    dy = unit8(J[:, skel[:, 1]] - J[:, skel[:, 0]])
    dx = torch.cross(dy, dz, dim=-1)
    dy = unit8(torch.cross(dz, dx, dim=-1))
    fl = force_local[img]
    return aw[:, 0:1] * b1 + aw[:, 1:2] * b2 + p0, fl[..., 0:1] * dx + fl[..., 1:2] * dy + fl[..., 2:3] * dz


def hand_phys_score(force_point, force_global, obj_vert, bs, n_cand):
    """(bs*n_cand,32,3) x2, (bs,nv,3) -> (bs,n_cand,5): finger f = sum over its four anchors of -(w_a d_a |sum_a u_a|)"""
    fp, fg = force_point.reshape(bs, n_cand, 32, 3), force_global.reshape(bs, n_cand, 32, 3)
    d = squared_distances(fp, obj_vert[:, None]).min(dim=-1)[0].sqrt()
    nrm = fg.norm(dim=-1)
    I = (fg / nrm[..., None]).sum(-2).norm(dim=-1)
    s = -((nrm / nrm.sum(-1, keepdim=True)) * d * I[..., None])
    return torch.stack([s[..., a].sum(-1) for a in FINGER_ANCHOR], -1)


def hand_phys_fuse(cand, idx):
    """cand (bs,n_cand,58), idx (bs,5,k): candidate 0 with, per finger, rotations LVL2[f] and LVL3[f] = the un-weighted quaternion mean
    over that finger's k listed candidates"""
    bs = cand.shape[0]
    out = cand[:, 0].clone()
    b = torch.arange(bs)[:, None]
    for f in range(5):
        for joint in (LVL2_JOINT[f], LVL3_JOINT[f]):
            q = axis_angle_to_quaternion(cand[b, idx[:, f].long()][..., joint * 3:joint * 3 + 3])
            out[:, joint * 3:joint * 3 + 3] = quaternion_to_axis_angle(average_quaternion(q))
    return out


def hand_pose_fuse(pose, idx, w, n):
    """pose (bs,C,ld): the 16 rotations of the fused pose = weighted quaternion means over the listed candidates (None: 0..n-1, weights 1)"""
    bs = pose.shape[0]
    idx = torch.arange(n)[None].expand(bs, n) if idx is None else idx.long()
    sel = pose[torch.arange(bs)[:, None], idx][..., :48].reshape(bs, idx.shape[1], 16, 3)
    q = axis_angle_to_quaternion(sel).permute(0, 2, 1, 3)
    W = None if w is None else w[:, None].expand(bs, 16, idx.shape[1])
    return quaternion_to_axis_angle(average_quaternion(q, W)).reshape(bs, 48)


def sequential_sum_f32(w):
    """sum over the last axis in float32, left to right from 0 (the kernel's ``wsum += w``)"""
    s = torch.zeros(w.shape[:-1], dtype=torch.float32)
    for r in range(w.shape[-1]):
        s = s + w[..., r].float()
    return s


def obj_fuse(pose, idx, w32):
    """pose (bs,n,9) float64, idx (bs,k), w32 (bs,k) FLOAT32 weights or None (uniform 1/k in float32): rotation = quaternion mean with
    the moment matrix divided by the float32 sum of the weights, translation = sum_r w_r t_r (not normalised) -> (bs,9) float64"""
    bs, k = idx.shape
    w32 = torch.full((bs, k), float(np.float32(1.0) / np.float32(k)), dtype=torch.float32) if w32 is None else w32
    sel = pose[torch.arange(bs)[:, None], idx.long()]
    W = w32.to(pose.dtype)
    q = average_quaternion(matrix_to_quaternion(rot6d_to_matrix(sel[..., :6])), W, wsum=sequential_sum_f32(w32).to(pose.dtype))
    return torch.cat([quaternion_to_matrix(q).reshape(bs, 9)[:, :6], (sel[..., 6:] * W[..., None]).sum(1)], -1)


# ------------------------------------------------------------------------------------------------ assets
def small_assets(n_obj=4, n_kpt=5, n_vert=37, dense_v2j=False, seed=0):
    """an asset dict ``ops.Aggregation(assets, skeleton, 'cuda')`` accepts, with tables of a chosen size.  dense_v2j: all 778 weights of
    every vert2joint row non-zero (a small floor under a joint's own cluster of vertices, rows summing to 1), else 10 non-zeros per row"""
    g = gen(1000 + seed)
    r = lambda *s: torch.rand(*s, generator=g)
    ycb = {f'object_{o}': dict(kpt3d=((r(n_kpt, 3) - 0.5) * 0.2).numpy(), verts_sampled=((r(n_vert, 3) - 0.5) * 0.2).numpy(),
                               CoM=((r(3) - 0.5) * 0.04).numpy()) for o in range(n_obj)}
    face = torch.stack([torch.randperm(778, generator=g)[:3] for _ in range(32)])
    v2j = torch.zeros(21, 778)
    for j in range(21):
        v2j[j, torch.randperm(778, generator=g)[:10]] = 0.5 + r(10)
    if dense_v2j:
        v2j = v2j + 0.2 * (0.5 + r(21, 778)) * (v2j.sum(1, keepdim=True) / 778)
    v2j = v2j / v2j.sum(1, keepdim=True)
    return dict(ycb=ycb, anchor=dict(face_vert_idx=face.numpy().astype(np.int64), anchor_weight=(0.1 + 0.4 * r(32, 2)).numpy(),
                                     vert2joint=v2j.numpy()))


def tables(assets):
    """the float32 CPU tables of an asset dict, stacked as ops.Aggregation stacks them"""
    y = assets['ycb']
    st = lambda key: torch.stack([torch.as_tensor(y[n][key], dtype=torch.float32).reshape(-1, 3) for n in y])
    a = assets['anchor']
    return dict(kpt=st('kpt3d'), vert=st('verts_sampled'), com=st('CoM').reshape(len(y), 3), face=torch.as_tensor(a['face_vert_idx']).long(),
                aw=torch.as_tensor(a['anchor_weight'], dtype=torch.float32), v2j=torch.as_tensor(a['vert2joint'], dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ input generators
def cameras(bs, g):
    """per-image intrinsics with a non-zero skew, a root joint in front of the camera and a non-square box"""
    K = torch.zeros(bs, 3, 3)
    K[:, 0, 0], K[:, 1, 1] = 550 + 100 * torch.rand(bs, generator=g), 480 + 100 * torch.rand(bs, generator=g)
    K[:, 0, 1] = 2 + 6 * torch.rand(bs, generator=g)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 300 + 40 * torch.rand(bs, generator=g), 230 + 40 * torch.rand(bs, generator=g), 1.0
    root = torch.cat([(torch.rand(bs, 2, generator=g) - 0.5) * 0.2, 0.5 + 0.3 * torch.rand(bs, 1, generator=g)], 1)
    return K, root


def box_around(centre_px, g, w=(230., 300.), h=(140., 190.)):
    bs = centre_px.shape[0]
    wh = torch.stack([w[0] + (w[1] - w[0]) * torch.rand(bs, generator=g), h[0] + (h[1] - h[0]) * torch.rand(bs, generator=g)], 1)
    c = centre_px + (torch.rand(bs, 2, generator=g) - 0.5) * 10
    return torch.cat([c - wh / 2, c + wh / 2], 1).contiguous()


HEAT_CLASSES = ('interior', 'interior', 'x_low', 'x_high', 'y_edge', 'centre', 'far')               # the position class of candidate c


def hand_heat_inputs(seed=0, bs=3):
    """joints (bs,7,21,3) placed BY CONSTRUCTION: candidate c's 21 joints all fall in position class HEAT_CLASSES[c] of their H_MAP x W_MAP
    map -- interior; grid x in [-2, 0) / [W-1, W+1) (some taps outside); grid y in [-2, 0) (even joints) or [H-1, H+1) (odd); on a pixel
    centre (to the rounding of the float32 inputs: either side of the floor); far outside with a grid coordinate up to 1e6.  The wanted
    grid index is turned into a pixel of the box and back-projected through K (skew included) at a depth z in (0.3, 1)."""
    g = gen(2000 + seed)
    C, J, H, W = len(HEAT_CLASSES), 21, H_MAP, W_MAP
    K, root = cameras(bs, g)
    bbox = box_around(torch.stack([K[:, 0, 2], K[:, 1, 2]], 1), g)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(bs, J, generator=g, dtype=torch.float64)
    ix, iy = torch.zeros(bs, C, J, dtype=torch.float64), torch.zeros(bs, C, J, dtype=torch.float64)
    odd = (torch.arange(J) % 2 == 1)[None]
    for c, cls in enumerate(HEAT_CLASSES):
        ix[:, c], iy[:, c] = u(1.2, W - 2.2), u(1.2, H - 2.2)
        if cls == 'x_low':
            ix[:, c] = u(-1.95, -0.05)
        elif cls == 'x_high':
            ix[:, c] = u(W - 0.95, W + 0.95)
        elif cls == 'y_edge':
            iy[:, c] = torch.where(odd, u(H - 0.95, H + 0.95), u(-1.95, -0.05))
        elif cls == 'centre':
            ix[:, c], iy[:, c] = torch.floor(u(0, W - 0.01)), torch.floor(u(0, H - 0.01))
        elif cls == 'far':
            far = torch.where(torch.arange(J)[None] % 4 < 2, 1.0, -1.0) * 10.0 ** u(2, 6)
            ix[:, c] = torch.where(odd, ix[:, c], far)
            iy[:, c] = torch.where(odd, far, iy[:, c])
    Kd, bd = K.double(), bbox.double()
    px = (ix + 0.5) / W * (bd[:, 2] - bd[:, 0])[:, None, None] + bd[:, 0, None, None]
    py = (iy + 0.5) / H * (bd[:, 3] - bd[:, 1])[:, None, None] + bd[:, 1, None, None]
    z = 0.3 + 0.7 * torch.rand(bs, C, J, generator=g, dtype=torch.float64)
    y = (py - Kd[:, 1, 2, None, None]) * z / Kd[:, 1, 1, None, None]
    x = ((px - Kd[:, 0, 2, None, None]) * z - Kd[:, 0, 1, None, None] * y) / Kd[:, 0, 0, None, None]
    joints = (torch.stack([x, y, z], -1) - root.double()[:, None, None]).float().contiguous()
    heatmap = (0.05 + torch.rand(bs, J, H, W, generator=g)).contiguous()
    return dict(joints=joints, root=root, K=K, bbox=bbox, heatmap=heatmap)


def heat_grid_indices(d):
    """the float64 grid coordinates (ix, iy) (bs,C,21) of the joints of hand_heat_inputs"""
    j, r, K, b = to64([d['joints'], d['root'], d['K'], d['bbox']])
    gx, gy = project_norm(j + r[:, None, None], K, b)
    return grid_index(gx, W_MAP), grid_index(gy, H_MAP)


def heat_classes_hold(d):
    """every joint of every candidate lies in the class hand_heat_inputs put it in, and in front of the camera"""
    ix, iy = heat_grid_indices(d)
    H, W = H_MAP, W_MAP
    odd = (torch.arange(21) % 2 == 1)[None]
    inside = lambda c: bool(((ix[:, c] > 1) & (ix[:, c] < W - 2) & (iy[:, c] > 1) & (iy[:, c] < H - 2)).all())
    ok = bool(((d['joints'][..., 2] + d['root'][:, None, None, 2]) > 0.05).all()) and bool(torch.isfinite(d['joints']).all())
    for c, cls in enumerate(HEAT_CLASSES):
        x, y = ix[:, c], iy[:, c]
        if cls == 'interior':
            ok &= inside(c)
        elif cls == 'x_low':
            ok &= bool(((x >= -2) & (x < 0)).all())
        elif cls == 'x_high':
            ok &= bool(((x >= W - 1) & (x < W + 1)).all())
        elif cls == 'y_edge':
            ok &= bool(torch.where(odd, (y >= H - 1) & (y < H + 1), (y >= -2) & (y < 0)).all())
        elif cls == 'centre':
            ok &= bool((((x - x.round()).abs() < 1e-3) & ((y - y.round()).abs() < 1e-3) & (x.round() >= 0) & (x.round() <= W - 1)
                        & (y.round() >= 0) & (y.round() <= H - 1)).all())
        elif cls == 'far':
            m = torch.where(odd, y.abs(), x.abs())
            ok &= bool(((m >= 99) & (m <= 1.01e6)).all())
    return ok


def obj_scene(seed, tab, bs=3, n=9, pose_f32=False):
    """an object batch on the tables `tab`: distinct ids (one the LAST table row), is_right = [1,0,1], non-orthonormal 6-D rotations,
    translations of a few centimetres, a camera whose box is centred on the (flipped) object.  pose_f32: the float64 poses hold float32
    values (for the kernels that cast them with (float))"""
    g = gen(3000 + seed)
    n_obj, n_kpt = tab['kpt'].shape[:2]
    K, root = cameras(bs, g)
    obj_id = torch.tensor([(n_obj - 1 - 3 * i) % n_obj for i in range(bs)], dtype=torch.int32)
    is_right = torch.tensor([(i + 1) % 2 for i in range(bs)], dtype=torch.uint8)
    pose = torch.cat([torch.randn(bs, n, 6, generator=g, dtype=torch.float64) + torch.tensor([1., 0, 0, 0, 1, 0], dtype=torch.float64) * 0.5,
                      (torch.rand(bs, n, 3, generator=g, dtype=torch.float64) - 0.5) * 0.06], -1)
    transl = (torch.rand(bs, 3, generator=g, dtype=torch.float64) - 0.5) * 0.06
    if pose_f32:
        pose, transl = pose.float().double(), transl.float().double()
    c = root.double().clone()
    c[:, 0] = c[:, 0] * torch.where(is_right.bool(), 1.0, -1.0).double()                            # where the flipped object lands
    gx, gy = project_norm(c, K.double(), torch.tensor([[0., 0, 2, 2]], dtype=torch.float64).expand(bs, 4))   # box (0,0,2,2): g + 1 = the pixel
    bbox = box_around(torch.stack([gx + 1, gy + 1], 1).float(), g)
    heatmap = (0.05 + torch.rand(bs, n_kpt, H_MAP, W_MAP, generator=g)).contiguous()
    peak = ((torch.rand(bs, n_kpt, 2, generator=g) - 0.5) * 1.6).contiguous()
    return dict(pose=pose.contiguous(), transl=transl.contiguous(), root=root, K=K, bbox=bbox, obj_id=obj_id, is_right=is_right, heatmap=heatmap, peak=peak)


def physics_scene(seed, tab, bs=3, n=6):
    """obj_scene (float32-valued poses) plus 32 force points within a few centimetres of the candidates' clouds and non-zero forces"""
    d = obj_scene(seed, tab, bs=bs, n=n, pose_f32=True)
    g = gen(4000 + seed)
    sgn = torch.where(d['is_right'].bool(), 1.0, -1.0)[:, None, None] * torch.tensor([1., 0, 0]) + torch.tensor([0., 1, 1])
    d['force_point'] = ((d['root'][:, None] + (torch.rand(bs, 32, 3, generator=g) - 0.5) * 0.12) * sgn).contiguous()
    d['force_global'] = (torch.randn(bs, 32, 3, generator=g) * (0.2 + torch.rand(bs, 32, 1, generator=g))).contiguous()
    return d


PHYSICS_CASES = [(37, 1), (37, 6), (2048, 1), (2048, 6), (4096, 1), (4096, 6)]                      # (n_vert, n): 4096 = the entry point's limit
SEPARATION = 1e-5


def physics_case(n_vert, n):
    assets = small_assets(n_vert=n_vert, seed=n_vert)
    return assets, physics_scene(n_vert + n, tables(assets), n=n)


def tie_case(a=0.03, i=5, j=18, n_vert=37):
    """two table vertices at (+a,0,0) [index i] and (-a,0,0) [index j > i, another lane of the 8-lane search], every other vertex at least
    2a away, identity rotation, zero translation and root, right hand, every force point at the origin: both are nearest at exactly a^2"""
    g = gen(77)
    v = _unit(torch.randn(n_vert, 3, generator=g)) * (2 * a + 0.05 * torch.rand(n_vert, 1, generator=g))
    v[i], v[j] = torch.tensor([a, 0., 0.]), torch.tensor([-a, 0., 0.])
    assets = small_assets(n_obj=1, n_vert=n_vert)
    assets['ycb']['object_0'].update(verts_sampled=v.numpy(), CoM=np.array([0.004, -0.007, 0.011], np.float32))
    d = dict(pose=torch.tensor([[[1., 0, 0, 0, 1, 0, 0, 0, 0]]], dtype=torch.float64), root=torch.zeros(1, 3), obj_id=torch.zeros(1, dtype=torch.int32),
             is_right=torch.ones(1, dtype=torch.uint8), force_point=torch.zeros(1, 32, 3),
             force_global=(torch.randn(1, 32, 3, generator=g) * 0.5).contiguous())
    return assets, d, i, j


FUSE_GAP = 0.2


def pose_fuse_inputs(seed, bs=5, C=6, ld=48, identical=False):
    """candidate poses (bs,C,ld): per (image, rotation) the C members lie within 0.4 rad of a common random rotation"""
    g = gen(5000 + seed)
    aa = clustered_axis_angles((bs, 16), C, g, identical=identical)                                   # (bs,16,C,3)
    pose = torch.full((bs, C, ld), SENT)
    pose[..., :48] = aa.permute(0, 2, 1, 3).reshape(bs, C, 48)
    return pose.contiguous(), g


def phys_fuse_inputs(seed, bs=3, n_cand=6, identical=False):
    pose, g = pose_fuse_inputs(100 + seed, bs=bs, C=n_cand, ld=58, identical=identical)
    pose[..., 48:] = torch.randn(bs, 1, 10, generator=g).expand(bs, n_cand, 10)
    return pose.contiguous(), g


def obj_fuse_inputs(seed, bs=65, n=7, identical=False):
    """float64 poses (bs,n,9): rotations within 0.4 rad of a common one per image, written as NON-orthonormal 6-D (rows scaled, the second
    sheared along the first); positive translations (no cancellation in the weighted sum)"""
    g = gen(6000 + seed)
    R = quaternion_to_matrix(clustered_quaternions((bs,), n, g, identical=identical))
    s = 0.5 + torch.rand(bs, n, 3, generator=g, dtype=torch.float64)
    d6 = torch.cat([R[..., 0, :] * s[..., 0:1], R[..., 1, :] * s[..., 1:2] + R[..., 0, :] * (s[..., 2:3] - 1)], -1)
    t = torch.tensor([0.1, 0.2, 0.6], dtype=torch.float64) + 0.05 * torch.rand(bs, n, 3, generator=g, dtype=torch.float64)
    return torch.cat([d6, t], -1).contiguous(), g


def pose_quaternions(pose, idx):
    """(bs,16,n,4) float64 quaternions of the listed candidates' rotations (the eigen-gap condition is asserted on these)"""
    bs = pose.shape[0]
    sel = pose.double()[torch.arange(bs)[:, None], idx.long()][..., :48].reshape(bs, idx.shape[1], 16, 3)
    return axis_angle_to_quaternion(sel).permute(0, 2, 1, 3)


def pt2d_inputs(seed=0, bs=2, C=130):
    """hand joints for the 2-D point scores; image 1 has a camera, box and root made of few-bit numbers and joint 4 of candidate 7 placed so
    that every operation of its projection is exact: its normalised point is (0.24951171875, -0.125) in any arithmetic -- the peak of
    that joint is put there"""
    g = gen(7000 + seed)
    K, root = cameras(bs, g)
    bbox = box_around(torch.stack([K[:, 0, 2], K[:, 1, 2]], 1), g)
    K[1] = torch.tensor([[512., 2, 320], [0, 512, 256], [0, 0, 1]])
    bbox[1] = torch.tensor([256., 128, 512, 384])
    root[1] = torch.tensor([0.125, -0.0625, 0.5])
    joints = (torch.randn(bs, C, 21, 3, generator=g) * 0.06).contiguous()
    joints[1, 7, 4] = torch.tensor([0.0625, 0.03125, 0.5])
    peak = ((torch.rand(bs, 21, 2, generator=g) - 0.5) * 1.6).contiguous()
    peak[1, 4] = torch.tensor([0.24951171875, -0.125])
    return dict(joints=joints, root=root, K=K, bbox=bbox, peak=peak)


# ------------------------------------------------------------------------------------------------ the fuse cases of both test files
def _randint(g, hi, *shape):
    return torch.randint(0, hi, shape, generator=g, dtype=torch.int32)


def _perms(g, n, k, *prefix):
    """k distinct indices out of n per prefix entry (as a top-k list is)"""
    flat = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(int(np.prod(prefix)))])
    return flat.reshape(*prefix, k).to(torch.int32).contiguous()


POSE_FUSE_CASES = ('idx_w', 'first_n', 'idx_only', 'repeats', 'identical')


def pose_fuse_case(name):
    """-> pose (5,6,ld), idx (5,n) int32 | None, w (5,n) | None, n.  bs = 5: 80 lanes, two 64-lane blocks"""
    bs, C = 5, 6
    if name == 'idx_w':
        pose, g = pose_fuse_inputs(1, bs, C, 48)
        return pose, _perms(g, C, 4, bs), (0.1 + torch.rand(bs, 4, generator=g)).contiguous(), 4
    if name == 'first_n':                                                                           # idx None with n < C, w None
        return pose_fuse_inputs(2, bs, C, 58)[0], None, None, 4
    if name == 'idx_only':
        pose, g = pose_fuse_inputs(3, bs, C, 48)
        return pose, _perms(g, C, 5, bs), None, 5
    if name == 'repeats':                                                                           # n = 2C: every candidate listed twice
        pose, g = pose_fuse_inputs(4, bs, C, 58)
        return pose, torch.cat([_perms(g, C, C, bs), _perms(g, C, C, bs)], 1).contiguous(), (0.1 + torch.rand(bs, 2 * C, generator=g)).contiguous(), 2 * C
    pose, g = pose_fuse_inputs(5, bs, C, 48, identical=True)
    return pose, _perms(g, C, 4, bs), (0.1 + torch.rand(bs, 4, generator=g)).contiguous(), 4


def pose_fuse_gap(pose, idx, w, n):
    bs = pose.shape[0]
    idx = torch.arange(n, dtype=torch.int32)[None].expand(bs, n) if idx is None else idx
    return float(eigen_gap(pose_quaternions(pose, idx), None if w is None else w[:, None].expand(bs, 16, idx.shape[1])).min())


PHYS_FUSE_CASES = ((1, False), (5, False), (5, True))                                               # (k, identical rotations); n_cand = 6


def phys_fuse_case(k, identical):
    cand, g = phys_fuse_inputs(k, 3, 6, identical)
    return cand, _perms(g, 6, k, 3, 5)


def phys_fuse_gap(cand, idx):
    gaps = []
    for f in range(5):
        q = pose_quaternions(cand, idx[:, f])                                                         # (bs,16,k,4)
        gaps.append(eigen_gap(q[:, [LVL2_JOINT[f], LVL3_JOINT[f]]]).min())
    return float(min(gaps))


OBJ_FUSE_CASES = ('uniform', 'two_sources', 'identical')


def obj_fuse_case(name):
    """-> pose (65,7,9) float64, idx_a, w_a, idx_b, w_b, pick_b (None where not used).  bs = 65: two 64-lane blocks"""
    bs, n, k = 65, 7, 4
    pose, g = obj_fuse_inputs(len(name), bs, n, identical=name == 'identical')
    idx_a, w_a = _perms(g, n, k, bs), (0.1 + torch.rand(bs, k, generator=g)).contiguous()
    if name == 'uniform':
        return pose, idx_a, None, None, None, None
    if name == 'identical':
        return pose, idx_a, w_a, None, None, None
    pick = torch.tensor([0, 1, 0] * 22, dtype=torch.uint8)[:bs].contiguous()
    return pose, idx_a, w_a, _perms(g, n, k, bs), (0.1 + torch.rand(bs, k, generator=g)).contiguous(), pick


def obj_fuse_selected(pose, idx_a, w_a, idx_b, w_b, pick_b):
    """the (idx, w32) every image really fuses: source b where pick_b is set"""
    if pick_b is None:
        return idx_a, w_a
    p = pick_b.bool()[:, None]
    return torch.where(p, idx_b, idx_a), torch.where(p, w_b, w_a)


def obj_fuse_gap(pose, idx, w32):
    sel = pose[torch.arange(pose.shape[0])[:, None], idx.long()]
    W = torch.full(idx.shape, 1.0 / idx.shape[1], dtype=torch.float64) if w32 is None else w32.double()
    return float(eigen_gap(matrix_to_quaternion(rot6d_to_matrix(sel[..., :6])), W).min())


def force_anchor_inputs(n_hands, hands_per_image):
    """hand vertices (n_hands,778,3) and, PER IMAGE, a root joint and a force_local row (all distinct)"""
    g = gen(8000 + 10 * n_hands + hands_per_image)
    n_img = n_hands // hands_per_image
    verts = (torch.randn(n_hands, 778, 3, generator=g) * 0.05).contiguous()
    root = torch.cat([(torch.rand(n_img, 2, generator=g) - 0.5) * 0.3, 0.4 + 0.4 * torch.rand(n_img, 1, generator=g)], 1).contiguous()
    return verts, root, (torch.randn(n_img, 32, 3, generator=g) * 0.5).contiguous()


def faces_are_not_degenerate(verts, face):
    p0, p1, p2 = verts[:, face[:, 0]].double(), verts[:, face[:, 1]].double(), verts[:, face[:, 2]].double()
    return float(torch.cross(p1 - p0, p2 - p0, dim=-1).norm(dim=-1).min()) > 1e-5                    # twice the area; the edges are ~0.07 long

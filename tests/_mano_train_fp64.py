"""Plain torch restatement of the training-mode MANO head (csrc/mano_train.hip, ops.Mano.train), written from the kernel's header comment:
6-D -> Gram-Schmidt matrices -> shape and pose blend -> parent-table chain -> skinning -> root centring -> manopth or HO3D joint order ->
the four losses.  TEST INFRASTRUCTURE ONLY: nothing here imports ``vpho_amd.ops``.  Dtype-generic and differentiable: one definition gives
the float64 reference (autograd) and torch's own float32 evaluation for R.bound.  Pinned against the oracle's chain through the axis-angle
(oracle/rotations.py, oracle/mano.py, oracle.vpho.joints_ho3d) by tests/test_mano_train_fp64_cpu.py.

The oracle's chain, like the project it restates, turns each Gram-Schmidt matrix into an axis-angle and back through manopth's Rodrigues,
which takes the angle as |axis_angle + 1e-8|: its joints turn up to 1.7e-8 rad too far and its d_rot6d carries a term of relative size
1e-8 / angle.  The kernel feeds the matrices to the chain directly, and so does this reference.  For the pin alone, ``rodrigues_eps``
sends the chain's matrices through that round trip (written out here as axis, angle and the Rodrigues matrix): with 1e-8 the reference
reproduces the unmodified oracle, with 0.0 the round trip is the identity and must give what the default gives."""
import torch

from oracle.rotations import matrix_to_axis_angle
from tests import _leaf_fp64 as R

PARENT = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
TIPS = [745, 317, 444, 556, 673]
TIPS_HO3D = [728, 353, 442, 576, 694]
JOINT_ORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]
TO_MANOLAYER = [0, 5, 6, 7, 9, 10, 11, 17, 18, 19, 13, 14, 15, 1, 2, 3, 4, 8, 12, 16, 20]
LOSSES = ('vert_loss', 'joint_loss', 'mano_pose_loss', 'mano_shape_loss')
WEIGHTS = (1e4, 1e4, 10.0, 1.0)                                     # the training step's


def gram_schmidt(d6):
    """(..., 6) -> (..., 3, 3) with ROWS b1 = a1 / |a1|, b2 = u / |u| (u = a2 - (b1 . a2) b1), b3 = b1 x b2"""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u / u.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], -2)


def manopth_round_trip(Rm, eps):
    """Rm -> axis-angle -> the rotation manopth's layer makes of it: the quaternion (cos(a / 2), sin(a / 2) axis_angle / a), normalised,
    with a = |axis_angle + eps|, i.e. the same axis and the angle phi = 2 atan2(sin(a / 2) |axis_angle| / a, cos(a / 2))"""
    aa = matrix_to_axis_angle(Rm)
    th = aa.norm(dim=-1, keepdim=True)
    a = (aa + eps).norm(dim=-1, keepdim=True)
    phi = 2 * torch.atan2(torch.sin(a / 2) * th / a, torch.cos(a / 2))[..., None]
    n = aa / th
    z = torch.zeros_like(n[..., 0])
    K = torch.stack([z, -n[..., 2], n[..., 1], n[..., 2], z, -n[..., 0], -n[..., 1], n[..., 0], z], -1).reshape(*n.shape[:-1], 3, 3)
    return torch.eye(3, dtype=Rm.dtype) + torch.sin(phi) * K + (1 - torch.cos(phi)) * (K @ K)


def shape_blend(mano, shape):
    """shape (bs, 10) -> v_shaped (bs, 778, 3), J (bs, 16, 3) in the dtype of `shape`"""
    t = lambda k: torch.as_tensor(mano[k], dtype=shape.dtype)
    v_shaped = torch.einsum('vck,bk->bvc', t('shapedirs'), shape) + t('v_template')
    return v_shaped, torch.einsum('jv,bvc->bjc', t('J_regressor'), v_shaped)


def chain(mano, Rm, shape, is_ho3d=None):
    """joint rotations Rm (bs, 16, 3, 3), shape (bs, 10) -> root-centred verts (bs, 778, 3), joints (bs, 21, 3) in metres: shape blend, J,
    pose blend, parent-table chain, skinning with the rest joint removed, tips, root centring, manopth or HO3D joint order.  Shared by the
    training front end (``forward``: Gram-Schmidt matrices) and the forward-kinematics one (tests/_mano_fk_fp64.py: Rodrigues)."""
    t = lambda k: torch.as_tensor(mano[k], dtype=Rm.dtype)
    bs = Rm.shape[0]
    v_shaped, J = shape_blend(mano, shape)
    pf = (Rm[:, 1:] - torch.eye(3, dtype=Rm.dtype)).reshape(bs, 135)
    v_posed = v_shaped + torch.einsum('vck,bk->bvc', t('posedirs'), pf)
    Gr, Gt = [None] * 16, [None] * 16
    for j, p in enumerate(PARENT):
        if p < 0:
            Gr[j], Gt[j] = Rm[:, j], J[:, j]
        else:
            Gr[j] = Gr[p] @ Rm[:, j]
            Gt[j] = (Gr[p] @ (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[p]
    Gr, Gt = torch.stack(Gr, 1), torch.stack(Gt, 1)                   # (bs,16,3,3), (bs,16,3)
    At = Gt - (Gr @ J[..., None])[..., 0]                             # the rest joint removed
    W = t('weights')
    Tr, Tt = torch.einsum('vj,bjrc->bvrc', W, Gr), torch.einsum('vj,bjr->bvr', W, At)
    x = torch.einsum('bvrc,bvc->bvr', Tr, v_posed) + Tt
    cen = Gt[:, :1]
    j21 = torch.cat([Gt, x[:, TIPS]], 1)[:, JOINT_ORDER]
    if is_ho3d is not None:
        ho = torch.cat([j21[:, TO_MANOLAYER][:, :16], x[:, TIPS_HO3D]], 1)
        j21 = torch.where(is_ho3d.bool()[:, None, None], ho, j21)
    return x - cen, j21 - cen


def forward(mano, rot6d, shape, is_ho3d=None, rodrigues_eps=None):
    """rot6d (bs, 96), shape (bs, 10) -> root-centred verts (bs, 778, 3), joints (bs, 21, 3) in metres, Gram-Schmidt matrices (bs, 16, 3, 3)"""
    gs = gram_schmidt(rot6d.reshape(rot6d.shape[0], 16, 6))           # what the pose loss reads
    Rm = gs if rodrigues_eps is None else manopth_round_trip(gs, rodrigues_eps)
    return chain(mano, Rm, shape, is_ho3d) + (gs,)


def losses(mano, rot6d, shape, gt_vert, gt_joint, gt_rot6d, gt_shape, is_right, weights, is_ho3d=None, rodrigues_eps=None):
    """-> the four WEIGHTED losses (4,), verts, joints.  vert / joint / pose are means over all their elements; the shape loss is
    w * sum over RIGHT hands of (beta - beta_gt)^2 / (10 bs) -- 0 when no hand is right"""
    bs = rot6d.shape[0]
    v, j, Rm = forward(mano, rot6d, shape, is_ho3d, rodrigues_eps)
    right = is_right.bool()[:, None].to(rot6d.dtype)
    w = [float(x) for x in weights]
    L = torch.stack([w[0] * ((v - gt_vert) ** 2).mean(), w[1] * ((j - gt_joint) ** 2).mean(),
                     w[2] * ((Rm[:, :, :2].reshape(bs, 96) - gt_rot6d) ** 2).mean(),
                     w[3] * (right * (shape - gt_shape) ** 2).sum() / (10.0 * bs)])
    return L, v, j


def loss_and_grads(mano, rot6d, shape, *rest, **kw):
    """-> losses (4,), d (sum of the losses) / d rot6d, / d shape (autograd), verts, joints"""
    r, s = rot6d.detach().clone().requires_grad_(True), shape.detach().clone().requires_grad_(True)
    L, v, j = losses(mano, r, s, *rest, **kw)
    d6, db = torch.autograd.grad(L.sum(), [r, s], allow_unused=True)
    d6 = torch.zeros_like(r) if d6 is None else d6
    db = torch.zeros_like(s) if db is None else db
    return L.detach(), d6, db, v.detach(), j.detach()


# ------------------------------------------------------------------------------------------------ inputs
def random_rotations(n, g):
    """n float64 rotation matrices uniform over SO(3) (normalised Gaussian quaternions)"""
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    r, i, j, k = q.unbind(-1)
    m = torch.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r),
                     2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r),
                     2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)], -1).reshape(n, 3, 3)
    return m


def axis_angle_rotations(n, g, lo, hi):
    """float64 rotation matrices with a uniform random axis and an angle uniform in [lo, hi] (Rodrigues)"""
    ax = torch.randn(n, 3, generator=g, dtype=torch.float64)
    ax = ax / ax.norm(dim=-1, keepdim=True)
    th = lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    K = torch.zeros(n, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return torch.eye(3, dtype=torch.float64) + torch.sin(th)[:, None, None] * K + (1 - torch.cos(th))[:, None, None] * (K @ K)


def sheared_6d(Rm, g):
    """6-vectors whose Gram-Schmidt matrix is Rm (rows): a1 = s1 b1, a2 = s2 b2 + t b1 with s1, s2 in [0.2, 4] and |t| <= 2 s2, so
    |u| / |a2| = s2 / sqrt(s2^2 + t^2) >= 1 / sqrt(5) > 0.2 and the Gram-Schmidt backward stays conditioned"""
    n = Rm.shape[0]
    s = 0.2 + 3.8 * torch.rand(n, 2, generator=g, dtype=torch.float64)
    t = (torch.rand(n, generator=g, dtype=torch.float64) * 4 - 2) * s[:, 1]
    a1 = Rm[:, 0].double() * s[:, :1]
    a2 = Rm[:, 1].double() * s[:, 1:] + Rm[:, 0].double() * t[:, None]
    return torch.cat([a1, a2], -1)


IDENTITY_6D = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def flags(kind, bs):
    """'mixed' (alternating, the first set), 'all' or 'none' -> uint8 (bs,)"""
    return {'mixed': torch.arange(bs) % 2 == 0, 'all': torch.ones(bs, dtype=torch.bool), 'none': torch.zeros(bs, dtype=torch.bool)}[kind].to(torch.uint8)


def make(bs, seed, right='mixed', ho3d='mixed', identity_hand=True):
    """float32 CPU inputs of one call: rotations uniform over SO(3) (angles near pi included: the kernel never passes through the
    axis-angle), written as scaled and sheared 6-vectors; the LAST hand holds exact identity 6-vectors (pose feature 0)"""
    g = R.gen(seed)
    Rm = random_rotations(bs * 16, g)
    d6 = sheared_6d(Rm, g).reshape(bs, 96)
    if identity_hand:
        d6[-1] = torch.tensor(IDENTITY_6D, dtype=torch.float64).repeat(16)
    beta = torch.randn(bs, 10, generator=g) * 0.5
    gt_v, gt_j = torch.randn(bs, 778, 3, generator=g) * 0.05, torch.randn(bs, 21, 3, generator=g) * 0.05
    gt6, gtb = torch.randn(bs, 96, generator=g) * 0.5, torch.randn(bs, 10, generator=g) * 0.5
    return dict(rot6d=d6.float().contiguous(), shape=beta, gt_vert=gt_v, gt_joint=gt_j, gt_rot6d=gt6, gt_shape=gtb,
                is_right=flags(right, bs), is_ho3d=flags(ho3d, bs))


ARGS = ('rot6d', 'shape', 'gt_vert', 'gt_joint', 'gt_rot6d', 'gt_shape', 'is_right')


def reference(mano, d, weights, dtype, rodrigues_eps=None):
    """loss_and_grads of the inputs dict `d` in `dtype`"""
    a = [d[k].to(dtype) if d[k].is_floating_point() else d[k] for k in ARGS]
    return loss_and_grads(mano, *a, weights, is_ho3d=d['is_ho3d'], rodrigues_eps=rodrigues_eps)


def max_angle(rot6d):
    """largest rotation angle among the Gram-Schmidt matrices of rot6d (bs, 96), radians"""
    Rm = gram_schmidt(rot6d.double().reshape(-1, 6))
    return float(torch.acos(((Rm.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2).clamp(-1, 1)).max())

"""Plain torch restatement of the MANO forward kinematics (csrc/mano.hip: mano_shape_kernel, mano_fk_kernel<1|4|16>, mano_fk_mfma_kernel;
ops.Mano.shape / ops.Mano.fk), written from the kernel file's comments and csrc/rot.h::mano_rodrigues: manopth's Rodrigues (angle
|aa + 1e-8|, axis aa / angle, the quaternion (cos a/2, sin a/2 axis) normalised, the matrix as the nine quaternion products), then the chain
of tests/_mano_train_fp64.py::chain (shape blend, J, pose blend, parent table, skinning with the rest joint removed, tips, root centring,
manopth or HO3D joint order).  TEST INFRASTRUCTURE ONLY: nothing here imports ``vpho_amd.ops``.  Dtype-generic: one definition gives the
float64 reference and torch's own float32 evaluation for R.bound.  Pinned without a GPU by tests/test_mano_fk_fp64_cpu.py (scipy rotations
in a parent-table LBS, the oracle's manopth restatement, oracle.vpho.joints_ho3d), which also asserts what the case lists below claim.

Betas and the HO3D flag are per IMAGE: hand h belongs to image h // hands_per_image, there are ceil(n / hands_per_image) images and the
last one may be partly filled."""
import collections

import torch

from tests import _leaf_fp64 as R
from tests import _mano_train_fp64 as T


def rodrigues(aa):
    """(..., 3) axis-angle -> (..., 3, 3), manopth's batch_rodrigues + quat2mat as rot.h::mano_rodrigues states them"""
    angle = (aa + 1e-8).norm(dim=-1, keepdim=True)
    axis = aa / angle
    half = angle * 0.5
    q = torch.cat([torch.cos(half), torch.sin(half) * axis], -1)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    m = torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                     2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                     2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], -1)
    return m.reshape(*aa.shape[:-1], 3, 3)


def n_images(n, hands_per_image):
    return (n + hands_per_image - 1) // hands_per_image


def shape(mano, betas):
    """betas (n_img, 10) -> v_shaped (n_img, 778, 3), J (n_img, 16, 3)"""
    return T.shape_blend(mano, betas)


CHUNK = 1032            # hands per evaluation of the chain: every hand is independent, the skinning transforms of 4 128 hands at once are not needed


def fk(mano, pose, betas, hands_per_image, is_ho3d=None):
    """pose (n, 48) axis-angle rows, betas (n_img, 10), is_ho3d (n_img,) or None -> root-centred verts (n, 778, 3), joints (n, 21, 3), metres"""
    n = pose.shape[0]
    assert pose.shape == (n, 48) and betas.shape == (n_images(n, hands_per_image), 10)
    img = torch.arange(n) // hands_per_image
    verts, joints = [], []
    for s in range(0, n, CHUNK):
        i = img[s:s + CHUNK]
        v, j = T.chain(mano, rodrigues(pose[s:s + CHUNK].reshape(-1, 16, 3)), betas[i], None if is_ho3d is None else is_ho3d[i])
        verts.append(v)
        joints.append(j)
    return torch.cat(verts), torch.cat(joints)


# ------------------------------------------------------------------------------------------------ the host's dispatch (vpho_mano_fk_f32)
MH = 32                 # hands per workgroup of the matrix-core kernel
BLOCK = {'<1>': 1, '<4>': 4, '<16>': 16, 'mfma': MH}


def fk_form(n, hands_per_image, want_verts=True, has_table=True):
    """which kernel a launch runs: the matrix-core one when vertices are wanted, the tiled table is there, n >= 4096 and at least 16 hands
    share an image; otherwise the packed kernel with 16 hands per block from 1 024 hands, 4 from 128, 1 below"""
    if want_verts and has_table and n >= 4096 and hands_per_image >= MH // 2:
        return 'mfma'
    return '<16>' if n >= 1024 else '<4>' if n >= 128 else '<1>'


Case = collections.namedtuple('Case', 'n hpi form want_verts has_table meets')


def _case(n, hpi, form, *meets, want_verts=True, has_table=True):
    return Case(n, hpi, form, want_verts, has_table, frozenset(meets))


# what a case claims in ``meets`` (asserted in tests/test_mano_fk_fp64_cpu.py): 'ragged' -- the last block is not full; 'partial' -- the last
# image is partly filled; 'straddle' -- a block holds hands of two images; 'three' -- a block holds hands of three images
CASES = [
    _case(1, 1, '<1>'),
    _case(21, 7, '<1>'),
    _case(127, 1, '<1>'),                                             # the last launch below 128 hands
    _case(128, 4, '<4>'),                                             # the first at 128: exact blocks, one image each
    _case(130, 13, '<4>', 'ragged', 'straddle'),                      # last block of 2
    _case(1023, 31, '<4>', 'ragged', 'straddle'),                     # the last below 1 024
    _case(1024, 16, '<16>'),
    _case(1030, 1030, '<16>', 'ragged'),                              # one image, last block of 6
    _case(4100, 15, '<16>', 'ragged', 'partial', 'straddle'),         # 15 hands per image: refused by the matrix-core clause
    _case(4095, 16, '<16>', 'ragged', 'partial'),                     # 4 095 hands: refused by count
    _case(4128, 24, '<16>', 'straddle', has_table=False),             # posedirs_mfma = NULL
    _case(4128, 24, '<16>', 'straddle', want_verts=False),            # joints only
    _case(4096, 16, 'mfma', 'straddle'),                              # two images per block, exact blocks
    _case(4128, 24, 'mfma', 'straddle'),                              # 129 exact blocks
    _case(4100, 31, 'mfma', 'ragged', 'partial', 'straddle'),         # last block of 4
    _case(4100, 4100, 'mfma', 'ragged'),                              # one image
    # A 32-hand block holds hands of three images only if it starts 1 .. 31 - hands_per_image hands before an image begins: never with 24
    # or 30 hands per image (a block starts at a multiple of 32) and never with 31.  21 hands per image: 61 of the 129 blocks do.
    _case(4128, 21, 'mfma', 'partial', 'straddle', 'three'),
]


def find(n, hpi, form, want_verts=True, has_table=True):
    return next(c for c in CASES if (c.n, c.hpi, c.form, c.want_verts, c.has_table) == (n, hpi, form, want_verts, has_table))


KINDS = ('randn', 'so3', 'wide', 'small')
# every case gets 'randn'; each other kind runs on one case per form
KIND_CASES = [find(127, 1, '<1>'), find(130, 13, '<4>'), find(4100, 15, '<16>'), find(4100, 31, 'mfma')]
# the HO3D flags, mixed per image, run on one case per form; the matrix-core one has the three-image blocks
HO3D_CASES = [find(21, 7, '<1>'), find(130, 13, '<4>'), find(4100, 15, '<16>'), find(4128, 21, 'mfma')]
KIND_RUNS = [(c, k) for k in KINDS[1:] for c in KIND_CASES]
RUNS = [(c, 'randn') for c in CASES] + KIND_RUNS


def case_id(c):
    return f'n{c.n}-per{c.hpi}-{c.form}' + ('' if c.want_verts else '-jointsonly') + ('' if c.has_table else '-notable')


def run_id(run):
    return f'{case_id(run[0])}-{run[1]}'


SMALL_ROWS = ('zero', '1e-7', '1e-4', 'root')


def small_row_kind(h):
    """the 'small' kind's row type of hand h: it advances by one from a 32-hand group to the next, so over four consecutive blocks of 4,
    16 or 32 hands every block position holds each type"""
    return (h + h // MH) % 4


def make_betas(n_img, g):
    """randn * 0.8; image 1 has betas 0 and image 2 three times its betas, where they exist"""
    betas = torch.randn(n_img, 10, generator=g) * 0.8
    if n_img >= 2:
        betas[1] = 0.0
    if n_img >= 3:
        betas[2] *= 3.0
    return betas


def make(case, kind):
    """float32 CPU inputs of one run: pose (n, 48), betas (n_img, 10); cases of one (n, hands per image) share them"""
    g = R.gen(10 * (case.n * 4099 + case.hpi) + KINDS.index(kind))
    n = case.n
    if kind == 'randn':
        pose = torch.randn(n, 48, generator=g) * 0.5
    elif kind == 'wide':
        pose = torch.randn(n, 48, generator=g) * 1.5
    elif kind == 'so3':
        from oracle.rotations import matrix_to_axis_angle
        pose = matrix_to_axis_angle(T.random_rotations(n * 16, g)).reshape(n, 48).float()
    elif kind == 'small':
        a, b, c = (torch.randn(n, 48, generator=g) * s for s in (1e-7, 1e-4, 0.5))
        c[:, 3:] = 0.0
        k = small_row_kind(torch.arange(n))[:, None]
        pose = torch.where(k == 0, torch.zeros(n, 48), torch.where(k == 1, a, torch.where(k == 2, b, c)))
    else:
        raise ValueError(kind)
    return pose.contiguous(), make_betas(n_images(n, case.hpi), g)


def ho3d_flags(n_img):
    """mixed per image: every third image, the first included"""
    return (torch.arange(n_img) % 3 == 0).to(torch.uint8)


def block_images(case, block=None):
    """(first image, last image) of every block of the case's kernel"""
    hb = BLOCK[case.form] if block is None else block
    first = torch.arange(0, case.n, hb)
    last = torch.clamp(first + hb - 1, max=case.n - 1)
    return first // case.hpi, last // case.hpi


def planted(case):
    """hands that get a non-finite pose value: NaN at the first position of a block that holds hands of more than one image, at a middle
    position of the block after it and at the last position of the block after that; +inf in the last hand of the launch.  -> (nan rows,
    inf rows)"""
    hb = BLOCK[case.form]
    lo, hi = block_images(case)
    b = int(torch.nonzero(hi > lo)[0])
    rows = [b * hb, (b + 1) * hb + hb // 2, (b + 2) * hb + hb - 1]
    assert rows[-1] < case.n - 1
    return rows, [case.n - 1]

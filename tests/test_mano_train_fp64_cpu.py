"""The MANO training reference of tests/_mano_train_fp64.py pinned without a GPU against the oracle's chain in float64, as it is:
rotation_6d_to_matrix -> matrix_to_axis_angle -> oracle.mano.get_hand_verts (manopth's layer restated: Rodrigues, the level-by-level chain,
skinning), plus oracle.vpho.joints_ho3d for HO3D hands -- vertices, joints, losses and both gradients to 1e-9 of their scale, arbitrary
axes, angles 0.05 .. 2.5 rad (the oracle's chain goes through the axis-angle, whose conversion loses accuracy towards pi and is not
differentiable at 0; the reference and the kernel never form it).  A wrong reference must not be what tests/test_gpu_mano_train.py
measures the kernel with.

manopth's Rodrigues takes the angle as |axis_angle + 1e-8| (oracle.mano.batch_rodrigues, as in the original).  The reference as the GPU
test uses it has no such term, and sits 3e-9 .. 9e-9 (vertices) and up to 1.2e-8 (d_rot6d: the derivative of that norm, of relative size
1e-8 / angle on any axis) of the scale from the oracle -- printed below, and more than the 1e-9 asked although neither side is wrong.  So
the pin has two links, both asserted:
  * with ``rodrigues_eps=1e-8`` the reference sends its chain matrices through manopth's round trip (M.manopth_round_trip, written as axis,
    angle and Rodrigues matrix, not as the oracle's quaternion) and then equals the UNMODIFIED oracle to 1e-9 in every quantity (1e-14 measured);
  * with ``rodrigues_eps=0.0`` that round trip is the identity, and the result equals the default reference -- no round trip at all, what
    the kernel is held to -- to 1e-12 in every quantity.
The two differ by the literal 1e-8 alone."""
import pytest
import torch

from oracle import mano as OM, rotations as OR
from oracle.vpho import joints_ho3d
from tests import _leaf_fp64 as R
from tests import _mano_train_fp64 as M
from vpho_amd.assets import synthetic_assets

f64 = torch.float64


@pytest.fixture(scope='module')
def mano():
    return synthetic_assets(0)['mano']


def _oracle(mano, d, W):
    bs = d['rot6d'].shape[0]
    d6 = d['rot6d'].double().reshape(bs, 16, 6).requires_grad_(True)
    beta = d['shape'].double().requires_grad_(True)
    aa = OR.matrix_to_axis_angle(OR.rotation_6d_to_matrix(d6)).reshape(bs, 48)
    v, j = OM.get_hand_verts(mano, aa, beta)
    j = torch.where(d['is_ho3d'].bool()[:, None, None], joints_ho3d(v, j), j)
    pd6 = OR.matrix_to_rotation_6d(OR.axis_angle_to_matrix(aa.reshape(bs, 16, 3))).reshape(bs, 96)
    right = d['is_right'].bool()
    L = torch.stack([W[0] * ((v - d['gt_vert'].double()) ** 2).mean(), W[1] * ((j - d['gt_joint'].double()) ** 2).mean(),
                     W[2] * ((pd6 - d['gt_rot6d'].double()) ** 2).mean(),
                     W[3] * ((beta[right] - d['gt_shape'].double()[right]) ** 2).sum() / (10.0 * bs)])
    g6, gb = torch.autograd.grad(L.sum(), [d6, beta])
    return L.detach(), g6.reshape(bs, 96), gb, v.detach(), j.detach()


def _inputs(bs, seed, right, ho3d, sheared):
    """M.make with the rotations replaced by ones of angle 0.05 .. 2.5 rad about arbitrary axes, no identity hand"""
    d = M.make(bs, seed, right, ho3d, identity_hand=False)
    g = R.gen(seed + 1000)
    Rm = M.axis_angle_rotations(bs * 16, g, 0.05, 2.5)
    d['rot6d'] = (M.sheared_6d(Rm, g) if sheared else Rm[:, :2].reshape(-1, 6)).reshape(bs, 96).float()
    assert 2.0 < M.max_angle(d['rot6d']) <= 2.5 + 1e-6
    return d


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _assert_equal(got, want, W, right, tol):
    """losses, d_rot6d, d_shape, verts, joints: each within tol of its scale; what a weight of 0 (or no right hand) makes 0 is 0 on both sides"""
    (L, g6, gb, v, j), (Lo, g6o, gbo, vo, jo) = got, want
    assert _rel(v, vo) <= tol and _rel(j, jo) <= tol, (_rel(v, vo), _rel(j, jo))
    for k in range(4):
        if W[k] == 0 or (k == 3 and right == 'none'):
            assert float(L[k]) == float(Lo[k]) == 0, M.LOSSES[k]
        else:
            assert abs(float(L[k]) - float(Lo[k])) <= tol * abs(float(Lo[k])), (M.LOSSES[k], float(L[k]), float(Lo[k]))
    for a, b in ((g6, g6o), (gb, gbo)):
        if float(b.abs().max()) == 0:
            assert float(a.abs().max()) == 0
        else:
            assert _rel(a, b) <= tol, _rel(a, b)


CASES = [(1, 'all', 'none', False), (3, 'mixed', 'mixed', True), (2, 'none', 'all', True)]
WS = [M.WEIGHTS, (1e4, 0, 0, 0), (0, 1e4, 0, 0), (0, 0, 10.0, 0), (0, 0, 0, 1.0)]


@pytest.mark.parametrize('bs,right,ho3d,sheared', CASES)
@pytest.mark.parametrize('W', WS, ids=['all', 'vert', 'joint', 'pose', 'shape'])
def test_reference_equals_the_oracles_chain_through_the_axis_angle(mano, bs, right, ho3d, sheared, W):
    """the unmodified oracle against the reference with manopth's round trip (rodrigues_eps=1e-8): every quantity to 1e-9 of its scale;
    and the same reference with the identity round trip (0.0) against the default reference: every quantity to 1e-12"""
    d = _inputs(bs, 10 * bs + len(right), right, ho3d, sheared)
    oracle, plain = _oracle(mano, d, W), M.reference(mano, d, W, f64)
    with_eps, with_zero = M.reference(mano, d, W, f64, rodrigues_eps=1e-8), M.reference(mano, d, W, f64, rodrigues_eps=0.0)
    names = ('losses', 'd_rot6d', 'd_shape', 'verts', 'joints')
    for tag, a, b in (('eps=1e-8 vs oracle', with_eps, oracle), ('eps=0 vs default', with_zero, plain), ('default vs oracle', plain, oracle)):
        print(f'PIN bs{bs} {right}/{ho3d} {tag}: ' + ' '.join(f'{n} {_rel(x, y):.1e}' for n, x, y in zip(names, a, b) if float(y.abs().max()) > 0))
    _assert_equal(with_eps, oracle, W, right, 1e-9)
    _assert_equal(with_zero, plain, W, right, 1e-12)


def test_the_round_trip_is_manopths_and_moves_a_rotation_by_at_most_its_epsilon():
    """M.manopth_round_trip against oracle.mano.batch_rodrigues on the axis-angle of the same matrices (1e-13), the identity without the
    epsilon (1e-13), and within sqrt(3) 1e-8 rad of it with"""
    Rm = M.axis_angle_rotations(200, R.gen(1), 0.05, 2.5)
    aa = OR.matrix_to_axis_angle(Rm)
    assert float((M.manopth_round_trip(Rm, 1e-8) - OM.batch_rodrigues(aa).view(-1, 3, 3)).abs().max()) <= 1e-13
    assert float((M.manopth_round_trip(Rm, 0.0) - Rm).abs().max()) <= 1e-13
    moved = float((M.manopth_round_trip(Rm, 1e-8) - Rm).abs().max())
    assert 1e-9 < moved <= 3 ** 0.5 * 1e-8, moved


def test_no_right_hand_the_empty_mean_is_nan_and_the_reference_says_zero(mano):
    """the project this was modelled on takes mse_loss of the right hands' rows: with none that is the mean of an empty tensor, NaN.
    The kernel's defined result -- and this reference's -- is a zero shape loss and no shape term in d_shape."""
    d = M.make(2, 5, right='none')
    assert bool(torch.isnan(torch.nn.functional.mse_loss(d['shape'][d['is_right'].bool()], d['gt_shape'][d['is_right'].bool()])))
    L, _, gb, _, _ = M.reference(mano, d, (0, 0, 0, 1.0), f64)
    assert float(L[3]) == 0.0 and float(gb.abs().max()) == 0.0


def test_inputs_are_what_the_gpu_test_says_they_are():
    d = M.make(5, 3)
    assert M.max_angle(d['rot6d']) > 3.0                                        # 80 uniform rotations: some within 0.15 rad of pi
    a = d['rot6d'].double().reshape(5, 16, 6)
    assert torch.equal(a[-1], torch.tensor(M.IDENTITY_6D, dtype=f64).repeat(16, 1))
    a1, a2 = a[:-1, :, :3], a[:-1, :, 3:]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    ratio = u.norm(dim=-1) / a2.norm(dim=-1)
    assert float(ratio.min()) >= 0.2 and float(a1.norm(dim=-1).min()) >= 0.2 - 1e-6 and float(a1.norm(dim=-1).max()) <= 4 + 1e-6
    assert float((b1 * a2).sum(-1).abs().max()) > 1.0                           # really sheared
    assert M.flags('mixed', 5).tolist() == [1, 0, 1, 0, 1] and M.flags('none', 3).sum() == 0 and M.flags('all', 3).sum() == 3

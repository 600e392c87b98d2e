"""The training-mode MANO head (csrc/mano_train.hip, ops.Mano.train: one kernel runs Gram-Schmidt, blend shapes, the 16-joint chain, skinning
and four losses, then the whole backward by hand) against float64 autograd of tests/_mano_train_fp64.py (pinned to the oracle's chain
without a GPU by tests/test_mano_train_fp64_cpu.py) on the float32 inputs the kernel saw.

One loss weight at a time -- (w,0,0,0), (0,w,0,0), (0,0,w,0), (0,0,0,w) -- so that a wrong mano_pose or mano_shape term is not hidden
under the vertex-loss gradient, then the training step's weights together; each loss, d_rot6d and d_shape held to R.bound on its own scale
(4 x torch's own float32 CPU error against float64, floor 4 ulp of the largest value), every element compared.  Rotations are uniform over
SO(3) -- the kernel never forms the axis-angle, so angles near pi are fair --, written as 6-vectors scaled by 0.2 .. 4 and sheared
(|u| / |a2| >= 0.2); the last hand of a batch of more than one holds exact identity 6-vectors, where the pose feature is 0."""
import pytest
import torch

from tests import _leaf_fp64 as R
from tests import _mano_train_fp64 as M

pytestmark = pytest.mark.gpu

WS = {'vert': (1e4, 0.0, 0.0, 0.0), 'joint': (0.0, 1e4, 0.0, 0.0), 'pose': (0.0, 0.0, 10.0, 0.0), 'shape': (0.0, 0.0, 0.0, 1.0), 'all': M.WEIGHTS}


@pytest.fixture(scope='module')
def mano(assets):
    return assets['mano']                                                        # synthetic_assets(0)['mano']


@pytest.fixture(scope='module')
def hand(mano):
    from vpho_amd import ops
    return ops.Mano(mano, 'cuda')


def _train(hand, d, W, want_outputs=False, ho3d=True):
    c = lambda t: t.cuda().contiguous()
    out = hand.train(*(c(d[k]) for k in M.ARGS), W, want_outputs=want_outputs, is_ho3d=c(d['is_ho3d']) if ho3d else None)
    return (torch.stack([out[0][k] for k in M.LOSSES]),) + tuple(out[1:])


_REF = {}


def _reference(mano, key, d, W):
    """float64 reference and float32 evaluation of one (inputs, weights) pair, computed once and shared (never modified)"""
    if (key, W) not in _REF:
        _REF[(key, W)] = (M.reference(mano, d, W, torch.float64), M.reference(mano, d, W, torch.float32))
    return _REF[(key, W)]


def _check_all(name, got, ref, f32):
    """losses one by one, d_rot6d, d_shape to R.bound; verts and joints within 2e-6 m"""
    L, d6, db = got[:3]
    for k, loss in enumerate(M.LOSSES):
        R.check(f'{name} {loss}', L[k:k + 1], ref[0][k:k + 1], R.bound(f32[0][k:k + 1], ref[0][k:k + 1]))
    R.check(f'{name} d_rot6d', d6, ref[1], R.bound(f32[1], ref[1]))
    R.check(f'{name} d_shape', db, ref[2], R.bound(f32[2], ref[2]))
    R.check(f'{name} verts', got[3], ref[3], 2e-6)
    R.check(f'{name} joints', got[4], ref[4], 2e-6)


@pytest.mark.parametrize('bs', [1, 5, 66])
@pytest.mark.parametrize('wk', list(WS))
def test_each_loss_alone_then_together_against_float64_autograd(hand, mano, bs, wk):
    """bs = 1 (one workgroup, sheared uniform rotations), 5 and 66 (more workgroups than the training batch of 64; the last hand is the
    identity pose); is_right and the HO3D flag alternate.  With one weight the other three losses are exactly 0 and -- pose or shape
    alone -- so is the gradient the loss does not reach (d_shape, d_rot6d): the bound is 0 there and the kernel must give 0."""
    d = M.make(bs, 100 + bs, identity_hand=bs > 1)
    ref, f32 = _reference(mano, ('main', bs), d, WS[wk])
    got = _train(hand, d, WS[wk], want_outputs=True)
    _check_all(f'mano bs{bs} {wk}', got, ref, f32)
    for k in range(4):
        if WS[wk][k] == 0:
            assert float(got[0][k]) == 0.0 == float(ref[0][k])
    if wk == 'pose':
        assert float(ref[2].abs().max()) == 0 and float(got[2].abs().max()) == 0
    if wk == 'shape':
        assert float(ref[1].abs().max()) == 0 and float(got[1].abs().max()) == 0


@pytest.mark.parametrize('right', ['mixed', 'all', 'none'])
@pytest.mark.parametrize('ho3d', ['mixed', 'all', 'none'])
def test_right_hand_and_ho3d_flags(hand, mano, right, ho3d):
    """is_right mixed / all right / all left and HO3D joints mixed / all / none, bs = 5, the training step's weights and the shape loss
    alone.  With NO right hand the project this was modelled on takes the mean of an empty tensor, NaN; the kernel's defined result is a
    zero shape loss and no shape term in d_shape -- asserted: the loss is exactly 0 and d_shape has the bits of a run with w_shape = 0.
    Without the flag array (is_ho3d = NULL) the kernel gives the bits of an all-zero one."""
    d = M.make(5, 7, right=right, ho3d=ho3d)
    for wk in ('all', 'shape', 'joint'):
        ref, f32 = _reference(mano, ('flags', right, ho3d), d, WS[wk])
        got = _train(hand, d, WS[wk], want_outputs=True)
        _check_all(f'mano right={right} ho3d={ho3d} {wk}', got, ref, f32)
    got = _train(hand, d, WS['all'])
    if right == 'none':
        assert float(got[0][3]) == 0.0 and bool(torch.isfinite(got[2]).all())
        w0 = _train(hand, d, M.WEIGHTS[:3] + (0.0,))
        assert R.bits_equal(got[2], w0[2]) and R.bits_equal(got[1], w0[1])
        assert float(_train(hand, d, WS['shape'])[2].abs().max()) == 0.0
    else:
        assert float(got[0][3]) > 0.0
    if ho3d == 'none':
        null = _train(hand, d, WS['all'], ho3d=False)
        assert all(R.bits_equal(a, b) for a, b in zip(got[1:], null[1:])) and torch.equal(got[0], null[0])


@pytest.mark.parametrize('bs', [1, 5, 66])
def test_want_outputs_changes_nothing_and_launches_repeat(hand, bs):
    """want_outputs=False (what the training step calls) gives the same bits of losses and gradients as want_outputs=True, and a second
    launch the same bits again (every reduction has a fixed order)"""
    d = M.make(bs, 100 + bs, identity_hand=bs > 1)
    a, b, c = _train(hand, d, M.WEIGHTS, want_outputs=True), _train(hand, d, M.WEIGHTS), _train(hand, d, M.WEIGHTS, want_outputs=True)
    assert torch.equal(a[0], b[0]) and R.bits_equal(a[1], b[1]) and R.bits_equal(a[2], b[2])
    assert torch.equal(a[0], c[0]) and all(R.bits_equal(x, y) for x, y in zip(a[1:], c[1:]))


@pytest.mark.parametrize('bs', [5, 66])
def test_permuted_batch_gives_permuted_gradients_bit_for_bit(hand, bs):
    """one workgroup per hand and nothing shared but the batch size in the loss scale: hand i of a permuted batch gets the bits hand
    perm[i] got, gradients, vertices and joints"""
    d = M.make(bs, 100 + bs)
    perm = torch.randperm(bs, generator=R.gen(bs))
    assert not torch.equal(perm, torch.arange(bs))
    dp = {k: v[perm].contiguous() for k, v in d.items()}
    a, b = _train(hand, d, M.WEIGHTS, want_outputs=True), _train(hand, dp, M.WEIGHTS, want_outputs=True)
    for x, y in zip(a[1:], b[1:]):
        assert R.bits_equal(x.cpu()[perm], y)

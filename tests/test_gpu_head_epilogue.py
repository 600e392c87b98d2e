"""Score head: the run-layout epilogue (default) against the reference epilogue it replaced (score_head_epi0_kernel, VPHO_HEAD_EPI=0).

The two differ only in how the epilogue's operands lie in LDS and when they are requested; every floating-point operation and its order
are the same, so every comparison here is torch.equal."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def seeded(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).normal(size=shape) * scale).astype(np.float32))


@pytest.fixture(scope='module')
def nets(sd):
    from vpho_amd import ops
    return {k: ops.ScoreNet(sd, f'denoiser_{k}', 'cuda') for k in ('hand', 'obj')}


def both_epilogues(fn):
    """fn() under VPHO_HEAD_EPI=0 (reference epilogue) and with the variable unset (default); the switch is read per call"""
    res = {}
    for key in ('epi0', 'default'):
        if key == 'epi0':
            os.environ['VPHO_HEAD_EPI'] = '0'
        try:
            res[key] = fn()
            torch.cuda.synchronize()
        finally:
            os.environ.pop('VPHO_HEAD_EPI', None)
    return res['epi0'], res['default']


SHAPES = [(2, 100),      # one full 128-row tile plus a ragged one; a tile spanning two images
          (3, 64),       # the smallest sample_num on the LDS path; a tile spanning three images
          (1, 130),      # a 2-row last tile
          (7, 40),       # global-load path
          (33, 4)]       # global-load path, 33 images in one tile
CASES = [(name, D, bs, S) for name, D in (('hand', 96), ('obj', 9)) for bs, S in SHAPES]
CASES.append(('hand', 96, 3, 2129))    # the one shape with 32-row tail tiles, the last one ragged (32 heads x 50 tiles exceed the workgroup slots)


@pytest.mark.parametrize('name,D,bs,S', CASES)
def test_score_is_bit_identical_to_the_reference_epilogue(nets, name, D, bs, S):
    feat, x = seeded((bs, 1024), 80, 0.3).cuda(), seeded((bs * S, D), 81, 1.5).cuda()
    for t in (0.65, 1e-5):
        ref, got = both_epilogues(lambda: nets[name].score(feat, x, t, S).clone())
        assert torch.isfinite(got).all() and float(got.abs().max()) > 0
        assert torch.equal(ref, got), (t, float((ref - got).abs().max()))


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize('name,D', [('hand', 96), ('obj', 9)])
def test_ode_solve_is_bit_identical_to_the_reference_epilogue(sd, nets, name, D):
    """One solve of 8 x 100 rows, 12 stamps (rhs_mode, the controller's scalars, out_slot): xs, x and nfev equal.  Then NaN:

    * a NaN planted in one row of the initial state.  It stays in the state (the guard zeroes the RHS, not y), the error norm's scale
      atol + max(|y|, |y_new|) rtol is NaN, every attempt is rejected and the solve ends in `step size underflow` before any output is
      returned (measured on MI355X, both epilogues; the reference's scipy controller does not recover from it either).  So this solve can only be
      required to END the same way under both epilogues;
    * what that solve was meant to check -- nan_count and the bit patterns of both outputs -- on a solve that finishes: the same rows with
      a NaN planted in one second-layer weight of head 1.  Hidden unit 77's product is NaN for every row, travels through the partial
      sums, the cross-half shuffle and the combine of the epilogue under test, and the guard zeroes and counts the head's three entries
      at every RHS evaluation, so the state stays finite."""
    from vpho_amd import ops
    init, feat8 = seeded((8 * 100, D), 82, 20.0).cuda(), seeded((8, 1024), 83, 0.3).cuda()

    def solve(net, x0):
        xs, x, st = net.sample(feat8, x0, 100, 0.65, 12, xs_f64=True)
        return xs.clone(), x.clone(), st

    ref, got = both_epilogues(lambda: solve(nets[name], init))
    assert ref[2]['nfev'] == got[2]['nfev'] and got[2]['nan_count'] == 0
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])

    planted = init.clone()
    planted[137, D // 2] = float('nan')

    def outcome():
        try:
            xs, x, st = solve(nets[name], planted)
        except ops.VphoError as e:
            return ('error', str(e))
        return ('ok', st['nan_count'], st['nfev'], bits(xs), bits(x))

    ref, got = both_epilogues(outcome)
    assert ref[0] == got[0] and ref[1:3] == got[1:3], (ref[:3], got[:3])
    assert all(torch.equal(a, b) for a, b in zip(ref[3:], got[3:]))

    w2 = sd[f'denoiser_{name}.head.head.2.weight'].clone()                # (n, 256, 3)
    w2[1, 77, 2] = float('nan')
    net = ops.ScoreNet({**sd, f'denoiser_{name}.head.head.2.weight': w2}, f'denoiser_{name}', 'cuda')
    ref, got = both_epilogues(lambda: solve(net, init))
    assert got[2]['nfev'] == ref[2]['nfev'] and got[2]['nan_count'] == ref[2]['nan_count'] == 800 * (got[2]['nfev'] - 1)
    assert torch.equal(bits(ref[0]), bits(got[0])) and torch.equal(bits(ref[1]), bits(got[1]))
    assert bool(torch.isnan(got[1][:, 5]).all()) and bool(torch.isfinite(got[0]).all())      # the final evaluation is not guarded (as in the reference)

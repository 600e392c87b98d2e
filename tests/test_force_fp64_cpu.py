"""The float64 reference of the force optimiser's GPU tests (tests/_force_fp64.py), pinned on the CPU: it is the loop the reference
fixture records, it stays finite on the degenerate rows, it obeys the invariants of an anchor out of contact, and on every long case its
own float32 noise is at least ten times smaller than what a wrong step count, a missing moment reset or a stale bias-correction table
would do to it -- so the GPU tests of those cases can tell such a kernel from a right one.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import _force_fp64 as R

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'golden_force_optim.npz')


def test_float32_path_is_the_reference_fixture_and_float64_stays_with_it(assets):
    """golden_force_optim.npz is the reference's own ForceOptimizer.optimize_batch: the float32 path reproduces it to the tolerances of
    test_oracle_golden.py (1e-6 after 40 steps, 1e-4 after 400); the float64 path is within `noise` (its distance to the float32
    path) plus that tolerance of it, and `noise` stays small at lr = 1e-3 up to 400 steps (measured 7e-10 / 2e-5 in scale / weight
    after 40 steps, 5e-6 / 5e-5 after 400 -- two float32 runs agree far better with each other than either does with float64)."""
    g = np.load(GOLDEN)
    B, seed = int(g['B']), int(g['seed'])
    ins = R.inputs(assets, B, seed)
    for iters, tol in ((40, 1e-6), (400, 1e-4)):
        r32 = R.reference(ins, iters, 300, 1e-3, torch.float32)
        r64 = R.reference(ins, iters, 300, 1e-3, torch.float64)
        n = R.noise(r64, r32)
        for k in ('scale', 'weight'):
            e32, e64 = np.abs(r32[k] - g[f'{k}_{iters}']).max(), np.abs(r64[k] - g[f'{k}_{iters}']).max()
            print(iters, k, 'float32 vs fixture', e32, 'float64 vs fixture', e64, 'noise', n[k])
            assert e32 < tol, (iters, k, e32)
            assert e64 <= n[k] + tol, (iters, k, e64, n[k])
        assert n['scale'] < 1e-4 and n['weight'] < 1e-3, n            # lr = 1e-3 is not yet chaotic at 400 steps (1100: 1.5e-2)
    np.testing.assert_allclose(r64['force_point'], g['force_point'], rtol=1e-5, atol=1e-7)
    assert torch.get_default_dtype() == torch.float32


def test_manual_loop_is_the_oracle():
    """the hand-written AdamW the mutations are applied to IS torch.optim.AdamW: the same numbers in either dtype (1e-12 of float64
    rounding, 1e-7 in float32 allowed; they are equal to the bit on this build)"""
    ins = R.build('degenerate', 9, 1, R.SEED)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-7)):
        for iters, phase1 in ((30, 12), (5, 0), (7, 9)):
            d = R.max_abs(R.reference(ins, iters, phase1, 1e-3, dtype), R.manual_loop(ins, iters, phase1, 1e-3, dtype))
            assert max(d.values()) <= tol, (dtype, iters, phase1, d)


@pytest.mark.parametrize('B,n_batches', [(1, 7), (4, 2), (17, 2), (64, 2)])
def test_float64_reference_is_finite_on_every_degenerate_row(B, n_batches):
    ins = R.build('degenerate', B, n_batches, R.SEED)
    fc, grav, grasped = ins[3], ins[1], ins[4]
    in_contact = R.contact_mask(fc).sum(1)
    assert (in_contact == 0).any()
    if B >= len(R.PATTERNS) or n_batches >= len(R.PATTERNS):            # every pattern is some sample's
        assert (in_contact == 1).any() and (in_contact == 32).any() and (fc == 1e3).any() and (fc.sum(1) == 0).any()
    assert (grav.abs().sum((1, 2)) == 0).any()
    assert grasped[:B].all() and not grasped[B:2 * B].any()
    r = R.reference_batches(ins, B, 12, 5, 1e-3)
    for k in R.OUTPUTS:
        assert np.isfinite(r[k]).all(), k
    assert r['loss_force'].shape == (n_batches,)


def test_the_float64_run_keeps_the_float32_mask():
    """float32(0.1) and the float32 below it are no contact, the float32 above it is: in the float64 run too (module docstring)"""
    ins = R.build('degenerate', 7, 1, R.SEED)
    fc = ins[3]
    row = R.PATTERNS.index('threshold')
    t = np.float32(0.1)
    assert fc[row, 3].item() == float(t) and fc[row, 4].item() > float(t) > fc[row, 5].item()
    assert R.contact_mask(fc)[row, 3:6].tolist() == [False, True, False]
    r = R.reference(ins, 6, 2, 1e-3)
    moved = np.abs(r['weight'][row]).max(-1) > 0
    assert moved[3:6].tolist() == [False, True, False] and moved[19:22].tolist() == [False, True, False]


@pytest.mark.parametrize('iters,phase1,lr', [(1, 0, 1e-3), (1, 1, 1e-3), (2, 1, 1e-3), (40, 39, 1e-3), (40, 40, 1e-3), (40, 1000, 1e-3), (120, 0, 1e-3),
                                             (300, 100, 1e-5)])
def test_masked_anchor_invariants(iters, phase1, lr):
    """Derived, not measured.  An anchor out of contact has scale * mask = 0, so no force and no gradient: its `weight` row stays exactly
    0 (decay of 0, Adam step of 0 / (0 + eps)), and its `scale` only decays, by 1 - lr * 0.01 per step of the SECOND optimiser (the
    first one does not hold `scale`): 0.05 * (1 - lr * 0.01) ** max(0, iters - phase1).  This pins weight decay and the phase-2 step
    count whatever Adam does to the anchors in contact."""
    for kind, B in (('plain', 5), ('degenerate', 17)):
        ins = R.build(kind, B, 1, R.SEED)
        out = ~R.contact_mask(ins[3]).numpy()
        assert out.any() and not out.all()
        r = R.reference(ins, iters, phase1, lr)
        assert (r['weight'][out] == 0).all()
        want = R.masked_scale(iters, phase1, lr)
        assert np.abs(r['scale'][out] - want).max() <= 4 * np.finfo(np.float64).eps * 0.05 * max(1, iters - phase1)
        if phase1 >= iters:
            assert (r['scale'] == 0.05).all()
        assert (np.abs(r['weight'][~out]).max(-1) > 0).all()          # and the anchors in contact did move


@pytest.mark.parametrize('iters,phase1,lr', R.TABLE)
def test_long_cases_are_quieter_than_the_mutations(iters, phase1, lr):
    """The small-lr property.  For each mutation of the loop, the largest shift over the outputs in units of max(noise, floor) must be at
    least 10: then a tolerance of a few units still fails a kernel that does what the mutation does.  `stale_table` (bias corrections
    not refilled after 1024 iterations) is asked of the cases that run at least 76 iterations on the second table; after one such
    iteration (1025) a 20 % error of a single 1e-5 step is below the noise -- that case is there for slot 0 of the fresh table being
    read at all."""
    ins, r64, r32 = R.case('plain', R.TABLE_B, 1, iters, phase1, lr, R.SEED)
    u = R.units(r64, r32)
    muts = [m for m in R.MUTATIONS if m != 'stale_table' or iters >= 1100]
    assert len(muts) >= 2
    for mut in muts:
        shift = R.max_abs(R.manual_loop(ins, iters, phase1, lr, mutation=mut), r64)
        margin = max(shift[k] / u[k] for k in R.OUTPUTS)
        print(iters, phase1, lr, mut, 'margin %.1f' % margin, {k: '%.1f' % (shift[k] / u[k]) for k in R.OUTPUTS})
        assert margin >= 10, (mut, margin)

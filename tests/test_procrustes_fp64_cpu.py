"""The families of tests/_procrustes_fp64.py are what they claim, and the numpy restatement of the device solve agrees with the SVD within
the tolerances the GPU tests use (tests/test_gpu_procrustes.py).  No GPU."""
import numpy as np
import pytest

import tests._procrustes_fp64 as P

SEED = 0


@pytest.fixture(scope='module')
def cases():
    return {(f, n): P.family(f, n, SEED) for f, n in P.cells()}


def test_the_cells_are_every_family_at_every_point_count():
    assert len(P.cells()) == 11 * 6 + 4 and len(set(P.cells())) == len(P.cells())
    assert set(P.families(21, SEED)) == set(P.GENERAL) and set(P.families(8, SEED)) == {'cube', 'cube_rot', 'cube_mirror_noise'}
    assert set(P.families(6, SEED)) == {'octa_rot_noise'}
    for (pd, gt) in P.families(65, SEED).values():
        assert pd.dtype == gt.dtype == np.float32 and pd.shape == gt.shape == (65, 3)
        assert 0.4 < pd[:, 2].mean() < 1.3 and 0.6 < gt[:, 2].mean() < 0.8 and np.ptp(gt, 0).max() < 0.2          # camera-space magnitudes
    a, b = P.family('thin', 21, 3), P.family('thin', 21, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])                                               # seeded


def test_singular_value_ratios_are_in_the_stated_ranges(cases):
    for (f, n), (pd, gt) in cases.items():
        s = P.singular_values(pd, gt)
        if f in P.RANK2 or n == 3:                                     # three points span a plane whatever the family
            assert s[2] / s[0] < 1e-6, (f, n, s)
        if f in P.RANK2 and n > 3:
            assert s[1] / s[0] > 1e-3, (f, n, s)                        # ... and no less than rank 2
        if f in P.RANK1:
            assert s[1] / s[0] < 1e-5, (f, n, s)
        if f in P.SYMMETRIC:
            assert s[2] / s[0] > 0.9, (f, n, s)
        if f in ('generic', 'mirror', 'similarity') and n >= 21:
            assert s[2] / s[0] > 1e-2, (f, n, s)
        if f in P.EXACT_PLANAR:
            flat = pd if f != 'gt_planar' else gt
            assert (flat[:, 2] == flat[0, 2]).all()                    # exactly: one coordinate constant


def test_reflection_and_rank_deficient_branches_are_taken(cases):
    info = {k: P.device_error(*v)[1] for k, v in cases.items()}
    refl = {k: P.svd_transform(*v)[2] for k, v in cases.items()}
    for n in (21, 65, 257, 778):
        assert refl[('mirror', n)] and info[('mirror', n)]['reflected']                 # a mirrored full-rank cloud: both routes reflect
    assert refl[('cube_mirror_noise', 8)] and info[('cube_mirror_noise', 8)]['reflected']
    assert any(refl[(f, n)] and info[(f, n)]['reflected'] for f in P.EXACT_PLANAR for n in P.POINT_COUNTS)
    assert any(info[('pd_planar_rot', n)]['reflected'] for n in P.POINT_COUNTS)        # decided on a third singular value ~1e-8 s1
    for f in P.EXACT_PLANAR:
        for n in P.POINT_COUNTS:
            assert info[(f, n)]['completed'], (f, n)                                   # |H v3| is no direction: U[:,2] = U0 x U1
    assert not any(info[('generic', n)]['completed'] for n in (21, 65, 257, 778))
    # rank 1 exactly (all ground-truth points on a coordinate axis): U[:,1] is an arbitrary perpendicular, and the error is still the SVD's
    pd, gt = P.family('generic', 21, SEED)
    gt = gt.copy()
    gt[:, 1:] = gt[0, 1:]
    got, i = P.device_error(pd, gt)
    assert i['perp'] and abs(got - P.align_error(pd, gt)) <= P.ATOL_RANK1


def test_align_error_is_the_oracle_rule_and_invariant_under_similarity(cases):
    from oracle import metrics as OM
    rng = np.random.default_rng(1)
    for (f, n) in (('generic', 21), ('mirror', 65), ('both_planar', 257), ('gt_collinear', 4), ('cube_rot', 8)):
        pd, gt = cases[(f, n)]
        ref = OM.mje_pamje(gt.astype(np.float64), pd.astype(np.float64))[1]
        assert abs(P.align_error(pd, gt) - ref) <= 1e-15
        moved = 0.6 * pd.astype(np.float64) @ P._rot(rng).T + rng.normal(size=3) * 0.1      # float64: the invariance itself, no rounding
        assert abs(P.align_error(moved, gt) - ref) <= 1e-12, (f, n)
    pd, gt = cases[('similarity', 778)]
    assert P.align_error(pd, gt) < 1e-7 < P.mean_error(pd, gt)                                # a similarity copy aligns to fp32 rounding


def test_postprocess_round_trip_keeps_a_constant_coordinate():
    pd, _ = P.family('pd_planar', 65, SEED)
    for right in (True, False):
        cam = P.postprocess(P.to_model(pd, P.ROOT_JOINT, right), P.ROOT_JOINT, right)
        assert np.abs(cam - pd).max() < 2e-7 and (cam[:, 2] == cam[0, 2]).all()


def test_restated_solve_agrees_with_the_svd_within_the_gpu_tolerances():
    """the figures behind ATOL and ATOL_RANK1: ten times the largest difference measured here is at most the tolerance, over eight
    seeds; the solve as it was before U was orthonormal by construction misses the rank-1 tolerance by orders of magnitude on
    gt_collinear and nowhere else by more than 2e-9"""
    worst, legacy = {}, {}
    for seed in range(8):
        for f, n in P.cells():
            pd, gt = P.family(f, n, seed)
            ref = P.align_error(pd, gt)
            worst[f] = max(worst.get(f, 0.0), abs(P.device_error(pd, gt)[0] - ref))
            legacy[f] = max(legacy.get(f, 0.0), abs(P.device_error(pd, gt, legacy=True)[0] - ref))
    print({f: f'{v:.1e}' for f, v in worst.items()}, {f: f'{v:.1e}' for f, v in legacy.items()})
    for f, v in worst.items():
        assert 10 * v <= P.atol_of(f), (f, v)
    assert P.ATOL == 1e-9 and P.ATOL_RANK1 <= 1e-7
    assert legacy['gt_collinear'] > 1e-5
    assert all(v < 2e-9 for f, v in legacy.items() if f != 'gt_collinear')

"""csrc/contact.hip on inputs whose fp32 arithmetic is exact (tests/_contact_lattice.py): the float64 oracle is then exact too, and every
element is compared -- indices and the in/out pattern for equality, weights to rtol 2e-7 (a float64 weight rounded to fp32 once).  Nothing
is excluded.  The sizes put queries on the first and last point of a 1024-point LDS tile, on the first point of the next, on the last
point of a partial tile and on the last lane of a 256-query block; tests/test_contact_lattice_cpu.py holds the constructions' claims."""
import numpy as np
import pytest
import torch

import tests._contact_lattice as CL
from oracle import contact as OC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def agg(assets):
    from vpho_amd import ops
    from vpho_amd.assets import ANCHOR_SKELETON
    return ops.Aggregation(assets, ANCHOR_SKELETON, DEV)


def _dev(*arrays):
    return [torch.as_tensor(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _stack(cases, *keys):
    return [np.stack([c[k] for c in cases]) for k in keys]


def _oracle(c, displaced_is_hand):
    f = lambda k: c[k].astype(np.float64)
    if displaced_is_hand:
        return OC.detect(f('queries'), f('query_normals'), f('targets'), f('target_normals'), **CL.KW)
    return OC.detect(f('targets'), f('target_normals'), f('queries'), f('query_normals'), **CL.KW)


def _run(agg, cases, displaced_is_hand):
    t, tn, q, qn = _stack(cases, 'targets', 'target_normals', 'queries', 'query_normals')
    args = (q, qn, t, tn) if displaced_is_hand else (t, tn, q, qn)
    hc, oc, o2h = agg.contact_detect(*_dev(*args), **CL.KW)
    assert hc.dtype == oc.dtype == torch.float32 and o2h.dtype == torch.int32
    return hc.cpu().numpy(), oc.cpu().numpy(), o2h.cpu().numpy()


def _same_weights(got, ref, what):
    assert np.array_equal(got > 0, ref > 0), (what, np.flatnonzero((got > 0) != (ref > 0))[:8])
    np.testing.assert_allclose(got, ref, rtol=2e-7, atol=0, err_msg=what)


@pytest.mark.parametrize('nq,nt', CL.SEAM_SIZES)
def test_seam_case_both_roles(agg, nq, nt):
    """three samples of different seeds in one launch.  With the lattice as the hand, the object-to-hand direction reports the index of
    every displaced point: it must be its own target.  With the roles swapped the displaced points are scanned as targets in tiles and
    the lattice as queries in blocks, so each direction sees each size.  All six outputs against the oracle, every element."""
    cases = [CL.seam_case(nq, nt, seed) for seed in range(3)]
    own, nd = _stack(cases, 'own', 'nd')
    closed = CL.closed_form_weight(nd)
    hc, oc, o2h = _run(agg, cases, displaced_is_hand=False)
    assert hc.shape == (3, nt) and oc.shape == o2h.shape == (3, nq)
    assert np.array_equal(o2h, own)
    _same_weights(oc, closed, 'displaced points as the object')
    for i, c in enumerate(cases):
        ref_h, ref_o, ref_i = _oracle(c, False)
        _same_weights(hc[i], ref_h, 'lattice as the hand')
        assert np.array_equal(ref_o, closed[i]) and np.array_equal(ref_i, own[i])
    hc, oc, o2h = _run(agg, cases, displaced_is_hand=True)
    assert hc.shape == (3, nq) and oc.shape == o2h.shape == (3, nt)
    _same_weights(hc, closed, 'displaced points as the hand')
    for i, c in enumerate(cases):
        ref_h, ref_o, ref_i = _oracle(c, True)
        _same_weights(oc[i], ref_o, 'lattice as the object')
        assert np.array_equal(o2h[i], ref_i), np.flatnonzero(o2h[i] != ref_i)[:8]


def test_gate_case_strict_gates_and_both_flanks(agg):
    c = CL.gate_case()
    _, oc, o2h = _run(agg, [c], displaced_is_hand=False)
    inside = c['inside']
    assert np.array_equal(o2h[0] >= 0, inside) and (o2h[0][~inside] == -1).all() and np.array_equal(o2h[0][inside], c['own'][inside])
    assert (oc[0][~inside] == 0).all()
    _same_weights(oc[0], np.where(inside, CL.closed_form_weight(c['nd']), 0.0), 'gate_case as the object')
    ref = _oracle(c, False)
    assert np.array_equal(o2h[0], ref[2])
    hc, _, _ = _run(agg, [c], displaced_is_hand=True)
    _same_weights(hc[0], _oracle(c, True)[0], 'gate_case as the hand')
    assert np.array_equal(hc[0] > 0, inside)


@pytest.mark.parametrize('second', (9, 1030))
def test_tie_takes_the_smaller_index(agg, second):
    c = CL.tie_case(second)
    _, oc, o2h = _run(agg, [c], displaced_is_hand=False)
    assert (o2h[0][:32] == 5).all() and np.array_equal(o2h[0], c['own'])
    _same_weights(oc[0], CL.closed_form_weight(c['nd']), 'tie_case')


@pytest.mark.parametrize('ld', (778, 800))
@pytest.mark.parametrize('n', (1, 64, 65, 130))
def test_force_contact_groups_strides_and_strict_threshold(agg, assets, n, ld):
    """0, 1, 2 and 6 positive finger groups (cycling over the samples); NaN in the columns past 778 must reach nothing; then a positive
    threshold equal to one group's pooled value, which the strict comparison must not count"""
    anchor = assets['anchor']
    want = [(0, 1, 2, 6)[(i + n) % 4] for i in range(n)]
    hc, chosen = CL.force_inputs(anchor, n, ld, want, seed=n + ld)
    fc, gr = agg.force_contact(*_dev(hc))
    assert fc.shape == (n, 32) and gr.shape == (n,) and gr.dtype == torch.uint8
    fc, gr = fc.cpu().numpy(), gr.cpu().numpy()
    ref = OC.force_contact(anchor, hc[:, :778].astype(np.float64))
    assert np.isfinite(fc).all() and np.array_equal(fc > 0, ref > 0)
    np.testing.assert_allclose(fc, ref, rtol=1e-6, atol=0)
    assert np.array_equal(gr, np.array([OC.is_grasped(ref[i]) for i in range(n)], np.uint8))
    assert np.array_equal(gr, np.array([k >= 2 for k in want], np.uint8))
    # two groups, pooled values a < b, one anchor each: the group sums are the kernel's own fp32 fc values (the other addends are 0)
    hc2, chosen2 = CL.force_inputs(anchor, n, ld, [2] * n, seed=n, levels=(0.5, 1.0))
    fc2 = agg.force_contact(*_dev(hc2))[0].cpu().numpy()
    a = fc2[np.arange(n), chosen2[:, 0]]
    b = fc2[np.arange(n), chosen2[:, 1]]
    assert (a > 0).all() and (a < b).all() and len(np.unique(a)) == 1             # the same anchor weights: one value for the launch
    thresh = float(a[0])
    for th, grasped in ((thresh, 0), (float(np.nextafter(a[0], np.float32(0))), 1), (float(b.max()), 0)):
        fc3, gr3 = agg.force_contact(*_dev(hc2), thresh=th)
        assert np.array_equal(fc3.cpu().numpy(), fc2)
        assert (gr3.cpu().numpy() == grasped).all(), (th, gr3.cpu().numpy())
        assert np.array_equal(gr3.cpu().numpy(), np.array([OC.is_grasped(fc2[i].astype(np.float64), th) for i in range(n)], np.uint8))

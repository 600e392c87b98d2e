"""The claims of tests/_contact_lattice.py against oracle/contact.py: the inputs are exactly representable, the nearest neighbours are
unambiguous in fp32 and in fp64, every query of seam_case is in contact with the closed-form weight, the gates of gate_case fall where the
construction says, and the fp32 arithmetic of the kernel (restated in numpy float32) gives the float64 decisions.  No GPU."""
import numpy as np
import pytest

import tests._contact_lattice as CL
from oracle import contact as OC


def _d2(q, t, dtype):
    q, t = q.astype(dtype), t.astype(dtype)
    d = q[:, None, :] - t[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def _detect(c, swap=False):
    f = lambda k: c[k].astype(np.float64)
    if swap:                                           # the displaced points take the hand role
        return OC.detect(f('queries'), f('query_normals'), f('targets'), f('target_normals'), **CL.KW)
    return OC.detect(f('targets'), f('target_normals'), f('queries'), f('query_normals'), **CL.KW)


def _unit_z(n):
    return bool(n.dtype == np.float32 and (n[:, :2] == 0).all() and (np.abs(n[:, 2]) == 1).all())


def test_thresholds_are_exact_and_ordered():
    for v in CL.NORMAL_THRESH + CL.DECAY + (CL.VERTICAL_THRESH, CL.PITCH):
        assert np.float32(v) == v and v / CL.U == round(v / CL.U)
    assert CL.NORMAL_THRESH[0] < CL.DECAY[0] < CL.DECAY[1] < CL.NORMAL_THRESH[1]          # what vpho_contact_detect_f32 requires


@pytest.mark.parametrize('nq,nt', CL.SEAM_SIZES)
def test_seam_case_is_exact_unambiguous_and_all_in_contact(nq, nt):
    for seed in range(3):
        c = CL.seam_case(nq, nt, seed)
        assert all(CL.is_exact(c[k]) for k in ('targets', 'queries')) and all(_unit_z(c[k]) for k in ('target_normals', 'query_normals'))
        assert c['queries'].shape == (nq, 3) and c['targets'].shape == (nt, 3) and len(np.unique(c['targets'], axis=0)) == nt
        special = set(np.clip([0, 1023, 1024, nt - 1], 0, nt - 1).tolist())
        assert (special <= set(c['own'].tolist())) if nq >= 4 else (set(c['own'].tolist()) <= special)
        d32, d64 = _d2(c['queries'], c['targets'], np.float32), _d2(c['queries'], c['targets'], np.float64)
        assert np.array_equal(d32.astype(np.float64), d64)                                # the fp32 distances are the exact ones
        assert np.array_equal(d64.argmin(1), c['own'])
        if nt > 1:
            gap = np.sort(d64, 1)[:, 1] - d64[np.arange(nq), c['own']]
            assert gap.min() >= 576 * CL.U ** 2 > 3.4e-5
        lattice_w, w, o2h = _detect(c)
        assert np.array_equal(o2h, c['own'])                                              # every query in contact, at its own target
        assert (w > 0).all() and np.array_equal(w, CL.closed_form_weight(c['nd']))
        assert np.array_equal(w, OC.contact_weight(c['nd'], CL.NORMAL_THRESH, CL.DECAY))
        w2, lattice_w2, _ = _detect(c, swap=True)
        assert np.array_equal(w2, w) and np.array_equal(lattice_w2, lattice_w)            # the roles only rename the outputs
        assert lattice_w.shape == (nt,) and (lattice_w > 0).any()


def test_a_wrong_neighbour_of_a_seam_query_changes_its_answer():
    """drop the own target of each seam query from the cloud: the query's weight becomes 0 or another weight, never the same"""
    c = CL.seam_case(257, 1025, 0)
    w = _detect(c)[1]
    for i in c['seam_queries']:
        keep = np.arange(1025) != c['own'][i]
        f = lambda a: a.astype(np.float64)
        w1 = OC.detect(f(c['targets'][keep]), f(c['target_normals'][keep]), f(c['queries'][i:i + 1]), f(c['query_normals'][i:i + 1]), **CL.KW)[1]
        assert w1[0] != w[i]


def test_gate_case_falls_where_the_construction_says():
    c = CL.gate_case()
    assert all(CL.is_exact(c[k]) for k in ('targets', 'queries')) and _unit_z(c['query_normals'])
    _, w, o2h = _detect(c)
    assert np.array_equal(o2h >= 0, c['inside']) and np.array_equal(o2h[c['inside']], c['own'][c['inside']])
    assert list(c['inside'][:8]) == [False, True, True, False, True, False, True, False]
    assert np.array_equal(w > 0, c['inside'])
    assert np.array_equal(w[c['inside']], CL.closed_form_weight(c['nd'][c['inside']]))
    sweep = w[8:]
    assert len(sweep) == 95 and sweep.min() < 1e-3 and sweep.max() > 0.999 and ((sweep > 0.05) & (sweep < 0.95)).sum() >= 8   # both flanks, not only the plateau
    # the kernel's own fp32 arithmetic on these inputs: nd and vd come out exactly
    v = c['queries'] - c['targets'][c['own']]
    nd32 = (v * c['query_normals']).sum(-1, dtype=np.float32)
    r = v - nd32[:, None] * c['query_normals']
    vd32 = np.sqrt((r * r).sum(-1, dtype=np.float32))
    assert np.array_equal(nd32.astype(np.float64), c['nd']) and np.array_equal(vd32.astype(np.float64), c['vd'])


@pytest.mark.parametrize('second', (9, 1030))
def test_tie_case_has_one_exact_tie_and_the_oracle_takes_the_smaller_index(second):
    c = CL.tie_case(second)
    assert all(CL.is_exact(c[k]) for k in ('targets', 'queries'))
    assert np.array_equal(c['targets'][5], c['targets'][second]) and len(np.unique(c['targets'], axis=0)) == 1099
    d = _d2(c['queries'], c['targets'], np.float64)
    assert np.array_equal(d[:, 5], d[:, second]) and (d[:32].argmin(1) == 5).all()
    _, w, o2h = _detect(c)
    assert np.array_equal(o2h, c['own']) and (o2h[:32] == 5).all() and np.array_equal(w, CL.closed_form_weight(c['nd']))


def test_force_inputs_reach_exactly_the_chosen_groups(assets):
    private = CL.private_anchors(assets['anchor'])
    assert all(len(v) >= 1 for v in private.values()), private
    want = [0, 1, 2, 6] * 3
    for ld in (778, 800):
        hc, chosen = CL.force_inputs(assets['anchor'], 12, ld, want, seed=3)
        assert hc.shape == (12, ld) and np.isnan(hc[:, 778:]).all() and np.isfinite(hc[:, :778]).all()
        fc = OC.force_contact(assets['anchor'], hc[:, :778].astype(np.float64))
        for i, k in enumerate(want):
            groups = [fc[i, OC.FINGER_LABEL[g]].sum() > 0 for g in CL.GROUPS]
            assert sum(groups) == k and groups == [True] * k + [False] * (6 - k)
            assert bool(OC.is_grasped(fc[i])) == (k >= 2)
            assert np.array_equal(np.flatnonzero(fc[i] > 0), np.sort(chosen[i][chosen[i] >= 0]))

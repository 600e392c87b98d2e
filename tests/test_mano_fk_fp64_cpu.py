"""The forward-kinematics reference of tests/_mano_fk_fp64.py pinned without a GPU, and the claims of its case lists asserted: a wrong
reference, or a case that does not meet the launch form or the block layout it names, must not be what tests/test_gpu_mano_fk.py measures
the kernels with.

  * float64 ``fk`` against tests/_leaf_independent.py::mano_lbs_fp64 (scipy rotations in a parent-table LBS, no 1e-8) within 2e-8 m.  The
    bound is derived: manopth's 1e-8 added to the rotation vector changes its norm by at most sqrt(3) 1e-8, so each of the at most four
    rotations of a chain (root and three finger joints) turns at most 1.8e-8 rad too far, on a lever under 0.25 m: 4 x 1.8e-8 x 0.25.
  * float32 ``fk`` against the oracle's restatement of manopth (oracle.mano.get_hand_verts) within the project's 2e-6 m, and the HO3D
    order against oracle.vpho.joints_ho3d.
  * torch's own float32 error of ``fk`` per run, printed (``pytest -s`` / ``-rP``): the source of the R.bound figures in docs/LOG.md."""
import math

import numpy as np
import pytest
import torch

from oracle import mano as OM
from oracle.vpho import joints_ho3d
from tests import _leaf_fp64 as R
from tests import _leaf_independent as L
from tests import _mano_fk_fp64 as F
from vpho_amd.assets import synthetic_assets

f64 = torch.float64


@pytest.fixture(scope='module')
def mano():
    return synthetic_assets(0)['mano']


PIN = F._case(64, 5, '<1>')                                        # 64 hands, 13 images, the last holds 4


def _angles(pose):
    return pose.double().reshape(-1, 3).norm(dim=-1)


@pytest.mark.parametrize('kind', F.KINDS)
def test_float64_fk_equals_the_scipy_parent_table_lbs(mano, kind):
    pose, betas = F.make(PIN, kind)
    img = torch.arange(PIN.n) // PIN.hpi
    v, j = F.fk(mano, pose.double(), betas.double(), PIN.hpi)
    wv, wj = L.mano_lbs_fp64(mano, pose.double().numpy(), betas.double()[img].numpy())
    ev, ej = float(np.abs(v.numpy() - wv).max()), float(np.abs(j.numpy() - wj).max())
    print(f'PIN scipy {kind}: verts {ev:.2e} joints {ej:.2e}')
    assert float(np.abs(wv).max()) < 0.25 + 0.15 * (kind != 'small')         # the lever of the derivation (the 3x betas image is larger)
    assert ev <= 2e-8 and ej <= 2e-8, (ev, ej)


@pytest.mark.parametrize('kind', F.KINDS)
def test_float32_fk_equals_the_oracles_manopth_and_its_ho3d_order(mano, kind):
    pose, betas = F.make(PIN, kind)
    n_img = betas.shape[0]
    img = torch.arange(PIN.n) // PIN.hpi
    flags = F.ho3d_flags(n_img)
    assert 0 < int(flags.sum()) < n_img
    for dt, tol in ((torch.float32, 2e-6), (f64, 1e-12)):
        p, b = pose.to(dt), betas.to(dt)
        ov, oj = OM.get_hand_verts(mano, p, b[img])
        v, j = F.fk(mano, p, b, PIN.hpi)
        vh, jh = F.fk(mano, p, b, PIN.hpi, flags)
        assert R.worst(v, ov) <= tol and R.worst(j, oj) <= tol, (kind, dt, R.worst(v, ov), R.worst(j, oj))
        assert torch.equal(vh, v)
        want = torch.where(flags.bool()[img][:, None, None], joints_ho3d(ov, oj), oj)
        assert R.worst(jh, want) <= tol
        assert R.worst(jh[flags.bool()[img]], oj[flags.bool()[img]]) > 1e-3              # the HO3D order really differs
    vs, J = F.shape(mano, betas.double())
    assert vs.shape == (n_img, 778, 3) and J.shape == (n_img, 16, 3)
    assert torch.equal(vs[1], torch.as_tensor(mano['v_template'], dtype=f64))           # the image with betas 0


def test_rodrigues_is_manopths():
    aa = torch.randn(500, 3, generator=R.gen(3), dtype=f64) * 1.5
    aa[:4] = torch.tensor([[0, 0, 0], [1e-7, 0, 0], [0, math.pi, 0], [3.0, -4.0, 5.0]], dtype=f64)
    assert float((F.rodrigues(aa) - OM.batch_rodrigues(aa).view(-1, 3, 3)).abs().max()) <= 1e-15
    Rm = F.rodrigues(aa)
    assert float((Rm @ Rm.transpose(-1, -2) - torch.eye(3, dtype=f64)).abs().max()) <= 1e-14
    assert torch.equal(F.rodrigues(aa[:1]), torch.eye(3, dtype=f64)[None])               # the zero vector: exactly the identity


def test_the_dispatch_restated_gives_the_form_each_case_names():
    for c in F.CASES:
        assert F.fk_form(c.n, c.hpi, c.want_verts, c.has_table) == c.form, c
    forms = [c.form for c in F.CASES]
    assert [forms.count(f) for f in ('<1>', '<4>', '<16>', 'mfma')] == [3, 3, 6, 5]
    # the edges: 127 / 128, 1 023 / 1 024, 4 095 / 4 096 hands and 15 / 16 hands per image
    assert (F.fk_form(127, 1), F.fk_form(128, 4)) == ('<1>', '<4>') and (F.fk_form(1023, 31), F.fk_form(1024, 16)) == ('<4>', '<16>')
    assert (F.fk_form(4095, 16), F.fk_form(4096, 16), F.fk_form(4096, 15)) == ('<16>', 'mfma', '<16>')
    assert {(c.n, c.hpi) for c in F.CASES} >= {(127, 1), (128, 4), (1023, 31), (1024, 16), (4095, 16), (4096, 16), (4100, 15)}
    assert F.fk_form(4128, 24, want_verts=False) == '<16>' and F.fk_form(4128, 24, has_table=False) == '<16>'
    assert [c.form for c in F.KIND_CASES] == ['<1>', '<4>', '<16>', 'mfma']
    assert len(F.RUNS) == 17 + 3 * 4 and len({F.run_id(r) for r in F.RUNS}) == len(F.RUNS)


def test_each_case_has_the_blocks_and_images_it_claims():
    for c in F.CASES:
        hb = F.BLOCK[c.form]
        lo, hi = F.block_images(c)
        span = hi - lo + 1
        assert ('ragged' in c.meets) == (c.n % hb != 0), c
        assert ('partial' in c.meets) == (c.n % c.hpi != 0), c
        assert ('straddle' in c.meets) == bool((span == 2).any()), c
        assert ('three' in c.meets) == bool((span == 3).any()), c
        assert int(span.max()) <= 3
        if c.form == 'mfma':
            assert c.hpi >= 16 and c.n >= 4096 and c.want_verts and c.has_table
    three = [c for c in F.CASES if 'three' in c.meets]
    assert [(c.n, c.hpi, c.form) for c in three] == [(4128, 21, 'mfma')] and three[0] in F.HO3D_CASES
    assert 4128 % 32 == 0 and 4128 // 32 == 129 and 4100 % 32 == 4 and 1030 % 16 == 6 and 130 % 4 == 2
    lo, hi = F.block_images(three[0])
    assert int((hi - lo == 2).sum()) >= 50 and int((hi - lo == 1).sum()) >= 50             # three-image and two-image blocks
    # the HO3D flags differ inside the three-image blocks of the matrix-core case that carries them
    c = three[0]
    flags = F.ho3d_flags(F.n_images(c.n, c.hpi))
    lo, hi = F.block_images(c)
    t = torch.nonzero(hi - lo == 2)[:, 0]
    assert len(t) > 10 and all(len({int(flags[i]) for i in range(int(lo[b]), int(hi[b]) + 1)}) == 2 for b in t)


def test_the_planted_hands_sit_where_the_gpu_test_says():
    cases = [c for c in F.CASES if 'straddle' in c.meets]
    assert {c.form for c in cases} == {'<4>', '<16>', 'mfma'}
    for c in cases:
        hb = F.BLOCK[c.form]
        nan, inf = F.planted(c)
        lo, hi = F.block_images(c)
        assert [h % hb for h in nan] == [0, hb // 2, hb - 1] and len({h // hb for h in nan + inf}) == 4
        assert hi[nan[0] // hb] > lo[nan[0] // hb]
        assert inf == [c.n - 1] and all(0 <= h < c.n for h in nan)


@pytest.mark.parametrize('run', F.KIND_RUNS, ids=F.run_id)
def test_the_input_kinds_are_what_they_are_named(run):
    case, kind = run
    pose, betas = F.make(case, kind)
    ang = _angles(pose)
    assert float((pose.double().reshape(-1, 3) + 1e-8).norm(dim=-1).min()) > 0
    assert float((pose.reshape(-1, 3) + torch.tensor(1e-8)).norm(dim=-1).min()) > 0      # in float32 too
    if kind == 'so3':
        assert int((ang > math.pi - 0.15).sum()) >= 50 and float(ang.max()) <= math.pi + 1e-6
    if kind == 'wide':
        assert int((ang > math.pi).sum()) >= 50
    if kind == 'small':
        k = F.small_row_kind(torch.arange(case.n))
        assert torch.equal(pose[k == 0], torch.zeros_like(pose[k == 0]))
        assert 0 < float(pose[k == 1].abs().max()) < 1e-6 and 1e-6 < float(pose[k == 2].abs().max()) < 1e-3
        assert float(pose[k == 3][:, 3:].abs().max()) == 0 and float(pose[k == 3][:, :3].abs().max()) > 0.1
        hb = F.BLOCK[case.form]
        if case.n >= 128:
            seen = {(int(h) % hb, int(t)) for h, t in zip(torch.arange(case.n), k)}
            assert len(seen) == 4 * hb                                               # every block position gets each row type
        else:
            assert set(k.tolist()) == {0, 1, 2, 3}


def test_randn_inputs_and_betas():
    for c in F.CASES:
        pose, betas = F.make(c, 'randn')
        assert pose.shape == (c.n, 48) and betas.shape == (F.n_images(c.n, c.hpi), 10) and pose.dtype == betas.dtype == torch.float32
        assert float((pose.reshape(-1, 3) + torch.tensor(1e-8)).norm(dim=-1).min()) > 0
    a, b = F.make(F.find(4128, 24, '<16>', has_table=False), 'randn'), F.make(F.find(4128, 24, 'mfma'), 'randn')              # one (n, hands per image): one input
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    got, raw = F.make_betas(5, R.gen(1)), torch.randn(5, 10, generator=R.gen(1)) * 0.8
    assert float(got[1].abs().max()) == 0 and torch.equal(got[2], raw[2] * 3.0) and torch.equal(got[[0, 3, 4]], raw[[0, 3, 4]])
    assert float(F.make_betas(1, R.gen(1)).abs().max()) > 0


_UNIQUE = list({(r[0].n, r[0].hpi, r[1]): r for r in F.RUNS}.values())


@pytest.mark.parametrize('run', _UNIQUE, ids=F.run_id)
def test_references_are_finite_and_torchs_float32_error_is_small(mano, run):
    """every reference the GPU file uses is finite, and R.bound of each run -- 4 x torch's float32 error of the same formula, floor 4 ulp of
    the largest output -- is far below the 2e-6 m the sampled tests hold the kernels to"""
    case, kind = run
    pose, betas = F.make(case, kind)
    v64, j64 = F.fk(mano, pose.double(), betas.double(), case.hpi)
    v32, j32 = F.fk(mano, pose, betas, case.hpi)
    assert bool(torch.isfinite(v64).all()) and bool(torch.isfinite(j64).all())
    assert bool(torch.isfinite(v32).all()) and bool(torch.isfinite(j32).all())
    bv, bj = R.bound(v32, v64), R.bound(j32, j64)
    print(f'FK32 {F.run_id(run)}: verts err {R.worst(v32, v64):.2e} bound {bv:.2e}  joints err {R.worst(j32, j64):.2e} bound {bj:.2e}')
    assert bv <= 1e-6 and bj <= 1e-6, (bv, bj)

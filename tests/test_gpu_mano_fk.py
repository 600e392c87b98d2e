"""MANO forward kinematics (csrc/mano.hip; ops.Mano.shape, ops.Mano.fk): every hand, vertex and joint of every launch form against the
float64 reference of tests/_mano_fk_fp64.py (pinned without a GPU by tests/test_mano_fk_fp64_cpu.py, which also asserts what the case
lists claim: the form each case reaches, its ragged last block, its partly filled last image, its two- and three-image blocks).

Nothing reports which kernel a launch ran, so each case names the dispatch clause of vpho_mano_fk_f32 it meets (F.fk_form restates it):
mano_fk_kernel<1> below 128 hands, <4> from 128, <16> from 1 024 and for every launch the matrix-core kernel refuses (fewer than 4 096
hands, fewer than 16 hands per image, no tiled table, no vertices wanted), mano_fk_mfma_kernel otherwise.  docs/LOG.md holds the value-only
mutant of each form and the test it failed.

Tolerance: R.bound of the case's own inputs -- 4 x torch's float32 error of the same formula against float64, floor 4 ulp of the largest
output -- for every comparison with float64; the comparisons of one launch with another are bit for bit, except the matrix-core vertices
against the packed kernel's (3e-7 m, the bar tests/test_gpu_glue.py holds)."""
import ctypes as C

import pytest
import torch

from tests import _leaf_fp64 as R
from tests import _mano_fk_fp64 as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mano(assets):
    return assets['mano']                                                        # synthetic_assets(0)['mano']


@pytest.fixture(scope='module')
def hand(mano):
    from vpho_amd import ops
    return ops.Mano(mano, 'cuda')


@pytest.fixture(scope='module')
def hand_notable(mano):
    """without the tiled table: the host then never picks the matrix-core kernel"""
    from vpho_amd import ops
    m = ops.Mano(mano, 'cuda')
    m.c.posedirs_mfma = None
    return m


@pytest.fixture(scope='module')
def hand_notips(mano):
    """without the compact tip table, with and without the tiled one"""
    from vpho_amd import ops
    a, b = ops.Mano(mano, 'cuda'), ops.Mano(mano, 'cuda')
    a.c.tip_posedirs_t = None
    b.c.tip_posedirs_t = b.c.posedirs_mfma = None
    return {True: a, False: b}


def _same(a, b):
    """bit for bit, on the device"""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


_DEV, _REF = {}, {}


def _device(hand, case, kind='randn'):
    """device pose (n, 48), betas and Mano.shape of them, once per (n, hands per image, kind)"""
    key = (case.n, case.hpi, kind)
    if key not in _DEV:
        pose, betas = F.make(case, kind)
        pose, betas = pose.cuda(), betas.cuda()
        _DEV[key] = (pose, betas, hand.shape(betas))
    return _DEV[key]


def _reference(mano, case, kind='randn', flags=False, want_verts=False):
    """float64 joints and the R.bound of verts and joints of one (inputs, flags) pair, computed once and shared, never modified; the float64
    vertices (77 MB at 4 128 hands) only for the one test that reads them"""
    key = (case.n, case.hpi, kind, flags)
    pose, betas = F.make(case, kind)
    fl = F.ho3d_flags(betas.shape[0]) if flags else None
    v64 = None
    if key not in _REF:
        v64, j64 = F.fk(mano, pose.double(), betas.double(), case.hpi, fl)
        v32, j32 = F.fk(mano, pose, betas, case.hpi, fl)
        _REF[key] = dict(j64=j64, bv=R.bound(v32, v64), bj=R.bound(j32, j64))
    elif want_verts:
        v64 = F.fk(mano, pose.double(), betas.double(), case.hpi, fl)[0]
    return dict(_REF[key], v64=v64 if want_verts else None)


def _check(items):
    """R.check of every (name, got, float64 reference, bound), every figure printed before the first assertion"""
    rows = [(name, R.worst(got, ref), tol, got, ref) for name, got, ref, tol in items]
    for name, err, tol, _, _ in rows:
        print(f'LEAF {name}: worst {err:.3e} bound {tol:.3e}')
    for name, err, tol, got, ref in rows:
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert bool(torch.isfinite(got).all()), name
        assert err <= tol, f'{name}: worst {err:.3e} bound {tol:.3e}'


@pytest.mark.parametrize('n_img', [1, 3, 274])
def test_shape_blend_and_joint_regression_against_float64(hand, mano, n_img):
    """mano_shape_kernel on its own: v_shaped and J of 1, 3 and 274 images (one workgroup per image; 274 = the images of the 4 100-hand
    launch with 15 per image); the image with betas 0 has the bits of v_template"""
    betas = F.make_betas(n_img, R.gen(n_img))
    (v64, J64), (bv, bJ) = R.ruled(lambda b: F.shape(mano, b), [betas])
    vs, J = hand.shape(betas.cuda())
    _check([(f'shape img{n_img} v_shaped', vs, v64, bv), (f'shape img{n_img} J', J, J64, bJ)])
    template = torch.as_tensor(mano['v_template'], dtype=torch.float32)
    if n_img >= 2:
        assert R.bits_equal(vs[1], template)
    vz, Jz = hand.shape(torch.zeros(2, 10, device='cuda'))
    assert R.bits_equal(vz[0], template) and R.bits_equal(vz[1], template) and R.bits_equal(Jz[0], Jz[1])
    assert R.worst(Jz[0], torch.as_tensor(mano['J_regressor'], dtype=torch.float64) @ template.double()) <= bJ


@pytest.mark.parametrize('run', F.RUNS, ids=F.run_id)
def test_every_form_against_float64_on_every_element(hand, hand_notable, mano, run):
    """vertices, joints and the joints of the joints-only launch (verts == NULL, grid.y = 1) of every case and input kind, every element,
    each to the R.bound of its own inputs"""
    case, kind = run
    M = hand if case.has_table else hand_notable
    pose, _, ctx = _device(hand, case, kind)
    ref = _reference(mano, case, kind, want_verts=case.want_verts)
    verts, joints = M.fk(pose, ctx, case.hpi, case.want_verts)
    name = f'fk {F.run_id(run)}'
    items = [(f'{name} joints', joints, ref['j64'], ref['bj'])]
    if case.want_verts:
        items += [(f'{name} verts', verts, ref['v64'], ref['bv']), (f'{name} joints-only', M.fk(pose, ctx, case.hpi, False)[1], ref['j64'], ref['bj'])]
    else:
        assert verts is None
    _check(items)


@pytest.mark.parametrize('case', F.HO3D_CASES, ids=F.case_id)
def test_ho3d_flags_mixed_per_image(hand, mano, case):
    """the HO3D joint order with its own five tip vertices on every third image (on the matrix-core case the flags differ inside the
    three-image blocks): joints against float64; the vertices do not depend on the flag; no flag array is an all-zero one"""
    pose, betas, ctx = _device(hand, case)
    flags = F.ho3d_flags(betas.shape[0])
    ref = _reference(mano, case, flags=True)
    v, j = hand.fk(pose, ctx, case.hpi, True, ho3d=flags.cuda())
    v0, j0 = hand.fk(pose, ctx, case.hpi, True)
    vz, jz = hand.fk(pose, ctx, case.hpi, True, ho3d=torch.zeros_like(flags).cuda())
    jo = hand.fk(pose, ctx, case.hpi, False, ho3d=flags.cuda())[1]
    _check([(f'fk {F.case_id(case)} ho3d joints', j, ref['j64'], ref['bj']), (f'fk {F.case_id(case)} ho3d joints-only', jo, ref['j64'], ref['bj'])])
    assert _same(v, v0) and _same(vz, v0) and _same(jz, j0) and _same(jo, j)
    on = flags.bool()[torch.arange(case.n) // case.hpi].cuda()
    assert _same(j[~on], j0[~on])
    assert bool(((j[on] - j0[on]).abs().amax(dim=(1, 2)) > 1e-4).all())                  # every flagged hand really got the other order


@pytest.mark.parametrize('case', F.CASES, ids=F.case_id)
def test_joints_only_and_repeated_launches_give_the_same_bits(hand, hand_notable, case):
    """the joints of a launch with vertices are the joints of the joints-only launch, and a second launch repeats the first, bit for bit"""
    M = hand if case.has_table else hand_notable
    pose, _, ctx = _device(hand, case)
    v, j = M.fk(pose, ctx, case.hpi, True)
    v2, j2 = M.fk(pose, ctx, case.hpi, True)
    jo, jo2 = M.fk(pose, ctx, case.hpi, False)[1], M.fk(pose, ctx, case.hpi, False)[1]
    assert _same(v, v2) and _same(j, j2) and _same(jo, jo2)
    assert _same(j, jo)


@pytest.mark.parametrize('case', [c for c in F.CASES if c.form == 'mfma'], ids=F.case_id)
def test_matrix_core_launch_against_the_packed_kernel_on_the_same_input(hand, hand_notable, case):
    """mano_fk_mfma_kernel against mano_fk_kernel<16> (the same launch without the tiled table): joints bit for bit -- the kinematic and
    tip code is one source --, vertices within 3e-7 m"""
    pose, _, ctx = _device(hand, case)
    v, j = hand.fk(pose, ctx, case.hpi, True)
    v16, j16 = hand_notable.fk(pose, ctx, case.hpi, True)
    err = float((v - v16).abs().max())
    print(f'LEAF fk {F.case_id(case)} verts mfma vs <16>: worst {err:.3e} bound 3.000e-07')
    assert _same(j, j16)
    assert err < 3e-7


@pytest.mark.parametrize('case', [c for c in F.CASES if c.form != '<1>' and c.hpi <= 127], ids=F.case_id)
def test_blocked_joints_have_the_bits_of_one_hand_per_block_launches(hand, hand_notable, case):
    """joints of <4>, <16> and the matrix-core kernel against mano_fk_kernel<1> on the same hands, one launch per image (at most 127 hands,
    its own v_shaped and J): the kinematic and tip code is one source and the build runs with contraction off, so the bits are the same
    whatever the block position of a hand and whichever images share its block"""
    M = hand if case.has_table else hand_notable
    pose, betas, (vs, J) = _device(hand, case)
    _, j = M.fk(pose, (vs, J), case.hpi, case.want_verts)
    parts = []
    for i in range(betas.shape[0]):
        rows = pose[i * case.hpi:(i + 1) * case.hpi]
        assert F.fk_form(rows.shape[0], case.hpi, False) == '<1>'
        parts.append(hand.fk(rows, (vs[i:i + 1], J[i:i + 1]), case.hpi, False)[1])
    assert _same(j, torch.cat(parts))


@pytest.mark.parametrize('case', F.CASES, ids=F.case_id)
def test_rows_of_58_columns_and_a_missing_tip_table_give_the_same_bits(hand, hand_notable, hand_notips, case):
    """ld_pose = 58 as the engine passes it (pose plus betas in one row), with NaN in columns 48 .. 57: the bits of the 48-column launch;
    tip_posedirs_t = NULL (the tip columns read from the full table): the same bits"""
    M = hand if case.has_table else hand_notable
    pose, _, ctx = _device(hand, case)
    v, j = M.fk(pose, ctx, case.hpi, case.want_verts)
    wide = torch.full((case.n, 58), float('nan'), device='cuda')
    wide[:, :48] = pose
    vw, jw = M.fk(wide, ctx, case.hpi, case.want_verts)
    vt, jt = hand_notips[case.has_table].fk(pose, ctx, case.hpi, case.want_verts)
    assert _same(jw, j) and _same(jt, j)
    if case.want_verts:
        assert _same(vw, v) and _same(vt, v)


@pytest.mark.parametrize('case', [c for c in F.CASES if 'straddle' in c.meets], ids=F.case_id)
def test_a_non_finite_hypothesis_stays_inside_its_own_hand(hand, hand_notable, case):
    """the sampler's last evaluation is not NaN-guarded, so a NaN or inf hypothesis can reach FK.  NaN in one pose value of the hand at the
    first position of a block that holds hands of two images, at a middle and at the last position of the next two blocks, +inf in the
    last hand of the launch: every other hand keeps the bits of the clean launch, every planted hand has a non-finite joint and vertex.
    Ordinary values through ordinary arithmetic: no address depends on them"""
    M = hand if case.has_table else hand_notable
    pose, _, ctx = _device(hand, case)
    nan_rows, inf_rows = F.planted(case)
    bad = pose.clone()
    bad[nan_rows, 4] = float('nan')
    bad[inf_rows, 7] = float('inf')
    v0, j0 = M.fk(pose, ctx, case.hpi, case.want_verts)
    v, j = M.fk(bad, ctx, case.hpi, case.want_verts)
    keep = torch.ones(case.n, dtype=torch.bool, device='cuda')
    keep[nan_rows + inf_rows] = False
    assert bool(torch.isfinite(j0).all())
    assert _same(j[keep], j0[keep])
    assert bool((~torch.isfinite(j[~keep])).flatten(1).any(1).all())
    if case.want_verts:
        assert _same(v[keep], v0[keep])
        assert bool((~torch.isfinite(v[~keep])).flatten(1).any(1).all())


def test_refusals_by_message_and_nothing_is_written(hand):
    """ld_pose < 48, n_hands = 0 and hands_per_image = 0 answer VphoError before anything is launched: the sentinel-filled outputs are
    untouched.  The buffers passed are valid for 4 hands of 58 columns"""
    from vpho_amd import ops
    pose = torch.zeros(4, 58, device='cuda')
    vs, J = hand.shape(torch.zeros(1, 10, device='cuda'))
    v, j = torch.full((4, 778, 3), R.SENT, device='cuda'), torch.full((4, 21, 3), R.SENT, device='cuda')
    for ld, n, per in ((47, 4, 4), (58, 0, 4), (58, 4, 0)):
        with pytest.raises(ops.VphoError, match=r'vpho_mano_fk_f32: bad argument'):
            ops._call('vpho_mano_fk_f32', C.byref(hand.c), pose, ld, n, per, vs, J, None, v, j)
    torch.cuda.synchronize()
    assert bool((v == R.SENT).all()) and bool((j == R.SENT).all())
    hand.fk(pose, (vs, J), 4)                                                     # the same buffers' sizes are served

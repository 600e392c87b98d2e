"""The sixteen aggregation-cascade kernels (csrc/aggregate.hip, csrc/aggregate_modes.hip) one by one, each wrapper called by name on an
``ops.Aggregation`` built here on small tables, against the float64 restatements of tests/_cascade_fp64.py evaluated on the inputs the
kernel saw.  Tolerance classes:

* bit-exact (``bits_equal``; ``torch.equal`` for float64): the pure gathers.
* single-rounded float64 chains (hand_heat, obj_heat_score, obj_pt2d_score), elementwise
      |got - ref64| <= 2^-23 |ref64| + 2^-45 S,      S = the sum of |tap * weight| of the look-up(s) / of the per-key-point distances.
  The kernel evaluates the chain in double and rounds to float32: half an ulp, 2^-24 |ref64|, for a result rounded once.  obj_heat_score
  rounds each key-point's look-up and then their double sum: 2^-24 (sum |v_j| + |sum v_j|) <= 2^-23 |ref64| for the non-negative maps
  used here.  The second term is the float64 arithmetic itself, which does not shrink with the result where taps of both signs cancel
  (the cubic weights are negative beyond one pixel) or where a score is a short sum of long distances: ~50 operations at 2^-53 on
  terms whose magnitudes add up to S stay below 2^-47 S; 2^-45 S leaves a factor 4 for a different summation order.
* float32 arithmetic: ``R.bound`` of tests/_leaf_fp64.py -- 4 x the error of torch's own float32 evaluation of the restatement against
  float64, floor 4 ulp of the largest output.
* rotation outputs are compared as rotations (``X.check_rotation``): the geodesic angle to the float64 reference, held to the same rule
  applied to the angle of the float32 restatement (floor: 4 ulp of the largest axis-angle component of the reference).

The input conditions (position classes, nearest-vertex separation, eigen-gaps) are asserted in tests/test_cascade_fp64_cpu.py on the
same generators, and again here where a score depends on them."""
import pytest
import torch

from tests import _cascade_fp64 as X

pytestmark = pytest.mark.gpu


def _ops():
    from vpho_amd import ops
    return ops


def _d(t):
    return None if t is None else t.cuda()


def _agg(assets):
    from vpho_amd.assets import ANCHOR_SKELETON
    ops = _ops()
    agg = ops.Aggregation(assets, ANCHOR_SKELETON, 'cuda')
    return agg


def _chain_tol(ref64, S):
    return 2.0 ** -23 * ref64.abs() + 2.0 ** -45 * S


def _nan_rows(got, rows):
    """exactly the listed leading rows are NaN, everywhere"""
    got = got.detach().cpu()
    bad = torch.isnan(got.reshape(got.shape[0], -1))
    want = torch.zeros(got.shape[0], dtype=torch.bool)
    want[list(rows)] = True
    return bool((bad == want[:, None]).all())


# ------------------------------------------------------------------------------------------------ bit-exact gathers
@pytest.mark.parametrize('bs,S,ld', [(1, 1, 48), (3, 5, 58), (2, 33, 51)])
def test_hand_candidates_bit_exact(bs, S, ld):
    """rows c < S copy the diffusion pose; rows c >= S take elements 0..2 from diffusion row c - S and 3..47 from the regression pose"""
    agg = _agg(X.small_assets())
    g = X.gen(bs * 100 + S)
    diff, reg = torch.randn(bs, S, ld, generator=g), torch.randn(bs, 48, generator=g)
    got = agg.hand_candidates(_d(diff), _d(reg), bs, S).cpu()
    assert got.shape == (bs, 2 * S, 48)
    assert X.bits_equal(got, X.hand_candidates(diff, reg))
    assert X.bits_equal(got[:, :S], diff[..., :48].contiguous())
    assert X.bits_equal(got[:, S:, :3], diff[..., :3].contiguous())
    assert X.bits_equal(got[:, S:, 3:], reg[:, None, 3:].expand(bs, S, 45).contiguous())


@pytest.mark.parametrize('ko', [1, 3, 10])
def test_obj_cross_candidates_bit_exact(ko):
    """cand[b, i*ko + j] = [rot6d of pose[b, rot_idx[b,j]], transl of pose[b, transl_idx[b,i]]], index lists with repeats"""
    agg = _agg(X.small_assets())
    bs, n = 2, 12
    g = X.gen(ko)
    pose = torch.randn(bs, n, 9, generator=g, dtype=torch.float64)
    t_idx, r_idx = X._randint(g, n, bs, ko), X._randint(g, n, bs, ko)
    if ko > 1:
        t_idx[:, -1], r_idx[:, 0] = t_idx[:, 0], r_idx[:, -1]                                        # repeats
    got = agg.obj_cross(_d(pose), _d(t_idx), _d(r_idx)).cpu()
    assert got.dtype == torch.float64 and torch.equal(got, X.obj_cross(pose, t_idx, r_idx))
    for b in range(bs):
        for i in range(ko):
            for j in range(ko):
                assert torch.equal(got[b, i * ko + j, :6], pose[b, int(r_idx[b, j]), :6]) and torch.equal(got[b, i * ko + j, 6:], pose[b, int(t_idx[b, i]), 6:])


@pytest.mark.parametrize('bs,k,ld', [(1, 1, 48), (3, 30, 58)])
def test_hand_phys_candidates_bit_exact(bs, k, ld):
    """only rotations 15, 3, 6, 12, 9 of the candidates c < k change, each to column f of topk_pose[b, c]; candidate k is the aggregated
    pose; columns 48..57 are the betas"""
    agg = _agg(X.small_assets())
    g = X.gen(bs + k)
    pose, betas, tp = torch.randn(bs, ld, generator=g), torch.randn(bs, 10, generator=g), torch.randn(bs, k, 5, 3, generator=g)
    got = agg.hand_phys_candidates(_d(pose), _d(betas), _d(tp)).cpu()
    assert got.shape == (bs, k + 1, 58) and X.bits_equal(got, X.hand_phys_candidates(pose, betas, tp))
    assert X.bits_equal(got[:, k, :48], pose[:, :48].contiguous()) and X.bits_equal(got[..., 48:], betas[:, None].expand(bs, k + 1, 10).contiguous())
    changed = sorted(c for j in X.LVL3_JOINT for c in (3 * j, 3 * j + 1, 3 * j + 2))
    same = [c for c in range(48) if c not in changed]
    assert X.bits_equal(got[:, :k][..., same], pose[:, None, same].expand(bs, k, len(same)).contiguous())
    for f, j in enumerate(X.LVL3_JOINT):
        assert X.bits_equal(got[:, :k, 3 * j:3 * j + 3], tp[:, :, f].contiguous())


# ------------------------------------------------------------------------------------------------ single-rounded float64 chains
@pytest.fixture(scope='module')
def heat():
    d = X.hand_heat_inputs()
    args64 = X.to64([d['joints'], d['root'], d['K'], d['bbox'], d['heatmap']])
    d['ref'], d['S'] = X.hand_heat(*args64, list(range(21)), want_S=True)                             # computed once for every observe list
    return d


@pytest.mark.parametrize('level', [-1, 0, 1, 2, 3])
def test_hand_heat_double_chain(heat, level, monkeypatch):
    """12 x 20 maps, per-image K with skew, non-square boxes; observe = all 21 joints, then each level's 20, 15, 10, 5 (a channel-for-column
    mix-up shows); candidates placed by construction in every position class (X.HEAT_CLASSES); far outside gives exactly 0.0"""
    monkeypatch.delenv('VPHO_SCORE_FP32', raising=False)
    agg = _agg(X.small_assets())
    obs = X.observe_list(level)
    assert X.heat_classes_hold(heat)
    got = agg.hand_heat(*[_d(heat[k]) for k in ('joints', 'root', 'K', 'bbox', 'heatmap')], obs).cpu()
    ref, S = heat['ref'][..., obs], heat['S'][..., obs]
    assert got.shape == ref.shape == (3, 7, len(obs))
    for c, cls in enumerate(X.HEAT_CLASSES):
        X.check_each(f'hand_heat obs{len(obs)} {cls}{c}', got[:, c], ref[:, c], _chain_tol(ref[:, c], S[:, c]))
    far = X.HEAT_CLASSES.index('far')
    assert bool((got[:, far] == 0).all()) and bool((ref[:, far] == 0).all())


def test_hand_heat_float32_chain(heat, monkeypatch):
    """VPHO_SCORE_FP32=1 (read per call): the float32 chain, held to R.bound on the in-range classes"""
    monkeypatch.setenv('VPHO_SCORE_FP32', '1')
    agg = _agg(X.small_assets())
    obs = X.observe_list(0)
    got = agg.hand_heat(*[_d(heat[k]) for k in ('joints', 'root', 'K', 'bbox', 'heatmap')], obs).cpu()
    monkeypatch.delenv('VPHO_SCORE_FP32')
    args = [heat[k] for k in ('joints', 'root', 'K', 'bbox', 'heatmap')]
    f32 = X.hand_heat(*args, obs)
    for c, cls in enumerate(X.HEAT_CLASSES):
        if cls != 'far':
            X.check(f'hand_heat fp32 {cls}{c}', got[:, c], heat['ref'][:, c][..., obs], X.bound(f32[:, c], heat['ref'][:, c][..., obs]))
    again = agg.hand_heat(*[_d(heat[k]) for k in ('joints', 'root', 'K', 'bbox', 'heatmap')], obs).cpu()   # the double chain is back
    X.check_each('hand_heat obs20 after fp32', again, heat['ref'][..., obs], _chain_tol(heat['ref'][..., obs], heat['S'][..., obs]))


@pytest.mark.parametrize('n_kpt,n', [(5, 1), (5, 9), (27, 9)])
def test_obj_heat_score_double_chain(n_kpt, n, monkeypatch):
    """tables of n_kpt key-points (5, and the standard 27), J = n_kpt maps of 12 x 20; distinct ids, one the last table row; is_right =
    [1,0,1]; non-orthonormal 6-D rotations; translation override absent and given; then the ids -1 / n_obj: NaN rows, the other unchanged"""
    monkeypatch.delenv('VPHO_SCORE_FP32', raising=False)
    assets = X.small_assets(n_kpt=n_kpt, seed=n_kpt)
    agg, tab = _agg(assets), X.tables(assets)
    d = X.obj_scene(n_kpt + n, tab, n=n)
    root, kpt, K, bbox, hm = X.to64([d['root'], tab['kpt'], d['K'], d['bbox'], d['heatmap']])
    dev = [_d(d[k]) for k in ('root', 'obj_id', 'is_right', 'K', 'bbox', 'heatmap')]
    for transl in (None, d['transl']):
        ref, S = X.obj_heat_score(d['pose'], transl, root, kpt, d['obj_id'], d['is_right'], K, bbox, hm, want_S=True)
        got = agg.obj_heat_score(_d(d['pose']), *dev, transl_override=_d(transl)).cpu()
        assert got.shape == (3, n)
        X.check_each(f'obj_heat_score kpt{n_kpt} n{n} override={transl is not None}', got, ref, _chain_tol(ref, S))
        if transl is not None:                                                                       # = the pose with its translation replaced
            assert X.bits_equal(got, agg.obj_heat_score(_d(X.with_translation(d['pose'], transl).contiguous()), *dev))
    ids = d['obj_id'].clone()
    ids[0], ids[2] = -1, tab['kpt'].shape[0]
    bad = agg.obj_heat_score(_d(d['pose']), dev[0], _d(ids), *dev[2:], transl_override=_d(d['transl'])).cpu()
    assert _nan_rows(bad, (0, 2)) and X.bits_equal(bad[1], got[1])


def test_obj_pt2d_score_double_chain():
    """n_kpt = 5, mixed handedness; S = the sum of the per-key-point distances = |ref|; ids -1 and n_obj give NaN rows (the kernel's guard)"""
    assets = X.small_assets(n_kpt=5, seed=5)
    agg, tab = _agg(assets), X.tables(assets)
    d = X.obj_scene(31, tab, n=9)
    root, kpt, K, bbox, peak = X.to64([d['root'], tab['kpt'], d['K'], d['bbox'], d['peak']])
    ref = X.obj_pt2d_score(d['pose'], root, kpt, d['obj_id'], d['is_right'], K, bbox, peak)
    got = agg.obj_pt2d_score(*[_d(d[k]) for k in ('pose', 'root', 'obj_id', 'is_right', 'K', 'bbox', 'peak')]).cpu()
    X.check_each('obj_pt2d_score kpt5 n9', got, ref, _chain_tol(ref, ref.abs()))
    ids = d['obj_id'].clone()
    ids[0], ids[2] = -1, tab['kpt'].shape[0]
    bad = agg.obj_pt2d_score(_d(d['pose']), _d(d['root']), _d(ids), *[_d(d[k]) for k in ('is_right', 'K', 'bbox', 'peak')]).cpu()
    assert _nan_rows(bad, (0, 2)) and X.bits_equal(bad[1], got[1])


# ------------------------------------------------------------------------------------------------ float32 arithmetic
@pytest.mark.parametrize('rows,k', [(1, 1), (5, 30), (257, 10)])
def test_topk_weights(rows, k):
    agg = _agg(X.small_assets())
    val = (0.05 + torch.rand(rows, k, generator=X.gen(rows + k)) * 3).contiguous()                     # positive, as heat sums are
    ref, tol = X.ruled(X.topk_weights, [val])
    got = agg.topk_weights(_d(val))
    X.check(f'topk_weights {rows}x{k}', got, ref, tol)
    assert float((got.double().sum(-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize('n_vert', [37, 2048])
def test_obj_verts(n_vert):
    """a vertex tail (37 % 8 != 0), mixed handedness, distinct ids; then the ids -1 / n_obj: NaN rows, the other unchanged"""
    assets = X.small_assets(n_vert=n_vert, seed=n_vert)
    agg, tab = _agg(assets), X.tables(assets)
    d = X.obj_scene(n_vert, tab, n=1, pose_f32=True)
    pose = d['pose'][:, 0].contiguous()
    ref, tol = X.ruled(X.obj_verts, [pose.float(), d['root'], tab['vert'], d['obj_id'], d['is_right']])
    got = agg.obj_verts(_d(pose), _d(d['root']), _d(d['obj_id']), _d(d['is_right'])).cpu()
    assert got.shape == (3, n_vert, 3)
    X.check(f'obj_verts nv{n_vert}', got, ref, tol)
    ids = d['obj_id'].clone()
    ids[0], ids[2] = -1, tab['vert'].shape[0]
    bad = agg.obj_verts(_d(pose), _d(d['root']), _d(ids), _d(d['is_right'])).cpu()
    assert _nan_rows(bad, (0, 2)) and X.bits_equal(bad[1], got[1])


def _phys_args(d, tab):
    return [d['pose'].float(), d['root'], tab['vert'], tab['com'], d['obj_id'], d['is_right'], d['force_point'], d['force_global']]


@pytest.mark.parametrize('n_vert,n', X.PHYSICS_CASES)
def test_obj_physics_score(n_vert, n):
    """n_vert 37 (a tail), 2048, 4096 (the most the entry point accepts), n = 1 and 6, bs = 3, mixed handedness.  The score depends on
    WHICH vertex is nearest: the float64 nearest and second-nearest squared distances of every (candidate, force point) are at least 1e-5
    relative apart (asserted), so float32 rounding cannot change the choice.  Then the ids -1 / n_obj: NaN rows, the other unchanged"""
    assets, d = X.physics_case(n_vert, n)
    agg, tab = _agg(assets), X.tables(assets)
    assert X.nearest_separation(d['pose'], d['root'], tab['vert'], d['obj_id'], d['is_right'], d['force_point']) >= X.SEPARATION
    ref, tol = X.ruled(X.obj_physics_score, _phys_args(d, tab))
    dev = [_d(d[k]) for k in ('pose', 'root', 'obj_id', 'is_right', 'force_point', 'force_global')]
    got = agg.obj_physics_score(*dev).cpu()
    assert got.shape == (3, n)
    X.check(f'obj_physics_score nv{n_vert} n{n}', got, ref, tol)
    ids = d['obj_id'].clone()
    ids[0], ids[2] = -1, tab['vert'].shape[0]
    bad = agg.obj_physics_score(dev[0], dev[1], _d(ids), *dev[3:]).cpu()
    assert _nan_rows(bad, (0, 2)) and X.bits_equal(bad[1], got[1])


def test_obj_physics_score_tie_takes_the_smaller_index():
    """two table vertices at (+-a, 0, 0), indices i < j in different lanes of the search, every force point at the origin: the documented
    rule (smaller squared distance, then smaller index) makes the score the one of vertex i; with vertex j it is far outside the bound"""
    assets, d, i, j = X.tie_case()
    agg, tab = _agg(assets), X.tables(assets)
    ref, tol = X.ruled(X.obj_physics_score, _phys_args(d, tab))
    other = X.obj_physics_score(*X.to64(_phys_args(d, tab)), pick=torch.full((1, 1, 32), j))
    assert float((ref - other).abs()) > 100 * tol
    got = agg.obj_physics_score(*[_d(d[k]) for k in ('pose', 'root', 'obj_id', 'is_right', 'force_point', 'force_global')])
    X.check('obj_physics_score tie', got, ref, tol)


@pytest.mark.parametrize('n_hands,hpi', [(1, 1), (8, 1), (8, 4)])
def test_force_anchor_dense_vert2joint(n_hands, hpi):
    """a dense vert2joint (the full 778-term reduction); per-image root and force_local distinct: hand h uses row h // hands_per_image
    (with the rows of the wrong image the result is far outside the bound); reference: local_to_global on verts + root"""
    from vpho_amd.assets import ANCHOR_SKELETON
    assets = X.small_assets(dense_v2j=True)
    agg, tab = _agg(assets), X.tables(assets)
    verts, root, fl = X.force_anchor_inputs(n_hands, hpi)
    assert X.faces_are_not_degenerate(verts, tab['face'])
    skel = torch.as_tensor(ANCHOR_SKELETON).long()
    f = lambda v, r, l, aw, v2j: X.force_anchor(v, r, l, hpi, tab['face'], aw, v2j, skel)
    (rp, rg), (tp, tg) = X.ruled(f, [verts, root, fl, tab['aw'], tab['v2j']])
    fp, fg = agg.force_anchor(_d(verts), _d(root), _d(fl), hpi)
    X.check(f'force_anchor point h{n_hands} hpi{hpi}', fp, rp, tp)
    X.check(f'force_anchor global h{n_hands} hpi{hpi}', fg, rg, tg)
    if n_hands // hpi > 1:
        wp, wg = f(*X.to64([verts, root.roll(1, 0), fl.roll(1, 0), tab['aw'], tab['v2j']]))
        assert float((wp - rp).abs().max()) > 100 * tp and float((wg - rg).abs().max()) > 100 * tg


@pytest.mark.parametrize('n_vert', [37, 4096])
def test_hand_phys_score(n_vert):
    """(bs, n_cand) = (2, 5); the value depends on the minimum distance only: no separation condition"""
    agg = _agg(X.small_assets())
    bs, n_cand = 2, 5
    g = X.gen(n_vert)
    ov = ((torch.rand(bs, n_vert, 3, generator=g) - 0.5) * 0.2).contiguous()
    fp = ((torch.rand(bs * n_cand, 32, 3, generator=g) - 0.5) * 0.24).contiguous()
    fg = (torch.randn(bs * n_cand, 32, 3, generator=g) * (0.2 + torch.rand(bs * n_cand, 32, 1, generator=g))).contiguous()
    ref, tol = X.ruled(X.hand_phys_score, [fp, fg, ov], bs, n_cand)
    got = agg.hand_phys_score(_d(fp), _d(fg), _d(ov), bs, n_cand)
    assert got.shape == (bs, n_cand, 5)
    X.check(f'hand_phys_score nv{n_vert}', got, ref, tol)


@pytest.mark.parametrize('per_joint', [False, True])
def test_hand_pt2d_score(per_joint):
    """bs * C = 260 crosses a block; joint 4 of candidate 7 of image 1 projects exactly onto its peak (every operation exact by
    construction): per joint the score there is 0 with either sign"""
    agg = _agg(X.small_assets())
    d = X.pt2d_inputs()
    args = [d[k] for k in ('joints', 'root', 'K', 'bbox', 'peak')]
    ref, tol = X.ruled(X.hand_pt2d_score, args, per_joint)
    got = agg.hand_pt2d_score(*[_d(a) for a in args], per_joint=per_joint).cpu()
    assert got.shape == ((2, 130, 21) if per_joint else (2, 130))
    X.check(f'hand_pt2d_score per_joint={per_joint}', got, ref, tol)
    if per_joint:
        assert float(ref[1, 7, 4]) == 0.0 and float(got[1, 7, 4].abs()) == 0.0


@pytest.mark.parametrize('bs,C,k', [(2, 9, 1), (5, 40, 7)])
def test_hand_joint_gather_mean(bs, C, k):
    """joint j = the mean over the k candidates listed for THAT joint; one out-of-range index makes only that (image, joint) NaN"""
    agg = _agg(X.small_assets())
    g = X.gen(bs * C + k)
    joints = torch.randn(bs, C, 21, 3, generator=g).contiguous()
    idx = X._randint(g, C, bs, 21, k)
    ref, tol = X.ruled(X.hand_joint_gather_mean, [joints, idx])
    got = agg.hand_joint_gather_mean(_d(joints), _d(idx)).cpu()
    assert got.shape == (bs, 21, 3)
    X.check(f'hand_joint_gather_mean {bs}x{C}x{k}', got, ref, tol)
    bad_idx = idx.clone()
    bad_idx[bs - 1, 13, k - 1] = C
    bad = agg.hand_joint_gather_mean(_d(joints), _d(bad_idx)).cpu()
    nan = torch.isnan(bad)
    assert bool(nan[bs - 1, 13].all()) and int(nan.sum()) == 3
    assert X.bits_equal(torch.where(nan, got, bad), got)


# ------------------------------------------------------------------------------------------------ quaternion means
def _aa_rot(aa48):
    return X.aa_to_matrix(aa48.double().reshape(aa48.shape[0], -1, 3))


@pytest.mark.parametrize('name', X.POSE_FUSE_CASES)
def test_hand_pose_fuse(name):
    """idx / w given; idx None with n < C and w None; w None; n = 2C with repeats; ld 48 and 58; bs = 5 (80 lanes: two blocks); identical
    rotations: finite and that rotation.  Members lie within 0.4 rad of a common rotation, some written with an angle in (pi, 2 pi);
    eigen-gap >= 0.2 asserted.  One out-of-range index: NaN in that image's 48 outputs, the other images unchanged"""
    agg = _agg(X.small_assets())
    pose, idx, w, n = X.pose_fuse_case(name)
    assert X.pose_fuse_gap(pose, idx, w, n) >= X.FUSE_GAP
    ref = X.hand_pose_fuse(*X.to64([pose, idx, w]), n)
    f32 = X.hand_pose_fuse(pose, idx, w, n)
    got = agg.hand_pose_fuse(_d(pose), _d(idx), _d(w), n=None if idx is not None else n).cpu()
    assert got.shape == (5, 48)
    X.check_rotation(f'hand_pose_fuse {name}', _aa_rot(got), _aa_rot(ref), _aa_rot(f32), ref.abs().max())
    if name == 'identical':
        X.check_rotation('hand_pose_fuse identical vs member', _aa_rot(got), _aa_rot(pose[:, 0, :48]), _aa_rot(f32), ref.abs().max())
    if idx is not None:
        bad_idx = idx.clone()
        bad_idx[3, 1] = pose.shape[1]
        bad = agg.hand_pose_fuse(_d(pose), _d(bad_idx), _d(w)).cpu()
        assert _nan_rows(bad, (3,)) and X.bits_equal(torch.where(torch.isnan(bad), got, bad), got)


@pytest.mark.parametrize('k,identical', X.PHYS_FUSE_CASES)
def test_hand_phys_fuse(k, identical):
    """k in {1, 5} of n_cand = 6; the ten fused rotations as rotations; every other column equals candidate 0 bit for bit"""
    agg = _agg(X.small_assets())
    cand, idx = X.phys_fuse_case(k, identical)
    assert X.phys_fuse_gap(cand, idx) >= X.FUSE_GAP
    ref, f32 = X.hand_phys_fuse(cand.double(), idx), X.hand_phys_fuse(cand, idx)
    got = agg.hand_phys_fuse(_d(cand), _d(idx)).cpu()
    assert got.shape == (3, 58)
    fused = sorted(c for j in X.LVL2_JOINT + X.LVL3_JOINT for c in (3 * j, 3 * j + 1, 3 * j + 2))
    rest = [c for c in range(58) if c not in fused]
    assert X.bits_equal(got[:, rest].contiguous(), cand[:, 0][:, rest].contiguous())
    X.check_rotation(f'hand_phys_fuse k{k} identical={identical}', _aa_rot(got[:, fused]), _aa_rot(ref[:, fused]), _aa_rot(f32[:, fused]),
                     ref[:, fused].abs().max())
    if identical or k == 1:                                                                          # the mean of one rotation is that rotation
        first = cand[torch.arange(3)[:, None], idx[:, :, 0].long()]                                    # (3,5,58): finger f's first pick
        member = torch.cat([first[:, f, 3 * j:3 * j + 3] for f in range(5) for j in (X.LVL2_JOINT[f], X.LVL3_JOINT[f])], -1)
        mine = torch.cat([got[:, 3 * j:3 * j + 3] for f in range(5) for j in (X.LVL2_JOINT[f], X.LVL3_JOINT[f])], -1)
        f32m = torch.cat([f32[:, 3 * j:3 * j + 3] for f in range(5) for j in (X.LVL2_JOINT[f], X.LVL3_JOINT[f])], -1)
        X.check_rotation(f'hand_phys_fuse k{k} vs member', _aa_rot(mine), _aa_rot(member), _aa_rot(f32m), member.abs().max())


@pytest.mark.parametrize('name', X.OBJ_FUSE_CASES)
def test_obj_fuse_float64(name):
    """w_a None (uniform 1/k in float32); two sources with pick_b = [0,1,0,...]; float32 weights whose float32 sum differs from their
    float64 sum (the reference divides by the float32 sum, as the kernel does); bs = 65 (two blocks); identical rotations.  The result is
    float64: rotation within 1e-9 rad of the reference, translation within 1e-12 relative"""
    agg = _agg(X.small_assets())
    pose, idx_a, w_a, idx_b, w_b, pick = X.obj_fuse_case(name)
    idx, w = X.obj_fuse_selected(pose, idx_a, w_a, idx_b, w_b, pick)
    assert X.obj_fuse_gap(pose, idx, w) >= X.FUSE_GAP
    ref = X.obj_fuse(pose, idx, w)
    got = agg.obj_fuse(_d(pose), _d(idx_a), _d(w_a), _d(idx_b), _d(w_b), _d(pick)).cpu()
    assert got.dtype == torch.float64 and got.shape == (65, 9) and bool(torch.isfinite(got).all())
    ang = X.geodesic(X.rot6d_to_matrix(got[:, :6]), X.rot6d_to_matrix(ref[:, :6]))
    X.check(f'obj_fuse {name} rotation', ang, torch.zeros_like(ang), 1e-9)
    X.check_each(f'obj_fuse {name} translation', got[:, 6:], ref[:, 6:], 1e-12 * ref[:, 6:].abs())
    rows = (got[:, :6].reshape(65, 2, 3) ** 2).sum(-1)
    assert float((rows - 1).abs().max()) < 1e-12                                                     # the 6-D output is two unit rows
    if name == 'identical':
        member = X.rot6d_to_matrix(pose[:, 0, :6])
        ang = X.geodesic(X.rot6d_to_matrix(got[:, :6]), member)
        X.check('obj_fuse identical vs member', ang, torch.zeros_like(ang), 1e-9)
    if w is not None and name == 'two_sources':
        assert bool((X.sequential_sum_f32(w).double() != w.double().sum(-1)).any())

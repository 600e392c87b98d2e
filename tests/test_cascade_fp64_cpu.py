"""The float64 restatements of tests/_cascade_fp64.py against oracle/aggregation.py at dtype float64 -- two statements of one formula in
double: they must agree to 1e-12 of the largest compared value -- and the input conditions that tests/test_gpu_cascade_leaves.py relies on
(position classes of the heat-map points, nearest / second-nearest separation, eigen-gap of the quaternion means), for every seed and
case that file uses: the generators are imported from _cascade_fp64, both files see the same tensors.  No GPU."""
import pytest
import torch

from oracle import aggregation as OA
from tests import _cascade_fp64 as X
from vpho_amd.assets import ANCHOR_SKELETON

REL = 1e-12


def agree(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float64
    scale = float(b.abs().max())
    assert scale > 0 and float((a - b).abs().max()) <= REL * scale, (float((a - b).abs().max()), scale)


def _ycb(assets):
    names = list(assets['ycb'])
    return assets['ycb'], names


def test_bicubic16_is_grid_sample_bicubic_zeros_in_range_and_at_the_border():
    d = X.hand_heat_inputs()
    j, r, K, b, hm = X.to64([d['joints'], d['root'], d['K'], d['bbox'], d['heatmap']])
    gx, gy = X.project_norm(j + r[:, None, None], K, b)
    for level in (-1, 0, 1, 2, 3):
        obs = X.observe_list(level)
        mine, S = X.bicubic16(hm[:, obs], gx[:, :, obs], gy[:, :, obs])
        theirs = OA._bicubic_lookup(hm, torch.stack([gx, gy], -1), obs)
        agree(mine, theirs)
        assert bool((S >= mine.abs()).all())
        far = X.HEAT_CLASSES.index('far')
        assert bool((mine[:, far] == 0).all()) and bool((theirs[:, far] == 0).all())
    # the oracle's own projection + normalisation lands on the same grid points
    pt = OA._norm_to_bbox(OA.project(j + r[:, None, None], K), b)
    agree(torch.stack([gx, gy], -1)[:, :-1], pt[:, :-1])                                             # (the far class: 1e6, compared apart)
    agree(torch.stack([gx, gy], -1)[:, -1], pt[:, -1])
    centre = X.HEAT_CLASSES.index('centre')                                                         # on a pixel centre the look-up IS that pixel
    ix, iy = X.heat_grid_indices(d)
    bi, ji = torch.arange(hm.shape[0])[:, None], torch.arange(21)[None]
    px = hm[bi, ji, iy[:, centre].round().long(), ix[:, centre].round().long()]
    assert float((X.hand_heat(j, r, K, b, hm, list(range(21)))[:, centre] - px).abs().max()) < 1e-3


def test_heat_map_points_lie_in_their_position_classes():
    for seed in (0,):
        assert X.heat_classes_hold(X.hand_heat_inputs(seed))


@pytest.mark.parametrize('n_kpt,n', [(5, 1), (5, 9), (27, 9)])
def test_obj_heat_score_is_the_oracles(n_kpt, n):
    assets = X.small_assets(n_kpt=n_kpt, seed=n_kpt)
    tab = X.tables(assets)
    d = X.obj_scene(n_kpt + n, tab, n=n)
    ycb, names = _ycb(assets)
    nm = [names[i] for i in d['obj_id'].tolist()]
    root, kpt, K, bbox, hm = X.to64([d['root'], tab['kpt'], d['K'], d['bbox'], d['heatmap']])
    for transl in (None, d['transl']):
        mine = X.obj_heat_score(d['pose'], transl, root, kpt, d['obj_id'], d['is_right'], K, bbox, hm)
        theirs = OA.obj_heat_scores(ycb, X.with_translation(d['pose'], transl), root, nm, d['is_right'].bool(), K, hm, bbox, dtype=torch.float64)
        agree(mine, theirs)
    assert sorted(d['obj_id'].tolist())[-1] == len(names) - 1 and len(set(d['obj_id'].tolist())) == 3 and d['is_right'].tolist() == [1, 0, 1]
    R6 = d['pose'][..., :6]
    assert float(((R6[..., :3] * R6[..., 3:]).sum(-1)).abs().min()) > 1e-3                            # not orthonormal: Gram-Schmidt matters


@pytest.mark.parametrize('n_vert,n', X.PHYSICS_CASES)
def test_obj_physics_score_is_the_oracles_and_the_nearest_vertex_is_separated(n_vert, n):
    assets, d = X.physics_case(n_vert, n)
    tab = X.tables(assets)
    ycb, names = _ycb(assets)
    nm = [names[i] for i in d['obj_id'].tolist()]
    sep = X.nearest_separation(d['pose'], d['root'], tab['vert'], d['obj_id'], d['is_right'], d['force_point'])
    assert sep >= X.SEPARATION, sep
    assert float(d['force_global'].norm(dim=-1).min()) > 1e-3
    assert bool((d['pose'].float().double() == d['pose']).all())                                      # float32 values: the kernel's (float) cast is exact
    root, vert, com, fp, fg = X.to64([d['root'], tab['vert'], tab['com'], d['force_point'], d['force_global']])
    mine = X.obj_physics_score(d['pose'], root, vert, com, d['obj_id'], d['is_right'], fp, fg)
    theirs = OA.obj_physics_scores(ycb, d['pose'], root, nm, d['is_right'].bool(), fp, fg, dtype=torch.float64)
    agree(mine, theirs)
    verts = X.obj_points(d['pose'], root, vert, d['obj_id'], d['is_right'])
    dist = X.squared_distances(fp[:, None], verts).min(dim=-1)[0].sqrt()
    assert float(dist.max()) < 0.09                                                                  # within centimetres of the cloud


def test_the_constructed_tie_is_a_tie_and_the_rule_decides_the_score():
    assets, d, i, j = X.tie_case()
    tab = X.tables(assets)
    args = [d['pose'], d['root'].double(), tab['vert'].double(), tab['com'].double(), d['obj_id'], d['is_right'], d['force_point'].double(), d['force_global'].double()]
    d2 = (tab['vert'][0] ** 2).sum(-1)                                                               # the float32 squared distances to the origin
    assert i < j and float(d2[i]) == float(d2[j]) and float(d2[i]) < float(torch.cat([d2[:i], d2[i + 1:j], d2[j + 1:]]).min())
    assert i % 8 != j % 8                                                                            # different lanes of the 8-lane search
    first = X.obj_physics_score(*args)
    other = X.obj_physics_score(*args, pick=torch.full((1, 1, 32), j))
    agree(first, X.obj_physics_score(*args, pick=torch.full((1, 1, 32), i)))
    assert float((first - other).abs().min()) > 1e-3 * float(first.abs().max())


def test_average_quaternion_and_fuse_topk_are_the_oracles():
    g = X.gen(11)
    Q = X.clustered_quaternions((4, 3), 6, g)
    Q[:, :, ::2] = -Q[:, :, ::2]                                                                     # mixed signs: the q0 > 0 fix acts
    W = 0.1 + torch.rand(4, 3, 6, generator=g, dtype=torch.float64)
    agree(X.average_quaternion(Q, W), OA.average_quaternion(Q, W))
    agree(X.average_quaternion(Q), OA.average_quaternion(Q))
    for name in X.OBJ_FUSE_CASES:
        pose, idx_a, w_a, idx_b, w_b, pick = X.obj_fuse_case(name)
        idx, _ = X.obj_fuse_selected(pose, idx_a, w_a, idx_b, w_b, pick)
        w = (torch.randint(1, 64, idx.shape, generator=g) / 64.0).float()                            # dyadic: the float32 sum of the weights is exact
        assert bool((X.sequential_sum_f32(w).double() == w.double().sum(-1)).all())
        mine = X.obj_fuse(pose, idx, w)
        theirs = OA.fuse_topk(pose, idx.long(), w.double())
        assert float(X.geodesic(X.rot6d_to_matrix(mine[:, :6]), X.rot6d_to_matrix(theirs[:, :6])).max()) < 1e-12
        agree(mine, theirs)
    # the rotation conversions the restatements spell out are the oracle's
    from oracle import rotations as OR
    aa = torch.randn(50, 3, generator=g, dtype=torch.float64) * 2
    agree(X.axis_angle_to_quaternion(aa), OR.axis_angle_to_quaternion(aa))
    q = X._unit(torch.randn(50, 4, generator=g, dtype=torch.float64))
    agree(X.quaternion_to_axis_angle(q), OR.quaternion_to_axis_angle(q))
    agree(X.quaternion_to_matrix(q), OR.quaternion_to_matrix(q))
    agree(X.matrix_to_quaternion(X.quaternion_to_matrix(q)), OR.matrix_to_quaternion(OR.quaternion_to_matrix(q)))
    d6 = torch.randn(50, 6, generator=g, dtype=torch.float64)
    agree(X.rot6d_to_matrix(d6), OR.rotation_6d_to_matrix(d6))


@pytest.mark.parametrize('n_hands,hpi', [(1, 1), (8, 1), (8, 4)])
def test_force_anchor_is_local_to_global_on_verts_plus_root(n_hands, hpi):
    assets = X.small_assets(dense_v2j=True)
    tab = X.tables(assets)
    assert bool((tab['v2j'] > 0).all()) and float((tab['v2j'].sum(1) - 1).abs().max()) < 1e-6          # dense: the full 778-term reduction
    verts, root, fl = X.force_anchor_inputs(n_hands, hpi)
    skel = torch.as_tensor(ANCHOR_SKELETON).long()
    fp, fg = X.force_anchor(verts.double(), root.double(), fl.double(), hpi, tab['face'], tab['aw'].double(), tab['v2j'].double(), skel)
    img = torch.arange(n_hands) // hpi
    anchor64 = {k: torch.as_tensor(v).double() if k != 'face_vert_idx' else v for k, v in assets['anchor'].items()}
    rp, rg = OA.local_to_global(anchor64, ANCHOR_SKELETON, fl.double()[img], verts.double() + root.double()[img][:, None])
    agree(fp, rp)
    agree(fg, rg)
    assert X.faces_are_not_degenerate(verts, tab['face'])
    if n_hands // hpi > 1:                                                                          # per-image rows distinct: h // hpi is provable
        assert float((root[0] - root[1]).abs().min()) > 1e-3 and float((fl[0] - fl[1]).abs().max()) > 1e-2


def test_the_quaternion_means_are_well_conditioned_for_every_case():
    for name in X.POSE_FUSE_CASES:
        assert X.pose_fuse_gap(*X.pose_fuse_case(name)) >= X.FUSE_GAP, name
    for k, identical in X.PHYS_FUSE_CASES:
        assert X.phys_fuse_gap(*X.phys_fuse_case(k, identical)) >= X.FUSE_GAP, (k, identical)
    for name in X.OBJ_FUSE_CASES:
        case = X.obj_fuse_case(name)
        idx, w = X.obj_fuse_selected(*case)
        assert X.obj_fuse_gap(case[0], idx, w) >= X.FUSE_GAP, name
    pose, idx, w, n = X.pose_fuse_case('idx_w')                                                       # members written the long way round are there
    ang = pose[..., :48].reshape(5, 6, 16, 3).norm(dim=-1)
    assert bool((ang > 3.1416).any()) and bool((ang < 3.1415).any()) and float(ang.max()) < 6.2832
    _, _, w_a, _, w_b, _ = X.obj_fuse_case('two_sources')                                            # float32 sum of the weights != their float64 sum
    assert bool((X.sequential_sum_f32(w_a).double() != w_a.double().sum(-1)).any())


def test_the_exact_peak_of_the_pt2d_inputs_is_exact_in_float32_and_float64():
    d = X.pt2d_inputs()
    for args in ([d['joints'], d['root'], d['K'], d['bbox'], d['peak']], X.to64([d['joints'], d['root'], d['K'], d['bbox'], d['peak']])):
        s = X.hand_pt2d_score(*args, True)
        assert float(s[1, 7, 4]) == 0.0 and int((s == 0).sum()) == 1

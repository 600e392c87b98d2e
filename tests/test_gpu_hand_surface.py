"""csrc/hand_surface.hip and the label chain behind it on the GPU.

Kernel = the float64 restatement of tests/_hand_surface_fp64.py (another route: a loop over vertices, angles from arctan2) rounded to
float32: every value within 1 float32 ulp (np.spacing) and at most 1 value in 10^4 different at all.  float64 noise of ~1e-15 straddles
a float32 rounding boundary with probability ~1e-8 per value; the cap is a condition that absorbs libm differences in acos, not a
measurement.  Only rows whose summed normal is >= 1e-6 of its angle sum are compared (the planted cancelling faces are not).  Every
mesh is posed by a random rotation first: a component that is zero by symmetry would carry float64 noise far above ITS float32 ulp.

Chain: HandSurface.fill -> Aggregation.hand_contact -> force_contact against the reference's own values (golden_hand_surface.npz) and
against the restatement.  Left out are vertices whose float64 normal or vertical distance lies within 1e-5 m of a gate or whose two
nearest object points differ by less than 1e-6 m (at most 1 %); outside that band masks are identical, weights within 2e-3 (the bound
tests/test_gpu_contact.py holds this kernel to: float32 coordinates under exp(1600 x)), pooled force_contact follows at rtol 1e-5 /
atol 1e-7, is_grasped is equal wherever no group sum is within 2e-3 of 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hand_surface_fp64 as HS  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES = HS.CALL_GATES


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_hand_surface.npz')))


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _judge(name, got, want64, rows=None):
    """got: float32 from the kernel, want64: the restatement; rows: boolean mask over the leading axes"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    with np.errstate(invalid='ignore'):
        want = np.asarray(want64).astype(np.float32)
    assert got.shape == want.shape and got.dtype == np.float32, (name, got.shape, want.shape, got.dtype)
    if rows is not None:
        got, want = got[rows], want[rows]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f'{name}: NaN pattern differs at {int((np.isnan(got) != nan).sum())} values'
    g, w = got[~nan], want[~nan]
    err = np.abs(g.astype(np.float64) - w.astype(np.float64))
    differ = int((g != w).sum())
    print(f'{name}: {g.size} values compared, {differ} differ, worst {float((err / np.spacing(np.abs(w))).max(initial=0.0)):.2f} ulp')
    assert (err <= np.spacing(np.abs(w))).all(), f'{name}: {int((err > np.spacing(np.abs(w))).sum())} values beyond 1 ulp'
    assert differ <= 1e-4 * g.size, f'{name}: {differ} of {g.size} values differ'


def _check_surface(name, verts32, faces, links, alpha, n_verts=None, want_all=False):
    from vpho_amd import ops
    surface = ops.HandSurface(faces, links, alpha, 'cuda', n_verts=n_verts)
    vf, nf = surface.fill(_dev(verts32))
    torch.cuda.synchronize()
    wv, wn, length, angles = HS.hand_surface(verts32, faces, links, alpha)
    V = verts32.shape[1]
    assert tuple(vf.shape) == tuple(nf.shape) == (verts32.shape[0], V + len(links), 3)
    rows = HS.comparable_rows(length, angles, links, V)
    _judge(name + ' verts', vf, wv)
    _judge(name + ' normals', nf, wn, rows)
    if want_all:
        assert rows.all(), (name, int((~rows).sum()))
    zero = np.concatenate([angles == 0, np.zeros((len(verts32), len(links)), bool)], 1)          # unreferenced vertices: exactly the zero vector
    assert not nf.cpu().numpy()[zero].any()
    return surface, vf, nf, rows


def _posed_batch(v, n, seed, scale=1.0):
    return np.stack([HS.posed(v, seed + i, scale) for i in range(n)])


# ------------------------------------------------------------------------------------------------------------------ kernel = restatement
def test_tetrahedron_and_cube():
    v, f = HS.tetrahedron()
    _check_surface('tetrahedron (1, 4, 4, 1)', _posed_batch(v, 1, 1, 0.02), f, [[0, 3]], [0.3], want_all=True)
    v, f = HS.cube(0)
    _check_surface('cube (2, 8, 12, 3)', _posed_batch(v, 2, 5, 0.03), f, [[0, 7], [1, 2], [3, 3]], [1 / 3, 0.25, 0.5], want_all=True)


@pytest.mark.parametrize('n', [3, 70])
def test_the_hand_sized_mesh_with_the_real_table(gold, n):
    """(n, 778, 1552, 302); 70 samples are more workgroups than one wave of the grid needs, and 100 KB of LDS take the large-LDS opt-in"""
    v, f = HS.ellipsoid()
    _check_surface(f'ellipsoid n={n}', _posed_batch(v, n, 40), f, gold['links'], gold['alpha'], want_all=True)


def test_open_mesh_no_links_and_the_size_limits(gold):
    v, f = HS.ellipsoid()
    open_f = f[(f != 0).all(1)]                                                   # the north pole's fan dropped: boundary vertices, pole unreferenced
    assert len(open_f) == 1552 - 97
    _, _, nf, rows = _check_surface('open mesh', _posed_batch(v, 2, 60), open_f, gold['links'], gold['alpha'], n_verts=778)
    assert not rows[:, 0].any() and rows[:, 1:778].all()
    _check_surface('L = 0', _posed_batch(v, 2, 62), f, np.zeros((0, 2), np.int64), np.zeros(0), want_all=True)
    r = np.random.default_rng(5)                                                   # V = 1024, F = 2048, L = 1024: 132 KB of LDS
    big_v = r.normal(0, 0.05, (2, 1024, 3)).astype(np.float32)
    big_f = np.stack([r.permutation(1024)[:3] for _ in range(2048)])
    big_l = r.integers(0, 1024, (1024, 2))
    _check_surface('limits', big_v, big_f, big_l, r.uniform(0, 1, 1024))


def test_degenerate_faces_unreferenced_vertices_and_a_nan():
    v, f = HS.octahedron()
    v = np.concatenate([v, [[5.0, 5.0, 5.0]]])                                      # vertex 6 is referenced by no face
    f2 = np.concatenate([f, [[0, 0, 2]], [[0, 2, 4]], [[0, 4, 2]]])                 # a repeated index; two coincident opposite faces (they cancel)
    # (4, 2) are neighbours: halfway between OPPOSITE vertices the interpolated normal would cancel and its direction be rounding noise
    links, alpha = [[5, 6], [4, 2], [5, 5], [0, 1]], [0.25, 0.5, 1 / 3, 0.75]
    p = _posed_batch(v, 2, 70, 0.04)
    _, _, nf, rows = _check_surface('degenerate', p, f2, links, alpha, n_verts=7)
    assert rows[:, :6].all() and not nf[:, 6].any()
    _, _, nf0, rows0 = _check_surface('cancelling pair only', p, [[0, 2, 4], [0, 4, 2]], links, alpha, n_verts=7)
    assert not rows0.any() and not nf0[:, :7].any()                                  # zero sums: zero normals, nothing compared
    bad = p.copy()
    bad[1, 4, 1] = np.nan                                                           # sample 1, the apex of four faces
    _, vf, nf, _ = _check_surface('NaN vertex', bad, f, links, alpha, n_verts=7)
    vf, nf = vf.cpu().numpy(), nf.cpu().numpy()
    assert np.isfinite(vf[0]).all() and np.isfinite(nf[0]).all()                     # the other sample is untouched
    assert np.isnan(nf[1, [0, 1, 2, 3, 4]]).all() and np.isfinite(nf[1, [5, 6]]).all()          # its faces' vertices; vertex 5 shares no face with it
    assert np.isfinite(nf[1, [7, 9]]).all() and np.isnan(nf[1, [8, 10]]).all()       # links (5,6), (5,5) stay finite, (4,2), (0,1) do not
    assert np.isnan(vf[1, 8, 1]) and np.isfinite(np.delete(vf[1].reshape(-1), [4 * 3 + 1, 8 * 3 + 1])).all()


def test_no_samples_refusals_sentinels_and_a_repeat_run(gold):
    from vpho_amd import ops
    v, f = HS.ellipsoid()
    surface = ops.HandSurface(f, gold['links'], gold['alpha'], 'cuda')
    vf, nf = surface.fill(torch.zeros(0, 778, 3, device='cuda'))
    assert tuple(vf.shape) == tuple(nf.shape) == (0, 1080, 3)
    with pytest.raises(ops.VphoError, match='1025 vertices'):
        ops.HandSurface(f, gold['links'], gold['alpha'], 'cuda', n_verts=1025)
    with pytest.raises(ops.VphoError, match='2049 faces'):
        ops.HandSurface(np.zeros((2049, 3), np.int64), gold['links'], gold['alpha'], 'cuda', n_verts=778)
    with pytest.raises(ops.VphoError, match='1025 links'):
        ops.HandSurface(f, np.zeros((1025, 2), np.int64), np.zeros(1025), 'cuda')
    wrong = f.copy()
    wrong[7, 1] = 778
    with pytest.raises(ops.VphoError, match=r'face 7 = \[.*778.*\] indexes outside the 778 vertices'):
        ops.HandSurface(wrong, gold['links'], gold['alpha'], 'cuda', n_verts=778)
    with pytest.raises(ops.VphoError, match='link 0'):
        ops.HandSurface(f, [[0, -1]], [0.5], 'cuda', n_verts=778)
    with pytest.raises(ops.VphoError, match='built for'):
        surface.fill(torch.zeros(1, 777, 3, device='cuda'))
    # the C side repeats the limits
    table =ops.HandSurfaceTable(surface.faces.data_ptr(), surface.csr_offset.data_ptr(), surface.csr_entry.data_ptr(), surface.links.data_ptr(),
                                 surface.alpha.data_ptr(), 1025, 1552, 302)
    assert ops.lib.vpho_hand_surface_f32(ops.C.byref(table), None, 0, None, None, None) != 0 and b'1025 vertices' in ops.lib.vpho_last_error()
    # sentinels behind both outputs, and two runs give the same bits
    verts = _dev(_posed_batch(v, 5, 80))
    n_out = 5 * 1080 * 3
    bufs = [torch.full((n_out + 64,), -77.0, device='cuda') for _ in range(2)]
    out = tuple(b[:n_out].view(5, 1080, 3) for b in bufs)
    surface.fill(verts, out=out)
    a = surface.fill(verts)
    b = surface.fill(verts)
    torch.cuda.synchronize()
    for k in range(2):
        assert bool((bufs[k][n_out:] == -77.0).all()) and torch.equal(out[k], a[k]) and torch.equal(a[k], b[k])
    assert bool(torch.isfinite(a[1]).all()) and float((a[1].double().norm(dim=-1) - 1).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ chain
def _judge_chain(name, hc, fc, grasped, filled_v, filled_n, cloud, anchors, ref_hc=None):
    """hc (Nh,), fc (32,), grasped: the kernels' values for one sample; filled_v / filled_n / cloud: what hand_contact was given"""
    chain = HS.hand_contact(filled_v, filled_n, cloud, **GATES)
    out = HS.band(chain, GATES['normal_thresh'], GATES['vertical_thresh'])
    want = np.clip(chain['weight'], 0, 1) if ref_hc is None else ref_hc
    print(f'{name}: band {int(out.sum())} of {len(out)}, in contact {int((want > 0).sum())}, worst weight error {float(np.abs(hc - want)[~out].max()):.2e}')
    assert out.mean() <= 0.01
    assert np.array_equal((hc > 0)[~out], (want > 0)[~out])
    assert np.abs(hc - want)[~out].max() <= 2e-3
    assert hc.min() >= 0 and hc.max() <= 1
    pooled = HS.force_contact(hc, *anchors)                                          # the pooling of the kernel's own map
    np.testing.assert_allclose(fc, pooled, rtol=1e-5, atol=1e-7)
    if np.abs(HS.group_sums(pooled)).min() > 2e-3:
        assert bool(grasped) == bool(HS.is_grasped(pooled))
    return chain, out


def test_chain_on_the_reference_cases(gold, assets):
    from vpho_amd import ops
    from vpho_amd.assets import ANCHOR_SKELETON
    agg = ops.Aggregation(assets, ANCHOR_SKELETON, 'cuda')
    surface = ops.HandSurface(gold['faces'], gold['links'], gold['alpha'], 'cuda')
    anchors = (assets['anchor']['face_vert_idx'], assets['anchor']['anchor_weight'])
    verts = np.stack([gold[f'case{k}_verts'] for k in range(3)])
    cloud = np.stack([gold[f'case{k}_cloud'] for k in range(3)])
    vf, nf = surface.fill(_dev(verts))
    _judge('fixture verts', vf, np.stack([gold[f'case{k}_verts_filled'] for k in range(3)]).astype(np.float64))
    _judge('fixture normals', nf, np.stack([gold[f'case{k}_normals_filled'] for k in range(3)]).astype(np.float64))
    hc = agg.hand_contact(vf, nf, _dev(cloud), GATES['normal_thresh'], GATES['vertical_thresh'], GATES['decay']).clamp_(0, 1)
    fc, gr = agg.force_contact(hc)
    torch.cuda.synchronize()
    for k in range(3):
        ref = gold[f'case{k}_hand_contact']
        _, out = _judge_chain(f'case {k} vs the reference', hc[k].cpu().numpy().astype(np.float64), fc[k].cpu().numpy().astype(np.float64), gr[k].item(),
                              vf[k].cpu().numpy(), nf[k].cpu().numpy(), cloud[k], anchors, ref_hc=ref)
        # the reference's own pooled values: an anchor none of whose three vertices lies in the band is a convex combination of three weights
        # that are each within 2e-3; the grasp flag wherever no group sum of the reference is within 2e-3 of 0 and no band vertex is pooled
        ref_fc = gold[f'case{k}_force_contact']
        clean = ~np.isin(np.asarray(anchors[0]), np.flatnonzero(out)).any(1)
        assert clean.any() and np.abs(fc[k].cpu().numpy() - ref_fc)[clean].max() <= 2e-3 + 1e-6
        if clean.all() and np.abs(HS.group_sums(ref_fc)).min() > 2e-3:
            assert bool(gr[k].item()) == bool(gold[f'case{k}_is_grasped'])


class _LabelCfg:
    def __init__(self, asset_root):
        from vpho_amd.configs.args import Config
        self.__dict__.update(Config().__dict__)
        self.asset_root = asset_root


@pytest.fixture(scope='module')
def real_table_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('asset_with_gap_table'))
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import install_gap_table
    install_gap_table.main([root])
    return root


def test_labeler_on_a_mixed_batch_through_the_padded_table(gold, assets, real_table_root):
    """three objects of 1500, 2048 and 700 vertices in one launch, a left hand among them: equal to the restatement outside the band and
    to per-object launches on the unpadded vertices bit for bit"""
    from vpho_amd.assets import YCB_NAMES
    from vpho_amd.physics_labels import PhysicsLabeler
    base, faces = HS.ellipsoid()
    ids, counts, right = [1, 5, 12], [1500, 2048, 700], [True, False, True]
    mine = dict(assets, mano=dict(assets['mano'], faces=faces), ycb={k: dict(v) for k, v in assets['ycb'].items()})
    for i, c in zip(ids, counts):
        mine['ycb'][YCB_NAMES[i]]['verts'] = assets['ycb'][YCB_NAMES[i]]['verts'][:c]
    lab = PhysicsLabeler(_LabelCfg(real_table_root), mine, 'cuda')
    assert lab.gap['source'].endswith('finger_gap_links.npz') and tuple(lab.obj_verts.shape) == (21, 2048, 3)
    r = np.random.default_rng(9)
    hv = np.repeat(base.astype(np.float32)[None], 3, 0)
    root = r.uniform(-0.05, 0.05, (3, 3)) + [0, 0, 0.7]
    rt = np.zeros((3, 3, 4))
    for s, i in enumerate(ids):                                                    # the box's top face just under the hand's underside
        half = np.abs(assets['ycb'][YCB_NAMES[i]]['verts']).max(0)
        a = r.uniform(0, 2 * np.pi)
        rt[s, :, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        rt[s, :, 3] = root[s] + [r.uniform(-0.01, 0.01), r.uniform(-0.005, 0.005), -half[2] - 0.015 + r.uniform(-0.001, 0.002)]
    batch = dict(gt_hand_vert_flip=_dev(hv), gt_obj_rt=_dev(rt), root_joint=_dev(root), obj_id=torch.tensor(ids).cuda(), is_right=torch.tensor(right).cuda())
    out = lab(batch)
    ov = lab.object_verts(batch['gt_obj_rt'], batch['root_joint'], batch['obj_id'], batch['is_right'])
    vf, nf = lab.surface.fill(batch['gt_hand_vert_flip'])
    torch.cuda.synchronize()
    assert tuple(out['hand_contact'].shape) == (3, 1080) and tuple(out['force_contact'].shape) == (3, 32) and out['is_grasped'].dtype == torch.bool
    sign = np.where(right, 1.0, -1.0)
    rt32, root32 = rt.astype(np.float32).astype(np.float64), root.astype(np.float32).astype(np.float64)
    anchors = (assets['anchor']['face_vert_idx'], assets['anchor']['anchor_weight'])
    for s, (i, c) in enumerate(zip(ids, counts)):
        v = assets['ycb'][YCB_NAMES[i]]['verts'][:c].astype(np.float64)
        want = v @ rt32[s, :, :3].T + (rt32[s, :, 3] - root32[s])
        want[:, 0] *= sign[s]
        got = ov[s].cpu().numpy()
        assert np.abs(got[:c] - want).max() <= np.spacing(np.float32(np.abs(want).max())) and np.array_equal(got[c:], np.repeat(got[c - 1:c], 2048 - c, 0))
        hc = out['hand_contact'][s].cpu().numpy().astype(np.float64)
        assert (hc > 0).sum() >= 5, (s, int((hc > 0).sum()))
        _judge_chain(f'mixed batch sample {s}', hc, out['force_contact'][s].cpu().numpy().astype(np.float64), out['is_grasped'][s].item(),
                     vf[s].cpu().numpy(), nf[s].cpu().numpy(), got[:c], anchors)
        alone = lab.agg.hand_contact(vf[s:s + 1].contiguous(), nf[s:s + 1].contiguous(), ov[s:s + 1, :c].contiguous(), lab.normal_thresh, lab.vertical_thresh,
                                     lab.DECAY).clamp_(0, 1)
        assert torch.equal(alone[0], out['hand_contact'][s])                         # the padding changes no bit
    with pytest.raises(ValueError, match='no hand_vert'):
        lab({k: v for k, v in batch.items() if k != 'gt_hand_vert_flip'})


# ------------------------------------------------------------------------------------------------------------------ labeler and entry points
def _frame_batches(assets, cfg, n, bs, seed=7):
    from vpho_amd import frames as FR
    src = FR.synthetic_frames(n, assets, seed=seed, size=(160, 120))
    return src, list(FR.FrameLoader(src, bs, FR.FramePipeline(cfg, assets, 'cuda', train=False, seed=seed)))


def test_full_batches_and_a_remainder_are_the_two_explicit_calls(assets, tmp_path):
    from vpho_amd.physics_labels import PhysicsLabeler
    cfg = _LabelCfg(str(tmp_path))
    lab = PhysicsLabeler(cfg, assets, 'cuda')
    assert lab.gap['source'] == 'synthetic'
    _, (batch,) = _frame_batches(assets, cfg, 19, 19)
    right = batch['is_right'].cpu().numpy()
    assert right.any() and (~right).any()                                           # left and right hands
    out = lab(batch, optimize=True, batch_size=8, iters=60, phase1=10)
    sign = torch.where(batch['is_right'], 1.0, -1.0)
    flip = lambda a: torch.stack([a[:, 0, 0] * sign, a[:, 0, 1], a[:, 0, 2]], -1).contiguous()
    grav, com, hv = flip(batch['gravity']), flip(batch['obj_CoM']), batch['gt_hand_vert_flip'].contiguous()
    fc, gr = out['force_contact'], out['is_grasped'].to(torch.uint8)
    one = lab.agg.force_optimize(hv[:16].contiguous(), grav[:16].contiguous(), com[:16].contiguous(), fc[:16].contiguous(), gr[:16].contiguous(), 8, iters=60, phase1=10)
    two = lab.agg.force_optimize(hv[16:].contiguous(), grav[16:].contiguous(), com[16:].contiguous(), fc[16:].contiguous(), gr[16:].contiguous(), 3, iters=60, phase1=10)
    torch.cuda.synchronize()
    for k in ('force_local', 'force_global'):
        assert tuple(out[k].shape) == (19, 32, 3) and torch.equal(out[k], torch.cat([one[k], two[k]])), k
    assert tuple(out['losses'].shape) == (3, 4) and torch.equal(out['losses'], torch.cat([one['losses'], two['losses']]))
    assert bool(torch.isfinite(out['force_local']).all()) and not out['force_local'][~out['is_grasped']].any()


def _child(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_force_optim_labels_a_synthetic_source_in_a_child_process(tmp_path):
    path = str(tmp_path / 'labels' / 'physics_labels.npz')
    r = _child([os.path.join(ROOT, 'force_optim.py'), '--frame_source', 'synthetic', '--num_frames', '40', '--batch_size', '16', '--iters', '60', '--phase1', '10',
                '--out', path])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['pairs'] == 40 and d['value'] > 0 and d['unit'] == 'pairs/s' and 0 <= d['grasped_share'] <= 1 and len(d['mean_losses_force_gravity_moment_dist']) == 4
    z = dict(np.load(path))
    shapes = dict(index=(40,), hand_contact=(40, 1080), force_contact=(40, 32), is_grasped=(40,), force_local=(40, 32, 3), force_global=(40, 32, 3))
    assert {k: z[k].shape for k in shapes} == shapes and z['index'].tolist() == list(range(40)) and z['is_grasped'].dtype == bool
    assert np.isfinite(z['force_local']).all() and not z['force_local'][~z['is_grasped']].any() and not z['force_global'][~z['is_grasped']].any()
    assert z['hand_contact'].min() >= 0 and z['hand_contact'].max() <= 1
    meta = json.loads(str(z['meta']))
    assert meta['contact_normal_distance_thresh'] == [-0.01, 0.01] and meta['contact_vertical_distance_thresh'] == 0.005 and meta['iters'] == 60
    assert meta['phase1'] == 10 and meta['gap_table'] == 'synthetic' and 'SYNTHETIC links' in r.stderr
    bad = _child([os.path.join(ROOT, 'force_optim.py'), '--frame_source', 'synthetic'])
    assert bad.returncode != 0 and '--out' in bad.stderr


class _Cfg:
    """the global cfg with a few attributes set for the length of a test"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from vpho_amd.configs.args import cfg
        self.saved = {k: getattr(cfg, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(cfg, k, v)
        return cfg

    def __exit__(self, *exc):
        from vpho_amd.configs.args import cfg
        for k, v in self.saved.items():
            setattr(cfg, k, v)


SMALL = dict(sample_num=4, sampling_steps=5, topk_hand=8, topk_obj=3, sample_T0=0.2, eval_batch_size=4, batch_size=4, num_batches=2, repeat_num=4,
             random_seed=7, checkpoint='')
ARGS = ['--sample_num', '4', '--sampling_steps', '5', '--topk_hand', '8', '--topk_obj', '3', '--sample_T0', '0.2', '--eval_batch_size', '4', '--num_batches', '2',
        '--random_seed', '7']
PARENT_KEYS = {'rgb', 'hm_hand', 'hm_obj', 'bbox_hand', 'bbox_obj', 'bbox_hand_rect', 'bbox_obj_rect', 'gt_jt2d', 'gt_obj2d', 'cam_intr_crop', 'cam_intr_crop_flip',
               'cam_intr', 'gt_joint', 'root_joint', 'root_joint_flip', 'gt_hand_jt3d_flip', 'gt_hand_vert', 'gt_hand_vert_flip', 'gt_obj_rt', 'gt_obj', 'obj_CoM',
               'gravity', 'gt_mano', 'is_right', 'is_ho3d', 'is_grasped', 'force_local', 'obj_name', 'obj_id', 'index'}


def test_label_file_feeds_a_training_step_and_frame_contact_an_evaluation(tmp_path):
    from vpho_amd import frames as FR
    from vpho_amd.physics_labels import PhysicsLabeler
    from vpho_amd.trainer import Trainer
    d = str(tmp_path / 'frames')
    with _Cfg(train_scope='full', asset_root=str(tmp_path), **SMALL) as cfg:
        tr = Trainer(cfg)
        src = FR.synthetic_frames(8, tr.assets, seed=7)
        FR.write_frame_directory(d, src)
        lab = PhysicsLabeler(cfg, tr.assets, tr.device)
        plain = list(FR.FrameLoader(FR.FrameDirectory(d), 4, FR.FramePipeline(cfg, tr.assets, tr.device, train=False, seed=7)))
        assert all(set(b) == PARENT_KEYS for b in plain)
        outs = [lab(b, optimize=True, batch_size=4, iters=40, phase1=10) for b in plain]
        cat = lambda k: torch.cat([o[k] for o in outs]).cpu().numpy()
        np.savez(os.path.join(d, FR.LABEL_FILE), index=np.arange(8), hand_contact=cat('hand_contact'), force_contact=cat('force_contact'),
                 is_grasped=cat('is_grasped'), force_local=cat('force_local'), force_global=cat('force_global'), meta=np.array(json.dumps(lab.meta())))
        labelled = FR.FrameDirectory(d)
        fed = list(FR.FrameLoader(labelled, 4, FR.FramePipeline(cfg, tr.assets, tr.device, train=False, seed=7)))
        for b, o, p in zip(fed, outs, plain):                                       # the labels reach the batch; everything else is unchanged
            assert torch.equal(b['is_grasped'], o['is_grasped']) and torch.equal(b['force_local'], o['force_local'])
            assert all(torch.equal(b[k], p[k]) for k in ('rgb', 'hm_hand', 'gt_mano', 'gt_hand_vert_flip'))
        hist = tr.run(n_batches=1, loader=FR.FrameLoader(labelled, 4, FR.FramePipeline(cfg, tr.assets, tr.device, train=True, seed=7), drop_last=True))
        assert len(hist) >= 1 and all(np.isfinite(v) for v in hist[0].values()), hist
        # --frame_contact: the labels per batch, is_grasped from the device
        with _Cfg(frame_contact=True):
            online = list(FR.FrameLoader(src, 4, FR.FramePipeline(cfg, tr.assets, tr.device, train=False, seed=7)))
            rows = tr.eval(FR.FrameLoader(src, 4, FR.FramePipeline(cfg, tr.assets, tr.device, train=False, seed=7)))
        assert rows.shape[0] == 8 and bool(torch.isfinite(rows).all())
        for b, o, p in zip(online, outs, plain):
            assert set(b) == PARENT_KEYS | {'hand_contact', 'force_contact'}
            assert torch.equal(b['is_grasped'], o['is_grasped']) and torch.equal(b['hand_contact'], o['hand_contact']) and torch.equal(b['force_contact'], o['force_contact'])
            for k in PARENT_KEYS - {'is_grasped', 'obj_name'}:                      # flag on or off: every other key has the same bytes
                assert torch.equal(b[k], p[k]), k
            # the flag off: the record's own value, as before
            assert b['obj_name'] == p['obj_name'] and p['is_grasped'].cpu().tolist() == [bool(src[int(i)][1]['is_grasped']) for i in p['index']]


_CONTACT_SCRIPT = '''
import sys, numpy as np, torch
sys.argv = ['main.py', '--mode', 'eval', '--model', 'vpho_net', '--frame_source', 'synthetic'] + {args!r}
import main
from vpho_amd import frames as FR
kept = []
plain = FR.FramePipeline.__call__
def keep(self, *a, **k):
    b = plain(self, *a, **k)
    kept.append(b)
    return b
FR.FramePipeline.__call__ = keep
main.main()
torch.cuda.synchronize()
np.savez({out!r}, keys=np.array(sorted(kept[0])), is_grasped=torch.cat([b['is_grasped'] for b in kept]).cpu().numpy(),
         index=torch.cat([b['index'] for b in kept]).numpy(), labels_imported=np.array('vpho_amd.physics_labels' in sys.modules))
'''


@pytest.mark.parametrize('flag', [True, False])
def test_main_eval_with_and_without_frame_contact_in_a_child_process(tmp_path, assets, flag):
    out = str(tmp_path / 'kept.npz')
    r = _child(['-c', _CONTACT_SCRIPT.format(args=ARGS + (['--frame_contact'] if flag else []), out=out)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'evaluated 8 images on 1 GPU(s)' in r.stdout, r.stdout[-2000:]
    z = dict(np.load(out))
    assert z['index'].tolist() == list(range(8)) and bool(z['labels_imported']) == flag
    assert set(z['keys'].tolist()) == PARENT_KEYS | ({'hand_contact', 'force_contact'} if flag else set())
    from vpho_amd import frames as FR
    src = FR.synthetic_frames(8, assets, seed=7)
    if not flag:
        assert z['is_grasped'].tolist() == [bool(src[i][1]['is_grasped']) for i in range(8)]
        return
    from vpho_amd.physics_labels import PhysicsLabeler
    with _Cfg(**SMALL) as cfg:
        lab = PhysicsLabeler(cfg, assets, 'cuda')
        want = torch.cat([lab(b)['is_grasped'] for b in FR.FrameLoader(src, 4, FR.FramePipeline(cfg, assets, 'cuda', train=False, seed=7))])
    assert z['is_grasped'].tolist() == want.cpu().tolist()

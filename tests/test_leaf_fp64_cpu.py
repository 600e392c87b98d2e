"""The float64 leaf references of tests/_leaf_fp64.py checked against each other, against the CPU oracle and against the committed golden of the physics training step
(tests/golden/golden_physics_train.npz):
a wrong reference must not be what the GPU tests (test_gpu_leaf_forward.py / test_gpu_leaf_train.py) measure the kernels with.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _leaf_fp64 as R

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.mark.parametrize('S,C', [(64, 21), (32, 1), (7, 3)])
@pytest.mark.parametrize('kind', ['equal', 'larger', 'smaller'])
def test_align_heatmap_gather_equals_grid_sample(S, C, kind):
    g = R.gen(S * 10 + C)
    N = 4
    hm = torch.randn(N, S, S, C, generator=g, dtype=torch.float64)
    bbox, rect = R.boxes(N, g, kind, torch.float64)
    flip = torch.tensor([0, 1, 0, 1], dtype=torch.uint8)
    a, b = R.align_heatmap_gather(hm, bbox, rect, flip), R.align_heatmap_grid_sample(hm, bbox, rect, flip)
    assert a.shape == (N, S, S, C)
    assert float((a - b).abs().max()) < 1e-12
    if kind == 'larger':
        assert bool((a[:, 0] == 0).all()) and bool((a[:, :, 0] == 0).all())                 # outside the map: exactly zero
    # the axis swap is what is being stated: the un-swapped reading differs
    sw = R.align_heatmap_gather(hm.transpose(1, 2), bbox, rect, None)
    assert float((R.align_heatmap_gather(hm, bbox, rect, None) - sw).abs().max()) > 1e-2


def test_nerf_embedding_equals_the_oracle():
    from oracle.nets import pos_embed_nerf
    g = torch.randn(9, 3, generator=R.gen(1), dtype=torch.float64)
    e = R.nerf_embed(g)
    assert e.shape == (9, 64) and bool((e[:, 63] == 0).all())
    assert float((e[:, :63] - pos_embed_nerf(g)).abs().max()) < 1e-12
    flip = torch.tensor([1, 0, 1, 0, 0, 0, 1, 1, 0], dtype=torch.uint8)
    gf = g.clone()
    gf[flip.bool(), 0] *= -1
    assert torch.equal(R.nerf_embed(g, flip)[:, :63], pos_embed_nerf(gf))


@pytest.mark.parametrize('step', [1, 2, 1000])
def test_adamw_reference_equals_the_oracle_and_the_formula(step):
    from oracle.train_score import adamw_step
    g = R.gen(step)
    p, gr = torch.randn(300, generator=g, dtype=torch.float64), torch.randn(300, generator=g, dtype=torch.float64) * 0.1
    m, v = torch.randn(300, generator=g, dtype=torch.float64) * 0.05, torch.rand(300, generator=g, dtype=torch.float64) * 0.01
    kw = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    got = R.adamw(p, gr, m, v, step, **kw)
    k32 = {k: R.f32r(x) for k, x in kw.items()}                   # the reference takes the hyper-parameters as the kernel receives them
    for a, b, c in zip(got, adamw_step(p, gr, m, v, step, **k32), R.adamw_formula(p, gr, m, v, step, **k32)):
        assert float((a - b).abs().max()) < 1e-13 and float((a - c).abs().max()) < 1e-13
    sc = R.adamw(p, gr, m, v, step, grad_scale=0.25, **kw)
    for a, b in zip(sc, adamw_step(p, gr * 0.25, m, v, step, **k32)):
        assert float((a - b).abs().max()) < 1e-13


def test_dsm_loss_reference_equals_the_oracle(sd):
    from oracle import nets as N
    from oracle.train_score import dsm_loss
    g = R.gen(5)
    bs, D = 3, 96
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items() if k.startswith('denoiser_hand.')}
    feat, gt = torch.randn(bs, 1024, generator=g, dtype=torch.float64) * 0.3, torch.randn(bs, D, generator=g, dtype=torch.float64) * 0.3
    t, z = torch.rand(bs, 1, generator=g, dtype=torch.float64) * 0.9 + 0.05, torch.randn(bs, D, generator=g, dtype=torch.float64)
    want = dsm_loss(sd64, 'denoiser_hand', feat, gt, t, z)
    xt, emb, std = R.dsm_prepare(gt, t.view(1, bs), z.view(1, bs, D), sd64['denoiser_hand.t_encoder.0.W'], D)
    assert float((xt - (gt + z * (N.SIGMA_MIN * (N.SIGMA_MAX / N.SIGMA_MIN) ** t))).abs().max()) < 1e-12
    score = N.denoiser(sd64, 'denoiser_hand', feat, xt, t)
    loss, seed = R.dsm_loss_from_score(score, z, std, bs)
    assert abs(float(loss) - float(want)) < 1e-10 * abs(float(want))
    # ... and the autograd form (through the un-normalised head output) gives the same loss and the kernel's seed gradient
    _, loss2, dout = R.dsm_loss(score * (std[:, None] + 1e-7), z, std, bs)
    assert abs(float(loss2) - float(want)) < 1e-10 * abs(float(want))
    assert float((dout - seed).abs().max()) < 1e-10 * float(seed.abs().max())


def test_prepare_and_head_references_rebuild_the_oracle_denoiser(sd):
    """dsm_prepare's Fourier features and padded x_t, then plinear2_fwd on the oracle's own hidden layer, give oracle.nets.denoiser's score"""
    from oracle import nets as N
    p = 'denoiser_obj'
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items() if k.startswith(p + '.')}
    g = R.gen(9)
    reps, bs, D, Dp = 2, 3, 9, 12
    feat, gt = torch.randn(bs, 1024, generator=g, dtype=torch.float64) * 0.3, torch.randn(bs, D, generator=g, dtype=torch.float64) * 0.3
    t, z = torch.rand(reps, bs, generator=g, dtype=torch.float64), torch.randn(reps, bs, D, generator=g, dtype=torch.float64)
    xt, emb, std = R.dsm_prepare(gt, t, z, sd64[p + '.t_encoder.0.W'], Dp)
    assert xt.shape == (reps * bs, Dp) and bool((xt[:, D:] == 0).all()) and emb.shape == (reps * bs, 128)
    want = N.denoiser(sd64, p, feat.repeat(reps, 1), xt[:, :D], t.reshape(-1, 1))
    tf = F.relu(F.linear(emb, sd64[p + '.t_encoder.1.weight'], sd64[p + '.t_encoder.1.bias']))
    pf = F.relu(N._lin(sd64, p + '.pose_encoder.2', F.relu(N._lin(sd64, p + '.pose_encoder.0', xt[:, :D]))))
    tot = torch.cat([tf, pf, feat.repeat(reps, 1)], -1)
    w1 = sd64[p + '.head.head.0.weight']
    nh = w1.shape[0]
    h = F.relu(torch.einsum('bc,ncd->bnd', tot, w1) + sd64[p + '.head.head.0.bias']).reshape(reps * bs, nh * 256)
    got = R.plinear2_fwd(h, sd64[p + '.head.head.2.weight'], sd64[p + '.head.head.2.bias'].reshape(nh, 3), std, nh)
    assert float((got - want).abs().max()) < 1e-10 * float(want.abs().max())


def test_force_local_reference_equals_the_oracle_head(sd):
    """the tail of oracle.nets.head_physics (physics.py:546-557, 700-712) written out"""
    g = R.gen(10)
    scale, logits = torch.randn(64, 1, generator=g, dtype=torch.float64), torch.randn(64, 8, generator=g, dtype=torch.float64) * 2
    anchor = sd['head_physics.anchor'].double()
    a = anchor.clone()
    a[:, :2] *= 0.8
    w = torch.softmax(torch.softmax(logits, -1), -1)
    d = w @ a
    want = d / (d.norm(dim=-1, keepdim=True) + 1e-8) * scale.abs()
    assert float((R.force_local(scale, logits, anchor, 64) - want).abs().max()) < 1e-14


@pytest.mark.parametrize('kh,kw,stride,py,px,cin,ld', [(3, 3, 1, 1, 1, 5, 5), (1, 1, 1, 0, 0, 33, 36), (3, 3, 2, 1, 1, 7, 8), (2, 2, 1, 1, 0, 6, 6),
                                                     (4, 4, 2, 1, 1, 3, 4)])
def test_im2col_reference_contracted_with_dy_is_the_conv_weight_gradient(kh, kw, stride, py, px, cin, ld):
    g = R.gen(kh * 100 + cin)
    N, H, W, cout = 2, 7, 6, 4
    x = torch.randn(N, H, W, ld, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, kh, kw, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x[..., :cin].permute(0, 3, 1, 2), w, None, stride, (py, px))
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    col = R.im2col_t(x, kh, kw, stride, py, px, cin=cin)
    P = N * y.shape[2] * y.shape[3]
    assert col.shape == (kh * kw * cin, (P + 3) // 4 * 4) and bool((col[:, P:] == 0).all())
    dw = dy.permute(1, 0, 2, 3).reshape(cout, P) @ col[:, :P].t()                                     # (cout, (r, s, ci))
    assert float((dw.view(cout, kh, kw, cin).permute(0, 3, 1, 2) - w.grad).abs().max()) < 1e-11


def test_force_local_reference_is_a_double_softmax_on_the_addressed_rows():
    g = R.gen(3)
    bs = 3
    scale, logits = torch.randn(bs * 65, 1, generator=g, dtype=torch.float64), torch.randn(bs * 65, 8, generator=g, dtype=torch.float64) * 3
    anchor = torch.randn(8, 3, generator=g, dtype=torch.float64)
    got = R.force_local(scale, logits, anchor, bs * 32, 32, 65, 0, 32)
    pick = lambda t, off: t.view(bs, 65, -1)[:, off:off + 32].reshape(bs * 32, -1)
    want = R.force_local(pick(scale, 0), pick(logits, 32), anchor, bs * 32)
    assert torch.equal(got, want)
    assert float((got.norm(dim=-1) - pick(scale, 0).abs()[:, 0]).abs().max()) < 1e-7                  # unit direction x |scale|
    single = R.force_local(pick(scale, 0), pick(logits, 32), anchor, bs * 32, double_softmax=False)
    assert float((got - single).abs().max()) > 1e-2


def test_layernorm_backward_reference_is_consistent():
    g = R.gen(4)
    x, r = torch.randn(5, 100, generator=g, dtype=torch.float64), torch.randn(5, 100, generator=g, dtype=torch.float64)
    gamma, dy = torch.randn(100, generator=g, dtype=torch.float64), torch.randn(5, 100, generator=g, dtype=torch.float64)
    dx, gx, dg, db = R.layernorm_bwd(x, r, gamma, dy)
    assert float((gx.sum(0) - dg).abs().max()) < 1e-12 and float((dy.sum(0) - db).abs().max()) < 1e-12
    eps = 1e-6
    d = torch.randn(5, 100, generator=g, dtype=torch.float64)
    beta = torch.zeros(100, dtype=torch.float64)
    num = ((R.add_layernorm(x + eps * d, r, gamma, beta) - R.add_layernorm(x - eps * d, r, gamma, beta)) * dy).sum() / (2 * eps)
    assert abs(float(num) - float((dx * d).sum())) < 1e-6 * max(1.0, abs(float(num)))


def test_cross_tokens_backward_reference_is_the_adjoint():
    g = R.gen(6)
    bs = 3
    ph, po = torch.randn(bs, 8, 8, 256, generator=g, dtype=torch.float64), torch.randn(bs, 8, 8, 256, generator=g, dtype=torch.float64)
    ge, pe = torch.randn(bs, 512, generator=g, dtype=torch.float64), torch.randn(7, 512, generator=g, dtype=torch.float64)
    tok = R.cross_tokens(ph, po, ge, pe)
    assert tok.shape == (bs, 65, 512)
    assert float(tok[1, 3, 70] - (ph[1, 70 % 64 // 8, 70 % 8, 8 * 3 + 1] + pe[1, 70])) == 0.0         # token 3, feature 70 = channel 25, pixel 6
    assert float(tok[2, 64, 9] - (ge[2, 9] + pe[2, 9])) == 0.0
    d = torch.randn(bs, 65, 512, generator=g, dtype=torch.float64)
    dph, dpo, dge = R.cross_tokens_bwd(d)
    lhs = (R.cross_tokens(ph, po, ge, torch.zeros_like(pe)) * d).sum()
    assert abs(float(lhs - ((ph * dph).sum() + (po * dpo).sum() + (ge * dge).sum()))) < 1e-9


def test_single_rounding_through_float64_is_the_float32_operation():
    g = R.gen(8)
    a, b = torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-3
    assert R.bits_equal(R.single_rounding(lambda x, y: x + y, [a, b]), a + b)
    assert R.bits_equal(R.single_rounding(lambda x, y: x * y, [a, b]), a * b)
    for slope in (0.0, 0.01, 1.0):
        assert R.bits_equal(R.add_lrelu_f32(a, b, slope), F.leaky_relu(a + b, slope) if slope else torch.where(a + b > 0, a + b, (a + b) * 0.0))
        assert R.bits_equal(R.lrelu_bwd_f32(a, b, slope), torch.where(b > 0, a, a * torch.tensor(slope, dtype=torch.float32)))


def test_bound_rule():
    ref = torch.tensor([1.0, -8.0], dtype=torch.float64)
    assert R.bound(ref.float(), ref) == 4 * 2.0 ** -23 * 8.0                                          # the floor: 4 ulp of the largest output
    assert R.bound(ref.float() + 1e-3, ref) == pytest.approx(4e-3, rel=1e-3)


def test_physics_losses_reproduce_the_committed_training_golden(assets):
    """tests/golden/golden_physics_train.npz holds the reference's force_local, force_global, force_point, CoM and its five weighted losses
    for the inputs of tests/_physics_train_inputs.py: the loss half of the physics reference reproduces them"""
    from tests._physics_train_inputs import inputs, W, BS
    G = np.load(os.path.join(GOLD, 'golden_physics_train.npz'))
    d = inputs(assets)
    t64 = lambda a: torch.as_tensor(np.asarray(a)).double()
    L = R.five_losses(t64(G['force_local']).view(BS * 32, 3), t64(G['force_global']), t64(G['CoM']).view(BS * 32, 3), t64(G['force_point']),
                      d['gt_force_local'].double(), d['gravity'].double().view(BS, 3), d['gt_CoM'].double().view(BS, 3), d['is_grasped'], tuple(W.values()))
    for k, v in zip(W, L):
        np.testing.assert_allclose(float(v), float(G[k]), rtol=2e-5, err_msg=k)
    assert bool(d['is_grasped'].any()) and not bool(d['is_grasped'].all())


"""Training-path leaf kernels (csrc/train_score.hip, csrc/train_physics.hip) one by one against the float64 references of
tests/_leaf_fp64.py -- autograd for every backward, torch.optim.AdamW for the optimiser -- on the float32 inputs the kernel saw.

Bit-exact group: data movement, masks, single roundings, the multi-tensor AdamW against the single-tensor one.  Arithmetic group: R.bound
(4 x torch's own float32 CPU error against float64, floor 4 ulp of the largest output), or a bound derived in the docstring."""
import math

import pytest
import torch

from tests import _leaf_fp64 as R

pytestmark = pytest.mark.gpu
SENT = R.SENT
U24 = 2.0 ** -24                                                  # unit roundoff of float32


def _ops():
    from vpho_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ bit-exact group
def test_relu_bwd_on_the_slices_the_training_step_passes():
    """element offsets / leading dimensions of vpho_amd/train_score.py: columns 0..127 and 128..383 of the 1408-wide concatenation, and a
    contiguous 256-wide layer; rows not a multiple of the block"""
    ops = _ops()
    g = R.gen(1)
    M = 37
    dy, y = torch.randn(M, 1408, generator=g), torch.relu(torch.randn(M, 1408, generator=g))
    for off, cols in ((0, 128), (128, 256), (384, 1024), (5, 3)):
        got = ops.relu_bwd(dy.cuda(), off, 1408, y.cuda(), off, 1408, M, cols)
        assert R.bits_equal(got, R.relu_bwd(dy[:, off:off + cols], y[:, off:off + cols]).contiguous())
    d2, y2 = torch.randn(M, 256, generator=g), torch.relu(torch.randn(M, 256, generator=g))
    assert R.bits_equal(ops.relu_bwd(d2.cuda(), 0, 256, y2.cuda(), 0, 256, M, 256), R.relu_bwd(d2, y2))
    assert float((y == 0).float().mean()) > 0.3                       # exact zeros are in the mask


@pytest.mark.parametrize('bs,reps,ld,c_off,cols', [(5, 2, 1408, 384, 1024), (7, 3, 20, 3, 9), (64, 20, 16, 0, 16), (1, 1, 8, 7, 1)])
def test_sum_repeats_is_the_left_to_right_float32_sum(bs, reps, ld, c_off, cols):
    ops = _ops()
    x = torch.randn(reps * bs, ld, generator=R.gen(bs + reps))
    assert R.bits_equal(ops.sum_repeats(x.cuda(), c_off, bs, reps, cols), R.sum_repeats_f32(x, c_off, bs, reps, cols))


@pytest.mark.parametrize('rows,cols', [(1, 1), (3, 5), (33, 31), (70, 100), (64, 64), (1280, 96), (5, 1408)])
def test_transpose_with_zero_padded_columns(rows, cols):
    ops = _ops()
    x = torch.randn(rows, cols, generator=R.gen(rows + cols))
    got = ops.transpose(x.cuda())
    assert R.bits_equal(got, R.transpose(x)) and bool((got[:, rows:] == 0).all())
    assert R.bits_equal(ops.transpose(x.cuda(), pad_to=32), R.transpose(x, 32))


IM2COL = [  # N, H, W, ld, cin, kh, kw, stride, pad_y, pad_x
    (2, 7, 6, 5, 5, 3, 3, 1, 1, 1), (1, 5, 5, 36, 33, 1, 1, 1, 0, 0), (2, 9, 11, 8, 7, 3, 3, 2, 1, 1), (1, 6, 7, 6, 6, 2, 2, 1, 1, 0),
    (3, 8, 8, 64, 64, 3, 3, 1, 1, 1), (1, 7, 9, 4, 3, 4, 4, 2, 1, 1), (1, 3, 3, 40, 40, 3, 3, 1, 0, 1)]


@pytest.mark.parametrize('N,H,W,ld,cin,kh,kw,stride,py,px', IM2COL)
def test_im2col_t_against_unfold(N, H, W, ld, cin, kh, kw, stride, py, px):
    ops = _ops()
    x = torch.randn(N, H, W, ld, generator=R.gen(H * W + cin))
    ref = R.im2col_t(x, kh, kw, stride, py, px, cin=cin)
    OH, OW = (H + 2 * py - kh) // stride + 1, (W + 2 * px - kw) // stride + 1
    P = N * OH * OW
    got = ops.im2col_t(x.cuda(), kh, kw, stride, py, px, OH, OW, cin=cin)
    assert R.bits_equal(got, ref) and bool((got[:, P:] == 0).all())


def _signed_zero_mix(n, g):
    y = torch.randn(n, generator=g)
    y[::7] = 0.0
    y[3::11] = -0.0
    return y


@pytest.mark.parametrize('n', [1, 3, 4, 1023, 1024, 1025, 4 * 777])
@pytest.mark.parametrize('slope', [0.0, 0.01, 1.0])
def test_lrelu_bwd_and_add_lrelu_bit_exact_on_both_paths(n, slope):
    """16-byte path (n % 4 == 0, aligned bases) and scalar path (n % 4 != 0, or a base one element off); y exactly 0 and -0.0 take the
    negative branch; slope 0 gives signed zeros -- all compared bit for bit"""
    ops = _ops()
    g = R.gen(n)
    dy, y, a = torch.randn(n, generator=g), _signed_zero_mix(n, g), torch.randn(n, generator=g)
    b = -a.clone()
    b[1::2] = torch.randn(n, generator=g)[1::2]                       # a + b exactly 0 in every other element
    want_bwd, want_add = R.lrelu_bwd_f32(dy, y, slope), R.add_lrelu_f32(a, b, slope)
    assert R.bits_equal(ops.lrelu_bwd(dy.cuda(), y.cuda(), slope), want_bwd)
    assert R.bits_equal(ops.add_lrelu(a.cuda(), b.cuda(), slope), want_add)
    for which in range(2):                                            # one operand on a base that is not 16-byte aligned
        ops_in = [dy.cuda(), y.cuda()]
        ops_in[which] = R.offset_view(ops_in[which].cpu())
        assert R.bits_equal(ops.lrelu_bwd(ops_in[0], ops_in[1], slope), want_bwd)
        ab = [a.cuda(), b.cuda()]
        ab[which] = R.offset_view(ab[which].cpu())
        assert R.bits_equal(ops.add_lrelu(ab[0], ab[1], slope), want_add)
    assert R.bits_equal(ops.lrelu_bwd(dy.view(1, n, 1).cuda(), y.view(1, n, 1).cuda(), slope).view(-1), want_bwd)


def _adam_tensors(n, g, dev='cuda'):
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    m, v = torch.randn(n, generator=g) * 0.05, torch.rand(n, generator=g) * 0.01
    return [t.to(dev) for t in (p, gr, m, v)]


@pytest.mark.parametrize('sizes', [[1, 1023, 1024, 1025, 5000], [1024, 1024, 1], [5000], [(i * 37) % 90 + 1 for i in range(400)]])
def test_adamw_list_is_bit_identical_to_single_tensor_steps(sizes):
    """tensors carved out of ONE flat buffer with sentinel gaps between them (the gaps must stay untouched: a block that bisects to the
    wrong segment, or runs past its segment's end, lands in one), every parameter's version counter increases"""
    ops = _ops()
    g = R.gen(len(sizes))
    gap = 5
    flat = {k: torch.full((sum(sizes) + gap * (len(sizes) + 1),), SENT, device='cuda') for k in 'pgmv'}
    quads, singles, mask, pos = [], [], torch.ones_like(flat['p'], dtype=torch.bool), gap
    for n in sizes:
        src = _adam_tensors(n, g)
        quad = []
        for k, s in zip('pgmv', src):
            view = flat[k][pos:pos + n]
            view.copy_(s)
            quad.append(view)
        mask[pos:pos + n] = False
        quads.append(tuple(quad))
        singles.append([s.clone() for s in src])
        pos += n + gap
    lst = ops.AdamWList(quads)
    before = [q[0]._version for q in quads]
    kw = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.02, grad_scale=0.5)
    for step in (1, 2, 7):
        lst.step(step, **kw)
        for s in singles:
            ops.adamw_(s[0], s[1], s[2], s[3], step, **kw)
    torch.cuda.synchronize()
    for q, s in zip(quads, singles):
        for a, b in zip(q, s):
            assert R.bits_equal(a, b)
    for k in 'pgmv':
        assert bool((flat[k][mask] == SENT).all()), k
    assert all(q[0]._version > b for q, b in zip(quads, before))


# ------------------------------------------------------------------------------------------------ arithmetic group
@pytest.mark.parametrize('bs,reps', [(1, 1), (5, 2), (7, 3), (64, 20)])
@pytest.mark.parametrize('D,Dp', [(96, 96), (9, 12)])
def test_dsm_prepare(bs, reps, D, Dp):
    """std and x_t: the rule.  Fourier features: the kernel's phase a = ((t W) 2) fl(pi) carries the rounding of t W and of the last
    product (2^-24 each, relative) and fl(pi) / pi - 1 = 2.8e-8, so |d sin| <= |a| (2 * 2^-24 + 2.8e-8) + 2 ulp(1) for the device function"""
    ops = _ops()
    g = R.gen(bs * 100 + D)
    gt, z = torch.randn(bs, D, generator=g), torch.randn(reps, bs, D, generator=g)
    t = torch.rand(reps, bs, generator=g) * (1 - 1e-5) + 1e-5
    t.view(-1)[0], t.view(-1)[-1] = 1e-5, 1.0                         # both ends of the time range
    Wf = torch.randn(64, generator=g) * 30
    (rx, re, rs), (tx, _, ts) = R.ruled(R.dsm_prepare, [gt, t, z, Wf], Dp)
    xt, emb, sd = ops.dsm_prepare(gt.cuda(), t.cuda(), z.cuda(), Wf.cuda(), Dp)
    R.check(f'dsm_prepare std bs{bs} reps{reps}', sd, rs, ts)
    R.check(f'dsm_prepare x_t bs{bs} reps{reps} D{D}', xt, rx, tx)
    assert bool((xt[:, D:] == 0).all())
    amax = float((t.double().reshape(-1, 1) * Wf.double()[None] * 2 * math.pi).abs().max())
    R.check(f'dsm_prepare fourier bs{bs} reps{reps}', emb, re, amax * (2 * 2.0 ** -24 + 2.8e-8) + 2 * 2.0 ** -23)


@pytest.mark.parametrize('nheads', [32, 3])
@pytest.mark.parametrize('rows', [1, 3, 5, 1280])
def test_plinear2_forward_and_backward(nheads, rows):
    ops = _ops()
    g = R.gen(nheads * 10000 + rows)
    pre = torch.randn(rows, nheads * 256, generator=g)
    pre[:, ::5] = 0.0                                                 # exact zeros in h: the mask is h > 0, not h >= 0
    h = torch.relu(pre)
    w2, b2 = torch.randn(nheads, 256, 3, generator=g) * 0.1, torch.randn(nheads, 3, generator=g) * 0.1
    std = torch.rand(rows, generator=g) * 5 + 0.02
    std[0] = 0.01                                                     # the smallest std of the schedule: the division amplifies most
    ref, tol = R.ruled(R.plinear2_fwd, [h, w2, b2, std], nheads)
    R.check(f'plinear2_fwd n{nheads} rows{rows}', ops.plinear2_fwd(h.cuda(), w2.cuda(), b2.cuda(), std.cuda(), nheads), ref, tol)
    dout = torch.randn(rows, 3 * nheads, generator=g)
    (rp, rw, rb), (tp, tw, tb) = R.ruled(R.plinear2_bwd, [pre, dout, w2], nheads)
    dpre, dw2, db2 = ops.plinear2_bwd(h.cuda(), dout.cuda(), w2.cuda(), nheads)
    R.check(f'plinear2_bwd dpre n{nheads} rows{rows}', dpre, rp, tp)
    R.check(f'plinear2_bwd dw2 n{nheads} rows{rows}', dw2, rw, tw)
    R.check(f'plinear2_bwd db2 n{nheads} rows{rows}', db2, rb, tb)
    assert bool((dpre[:, ::5] == 0).all())
    again = ops.plinear2_bwd(h.cuda(), dout.cuda(), w2.cuda(), nheads)
    assert R.bits_equal(again[1], dw2) and R.bits_equal(again[2], db2)            # fixed summation order: two runs, the same bits


@pytest.mark.parametrize('rows,D', [(2, 96), (27, 9), (4096, 64), (2731, 96), (2800, 97), (120, 9)])
def test_dsm_loss(rows, D):
    """element counts below 256, exactly 262 144 (1024 blocks x 256, the grid cap) and above it (the grid-stride path).

    Loss, derived (u = 2^-24, first order): each term w d^2 is float32 arithmetic -- w = fl(sd^2) [u], target = fl(fl(-z sd) / w) [3u of
    |z / sd|], d = fl(score - target) [u |d| + 3u |z / sd|: the subtraction cancels, so the target's error does not scale with d], then
    fl(w fl(d d)) [2u] -- and the terms, all >= 0, are accumulated in float64 (n 2^-53, relative).  Hence
        |loss - ref| <= sum_i (5u w d^2 + 6u w |d| |z / sd|) / count + (n + 2) 2^-53 ref
    evaluated below in float64 on the same inputs (times 1 + 8u for the second-order terms).  The assertion takes the smaller of this and the rule.  Seed gradient: the rule."""
    ops = _ops()
    g = R.gen(rows + D)
    z, std = torch.randn(rows, D, generator=g), torch.rand(rows, generator=g) * 5 + 0.01
    score = -z / std[:, None] + torch.randn(rows, D, generator=g) * 0.3
    btr = max(rows // 2, 1)
    (rl, rd), (tl, td) = R.ruled(R.dsm_loss_from_score, [score, z, std], btr)
    loss, dout = ops.dsm_loss(score.cuda(), z.cuda(), std.cuda(), btr)
    assert loss.dtype == torch.float64
    sd64, z64 = std.double()[:, None], z.double()
    d64 = score.double() + z64 / sd64
    derived = U24 * (1 + 8 * U24) * float((5 * sd64 ** 2 * d64 ** 2 + 6 * sd64 ** 2 * d64.abs() * (z64 / sd64).abs()).sum()) / btr + (rows * D + 2) * 2.0 ** -53 * float(rl)
    print(f'LEAF dsm_loss loss {rows}x{D}: rule {tl:.3e} derived {derived:.3e}')
    R.check(f'dsm_loss loss {rows}x{D}', loss, rl, min(tl, derived))
    R.check(f'dsm_loss dout {rows}x{D}', dout, rd, td)
    # the autograd form through the un-normalised head output gives the same seed
    _, l2, d2 = R.dsm_loss(score.double() * (std.double()[:, None] + 1e-7), z.double(), std.double(), btr)
    assert abs(float(l2 - rl)) <= 1e-9 * abs(float(rl)) and float((d2 - rd).abs().max()) <= 1e-9 * float(rd.abs().max())


@pytest.mark.parametrize('shape', [(5,), (3, 85), (512, 512), (512, 513), (700, 999)])
@pytest.mark.parametrize('weight', [1.0, 10.0])
def test_mse_loss(shape, weight):
    """5, 255, exactly 262 144 and more elements (grid-stride above 1024 blocks of 256).

    Loss, derived (u = 2^-24, first order): each term fl(fl(pd - gt)^2) carries 3u relative (u of the difference, twice in the square, u of
    the product), the terms are all >= 0 and are accumulated and scaled by weight / n in float64 (n 2^-53 relative), so
        |loss - ref| <= ((1 + u)^3 - 1 + (n + 2) 2^-53) ref
    which is below the rule's floor of 4 ulp = 8u: the assertion takes the smaller of the two.  Gradient (two roundings): the rule."""
    ops = _ops()
    g = R.gen(sum(shape))
    pd, gt = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    (rl, rg), (tl, tg) = R.ruled(R.mse_loss, [pd, gt], weight)
    loss, grad = ops.mse_loss(pd.cuda(), gt.cuda(), weight)
    assert loss.dtype == torch.float64
    derived = ((1 + U24) ** 3 - 1 + (pd.numel() + 2) * 2.0 ** -53) * float(rl)
    print(f'LEAF mse_loss loss {shape} w{weight}: rule {tl:.3e} derived {derived:.3e}')
    R.check(f'mse_loss loss {shape} w{weight}', loss, rl, min(tl, derived))
    R.check(f'mse_loss grad {shape} w{weight}', grad, rg, tg)


@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('grad_scale', [1.0, 0.125, 1.0 / 3.0])
def test_adamw_against_float64_torch_optim(step, grad_scale):
    """one update at step k resumed from saved moments, against torch.optim.AdamW on float64 copies; n covers a partial last block"""
    ops = _ops()
    g = R.gen(step)
    n = 3000
    p, gr, m, v = _adam_tensors(n, g, 'cpu')
    gr[::4] = 0.0                                                     # zero gradients
    m[::8], v[::8] = 0.0, 0.0                                         # ... also with empty moments: 0 / (0 + eps)
    kw = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=grad_scale)
    ref, tol = R.ruled(R.adamw, [p, gr, m, v], step, **kw)
    dp, dg, dm, dv = p.cuda(), gr.cuda(), m.cuda(), v.cuda()
    ops.adamw_(dp, dg, dm, dv, step, **kw)
    for name, got, r, t in zip(('param', 'exp_avg', 'exp_avg_sq'), (dp, dm, dv), ref, tol):
        R.check(f'adamw {name} step{step} gs{grad_scale:.3f}', got, r, t)
    assert R.bits_equal(dg, gr)


@pytest.mark.parametrize('rows', [1, 3, 4, 5, 65 * 64])
@pytest.mark.parametrize('E', [512, 64, 100])
def test_layernorm_backward(rows, E):
    """dx against autograd; dy * xhat; and its column sums / those of dy (vpho_colsum_f32, as the training step takes them) against
    autograd's d gamma / d beta"""
    ops = _ops()
    g = R.gen(rows * 3 + E)
    gamma = 1 + 0.2 * torch.randn(E, generator=g)
    for tag, x, r in (('', torch.randn(rows, E, generator=g), torch.randn(rows, E, generator=g)),
                      (' mean>>spread', 100 + 0.01 * torch.randn(rows, E, generator=g), 0.001 * torch.randn(rows, E, generator=g))):
        dy = torch.randn(rows, E, generator=g)
        (rdx, rgx, rdg, rdb), (tdx, tgx, tdg, tdb) = R.ruled(R.layernorm_bwd, [x, r, gamma, dy])
        dx, gx = ops.layernorm_bwd(x.cuda(), r.cuda(), gamma.cuda(), dy.cuda())
        R.check(f'layernorm_bwd dx {rows}x{E}{tag}', dx, rdx, tdx)
        R.check(f'layernorm_bwd gxhat {rows}x{E}{tag}', gx, rgx, tgx)
        R.check(f'layernorm_bwd dgamma {rows}x{E}{tag}', ops.colsum(gx), rdg, tdg)
        R.check(f'layernorm_bwd dbeta {rows}x{E}{tag}', ops.colsum(dy.cuda()), rdb, tdb)


def _physics_inputs(bs, g, grasp):
    rn = lambda *s: torch.randn(*s, generator=g)
    scale, logits, com = rn(bs * 32, 1), rn(bs * 32, 8) * 2, rn(bs * 32, 3) * 0.05 + torch.tensor([0.05, 0.0, 0.7])
    scale[::5] = 0.0                                                  # d|s|/ds at exactly 0 is 0
    scale[1::5] = -scale[1::5].abs()
    anchor = rn(8, 3)
    q, _ = torch.linalg.qr(rn(bs, 32, 3, 3))                          # orthonormal frames
    point = rn(bs, 32, 3) * 0.03 + torch.tensor([0.02, -0.01, 0.7])
    gt_local, gt_com = rn(bs, 32, 3) * 0.1, rn(bs, 3) * 0.02 + torch.tensor([0.05, 0.0, 0.7])
    grav = rn(bs, 3)
    grav = grav / grav.norm(dim=-1, keepdim=True)
    gr = {'all': torch.ones(bs), 'none': torch.zeros(bs), 'mixed': (torch.arange(bs) % 3 != 1).float()}[grasp].to(torch.uint8)
    return [scale, logits, com, anchor, q.contiguous(), point, gt_local, grav, gt_com, gr]


@pytest.mark.parametrize('bs', [1, 5, 64, 130])
@pytest.mark.parametrize('grasp', ['all', 'none', 'mixed'])
def test_physics_loss(bs, grasp):
    """the five weighted losses, force_local and the three gradients (autograd of the losses' sum in float64); two runs, the same bits.

    The losses keep the rule.  Only the last square and the sum over the images are float64 in the kernel: what is squared (F + g,
    F . g + 1, the torque, the 96-term sums of e^2) comes out of a float32 chain of two soft-maxes (device expf), a normalisation and
    32-anchor float32 sums, with cancellation in F + g, so no short derivation gives less than the rule.  The simplest of the five, the
    CoM loss, shows it: 3u per term (as in test_mse_loss) + 2u for the three-component sum + 5u for the 32-lane tree = 10u relative
    (u = 2^-24), already above the rule's floor of 4 ulp = 8u."""
    ops = _ops()
    args = _physics_inputs(bs, R.gen(bs), grasp)
    W = (1.0, 1.0, 30.0, 10.0, 100.0)
    ref, tol = R.ruled(R.physics_loss, args, W)
    dev = [a.cuda() for a in args]
    out = ops.physics_loss(*dev, W)
    names = ('force_local', 'losses', 'd_scale', 'd_logits', 'd_com')
    for name, got, r, t in zip(names, out, ref, tol):
        assert name != 'losses' or got.dtype == torch.float64
        R.check(f'physics_loss {name} bs{bs} {grasp}', got, r, t)
    if grasp == 'none':
        assert float(out[1][0]) == 0.0 and float(out[1][1]) == 0.0 and float(out[1][2]) == 0.0
    assert bool((out[2].view(-1)[::5] == 0).all())
    again = ops.physics_loss(*dev, W)
    for a, b in zip(out, again):
        assert bool(torch.equal(a, b))
    fl2 = ops.force_local(dev[0], dev[1], dev[3], bs * 32)            # the inference kernel computes the same forces
    R.check(f'physics_loss force_local vs force_local kernel bs{bs}', fl2, ref[0], tol[0])

"""Train-mode BatchNorm statistics against a float64 reference, at statistics where the reduction order matters: channels whose mean
is up to 1000 times their standard deviation (either sign), standard deviations from 1e-3 to 1e2, exactly constant channels, and the
no-bias ResNet case (post-ReLU input times weights with a common positive offset).  var = E[v^2] - mean^2 cancels there, and the
error of every partial sum is multiplied by (mean^2 + var) / var.

The reference is float64 applied to the fp32 tensor the convolution STORED, so the convolution's own rounding drops out.  Every
producer of partial rows (the direct kernel's three tile classes, the persistent kernel, both Winograd forms, the four-phase
transposed convolution, the two-level finish) and the backward epilogues must be as accurate as the stand-alone reduction on the
same tensor: error against float64 at most 2x the stand-alone path's, plus 2e-6."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, MOM, SLOPE = 1e-5, 0.1, 0.01
RATIOS = (0., 1., -1., 30., -30., 100., -100., 1000., -1000.)
CONSTS = (0., 1.7, -3.3, 42.1, -99.3)          # constant channels (zero weight row): y = bias


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _channel_stats(C):
    """per channel: (target std, target mean, constant?) -- every ratio meets stds across 1e-3 .. 1e2"""
    std = torch.tensor([10.0 ** (-3 + 5 * ((7 * c) % C) / max(C - 1, 1)) for c in range(C)], dtype=torch.float64)
    mean = torch.tensor([RATIOS[c % len(RATIOS)] for c in range(C)], dtype=torch.float64) * std
    const = torch.tensor([c % 11 == 5 for c in range(C)])
    mean[const] = torch.tensor([CONSTS[(c // 11) % len(CONSTS)] for c in range(C) if c % 11 == 5], dtype=torch.float64)
    return std, mean, const


def _adversarial(N, H, W, cin, cout, k, seed):
    """x ~ N(0, 1); unit-norm weight rows scaled by the channel's std and bias = its mean: y_c ~ N(mean_c, std_c) (a little less spread
    at the padded border); zero rows for the constant channels"""
    x = torch.randn((N, H, W, cin), generator=_gen(seed))
    std, mean, const = _channel_stats(cout)
    w = torch.randn((cout, k * k * cin), generator=_gen(seed + 1), dtype=torch.float64)
    w = w / w.norm(dim=1, keepdim=True) * std[:, None]
    w[const] = 0.
    return x.cuda(), w.float().cuda(), mean.float().cuda()


def _resnet(N, H, W, cin, cout, k, seed):
    """no bias: non-negative post-ReLU input times weights with a common positive offset per output channel"""
    x = torch.randn((N, H, W, cin), generator=_gen(seed)).clamp_min(0.)
    off = 0.02 * (1 + torch.arange(cout) % 5).float()
    w = off[:, None] * (1 + 0.05 * torch.randn((cout, k * k * cin), generator=_gen(seed + 1)))
    return x.cuda(), w.cuda(), None


def _affine(C, seed):
    g = _gen(seed)
    return (torch.rand(C, generator=g) + 0.5).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()


def _ref_forward(y, gamma, beta):
    """float64 BatchNorm forward of the stored tensor: mean, invstd, running mean / var (from 0 / 1), activated output"""
    C = y.shape[-1]
    y2 = y.reshape(-1, C).double()
    n = y2.shape[0]
    mean = y2.mean(0)
    var = ((y2 - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    a = (y2 - mean) * invstd * gamma.double() + beta.double()
    return dict(mean=mean, var=var, invstd=invstd, rm=MOM * mean, rv=(1 - MOM) + MOM * var * n / (n - 1), a=torch.where(a > 0, a, a * SLOPE))


def _errors(ref, a, m, i, rm, rv):
    """the errors against float64: mean / running mean relative to |mean| + std, invstd / running var relative, output relative to 1 + |a|"""
    scale = ref['mean'].abs() + ref['var'].sqrt() + 1e-30
    C = ref['mean'].shape[0]
    return dict(mean=float(((m.double() - ref['mean']).abs() / scale).max()),
                running_mean=float(((rm.double() - ref['rm']).abs() / scale).max()),
                invstd=float(((i.double() - ref['invstd']).abs() / ref['invstd']).max()),
                running_var=float(((rv.double() - ref['rv']).abs() / ref['rv']).max()),
                out=float(((a.reshape(-1, C).double() - ref['a']).abs() / (1 + ref['a'].abs())).max()))


def _check_as_accurate(y, f, gamma, beta, what):
    """the fused statistics (f's partial rows) against float64, with the stand-alone reduction of the same tensor as the yardstick"""
    from vpho_amd import ops
    C = y.shape[-1]
    assert f.live(), f'{what}: the fused epilogue serves this shape'
    ref = _ref_forward(y, gamma, beta)
    errs = []
    for partials in (f, None):
        rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
        a, (m, i) = ops.bn_train_forward(y, gamma, beta, rm, rv, eps=EPS, momentum=MOM, slope=SLOPE, partials=partials)
        errs.append(_errors(ref, a, m, i, rm, rv))
        # exactly constant channels: var = 0, invstd = 1 / sqrt(eps)
        const = ref['var'] == 0
        if bool(const.any()):
            want = 1.0 / math.sqrt(EPS)
            got = i.double()[const]
            assert float(((got - want).abs() / want).max()) <= 1e-5, (what, 'fused' if partials else 'stand-alone', got.tolist())
    fused, alone = errs
    bad = {k: (fused[k], alone[k]) for k in fused if not fused[k] <= 2 * alone[k] + 2e-6}
    assert not bad, f'{what}: fused error vs float64 above 2x stand-alone + 2e-6 (fused, stand-alone): {bad}'


def _merged(part):
    """float64 merge of the centred planes of the partial rows [rows][6][C] (2 .. 5: pivot p | sum (v - p) | sum (v - p)^2 | count)
    -> (count, mean, M2) per channel"""
    p, s, q, n = (part[:, i].double() for i in range(2, 6))
    N = n.sum(0)
    tm = p + s / n
    mean = (n * tm).sum(0) / N
    return N, mean, (q - s * s / n).sum(0) + (n * (tm - mean) ** 2).sum(0)


def _rows_match_tiles(part, y2, bm):
    """row t of the partial matrix = the sums of output rows [t*bm, (t+1)*bm), plain and about their first value, recomputed in float64"""
    M, C = y2.shape
    T = (M + bm - 1) // bm
    assert part.shape[0] == T
    p = part.double()
    for t in range(T):
        blk = y2[t * bm:(t + 1) * bm]
        assert float(((p[t, 0] - blk.sum(0)).abs() / (blk.abs().sum(0) + 1e-30)).max()) < 1e-5, t
        assert float(((p[t, 1] - (blk * blk).sum(0)).abs() / ((blk * blk).sum(0) + 1e-30)).max()) < 1e-5, t
        assert torch.equal(p[t, 2], blk[0]), t                              # the pivot: the tile's first row
        dv = blk - blk[0]
        assert torch.equal(p[t, 5], torch.full_like(p[t, 5], blk.shape[0])), t
        assert float(((p[t, 3] - dv.sum(0)).abs() / (dv.abs().sum(0) + 1e-30)).max()) < 1e-5, t
        assert float(((p[t, 4] - (dv * dv).sum(0)).abs() / ((dv * dv).sum(0) + 1e-30)).max()) < 1e-5, t


# (N, H, W, cin, cout, k, bm): the direct kernel's 128x128 / 128x64 / 64x64 tile classes (VPHO_CONV_PERS=0), ragged M and channel tails
# (pinned without a device by tests/_conv_plan_cases.py: a_bn_stats_direct_*, and a_bn_stats_persistent_* for the test after this one)
DIRECT = [(61, 33, 33, 64, 256, 1, 128), (64, 16, 16, 128, 128, 3, 128), (63, 16, 17, 128, 128, 3, 128), (16, 16, 16, 256, 64, 1, 64),
          (2, 9, 7, 32, 40, 1, 64), (3, 8, 8, 36, 132, 1, 64), (2, 10, 6, 16, 64, 3, 64), (3, 12, 12, 64, 128, 3, 64)]


@pytest.mark.parametrize('kind', ['adversarial', 'resnet'])
@pytest.mark.parametrize('N,H,W,cin,cout,k,bm', DIRECT)
def test_direct_kernel_statistics_against_float64(monkeypatch, N, H, W, cin, cout, k, bm, kind):
    from vpho_amd import ops
    monkeypatch.setenv('VPHO_CONV_PERS', '0')
    x, w, b = (_adversarial if kind == 'adversarial' else _resnet)(N, H, W, cin, cout, k, 100 + N + k)
    f = ops.BnFuse()
    y = ops.conv2d_nhwc(x, w, b, kh=k, kw=k, pad=k // 2, bn=f)
    assert f.rows == (N * H * W + bm - 1) // bm, 'the tile class the shape was chosen for'
    assert torch.equal(y, ops.conv2d_nhwc(x, w, b, kh=k, kw=k, pad=k // 2))      # the epilogue does not touch the stored values
    f2 = ops.BnFuse()
    ops.conv2d_nhwc(x, w, b, kh=k, kw=k, pad=k // 2, bn=f2)
    assert f2.rows == f.rows and torch.equal(f2.stats[:f.rows], f.stats[:f.rows])  # bit-reproducible
    _check_as_accurate(y, f, *_affine(cout, 7), f'direct {bm} {kind}')
    _rows_match_tiles(f.stats[:f.rows], y.reshape(-1, cout).double(), bm)


@pytest.mark.parametrize('N,H,W', [(64, 32, 32), (61, 33, 33)])
def test_persistent_kernel_statistics_against_float64(monkeypatch, N, H, W):
    from vpho_amd import ops
    cin, cout = 64, 256
    x, w, b = _adversarial(N, H, W, cin, cout, 1, 200 + N)
    monkeypatch.setenv('VPHO_CONV_PERS', '0')
    want = ops.conv2d_nhwc(x, w, b)
    monkeypatch.setenv('VPHO_CONV_PERS', '2')
    f = ops.BnFuse()
    y = ops.conv2d_nhwc(x, w, b, bn=f)
    assert f.rows == (N * H * W + 127) // 128 and torch.equal(y, want)
    f2 = ops.BnFuse()
    ops.conv2d_nhwc(x, w, b, bn=f2)
    assert torch.equal(f2.stats[:f.rows], f.stats[:f.rows])
    _check_as_accurate(y, f, *_affine(cout, 8), 'persistent')
    _rows_match_tiles(f.stats[:f.rows], y.reshape(-1, cout).double(), 128)


@pytest.mark.parametrize('staged', ['0', '1'])
@pytest.mark.parametrize('N,H,W,cin,cout', [(4, 32, 32, 64, 64), (3, 12, 12, 64, 128), (2, 20, 12, 128, 64), (8, 16, 16, 64, 128)])
def test_winograd_statistics_against_float64(monkeypatch, N, H, W, cin, cout, staged):
    from vpho_amd import ops
    monkeypatch.setenv('VPHO_WINO_STAGED', staged)
    x, w, b = _adversarial(N, H, W, cin, cout, 3, 300 + N)
    f = ops.BnFuse()
    y = ops.conv3x3_train(x, w, b, bn=f)
    assert f.rows == (N * H * W + 255) // 256, 'the Winograd kernel (256-pixel tile blocks) ran'
    assert torch.equal(y, ops.conv3x3_train(x, w, b))
    f2 = ops.BnFuse()
    ops.conv3x3_train(x, w, b, bn=f2)
    assert torch.equal(f2.stats[:f.rows], f.stats[:f.rows])
    _check_as_accurate(y, f, *_affine(cout, 9), f'winograd staged={staged}')
    part = f.stats[:f.rows]
    y2 = y.reshape(-1, cout).double()
    n, mean, m2 = _merged(part)
    assert torch.equal(n, torch.full_like(n, N * H * W))
    ref_m2 = ((y2 - y2.mean(0)) ** 2).sum(0)
    assert float(((m2 - ref_m2).abs() / (ref_m2 + 1e-30)).max()) < 2e-5 and bool(((m2 == 0) == (ref_m2 == 0)).all())


def test_transposed_convolution_phases_against_float64():
    """four 2x2 phase convolutions into one (N, 2H, 2W, C) map, each appending its partial rows (BnFuse(parts=4))"""
    from vpho_amd import ops
    N, H, W, cin, co = 4, 16, 16, 32, 64
    x, _, b = _adversarial(N, H, W, cin, co, 2, 400)
    up = torch.empty((N, 2 * H, 2 * W, co), device='cuda')
    f = ops.BnFuse(parts=4)
    for py in (0, 1):
        for px in (0, 1):
            _, wp, _ = _adversarial(1, 1, 1, cin, co, 2, 410 + 2 * py + px)
            ops.conv2d_nhwc(x, wp, b, kh=2, kw=2, pad_y=1 - py, pad_x=1 - px, out_hw=(H, W),
                            out_view=(up, 4 * H * W * co, 4 * W * co, 2 * co, (py * 2 * W + px) * co), bn=f)
    _check_as_accurate(up, f, *_affine(co, 10), 'transposed phases')
    n, mean, m2 = _merged(f.stats[:f.rows])
    assert torch.equal(n, torch.full_like(n, 4 * N * H * W))


@pytest.mark.parametrize('N,H,W', [(64, 64, 64), (5, 60, 60)])
def test_two_level_finish_against_float64(N, H, W):
    """more than 256 partial rows: the partial matrix is merged in chunks before the finish"""
    from vpho_amd import ops
    x, w, b = _adversarial(N, H, W, 64, 64, 1, 500 + N)
    f = ops.BnFuse()
    y = ops.conv2d_nhwc(x, w, b, bn=f)
    assert f.rows > 256
    _check_as_accurate(y, f, *_affine(64, 11), 'two-level finish')


# (N, H, W, cin, cout, k, stored gate): the input gradient dy (cout) -> da (cin) of y = conv(a), a = lrelu(bn(c) [+ shortcut]); the
# BatchNorm input c has the adversarial channel statistics.  k = 3 with a Winograd shape: the Winograd backward epilogue
BACKWARD = [(16, 16, 16, 64, 256, 1, False), (2, 9, 7, 132, 40, 1, False), (4, 16, 16, 64, 64, 3, False), (3, 10, 6, 64, 32, 3, False),
            (16, 16, 16, 256, 64, 1, True), (2, 9, 7, 40, 32, 1, True)]


@pytest.mark.parametrize('N,H,W,cin,cout,k,stored', BACKWARD)
def test_backward_sums_against_float64_autograd(N, H, W, cin, cout, k, stored):
    from vpho_amd import ops, conv_backward as CB
    std, mean, const = _channel_stats(cin)
    g = _gen(600 + N)
    c = (torch.randn((N, H, W, cin), generator=g) * std.float() + mean.float()).cuda()
    gamma, beta = _affine(cin, 601)
    short = torch.randn((N, H, W, cin), generator=g).cuda() if stored else None
    a, saved = ops.bn_train_forward(c, gamma, beta, slope=SLOPE, res=short)
    w = (torch.randn((cout, k * k * cin), generator=g) * (k * k * cin) ** -0.5).cuda()
    dy = torch.randn((N, H, W, cout), generator=g).cuda()
    pad = k // 2
    want = CB.conv2d_dgrad(dy, w, (H, W), k, k, 1, pad, gate=(a, SLOPE))
    f = ops.BnFuse(c, saved, gamma, beta, stored_gate=stored)
    got = CB.conv2d_dgrad(dy, w, (H, W), k, k, 1, pad, gate=(a, SLOPE), bn=f)
    assert f.live() and torch.equal(got, want)
    if k == 3:
        assert f.rows == (N * H * W + 255) // 256, 'the Winograd backward epilogue ran'
    # float64 autograd of the BatchNorm on the stored gradient
    c64 = c.reshape(-1, cin).double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    Fn.batch_norm(c64, None, None, g64, b64, training=True, eps=EPS).backward(got.reshape(-1, cin).double())
    ref = dict(dx=c64.grad, dg=g64.grad, db=b64.grad)
    d2 = got.reshape(-1, cin).double()
    xh = (c64.detach() - c64.detach().mean(0)) / c64.detach().var(0, unbiased=False).add(EPS).sqrt()
    scale = dict(dx=ref['dx'].abs().amax(0) + 1e-30, dg=(d2 * xh).abs().sum(0) + 1e-30, db=d2.abs().sum(0) + 1e-30)
    errs = []
    for partials in (f, None):
        dx, dg, db = ops.bn_train_backward(c, got, gamma, saved, partials=partials)
        out = dict(dx=dx.reshape(-1, cin), dg=dg, db=db)
        errs.append({k_: float(((out[k_].double() - ref[k_]).abs() / scale[k_]).max()) for k_ in ref})
    fused, alone = errs
    bad = {k_: (fused[k_], alone[k_]) for k_ in fused if not fused[k_] <= 2 * alone[k_] + 2e-6}
    assert not bad, f'backward: fused error vs float64 above 2x stand-alone + 2e-6 (fused, stand-alone): {bad}'


_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
from vpho_amd import ops, conv_backward as CB
g = torch.Generator().manual_seed(7)
for N, H, W, cin, cout, stored in ((4, 16, 16, 64, 128, False), (4, 16, 16, 64, 128, True)):
    c = (torch.randn((N, H, W, cin), generator=g) * 3 + 50).cuda()
    gamma, beta = (torch.rand(cin, generator=g) + 0.5).cuda(), (0.3 * torch.randn(cin, generator=g)).cuda()
    short = torch.randn((N, H, W, cin), generator=g).cuda() if stored else None
    a, saved = ops.bn_train_forward(c, gamma, beta, slope=0.01, res=short)
    w = (torch.randn((cout, cin), generator=g) * cin ** -0.5).cuda()
    dy = torch.randn((N, H, W, cout), generator=g).cuda()
    f = ops.BnFuse(c, saved, gamma, beta, stored_gate=stored)
    got = CB.conv2d_dgrad(dy, w, (H, W), 1, 1, gate=(a, 0.01), bn=f)
    assert not f.live(), 'the forced register-staged tile has no BatchNorm epilogue'
    want = CB.conv2d_dgrad(dy, w, (H, W), 1, 1, gate=(a, 0.01))
    r1 = ops.bn_train_backward(c, got, gamma, saved, partials=f)
    r0 = ops.bn_train_backward(c, want, gamma, saved)
    assert torch.equal(got, want)
    assert all(torch.equal(p, q) for p, q in zip(r1, r0))
print('ok')
'''


def test_fused_backward_request_on_a_kernel_without_the_epilogue_degrades():
    """VPHO_CONV_TILE=128 (read once per process: a fresh child) forces the register-staged tile, which has no BatchNorm epilogue: the
    gated input gradient falls back to the stored gate, reports no partial rows, and the BatchNorm backward runs its own pass"""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env['VPHO_CONV_TILE'] = '128'
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]

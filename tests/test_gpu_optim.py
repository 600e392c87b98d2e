"""The optimiser tail (csrc/optim.hip) leaf by leaf: ``ops.grad_sqnorm`` against an exactly rounded sum (math.fsum) and
``ops.OptimList.step`` against torch.optim.Adam / AdamW on float64 copies (tests/_optim_fp64.py), under the rule of tests/_leaf_fp64.py
(4x torch's own float32 CPU error against float64, floor 4 ulp of the largest output).  Bit-exact group: run-to-run identity of the
norm, the unclipped update when the coefficient clamps to 1, the untouched gradient and sentinels."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _leaf_fp64 as R  # noqa: E402
import _optim_fp64 as O  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = R.SENT
# csrc/optim.hip: a workgroup of 256 threads walks float4 vectors, at most 1024 workgroups -> one round of the full grid covers
# 1024 * 256 * 4 elements; the last size needs a second (partial) round of every workgroup
SQN_THREADS, SQN_MAX_BLOCKS = 256, 1024
ONE_ROUND = SQN_THREADS * SQN_MAX_BLOCKS * 4
SIZES = [1, 3, 255, 1024, 1025, 65537, ONE_ROUND + 4 * SQN_THREADS * 300 + 7]
assert ONE_ROUND < SIZES[-1] < 4 * 1024 * 1024


def _ops():
    from vpho_amd import ops
    return ops


def _mixed(n, seed):
    """values mixing 1e4 and 1e-4: the small squares vanish from a float32 running sum"""
    g = R.gen(seed)
    x = torch.randn(n, generator=g)
    big = torch.rand(n, generator=g) < 0.05
    return torch.where(big, x * 1e4, x * 1e-4)


def _same_bits64(a, b):
    return a.dtype == b.dtype == torch.float64 and bool(torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64)))


def _run_sqnorm(ops, host, off):
    n = host.numel()
    buf = torch.full((n + off + 5,), SENT, device='cuda')
    view = buf[off:off + n]
    view.copy_(host)
    assert view.data_ptr() % 16 == (4 * off) % 16
    need = ops.grad_sqnorm_workspace_bytes(n)
    assert need > 0 and need % 8 == 0 and need <= 8 * SQN_MAX_BLOCKS
    wsbuf = torch.full((need // 8 + 4,), SENT, device='cuda', dtype=torch.float64)
    ws = wsbuf[2:2 + need // 8]
    outbuf = torch.full((3,), SENT, device='cuda', dtype=torch.float64)
    a = ops.grad_sqnorm(view, ws=ws, out=outbuf[1]).clone()
    b = ops.grad_sqnorm(view, ws=ws, out=outbuf[1]).clone()
    c = ops.grad_sqnorm(view)                                       # workspace and result of its own
    torch.cuda.synchronize()
    assert _same_bits64(a, b) and _same_bits64(a, c)
    assert bool((buf[:off] == SENT).all()) and bool((buf[off + n:] == SENT).all()) and R.bits_equal(view.cpu(), host)
    assert bool((wsbuf[:2] == SENT).all()) and bool((wsbuf[2 + need // 8:] == SENT).all())
    assert float(outbuf[0]) == SENT and float(outbuf[2]) == SENT
    return a


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_grad_sqnorm_against_fsum(n, off):
    ops = _ops()
    host = _mixed(n, n + off)
    got = float(_run_sqnorm(ops, host, off))
    ref = O.sqnorm_fsum(host)
    f32 = float((host * host).sum())                               # what a float32 sum makes of it (printed, not judged)
    rel = abs(got - ref) / ref
    print(f'LEAF grad_sqnorm n={n} off={off}: rel {rel:.3e} bound {n * 2.0 ** -53:.3e}  (float32 sum: rel {abs(f32 - ref) / ref:.3e})')
    assert rel <= n * 2.0 ** -53


@pytest.mark.parametrize('off', [0, 1])
def test_grad_sqnorm_zeros_and_nan(off):
    ops = _ops()
    n = 65537
    assert float(_run_sqnorm(ops, torch.zeros(n), off)) == 0.0
    x = _mixed(n, 5)
    x[40001] = float('nan')
    assert math.isnan(float(_run_sqnorm(ops, x, off)))
    y = _mixed(3, 6)
    y[2] = float('nan')                                            # in the scalar head / tail
    assert math.isnan(float(_run_sqnorm(ops, y, off)))


def test_grad_sqnorm_rejects_bad_arguments():
    ops = _ops()
    x = torch.ones(4096, device='cuda')
    with pytest.raises(ops.VphoError):
        ops.grad_sqnorm(x, ws=torch.empty(8, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ops.VphoError):
        ops.grad_sqnorm(x.double())
    with pytest.raises(ops.VphoError):
        ops.grad_sqnorm(torch.ones(8))


# ------------------------------------------------------------------------------------------------------------------ OptimList.step
SEG_SIZES = [1, 3, 1023, 1024, 1025, 4099]
GAP = 5
KW = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.02)


def _tensors(n, g):
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    m, v = torch.randn(n, generator=g) * 0.05, torch.rand(n, generator=g) * 0.01
    gr[::4] = 0.0                                                  # zero gradients
    m[::8], v[::8] = 0.0, 0.0                                      # ... also with empty moments: 0 / (0 + eps)
    return [p, gr, m, v]


class Carved:
    """segments carved out of ONE flat buffer per role with sentinel gaps (odd offsets: no segment but the 1024-element one, placed on a
    16-byte boundary, can take the vector path), host copies beside them"""
    def __init__(self, seed, grads=None, first=GAP):
        g = R.gen(seed)
        # the 1024 segment starts at a multiple of 4 elements in every role, the others wherever the gaps put them
        total = first + sum(SEG_SIZES) + GAP * (len(SEG_SIZES) + 1) + 8
        self.flat = {k: torch.full((total,), SENT, device='cuda') for k in 'pgmv'}
        self.mask = torch.ones(total, dtype=torch.bool, device='cuda')
        self.quads, self.host, self.span, pos = [], [], [], first
        for j, n in enumerate(SEG_SIZES):
            if n == 1024:
                pos += (-pos) % 4
            src = _tensors(n, g)
            if grads is not None:
                src[1] = grads[j].clone()
            quad = []
            for k, s in zip('pgmv', src):
                view = self.flat[k][pos:pos + n]
                view.copy_(s)
                quad.append(view)
            self.mask[pos:pos + n] = False
            self.quads.append(tuple(quad))
            self.host.append(src)
            self.span.append((pos, n))
            pos += n + GAP
        assert any(q[1].data_ptr() % 16 for q in self.quads) and any(all(t.data_ptr() % 16 == 0 for t in q) for q in self.quads)
        self.grad0 = self.flat['g'].clone()

    def grad_values(self):
        """the gradient elements alone (what a flat gradient buffer without gaps would hold), as one host tensor"""
        return torch.cat([h[1] for h in self.host])

    def check_untouched(self):
        for k in 'pgmv':
            assert bool((self.flat[k][self.mask] == SENT).all()), k
        assert R.bits_equal(self.flat['g'], self.grad0)


def _sqnorm_of(ops, c):
    """the device-resident sum of squares of the segments' gradients (a compact copy: the carved buffer has sentinels between them)"""
    return ops.grad_sqnorm(c.grad_values().cuda())


@pytest.mark.parametrize('kind', ['adamw', 'adam'])
@pytest.mark.parametrize('grad_scale', [1.0, 0.5, 1.0 / 12.0])
def test_optim_list_against_float64_torch_optim(kind, grad_scale):
    """steps 1, 2 and 7 without clipping: every step is judged from the device's own state before it (moments resumed), both kinds"""
    ops = _ops()
    c = Carved(3)
    lst = ops.OptimList(c.quads)
    before = [q[0]._version for q in c.quads]
    for step in (1, 2, 7):
        state = [[t.cpu().clone() for t in q] for q in c.quads]
        lst.step(step, kind=kind, grad_scale=grad_scale, **KW)
        for j, (q, s) in enumerate(zip(c.quads, state)):
            ref, tol = R.ruled(O.optim, s, step, kind=kind, grad_scale=grad_scale, **KW)
            for name, got, r, t in zip(('param', 'exp_avg', 'exp_avg_sq'), (q[0], q[2], q[3]), ref, tol):
                R.check(f'optim {kind} n={SEG_SIZES[j]} {name} step{step} gs{grad_scale:.3f}', got, r, t)
    c.check_untouched()
    assert all(q[0]._version > b for q, b in zip(c.quads, before))


def test_optim_list_kind_names_and_numbers_agree_and_runs_repeat():
    ops = _ops()
    a, b = Carved(4), Carved(4)
    ops.OptimList(a.quads).step(2, kind='adam', grad_scale=0.5, **KW)
    ops.OptimList(b.quads).step(2, kind=1, grad_scale=0.5, **KW)
    for k in 'pmv':
        assert R.bits_equal(a.flat[k], b.flat[k])


@pytest.mark.parametrize('kind', ['adamw', 'adam'])
def test_clip_below_the_norm_is_bit_identical_to_unclipped(kind):
    ops = _ops()
    a, b = Carved(5), Carved(5)
    sq = _sqnorm_of(ops, a)
    norm = 0.5 * math.sqrt(float(sq))
    for step in (1, 2):
        ops.OptimList(a.quads).step(step, kind=kind, grad_scale=0.5, sqnorm=sq, max_norm=norm * 1.5, **KW)
        ops.OptimList(b.quads).step(step, kind=kind, grad_scale=0.5, **KW)
    for k in 'pmv':
        assert R.bits_equal(a.flat[k], b.flat[k]), k
    a.check_untouched()


@pytest.mark.parametrize('kind', ['adamw', 'adam'])
@pytest.mark.parametrize('grad_scale', [1.0, 1.0 / 12.0])
def test_clip_above_the_norm_against_the_restatement(kind, grad_scale):
    ops = _ops()
    c = Carved(6)
    sq = _sqnorm_of(ops, c)
    ref_sq = O.sqnorm_fsum(c.grad_values())
    max_norm = 0.25 * grad_scale * math.sqrt(ref_sq)
    coef = O.clip_coef(ref_sq, max_norm, grad_scale)
    assert 0.2 < coef < 0.3
    lst = ops.OptimList(c.quads)
    for step in (1, 2, 7):
        state = [[t.cpu().clone() for t in q] for q in c.quads]
        lst.step(step, kind=kind, grad_scale=grad_scale, sqnorm=sq, max_norm=max_norm, **KW)
        for j, (q, s) in enumerate(zip(c.quads, state)):
            ref, tol = R.ruled(O.optim, s, step, kind=kind, grad_scale=grad_scale, coef=coef, **KW)
            for name, got, r, t in zip(('param', 'exp_avg', 'exp_avg_sq'), (q[0], q[2], q[3]), ref, tol):
                R.check(f'clip {kind} n={SEG_SIZES[j]} {name} step{step} gs{grad_scale:.3f}', got, r, t)
    c.check_untouched()


@pytest.mark.parametrize('kind', ['adamw', 'adam'])
def test_clip_with_a_zero_gradient(kind):
    """norm 0: coef = min(1, max_norm / 1e-6) = 1, the update is the decay (AdamW) / the L2 term (Adam) alone and stays finite"""
    ops = _ops()
    zeros = [torch.zeros(n) for n in SEG_SIZES]
    a, b = Carved(7, grads=zeros), Carved(7, grads=zeros)
    sq = _sqnorm_of(ops, a)
    assert float(sq) == 0.0 and O.clip_coef(0.0, 5.0) == 1.0
    ops.OptimList(a.quads).step(3, kind=kind, sqnorm=sq, max_norm=5.0, **KW)
    ops.OptimList(b.quads).step(3, kind=kind, **KW)
    for k in 'pmv':
        assert R.bits_equal(a.flat[k], b.flat[k]), k
    for q in a.quads:
        assert bool(torch.isfinite(q[0]).all())
    a.check_untouched()


@pytest.mark.parametrize('kind', ['adamw', 'adam'])
def test_clip_with_a_nan_gradient_makes_the_update_nan(kind):
    """torch (error_if_nonfinite=False): a NaN norm gives a NaN coefficient, every gradient -- and so every parameter and moment -- is NaN"""
    ops = _ops()
    grads = [torch.randn(n, generator=R.gen(n)) * 0.1 for n in SEG_SIZES]
    grads[4][77] = float('nan')
    c = Carved(8, grads=grads)
    sq = _sqnorm_of(ops, c)
    assert math.isnan(float(sq)) and math.isnan(O.clip_coef(float('nan'), 5.0))
    ops.OptimList(c.quads).step(1, kind=kind, sqnorm=sq, max_norm=5.0, **KW)
    for q in c.quads:
        for t in (q[0], q[2], q[3]):
            assert bool(torch.isnan(t).all())
    c.check_untouched()


def test_optim_list_rejects_bad_arguments():
    ops = _ops()
    c = Carved(9)
    lst = ops.OptimList(c.quads)
    sq = _sqnorm_of(ops, c)
    with pytest.raises(ops.VphoError):
        lst.step(0, **KW)                                          # step < 1
    with pytest.raises(ops.VphoError):
        lst.step(1, kind=2, **KW)
    with pytest.raises(ops.VphoError):
        lst.step(1, sqnorm=sq, max_norm=0.0, **KW)                 # a norm without a bound
    with pytest.raises(ops.VphoError):
        lst.step(1, sqnorm=sq.float(), max_norm=1.0, **KW)
    c.check_untouched()

"""The attention reference of tests/_attention_fp64.py pinned without a GPU: against nn.MultiheadAttention in float64 (output and the
gradient with respect to qkv), against the adjoint written out per (b, h) to 1e-12 of the scale, and -- for every case the GPU test runs --
a second float32 formulation with another summation order must sit within 0.6 x R.bound of the float64 reference: a bound that torch's own
re-ordered float32 arithmetic could not keep would not be a fair one to hold a kernel to.  The case lists are checked against the host's
dispatch restated in the reference module, so every form, shape and input kind the issue names is really in them."""
import pytest
import torch

from tests import _attention_fp64 as A
from tests import _leaf_fp64 as R

f64 = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape and a.dtype == b.dtype == f64
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize('S,B,E,nhead', [(1, 3, 8, 2), (5, 2, 12, 2), (7, 3, 24, 4), (9, 1, 6, 1)])
def test_attention_is_nn_multihead_attention_in_float64(S, B, E, nhead):
    """qkv = x W^T with a random in_proj_weight, identity out_proj, no bias, p = 0: the module's output is `attention`, and the gradient
    with respect to qkv (taken through a leaf that replaces x W^T) is `attention_bwd`"""
    g = R.gen(S * E)
    mha = torch.nn.MultiheadAttention(E, nhead, bias=False, dropout=0.0).double()
    W = torch.randn(3 * E, E, generator=g, dtype=f64) * 0.4
    with torch.no_grad():
        mha.in_proj_weight.copy_(W)
        mha.out_proj.weight.copy_(torch.eye(E, dtype=f64))
    x = torch.randn(S, B, E, generator=g, dtype=f64, requires_grad=True)
    d_out = torch.randn(S, B, E, generator=g, dtype=f64)
    want = mha(x, x, x, need_weights=False)[0]
    qkv = (x.detach() @ W.t()).reshape(S * B, 3 * E)
    _close(A.attention(qkv, S, B, E, nhead), want.detach())
    # d loss / d x = (d loss / d qkv) W, and W (3E x E, random) has full column rank: compare through it and directly through a leaf qkv
    dx, = torch.autograd.grad(want, x, d_out)
    dqkv = A.attention_bwd(qkv, d_out, S, B, E, nhead)
    _close((dqkv @ W).reshape(S, B, E), dx, 1e-11)
    leaf = qkv.clone().requires_grad_(True)
    q, k, v = (t.reshape(S, B, E) for t in leaf.split(E, dim=1))
    # the module's function with identity projections applied to (q, k, v) separately
    out2 = torch.nn.functional.multi_head_attention_forward(
        q, k, v, E, nhead, None, None, None, None, False, 0.0, torch.eye(E, dtype=f64), None, use_separate_proj_weight=True,
        q_proj_weight=torch.eye(E, dtype=f64), k_proj_weight=torch.eye(E, dtype=f64), v_proj_weight=torch.eye(E, dtype=f64), need_weights=False)[0]
    _close(out2.detach(), want.detach(), 1e-11)
    _close(torch.autograd.grad(out2, leaf, d_out)[0], dqkv, 1e-11)


@pytest.mark.parametrize('S,B,E,nhead', [(1, 2, 8, 2), (5, 3, 24, 2), (13, 2, 12, 2), (66, 1, 8, 1)])
@pytest.mark.parametrize('p', [0.0, 0.3])
def test_attention_bwd_is_the_closed_form_adjoint(S, B, E, nhead, p):
    """autograd of the reference == dV = (P o M)^T dO, dP = (dO V^T) o M, dS = P o (dP - rowsum(dP o P)), dQ = dS K / sqrt(hd),
    dK = dS^T Q / sqrt(hd), to 1e-12 of the scale, with and without a mask (the mask with a fully dropped row)"""
    qkv, d_out, mask = A.make((S, B, E, nhead, p, 'droprows' if p else 'randn'))
    qkv, d_out, mask = qkv.double(), d_out.double(), None if mask is None else mask.double()
    got = A.attention_bwd(qkv, d_out, S, B, E, nhead, mask)
    _close(got, A.attention_bwd_closed(qkv, d_out, S, B, E, nhead, mask))
    _close(got, A.attention_bwd_closed(qkv, d_out, S, B, E, nhead, mask, reverse=True))
    _close(A.attention(qkv, S, B, E, nhead, mask), A.attention_alt(qkv, S, B, E, nhead, mask))
    if mask is not None:
        for bh, i in A.dropped_rows(S, B, nhead):
            b, h = divmod(bh, nhead)
            hd = E // nhead
            assert bool((got[i * B + b, h * hd:(h + 1) * hd] == 0).all())           # d q of a dropped row
            assert bool((A.attention(qkv, S, B, E, nhead, mask)[i, b, h * hd:(h + 1) * hd] == 0).all())


# ------------------------------------------------------------------------------------------------ the case lists
def test_the_case_lists_hold_every_form_shape_and_kind_of_the_issue():
    for (S, B, E, nhead, p, kind), form, _ in A.FWD_CASES:
        assert A.fwd_form(S, B, E, nhead, p > 0 or kind == 'droprows') == form, (S, B, E, nhead, p, kind)
    for (S, B, E, nhead, p, kind), form, _ in A.BWD_CASES:
        assert A.bwd_form(S, B, E, nhead) == form, (S, B, E, nhead, p, kind)
    fwd = {c[:4] for c, _, _ in A.FWD_CASES}
    assert {(1, 3, 8, 2), (17, 2, 24, 2), (64, 2, 512, 2), (256, 1, 64, 4), (257, 1, 64, 4), (300, 2, 512, 2), (1024, 1, 32, 2), (7, 3, 12, 2),
            (256, 1, 6, 1), (59, 1, 640, 2), (60, 1, 640, 2), (256, 1, 300, 2)} <= fwd
    assert A.generic_lds_bytes(59, 320) == 151276 <= A.GENERIC_LDS_LIMIT < 153840 == A.generic_lds_bytes(60, 320)
    # masks of both rates on both fast instantiations, S > 256 included
    for form in ('mha_kernel<4>', 'mha_kernel<16>'):
        assert {0.1, 0.3} <= {c[4] for c, f, _ in A.FWD_CASES if f == form}
    bwd = {c[:4] for c, _, _ in A.BWD_CASES}
    want = {(1, 2, 8, 2), (5, 3, 24, 2), (63, 2, 40, 2), (64, 2, 128, 4), (64, 1, 1024, 2), (65, 2, 24, 2), (128, 1, 64, 2), (129, 1, 600, 2),
            (1024, 1, 16, 2)}
    assert want <= bwd
    for shape in want:                                                          # each with p = 0 and with a mask
        ps = {c[4] for c, _, _ in A.BWD_CASES if c[:4] == shape}
        assert 0.0 in ps and any(p > 0 for p in ps), shape
    # every input kind on every form (masks, so 'droprows', exist on the fast forward forms and the backward only)
    for cases, forms, masked in ((A.FWD_CASES, ('mha_kernel<4>', 'mha_kernel<16>'), True), (A.FWD_CASES, ('generic, LDS', 'generic, in place'), False),
                                 (A.BWD_CASES, ('one launch', 'three launches'), True)):
        for form in forms:
            kinds = {c[5] for c, f, _ in cases if f == form}
            assert kinds >= {'randn', 'large', 'qzero'} | ({'droprows'} if masked else set()), (form, kinds)
    assert len({A.case_id(c) for c, _, _ in A.FWD_CASES}) == len(A.FWD_CASES) and len({A.case_id(c) for c, _, _ in A.BWD_CASES}) == len(A.BWD_CASES)
    # the refusals of the GPU test, by the restated dispatch
    assert A.bwd_form(5, 1, 12, 2).startswith('refused') and A.bwd_form(1025, 1, 16, 2).startswith('refused')
    assert A.fwd_form(5, 1, 12, 2, masked=True).startswith('refused') and A.fwd_form(300, 1, 12, 2).startswith('refused')


def test_large_inputs_do_overflow_a_naive_softmax():
    """the 'large' kind is what it is for: float32 exp of the raw logits is infinite somewhere, the reference stays finite"""
    for cases in (A.FWD_CASES, A.BWD_CASES):
        for case, _, _ in cases:
            if case[5] == 'large':
                S, B, E, nhead = case[:4]
                qkv = A.make(case)[0]
                q, k, _ = A.split(qkv, S, B, E, nhead)
                logits = (q / (E // nhead) ** 0.5) @ k.transpose(-1, -2)
                assert float(logits.abs().max()) > 100 and bool(torch.isinf(torch.exp(logits)).any()), (case, float(logits.abs().max()))
                assert bool(torch.isfinite(A.attention(qkv, S, B, E, nhead)).all())


@pytest.mark.parametrize('case', [c for c, _, _ in A.FWD_CASES], ids=A.case_id)
def test_forward_bound_holds_another_float32_summation_order(case):
    S, B, E, nhead = case[:4]
    qkv, _, mask = A.make(case)
    ref = A.attention(qkv.double(), S, B, E, nhead, None if mask is None else mask.double())
    tol = R.bound(A.attention(qkv, S, B, E, nhead, mask), ref)
    err = R.worst(A.attention_alt(qkv, S, B, E, nhead, mask), ref)
    print(f'ALT fwd {A.case_id(case)}: worst {err:.3e} bound {tol:.3e} ratio {err / tol:.2f}')
    assert err <= 0.6 * tol, (err, tol)
    if case[5] == 'qzero' and mask is None:                                      # uniform probabilities: the mean of v
        v = A.split(qkv.double(), S, B, E, nhead)[2]
        assert R.worst(ref, v.mean(2, keepdim=True).expand_as(v).permute(2, 0, 1, 3).reshape(S, B, E)) <= 1e-14


@pytest.mark.parametrize('case', [c for c, _, _ in A.BWD_CASES], ids=A.case_id)
def test_backward_bound_holds_another_float32_summation_order(case):
    S, B, E, nhead = case[:4]
    qkv, d_out, mask = A.make(case)
    m64 = None if mask is None else mask.double()
    ref = A.attention_bwd(qkv.double(), d_out.double(), S, B, E, nhead, m64)
    tol = R.bound(A.attention_bwd(qkv, d_out, S, B, E, nhead, mask), ref)
    err = R.worst(A.attention_bwd_closed(qkv, d_out, S, B, E, nhead, mask, reverse=True), ref)
    print(f'ALT bwd {A.case_id(case)}: worst {err:.3e} bound {tol:.3e} ratio {err / tol:.2f}')
    assert err <= 0.6 * tol, (err, tol)

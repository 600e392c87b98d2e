"""Every launch form of the attention kernels (csrc/misc.hip: mha_kernel<4>, mha_kernel<16>, mha_generic_kernel with K / V in LDS or read
in place; csrc/train_physics.hip: mha_bwd_kernel and the three-launch long form) against the float64 reference of tests/_attention_fp64.py
(pinned without a GPU by tests/test_attention_fp64_cpu.py) on the float32 inputs the kernel saw.  The host picks a form by head size,
sequence length and LDS bytes; nothing reports which one ran, so each case carries the dispatch clause its shape meets
(A.FWD_CASES / A.BWD_CASES, checked against the restated dispatch on the CPU; confirmed with one value-only mutant per form, docs/LOG.md).

Arithmetic is held to R.bound (4 x torch's own float32 CPU error against float64, floor 4 ulp of the largest output), computed in each test
from the same inputs; every comparison covers every output element."""
import pytest
import torch

from tests import _attention_fp64 as A
from tests import _leaf_fp64 as R

pytestmark = pytest.mark.gpu


def _ops():
    from vpho_amd import ops
    return ops


def _dev(t):
    return None if t is None else t.cuda().contiguous()


_REF = {}


def _reference(case, bwd):
    """float32 CPU inputs, float64 reference and bound of one case, computed once and shared (never modified)"""
    key = (case, bwd)
    if key not in _REF:
        S, B, E, nhead = case[:4]
        qkv, d_out, mask = A.make(case)
        m64 = None if mask is None else mask.double()
        if bwd:
            ref = A.attention_bwd(qkv.double(), d_out.double(), S, B, E, nhead, m64)
            tol = R.bound(A.attention_bwd(qkv, d_out, S, B, E, nhead, mask), ref)
        else:
            ref = A.attention(qkv.double(), S, B, E, nhead, m64)
            tol = R.bound(A.attention(qkv, S, B, E, nhead, mask), ref)
        _REF[key] = (qkv, d_out, mask, ref, tol)
    return _REF[key]


def _head_cols(h, hd):
    return slice(h * hd, (h + 1) * hd)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('case,form,why', A.FWD_CASES, ids=[A.case_id(c) for c, _, _ in A.FWD_CASES])
def test_forward_every_form_against_float64(case, form, why):
    """ops.mha -> vpho_mha_dropout_f32.  Dispatch: head_dim % 4 == 0 and head_dim <= 256 -> mha_kernel<4> (S <= 256) or mha_kernel<16>
    (257 <= S <= 1024); any other head_dim (S <= 256, no mask) -> mha_generic_kernel, K / V staged in LDS when 4 S (2 hd + 1) <= 150 KB
    ('generic, LDS'), read in place above that ('generic, in place').  `form` is the clause the case meets (A.fwd_form), `why` what the
    shape is there for.  Input kinds: randn * 0.5; 'large' = randn * 6, logits near +-150 (a soft-max without the max subtraction
    overflows); 'qzero' = q = 0, uniform probabilities, so without a mask the output is the mean of v within the bound; 'droprows' = a
    mask with fully dropped rows, whose output rows are exactly 0.  Repeated launches give the same bits."""
    ops = _ops()
    S, B, E, nhead, p, kind = case
    hd = E // nhead
    qkv, _, mask, ref, tol = _reference(case, False)
    assert A.fwd_form(S, B, E, nhead, mask is not None) == form
    dq, dm = _dev(qkv), _dev(mask)
    got = ops.mha(dq, S, B, E, nhead, drop=dm)
    R.check(f'mha fwd {form} {A.case_id(case)}', got, ref, tol)
    assert R.bits_equal(ops.mha(dq, S, B, E, nhead, drop=dm), got)
    if kind == 'qzero' and mask is None:
        v = A.split(qkv.double(), S, B, E, nhead)[2]                               # (B, nhead, S, hd)
        mean = v.mean(2, keepdim=True).expand_as(v).permute(2, 0, 1, 3).reshape(S, B, E)
        assert R.worst(got, mean) <= tol
    if kind == 'droprows':
        g = got.cpu()
        for bh, i in A.dropped_rows(S, B, nhead):
            assert bool((g[i, bh // nhead, _head_cols(bh % nhead, hd)] == 0).all()), (bh, i)
        assert bool((ref != 0).any())


@pytest.mark.parametrize('case,form', [(c, f) for c, f, _ in A.FWD_CASES if c[1] > 1], ids=[A.case_id(c) for c, _, _ in A.FWD_CASES if c[1] > 1])
def test_forward_batch_slice_equals_a_launch_with_one_batch_entry(case, form):
    """every form with B > 1: the (b) slice of the launch is bit-identical to the same rows launched with B = 1 (the row stride B * 3E
    and the block index are the only things B enters; the form does not depend on B)"""
    ops = _ops()
    S, B, E, nhead = case[:4]
    qkv, _, mask, _, _ = _reference(case, False)
    got = ops.mha(_dev(qkv), S, B, E, nhead, drop=_dev(mask)).cpu()
    for b in range(B):
        one = ops.mha(_dev(qkv.view(S, B, 3 * E)[:, b]), S, 1, E, nhead, drop=None if mask is None else _dev(mask[b * nhead:(b + 1) * nhead]))
        assert R.bits_equal(one.cpu()[:, 0], got[:, b]), (form, b)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize('case,form,why', A.BWD_CASES, ids=[A.case_id(c) for c, _, _ in A.BWD_CASES])
def test_backward_both_forms_against_float64_autograd(case, form, why):
    """ops.mha_bwd -> vpho_mha_bwd_ws_f32.  Dispatch: S <= 64 -> mha_bwd_kernel, one launch, P and dS in LDS; 65 <= S <= 1024 ->
    mha_bwd_scores_kernel, mha_bwd_softmax_kernel, mha_bwd_grads_kernel over a workspace of two S x S tables per (b, head).  Head sizes
    that are no multiple of 16 (12, 20, 300: the `nc` column tail of the 16-column LDS chunks), below 64 (the c < hd guard of the grads
    kernel), above 256 (the c += 256 loop of the one-launch kernel, several 64-column passes of the grads kernel), more than four
    64-blocks and S = 1024 (all 16 slots per lane of the soft-max kernel).  d q, d k and d v are each held to the bound of the whole
    gradient and to their own.  With fully dropped mask rows the d q rows are exactly 0.  Repeated launches give the same bits."""
    ops = _ops()
    S, B, E, nhead, p, kind = case
    hd = E // nhead
    qkv, d_out, mask, ref, tol = _reference(case, True)
    assert A.bwd_form(S, B, E, nhead) == form
    dq, dd, dm = _dev(qkv), _dev(d_out), _dev(mask)
    got = ops.mha_bwd(dq, dd, S, B, E, nhead, drop=dm)
    R.check(f'mha bwd {form} {A.case_id(case)}', got, ref, tol)
    f32 = A.attention_bwd(qkv, d_out, S, B, E, nhead, mask)
    for i, name in enumerate(('dq', 'dk', 'dv')):
        cols = slice(i * E, (i + 1) * E)
        R.check(f'mha bwd {form} {A.case_id(case)} {name}', got[:, cols], ref[:, cols], R.bound(f32[:, cols], ref[:, cols]))
    assert R.bits_equal(ops.mha_bwd(dq, dd, S, B, E, nhead, drop=dm), got)
    if kind == 'droprows':
        g = got.cpu()
        for bh, i in A.dropped_rows(S, B, nhead):
            assert bool((g[i * B + bh // nhead, _head_cols(bh % nhead, hd)] == 0).all()), (bh, i)


@pytest.mark.parametrize('case,form', [(c, f) for c, f, _ in A.BWD_CASES if c[1] > 1], ids=[A.case_id(c) for c, _, _ in A.BWD_CASES if c[1] > 1])
def test_backward_batch_slice_equals_a_launch_with_one_batch_entry(case, form):
    """both backward forms with B > 1: the (b) rows of d qkv are bit-identical to the same data launched with B = 1"""
    ops = _ops()
    S, B, E, nhead = case[:4]
    qkv, d_out, mask, _, _ = _reference(case, True)
    got = ops.mha_bwd(_dev(qkv), _dev(d_out), S, B, E, nhead, drop=_dev(mask)).cpu().view(S, B, 3 * E)
    for b in range(B):
        one = ops.mha_bwd(_dev(qkv.view(S, B, 3 * E)[:, b]), _dev(d_out[:, b]), S, 1, E, nhead,
                          drop=None if mask is None else _dev(mask[b * nhead:(b + 1) * nhead]))
        assert R.bits_equal(one.cpu(), got[:, b]), (form, b)


# ------------------------------------------------------------------------------------------------ the alias entry points
@pytest.mark.parametrize('case', [c for c, _, _ in A.FWD_CASES if c[4] == 0 and c[5] == 'randn'], ids=A.case_id)
def test_alias_vpho_mha_f32_gives_the_wrappers_bits(case):
    """vpho_mha_f32 = vpho_mha_dropout_f32 without a mask: every forward form, the same bits as ops.mha"""
    ops = _ops()
    S, B, E, nhead = case[:4]
    qkv = _dev(_reference(case, False)[0])
    out = torch.full((S, B, E), R.SENT, device='cuda')
    ops._call('vpho_mha_f32', qkv, S, B, E, nhead, out)
    assert R.bits_equal(out, ops.mha(qkv, S, B, E, nhead))


@pytest.mark.parametrize('case', [c for c, f, _ in A.BWD_CASES if f == 'one launch'], ids=A.case_id)
def test_alias_vpho_mha_bwd_f32_gives_the_wrappers_bits(case):
    """vpho_mha_bwd_f32 = vpho_mha_bwd_ws_f32 without a workspace, S <= 64: the same bits as ops.mha_bwd, with and without a mask"""
    ops = _ops()
    S, B, E, nhead = case[:4]
    qkv, d_out, mask = (_dev(t) for t in _reference(case, True)[:3])
    dqkv = torch.full((S * B, 3 * E), R.SENT, device='cuda')
    ops._call('vpho_mha_bwd_f32', qkv, d_out, S, B, E, nhead, mask, dqkv)
    assert R.bits_equal(dqkv, ops.mha_bwd(qkv, d_out, S, B, E, nhead, drop=mask))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_limit_and_launch_nothing():
    """vpho_mha_bwd_f32 at S = 65 (the one-launch kernel holds 64 positions); the backward with head_dim 6 (four feature columns at a
    time) and at S = 1025 (at most 1024 positions); a dropout mask with head_dim 6 (the generic kernel takes none); head_dim 6 at
    S = 300 (the generic kernel holds 4 slots: 256 positions).  Each answers VphoError with the limit in its message before anything is
    launched: the destination keeps its sentinel.  The buffers passed are valid for the sizes each call names."""
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device='cuda')
    sent = lambda *s: torch.full(s, R.SENT, device='cuda')
    E, nhead = 24, 2
    d65 = sent(65 * 1, 3 * E)
    with pytest.raises(ops.VphoError, match=r'65 exceeds the 64 positions'):
        ops._call('vpho_mha_bwd_f32', z(65, 3 * E), z(65, E), 65, 1, E, nhead, None, d65)
    with pytest.raises(ops.VphoError, match=r'head_dim 6 is not a multiple of 4'):
        ops.mha_bwd(z(5, 36), z(5, 12), 5, 1, 12, 2)
    d6 = sent(5, 36)
    with pytest.raises(ops.VphoError, match=r'head_dim 6 is not a multiple of 4'):
        ops._call('vpho_mha_bwd_ws_f32', z(5, 36), z(5, 12), 5, 1, 12, 2, None, d6, None)
    with pytest.raises(ops.VphoError, match=r'at most 1024 positions'):
        ops.mha_bwd(z(1025, 3 * 16), z(1025, 16), 1025, 1, 16, 2)
    d1025, ws = sent(1025, 48), torch.zeros(16, dtype=torch.uint8, device='cuda')
    with pytest.raises(ops.VphoError, match=r'1025 exceeds the 1024 positions'):
        ops._call('vpho_mha_bwd_ws_f32', z(1025, 48), z(1025, 16), 1025, 1, 16, 2, None, d1025,
                  ws)
    with pytest.raises(ops.VphoError, match=r'dropout mask needs head_dim % 4 == 0 and head_dim <= 256 \(got 6\)'):
        ops.mha(z(5, 36), 5, 1, 12, 2, drop=torch.ones(2, 5, 5, device='cuda'))
    with pytest.raises(ops.VphoError, match=r'head_dim 6 is served for sequences .* up to 256 only; got 300'):
        ops.mha(z(300, 36), 300, 1, 12, 2)
    torch.cuda.synchronize()
    assert bool((d65 == R.SENT).all()) and bool((d6 == R.SENT).all()) and bool((d1025 == R.SENT).all())

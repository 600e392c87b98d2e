"""Plain torch restatement of the attention kernels (csrc/misc.hip: mha_kernel<4>, mha_kernel<16>, mha_generic_kernel; csrc/train_physics.hip:
mha_bwd_kernel and the three-launch long form) and the case lists tests/test_gpu_attention.py and tests/test_attention_fp64_cpu.py share.
TEST INFRASTRUCTURE ONLY: nothing here imports ``vpho_amd.ops``.

As in tests/_leaf_fp64.py every function computes in the dtype of its tensor arguments: ``attention(*to64(args))`` is the float64 reference
on the float32 inputs the kernel saw, ``attention(*args)`` torch's own float32 evaluation from which R.bound derives the tolerance.
Layout: qkv (S*B, 3E), row s*B + b, columns [q | k | v], head h = columns h*hd .. h*hd + hd - 1 of each third; the output (S, B, E);
the mask (B*nhead, S, S) is the keep-mask already divided by 1 - p (nn.MultiheadAttention's dropout on the probabilities)."""
import math

import torch

from tests import _leaf_fp64 as R


def _heads(x, S, B, nhead, hd):
    """(S*B, nhead*hd) -> (B, nhead, S, hd)"""
    return x.reshape(S, B, nhead, hd).permute(1, 2, 0, 3)


def _rows(x, S, B, E):
    """(B, nhead, S, hd) -> (S, B, E)"""
    return x.permute(2, 0, 1, 3).reshape(S, B, E)


def split(qkv, S, B, E, nhead):
    hd = E // nhead
    return [_heads(qkv[:, i * E:(i + 1) * E], S, B, nhead, hd) for i in range(3)]


def attention(qkv, S, B, E, nhead, mask=None):
    """softmax((q / sqrt(hd)) k^T) [* mask] v -> (S, B, E)"""
    hd = E // nhead
    q, k, v = split(qkv, S, B, E, nhead)
    P = torch.softmax((q / math.sqrt(hd)) @ k.transpose(-1, -2), dim=-1)
    if mask is not None:
        P = P * mask.reshape(B, nhead, S, S)
    return _rows(P @ v, S, B, E)


def attention_bwd(qkv, d_out, S, B, E, nhead, mask=None):
    """autograd of `attention` with the seed d_out (S, B, E) -> d qkv (S*B, 3E)"""
    x = qkv.detach().clone().requires_grad_(True)
    return torch.autograd.grad(attention(x, S, B, E, nhead, mask), x, d_out.reshape(S, B, E))[0]


def attention_alt(qkv, S, B, E, nhead, mask=None):
    """the same operator summed in another order: feature axis and key axis reversed, the soft-max written out"""
    hd = E // nhead
    q, k, v = split(qkv, S, B, E, nhead)
    s = torch.einsum('bhid,bhjd->bhij', q.flip(-1), k.flip(-1).flip(-2)) / math.sqrt(hd)          # keys reversed
    e = torch.exp(s - s.amax(-1, keepdim=True))
    P = e / e.sum(-1, keepdim=True)
    if mask is not None:
        P = P * mask.reshape(B, nhead, S, S).flip(-1)
    return _rows(torch.einsum('bhij,bhjd->bhid', P, v.flip(-2)), S, B, E)


def attention_bwd_closed(qkv, d_out, S, B, E, nhead, mask=None, reverse=False):
    """the adjoint written out per (b, h):  dV = (P o M)^T dO,  dP = (dO V^T) o M,  dS = P o (dP - rowsum(dP o P)),
    dQ = dS K / sqrt(hd),  dK = dS^T Q / sqrt(hd).  reverse=True walks every reduction axis backwards (another summation order)."""
    hd = E // nhead
    scl = 1.0 / math.sqrt(hd)
    q, k, v = split(qkv, S, B, E, nhead)
    dO = _heads(d_out.reshape(S * B, E), S, B, nhead, hd)
    M = None if mask is None else mask.reshape(B, nhead, S, S)
    if reverse:                                                       # queries, keys and features all reversed, undone at the end
        q, k, v, dO = (t.flip(-1).flip(-2) for t in (q, k, v, dO))
        M = None if M is None else M.flip(-1).flip(-2)
    s = (q @ k.transpose(-1, -2)) * scl
    e = torch.exp(s - s.amax(-1, keepdim=True))
    P = e / e.sum(-1, keepdim=True)
    PM = P if M is None else P * M
    dV = PM.transpose(-1, -2) @ dO
    dP = dO @ v.transpose(-1, -2)
    if M is not None:
        dP = dP * M
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    dQ, dK = (dS @ k) * scl, (dS.transpose(-1, -2) @ q) * scl
    if reverse:
        dQ, dK, dV = (t.flip(-1).flip(-2) for t in (dQ, dK, dV))
    return torch.cat([_rows(t, S, B, E).reshape(S * B, E) for t in (dQ, dK, dV)], 1)


# ------------------------------------------------------------------------------------------------ the host's dispatch, restated
GENERIC_LDS_LIMIT = 150 * 1024


def generic_lds_bytes(S, hd):
    return 4 * S * (2 * hd + 1)


def fwd_form(S, B, E, nhead, masked=False):
    """the launch form vpho_mha_dropout_f32 picks (csrc/misc.hip), or the refusal it answers"""
    hd = E // nhead
    if S > 1024:
        return 'refused: S > 1024'
    if hd % 4 == 0 and hd <= 256 and E % 4 == 0:
        return 'mha_kernel<4>' if S <= 256 else 'mha_kernel<16>'
    if S > 256:
        return 'refused: this head_dim up to 256 positions only'
    if masked:
        return 'refused: mask needs head_dim % 4 == 0 and <= 256'
    return 'generic, LDS' if generic_lds_bytes(S, hd) <= GENERIC_LDS_LIMIT else 'generic, in place'


def bwd_form(S, B, E, nhead):
    """the launch form vpho_mha_bwd_ws_f32 picks (csrc/train_physics.hip)"""
    hd = E // nhead
    if hd % 4 != 0:
        return 'refused: head_dim % 4 != 0'
    if S > 1024:
        return 'refused: S > 1024'
    return 'one launch' if S <= 64 else 'three launches'


# ------------------------------------------------------------------------------------------------ cases
# (S, B, E, nhead, p, input kind), the form the dispatch sends it to, and what the shape is there for.
# kinds: 'randn' = randn * 0.5;  'large' = randn * 6 (logit std 36 whatever the head size: logits near +-150, a soft-max without the max
# subtraction overflows);  'qzero' = q = 0 (uniform probabilities);  'droprows' = a mask with fully dropped rows (p as given elsewhere).
FWD_CASES = [
    ((1, 3, 8, 2, 0.0, 'randn'), 'mha_kernel<4>', 'hd 4, one position'),
    ((17, 2, 24, 2, 0.0, 'randn'), 'mha_kernel<4>', 'hd 12, a last chunk of one query'),
    ((17, 2, 24, 2, 0.3, 'droprows'), 'mha_kernel<4>', 'hd 12, dropped rows'),
    ((64, 2, 512, 2, 0.0, 'randn'), 'mha_kernel<4>', 'hd 256: all four feature chunks'),
    ((64, 2, 512, 2, 0.1, 'randn'), 'mha_kernel<4>', 'hd 256 with a mask'),
    ((256, 1, 64, 4, 0.0, 'randn'), 'mha_kernel<4>', 'the last S of the 4-slot form'),
    ((256, 1, 64, 4, 0.3, 'randn'), 'mha_kernel<4>', 'the last S of the 4-slot form, mask'),
    ((33, 2, 64, 2, 0.0, 'large'), 'mha_kernel<4>', 'hd 32, logits near +-150'),
    ((33, 2, 64, 2, 0.1, 'qzero'), 'mha_kernel<4>', 'uniform probabilities under a mask'),
    ((33, 2, 64, 2, 0.0, 'qzero'), 'mha_kernel<4>', 'uniform probabilities'),
    ((257, 1, 64, 4, 0.0, 'randn'), 'mha_kernel<16>', 'one key in the fifth slot'),
    ((257, 1, 64, 4, 0.1, 'randn'), 'mha_kernel<16>', 'one key in the fifth slot, mask'),
    ((257, 1, 64, 2, 0.0, 'large'), 'mha_kernel<16>', 'hd 32, logits near +-150'),
    ((257, 1, 64, 2, 0.0, 'qzero'), 'mha_kernel<16>', 'uniform probabilities'),
    ((300, 2, 512, 2, 0.0, 'randn'), 'mha_kernel<16>', 'hd 256, B = 2'),
    ((300, 2, 512, 2, 0.3, 'droprows'), 'mha_kernel<16>', 'hd 256, mask with dropped rows'),
    ((1024, 1, 32, 2, 0.0, 'randn'), 'mha_kernel<16>', 'all 16 slots'),
    ((1024, 1, 32, 2, 0.1, 'randn'), 'mha_kernel<16>', 'all 16 slots, mask'),
    ((7, 3, 12, 2, 0.0, 'randn'), 'generic, LDS', 'hd 6'),
    ((7, 3, 12, 2, 0.0, 'large'), 'generic, LDS', 'hd 6, logits near +-150'),
    ((7, 3, 12, 2, 0.0, 'qzero'), 'generic, LDS', 'hd 6, uniform probabilities'),
    ((256, 1, 6, 1, 0.0, 'randn'), 'generic, LDS', 'hd 6 at the longest sequence'),
    ((59, 1, 640, 2, 0.0, 'randn'), 'generic, LDS', 'hd 320: 151 276 B, just under the switch'),
    ((60, 1, 640, 2, 0.0, 'randn'), 'generic, in place', 'hd 320: 153 840 B, just over the switch'),
    ((60, 1, 640, 2, 0.0, 'large'), 'generic, in place', 'hd 320, logits near +-150'),
    ((60, 1, 640, 2, 0.0, 'qzero'), 'generic, in place', 'hd 320, uniform probabilities'),
    ((256, 1, 300, 2, 0.0, 'randn'), 'generic, in place', 'hd 150 at the longest sequence'),
]

_BWD_SHAPES = [
    ((1, 2, 8, 2), 'one launch', 'hd 4, one position'),
    ((5, 3, 24, 2), 'one launch', 'hd 12: one chunk of 12 columns'),
    ((63, 2, 40, 2), 'one launch', 'hd 20: chunks of 16 and 4'),
    ((64, 2, 128, 4), 'one launch', 'the full 64 x 64 table'),
    ((64, 1, 1024, 2), 'one launch', 'hd 512: the c += 256 loop'),
    ((65, 2, 24, 2), 'three launches', 'one row in the second block, hd 12 < 64'),
    ((128, 1, 64, 2), 'three launches', 'whole blocks'),
    ((129, 1, 600, 2), 'three launches', 'hd 300: four full 64-column passes and one of 44'),
    ((1024, 1, 16, 2), 'three launches', '16 slots per lane, 16 MB workspace'),
]
BWD_CASES = []
for _i, (_shape, _form, _why) in enumerate(_BWD_SHAPES):
    BWD_CASES += [((*_shape, 0.0, 'randn'), _form, _why), ((*_shape, (0.1, 0.3)[_i % 2], 'randn'), _form, _why + ', mask')]
BWD_CASES += [
    ((33, 2, 64, 2, 0.0, 'large'), 'one launch', 'hd 32, logits near +-150'),
    ((33, 2, 64, 2, 0.0, 'qzero'), 'one launch', 'uniform probabilities'),
    ((33, 2, 64, 2, 0.3, 'droprows'), 'one launch', 'dropped rows: d q rows exactly 0'),
    ((130, 2, 64, 2, 0.0, 'large'), 'three launches', 'hd 32, logits near +-150'),
    ((130, 2, 64, 2, 0.0, 'qzero'), 'three launches', 'uniform probabilities'),
    ((130, 2, 64, 2, 0.1, 'droprows'), 'three launches', 'dropped rows: d q rows exactly 0'),
]


def case_id(case):
    S, B, E, nhead, p, kind = case
    return f'S{S}-B{B}-E{E}-h{nhead}-p{p}-{kind}'


def dropped_rows(S, B, nhead):
    """[(bh, i)] of the rows a 'droprows' mask clears entirely: the first and the last query of every odd head-batch, one in the middle of 0"""
    rows = [(0, S // 2)]
    for bh in range(1, B * nhead, 2):
        rows += [(bh, 0), (bh, S - 1)]
    return sorted(set(rows))


def make(case, seed=None):
    """-> float32 CPU qkv (S*B, 3E), d_out (S, B, E), mask (B*nhead, S, S) or None"""
    S, B, E, nhead, p, kind = case
    g = R.gen(S * 1000 + E + nhead + int(p * 10) if seed is None else seed)
    qkv = torch.randn(S * B, 3 * E, generator=g) * (6.0 if kind == 'large' else 0.5)
    if kind == 'qzero':
        qkv[:, :E] = 0.0
    d_out = torch.randn(S, B, E, generator=g)
    mask = None
    if p > 0 or kind == 'droprows':
        mask = (torch.rand(B * nhead, S, S, generator=g) >= p).float() / (1.0 - p)
        if kind == 'droprows':
            for bh, i in dropped_rows(S, B, nhead):
                mask[bh, i] = 0.0
    return qkv.contiguous(), d_out.contiguous(), mask

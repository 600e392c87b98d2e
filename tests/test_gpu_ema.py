"""``ops.EmaList.update`` (vpho_ema_multi_f32, csrc/ema.hip) against the reference's ``ExponentialMovingAverage`` on the CPU: the fixture
written from that class (tests/golden/golden_ema.npz) and its numpy restatement (tests/_ema_fp32.py), bit for bit.

Bit for bit means every element, the planted NaN and what the planted +inf turns into (inf - inf one update later) included."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ema_fp32 as EF  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 12345.0


def _ops():
    from vpho_amd import ops
    return ops


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_ema.npz')))


def _split(flat):
    out, o = [], 0
    for n in EF.SIZES:
        out.append(flat[o:o + n])
        o += n
    return out


def _check(name, got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    differ = int((EF.bits(got) != EF.bits(want)).sum())
    print(f'EMA {name}: {got.size} elements, {int(np.isnan(want).sum())} NaN, {differ} differ')
    assert EF.same_bits(got, want), f'{name}: {differ} elements differ'


@pytest.mark.parametrize('decay', EF.DECAYS)
def test_fixture_sequence_bit_for_bit(gold, decay):
    """twelve updates with new parameter values each time, separately allocated tensors; updates 1, 2, 8 and 12 against the class's shadows"""
    ops = _ops()
    p = [torch.from_numpy(a.copy()).cuda() for a in _split(gold['init'])]
    s = [t.clone() for t in p]
    lst = ops.EmaList(list(zip(p, s)))
    assert lst.n == len(EF.SIZES) and lst.blocks == sum((n + 1023) // 1024 for n in EF.SIZES)
    count, seen = 0, 0
    for u in range(1, EF.UPDATES + 1):
        for t, a in zip(p, _split(gold['params'][u - 1])):
            t.copy_(torch.from_numpy(a.copy()))
        omd, count = EF.one_minus_decay(decay, count)
        lst.update(omd)
        if u in EF.KEPT:
            _check(f'decay {decay} update {u}', torch.cat(s).cpu().numpy(), gold[f'shadow_{decay}'][EF.KEPT.index(u)])
            seen += 1
        assert EF.same_bits(torch.cat(p).cpu().numpy(), gold['params'][u - 1])           # the parameters are only read
    assert seen == 4 and count == EF.UPDATES


@pytest.mark.parametrize('p_off,s_off', [(0, 0), (1, 0), (0, 3), (2, 1)])
def test_carved_out_of_one_buffer_with_sentinels(gold, p_off, s_off):
    """every tensor at an offset of its own inside one buffer: p_off / s_off elements past a 16-byte boundary, so both pointers, one or
    neither are aligned (the float4 path needs both) and, with sentinels between the segments, a store past an end shows"""
    ops = _ops()

    def carve(arrays, off):
        starts, o = [], 0
        for a in arrays:
            o = (o + 3) // 4 * 4 + 4 + off                        # >= 4 sentinels before every segment, the wanted residue mod 4
            starts.append(o)
            o += a.size
        buf = torch.full((o + 8,), SENT, device='cuda')
        assert buf.data_ptr() % 16 == 0
        views = [buf[b:b + a.size] for b, a in zip(starts, arrays)]
        for v, a in zip(views, arrays):
            v.copy_(torch.from_numpy(a.copy()))
            assert v.data_ptr() % 16 == 4 * off
        mask = torch.ones_like(buf, dtype=torch.bool)
        for b, a in zip(starts, arrays):
            mask[b:b + a.size] = False
        return buf, views, mask

    init, par = _split(gold['init']), _split(gold['params'][1])              # update 2's parameters: the planted NaN and inf
    pbuf, p, pmask = carve(par, p_off)
    sbuf, s, smask = carve(init, s_off)
    p_before = pbuf.clone()
    omd = float(gold['omd_0.999'][3])
    ops.EmaList(list(zip(p, s))).update(omd)
    for i, (sv, a, b) in enumerate(zip(s, init, par)):
        _check(f'carved p+{p_off} s+{s_off} tensor {i}', sv.cpu().numpy(), EF.update(a, b, omd))
    assert bool((sbuf[smask] == SENT).all()) and int(smask.sum()) >= 4 * len(EF.SIZES)
    assert EF.same_bits(pbuf.cpu().numpy(), p_before.cpu().numpy())


@pytest.fixture(scope='module')
def real_layout():
    """569 tensors with the element counts of the real parameters (63.7 M elements), random values; the host result of one update"""
    shapes = [p['shape'] for p in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'golden_param_order.json')))['params']]
    sizes = [int(np.prod(s)) if s else 1 for s in shapes]
    assert len(sizes) == 569 and 63_000_000 < sum(sizes) < 64_500_000
    g = torch.Generator().manual_seed(11)
    s0 = [torch.randn(n, generator=g) for n in sizes]
    p0 = [t + 0.01 * torch.randn(n, generator=g) for t, n in zip(s0, sizes)]
    omd = 1.0 - min(0.999, (1 + 5) / (10 + 5))
    want = [EF.update(s.numpy(), p.numpy(), omd) for s, p in zip(s0, p0)]
    return dict(sizes=sizes, s0=s0, p0=p0, omd=omd, want=want)


def test_real_layout_equals_the_host_restatement_and_repeats(real_layout):
    ops = _ops()
    R = real_layout
    runs = []
    for _ in range(2):
        p = [t.cuda() for t in R['p0']]
        s = [t.cuda() for t in R['s0']]
        lst = ops.EmaList(list(zip(p, s)))
        assert lst.n == 569 and lst.blocks == sum((n + 1023) // 1024 for n in R['sizes'])
        lst.update(R['omd'])
        runs.append([t.cpu().numpy() for t in s])
        assert all(torch.equal(a.cpu(), b) for a, b in zip(p[:8], R['p0'][:8]))
    bad = [i for i, (g, w) in enumerate(zip(runs[0], R['want'])) if not EF.same_bits(g, w)]
    assert not bad, f'tensors that differ from the restatement: {bad[:8]} (sizes {[R["sizes"][i] for i in bad[:8]]})'
    assert all(EF.same_bits(a, b) for a, b in zip(*runs))                               # two runs, the same bits


def test_zero_rate_leaves_finite_shadows_unchanged(gold):
    ops = _ops()
    p = [torch.from_numpy(a.copy()).cuda() for a in _split(gold['params'][0])]
    s = [torch.from_numpy(a.copy()).cuda() for a in _split(gold['init'])]
    before = torch.cat(s).cpu().numpy()
    assert np.isfinite(before).all() and (before != 0).all()                            # (a shadow of -0.0 would become -0 - (+-0), as in torch)
    ops.EmaList(list(zip(p, s))).update(0.0)
    assert EF.same_bits(torch.cat(s).cpu().numpy(), before)                             # s - 0 * d = s for finite d


def test_empty_list_launches_nothing():
    ops = _ops()
    lst = ops.EmaList([])
    assert lst.n == 0 and lst.blocks == 0 and lst.table is None
    lst.update(0.5)
    # the entry point itself: no tensors = success without a launch; a negative count or a missing table = the argument error
    call = lambda table, n, blocks: ops.lib.vpho_ema_multi_f32(table, n, blocks, 0.5, None)
    assert call(None, 0, 0) == 0
    for table, n, blocks in ((None, 1, 1), (None, -1, 0), (None, 0, -1)):
        assert call(table, n, blocks) != 0
        assert 'vpho_ema_multi_f32: bad argument' in ops.lib.vpho_last_error().decode()
    torch.cuda.synchronize()


def test_wrapper_refuses_mismatched_pairs():
    ops = _ops()
    a = torch.zeros(8, device='cuda')
    with pytest.raises(ops.VphoError, match='elements'):
        ops.EmaList([(a, torch.zeros(9, device='cuda'))])
    with pytest.raises(ops.VphoError, match='float32'):
        ops.EmaList([(a, torch.zeros(8, device='cuda', dtype=torch.float64))])
    with pytest.raises(ops.VphoError, match='float32'):
        ops.EmaList([(a.half(), a)])
    with pytest.raises(ops.VphoError, match='GPU tensors only'):
        ops.EmaList([(a, torch.zeros(8))])
    with pytest.raises(ops.VphoError, match='contiguous'):
        ops.EmaList([(a, torch.zeros(8, 2, device='cuda')[:, 0])])

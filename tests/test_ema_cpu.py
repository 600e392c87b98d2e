"""The weights' moving average without a GPU: the numpy restatement (tests/_ema_fp32.py) against the fixture written from the reference's
class (tests/golden/golden_ema.npz), ``WeightEma``'s decay sequence and ``state_dict()`` layout, the exchange of
``custom_checkpoint_0.pkl`` with accelerate in both directions, the file sets with and without ``custom``, the two flags, the errors of
``--use_ema``, and the compiler's report for the kernel."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ema_fp32 as EF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'golden_ema.npz')
ORDER = os.path.join(ROOT, 'tests', 'golden', 'golden_param_order.json')
FILES = {'model.safetensors', 'optimizer.bin', 'scheduler.bin', 'random_states_0.pkl'}
EMA_FILE = 'custom_checkpoint_0.pkl'


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


# ---------------------------------------------------------------------------------------------------------------------- arithmetic
def test_fixture_holds_what_the_issue_lists(gold):
    assert tuple(gold['sizes']) == EF.SIZES == (1, 3, 1023, 1024, 1025, 2048, 4099) and tuple(gold['kept']) == EF.KEPT == (1, 2, 8, 12)
    assert tuple(gold['decays']) == EF.DECAYS == (0.999, 0.5) and gold['params'].shape == (EF.UPDATES, sum(EF.SIZES)) == (12, 9223)
    assert list(gold['state_dict_keys']) == ['decay', 'num_updates', 'shadow_params']
    assert os.path.getsize(GOLD) < 1000000
    u, t, inf_at, nan_at = (int(v) for v in gold['planted'])
    off = sum(EF.SIZES[:t])
    p = gold['params']
    assert np.isposinf(p[u - 1, off + inf_at]) and np.isnan(p[u - 1, off + nan_at]) and np.isfinite(p).sum() == p.size - 2
    assert np.isfinite(gold['init']).all()
    lo, hi = (float(np.abs(gold['init'][:1]).max()), float(np.abs(gold['init'][-EF.SIZES[-1]:]).max()))
    assert lo < 0.1 and hi > 100.0                                                      # magnitudes from 1e-2 to 1e2
    for d in EF.DECAYS:                                                                 # 0.999: warm-up throughout; 0.5: `decay` from update 8
        want = [1.0 - min(d, (1 + k) / (10 + k)) for k in range(1, EF.UPDATES + 1)]
        assert list(gold[f'omd_{d}']) == want
    assert all(o == 0.5 for o in gold['omd_0.5'][7:]) and all(o > 0.5 for o in gold['omd_0.5'][:7]) and all(o > 0.001 for o in gold['omd_0.999'])


@pytest.mark.parametrize('decay', EF.DECAYS)
def test_restatement_equals_the_reference_class_to_the_bit(gold, decay):
    s, count, kept = gold['init'].copy(), 0, {}
    for u in range(1, EF.UPDATES + 1):
        omd, count = EF.one_minus_decay(decay, count)
        assert omd == gold[f'omd_{decay}'][u - 1]
        s = EF.update(s, gold['params'][u - 1], omd)
        if u in EF.KEPT:
            kept[u] = s.copy()
    for i, u in enumerate(EF.KEPT):
        assert EF.same_bits(kept[u], gold[f'shadow_{decay}'][i]), (decay, u)
    # what IEEE makes of the planted values: the NaN stays, the inf arrives as +inf and is inf - inf from the next update on
    pu, t, inf_at, nan_at = (int(v) for v in gold['planted'])
    off = sum(EF.SIZES[:t])
    assert np.isfinite(kept[1]).all() and np.isposinf(kept[pu][off + inf_at]) and np.isnan(kept[pu][off + nan_at])
    for u in (8, 12):
        assert np.isnan(kept[u][[off + inf_at, off + nan_at]]).all() and np.isfinite(kept[u]).sum() == kept[u].size - 2


def test_a_contracted_multiply_subtract_would_show(gold):
    """fma(-omd32, d, s): the product of two float32 is exact in float64, so this is the fused operation up to a double rounding"""
    s, p, omd = gold['init'], gold['params'][0], float(np.float32(gold['omd_0.999'][0]))
    fused = (s.astype(np.float64) - omd * (s - p).astype(np.float32).astype(np.float64)).astype(np.float32)
    assert int((EF.bits(fused) != EF.bits(gold['shadow_0.999'][0])).sum()) > 0          # 3 869 of 9 223 when the fixture was written


# ---------------------------------------------------------------------------------------------------------------------- host object
def test_weight_ema_decay_sequence_and_value_error():
    from vpho_amd.ema import WeightEma
    for decay in EF.DECAYS:
        e, count = WeightEma(decay), 0
        assert e.num_updates == 0
        for _ in range(30):
            want, count = EF.one_minus_decay(decay, count)
            got = e.next_one_minus_decay()
            assert got == want and isinstance(got, float) and e.num_updates == count
    fixed = WeightEma(0.75, use_num_updates=False)
    assert fixed.num_updates is None and [fixed.next_one_minus_decay() for _ in range(3)] == [0.25] * 3 and fixed.num_updates is None
    assert WeightEma(0.0).decay == 0.0 and WeightEma(1.0).decay == 1.0
    for bad in (-0.01, 1.01):
        with pytest.raises(ValueError, match='Decay must be between 0 and 1'):
            WeightEma(bad)


def test_state_dict_layout_is_the_reference_class(gold):
    from vpho_amd.ema import STATE_KEYS, WeightEma
    e = WeightEma(0.999)
    assert list(e.state_dict()) == list(gold['state_dict_keys']) == list(STATE_KEYS)
    sd = dict(decay=0.5, num_updates=None, shadow_params=[torch.arange(6.).view(2, 3), torch.ones(4, dtype=torch.float64)])
    e.load_state_dict(sd)
    out = e.state_dict()
    assert out['decay'] == 0.5 and out['num_updates'] is None                          # None = a fixed decay, as in the reference
    assert [tuple(t.shape) for t in out['shadow_params']] == [(2, 3), (4,)] and all(t.dtype == torch.float32 and not t.is_cuda for t in out['shadow_params'])
    assert e.next_one_minus_decay() == 0.5 and e.num_updates is None
    with pytest.raises(KeyError):
        e.load_state_dict(dict(decay=0.5))


def test_overlay_follows_the_reference_parameter_order(model_cpu):
    """shadow i belongs to parameter i of the 569 of tests/golden/golden_param_order.json (all trainable), in the REFERENCE's shape;
    buffers are not averaged"""
    from vpho_amd.ema import overlay
    G = json.load(open(ORDER))['params']
    assert len(G) == 569 and all(p['requires_grad'] for p in G)
    names = [k for k, p in model_cpu.named_parameters() if p.requires_grad]
    assert names == [p['name'] for p in G]
    sd = model_cpu.state_dict()
    state = dict(decay=0.999, num_updates=3, shadow_params=[torch.full(p['shape'], float(i)) for i, p in enumerate(G)])
    out = overlay(sd, state, names)
    assert list(out) == list(sd)
    for i, p in enumerate(G):
        assert list(out[p['name']].shape) == p['shape'] and bool((out[p['name']] == float(i)).all())
    buffers = [k for k in sd if k not in set(names)]
    assert buffers and all(out[k] is sd[k] for k in buffers) and any(k.endswith('running_mean') for k in buffers)
    with pytest.raises(ValueError):
        overlay(sd, dict(state, shadow_params=state['shadow_params'][:-1]), names)
    with pytest.raises(ValueError):
        overlay(sd, dict(state, shadow_params=[torch.zeros(7)] + state['shadow_params'][1:]), names)


# ---------------------------------------------------------------------------------------------------------------------- files
class StandIn:
    """an object as ``accel.register_for_checkpointing`` takes it: ``state_dict`` / ``load_state_dict``, the reference's layout"""
    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.state = dict(decay=0.999, num_updates=seed, shadow_params=[torch.randn(4, 3, 3, 3, generator=g), torch.randn(5, generator=g)])

    def state_dict(self):
        return self.state

    def load_state_dict(self, state):
        self.state = state


def _same_state(a, b):
    return (list(a) == list(b) and a['decay'] == b['decay'] and a['num_updates'] == b['num_updates'] and len(a['shadow_params']) == len(b['shadow_params'])
            and all(torch.equal(x, y) and x.shape == y.shape for x, y in zip(a['shadow_params'], b['shadow_params'])))


def _tiny_state():
    from vpho_amd import checkpoint as CK
    import test_checkpoint_state_cpu as T
    m = T.Tiny(1)
    sched = CK.make_scheduler('exp', 2e-4)
    return m, T._fabricated_optimizer_state(m, 2, sched.lr), sched


def test_file_sets_with_and_without_custom(tmp_path):
    from vpho_amd import checkpoint as CK
    m, opt, sched = _tiny_state()
    plain = CK.save_state(str(tmp_path / 'epoch_1.state'), m.state_dict(), opt, sched.state_dict())
    assert set(os.listdir(plain)) == FILES and CK.load_state(plain, restore_rng=False)['custom'] == []
    for i, empty in enumerate((None, [], ())):
        d = CK.save_state(str(tmp_path / f'e{i}'), m.state_dict(), opt, sched.state_dict(), custom=empty)
        assert set(os.listdir(d)) == FILES
    a, b = StandIn(3), StandIn(4)
    d = CK.save_state(str(tmp_path / 'epoch_2.state'), m.state_dict(), opt, sched.state_dict(), custom=[a.state_dict()])
    assert set(os.listdir(d)) == FILES | {EMA_FILE} and CK.custom_file(0) == EMA_FILE
    got = CK.load_state(d, restore_rng=False)
    assert len(got['custom']) == 1 and _same_state(got['custom'][0], a.state_dict())
    d = CK.save_state(str(tmp_path / 'epoch_3.state'), m.state_dict(), opt, sched.state_dict(), custom=[a.state_dict(), b.state_dict()])
    assert set(os.listdir(d)) == FILES | {EMA_FILE, 'custom_checkpoint_1.pkl'}
    got = CK.load_state(d, restore_rng=False)
    assert [_same_state(x, y.state_dict()) for x, y in zip(got['custom'], (a, b))] == [True, True]
    # a rank other than 0 writes its generator file only
    d = CK.save_state(str(tmp_path / 'rank1'), m.state_dict(), opt, sched.state_dict(), rank=1, custom=[a.state_dict()])
    assert os.listdir(d) == ['random_states_1.pkl']
    # the other files are byte for byte what a call without the keyword writes
    for f in ('model.safetensors', 'optimizer.bin', 'scheduler.bin'):
        assert open(os.path.join(plain, f), 'rb').read() == open(os.path.join(str(tmp_path / 'epoch_2.state'), f), 'rb').read(), f


def test_accelerate_reads_the_custom_file_save_state_writes(tmp_path):
    """``accel.load_state`` of a reference user who registered the object (it calls ``load_custom_state`` for it), and that function alone"""
    import test_checkpoint_state_cpu as T
    from accelerate.checkpointing import load_custom_state
    from vpho_amd import checkpoint as CK
    m, opt_state, sched = _tiny_state()
    for g in opt_state['param_groups']:
        g.update(sched.group_extras())
    ours = StandIn(5)
    d = CK.save_state(str(tmp_path / 'epoch_1.state'), m.state_dict(), opt_state, sched.state_dict(), custom=[ours.state_dict()])
    model = T.Tiny(7)
    opt = torch.optim.AdamW(model.parameters(), betas=(0.9, 0.999), eps=1e-8, lr=2e-4)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, 0.96)
    accel = T._accelerator()
    model, opt, sch = accel.prepare(model, opt, sch)
    theirs, alone = StandIn(6), StandIn(9)
    assert not _same_state(theirs.state_dict(), ours.state_dict())
    accel.register_for_checkpointing(theirs)
    accel.load_state(d)
    assert _same_state(theirs.state_dict(), ours.state_dict())
    assert all(torch.equal(model.state_dict()[k], v) for k, v in m.state_dict().items())          # the four other files still load beside it
    load_custom_state(alone, d, 0)
    assert _same_state(alone.state_dict(), ours.state_dict())


def test_load_state_reads_the_custom_file_accelerate_writes(tmp_path):
    """a whole ``accel.save_state`` with a registered object, so that the file is where and what accelerate itself makes it"""
    import test_checkpoint_state_cpu as T
    from vpho_amd import checkpoint as CK
    model = T.Tiny(3)
    opt = torch.optim.AdamW(model.parameters(), lr=2e-4)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, 0.96)
    accel = T._accelerator()
    model, opt, sch = accel.prepare(model, opt, sch)
    obj = StandIn(8)
    accel.register_for_checkpointing(obj)
    d = str(tmp_path / 'epoch_1.state')
    accel.save_state(d)
    assert set(os.listdir(d)) == FILES | {EMA_FILE}
    got = CK.load_state(d, restore_rng=False)
    assert len(got['custom']) == 1 and _same_state(got['custom'][0], obj.state_dict())


# ---------------------------------------------------------------------------------------------------------------------- flags, --use_ema
def test_flags_defaults_and_parsing():
    from vpho_amd.configs import args as A
    p = A._parser()
    d = p.parse_args([])
    assert d.ema_rate == 0.0 and isinstance(d.ema_rate, float) and d.use_ema is False
    c = A.Config()
    assert c.ema_rate == 0.0 and c.use_ema is False
    a = p.parse_args(['--mode', 'train', '--max_epochs', '2', '--ema_rate', '0.999'])
    assert a.ema_rate == 0.999 and a.use_ema is False
    for mode in ('eval', 'infer'):
        a = p.parse_args(['--mode', mode, '--checkpoint', 'x/checkpoint/epoch_1.state', '--use_ema'])
        assert a.use_ema is True and a.ema_rate == 0.0
    with pytest.raises(SystemExit):
        p.parse_args(['--ema_rate', 'fast'])
    import inspect
    from vpho_amd import checkpoint as CK
    sig = inspect.signature(CK.save_state).parameters
    assert list(sig)[-1] == 'custom' and sig['custom'].default is None and list(sig)[:7] == ['dir', 'model_state_dict', 'optimizer_state', 'scheduler_state',
                                                                                           'rank', 'world', 'step']


def test_use_ema_errors_name_the_file_and_the_way_out(tmp_path):
    from vpho_amd import checkpoint as CK
    from vpho_amd.trainer import ema_state_dict
    m, opt, sched = _tiny_state()
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    without = CK.save_state(str(tmp_path / 'epoch_1.state'), m.state_dict(), opt, sched.state_dict())
    with pytest.raises(FileNotFoundError, match=re.escape(EMA_FILE)):
        ema_state_dict(without, m.state_dict(), names)
    plain = CK.save_model(str(tmp_path / 'final_model.pt'), m.state_dict())
    with pytest.raises(ValueError, match='final_model_ema.pt'):
        ema_state_dict(plain, m.state_dict(), names)
    with pytest.raises(ValueError, match='--checkpoint'):
        ema_state_dict('', m.state_dict(), names)
    # and with the file: the shadows land on the trained tensors by order, the frozen bias and the buffers stay
    shadows = [torch.full(tuple(m.state_dict()[k].shape), 7.0 + i) for i, k in enumerate(names)]
    with_file = CK.save_state(str(tmp_path / 'epoch_2.state'), m.state_dict(), opt, sched.state_dict(),
                              custom=[dict(decay=0.999, num_updates=4, shadow_params=shadows)])
    out, path = ema_state_dict(with_file, m.state_dict(), names)
    assert path.endswith(EMA_FILE) and list(out) == list(m.state_dict())
    for k, v in m.state_dict().items():
        assert bool((out[k] == 7.0 + names.index(k)).all()) if k in names else torch.equal(out[k], v), k
    assert 'fc.bias' not in names and 'bn.running_mean' in out


# ---------------------------------------------------------------------------------------------------------------------- kernel, header
def test_ema_kernel_reports_no_spill_and_no_scratch():
    """the compiler's own report (vpho_amd/build.py keeps it next to the object), as tests/test_kernel_resources.py reads it"""
    from vpho_amd.build import build_extension
    build_extension()
    seen, name = {}, None
    for line in open(os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'ema.hip.usage.txt')):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (('spill', r'VGPRs Spill: (\d+)'), ('sspill', r'SGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds', r'LDS Size \[bytes/block\]: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    ks = [k for k in seen if 'ema_multi_kernel' in k]
    assert len(ks) == 1 and len(seen) == 1, sorted(seen)
    assert seen[ks[0]] == dict(spill=0, sspill=0, scratch=0, lds=0), seen[ks[0]]


def test_entry_point_is_an_addition_at_abi_13():
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert re.search(r'VPHO_API int vpho_ema_multi_f32\(const void\* table, int n_tensors, long long blocks, float one_minus_decay, void\* stream\);', hdr)
    assert 'lib/model/ema.py:25-44' in hdr
    count = hdr.count('VPHO_API ') - 1                              # the #define aside: one per declaration
    assert count >= 118                                             # 117 before this one
    for doc in ('README.md', 'INTEGRATION.md'):                     # the documents say what the header says
        assert f'{count} ' in open(os.path.join(ROOT, doc)).read(), (doc, count)
    src = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'ema.hip')).read()
    assert 'fp contract(off)' in src and '__shared__' not in src and 'atomic' not in src

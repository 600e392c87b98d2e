"""The weights' moving average inside training: ``DiffusionTrainStep(..., ema=decay)`` only reads the weights, its shadows equal a host
replay of the reference's class (tests/_ema_fp32.py) through ``state_dict()`` in the reference's layout, ``Trainer.fit`` with
``--ema_rate`` writes ``custom_checkpoint_0.pkl`` / ``final_model_ema.pt`` and resumes exactly, and ``main.py --mode eval --use_ema``
evaluates the averaged weights.  Fixture and helpers of tests/test_gpu_train_fit.py (BS 12; batch 8 / repeat_num 4 for ``Trainer``)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ema_fp32 as EF  # noqa: E402
import _leaf_fp64 as R  # noqa: E402
import test_gpu_train_fit as TF  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = TF.ROOT
DECAY = 0.999
EMA_FILE = 'custom_checkpoint_0.pkl'
FILES = {'model.safetensors', 'optimizer.bin', 'scheduler.bin', 'random_states_0.pkl'}
case = TF.case                                                     # the 13-loss fixture: every one of the 569 tensors gets a gradient


def _step(s, case, **kw):
    return s.step(case['data'], case['gt_h'], case['gt_o'], case['draws'], **kw)


@pytest.fixture(scope='module')
def trio(case):
    """two steps side by side, with and without the average, three fused steps each; what each held after every step"""
    a, b = TF._make(case, ema=DECAY), TF._make(case)
    rec = dict(a=a, b=b, init=a.state_dict(), init_ema=a.ema_state(), losses=[], sd=[], ema=[])
    for _ in range(3):
        La, Lb = _step(a, case, fused=True), _step(b, case, fused=True)
        rec['losses'].append(({k: float(v) for k, v in La.items()}, {k: float(v) for k, v in Lb.items()}))
        rec['sd'].append(a.state_dict())
        rec['ema'].append(a.ema_state())
    return rec


def test_the_average_only_reads(trio):
    a, b = trio['a'], trio['b']
    assert a.steps == b.steps == 3 and len(a.names) == 569
    assert all(la == lb for la, lb in trio['losses'])
    for k in a.names:
        assert R.bits_equal(a.master[k], b.master[k]) and R.bits_equal(a.m[k], b.m[k]) and R.bits_equal(a.v[k], b.v[k]), k
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(R.bits_equal(sa[k], sb[k]) for k in sa)               # running statistics included
    # without a rate: nothing allocated, nothing to launch, and the accessors say so
    assert b.ema is None and b.shadow is None and b._ema_list is None
    for f in (b.ema_state, lambda: b.state_dict(ema=True), lambda: b.load_ema_state(trio['init_ema'])):
        with pytest.raises(ValueError, match='ema='):
            f()
    assert set(a.shadow) == set(a.master) and all(a.shadow[k].shape == a.master[k].shape and a.shadow[k].data_ptr() != a.master[k].data_ptr() for k in a.master)


def test_shadows_equal_a_host_replay_in_the_reference_layout(trio):
    """shadow' = update(shadow, parameter after the step) on the tensors of ``state_dict()``, in the reference's shapes and order: a wrong
    permutation between the packed layout and (cout, cin, kh, kw) shows on every convolution"""
    a = trio['a']
    order = a.param_order
    G = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'golden_param_order.json')))['params']
    assert order == [p['name'] for p in G]
    st0 = trio['init_ema']
    assert list(st0) == ['decay', 'num_updates', 'shadow_params'] and st0['decay'] == DECAY and st0['num_updates'] == 0
    assert [list(t.shape) for t in st0['shadow_params']] == [p['shape'] for p in G]
    assert all(t.dtype == torch.float32 and not t.is_cuda and t.is_contiguous() for t in st0['shadow_params'])
    assert all(R.bits_equal(t, trio['init'][k].cpu().reshape(t.shape)) for k, t in zip(order, st0['shadow_params']))       # clones of the parameters
    shadow, count = [t.numpy().copy() for t in st0['shadow_params']], 0
    for u in range(3):
        omd, count = EF.one_minus_decay(DECAY, count)
        st, sd = trio['ema'][u], trio['sd'][u]
        assert st['num_updates'] == count == u + 1 and st['decay'] == DECAY
        shadow = [EF.update(s, sd[k].cpu().numpy().reshape(s.shape), omd) for k, s in zip(order, shadow)]
        bad = [k for k, s, got in zip(order, shadow, st['shadow_params']) if got.shape != s.shape or not EF.same_bits(got.numpy(), s)]
        assert not bad, (u, len(bad), bad[:5])
    # ALL tensors are averaged: a shadow has moved wherever its parameter has (a tensor with zero gradient and zero value stays put)
    moved = [not torch.equal(x, y) for x, y in zip(trio['ema'][2]['shadow_params'], st0['shadow_params'])]
    stepped = [not torch.equal(trio['sd'][2][k], trio['init'][k]) for k in order]
    assert moved == stepped and sum(moved) > 500, (sum(moved), sum(stepped))
    # padding lanes of a packed convolution weight stay zero in the shadow, as in the master
    k = 'feature_extractor.layer0_h.0.weight'
    cout, cin, kh, kw = a._conv_meta[k]
    pad = a.shadow[k].view(cout, kh, kw, -1)[..., cin:]
    assert pad.numel() > 0 and not bool(pad.any()) and not bool(a.master[k].view(cout, kh, kw, -1)[..., cin:].any())


def test_state_dict_with_the_average_and_the_round_trip(trio, case):
    a = trio['a']
    live, avg, st = a.state_dict(), a.state_dict(ema=True), a.ema_state()
    assert list(live) == list(avg)
    trained = set(a.master)
    differ = 0
    for k in live:
        assert avg[k].shape == live[k].shape and avg[k].is_cuda
        if k in trained:                                           # the average lags behind every tensor the optimiser has moved
            assert torch.equal(avg[k], live[k]) == torch.equal(live[k], trio['init'][k]), k
            differ += not torch.equal(avg[k], live[k])
        else:
            assert R.bits_equal(avg[k], live[k]), k
    assert differ > 500 and sum(k not in trained for k in live) > 100 and any(k.endswith('t_encoder.0.W') for k in live if k not in trained)
    for k, t in zip(a.param_order, st['shadow_params']):
        assert R.bits_equal(avg[k].cpu().reshape(t.shape), t), k
    # load_ema_state(ema_state()) is the identity: into the step itself, and into a fresh one with another rate
    before = {k: v.clone() for k, v in a.shadow.items()}
    a.load_ema_state(st)
    assert a.ema.num_updates == 3 and a.ema.decay == DECAY and all(R.bits_equal(a.shadow[k], before[k]) for k in before)
    other = TF._make(case, ema=0.5)
    other.load_ema_state(st)
    assert other.ema.num_updates == 3 and other.ema.decay == DECAY and all(R.bits_equal(other.shadow[k], before[k]) for k in before)
    again = other.ema_state()
    assert all(R.bits_equal(x, y) for x, y in zip(again['shadow_params'], st['shadow_params']))
    fixed = dict(st, num_updates=None)
    other.load_ema_state(fixed)
    assert other.ema.num_updates is None and other.ema.next_one_minus_decay() == 1.0 - DECAY       # None: a fixed decay, as in the reference
    with pytest.raises(ValueError):
        other.load_ema_state(dict(st, shadow_params=st['shadow_params'][:-1]))


def test_accumulation_counts_optimiser_updates_and_the_plain_step_counts_too(case):
    s = TF._make(case, ema=DECAY)
    for i in range(4):                                                                        # A = 2 over 4 batches
        _step(s, case, fused=True, accumulation=(i % 2, 2))
        assert s.ema.num_updates == s.steps == (i + 1) // 2
    assert s.ema.num_updates == 2
    frozen = {k: v.clone() for k, v in s.shadow.items()}
    _step(s, case, fused=True, accumulation=(0, 2))                                           # a micro-step that does not step: nothing moves
    assert s.ema.num_updates == 2 and all(R.bits_equal(s.shadow[k], frozen[k]) for k in frozen)
    _step(s, case, fused=True, accumulation=(1, 2))
    prev = s.ema_state()
    _step(s, case)                                                                            # the unfused form of step
    assert s.ema.num_updates == s.steps == 4
    omd, _ = EF.one_minus_decay(DECAY, 3)
    sd, now = s.state_dict(), s.ema_state()
    for k, was, got in zip(s.param_order, prev['shadow_params'], now['shadow_params']):
        assert EF.same_bits(got.numpy(), EF.update(was.numpy(), sd[k].cpu().numpy().reshape(was.shape), omd)), k


# ------------------------------------------------------------------------------------------------------------------ Trainer.fit
COMMON = dict(batch_size=8, num_batches=2, train_scope='full', repeat_num=4, gradient_clip=5.0, scheduler='exp', optimizer='adamw',
              gradient_accumulation_steps=1, max_epochs=2, print_freq=1, use_ema=False)


def _fit(save_dir, checkpoint='', epochs=None, **kw):
    from vpho_amd.trainer import Trainer
    with TF._Cfg(checkpoint=checkpoint, **dict(COMMON, **kw)) as cfg:
        return Trainer(cfg).fit(epochs=epochs, save_dir=save_dir)


def _same_ema(a, b):
    return (list(a) == list(b) == ['decay', 'num_updates', 'shadow_params'] and a['decay'] == b['decay'] and a['num_updates'] == b['num_updates']
            and len(a['shadow_params']) == len(b['shadow_params']) == 569
            and all(x.shape == y.shape and R.bits_equal(x, y) for x, y in zip(a['shadow_params'], b['shadow_params'])))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """A: 2 epochs x 2 steps with the average; B: its first epoch; C: B resumed; D: one epoch WITHOUT the average"""
    d = tmp_path_factory.mktemp('ema_fit')
    A, B, C, D = (str(d / n) for n in 'ABCD')
    out = dict(A=A, B=B, C=C, D=D, dir=d)
    out['straight'] = _fit(A, ema_rate=DECAY)
    out['first'] = _fit(B, epochs=1, ema_rate=DECAY)
    out['resumed'] = _fit(C, checkpoint=os.path.join(B, 'checkpoint', 'epoch_1.state'), ema_rate=DECAY)
    out['plain'] = _fit(D, epochs=1, ema_rate=0.0)
    return out


def test_resume_with_the_average_is_exact(runs):
    A, B, C = runs['A'], runs['B'], runs['C']
    assert runs['straight']['ema'] is True and runs['resumed']['ema'] is True and 'ema' not in runs['plain']
    assert (runs['straight']['start_epoch'], runs['resumed']['start_epoch'], runs['resumed']['epochs']) == (0, 1, 2)
    assert runs['resumed']['losses'][0] == runs['straight']['losses'][1]
    ck = os.path.join(B, 'checkpoint', 'epoch_1.state')
    assert set(os.listdir(ck)) == FILES | {EMA_FILE} and set(os.listdir(A)) == {'checkpoint', 'final_model.pt', 'final_model_ema.pt'}
    ea, ec = (os.path.join(x, 'checkpoint', 'epoch_2.state') for x in (A, C))
    ca, cc, c1 = TF._load(os.path.join(ea, EMA_FILE)), TF._load(os.path.join(ec, EMA_FILE)), TF._load(os.path.join(ck, EMA_FILE))
    assert _same_ema(ca, cc) and ca['num_updates'] == 4 and ca['decay'] == DECAY and c1['num_updates'] == 2
    assert all(not t.is_cuda and t.dtype == torch.float32 for t in ca['shadow_params'])
    ma, mc = TF._load(os.path.join(A, 'final_model_ema.pt')), TF._load(os.path.join(C, 'final_model_ema.pt'))
    fa, fc = TF._load(os.path.join(A, 'final_model.pt')), TF._load(os.path.join(C, 'final_model.pt'))
    assert list(ma) == list(mc) == list(fa) == list(fc)
    assert all(TF._same(ma[k], mc[k]) for k in ma) and all(TF._same(fa[k], fc[k]) for k in fa)
    oa, oc = TF._load(os.path.join(ea, 'optimizer.bin')), TF._load(os.path.join(ec, 'optimizer.bin'))
    assert set(oa['state']) == set(oc['state']) == set(range(569)) and oa['param_groups'] == oc['param_groups']
    for i in oa['state']:
        assert all(R.bits_equal(oa['state'][i][k], oc['state'][i][k]) for k in ('step', 'exp_avg', 'exp_avg_sq')), i
    # final_model_ema.pt = the live model with the 569 trained tensors replaced by the shadows of the last state directory
    G = [p['name'] for p in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'golden_param_order.json')))['params']]
    for k, t in zip(G, ca['shadow_params']):
        assert R.bits_equal(ma[k].reshape(t.shape), t), k
    assert all(TF._same(ma[k], fa[k]) for k in fa if k not in set(G))
    # model.safetensors always holds the LIVE weights
    from safetensors.torch import load_file
    m2, m1 = load_file(os.path.join(ea, 'model.safetensors')), load_file(os.path.join(ck, 'model.safetensors'))
    bad = [k for k in fa if not TF._same(m2[k], fa[k])]
    assert not bad, (len(bad), bad[:8])
    # ... and the average lags behind exactly the tensors that training moves (a zero tensor with a zero gradient stays where it is)
    lags, moves = [not torch.equal(ma[k], fa[k]) for k in G], [not torch.equal(m1[k], fa[k]) for k in G]
    print(f'EMA fit: {sum(lags)} of {len(G)} averaged tensors differ from the live ones, {sum(moves)} moved in the second epoch')
    assert lags == moves and all(lags[G.index(k)] for k in ('head_physics.fc_scale.2.weight', 'feature_extractor.layer1_h.0.0.conv1.weight',
                                                             'denoiser_hand.head.head.0.weight', 'encoder_obj.project.weight'))


def test_a_run_without_the_rate_writes_what_it_always_wrote(runs):
    """the epoch of a run without --ema_rate beside the same epoch with it: the four files only, and byte for byte the same weights,
    optimiser and scheduler -- the average changes nothing it does not own"""
    d0, d1 = (os.path.join(runs[x], 'checkpoint', 'epoch_1.state') for x in ('D', 'B'))
    assert set(os.listdir(d0)) == FILES and set(os.listdir(runs['D'])) == {'checkpoint', 'final_model.pt'}
    for f in ('model.safetensors', 'optimizer.bin', 'scheduler.bin'):
        assert open(os.path.join(d0, f), 'rb').read() == open(os.path.join(d1, f), 'rb').read(), f
    assert open(os.path.join(runs['D'], 'final_model.pt'), 'rb').read() == open(os.path.join(runs['B'], 'final_model.pt'), 'rb').read()


def test_resume_from_a_state_without_the_file_starts_from_the_live_weights(runs, capfd):
    from safetensors.torch import load_file
    ck = os.path.join(runs['D'], 'checkpoint', 'epoch_1.state')
    E = str(runs['dir'] / 'E')
    out = _fit(E, checkpoint=ck, ema_rate=DECAY, num_batches=1)                              # one more epoch of ONE step: an exact replay
    assert out['ema'] is True and out['start_epoch'] == 1
    assert f'holds no {EMA_FILE}' in capfd.readouterr().out
    e2 = os.path.join(E, 'checkpoint', 'epoch_2.state')
    st = TF._load(os.path.join(e2, EMA_FILE))
    assert st['num_updates'] == 1 and st['decay'] == DECAY
    start, after = load_file(os.path.join(ck, 'model.safetensors')), load_file(os.path.join(e2, 'model.safetensors'))
    omd, _ = EF.one_minus_decay(DECAY, 0)
    G = [p['name'] for p in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'golden_param_order.json')))['params']]
    for k, t in zip(G, st['shadow_params']):
        assert EF.same_bits(t.numpy(), EF.update(start[k].numpy().reshape(t.shape), after[k].numpy().reshape(t.shape), omd)), k


def test_eval_loader_sees_the_average_and_training_goes_on_from_the_live_weights(tmp_path, monkeypatch):
    """the module's tensors can BE the step's masters (a packed 1x1 weight is a view of the parameter it was built from), so evaluating
    the average must not leak it into training: two epochs with an ``eval_loader`` end in the bits of two epochs without one, and what
    ``eval`` found in the module after each epoch were that epoch's shadows beside the live running statistics"""
    from safetensors.torch import load_file
    from vpho_amd.trainer import Trainer
    X, Y = str(tmp_path / 'X'), str(tmp_path / 'Y')
    _fit(X, ema_rate=DECAY, num_batches=1)
    seen = []
    monkeypatch.setattr(Trainer, 'eval', lambda self, loader=None, **kw: seen.append({k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}))
    with TF._Cfg(checkpoint='', **dict(COMMON, ema_rate=DECAY, num_batches=1)) as cfg:
        Trainer(cfg).fit(save_dir=Y, eval_loader=[{}])
    assert len(seen) == 2
    G = [p['name'] for p in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'golden_param_order.json')))['params']]
    for e, model in enumerate(seen):
        d = os.path.join(Y, 'checkpoint', f'epoch_{e + 1}.state')
        st, live = TF._load(os.path.join(d, EMA_FILE)), load_file(os.path.join(d, 'model.safetensors'))
        assert st['num_updates'] == e + 1
        for k, t in zip(G, st['shadow_params']):
            assert R.bits_equal(model[k].reshape(t.shape), t) and not torch.equal(model[k], live[k]), (e, k)
        assert all(TF._same(model[k], live[k]) for k in live if k not in set(G))
    for f in ('final_model.pt', 'final_model_ema.pt'):
        a, b = TF._load(os.path.join(X, f)), TF._load(os.path.join(Y, f))
        assert list(a) == list(b) and all(TF._same(a[k], b[k]) for k in a), f
    for e in (1, 2):
        a, b = (TF._load(os.path.join(d, 'checkpoint', f'epoch_{e}.state', EMA_FILE)) for d in (X, Y))
        assert _same_ema(a, b), e


# ------------------------------------------------------------------------------------------------------------------ main.py
def _main(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py')] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _eval_table(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith('EVAL_JSON ')]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0][len('EVAL_JSON '):])


def test_main_train_with_ema_rate_then_eval_with_use_ema(tmp_path):
    from vpho_amd import evaluate as E
    from vpho_amd.trainer import Trainer
    out = str(tmp_path / 'out')
    stdout = _main(['--mode', 'train', '--model', 'vpho_net', '--max_epochs', '1', '--num_batches', '1', '--batch_size', '8', '--repeat_num', '4',
                    '--ema_rate', str(DECAY), '--mark', 'ema', '--output_dir', out])
    assert 'Epoch: 0/1' in stdout
    run = os.path.join(out, os.listdir(out)[0])
    assert set(os.listdir(run)) == {'checkpoint', 'final_model.pt', 'final_model_ema.pt'}
    ck = os.path.join(run, 'checkpoint', 'epoch_1.state')
    assert set(os.listdir(ck)) == FILES | {EMA_FILE} and TF._load(os.path.join(ck, EMA_FILE))['num_updates'] == 1
    small = ['--mode', 'eval', '--model', 'vpho_net', '--num_batches', '1', '--eval_batch_size', '8', '--checkpoint', ck]
    with_ema, without = _eval_table(_main(small + ['--use_ema'])), _eval_table(_main(small))
    assert with_ema['images'] == without['images'] == 8
    canon = lambda t: json.dumps(t, sort_keys=True)              # as text: a NaN cell equals itself
    assert canon(with_ema['table']) != canon(without['table'])
    # the same rows from a model that was handed final_model_ema.pt itself
    with TF._Cfg(checkpoint=os.path.join(run, 'final_model_ema.pt'), mode='eval', num_batches=1, eval_batch_size=8, use_ema=False) as cfg:
        rows = Trainer(cfg).eval()
    table = E.summarize(rows.cpu(), E.RowLayout.resolve(eval_best=None, eval_physics=None, physics_multi=None, eval_volume=None, volume_multi=None,
                                                          eval_hand_bench=None, hand_bench_multi=None))
    assert rows.shape[0] == 8 and canon(json.loads(json.dumps(table))) == canon(with_ema['table'])
    # --use_ema with the plain file: the error names the way out
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--mode', 'eval', '--model', 'vpho_net', '--num_batches', '1', '--eval_batch_size', '8',
                        '--checkpoint', os.path.join(run, 'final_model.pt'), '--use_ema'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and 'final_model_ema.pt' in r.stderr

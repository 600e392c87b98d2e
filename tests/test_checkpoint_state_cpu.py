"""Training state on disk (vpho_amd/checkpoint.py) without a GPU: accelerate reads what ``save_state`` writes and ``load_state`` reads what
accelerate writes; the three LR schedules equal torch's own schedulers stepped as the reference steps them; the parameter order
optimizer.bin is indexed by equals the reference's (tests/golden/golden_param_order.json); the new flags and the checkpoint-path parsing."""
import json
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'golden_param_order.json')
FILES = {'model.safetensors', 'optimizer.bin', 'scheduler.bin', 'random_states_0.pkl'}


class Tiny(torch.nn.Module):
    """one Conv2d, one BatchNorm2d, one Linear with a frozen bias"""
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv = torch.nn.Conv2d(3, 4, 3)
        self.bn = torch.nn.BatchNorm2d(4)
        self.fc = torch.nn.Linear(4, 2)
        with torch.no_grad():
            for t in list(self.parameters()) + [self.bn.running_mean, self.bn.running_var]:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
        self.fc.bias.requires_grad_(False)

    def forward(self, x):
        return self.fc(self.bn(self.conv(x)).mean((2, 3)))


def _fabricated_optimizer_state(model, seed, lr, step=3):
    from vpho_amd import checkpoint as CK
    g = torch.Generator().manual_seed(seed)
    params = list(model.named_parameters())
    state = {i: dict(step=torch.tensor(float(step)), exp_avg=torch.randn(p.shape, generator=g), exp_avg_sq=torch.rand(p.shape, generator=g))
             for i, (_, p) in enumerate(params) if p.requires_grad}
    groups = CK.param_groups('adamw', len(params), lr)
    return dict(state=state, param_groups=groups)


def _accelerator():
    from accelerate import Accelerator
    from accelerate.state import AcceleratorState, GradientState
    AcceleratorState._reset_state(True)
    GradientState._reset_state()
    return Accelerator(cpu=True)


def test_accelerate_reads_what_save_state_writes(tmp_path):
    from vpho_amd import checkpoint as CK
    ours = Tiny(1)
    sched = CK.make_scheduler('exp', 2e-4, world=1, gamma=0.96)
    for _ in range(3):
        sched.step_epoch()
    opt_state = _fabricated_optimizer_state(ours, 2, sched.lr)
    for g in opt_state['param_groups']:
        g.update(sched.group_extras())
    d = str(tmp_path / 'checkpoint' / 'epoch_3.state')
    CK.save_state(d, ours.state_dict(), opt_state, sched.state_dict(), rank=0, world=1, step=3)
    assert set(os.listdir(d)) == FILES

    theirs = Tiny(7)                                               # other weights, other statistics
    opt = torch.optim.AdamW(theirs.parameters(), betas=(0.9, 0.999), eps=1e-8, lr=2e-4)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, 0.96)
    accel = _accelerator()
    theirs, opt, sch = accel.prepare(theirs, opt, sch)
    accel.load_state(d)
    plist = list(theirs.parameters())
    for i, p in enumerate(plist):
        if not p.requires_grad:
            assert p not in opt.state and i not in opt_state['state']          # the frozen bias is counted and carries no state
            continue
        st = opt.state[p]
        assert float(st['step']) == 3.0
        assert torch.equal(st['exp_avg'], opt_state['state'][i]['exp_avg']) and torch.equal(st['exp_avg_sq'], opt_state['state'][i]['exp_avg_sq'])
    assert sum(1 for p in plist if not p.requires_grad) == 1
    assert opt.param_groups[0]['lr'] == sched.lr == pytest.approx(2e-4 * 0.96 ** 3, rel=1e-12)
    assert sch.get_last_lr() == [sched.lr]
    for k, v in ours.state_dict().items():
        assert torch.equal(theirs.state_dict()[k], v), k           # weights and BatchNorm buffers
    # and the next epoch continues the same schedule on both sides
    sch.step()
    sched.step_epoch()
    assert opt.param_groups[0]['lr'] == sched.lr


def test_load_state_reads_what_accelerate_writes(tmp_path):
    from vpho_amd import checkpoint as CK
    model = Tiny(3)
    opt = torch.optim.AdamW(model.parameters(), betas=(0.9, 0.999), eps=1e-8, lr=2e-4)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, 0.96)
    accel = _accelerator()
    model, opt, sch = accel.prepare(model, opt, sch)
    for _ in range(2):                                             # two real steps: moments, step counts, two scheduler steps
        model(torch.randn(5, 3, 6, 6)).sum().backward()
        opt.step()
        opt.zero_grad()
        sch.step()
    d = str(tmp_path / 'epoch_2.state')
    accel.save_state(d)
    assert set(os.listdir(d)) == FILES
    random.seed(99), np.random.seed(99), torch.manual_seed(99)
    expect = (random.random(), float(np.random.rand()), float(torch.rand(())))
    got = CK.load_state(d, rank=0)
    want_opt, want_model = opt.state_dict(), accel.unwrap_model(model).state_dict()
    assert set(got['model']) == set(want_model) and all(torch.equal(got['model'][k], want_model[k]) for k in want_model)
    assert set(got['optimizer']['state']) == set(want_opt['state']) == {0, 1, 2, 3, 4}          # five trained tensors, the frozen one (5) absent
    for i, st in want_opt['state'].items():
        for k in ('step', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(got['optimizer']['state'][i][k], st[k]), (i, k)
    assert got['optimizer']['param_groups'] == want_opt['param_groups']
    assert got['scheduler'] == sch.state_dict()
    # the generators are back where accelerate saved them, not where seed 99 left them
    after = (random.random(), float(np.random.rand()), float(torch.rand(())))
    assert after != expect
    CK.set_rng_state(got['rng'])
    assert after == (random.random(), float(np.random.rand()), float(torch.rand(())))
    # our scheduler continues theirs
    mine = CK.make_scheduler('exp', 2e-4)
    mine.load_state_dict(got['scheduler'])
    mine.load_group(got['optimizer']['param_groups'][0])
    assert mine.lr == opt.param_groups[0]['lr']
    mine.step_epoch(), sch.step()
    assert mine.lr == opt.param_groups[0]['lr']


def test_save_model_and_missing_state(tmp_path):
    from vpho_amd import checkpoint as CK
    m = Tiny(4)
    path = CK.save_model(str(tmp_path / 'run' / 'final_model.pt'), m.state_dict())
    sd = torch.load(path, map_location='cpu', weights_only=True)
    assert list(sd) == list(m.state_dict()) and all(torch.equal(sd[k], v) for k, v in m.state_dict().items())
    with pytest.raises(FileNotFoundError):
        CK.load_state(str(tmp_path / 'run'))                       # a directory without optimizer.bin is no training state
    assert not CK.is_training_state(path) and not CK.is_training_state('')


# ---------------------------------------------------------------------------------------------------------------------- schedules
EPOCHS, STEPS, BASE = 12, 7, 2e-4


def _torch_sequence(name, world, epochs=EPOCHS):
    """torch's own scheduler on a real optimiser, stepped as the reference runs it: world steps at the end of every epoch (accelerate's
    prepared scheduler), the OneCycleLR too (train_diff_hand_obj.py:198-199) -- lr in force during each epoch"""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=BASE)
    S = torch.optim.lr_scheduler
    if name == 'exp':
        sch = S.ExponentialLR(opt, 0.96 ** (1 / world))
    elif name == 'step':
        sch = S.StepLR(opt, step_size=5, gamma=0.96 ** (1 / world))
    else:
        sch = S.OneCycleLR(optimizer=opt, max_lr=BASE, epochs=EPOCHS, steps_per_epoch=STEPS, pct_start=0.1, anneal_strategy='cos')
    lrs, betas = [], []
    for _ in range(epochs):
        lrs.append(opt.param_groups[0]['lr'])
        betas.append(opt.param_groups[0]['betas'][0])
        opt.step()
        for _ in range(world):
            sch.step()
    return lrs, betas


@pytest.mark.parametrize('world', [1, 4])
@pytest.mark.parametrize('name', ['exp', 'step', 'cosine'])
def test_lr_sequences_equal_torch_schedulers_and_survive_a_reload(name, world):
    from vpho_amd import checkpoint as CK
    make = lambda: CK.make_scheduler(name, BASE, world=world, gamma=0.96, lr_step=5, max_epochs=EPOCHS, steps_per_epoch=STEPS)
    want, want_b = _torch_sequence(name, world)
    s = make()
    got, got_b, saved = [], [], None
    for e in range(EPOCHS):
        if e == 5:
            saved = (s.state_dict(), s.lr, s.beta1)
        got.append(s.lr)
        got_b.append(s.beta1)
        s.step_epoch()
    assert got == want and got_b == want_b
    if name == 'exp':
        assert got[3] == pytest.approx(BASE * 0.96 ** 3, rel=1e-12)                         # gamma per epoch at any world size
    if name == 'step':                                                                    # the kept quirk: world 4 decays 4x as often, by gamma ** (1/4)
        first = next(e for e in range(EPOCHS) if got[e] != BASE)
        assert first == (5 if world == 1 else 2)
    if name == 'cosine':
        assert got[0] == pytest.approx(BASE / 25) and max(got) < BASE                     # 12 * world of 84 per-batch steps: still warming up
        assert got_b[0] == pytest.approx(0.95) and got_b[-1] < got_b[0]                   # OneCycleLR cycles beta1 as well
    r = make()
    state = torch.load(_roundtrip(saved[0]), weights_only=False)
    r.load_state_dict(state)
    r.load_group(dict(lr=saved[1], betas=(saved[2], 0.999)))
    cont, cont_b = [], []
    for e in range(5, EPOCHS):
        cont.append(r.lr)
        cont_b.append(r.beta1)
        r.step_epoch()
    assert cont == want[5:] and cont_b == want_b[5:]


def _roundtrip(state):
    import io
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    return buf


# ---------------------------------------------------------------------------------------------------------------------- order, flags
def test_parameter_order_equals_the_reference(model_cpu):
    G = json.load(open(GOLD))
    ours = [dict(name=k, shape=list(p.shape), requires_grad=bool(p.requires_grad)) for k, p in model_cpu.named_parameters()]
    assert ours == G['params'] and len(ours) == 569
    # the state_dict order with the buffers taken out -- what DiffusionTrainStep indexes optimizer.bin by -- is that order
    params = {k for k, _ in model_cpu.named_parameters()}
    assert [k for k in model_cpu.state_dict() if k in params] == [p['name'] for p in G['params']]
    from vpho_amd import checkpoint as CK
    for kind in ('adamw', 'adam'):
        want = G['param_groups'][kind]
        got = CK.param_groups(kind, len(ours), 2e-4)
        assert len(got) == len(want) == 1 and got[0]['params'] == want[0]['params'] == list(range(569))
        for k in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize'):
            assert list(got[0][k]) == want[0][k] if k == 'betas' else got[0][k] == want[0][k], (kind, k)
        assert set(got[0]) == set(want[0]) or G['torch'] != torch.__version__.split('+')[0]
    assert G['param_groups']['adam'][0]['weight_decay'] == CK.ADAM_L2 and G['param_groups']['adamw'][0]['weight_decay'] == 0.01


def test_new_flags_defaults_choices_and_entry():
    from vpho_amd.configs import args as A
    from vpho_amd.trainer import train_entry
    G = json.load(open(GOLD))['flags']
    p = A._parser()
    d = p.parse_args([])
    for k in ('optimizer', 'scheduler', 'gamma', 'lr_step', 'gradient_accumulation_steps', 'print_freq'):
        assert getattr(d, k) == G[k] == getattr(A.Config(), k), k
    assert (d.optimizer, d.scheduler, d.gamma, d.lr_step, d.gradient_accumulation_steps, d.print_freq) == ('adamw', 'exp', 0.96, 5, 1, 500)
    assert d.max_epochs is None and A.Config().max_epochs is None and G['max_epochs'] == 100         # here: absent = one pass of run
    assert train_entry(d) == 'run' and train_entry(p.parse_args(['--max_epochs', '3'])) == 'fit'
    choices = {a.dest: a.choices for a in p._actions}
    assert choices['optimizer'] == ['adamw', 'adam'] and choices['scheduler'] == ['exp', 'cosine', 'step']
    for bad in (['--optimizer', 'sgd'], ['--scheduler', 'linear']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    full = p.parse_args(['--max_epochs', '2', '--optimizer', 'adam', '--scheduler', 'step', '--gamma', '0.5', '--lr_step', '3',
                         '--gradient_accumulation_steps', '4', '--print_freq', '10'])
    assert (full.max_epochs, full.optimizer, full.scheduler, full.gamma, full.lr_step, full.gradient_accumulation_steps, full.print_freq) == \
        (2, 'adam', 'step', 0.5, 3, 4, 10)


def test_epoch_is_parsed_from_the_checkpoint_path():
    from vpho_amd import checkpoint as CK
    assert CK.epoch_of('') == 0
    assert CK.epoch_of('output/20240101_000000__train_vpho_net/checkpoint/epoch_45.state') == 45
    assert CK.epoch_of('/abs/checkpoint/epoch_7.state/') == 7
    assert CK.epoch_of('epoch_12.state') == 12
    with pytest.raises(ValueError):
        CK.epoch_of('output/run/final_model.pt')                   # the reference's int() fails the same way


def test_optimizer_names():
    from vpho_amd import checkpoint as CK
    assert CK.optimizer_hyper('adamw', 1e-3)['weight_decay'] == 0.01 and CK.optimizer_hyper('adam', 1e-3)['weight_decay'] == 0.0005
    assert CK.optimizer_hyper('adam', 1e-3, weight_decay=0.0)['weight_decay'] == 0.0
    with pytest.raises(ValueError):
        CK.optimizer_hyper('sgd', 1e-3)
    with pytest.raises(ValueError):
        CK.make_scheduler('linear', 1e-3)

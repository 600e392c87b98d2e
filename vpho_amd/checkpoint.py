"""Training state on disk in the reference's own format: the directory ``accel.save_state`` writes after every epoch
(lib/engine/base_trainer.py:81-96) -- ``model.safetensors``, ``optimizer.bin`` (``torch.optim.AdamW/Adam.state_dict()``),
``scheduler.bin`` (the torch scheduler's ``state_dict()``), ``random_states_<rank>.pkl`` -- and ``final_model.pt``.  A run started here
can be continued by the reference (``accel.load_state``) and the other way round.  Pure host code: no GPU, no HIP
library; the CUDA generator states are saved and restored only where a GPU is present.

The schedulers are torch's own objects on a one-parameter dummy optimiser (``make_scheduler``), stepped as the reference steps them
*as it runs* (``step_epoch``): accelerate's prepared scheduler steps ``world`` times per call, and train_diff_hand_obj.py:198-199 compares
the scheduler OBJECT with the string 'cosine', so every scheduler -- the per-batch OneCycleLR included -- is stepped once per epoch.
"""
import os
import random

import numpy as np
import torch

MODEL_FILE, OPTIMIZER_FILE, SCHEDULER_FILE = 'model.safetensors', 'optimizer.bin', 'scheduler.bin'
SCHEDULERS = ('exp', 'cosine', 'step')
OPTIMIZERS = ('adamw', 'adam')
ADAM_L2 = 0.0005                      # train_diff_hand_obj.py:54; AdamW keeps torch's default decay of 0.01 (:52)


def rng_file(rank):
    return f'random_states_{rank}.pkl'


def epoch_of(checkpoint):
    """the epoch a ``--checkpoint .../epoch_N.state`` resumes at, parsed as base_trainer.py:26-29 parses it; '' -> 0"""
    if not checkpoint:
        return 0
    return int(str(checkpoint).rstrip('/').split('/')[-1].split('.')[0].split('epoch_')[-1])


def is_training_state(path):
    """a directory of ``accel.save_state`` that can be resumed (it holds the optimiser), not just a model file"""
    return bool(path) and os.path.isdir(path) and os.path.exists(os.path.join(path, OPTIMIZER_FILE))


# ---------------------------------------------------------------------------------------------------------------------- optimiser
def optimizer_hyper(kind, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=None):
    """the optimiser the reference builds for ``--optimizer kind`` (train_diff_hand_obj.py:49-54)"""
    if kind not in OPTIMIZERS:
        raise ValueError(f"Invalid optimizer name: {kind} (one of {OPTIMIZERS})")
    return dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=(0.01 if kind == 'adamw' else ADAM_L2) if weight_decay is None else weight_decay)


def param_groups(kind, n_params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=None):
    """``state_dict()['param_groups']`` of torch.optim.AdamW / Adam over n_params parameters: torch's own keys, whatever its version"""
    dummy = [torch.nn.Parameter(torch.zeros(())) for _ in range(n_params)]
    cls = torch.optim.AdamW if kind == 'adamw' else torch.optim.Adam
    return cls(dummy, **optimizer_hyper(kind, lr, betas, eps, weight_decay)).state_dict()['param_groups']


# ---------------------------------------------------------------------------------------------------------------------- schedulers
class Schedule:
    """A torch LR scheduler on a one-parameter dummy optimiser.  ``lr`` (and ``beta1``: OneCycleLR cycles the momentum of an Adam
    optimiser between 0.85 and 0.95 by default, which the reference leaves on) is what the next optimiser step uses, ``step_epoch()``
    what the reference's loop does at the end of an epoch, ``state_dict()`` is ``scheduler.bin``."""
    def __init__(self, name, base_lr, world=1, gamma=0.96, lr_step=5, max_epochs=None, steps_per_epoch=None, betas=(0.9, 0.999)):
        if name not in SCHEDULERS:
            raise ValueError(f"Invalid scheduler name: {name} (one of {SCHEDULERS})")
        self.name, self.world = name, int(world)
        self.opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(()))], lr=base_lr, betas=tuple(betas))
        S = torch.optim.lr_scheduler
        if name == 'exp':                                  # gamma ** (1 / world), stepped world times: gamma per epoch
            self.sched = S.ExponentialLR(self.opt, gamma ** (1 / self.world))
        elif name == 'step':                               # world > 1: decays every lr_step / world epochs by gamma ** (1 / world) (kept quirk)
            self.sched = S.StepLR(self.opt, step_size=lr_step, gamma=gamma ** (1 / self.world))
        else:                                              # a per-batch schedule stepped once per epoch (kept quirk)
            if not max_epochs or not steps_per_epoch:
                raise ValueError('--scheduler cosine needs max_epochs and steps_per_epoch (OneCycleLR)')
            self.sched = S.OneCycleLR(optimizer=self.opt, max_lr=base_lr, epochs=max_epochs, steps_per_epoch=steps_per_epoch, pct_start=0.1,
                                      anneal_strategy='cos')

    @property
    def lr(self):
        return float(self.opt.param_groups[0]['lr'])

    @property
    def beta1(self):
        return float(self.opt.param_groups[0]['betas'][0])

    def group_extras(self):
        """the keys the scheduler keeps in the optimiser's param_group (initial_lr; OneCycleLR: max_lr, min_lr, base / max_momentum)"""
        g = self.opt.param_groups[0]
        return {k: g[k] for k in ('initial_lr', 'max_lr', 'min_lr', 'base_momentum', 'max_momentum') if k in g}

    def step_epoch(self):
        self.opt._opt_called = True                        # the dummy optimiser never steps: no "scheduler before optimizer" warning
        for _ in range(self.world):                        # accelerate's AcceleratedScheduler.step (split_batches=False)
            if self.name == 'cosine' and self.sched._step_count > self.sched.total_steps:
                break                                      # ... which stops a OneCycleLR at its total_steps instead of raising
            self.sched.step()

    def state_dict(self):
        return self.sched.state_dict()

    def load_state_dict(self, state):
        self.sched.load_state_dict(state)
        lrs = state.get('_last_lr')
        if lrs:                                            # the scheduler's state does not hold the optimiser's lr: it lives in optimizer.bin
            self.opt.param_groups[0]['lr'] = float(lrs[0])

    def load_group(self, group):
        """lr and betas of the optimiser's param_group as optimizer.bin holds them (a OneCycleLR has moved beta1)"""
        self.opt.param_groups[0]['lr'] = float(group['lr'])
        self.opt.param_groups[0]['betas'] = tuple(float(b) for b in group['betas'])


def make_scheduler(name, base_lr, world=1, gamma=0.96, lr_step=5, max_epochs=None, steps_per_epoch=None, betas=(0.9, 0.999)):
    return Schedule(name, base_lr, world, gamma, lr_step, max_epochs, steps_per_epoch, betas)


# ---------------------------------------------------------------------------------------------------------------------- files
def _world():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def _barrier():
    if _world():
        import torch.distributed as dist
        dist.barrier()


def rng_state(step=0):
    """what accelerate puts into random_states_<rank>.pkl (checkpointing.py: save_accelerator_state)"""
    states = dict(step=int(step), random_state=random.getstate(), numpy_random_seed=np.random.get_state(), torch_manual_seed=torch.get_rng_state())
    if torch.cuda.is_available():
        states['torch_cuda_manual_seed'] = torch.cuda.get_rng_state_all()
    return states


def set_rng_state(states):
    random.setstate(states['random_state'])
    np.random.set_state(states['numpy_random_seed'])
    torch.set_rng_state(states['torch_manual_seed'])
    if 'torch_cuda_manual_seed' in states and torch.cuda.is_available():
        cuda = states['torch_cuda_manual_seed']
        if len(cuda) == torch.cuda.device_count():
            torch.cuda.set_rng_state_all(cuda)
        else:                                              # written on a machine with another number of visible devices
            torch.cuda.set_rng_state(cuda[min(torch.cuda.current_device(), len(cuda) - 1)])


def _cpu(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu().contiguous()
    if isinstance(obj, dict):
        return {k: _cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_cpu(v) for v in obj)
    return obj


def custom_file(index):
    """accelerate's file of the index-th object passed to ``register_for_checkpointing`` (checkpointing.py: save_custom_state)"""
    return f'custom_checkpoint_{index}.pkl'


def save_state(dir, model_state_dict, optimizer_state, scheduler_state, rank=0, world=1, step=0, *, custom=None):
    """``accel.save_state(dir)``: rank 0 writes the three shared files, every rank its RNG file, then a barrier.  ``custom``: the
    ``state_dict()`` of every object registered for checkpointing, in order (the weights' moving average, vpho_amd/ema.py): rank 0 writes
    ``custom_checkpoint_<i>.pkl`` as ``save_custom_state`` does; None or empty: no such file"""
    os.makedirs(dir, exist_ok=True)
    if rank == 0:
        from safetensors.torch import save_file
        save_file({k: v.clone() for k, v in _cpu(model_state_dict).items()}, os.path.join(dir, MODEL_FILE), metadata={'format': 'pt'})
        torch.save(_cpu(optimizer_state), os.path.join(dir, OPTIMIZER_FILE))
        torch.save(_cpu(scheduler_state), os.path.join(dir, SCHEDULER_FILE))
        for i, state in enumerate(custom or ()):
            torch.save(_cpu(state), os.path.join(dir, custom_file(i)))
    torch.save(rng_state(step), os.path.join(dir, rng_file(rank)))
    _barrier()
    return dir


def load_state(dir, rank=0, restore_rng=True):
    """-> dict(model=state_dict, optimizer=..., scheduler=..., rng=..., step=..., custom=[...]) of a directory written by ``save_state``
    or by ``accel.save_state``; the process's generators are set from the rank's RNG file (a missing one is tolerated, as accelerate
    does); ``custom``: the content of ``custom_checkpoint_0.pkl``, ``_1`` ... (an empty list when the directory has none)"""
    if not is_training_state(dir):
        raise FileNotFoundError(f'{dir} is no training state: it needs {OPTIMIZER_FILE} (an accel.save_state directory, <save_dir>/checkpoint/epoch_N.state)')
    from safetensors.torch import load_file
    model_path = os.path.join(dir, MODEL_FILE)
    if os.path.exists(model_path):
        model = load_file(model_path)
    else:                                                  # accelerate with safe_serialization=False
        model = torch.load(os.path.join(dir, 'pytorch_model.bin'), map_location='cpu', weights_only=True)
    out = dict(model={(k[len('module.'):] if k.startswith('module.') else k): v for k, v in model.items()},
               optimizer=torch.load(os.path.join(dir, OPTIMIZER_FILE), map_location='cpu', weights_only=True),
               scheduler=torch.load(os.path.join(dir, SCHEDULER_FILE), map_location='cpu', weights_only=False), rng=None, step=0, custom=[])
    while os.path.exists(os.path.join(dir, custom_file(len(out['custom'])))):     # registered objects, as load_custom_state reads them
        out['custom'].append(torch.load(os.path.join(dir, custom_file(len(out['custom']))), map_location='cpu', weights_only=False))
    rng = os.path.join(dir, rng_file(rank))
    if os.path.exists(rng):
        out['rng'] = torch.load(rng, map_location='cpu', weights_only=False)      # python / numpy generator states: plain pickled tuples
        out['step'] = int(out['rng'].get('step', 0))
        if restore_rng:
            set_rng_state(out['rng'])
    _barrier()
    return out


def save_model(path, state_dict, rank=0):
    """``final_model.pt`` (base_trainer.py:91-96): the plain state_dict, written by rank 0"""
    if rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(_cpu(state_dict), path)
    _barrier()
    return path

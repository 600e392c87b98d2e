"""Exponential moving average of the trained weights: the host side of the reference's ``ExponentialMovingAverage``
(lib/model/ema.py:3-92, the class of score_sde_pytorch that VPHO.py:20 imports).  The arithmetic runs on the device
(``ops.EmaList``, one launch over every tensor of ``DiffusionTrainStep``); this object keeps what the class keeps beside its shadows --
``decay`` and ``num_updates`` -- forms the step's ``one_minus_decay`` in Python double as ``update()`` does (:36-40) and holds the
shadows of a ``state_dict()`` in the reference's layout: ``dict(decay, num_updates, shadow_params=[one CPU fp32 tensor per trainable
parameter, in the order of vpho_net(...).named_parameters(), in the reference's shapes])``.  Pure host code."""
import torch

STATE_KEYS = ('decay', 'num_updates', 'shadow_params')
CUSTOM_INDEX = 0                      # the EMA is the one object registered for checkpointing: custom_checkpoint_0.pkl


class WeightEma:
    def __init__(self, decay, use_num_updates=True):
        if decay < 0.0 or decay > 1.0:
            raise ValueError('Decay must be between 0 and 1')
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        self.shadow_params = []

    def next_one_minus_decay(self):
        """advance ``num_updates`` and return ``1.0 - decay`` of this update (ema.py:36-40); ``num_updates`` None: the fixed decay"""
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = min(decay, (1 + self.num_updates) / (10 + self.num_updates))
        return 1.0 - decay

    def state_dict(self):
        return dict(decay=self.decay, num_updates=self.num_updates, shadow_params=self.shadow_params)

    def load_state_dict(self, state_dict):
        missing = [k for k in STATE_KEYS if k not in state_dict]
        if missing:
            raise KeyError(f'EMA state lacks {missing} (the keys of ExponentialMovingAverage.state_dict(): {STATE_KEYS})')
        self.decay = state_dict['decay']
        self.num_updates = state_dict['num_updates']
        self.shadow_params = [t.detach().to('cpu', torch.float32).contiguous() for t in state_dict['shadow_params']]


def overlay(state_dict, ema_state, param_names):
    """``state_dict`` with its trained tensors replaced by the shadows of ``ema_state`` (what ``copy_to`` does, ema.py:47-58):
    shadow i belongs to ``param_names[i]``; buffers (running statistics) stay as they are"""
    shadows = ema_state['shadow_params']
    if len(shadows) != len(param_names):
        raise ValueError(f'EMA state of {len(shadows)} tensors, the model has {len(param_names)} trainable parameters')
    out = dict(state_dict)
    for k, s in zip(param_names, shadows):
        if k not in out:
            raise KeyError(f'the checkpoint has no tensor {k} to put its average into')
        if s.numel() != out[k].numel():
            raise ValueError(f'EMA shadow of {k}: {tuple(s.shape)}, the parameter is {tuple(out[k].shape)}')
        out[k] = s.detach().to(out[k].dtype).reshape(out[k].shape)
    return out

"""Float64 restatements of the optimiser tail (csrc/optim.hip), in the style of tests/_leaf_fp64.py: written from torch's own definitions
(``torch.nn.utils.clip_grad_norm_``, ``torch.optim.Adam / AdamW``), computing in the dtype of their tensor arguments so that
``_leaf_fp64.ruled`` gives the float64 reference and the rule-based bound from one definition.  TEST INFRASTRUCTURE ONLY: nothing here
imports ``vpho_amd.ops``."""
import math

import numpy as np
import torch

from _leaf_fp64 import f32r


def sqnorm_fsum(flat):
    """sum of squares of a float32 tensor, exactly rounded: a float32 squared is exact in float64, math.fsum adds without error"""
    a = flat.detach().cpu().double().reshape(-1).numpy()
    return math.fsum((a * a).tolist())


def clip_coef(sqnorm, max_norm, grad_scale=1.0):
    """torch.nn.utils.clip_grad_norm_ on the averaged gradient (g * grad_scale): min(1, max_norm / (total_norm + 1e-6)) in float64, rounded
    once to float32 -- the kernel's rule.  max_norm and grad_scale are the float32 values the kernel receives.  A NaN norm gives NaN
    (torch.clamp keeps it), an infinite one 0."""
    norm = f32r(grad_scale) * math.sqrt(sqnorm) if sqnorm == sqnorm else float('nan')
    c = f32r(max_norm) / (norm + 1e-6)
    return float(np.float32(1.0 if c > 1.0 else c))


def optim(param, grad, m, v, step, kind='adamw', lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, coef=None):
    """one torch.optim.AdamW (kind 'adamw') / torch.optim.Adam with L2 decay (kind 'adam') update at step `step`, resumed from the saved
    moments, on the gradient (grad * grad_scale) * coef, in the dtype of `param`; hyper-parameters as the float32 values the kernel
    receives.  -> new (param, exp_avg, exp_avg_sq)"""
    p = param.detach().clone().requires_grad_(True)
    cls = torch.optim.AdamW if kind == 'adamw' else torch.optim.Adam
    opt = cls([p], lr=f32r(lr), betas=(f32r(beta1), f32r(beta2)), eps=f32r(eps), weight_decay=f32r(weight_decay), foreach=False)
    g = grad.detach().clone() * f32r(grad_scale)
    p.grad = g if coef is None else g * coef
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.detach().clone(), exp_avg_sq=v.detach().clone())
    opt.step()
    st = opt.state[p]
    return p.detach(), st['exp_avg'], st['exp_avg_sq']

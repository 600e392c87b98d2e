"""float64 reference of the pseudo-force optimisation (csrc/force_optim.hip) and the cases its tests run.  No GPU.

* ``reference`` runs ``oracle.force_optim.optimize`` on ONE batch with float64 inputs, float64 anchor tables and float64 as the default
  dtype (restored in a ``finally``), or the same call in float32.  ``reference_batches`` loops over the batches of a launch (the batch
  mean couples the samples of a batch, nothing couples two batches) and stacks: ``losses`` come back as (n_batches, 4).
* ``noise`` is the largest absolute difference, per output, between the float32 and the float64 run of the same inputs: the
  reference's own arithmetic noise.  Every tolerance of the GPU tests is ``k * max(noise, floor)`` (``units``), ``floor`` a few float32
  ulps of the output's magnitude; ``ratios`` takes both from each batch's own run.
* ``manual_loop`` is a copy of the loop with a hand-written AdamW, equal to the oracle when not mutated (tests/test_force_fp64_cpu.py
  holds that).  Its mutations restate, on the reference, what a wrong kernel would do: they size what a test can see, they are never
  the reference of a GPU test.
* ``inputs`` is the recipe of tests/test_gpu_force_optim.py; ``degenerate_inputs`` overwrites rows with the contact patterns at which the
  kernel's guards and its ``> 0.1`` mask decide.

The float32 program compares ``force_contact > 0.1`` in float32, i.e. against float32(0.1) = 0.100000001490116; a float64 run of the
same text compares against the double 0.1 and would call float32(0.1) itself a contact.  The float64 run therefore receives the double
0.1 where an input equals float32(0.1) exactly (a change of 1.5e-9 in that value, far below every floor): the mask is then the float32
program's mask for every float32 input."""
import functools

import numpy as np
import torch

OUTPUTS = ('scale', 'weight', 'force_local', 'force_global', 'loss_force', 'loss_gravity', 'loss_moment', 'loss_dist')
EPS32 = float(np.finfo(np.float32).eps)
FLOOR_ULPS = 4.0                                   # floor = 4 float32 ulps of the output's largest magnitude
WD = 0.01                                          # torch.optim.AdamW default

# (B, n_batches, iters, phase1): the workgroup shapes -- all 1024 threads valid, one row of 16 lanes idle, B % 4 != 0 with several
# batches in flight, exactly one float4 of the batch-mean read, a single sample
SHAPES = ((64, 2, 120, 40), (63, 1, 60, 20), (17, 3, 120, 40), (4, 2, 120, 40), (1, 4, 120, 40))
# (iters, phase1): report before the first update in either phase, report in the iteration that zeroes the moments, phase 2 never
# entered, phase 1 never entered
PHASE_EDGES = ((1, 0), (1, 1), (2, 1), (40, 39), (40, 40), (40, 1000), (120, 0))
PHASE_B = (5, 17)
# (iters, phase1, lr) at B = 5: table slot 1023 last, slot 0 of the second table, a phase switch before / inside the second table run,
# a switch at the refill itself, two refills.  lr is small: at 1e-3 an fp32 Adam trajectory of 1100 steps is chaotic (1.5e-2 in weight)
TABLE = ((1024, 300, 1e-5), (1025, 300, 1e-5), (1100, 300, 1e-5), (1100, 1030, 1e-5), (2100, 1024, 1e-5), (2100, 1000, 1e-6))
TABLE_B = 5
SEED = 1                                           # every case draws its inputs with this seed
# the launches the VPHO_FORCE_EXACT=1 child repeats: name -> (kind, B, n_batches, iters, phase1, lr)
EXACT_CASES = {'b64': ('plain', 64, 2, 120, 40, 1e-3), 'deg17': ('degenerate', 17, 3, 120, 40, 1e-3), 'tab1030': ('plain', 5, 1, 1100, 1030, 1e-5)}


def _assets():
    from vpho_amd.assets import synthetic_assets
    return synthetic_assets(0)


def inputs(assets, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    v = torch.as_tensor(assets['mano']['v_template'])[None] + torch.randn(B, 778, 3, generator=g) * 0.002 + torch.tensor([0.0, 0.0, 0.7])
    grav = torch.nn.functional.normalize(torch.randn(B, 1, 3, generator=g), dim=-1)
    com = torch.tensor([0.05, 0.0, 0.7]) + torch.randn(B, 1, 3, generator=g) * 0.02
    fc = torch.rand(B, 32, generator=g)
    grasped = torch.rand(B, generator=g) < 0.8
    return v.contiguous(), grav.contiguous(), com.contiguous(), fc.contiguous(), grasped


PATTERNS = ('all_zero', 'all_below', 'one_above', 'threshold', 'all_equal', 'one_huge', 'all_zero_no_gravity')


def _pattern(name, fc_row, grav_row, g):
    """overwrite one sample's force_contact (32,) and gravity (1,3) in place"""
    t = np.float32(0.1)
    if name == 'all_zero':                                         # (a) fnorm + 1e-8 is the whole denominator; no contact anchor
        fc_row.zero_()
    elif name == 'all_below':                                      # (b) every value in (0, 0.1): no contact anchor, fnorm > 0
        fc_row.copy_(torch.rand(32, generator=g) * 0.098 + 0.001)
    elif name == 'one_above':                                      # (c) exactly one contact anchor
        fc_row.copy_(torch.rand(32, generator=g) * 0.098 + 0.001)
        fc_row[int(torch.randint(32, (1,), generator=g))] = 0.6
    elif name == 'threshold':                                      # (d) float32(0.1) and its two neighbours, side by side, in both halves of a lane pair
        for k in (3, 19):
            fc_row[k], fc_row[k + 1], fc_row[k + 2] = float(t), float(np.nextafter(t, np.float32(1))), float(np.nextafter(t, np.float32(0)))
    elif name == 'all_equal':                                      # (e) all 32 anchors in contact with one value
        fc_row.fill_(0.5)
    elif name == 'one_huge':                                       # (f) one very large value among ordinary ones
        fc_row[int(torch.randint(32, (1,), generator=g))] = 1e3
    elif name == 'all_zero_no_gravity':                            # no contact anchor and no gravity: resultant exactly 0 (the `rn > 0` guard)
        fc_row.zero_()
        grav_row.zero_()
    else:
        raise KeyError(name)


def degenerate_inputs(assets, B, n_batches=1, seed=0):
    """``inputs`` for n_batches * B samples with the PATTERNS written over rows k % B of every batch (rotated by the batch index, so that
    a small B meets every pattern in some batch); is_grasped all true in even batches, all false in odd ones."""
    v, grav, com, fc, grasped = inputs(assets, B * n_batches, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    for i in range(n_batches):
        for k in range(len(PATTERNS)):
            row = i * B + k % B
            _pattern(PATTERNS[(k + i) % len(PATTERNS)], fc[row], grav[row], g)
        grasped[i * B:(i + 1) * B] = (i % 2 == 0)
    return v, grav, com, fc, grasped


def build(kind, B, n_batches, seed):
    a = _assets()
    return inputs(a, B * n_batches, seed) if kind == 'plain' else degenerate_inputs(a, B, n_batches, seed)


def _cast(ins, dtype):
    v, grav, com, fc, grasped = ins
    if dtype == torch.float32:
        return v, grav, com, fc, grasped
    fc64 = fc.double()
    fc64[fc == float(np.float32(0.1))] = 0.1                       # see the module docstring: the float32 program's mask
    return v.double(), grav.double(), com.double(), fc64, grasped


def _pack(r):
    out = {k: r[k].detach().double().numpy() for k in ('scale', 'weight', 'force_local', 'force_global')}
    for k, name in enumerate(('loss_force', 'loss_gravity', 'loss_moment', 'loss_dist')):
        out[name] = np.array([r['losses'][k]], np.float64)
    out['force_point'] = r['force_point'].detach().double().numpy()
    out['frames'] = r['frames'].detach().double().numpy()
    return out


def reference(ins, iters, phase1, lr, dtype=torch.float64):
    """one batch through oracle.force_optim.optimize in ``dtype``; every output as a float64 array"""
    from oracle import force_optim as FO
    from oracle.aggregation import vert2anchor
    from vpho_amd.assets import ANCHOR_SKELETON
    a = _assets()
    v, grav, com, fc, grasped = _cast(ins, dtype)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        r = FO.optimize(a['anchor'], ANCHOR_SKELETON, v, grav, com, fc, grasped, iters=iters, phase1=phase1, lr=lr)
        r['frames'] = vert2anchor(a['anchor'], ANCHOR_SKELETON, v)[1]
    finally:
        torch.set_default_dtype(old)
    assert r['scale'].dtype == dtype and r['force_global'].dtype == dtype
    return _pack(r)


def _stack(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def reference_batches(ins, B, iters, phase1, lr, dtype=torch.float64):
    n = ins[0].shape[0]
    assert n % B == 0
    return _stack([reference(tuple(t[i:i + B] for t in ins), iters, phase1, lr, dtype) for i in range(0, n, B)])


@functools.lru_cache(maxsize=None)
def case(kind, B, n_batches, iters, phase1, lr, seed):
    """(inputs, float64 reference, float32 run of the reference) of one launch, computed once per process"""
    ins = build(kind, B, n_batches, seed)
    return ins, reference_batches(ins, B, iters, phase1, lr, torch.float64), reference_batches(ins, B, iters, phase1, lr, torch.float32)


def max_abs(a, b):
    return {k: float(np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)).max()) for k in OUTPUTS}


def noise(ref64, ref32):
    return max_abs(ref32, ref64)


def floor(ref64):
    return {k: FLOOR_ULPS * EPS32 * float(np.abs(ref64[k]).max()) for k in OUTPUTS}


def units(ref64, ref32):
    """max(noise, floor) per output: the unit every bound is a multiple of"""
    n, f = noise(ref64, ref32), floor(ref64)
    return {k: max(n[k], f[k]) for k in OUTPUTS}


def _batch(d, i, n_batches):
    return {k: np.asarray(d[k]).reshape((n_batches, -1) + np.asarray(d[k]).shape[1:])[i] for k in OUTPUTS}


def ratios(got, ref64, ref32):
    """error / max(noise, floor) per output, the largest over the batches of the launch.  Noise and floor are each batch's own: the
    reference runs one batch at a time, and one ill-conditioned sample (a scale driven through zero, where |scale| has its kink and the
    contact distance its pole) then loosens the bounds of its own batch only."""
    n_batches = len(ref64['loss_force'])
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for i in range(n_batches):
        g, r64, r32 = (_batch(d, i, n_batches) for d in (got, ref64, ref32))
        e, u = max_abs(g, r64), units(r64, r32)
        for k in OUTPUTS:
            worst[k] = max(worst[k], e[k] / u[k] if u[k] > 0 else (0.0 if e[k] == 0 else float('inf')))
    return worst


def masked_scale(iters, phase1, lr):
    """scale of an anchor out of contact: no gradient ever, so only the second optimiser's weight decay, once per phase-2 step"""
    return 0.05 * (1.0 - lr * WD) ** max(0, iters - phase1)


def contact_mask(fc):
    return fc > 0.1                                                 # float32 tensor against a Python scalar: compared in float32


# --------------------------------------------------------------------------------------- the loop by hand, and what a wrong kernel would do
MUTATIONS = ('no_restart', 'no_reset', 'stale_table')


def manual_loop(ins, iters, phase1, lr, dtype=torch.float64, mutation=None, table=1024):
    """oracle.force_optim.optimize on one batch with AdamW written out (torch/optim/adamw.py, single tensor, not amsgrad).
    mutation: 'no_restart' = the step count of the bias corrections runs on through the phase switch; 'no_reset' = the moments of
    `weight` survive the switch; 'stale_table' = from iteration `table` on, the bias corrections of iteration it - table."""
    from oracle import force_optim as FO
    from oracle.aggregation import vert2anchor
    from vpho_amd.assets import ANCHOR_SKELETON
    import torch.nn.functional as F
    assert mutation is None or mutation in MUTATIONS
    a = _assets()
    vert, gravity, com, force_contact, grasped = _cast(ins, dtype)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        B = vert.shape[0]
        scale_p = (torch.ones(B, 32) * 0.05).requires_grad_()
        weight_p = torch.zeros(B, 32, 8).requires_grad_()
        mom = {id(p): [torch.zeros_like(p), torch.zeros_like(p)] for p in (scale_p, weight_p)}
        mask = force_contact > 0.1
        pts, frame = vert2anchor(a['anchor'], ANCHOR_SKELETON, vert)
        b1, b2, eps = 0.9, 0.999, 1e-8
        losses = None
        for i in range(iters):
            scale = scale_p.clone() * mask
            fl = FO.get_local_force(scale, weight_p.clone())
            fg = torch.einsum('...bi,...bji->...bj', fl, frame)
            res = (fg.sum(1, keepdim=True) + gravity).squeeze(1)
            force_loss = torch.norm(res, dim=-1).mean()
            sw = force_loss.detach()
            cos = torch.einsum('...i,...i->...', fg.sum(1, keepdim=True), -1 * gravity)
            gravity_loss = F.mse_loss(cos, torch.ones_like(cos))
            moment = torch.cross(pts - com, fg, dim=-1).sum(1)
            moment_loss = torch.norm(moment, dim=-1).mean() * 30 / (100 * sw ** 2 + 1e-8)
            scale_norm = scale / (scale.norm(dim=-1, keepdim=True).detach() + 1e-8).detach()
            fc_norm = force_contact / (force_contact.norm(dim=-1, keepdim=True).detach() + 1e-8)
            dist = torch.log(torch.abs(fc_norm / (scale_norm + 1e-8)) + 1e-8) * mask
            dist_loss = (dist ** 2).mean() * 0.1 / (1000 * sw ** 2 + 1e-8)
            ph2 = i >= phase1
            params = [scale_p, weight_p] if ph2 else [weight_p]
            grads = torch.autograd.grad(force_loss + moment_loss + dist_loss if ph2 else gravity_loss, params)
            if i == phase1 and mutation != 'no_reset':
                for m in mom.values():
                    m[0].zero_(); m[1].zero_()
            it = i - table if (mutation == 'stale_table' and i >= table) else i
            n = (it - phase1 if (it >= phase1 and mutation != 'no_restart') else it) + 1
            with torch.no_grad():
                for p, g in zip(params, grads):
                    m, v = mom[id(p)]
                    p.mul_(1 - lr * WD)
                    m.lerp_(g, 1 - b1)
                    v.mul_(b2).addcmul_(g, g, value=1 - b2)
                    denom = (v.sqrt() / (1 - b2 ** n) ** 0.5).add_(eps)
                    p.addcdiv_(m, denom, value=-(lr / (1 - b1 ** n)))
            losses = (float(force_loss), float(gravity_loss), float(moment_loss), float(dist_loss))
        fl, fg = fl.detach().clone(), fg.detach().clone()
        fl[~grasped] = 0
        fg[~grasped] = 0
        r = dict(force_local=fl, force_global=fg, losses=losses, scale=scale_p.detach().clone(), weight=weight_p.detach().clone(), force_point=pts, frames=frame)
    finally:
        torch.set_default_dtype(old)
    return _pack(r)

"""Child process of tests/test_gpu_force_optim.py::test_exact_form_matches_fp64: the launches of _force_fp64.EXACT_CASES through
``Aggregation.force_optimize`` with VPHO_FORCE_EXACT=1 (force_optim_kernel<true>; the switch is read once per process, so the exact
form needs a process of its own).  Usage: ``python _force_exact_driver.py OUT.npz``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def launch(agg, ins, B, iters, phase1, lr):
    """one launch of the kernel on the inputs of _force_fp64.build; every output as a numpy array, the losses as four (n_batches,) columns"""
    import torch
    v, grav, com, fc, grasped = ins
    out = agg.force_optimize(v.cuda(), grav.view(-1, 3).cuda(), com.view(-1, 3).cuda(), fc.cuda(), grasped.to(torch.uint8).cuda(), B,
                             iters=iters, phase1=phase1, lr=lr)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in ('scale', 'weight', 'force_local', 'force_global', 'force_point', 'frames')}
    losses = out['losses'].cpu().numpy()
    for k, name in enumerate(('loss_force', 'loss_gravity', 'loss_moment', 'loss_dist')):
        got[name] = losses[:, k].copy()
    return got


def main():
    assert os.environ.get('VPHO_FORCE_EXACT') == '1', 'the driver is for the exact form'
    path = sys.argv[1]
    sys.argv = sys.argv[:1]
    import numpy as np
    from tests import _force_fp64 as R
    from vpho_amd import ops
    from vpho_amd.assets import ANCHOR_SKELETON
    agg = ops.Aggregation(R._assets(), ANCHOR_SKELETON, 'cuda')
    res = {}
    for name, (kind, B, n_batches, iters, phase1, lr) in R.EXACT_CASES.items():
        got = launch(agg, R.build(kind, B, n_batches, R.SEED), B, iters, phase1, lr)
        res.update({f'{name}/{k}': got[k] for k in R.OUTPUTS})
    np.savez(path, **res)


if __name__ == '__main__':
    main()

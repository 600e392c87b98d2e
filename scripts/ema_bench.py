"""The weights' moving average at the real layout (569 tensors, 63.7 M elements), three forms of one ``ExponentialMovingAverage.update``:
  (a) ``ops.EmaList.update`` (vpho_ema_multi_f32) on the training step's packed masters and shadows: one launch, 12 B per element
  (b) the chain a user would write on reference-layout tensors: ``torch._foreach_sub``, ``_foreach_mul_``, ``_foreach_sub_``
  (c) the reference's own loop (lib/model/ema.py:43-44): ``s.sub_(one_minus_decay * (s - p))`` per tensor
HIP events around each form, the three interleaved in one process, median of 10 after 3 warm-ups.  Before timing, (a) and (b) run once
from the same start and must agree to the bit (through ``state_dict(ema=True)``, i.e. the reference's layout).  Exits non-zero unless
(a) beats (b) by more than (b)'s max - min spread.  ``--step``: also the 64-image training step with ``ema`` on and off, interleaved
(reported, not gated).
    python scripts/ema_bench.py [--step] [--out profiles/<name>.txt]        (on the GPU box)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
with_step = '--step' in sys.argv
sys.argv = sys.argv[:1]
import torch  # noqa: E402
from vpho_amd.assets import synthetic_assets  # noqa: E402
from vpho_amd.model.VPHO import vpho_net  # noqa: E402
from vpho_amd.synth import synth_state_dict  # noqa: E402
from vpho_amd.train_step import DiffusionTrainStep  # noqa: E402

REPS, WARM, DECAY = 10, 3, 0.999
OPTIM_TBPS = 5.9                                                   # optim_multi_kernel on the same tensors (profiles/optim_tail_bench.txt)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    assets = synthetic_assets(0)
    sd = synth_state_dict(vpho_net(assets), seed=1)
    step = DiffusionTrainStep(sd, 'cuda', assets=assets, ema=DECAY)
    order = step.param_order
    n = sum(v.numel() for v in step.master.values())
    # shadows a little off their parameters, set through the public state (reference layout in, packed layout inside)
    g = torch.Generator().manual_seed(0)
    st = step.ema_state()
    st['shadow_params'] = [t + 0.01 * torch.randn(t.shape, generator=g) for t in st['shadow_params']]
    step.load_ema_state(st)
    live = step.state_dict()
    P = [live[k].contiguous() for k in order]                      # reference-layout tensors, as a user of the reference holds them
    S = [t.cuda() for t in st['shadow_params']]
    S_loop = [t.clone() for t in S]
    omd = step.ema.next_one_minus_decay()

    def ours():
        step._ema_list.update(omd)

    def foreach():
        d = torch._foreach_sub(S, P)
        torch._foreach_mul_(d, omd)
        torch._foreach_sub_(S, d)

    def loop():
        for s, p in zip(S_loop, P):
            s.sub_(omd * (s - p))

    ours(), foreach(), loop()
    avg = step.state_dict(ema=True)
    bad = [k for k, s, l in zip(order, S, S_loop) if not (torch.equal(avg[k].reshape(s.shape), s) and torch.equal(s, l))]
    assert not bad, f'(a), (b) and (c) differ on {len(bad)} tensors: {bad[:5]}'
    variants = {'(a) EmaList.update (one launch)': ours, '(b) _foreach_sub, _foreach_mul_, _foreach_sub_': foreach, '(c) per-tensor s.sub_(omd * (s - p))': loop}
    times = {k: [] for k in variants}
    for it in range(WARM + REPS):
        for name, fn in variants.items():                          # interleaved: every form once per round
            t = timed(fn)
            if it >= WARM:
                times[name].append(t)
    pairs = step._ema_list.keep
    vec = sum(p.numel() // 1024 * 1024 for p, s in pairs if p.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0)
    lines = [f'weights moving average, {len(pairs)} tensors, {n} elements ({n * 4 / 1e6:.1f} MB per pass; {vec / n * 100:.1f} % of the elements take the '
             f'float4 path); {torch.cuda.get_device_name(0)}',
             f'HIP events, median of {REPS} (min .. max), forms interleaved, us; (a) == (b) == (c) to the bit on all {len(order)} tensors']
    for name, t in times.items():
        lines.append(f'{name:50s} {statistics.median(t):9.1f}  ({min(t):.1f} .. {max(t):.1f})')
    ks = list(variants)
    a, b = statistics.median(times[ks[0]]), statistics.median(times[ks[1]])
    spread = max(times[ks[1]]) - min(times[ks[1]])
    lines.append(f'(a): {n * 12 / 1e9:.3f} GB by count (12 B per element) in {a:.1f} us = {n * 12 / a / 1e6:.2f} TB/s; optim_multi_kernel reaches '
                 f'{OPTIM_TBPS} TB/s on the same tensors (28 B per element)')
    lines.append(f'(b) - (a) = {b - a:.1f} us against (b)\'s spread of {spread:.1f} us; (a) / (b) = {a / b:.3f}')
    if with_step:
        lines += step_on_off(assets, sd)
    text = '\n'.join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(text + '\n')
    if not b - a > spread:
        sys.exit(f'gate: (a) {a:.1f} us does not beat (b) {b:.1f} us by more than (b)\'s spread {spread:.1f} us')


def step_on_off(assets, sd, bs=64, reps=5, warm=2):
    """the 64-image training step (all 13 losses, fused tail) with the average on and off, interleaved, wall clock around a synchronised step"""
    import time
    from vpho_amd.configs.args import cfg
    from vpho_amd.trainer import Trainer
    cfg.batch_size, cfg.checkpoint = bs, ''
    tr = Trainer(cfg)
    steps = {'ema off': DiffusionTrainStep(sd, 'cuda', assets=assets), 'ema on': DiffusionTrainStep(sd, 'cuda', assets=assets, ema=DECAY)}
    batch, gt_hand, gt_obj = next(tr._train_batches(None, 1, steps['ema off'].mano_head.mano))
    times = {k: [] for k in steps}
    for it in range(warm + reps):
        for name, s in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.step(batch, gt_hand, gt_obj, fused=True)
            torch.cuda.synchronize()
            if it >= warm:
                times[name].append((time.perf_counter() - t0) * 1e3)
    out = [f'{bs}-image training step, fused tail, median of {reps} (min .. max), interleaved, ms']
    for name, t in times.items():
        out.append(f'{name:50s} {statistics.median(t):9.2f}  ({min(t):.2f} .. {max(t):.2f})')
    return out


if __name__ == '__main__':
    main()

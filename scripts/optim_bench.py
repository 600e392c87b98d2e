"""The optimiser tail of the training step at the real layout (569 tensors, 63.7 M elements of one flat gradient buffer), clipping on:
  old   what ``DiffusionTrainStep.step(gradient_clip=5)`` runs: [flat.mul_(scale) when scale != 1,] flat.norm(2), flat.mul_(coef),
        ``ops.AdamWList.step`` (vpho_adamw_multi_f32)
  fused what ``step(..., fused=True)`` runs: ``ops.grad_sqnorm`` (vpho_grad_sqnorm_f64) + ``ops.OptimList.step`` (vpho_optim_multi_f32)
HIP events around each variant, the two interleaved, median of 10 after 3 warm-ups; the gradient is restored before every sample (the old
path scales it in place).  Also each launch of the fused tail alone, and the update without clipping in both forms.
    python scripts/optim_bench.py [--out profiles/<name>.txt]        (on the GPU box)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
sys.argv = sys.argv[:1]
import torch  # noqa: E402
from vpho_amd import ops  # noqa: E402
from vpho_amd.assets import synthetic_assets  # noqa: E402
from vpho_amd.model.VPHO import vpho_net  # noqa: E402
from vpho_amd.synth import synth_state_dict  # noqa: E402
from vpho_amd.train_step import DiffusionTrainStep  # noqa: E402

REPS, WARM, CLIP = 10, 3, 5.0
KW = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


def main():
    assets = synthetic_assets(0)
    step = DiffusionTrainStep(synth_state_dict(vpho_net(assets), seed=1), 'cuda', assets=assets)
    flat = step.flat_grad
    n = flat.numel()
    g = torch.Generator(device='cuda').manual_seed(0)
    grad0 = torch.randn(n, device='cuda', generator=g) * 1e-2            # norm ~ 80: the clip is active
    quads = [(step.master[k], step.grad_view[k], step.m[k], step.v[k]) for k in step.names]
    old, new = ops.AdamWList(quads), ops.OptimList(quads)
    ws = torch.empty(ops.grad_sqnorm_workspace_bytes(n) // 8, device='cuda', dtype=torch.float64)
    aligned = sum(1 for q in quads if all(t.data_ptr() % 16 == 0 for t in q))
    elems_vec = sum(q[0].numel() // 1024 * 1024 for q in quads if all(t.data_ptr() % 16 == 0 for t in q))

    def old_tail(scale):
        s = scale
        if s != 1.0:
            flat.mul_(s)
            s = 1.0
        coef = (CLIP / (flat.norm(2) + 1e-6)).clamp(max=1.0)
        flat.mul_(coef)
        old.step(1, grad_scale=s, **KW)

    def fused_tail(scale):
        sq = ops.grad_sqnorm(flat, ws=ws)
        new.step(1, kind=0, grad_scale=scale, sqnorm=sq, max_norm=CLIP, **KW)

    variants = {
        'old   scale 1   (norm, mul_, adamw_multi)': lambda: old_tail(1.0),
        'fused scale 1   (grad_sqnorm, optim_multi)': lambda: fused_tail(1.0),
        'old   scale 1/8 (mul_, norm, mul_, adamw_multi)': lambda: old_tail(0.125),
        'fused scale 1/8 (grad_sqnorm, optim_multi)': lambda: fused_tail(0.125),
        'grad_sqnorm alone': lambda: ops.grad_sqnorm(flat, ws=ws),
        'adamw_multi alone (no clip)': lambda: old.step(1, **KW),
        'optim_multi alone (no clip, kind 0)': lambda: new.step(1, kind=0, **KW),
        'optim_multi alone (no clip, kind 1)': lambda: new.step(1, kind=1, **KW),
    }
    times = {k: [] for k in variants}
    for it in range(WARM + REPS):
        for name, fn in variants.items():                                  # interleaved: every variant once per round
            flat.copy_(grad0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if it >= WARM:
                times[name].append(a.elapsed_time(b) * 1e3)
    lines = [f'optimiser tail, {len(quads)} tensors, {n} elements ({n * 4 / 1e6:.1f} MB per pass); {aligned} segments with four 16-byte aligned '
             f'pointers ({elems_vec / n * 100:.1f} % of the elements take the float4 path); {torch.cuda.get_device_name(0)}',
             f'HIP events, median of {REPS} (min .. max), variants interleaved, us']
    for name, t in times.items():
        lines.append(f'{name:50s} {statistics.median(t):9.1f}  ({min(t):.1f} .. {max(t):.1f})')
    med = {k: statistics.median(v) for k, v in times.items()}
    ks = list(variants)
    lines.append(f'fused / old: scale 1 {med[ks[1]] / med[ks[0]]:.3f}, scale 1/8 {med[ks[3]] / med[ks[2]]:.3f}')
    lines.append(f'bytes by count: old {n * (8 + 4 + 28) / 1e9:.2f} GB (scale 1: norm 4 B + mul_ 8 B + update 28 B per element; + 8 B with the scale pass), '
                 f'fused {n * (4 + 28) / 1e9:.2f} GB')
    text = '\n'.join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()

"""Timing of the hand contact map of every sampled hypothesis (--eval_best with --eval_grasp) at the README configuration: 64 images x 50
hypotheses, 1 080 filled hand vertices, 21 objects of 8 000 .. 26 000 vertices (seeded ellipsoids: the sizes of full object meshes).
Two legs in one process, interleaved, HIP events around each, 5 warm-ups, then the median of ``--reps`` passes with min and max:
  pruned    ops.ContactMulti (vpho_contact_multi_f32): model frame, fp64, the pruned walk; no posed object vertex exists
  brute     Aggregation.hand_contact (vpho_contact_detect_f32) fed the posed fp32 vertices of all pairs, padded to the longest object --
            the only way to get these maps without the new kernel; the posing itself (fp64 torch ops) is timed separately, once
and the two agreement launches (vpho_contact_agreement_f32) on the pruned leg's maps.  The hands are near-contact: every hand vertex
within 12 mm of the object's surface.  Prints one CONTACT_MULTI_BENCH JSON line.
A wave of the pruned kernel visits every cluster that any of its 64 consecutive hand vertices needs, so its time depends on how close to
each other those vertices are: ``--coherent`` sorts each hand's vertices along the object's Morton order.
``python scripts/contact_multi_bench.py [--reps 20] [--bs 64] [--samples 50] [--brute_samples 50] [--coherent]``"""
import argparse
import json
import os
import statistics
import sys

sys.argv, _argv = sys.argv[:1], sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

NH = 1080
GATES = dict(normal_thresh=(-0.01, 0.01), vertical_thresh=0.005, decay=(-0.005, 0.005))


def _ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _rotations(r, k):
    q = r.normal(size=(k, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--bs', type=int, default=64)
    ap.add_argument('--samples', type=int, default=50)
    ap.add_argument('--brute_samples', type=int, default=50, help='hypotheses per image of the brute leg (fewer if the posed table does not fit)')
    ap.add_argument('--coherent', action='store_true', help='consecutive hand vertices are neighbours on the object (sorted along its Morton order), '
                                                            'as the vertices of a hand mesh are; default: every hand vertex anywhere on the object')
    a = ap.parse_args(_argv)
    from vpho_amd import grasp_eval as GE
    from vpho_amd import ops
    from vpho_amd.assets import ANCHOR_SKELETON, synthetic_assets
    n, S, Sb, dev = a.bs, a.samples, min(a.brute_samples, a.samples), 'cuda'
    r = np.random.default_rng(0)
    sizes = np.linspace(8000, 26000, 21).astype(int)
    objs = []
    for k in sizes:
        u = r.normal(size=(k, 3))
        objs.append(u / np.linalg.norm(u, axis=1, keepdims=True) * np.array([0.04, 0.05, 0.06]) + np.array([0.01, -0.02, 0.005]))
    ids = r.integers(0, len(objs), n)
    root = r.normal(size=(n, 3)) * 0.05 + np.array([0.03, -0.02, 0.6])
    right = (np.arange(n) % 2).astype(np.uint8)
    R = _rotations(r, n * S).reshape(n, S, 3, 3)
    t = root[:, None] + r.normal(size=(n, S, 3)) * 0.03
    rt = np.concatenate([R, t[..., None]], -1)
    vf, nf = np.zeros((n, S, NH, 3), np.float32), np.zeros((n, S, NH, 3), np.float32)
    for i in range(n):
        v = objs[ids[i]]
        centre, sg = v.mean(0), np.array([1.0 if right[i] else -1.0, 1.0, 1.0])
        which = r.integers(0, len(v), (S, NH))
        if a.coherent:
            rank = np.argsort(GE.vertex_accel(v)['index'])
            which = np.take_along_axis(which, np.argsort(rank[which], axis=1), 1)
        pick = v[which]
        u = pick - centre
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        p = pick + u * r.uniform(-0.012, 0.012, (S, NH, 1)) + r.normal(size=(S, NH, 3)) * 0.002
        m = -u + r.normal(size=(S, NH, 3)) * 0.2
        m /= np.linalg.norm(m, axis=-1, keepdims=True)
        vf[i] = (np.einsum('sij,svj->svi', R[i], p) + (t[i] - root[i])[:, None]) * sg
        nf[i] = np.einsum('sij,svj->svi', R[i], m) * sg
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(dev, dt).contiguous()
    vf_d, nf_d, root_d, right_d, rt_d, ids_d = d(vf, torch.float32), d(nf, torch.float32), d(root, torch.float64), d(right, torch.uint8), \
        d(rt, torch.float64), d(ids, torch.int32)
    kernel = ops.ContactMulti(GE.vertex_accel_tables(objs), dev)
    gates = (GATES['normal_thresh'], GATES['vertical_thresh'], GATES['decay'])
    pruned = lambda: kernel(vf_d, nf_d, root_d, right_d, rt_d, ids_d, *gates)
    # the brute leg's input: every pair's object posed into the hand's frame (PhysicsLabeler.object_verts), padded to the longest object
    agg = ops.Aggregation(synthetic_assets(0), ANCHOR_SKELETON, torch.device(dev))
    top = int(sizes.max())
    padded = torch.from_numpy(np.stack([np.concatenate([v, np.repeat(v[-1:], top - len(v), 0)]) for v in objs])).to(dev)
    sign = torch.where(right_d.bool(), 1.0, -1.0).to(torch.float64)

    def pose():
        out = torch.empty((n, Sb, top, 3), dtype=torch.float32, device=dev)
        for i in range(n):                                   # per image: the fp64 intermediate of all pairs at once would be 2 x the table
            p = padded[ids[i]][None] @ rt_d[i, :Sb, :, :3].transpose(1, 2) + (rt_d[i, :Sb, :, 3] - root_d[i])[:, None]
            p[..., 0] *= sign[i]
            out[i] = p.float()
        return out.view(n * Sb, top, 3)

    pose_ms = _ms(lambda: pose())
    posed = pose()
    hv_b, hn_b = vf_d[:, :Sb].reshape(n * Sb, NH, 3).contiguous(), nf_d[:, :Sb].reshape(n * Sb, NH, 3).contiguous()
    brute = lambda: agg.hand_contact(hv_b, hn_b, posed, *gates)
    w = pruned()
    wb = brute().view(n, Sb, NH)
    fc, gr = agg.force_contact(w.view(n * S, NH))
    fc, gr = fc.view(n, S, 32), gr.view(n, S)
    w_gt = w[:, 0].contiguous()
    agree = lambda: ops.contact_agreement(w, w_gt, fc, gr, fc[:, 0].contiguous(), gr[:, 0].contiguous())
    torch.cuda.synchronize()
    same_state = float(((w[:, :Sb] > 0) == (wb > 0)).double().mean())
    legs = dict(pruned=pruned, brute=brute, agreement=agree)
    for _ in range(5):
        for fn in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            ts[k].append(_ms(fn))
    res = dict(coherent=bool(a.coherent), n=n, S=S, brute_S=Sb, Nh=NH, objects=len(objs), verts_min=int(sizes.min()), verts_max=top, reps=a.reps,
               posed_table_GB=round(posed.numel() * 4 / 1e9, 3), pose_ms_once=round(pose_ms, 1), in_contact_share=round(float((w > 0).double().mean()), 4),
               same_contact_state_share=round(same_state, 6), max_weight_diff=float((w[:, :Sb] - wb.clamp(0, 1)).abs().max()))
    for k, v in ts.items():
        res[k] = dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
    res['brute_per_pair_us'] = round(res['brute']['median_ms'] * 1e3 / (n * Sb), 2)
    res['pruned_per_pair_us'] = round(res['pruned']['median_ms'] * 1e3 / (n * S), 2)
    res['brute_over_pruned_per_pair'] = round(res['brute_per_pair_us'] / res['pruned_per_pair_us'], 2)
    print('CONTACT_MULTI_BENCH ' + json.dumps(res))


if __name__ == '__main__':
    main()

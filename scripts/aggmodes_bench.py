"""Aggregation time of every --aggregation_mode_hand / --aggregation_mode_obj against the default cascade, at the README config
(bs 64, sample_num 100, topk 30 / 10): HIP events around Engine.aggregate (plain launches), median of 10, each mode interleaved with
the default.  python scripts/aggmodes_bench.py [--bs 64] [--sample_num 100]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=64)
    ap.add_argument('--sample_num', type=int, default=100)
    ap.add_argument('--topk_hand', type=int, default=30)
    ap.add_argument('--topk_obj', type=int, default=10)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    sys.argv = sys.argv[:1]
    os.environ['VPHO_GRAPHS'] = '0'
    import torch
    from vpho_amd.assets import synthetic_assets
    from vpho_amd.configs.args import cfg, AGGREGATION_MODES_HAND, AGGREGATION_MODES_OBJ
    from vpho_amd.model.VPHO import vpho_net
    from vpho_amd.model.engine import Engine
    from vpho_amd.synth import bench_state_dict, synth_batch
    cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = a.sample_num, 5, a.topk_hand, a.topk_obj, 0.2
    assets = synthetic_assets(0)
    model = vpho_net(assets)
    model.load_state_dict(bench_state_dict(model, seed=1))
    eng = Engine(model.cuda().eval())
    data = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth_batch(a.bs, assets, seed=206).items()}
    torch.manual_seed(0)
    out = eng.predict(data)
    f = eng.last_info['features']
    final, x_o = out['diff_final_hand_mano'].reshape(-1, 58).contiguous(), out['diff_final_obj_6d'].contiguous()

    def once(mh, mo):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.aggregate(f, data, final, x_o, a.sample_num, a.topk_hand, a.topk_obj, mode_hand=mh, mode_obj=mo)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    D = 'heatmap_cascade'
    pairs = [(h, 'random') for h in AGGREGATION_MODES_HAND if h != D] + [('random', o) for o in AGGREGATION_MODES_OBJ if o != D]
    res = {}
    for mh, mo in pairs:
        once(mh, mo), once(D, D)                                   # warm-up
        t_mode, t_def = [], []
        for _ in range(a.reps):
            t_mode.append(once(mh, mo))
            t_def.append(once(D, D))
        res[f'{mh}+{mo}'] = dict(ms=statistics.median(t_mode), default_cascade_ms=statistics.median(t_def))
    print('AGGMODES_BENCH ' + json.dumps(dict(bs=a.bs, sample_num=a.sample_num, topk_hand=a.topk_hand, topk_obj=a.topk_obj, modes=res)))


if __name__ == '__main__':
    main()

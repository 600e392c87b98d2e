"""Golden vectors for the multi-hypothesis evaluation (--eval_best) by calling the reference's own TesterHand / TesterObject
(lib/engine/test.py).

Run in the build container only.  Same stubs as make_golden_objmetrics.py (``object.__new__`` for TesterObject, whose __init__
opens an absent JSON; ``torch.Tensor.cuda`` as an identity).
* Hand: the candidates are drawn in the model frame, as predict returns diff_final_hand_joint / _vert; the reference's
  postprocess (train_diff_hand_obj.py:578-602: x un-flipped for left hands, root joint added, fp32) is applied here, then
  ``TesterHand.__call__`` scores pd (N, S, P, 3) against gt (N, P, 3) (test.py:589-597,657-679).
* Object: ``TesterObject.__call__`` cannot take pd_rt (N, S, 3, 4) in one call (criterion_MCE2 hands (1, S, n, 3) to
  compute_obj_metrics_dexycb, which unpacks three dimensions, test.py:155-156,413-416), so it is called once per candidate slice
  pd_rt[:, s]; the results are stacked along a last axis of length S and given to ``TesterObject.postprocess`` (test.py:522-582).
Writes golden_multihyp.npz: inputs, the per-hypothesis arrays and the postprocess table (average_instance, truncated units).
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

N, S = 6, 8


def main():
    from vpho_amd.assets import synthetic_assets
    from oracle.metrics import OBJ_METRIC_NAMES
    from oracle import rotations as R
    assets = synthetic_assets(0)
    tmp = tempfile.mkdtemp(prefix='vpho_golden_multihyp_')
    MG.write_assets(tmp, assets)
    os.chdir(tmp)
    sys.argv = ['main.py', '--mode', 'eval']
    sys.path.insert(0, MG.REF)
    MG.install_stubs(assets)
    ycb = sys.modules['lib.dataset.base'].YCB_MESHES
    for k, v in assets['ycb'].items():          # fp64 tables like trimesh's (base.py:222-244)
        ycb[k] = {kk: (np.asarray(vv, np.float64) if isinstance(vv, np.ndarray) else vv) for kk, vv in ycb[k].items()}
        ycb[k]['bbox3d'] = np.asarray(v['bbox3d'], np.float64)
        ycb[k]['verts'] = np.asarray(v['verts'], np.float64)
        ycb[k]['verts_sampled'] = np.asarray(v['verts_sampled'], np.float64)
        ycb[k]['diameter'] = v['diameter']
    torch.Tensor.cuda = lambda self, *a, **kw: self
    from lib.engine.test import TesterHand, TesterObject
    rng = np.random.default_rng(2024)

    # ---- hand ---------------------------------------------------------------------------------------------------------
    is_right = np.array([True, False, True, True, False, True])          # one left hand at least
    root = (rng.normal(size=(N, 3)) * 0.05 + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    gtj = (rng.normal(size=(N, 21, 3)) * 0.04).astype(np.float32) + root[:, None]
    gtv = (rng.normal(size=(N, 778, 3)) * 0.04).astype(np.float32) + root[:, None]
    sgn = np.where(is_right, 1.0, -1.0).astype(np.float32)[:, None, None, None]

    def model_frame(gt, scale):
        cam = gt[:, None] + (rng.normal(size=(N, S) + gt.shape[1:]) * scale[None, :, None, None]).astype(np.float32)
        m = (cam - root[:, None, None]).astype(np.float32)
        m[..., 0] *= sgn[..., 0]
        return m.astype(np.float32)
    scale = np.linspace(0.002, 0.03, S)
    pdj_m, pdv_m = model_frame(gtj, scale), model_frame(gtv, scale)

    def post(m):                                 # train_diff_hand_obj.py:578-602 in fp32
        v = m.copy()
        v[..., 0] = v[..., 0] * sgn[..., 0]
        return v + root[:, None, None]
    res = TesterHand()({'is_right': is_right, 'gt_joint': gtj, 'pd_joint': post(pdj_m), 'gt_vert': gtv, 'pd_vert': post(pdv_m)})
    hand = np.stack([np.asarray(res[k]['both'], np.float64).reshape(N, S) for k in ('MJE', 'PA_MJE', 'MVE', 'PAMVE')], -1)

    # ---- object -------------------------------------------------------------------------------------------------------
    tester = object.__new__(TesterObject)
    tester.obj_mesh = ycb
    names = list(ycb.keys())
    obj_idx = np.array([0, 1, 2, 0, 3, 1])                              # four objects, two of them twice
    obj_name = np.array([names[i] for i in obj_idx])
    aa = torch.from_numpy(rng.normal(size=(N, 3)))
    gRm = R.axis_angle_to_matrix(aa).numpy()
    gt_rt = np.concatenate([gRm, (rng.normal(size=(N, 3)) * 0.05 + np.array([0, 0, 0.7]))[:, :, None]], -1).astype(np.float32)
    rot_s = np.linspace(0.003, 0.5, S)
    tr_s = np.linspace(0.0005, 0.04, S)
    pd_rt = np.zeros((N, S, 3, 4), np.float64)
    for s in range(S):
        dR = R.axis_angle_to_matrix(torch.from_numpy(rng.normal(size=(N, 3)) * rot_s[s])).numpy()
        pd_rt[:, s, :, :3] = dR @ gt_rt[:, :, :3]
        pd_rt[:, s, :, 3] = gt_rt[:, :, 3] + rng.normal(size=(N, 3)) * tr_s[s]
    pd_rt = pd_rt.astype(np.float32)
    pd_rt[0, 3] = gt_rt[0]                                              # a candidate equal to the ground truth
    f = rng.uniform(400, 600, size=N)
    cam = np.stack([np.array([[fi, 0, 128.0], [0, fi, 128.0], [0, 0, 1.0]]) for fi in f]).astype(np.float32)
    per_s = [tester({'pd_rt': pd_rt[:, s], 'gt_rt': gt_rt, 'obj_name': obj_name, 'cam_intr': cam}) for s in range(S)]
    # one value per image and candidate (the F-score / Chamfer criteria keep a singleton batch axis: (m, 1) -> (m,))
    flat = lambda a: np.asarray(a).reshape(np.asarray(a).shape[0])
    stacked = {k: {kk: np.stack([flat(r[k][kk]) for r in per_s], -1) for kk in per_s[0][k]} for k in per_s[0]}
    # REP5 is computed by __call__ (cal_REP5, test.py:518-519) but not put into its result dict: derived here from REP
    col = lambda k: (stacked['REP']['average_instance'] < 5) if k == 'REP5' else stacked[k]['average_instance']
    obj = np.stack([np.asarray(col(k), np.float64).reshape(N, S) for k in OBJ_METRIC_NAMES], -1)      # (N, S, 16)
    table = tester.postprocess(stacked)
    post_names = [k for k in OBJ_METRIC_NAMES if k in table]
    post_vals = np.array([table[k]['average_instance'] for k in post_names], np.float64)
    print(post_names)
    print(post_vals)
    out = os.path.join(HERE, 'golden_multihyp.npz')
    np.savez_compressed(out, is_right=is_right, root_joint=root, gt_joint=gtj, gt_vert=gtv, pd_joint_model=pdj_m, pd_vert_model=pdv_m,
                        hand=hand, pd_rt=pd_rt, gt_rt=gt_rt, cam_intr=cam, obj_idx=obj_idx.astype(np.int64), obj=obj,
                        post_names=np.array(post_names), post_table=post_vals)
    print(out, os.path.getsize(out) // 1024, 'KiB')


if __name__ == '__main__':
    main()

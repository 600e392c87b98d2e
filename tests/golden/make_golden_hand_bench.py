"""Golden vectors for the hand benchmark metrics (--eval_hand_bench): the reference's own ``rigid_align_AtoB``
(lib/utils/transform_fn.py:43-66) run on the 48 (hypothesis, ground truth) pairs of golden_multihyp.npz.

Run in the build container only (same stubs as make_golden_multihyp.py; the reference is imported here and nowhere else).  The inputs are
the post-processed points (train_diff_hand_obj.py:578-602 in fp32: x un-flipped for left hands, root added), float32 as the reference
passes them, so the alignment is the reference's float32-numpy one.  Writes golden_hand_bench.npz:
* aligned_joint (6, 8, 21, 3), aligned_vert (6, 8, 778, 3) float32: the reference's aligned points, as data;
* from the float64 restatement tests/_hand_bench_fp64.py on the same inputs: values_* (6, 8, 6), counts_* (6, 8, 10) and, per
  (pair, set, direction, threshold), band_mask_vert (6, 8, 8, 778): the nearest-neighbour distances within 2e-7 m of their threshold,
  in the order of the kernel's eight counts; margin = the smallest |e - t_j| of any point error to any AUC table entry.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402
import tests._hand_bench_fp64 as HB  # noqa: E402


def main():
    from vpho_amd.assets import synthetic_assets
    sys.argv = ['main.py', '--mode', 'eval']
    sys.path.insert(0, MG.REF)
    MG.install_stubs(synthetic_assets(0))
    from lib.utils.transform_fn import rigid_align_AtoB
    z = np.load(os.path.join(HERE, 'golden_multihyp.npz'))
    N, S = z['pd_vert_model'].shape[:2]
    out = {}
    for key, pd_m, gt in (('joint', z['pd_joint_model'], z['gt_joint']), ('vert', z['pd_vert_model'], z['gt_vert'])):
        cam = HB.postprocess(pd_m, z['root_joint'], z['is_right'])
        out['aligned_' + key] = np.stack([np.stack([np.asarray(rigid_align_AtoB(cam[b, s], gt[b]), np.float32) for s in range(S)]) for b in range(N)])
        values, counts, band, margin = HB.bench_multi(pd_m, gt, z['root_joint'], z['is_right'], with_fscore=key == 'vert')
        out['values_' + key], out['counts_' + key] = values, counts.astype(np.int32)
        out['margin_e_' + key] = np.float64(margin[0])
        print(key, 'margin to the AUC table', margin[0], 'to the F thresholds', margin[1], 'in band', int(band.sum()), 'of', band.size * gt.shape[1])
        if key == 'vert':
            mask = np.zeros((N, S, 8, gt.shape[1]), bool)
            for b in range(N):
                for s in range(S):
                    A, B = cam[b, s], gt[b]
                    for k, X in enumerate((A, HB.align(A, B))):
                        for j, d in enumerate(HB.nn_dists(X, B)):
                            for i, th in enumerate(HB.F_THRESH):
                                mask[b, s, k * 4 + j * 2 + i] = np.abs(d - th) <= HB.BAND
            assert (mask.sum(-1) == band).all()
            out['band_mask_vert'] = mask
    path = os.path.join(HERE, 'golden_hand_bench.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()

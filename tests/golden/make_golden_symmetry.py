"""Golden vectors for the symmetry table and the symmetric mean corner error, by calling the reference's own ``TesterObject``
(lib/engine/test.py): its ``__init__`` (:197-227, which builds the padded R / t table with get_symmetry_transformations) and
``criterion_SMCE`` (:377-398).

Run in the build container only.  Same stubs as make_golden_objmetrics.py; this time a synthetic
``asset/2023_NIPS_DeepSimHO/assets_models_info.json`` is written into the temporary working directory first, so that ``TesterObject()``
runs its own ``__init__``.  Three objects (the first three YCB classes, keys "1" .. "3"):
  1  no symmetry at all (K = 1 of its own)
  2  discrete symmetries only: a half-turn about z and a half-turn about x that also shifts along x (K = 3 of its own)
  3  a continuous symmetry about an axis with an offset, and one discrete half-turn: (1 + 1) x 314 = 628 transforms at step 0.01
Writes golden_symmetry.npz: the JSON text, the reference's padded R / t (3, 628, 3, 3) / (3, 628, 3) in metres, float64 poses pd_rt
(n, S, 3, 4) / gt_rt (n, 3, 4) / obj_idx (n,), and criterion_SMCE's values (n, S) -- its ``...`` axes take the S hypotheses at once.
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402


def model_info():
    half_z = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    half_x_shift = [1, 0, 0, 12.5, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]          # millimetres
    half_y = [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
    return {'1': {'diameter': 100.0},
            '2': {'symmetries_discrete': [half_z, half_x_shift]},
            '3': {'symmetries_continuous': [{'axis': [0.2, -0.1, 1.0], 'offset': [4.0, -3.0, 1.5]}], 'symmetries_discrete': [half_y]}}


def main():
    from vpho_amd.assets import YCB_NAMES, synthetic_assets
    assets = synthetic_assets(0)
    tmp = tempfile.mkdtemp(prefix='vpho_golden_sym_')
    MG.write_assets(tmp, assets)
    text = json.dumps(model_info())
    os.makedirs(os.path.join(tmp, 'asset', '2023_NIPS_DeepSimHO'))
    with open(os.path.join(tmp, 'asset', '2023_NIPS_DeepSimHO', 'assets_models_info.json'), 'w') as f:
        f.write(text)
    os.chdir(tmp)
    sys.argv = ['main.py', '--mode', 'eval']
    sys.path.insert(0, MG.REF)
    MG.install_stubs(assets)
    ycb = sys.modules['lib.dataset.base'].YCB_MESHES
    for k, v in assets['ycb'].items():
        ycb[k]['bbox3d'] = np.asarray(v['bbox3d'], np.float64)
    torch.Tensor.cuda = lambda self, *a, **kw: self
    from lib.engine.test import TesterObject
    tester = TesterObject()
    assert tester.R.shape == (3, 628, 3, 3) and tester.t.shape == (3, 628, 3, 1), (tester.R.shape, tester.t.shape)

    rng = np.random.default_rng(2024)
    from oracle import rotations as R
    n, S = 6, 5
    obj_idx = np.array([0, 1, 2, 2, 1, 0])

    def rot(scale, size):
        return R.axis_angle_to_matrix(torch.from_numpy(rng.normal(size=size + (3,)) * scale)).numpy()

    gt_rt = np.concatenate([rot(1.0, (n,)), (rng.normal(size=(n, 3)) * 0.05 + [0.0, 0.0, 0.7])[:, :, None]], -1)
    pd_rt = np.zeros((n, S, 3, 4))
    for b in range(n):
        K_own = (1, 3, 628)[obj_idx[b]]
        for s in range(S):
            # hypothesis 0: the ground truth moved by one of the object's OWN symmetries, exactly; then from near to far off, each near
            # another symmetric copy of the ground truth
            k = int(rng.integers(0, K_own))
            Sk = np.concatenate([tester.R[obj_idx[b], k], tester.t[obj_idx[b], k]], -1)
            base = gt_rt[b] @ np.concatenate([Sk, [[0, 0, 0, 1]]], 0)
            if s > 0:
                dR = rot(0.02 * 4.0 ** (s - 1), ())
                base = np.concatenate([dR @ base[:, :3], (base[:, 3] + rng.normal(size=3) * 0.002 * 3.0 ** (s - 1))[:, None]], -1)
            pd_rt[b, s] = base
    smce = np.stack([tester.criterion_SMCE(pd_rt[b], gt_rt[b], YCB_NAMES[obj_idx[b]]) for b in range(n)])
    mce = np.stack([tester.criterion_MCE_OCE(pd_rt[b], gt_rt[b], YCB_NAMES[obj_idx[b]])[0] for b in range(n)])
    assert smce.shape == (n, S)
    print(np.array2string(smce, precision=6), '\n', np.array2string(mce, precision=6))
    out = os.path.join(HERE, 'golden_symmetry.npz')
    np.savez_compressed(out, json=np.array(text), R=tester.R, t=tester.t[..., 0], pd_rt=pd_rt, gt_rt=gt_rt, obj_idx=obj_idx.astype(np.int64),
                        smce=smce, mce=mce)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()

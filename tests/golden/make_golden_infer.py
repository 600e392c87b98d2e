"""Golden vectors for --mode infer (Trainer.infer, lib/engine/train_diff_hand_obj.py:359-444) from the reference's own functions.

Run in the build container only; needs the reference checkout (make_golden.REF).  ``lib.engine.train_diff_hand_obj`` does not import
there (accelerate, thop, the data sets), so the four functions this fixture needs -- ``Trainer.postprocess`` with its two private
helpers ``__postprocess_obj_rt`` / ``__postprocess_hand_vert`` (:578-602) and the module-level ``dump`` (:872-880) -- are taken out of
the reference FILE at generation time (their syntax trees, compiled here inside an empty ``class Trainer`` so that the private names
mangle as they do there); ``obj_9D_to_mat`` and ``OPENGL_TO_OPENCV`` are imported from lib.utils.transform_fn with make_golden's stubs.
Nothing of the reference's text is stored: the fixture holds inputs and results only.

6 images in 2 batches of 3, ``index`` a shuffled permutation, two left hands.  Images 3 (right) and 4 (left) have a zero root joint,
so that chosen fp32 values reach the half conversion unchanged: exact fp16 rounding ties and their fp32 neighbours, values at and
above the overflow threshold 65520, and values around the smallest half subnormal 2^-24 = 5.96e-8 (below 6e-8).
The flow is the reference's (:372-431): postprocess -> to_numpy -> phy_data_dt (astype(np.float16)) -> @ OPENGL_TO_OPENCV -> the
per-index dict -> lists in index order -> dump.
Writes golden_infer.npz: inputs, post-processed arrays, fp16 bits (uint16), pd_obj_rt, the two JSON files' bytes (uint8).
"""
import ast
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

N, BATCH = 6, 3
HAND_KEYS = ('reg_hand_joint', 'reg_hand_vert', 'agg_hand_joint', 'agg_hand_vert')


def reference_functions(namespace):
    """(Trainer class holding postprocess + its helpers, dump) compiled from the reference file's own syntax trees"""
    path = os.path.join(MG.REF, 'lib', 'engine', 'train_diff_hand_obj.py')
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'Trainer')
    want = ('postprocess', '__postprocess_obj_rt', '__postprocess_hand_vert')
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(m.name for m in methods) == sorted(want)
    dump = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'dump')
    mod = ast.Module(body=[ast.ClassDef(name='Trainer', bases=[], keywords=[], body=methods, decorator_list=[]), dump], type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, 'exec'), namespace)
    return namespace['Trainer'], namespace['dump']


def edge_values():
    """fp32 values for the half conversion: ties, their neighbours, overflow, subnormals (both signs)"""
    f = np.float32
    up = lambda x: np.nextafter(f(x), f(np.inf))
    dn = lambda x: np.nextafter(f(x), f(-np.inf))
    tie_even, tie_odd = f(1.0 + 2.0 ** -11), f(1.0 + 3 * 2.0 ** -11)          # halfway 1 | 1+2^-10 (-> 1), halfway 1+2^-10 | 1+2^-9 (-> 1+2^-9)
    v = [tie_even, up(tie_even), dn(tie_even), tie_odd, up(tie_odd), dn(tie_odd),
         f(65504.0), f(65519.0), dn(65520.0), f(65520.0), up(65520.0), f(70000.0), f(1e5),          # 65520 = halfway 65504 | 2^16 -> inf
         f(2.0 ** -24), f(5.9e-8), f(2.0 ** -25), up(2.0 ** -25), dn(2.0 ** -25), f(1e-8), f(3 * 2.0 ** -25), up(3 * 2.0 ** -25),
         f(1e-6), f(3e-5), f(6.1e-5), f(2.0 ** -14), dn(2.0 ** -14)]                                   # half subnormals and the first normal
    v = np.array(v, np.float32)
    return np.concatenate([v, -v])


def main():
    from vpho_amd.assets import synthetic_assets
    assets = synthetic_assets(0)
    tmp = tempfile.mkdtemp(prefix='vpho_golden_infer_')
    MG.write_assets(tmp, assets)
    os.chdir(tmp)
    sys.argv = ['main.py', '--mode', 'infer']
    sys.path.insert(0, MG.REF)
    MG.install_stubs(assets)
    from lib.utils.transform_fn import obj_9D_to_mat, OPENGL_TO_OPENCV
    Trainer, dump = reference_functions({'torch': torch, 'np': np, 'json': json, 'obj_9D_to_mat': obj_9D_to_mat})
    trainer = object.__new__(Trainer)

    rng = np.random.default_rng(359)
    is_right = np.array([True, False, True, True, False, True])
    root = (rng.normal(size=(N, 3)) * 0.05 + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    root[3] = 0.0
    root[4] = 0.0
    inp = {'reg_hand_joint': (rng.normal(size=(N, 21, 3)) * 0.04).astype(np.float32), 'reg_hand_vert': (rng.normal(size=(N, 778, 3)) * 0.04).astype(np.float32),
           'agg_hand_joint': (rng.normal(size=(N, 21, 3)) * 0.04).astype(np.float32), 'agg_hand_vert': (rng.normal(size=(N, 778, 3)) * 0.04).astype(np.float32)}
    ev = edge_values()
    for img in (3, 4):                                   # all three components, x included (negated for the left hand, image 4)
        flat = inp['agg_hand_vert'][img].reshape(-1)
        flat[:ev.size] = ev
        flat[ev.size:2 * ev.size] = ev[::-1]             # the other phase of (component, pair slot)
    pose9 = np.concatenate([rng.normal(size=(N, 6)), rng.normal(size=(N, 3)) * 0.05 + np.array([0.0, 0.0, 0.1])], -1)       # float64
    index = rng.permutation(N).astype(np.int64)
    paths = np.array([f'synthetic/subject-{i % 3:02d}/color_{int(index[i]):06d}.jpg' for i in range(N)])

    post, f16, obj_rt, obj_rt_dtype = {k: [] for k in HAND_KEYS}, [], [], None
    collector_hand = []
    for b0 in range(0, N, BATCH):
        sl = slice(b0, b0 + BATCH)
        res_dt = {k: torch.from_numpy(v[sl].copy()) for k, v in inp.items()}
        res_dt['agg_obj_6d'] = torch.from_numpy(pose9[sl].copy())
        root_t, right_t = torch.from_numpy(root[sl].copy()), torch.from_numpy(is_right[sl].copy())
        res_dt = trainer.postprocess(res_dt, root_t, right_t)        # fp64 pose + fp32 root: einsum promotes, agg_obj_rt is float64
        res_dt = {k: v.numpy() for k, v in res_dt.items()}                       # to_numpy (:375)
        obj_rt.append(res_dt['agg_obj_rt'])
        obj_rt_dtype = res_dt['agg_obj_rt'].dtype
        f16.append(res_dt['agg_hand_vert'].astype(np.float16))                   # :383
        for k in HAND_KEYS:
            post[k].append(res_dt[k].copy())
            res_dt[k] = res_dt[k] @ OPENGL_TO_OPENCV                             # :387-390
        for ind in range(BATCH):                                                  # :394-403
            collector_hand.append({index[b0 + ind].item(): {'joint_reg': res_dt['reg_hand_joint'][ind], 'vert_reg': res_dt['reg_hand_vert'][ind],
                                                            'joint_diff': res_dt['agg_hand_joint'][ind], 'vert_diff': res_dt['agg_hand_vert'][ind]}})
    collector_hand = {k: v for dt in collector_hand for k, v in dt.items()}       # :420-426
    lists = {k: [collector_hand[i][k] for i in range(len(collector_hand))] for k in ('joint_reg', 'vert_reg', 'joint_diff', 'vert_diff')}
    print('dtype of the arrays handed to dump:', lists['joint_reg'][0].dtype, ' pd_obj_rt:', obj_rt_dtype)
    reg_path, diff_path = os.path.join(tmp, 'hand_reg.json'), os.path.join(tmp, 'hand_diff.json')
    dump(reg_path, lists['joint_reg'], lists['vert_reg'])
    dump(diff_path, lists['joint_diff'], lists['vert_diff'])
    G = {'in_' + k: v for k, v in inp.items()}
    G.update({'post_' + k: np.concatenate(v, 0) for k, v in post.items()})
    f16 = np.concatenate(f16, 0)
    assert np.isinf(f16).any() and (f16 == 0).any() and f16.dtype == np.float16
    G.update(in_agg_obj_6d=pose9, root_joint=root, is_right=is_right, index=index, path=paths, batch_size=np.array(BATCH),
             agg_hand_vert_f16_bits=f16.view(np.uint16), pd_obj_rt=np.concatenate(obj_rt, 0),
             hand_reg_json=np.frombuffer(open(reg_path, 'rb').read(), np.uint8), hand_diff_json=np.frombuffer(open(diff_path, 'rb').read(), np.uint8))
    out = os.path.join(HERE, 'golden_infer.npz')
    np.savez_compressed(out, **G)
    print(out, os.path.getsize(out) // 1024, 'KiB;', {k: (v.dtype, v.shape) for k, v in G.items()})


if __name__ == '__main__':
    main()

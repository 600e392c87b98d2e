"""Fixtures of the data front end (vpho_amd/frames.py, csrc/frames.hip): ``golden_frames.npz``, data only.

Heat-maps and boxes come from the reference's OWN ``lib.utils.misc_fn``, imported unchanged under the stubs of make_golden.py plus
``cv2`` and ``natsort`` stubs (as make_golden_force_optim.py): ``HeatmapGenerator.get_heatmap``, ``AdaptiveHeatmapGenerator.__call__`` with
``cv2.resize`` replaced by a function that keeps its INPUT -- the tight map before the resize, together with the reference's own
arithmetic for its resolution and points --, ``pt2d_to_bbox2d``, ``expand_bbox2d``, ``get_rectanglular_bbox2d`` and ``check_bbox2d``.

Crop matrices: route 1 of the two the issue allows WORKED -- the real ``lib/dataset/base.py`` is loaded under a private module name
(its absent imports -- cv2, trimesh, fpsample, albumentations, natsort, timm.data.random_erasing, the renderer and the plotting helpers
-- stubbed, manopth's layer replaced by an empty class, the working directory a temporary one that holds an empty
``asset/ours/object_mesh_info.pkl``) and ``BaseDataset.get_augmentation_rotmat`` is called on a SimpleNamespace that carries ``cfg``.
Run in the build container only (needs /root/reference)."""
import importlib.util
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

HM_CASES = ((64, 2.0, 3), (16, 2.0, 1), (64, 1.5, 1))          # (S, sigma, samples)
PATCH = 256


def hm_inputs(S, sigma, n, seed):
    """per sample: 27 object points and 21 hand points in patch coordinates, a box, the hand's side.  Besides random points inside the box:
    points whose window is clipped at each edge and corner of the map, points just outside each edge, points ON the edges, and for the
    first sample a left hand (whose + 1 pushes the last column's points out of the map)"""
    r = np.random.default_rng(seed)
    out = []
    for s in range(n):
        c = np.array([PATCH / 2, PATCH / 2]) + r.uniform(-20, 20, 2)
        wh = r.uniform(60, 150, 2)
        box = np.concatenate([c - wh / 2, c + wh / 2])
        m = wh.max()
        rect = np.concatenate([c - m / 2, c + m / 2])

        def pts(J, b):
            lo, span = b[:2], b[2:] - b[:2]
            u = r.uniform(0.05, 0.95, (J, 2))
            edge = np.array([[0.0, 0.5], [1.0, 0.5], [0.5, 0.0], [0.5, 1.0], [0.001, 0.002], [0.999, 0.998], [0.01, 0.99], [0.99, 0.01],
                             [-0.03, 0.5], [1.03, 0.5], [0.5, -0.03], [0.5, 1.04], [0.97, 0.3]])
            u[:len(edge)] = edge
            return lo + u * span
        out.append(dict(obj=pts(27, rect), hand=pts(21, box), box=box, rect=rect, is_right=bool(s != 0)))
    return out


def load_reference_base(tmp):
    """the real lib/dataset/base.py under a private name; returns the module"""
    os.makedirs(os.path.join(tmp, 'asset', 'ours'), exist_ok=True)
    with open(os.path.join(tmp, 'asset', 'ours', 'object_mesh_info.pkl'), 'wb') as f:
        pickle.dump({}, f)

    class Anything:
        def __init__(self, *a, **k):
            pass

    for name in ('trimesh', 'fpsample', 'albumentations'):
        MG._stub(name)
    MG._stub('timm.data')
    MG._stub('timm.data.random_erasing', RandomErasing=Anything)
    MG._stub('manopth.manolayer', ManoLayer=Anything)
    MG._stub('lib.utils.render_fn', Pytorch3DRenderer=Anything)
    MG._stub('lib.utils.viz_fn', get_random_color=None, depth_to_rgb=None)
    spec = importlib.util.spec_from_file_location('_vpho_ref_dataset_base', os.path.join(MG.REF, 'lib', 'dataset', 'base.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from vpho_amd.assets import synthetic_assets
    assets = synthetic_assets(0)
    tmp = tempfile.mkdtemp(prefix='vpho_golden_frames_')
    MG.write_assets(tmp, assets)
    os.chdir(tmp)
    sys.argv = ['main.py']
    sys.path.insert(0, MG.REF)
    MG.install_stubs(assets)
    kept = []

    def keep_input(img, size, interpolation=None):
        kept.append(np.array(img, copy=True))
        return np.zeros((size[1], size[0], img.shape[2]), np.float32)

    MG._stub('cv2', resize=keep_input, INTER_LINEAR=1)
    MG._stub('natsort', natsorted=sorted)
    import lib.utils.misc_fn as F

    G = {'hm_cases': np.array([[S, sigma, n] for S, sigma, n in HM_CASES], np.float64)}
    for ci, (S, sigma, n) in enumerate(HM_CASES):
        sq, ad = F.HeatmapGenerator(S, sigma), F.AdaptiveHeatmapGenerator(21, sigma, S)
        G[f'hm{ci}_g'] = sq.g
        for si, d in enumerate(hm_inputs(S, sigma, n, 100 + ci)):
            p = f'hm{ci}_{si}_'
            for k in ('obj', 'hand', 'box', 'rect'):
                G[p + k] = d[k]
            G[p + 'is_right'] = np.array(d['is_right'])
            G[p + 'square'] = sq.get_heatmap(d['obj'].copy(), d['rect'].copy(), d['is_right'])
            del kept[:]
            ad(d['hand'].copy(), d['box'].copy())
            G[p + 'tight'] = np.ascontiguousarray(kept[0].transpose(2, 0, 1))            # (21, res_h, res_w)
    # box helpers
    r = np.random.default_rng(7)
    pts = r.uniform(-30, 290, (8, 21, 2))
    pts[0] = r.uniform(100, 140, (21, 2))
    pts[1] = r.uniform(0, 256, (21, 2))
    b = np.stack([F.pt2d_to_bbox2d(p, mode='x1y1x2y2') for p in pts])
    e = np.stack([F.expand_bbox2d(x, scale_factor=1.15) for x in b])
    rect = [F.get_rectanglular_bbox2d(x) for x in e]
    img = np.zeros((PATCH, PATCH, 3), np.uint8)
    G.update(box_pts=pts, box_bbox=b, box_expand=e, box_rect=np.stack([x[0] for x in rect]), box_max_wh=np.stack([x[1] for x in rect]),
             box_ok=np.array([bool(F.check_bbox2d(x[0], img)) for x in rect]))
    # crop matrices: the reference's own method
    base = load_reference_base(tmp)
    r = np.random.default_rng(11)
    crop = dict(jt2d=[], obj2d=[], K=[], jitter=[], scale=[], rot=[], patch=[], bsf=[], R3=[], M=[], Kc=[])
    for i in range(8):
        patch, bsf = (256, 1.2) if i < 6 else (224, 1.0)
        c = np.array([320.0, 240.0]) + r.uniform(-120, 120, 2)
        jt = c + r.normal(0, 35, (21, 2))
        ob = c + r.uniform(-40, 40, 2) + r.normal(0, 30, (27, 2))
        K = np.array([[r.uniform(500, 700), 0, r.uniform(300, 340)], [0, r.uniform(500, 700), r.uniform(220, 260)], [0, 0, 1]])
        jitter, scale, rot = (np.zeros(2), 1.0, 0.0) if i == 0 else (0.2 * r.uniform(-1, 1, 2), 0.2 * r.uniform() + 1, r.uniform(-1, 1) * 30 / 180 * np.pi)
        me = types.SimpleNamespace(cfg=types.SimpleNamespace(patch_size=patch, bbox_scale_factor=bsf))
        R3, M, Kc = base.BaseDataset.get_augmentation_rotmat(me, jitter, scale, rot, jt, ob, K)
        for k, v in zip(crop, (jt, ob, K, jitter, scale, rot, patch, bsf, R3, M, Kc)):
            crop[k].append(v)
    G.update({'crop_' + k: np.array(v) for k, v in crop.items()})
    out = os.path.join(HERE, 'golden_frames.npz')
    np.savez_compressed(out, **G)
    print(out, os.path.getsize(out), 'bytes;', len(G), 'arrays')


if __name__ == '__main__':
    main()

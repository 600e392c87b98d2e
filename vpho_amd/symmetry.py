"""Object symmetries for the symmetry-aware pose errors (--eval_symmetric): the padded table of rigid transforms
under which an object looks the same, numpy float64, importable without the HIP library.

The reference builds it in ``TesterObject.__init__`` (lib/engine/test.py:204-226) from ``asset/2023_NIPS_DeepSimHO/assets_models_info.json``
with ``get_symmetry_transformations`` (:103-150, the BOP toolkit's) and ``rotation_matrix`` (:59-100); ``criterion_SMCE`` (:377-398)
indexes ALL rows of an object's padded table.  Its quirks are kept, because the table is the metric's definition:
* a continuous symmetry becomes the rotations ``i = 1 .. steps - 1`` of ``steps = ceil(pi / max_sym_disc_step)``: the identity is not among
  them, so an object with a continuous symmetry has no identity in its own list;
* the discrete symmetries of the JSON are not composed with each other, only each (and the identity) with every continuous rotation;
* every object is padded with identities to the longest list; for an object shorter than the longest the pad adds the plain corner error
  as one more candidate.
Imported only when a caller asks for the symmetric errors."""
import json
import math
import os

import numpy as np

from .assets import YCB_NAMES, AssetError, _report

INFO_FILE = os.path.join('2023_NIPS_DeepSimHO', 'assets_models_info.json')
MAX_TRANSFORMS = 4096              # what vpho_obj_symmetry_multi_f64 takes per object


def axis_rotation(angle, axis):
    """(3, 3) rotation by ``angle`` about the direction ``axis`` through the origin (rotation_matrix, test.py:59-100, without the 4 x 4
    frame): cos * I + (1 - cos) * u u^T + sin * [u]x, summed in that order"""
    u = np.array(axis, dtype=np.float64).reshape(3)
    u = u / math.sqrt(np.dot(u, u))
    s, c = math.sin(angle), math.cos(angle)
    R = np.diag([c, c, c])
    R += np.outer(u, u) * (1.0 - c)
    w = u * s
    R += np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return R


def symmetry_transforms(model_info, max_sym_disc_step):
    """[(R (3, 3), t (3,)), ...] of one object's JSON entry, in the reference's order (get_symmetry_transformations, test.py:103-150): for
    the identity and then each ``symmetries_discrete`` entry (16 numbers, a row-major 4 x 4), every discretised rotation of every
    ``symmetries_continuous`` entry ({'axis', 'offset'}) applied after it -- or the discrete transform alone when there is no continuous
    symmetry.  Translations in the JSON's unit (millimetres)."""
    discrete = [(np.eye(3), np.zeros(3))]
    for sym in model_info.get('symmetries_discrete', ()):
        m = np.asarray(sym, np.float64).reshape(4, 4)
        discrete.append((m[:3, :3], m[:3, 3]))
    continuous = []
    for sym in model_info.get('symmetries_continuous', ()):
        offset = np.asarray(sym['offset'], np.float64).reshape(3)
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        for i in range(1, steps):                  # the reference starts at 1: no identity
            R = axis_rotation(i * step, sym['axis'])
            continuous.append((R, -R.dot(offset) + offset))
    if not continuous:
        return discrete
    return [(Rc.dot(Rd), Rc.dot(td) + tc) for Rd, td in discrete for Rc, tc in continuous]


def info_key(name):
    """the JSON key of a YCB class: the reference's YCB_ID (lib/dataset/base.py:40-63), i.e. object i of assets.YCB_NAMES reads str(i + 1)"""
    return str(YCB_NAMES.index(name) + 1)


def symmetry_table(infos, names, max_sym_disc_step):
    """R (n_obj, K, 3, 3), t (n_obj, K, 3) float64 for the classes ``names`` (TesterObject.__init__, test.py:207-226): each object's
    transforms, padded with identities to the longest list K among them, translations in metres (the JSON holds millimetres)."""
    lists = [symmetry_transforms(infos[info_key(n)], max_sym_disc_step) for n in names]
    K = max(len(l) for l in lists)
    R = np.tile(np.eye(3), (len(lists), K, 1, 1))
    t = np.zeros((len(lists), K, 3))
    for i, l in enumerate(lists):
        for k, (Rk, tk) in enumerate(l):
            R[i, k] = Rk
            t[i, k] = np.asarray(tk, np.float64).reshape(3) / 1000.0
    return R, t


def synthetic_model_info(names=YCB_NAMES, seed=0):
    """a model-info for the synthetic boxes (assets.synthetic_ycb): every object has the three half-turns about its box axes, which are
    true of a box centred on the origin; object i with (i + seed) % 3 == 0 also DECLARES a continuous symmetry about z, which is not
    true of a box -- it is there so that the long table (hundreds of transforms) is exercised without the real file"""
    half_turns = []
    for ax in range(3):
        m = -np.eye(4)
        m[ax, ax] = m[3, 3] = 1.0
        half_turns.append([float(x) for x in m.reshape(-1)])
    infos = {}
    for n in names:
        i = YCB_NAMES.index(n)
        infos[str(i + 1)] = {'symmetries_discrete': [list(h) for h in half_turns]}
        if (i + seed) % 3 == 0:
            infos[str(i + 1)]['symmetries_continuous'] = [{'axis': [0, 0, 1], 'offset': [0, 0, 0]}]
    return infos


def load_symmetries(asset_root, names=YCB_NAMES, seed=0):
    """the model-info {str(class id): entry} of ``names``: ``<asset_root>/2023_NIPS_DeepSimHO/assets_models_info.json`` when it exists (a
    file that cannot be read, or lacks one of the classes, raises AssetError), else ``synthetic_model_info``, said once on stderr.  Not a
    part of ``load_assets``: only the symmetric errors need it."""
    path = os.path.join(asset_root, INFO_FILE)
    if os.path.exists(path):
        try:
            with open(path) as f:
                infos = json.load(f)
        except Exception as e:
            raise AssetError(f'symmetries: {path} exists but cannot be parsed ({type(e).__name__}: {e})') from e
        missing = [n for n in names if not isinstance(infos, dict) or info_key(n) not in infos]
        if missing:
            raise AssetError(f'symmetries: {path} has no entry for {[(n, info_key(n)) for n in missing]}')
        return infos
    _report(f'object symmetries: no file {os.path.abspath(path)!r} -> SYNTHETIC model-info (seed {seed}): three half-turns per box, and a '
            f'declared continuous z symmetry for every third object, which is not true of a box')
    return synthetic_model_info(names, seed)

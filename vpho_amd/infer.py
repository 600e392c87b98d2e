"""Host side of ``--mode infer`` (the reference's ``Trainer.infer``, lib/engine/train_diff_hand_obj.py:359-444): what leaves the project.

The device side is one kernel and one copy per batch (ops.InferPacker, vpho_infer_pack_f32); everything here works on the numpy records
it delivers (ops.infer_record_dtype): per-rank shards, the merge on rank 0, and the three writers --
* ``submit/hand_reg.zip`` / ``submit/hand_diff.zip``: the HO3D-style submission JSON ``[xyz_list, verts_list]`` of the regression and the
  aggregated hand in OpenGL convention, ordered by image index, bytes as the reference's ``dump`` (:872-880) writes them;
* ``my-prediction_align-<clean_data_mode>.pkl``: one dict per batch (:378-385), the input of the downstream physics evaluations.
No GPU is needed for anything in this module.
"""
import json
import os
import pickle
import sys
import zipfile

import numpy as np

# lib/utils/transform_fn.py:156-158.  An INTEGER matrix, as there: ``fp32 array @ int64 matrix`` promotes to float64, so the numbers that
# reach the JSON are the float64 images of the fp32 predictions, rounded to 6 decimals in float64 (0.068967, not 0.06896700114011765)
OPENGL_TO_OPENCV = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])

RECORD_FIELDS = ('reg_joint', 'reg_vert', 'agg_joint', 'agg_vert', 'agg_vert_f16', 'pd_obj_rt')


def submission_json(joints, verts):
    """the text of one submission file: joints (N,21,3), verts (N,778,3) fp32 in the CAMERA frame, already ordered by index.  The OpenGL
    step (:387-390) and ``dump`` (:872-880): ``json.dump([[np.around(x, 6).tolist() ...], [...]])``."""
    xyz = [np.around(x @ OPENGL_TO_OPENCV, decimals=6).tolist() for x in joints]
    vts = [np.around(x @ OPENGL_TO_OPENCV, decimals=6).tolist() for x in verts]
    return json.dumps([xyz, vts])


def write_submission_zip(path, joints, verts):
    """``<name>.zip`` holding ``<name>.json`` (what ``zip -j`` leaves, :432-435), written with zipfile: no shell, no bare .json left behind"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    member = os.path.basename(path)[:-len('.zip')] + '.json'
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        z.writestr(member, submission_json(joints, verts))
    return path


def prediction_batches(rec, index, path, batch_sizes):
    """the list the reference pickles (:378-385,392,443-444): per batch ``index`` (n,) int64, ``path`` (list of n str), ``pd_obj_rt``
    (n,3,4) float64, ``pd_hand_vert`` (n,778,3) float16, ``pd_hand_joint`` (n,21,3) float32 -- in batch order, NOT sorted"""
    res, o = [], 0
    for n in batch_sizes:
        n = int(n)
        s = slice(o, o + n)
        res.append({'index': np.ascontiguousarray(index[s], dtype=np.int64), 'path': [str(p) for p in path[s]],
                    'pd_obj_rt': np.ascontiguousarray(rec['pd_obj_rt'][s]), 'pd_hand_vert': np.ascontiguousarray(rec['agg_vert_f16'][s]),
                    'pd_hand_joint': np.ascontiguousarray(rec['agg_joint'][s])})
        o += n
    assert o == len(index), (o, len(index))
    return res


def write_prediction_pickle(path, batches):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump(batches, f)
    return path


def shard_path(save_dir, rank):
    return os.path.join(save_dir, 'shards', f'rank{rank}.npz')


def write_shard(save_dir, rank, rec, index, path, batch_sizes, has_index):
    """one rank's records: the fields of the record dtype as plain arrays + image identity.  No collective carries them (the DexYCB test
    split is 78 k images x 24 KB = 1.9 GB)."""
    p = shard_path(save_dir, rank)
    os.makedirs(os.path.dirname(p), exist_ok=True)
    tmp = p + '.tmp.npz'
    np.savez(tmp, index=np.asarray(index, np.int64), path=np.asarray(list(path), dtype=np.str_), batch_sizes=np.asarray(batch_sizes, np.int64),
             has_index=np.array(bool(has_index)), **{k: np.ascontiguousarray(rec[k]) for k in RECORD_FIELDS})
    os.replace(tmp, p)                     # a reader never sees half a file
    return p


def merge_shards(paths, err=None):
    """Shards (files of write_shard, or dicts with the same keys) in rank order -> (records by field, index, path, batch_sizes, order, gaps).
    records / index / path / batch_sizes: all ranks' images in batch order, rank 0 first (the pickle's order).
    A shard written without a data-set ``index`` holds its own running positions; they become rank-major positions here (each rank's
    shifted by the image count of the ranks before it).
    order: positions into the above, sorted by index, the FIRST occurrence of an index kept (a DistributedSampler pads its last batches
    with repeats; accelerate's gather_for_metrics drops them, to the same effect).
    gaps: the indices of 0..max that no image carries, also named on ``err`` (stderr) -- not an error here; the reference's
    ``collector_hand[i]`` (:422-426) raises KeyError at the first one."""
    err = sys.stderr if err is None else err
    fields = {k: [] for k in RECORD_FIELDS}
    index, path, sizes, seen = [], [], [], 0
    for p in paths:
        z = p if isinstance(p, dict) else np.load(p)              # a dict: a rank's records still in memory (single-process runs)
        idx = np.asarray(z['index'], np.int64)
        index.append(idx if bool(z['has_index']) else idx + seen)
        path += [str(s) for s in z['path']]
        sizes += [int(n) for n in z['batch_sizes']]
        for k in RECORD_FIELDS:
            fields[k].append(np.asarray(z[k]))
        seen += idx.shape[0]
        if not isinstance(p, dict):
            z.close()
    index = np.concatenate(index) if index else np.zeros(0, np.int64)
    rec = {k: np.concatenate(v, 0) for k, v in fields.items()}
    srt = np.argsort(index, kind='stable')                                  # stable: among equal indices the first occurrence leads
    keep = np.ones(srt.shape[0], bool)
    keep[1:] = index[srt][1:] != index[srt][:-1]
    order = srt[keep]
    dup = int((~keep).sum())
    if dup:
        print(f'infer: {dup} image(s) carry an index seen before (sampler padding): first occurrence kept', file=err)
    have = index[order]
    gaps = np.setdiff1d(np.arange(0, int(have.max()) + 1 if have.size else 0, dtype=np.int64), have)
    if have.size and have.min() < 0:
        print(f'infer: {int((have < 0).sum())} negative image indices', file=err)
    if gaps.size:
        head = ', '.join(str(int(g)) for g in gaps[:20]) + (', ...' if gaps.size > 20 else '')
        print(f'infer: {gaps.size} of the indices 0..{int(have.max())} are missing from the predictions: {head} '
              f'(the submission lists hold {have.size} entries, in index order)', file=err)
    return rec, index, path, sizes, order, gaps


def write_outputs(save_dir, clean_data_mode, rec, index, path, batch_sizes, order):
    """the three files of rank 0; returns {name: path}"""
    files = {
        'hand_reg': write_submission_zip(os.path.join(save_dir, 'submit', 'hand_reg.zip'), rec['reg_joint'][order], rec['reg_vert'][order]),
        'hand_diff': write_submission_zip(os.path.join(save_dir, 'submit', 'hand_diff.zip'), rec['agg_joint'][order], rec['agg_vert'][order]),
        'prediction': write_prediction_pickle(os.path.join(save_dir, f'my-prediction_align-{clean_data_mode}.pkl'),
                                              prediction_batches(rec, index, path, batch_sizes)),
    }
    return files


def read_submission_zip(path):
    """(member name, bytes) of a submission zip"""
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
        assert len(names) == 1, names
        return names[0], z.read(names[0])

"""--mode infer without a GPU: the JSON / zip / pickle writers against the reference's own bytes (tests/golden/golden_infer.npz,
make_golden_infer.py), the shard merge, the command line, and the new kernel's compiler usage report."""
import io
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_infer.npz')))


def _records(G):
    """the fixture's post-processed arrays under the record's field names"""
    return {'reg_joint': G['post_reg_hand_joint'], 'reg_vert': G['post_reg_hand_vert'], 'agg_joint': G['post_agg_hand_joint'],
            'agg_vert': G['post_agg_hand_vert'], 'agg_vert_f16': G['agg_hand_vert_f16_bits'].view(np.float16), 'pd_obj_rt': G['pd_obj_rt']}


def test_fixture_exercises_the_half_conversion_edges(G):
    """what the issue asks of the fixture: two left hands, a shuffled index, values next to a rounding tie, above 65504, below 6e-8"""
    assert (~G['is_right']).sum() >= 2
    idx = G['index']
    assert sorted(idx.tolist()) == list(range(6)) and idx.tolist() != list(range(6))
    v = G['post_agg_hand_vert'].astype(np.float64).reshape(-1)
    assert (np.abs(v) > 65504).any() and ((np.abs(v) < 6e-8) & (v != 0)).any()
    # a value within half an fp16 ulp of a tie: between 1 and 2 the halves are 2^-10 apart, ties sit at odd multiples of 2^-11
    near = v[(np.abs(v) > 1) & (np.abs(v) < 2)]
    frac = np.abs(near) / 2.0 ** -11
    assert ((np.abs(frac - np.round(frac)) < 0.5) & (np.round(frac) % 2 == 1)).any()
    h = G['agg_hand_vert_f16_bits'].view(np.float16)
    assert np.isinf(h).any() and ((h != 0) & (np.abs(h.astype(np.float64)) < 6.2e-5)).any()          # overflow and subnormal results


def test_submission_json_reproduces_the_reference_bytes(G, tmp_path):
    from vpho_amd import infer as INF
    rec = _records(G)
    order = np.argsort(G['index'], kind='stable')
    for name, j, v in (('hand_reg', 'reg_joint', 'reg_vert'), ('hand_diff', 'agg_joint', 'agg_vert')):
        want = G[name + '_json'].tobytes()
        assert INF.submission_json(rec[j][order], rec[v][order]).encode() == want
        p = INF.write_submission_zip(str(tmp_path / 'submit' / f'{name}.zip'), rec[j][order], rec[v][order])
        member, data = INF.read_submission_zip(p)
        assert member == f'{name}.json' and data == want
    assert sorted(os.listdir(tmp_path / 'submit')) == ['hand_diff.zip', 'hand_reg.zip']          # no bare .json left behind


def test_prediction_pickle_has_the_reference_layout(G, tmp_path):
    from vpho_amd import infer as INF
    rec, bs = _records(G), int(G['batch_size'])
    p = INF.write_prediction_pickle(str(tmp_path / 'my-prediction_align-2023_CVPR_HFL.pkl'),
                                    INF.prediction_batches(rec, G['index'], G['path'], [bs, bs]))
    got = pickle.load(open(p, 'rb'))
    assert isinstance(got, list) and len(got) == 2
    for b, d in enumerate(got):
        s = slice(b * bs, (b + 1) * bs)
        assert list(d.keys()) == ['index', 'path', 'pd_obj_rt', 'pd_hand_vert', 'pd_hand_joint']
        assert d['index'].dtype == np.int64 and d['index'].tolist() == G['index'][s].tolist()
        assert d['path'] == G['path'][s].tolist()
        assert d['pd_obj_rt'].dtype == G['pd_obj_rt'].dtype == np.float64 and d['pd_obj_rt'].shape == (bs, 3, 4)
        assert d['pd_obj_rt'].tobytes() == G['pd_obj_rt'][s].tobytes()
        assert d['pd_hand_vert'].dtype == np.float16 and d['pd_hand_vert'].shape == (bs, 778, 3)
        assert d['pd_hand_vert'].view(np.uint16).tobytes() == G['agg_hand_vert_f16_bits'][s].tobytes()
        assert d['pd_hand_joint'].dtype == np.float32 and d['pd_hand_joint'].tobytes() == G['post_agg_hand_joint'][s].tobytes()


def test_numpy_half_cast_of_block_a_is_the_fixture(G):
    """block B's rule stated on the host: astype(np.float16) of the post-processed fp32 vertices gives the fixture's bits"""
    with np.errstate(over='ignore'):
        assert (G['post_agg_hand_vert'].astype(np.float16).view(np.uint16) == G['agg_hand_vert_f16_bits']).all()


def _shard(rng, index, sizes, tag):
    n = len(index)
    rec = {'reg_joint': rng.normal(size=(n, 21, 3)).astype(np.float32), 'reg_vert': rng.normal(size=(n, 778, 3)).astype(np.float32),
           'agg_joint': rng.normal(size=(n, 21, 3)).astype(np.float32), 'agg_vert': rng.normal(size=(n, 778, 3)).astype(np.float32),
           'pd_obj_rt': rng.normal(size=(n, 3, 4))}
    rec['agg_vert_f16'] = rec['agg_vert'].astype(np.float16)
    return rec, np.asarray(index, np.int64), [f'{tag}/{i}.jpg' for i in index], sizes


def test_shard_merge_sorts_keeps_the_first_duplicate_and_names_the_gap(tmp_path):
    from vpho_amd import infer as INF
    rng = np.random.default_rng(3)
    # indices 0..9 without 6; 4 appears on both ranks (rank 0 first)
    r0 = _shard(rng, [7, 0, 4, 9, 2], [3, 2], 'r0')
    r1 = _shard(rng, [3, 8, 1, 4, 5], [2, 3], 'r1')
    for r, (rec, idx, path, sizes) in enumerate((r0, r1)):
        INF.write_shard(str(tmp_path), r, rec, idx, path, sizes, True)
    assert sorted(os.listdir(tmp_path / 'shards')) == ['rank0.npz', 'rank1.npz']
    err = io.StringIO()
    rec, index, path, sizes, order, gaps = INF.merge_shards([INF.shard_path(str(tmp_path), r) for r in range(2)], err=err)
    assert index.tolist() == [7, 0, 4, 9, 2, 3, 8, 1, 4, 5] and sizes == [3, 2, 2, 3]          # batch order, rank 0 first
    assert index[order].tolist() == [0, 1, 2, 3, 4, 5, 7, 8, 9]
    assert order[4] == 2 and path[order[4]] == 'r0/4.jpg'                                     # the first occurrence of index 4
    assert gaps.tolist() == [6]
    msg = err.getvalue()
    assert 'missing' in msg and ' 6 ' in msg.replace(':', ' ') and 'first occurrence kept' in msg
    allrec = {k: np.concatenate([r0[0][k], r1[0][k]]) for k in INF.RECORD_FIELDS}
    for k in INF.RECORD_FIELDS:
        assert rec[k].dtype == allrec[k].dtype and rec[k].tobytes() == allrec[k].tobytes()
    # the files written from the merge: JSON lists by index, pickle by batch
    files = INF.write_outputs(str(tmp_path), 'stable_grasping', rec, index, path, sizes, order)
    assert os.path.basename(files['prediction']) == 'my-prediction_align-stable_grasping.pkl'
    import json
    xyz, verts = json.loads(INF.read_submission_zip(files['hand_diff'])[1])
    assert len(xyz) == len(verts) == 9
    want = np.around(allrec['agg_joint'][order].astype(np.float64) * np.array([1.0, -1.0, -1.0]), 6)
    assert np.array_equal(np.asarray(xyz), want + 0.0)
    got = pickle.load(open(files['prediction'], 'rb'))
    assert [d['index'].tolist() for d in got] == [[7, 0, 4], [9, 2], [3, 8], [1, 4, 5]]


def test_shards_without_a_dataset_index_get_rank_major_positions():
    from vpho_amd import infer as INF
    rng = np.random.default_rng(4)
    shards = []
    for r, n in enumerate((3, 2)):
        rec, idx, path, sizes = _shard(rng, list(range(n)), [n], f'r{r}')
        shards.append(dict(index=idx, path=path, batch_sizes=sizes, has_index=False, **rec))
    rec, index, path, sizes, order, gaps = INF.merge_shards(shards, err=io.StringIO())
    assert index.tolist() == [0, 1, 2, 3, 4] and order.tolist() == [0, 1, 2, 3, 4] and gaps.size == 0


def _parse(argv):
    code = 'import sys; from vpho_amd.configs.args import cfg; print(cfg.mode, cfg.clean_data_mode)'
    return subprocess.run([sys.executable, '-c', code] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_argparse_takes_clean_data_mode_with_the_reference_choices():
    r = _parse(['--mode', 'infer', '--clean_data_mode', '2023_NIPS_DeepSimHO'])
    assert r.returncode == 0 and r.stdout.split() == ['infer', '2023_NIPS_DeepSimHO'], r.stderr[-800:]
    r = _parse(['--mode', 'infer'])
    assert r.returncode == 0 and r.stdout.split() == ['infer', '2023_CVPR_HFL'], r.stderr[-800:]
    r = _parse(['--mode', 'infer', '--clean_data_mode', '2031_made_up'])
    assert r.returncode != 0 and 'invalid choice' in r.stderr
    from vpho_amd.configs.args import CLEAN_DATA_MODES
    assert CLEAN_DATA_MODES == ('2023_CVPR_HFL', '2022_CVPR_ArtiBoost', '2023_WACV_DMA', 'stable_grasping', '2023_NIPS_DeepSimHO')


def test_infer_pack_kernel_has_no_spill_and_no_scratch():
    import __graft_entry__ as g
    g.build()
    txt = open(os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'infer_pack.hip.usage.txt')).read()
    assert 'infer_pack_kernel' in txt
    field = lambda name: [int(v) for v in re.findall(name + r'[^:\n]*: (\d+)', txt)]
    assert field('VGPRs Spill') == [0] and field('SGPRs Spill') == [0] and field('ScratchSize') == [0] and field('LDS Size') == [0]


def test_record_layout_matches_the_header():
    """ops.infer_record_dtype against vpho_infer_record_bytes: 4794 floats, 2334 halves padded to 8 bytes, 12 doubles"""
    import __graft_entry__ as g
    g.build()
    from vpho_amd import ops
    dt = ops.infer_record_dtype()
    assert dt.itemsize == 23944 == ops.lib.vpho_infer_record_bytes(21, 778) and dt.itemsize % 8 == 0
    assert [dt.fields[k][1] for k in dt.names] == [0, 252, 9588, 9840, 19176, 23848]
    assert ops.lib.vpho_infer_record_bytes(21, 777) == -1 and ops.lib.vpho_infer_record_bytes(0, 778) == -1

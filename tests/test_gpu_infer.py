"""--mode infer on the GPU: the record kernel (vpho_infer_pack_f32) against the reference's own arrays (tests/golden/golden_infer.npz),
its shapes and refusals, and ``Trainer.infer`` end to end -- files against ``Engine.predict`` + ``evaluate.postprocess`` +
``ops.obj_9d_to_rt`` on the same batches, run-to-run identity, graph replay on / off, and ``main.py`` in child processes."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ['--sample_num', '4', '--sampling_steps', '5', '--topk_hand', '8', '--topk_obj', '3', '--sample_T0', '0.2',
        '--eval_batch_size', '2', '--num_batches', '2', '--random_seed', '7']
# the bound of the existing test through vpho_obj_9d_to_rt_f64 against an fp64 restatement of the reference:
# tests/test_gpu_metrics.py::test_object_metric_block_of_the_evaluation_rows, _check_obj(..., nn_atol=1e-7)
OBJ_RT_ATOL = 1e-7


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_infer.npz')))


def _pack(packer, out, root, is_right, slot=0):
    packer.pack(out, {'root_joint': root, 'is_right': is_right}, slot=slot)
    return packer.collect(slot).copy()


def _random_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    out = {'reg_hand_joint': torch.randn(n, 21, 3, generator=g) * 0.04, 'reg_hand_vert': torch.randn(n, 778, 3, generator=g) * 0.04,
           'agg_hand_joint': torch.randn(n, 21, 3, generator=g) * 0.04, 'agg_hand_vert': torch.randn(n, 778, 3, generator=g) * 0.04,
           'agg_obj_6d': torch.randn(n, 9, generator=g, dtype=torch.float64)}
    root = torch.randn(n, 3, generator=g) * 0.05 + torch.tensor([0.0, 0.0, 0.6])
    is_right = torch.rand(n, generator=g) < 0.5
    return {k: v.cuda() for k, v in out.items()}, root.cuda(), is_right.cuda()


def _check_against_host(rec, out, root, is_right):
    """blocks A, B, C of `rec` against the existing evaluate.postprocess / numpy half cast / ops.obj_9d_to_rt"""
    from vpho_amd import evaluate as E
    from vpho_amd import ops
    pp = E.postprocess({**out, 'diff_final_hand_joint': out['agg_hand_joint'][:, None]}, root, is_right)
    for f, k in (('reg_joint', 'reg_hand_joint'), ('reg_vert', 'reg_hand_vert'), ('agg_joint', 'agg_hand_joint'), ('agg_vert', 'agg_hand_vert')):
        assert rec[f].tobytes() == pp[k].cpu().numpy().tobytes(), f
    with np.errstate(over='ignore'):
        assert (rec['agg_vert_f16'].view(np.uint16) == rec['agg_vert'].astype(np.float16).view(np.uint16)).all()
    rt = ops.obj_9d_to_rt(out['agg_obj_6d'].contiguous(), root.contiguous())
    assert rec['pd_obj_rt'].tobytes() == rt.cpu().numpy().tobytes()


def test_kernel_against_the_reference_fixture(G):
    from vpho_amd import ops
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = {k: d(G['in_' + k]) for k in ('reg_hand_joint', 'reg_hand_vert', 'agg_hand_joint', 'agg_hand_vert', 'agg_obj_6d')}
    root, is_right = d(G['root_joint']), d(G['is_right'])
    packer = ops.InferPacker('cuda', max_batch=8)
    rec = _pack(packer, out, root, is_right)
    assert rec.shape == (6,) and rec.dtype.itemsize == 23944
    # block A: the reference's postprocess, bit for bit
    for f, k in (('reg_joint', 'reg_hand_joint'), ('reg_vert', 'reg_hand_vert'), ('agg_joint', 'agg_hand_joint'), ('agg_vert', 'agg_hand_vert')):
        assert rec[f].dtype == np.float32 and rec[f].tobytes() == G['post_' + k].tobytes(), f
    # block B: numpy's astype(np.float16) of it, every element (ties, overflow to inf, subnormals)
    got = rec['agg_vert_f16'].view(np.uint16)
    bad = np.argwhere(got != G['agg_hand_vert_f16_bits'])
    assert bad.size == 0, (bad[:5], [(hex(got[tuple(b)]), hex(G['agg_hand_vert_f16_bits'][tuple(b)]), G['post_agg_hand_vert'][tuple(b)]) for b in bad[:5]])
    # block C: ops.obj_9d_to_rt bit for bit, the reference's fp64 pd_obj_rt within the existing bound
    rt = ops.obj_9d_to_rt(out['agg_obj_6d'], root)
    assert rec['pd_obj_rt'].dtype == np.float64 and rec['pd_obj_rt'].tobytes() == rt.cpu().numpy().tobytes()
    err = np.abs(rec['pd_obj_rt'] - G['pd_obj_rt']).max()
    print(f'block C vs the reference pd_obj_rt: max abs {err:.3e} (bound {OBJ_RT_ATOL:g})')
    assert err <= OBJ_RT_ATOL
    # the padding between blocks B and C is written (zero), so whole records compare equal run to run
    # (read in the pinned buffer itself: numpy copies a structured array field by field and leaves the gaps alone)
    raw = packer.host[0].numpy()[:6 * 23944].reshape(6, -1)
    assert (raw[:, 19176 + 4668:23848] == 0).all()
    _pack(packer, out, root, is_right, slot=2)
    assert packer.host[2].numpy()[:6 * 23944].tobytes() == raw.tobytes()


@pytest.mark.parametrize('n', [1, 65, 96])
def test_kernel_shapes(n):
    from vpho_amd import ops
    packer = ops.InferPacker('cuda', max_batch=96)
    out, root, is_right = _random_inputs(n, seed=n)
    rec = _pack(packer, out, root, is_right, slot=n % 3)
    assert rec.shape == (n,)
    _check_against_host(rec, out, root, is_right)


def test_a_batch_larger_than_max_batch_is_refused():
    from vpho_amd import ops
    packer = ops.InferPacker('cuda', max_batch=4)
    out, root, is_right = _random_inputs(5, seed=0)
    with pytest.raises(ops.VphoError, match='max_batch = 4'):
        packer.pack(out, {'root_joint': root, 'is_right': is_right})
    with pytest.raises(ops.VphoError, match='nothing was packed'):
        packer.collect(1)
    with pytest.raises(ops.VphoError, match='slot 3'):
        packer.pack({k: v[:2] for k, v in out.items()}, {'root_joint': root[:2], 'is_right': is_right[:2]}, slot=3)


# ------------------------------------------------------------------------------------------------------------ Trainer.infer
KEYS = ('sample_num', 'sampling_steps', 'topk_hand', 'topk_obj', 'sample_T0', 'eval_batch_size', 'num_batches', 'random_seed', 'checkpoint',
        'clean_data_mode')


@pytest.fixture()
def small_cfg():
    from vpho_amd.configs.args import cfg
    saved = {k: getattr(cfg, k) for k in KEYS}
    cfg.sample_num, cfg.sampling_steps, cfg.topk_hand, cfg.topk_obj, cfg.sample_T0 = 4, 5, 8, 3, 0.2
    cfg.eval_batch_size, cfg.num_batches, cfg.random_seed, cfg.checkpoint, cfg.clean_data_mode = 2, 3, 7, None, '2023_CVPR_HFL'
    yield cfg
    for k, v in saved.items():
        setattr(cfg, k, v)


INDEX = [[41, 3], [17, 0], [8]]                       # shuffled across batches; the last batch is ragged


def _batches(t, with_object=True):
    from vpho_amd.synth import synth_batch
    res = []
    for i, idx in enumerate(INDEX):
        b = synth_batch(2, t.assets, seed=7 + i, rank=0)
        b = {k: v[:len(idx)] for k, v in b.items()}
        b['index'] = torch.tensor(idx)
        b['rgb_path'] = [f'img/{j:05d}.jpg' for j in idx]
        if not with_object:
            del b['gt_obj_rt']
        assert 'gt_joint' not in b and 'gt_hand_vert' not in b          # infer needs no hand ground truth
        res.append(b)
    return res


def _read(res):
    from vpho_amd import infer as INF
    files = res['files']
    reg, diff = INF.read_submission_zip(files['hand_reg']), INF.read_submission_zip(files['hand_diff'])
    assert reg[0] == 'hand_reg.json' and diff[0] == 'hand_diff.json'
    return reg[1], diff[1], pickle.load(open(files['prediction'], 'rb'))


def _same_pickle(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x.keys()) == list(y.keys()) and x['path'] == y['path']
        for k in ('index', 'pd_obj_rt', 'pd_hand_vert', 'pd_hand_joint'):
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), k


def test_infer_end_to_end_against_predict(small_cfg, tmp_path, capfd):
    from vpho_amd import evaluate as E
    from vpho_amd import ops
    from vpho_amd.model.engine import Engine
    from vpho_amd.trainer import Trainer
    t = Trainer(small_cfg)
    batches = _batches(t)
    torch.manual_seed(11)                                     # the prior comes from the CPU default generator
    res = t.infer(loader=iter(batches), save_dir=str(tmp_path / 'run'))
    stdout = capfd.readouterr().out
    assert isinstance(res, dict), 'Trainer.infer must return the INFER_JSON dict on rank 0 (the parent returns metric rows and writes nothing)'
    line = [l for l in stdout.splitlines() if l.startswith('INFER_JSON ')]
    assert len(line) == 1 and json.loads(line[0][len('INFER_JSON '):]) == json.loads(json.dumps(res))
    assert 'EVAL_JSON' not in stdout and 'Mean Pose' in stdout
    assert res['images'] == 5 and res['world'] == 1 and res['images_per_s'] > 0 and set(res['object']) == set(ops.OBJ_METRIC_NAMES)
    assert sorted(os.listdir(tmp_path / 'run' / 'submit')) == ['hand_diff.zip', 'hand_reg.zip']
    assert os.path.basename(res['files']['prediction']) == 'my-prediction_align-2023_CVPR_HFL.pkl'
    reg, diff, pkl = _read(res)
    # the same batches, sequentially, through Engine.predict and the EXISTING post-processing
    eng = Engine(t.model)
    torch.manual_seed(11)
    want = []
    for b in batches:
        gb = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
        n = gb['rgb'].shape[0]
        nh, no = torch.randn(n * small_cfg.sample_num, 96), torch.randn(n * small_cfg.sample_num, 9)
        out = eng.predict(gb, noise_hand=nh, noise_obj=no)
        pp = E.postprocess(out, gb['root_joint'], gb['is_right'])
        rt = ops.obj_9d_to_rt(out['agg_obj_6d'].double().contiguous(), gb['root_joint'].float().contiguous())
        want.append(({k: v.cpu().numpy() for k, v in pp.items()}, rt.cpu().numpy()))
    flat = [i for idx in INDEX for i in idx]
    order = np.argsort(flat, kind='stable')
    cat = lambda k: np.concatenate([w[0][k] for w in want])[order]
    gl = np.array([1.0, -1.0, -1.0])
    for data, kj, kv in ((reg, 'reg_hand_joint', 'reg_hand_vert'), (diff, 'agg_hand_joint', 'agg_hand_vert')):
        xyz, verts = json.loads(data)
        assert len(xyz) == len(verts) == 5                    # ordered by index: 0, 3, 8, 17, 41
        for got, k in ((xyz, kj), (verts, kv)):
            w = cat(k)
            assert w.dtype == np.float32
            got = np.asarray(got) * gl                        # back to the camera frame
            assert np.array_equal(got, np.around(w.astype(np.float64), 6) + 0.0)
            # "un-rounded": the 6-decimal value identifies the fp32 number wherever the fp32 grid is coarser than 1e-6 -- and it is within
            # 5e-7 of it everywhere
            assert np.abs(got - w.astype(np.float64)).max() <= 5.0000001e-7
    assert len(pkl) == 3
    for d, idx, (pp, rt) in zip(pkl, INDEX, want):
        assert d['index'].tolist() == idx and d['path'] == [f'img/{j:05d}.jpg' for j in idx]
        assert d['pd_hand_joint'].dtype == np.float32 and d['pd_hand_joint'].tobytes() == pp['agg_hand_joint'].tobytes()
        assert d['pd_hand_vert'].dtype == np.float16 and d['pd_hand_vert'].tobytes() == pp['agg_hand_vert'].astype(np.float16).tobytes()
        assert d['pd_obj_rt'].dtype == np.float64 and d['pd_obj_rt'].tobytes() == rt.tobytes()

    # a second run with the same seed: byte-identical JSON members, equal pickles
    torch.manual_seed(11)
    res2 = t.infer(loader=iter(batches), save_dir=str(tmp_path / 'run2'))
    reg2, diff2, pkl2 = _read(res2)
    assert reg2 == reg and diff2 == diff
    _same_pickle(pkl, pkl2)
    assert res2['object'] == res['object']

    # batches without object ground truth: the files are the same, the object table is skipped with one line
    capfd.readouterr()
    torch.manual_seed(11)
    res3 = t.infer(loader=iter(_batches(t, with_object=False)), save_dir=str(tmp_path / 'run3'))
    out3 = capfd.readouterr().out
    assert res3['object'] is None and out3.count('Object Evaluation: skipped') == 1
    reg3, diff3, pkl3 = _read(res3)
    assert reg3 == reg and diff3 == diff
    _same_pickle(pkl, pkl3)

    # eval still wants its ground truth
    with pytest.raises(KeyError, match='gt_joint'):
        t.eval(loader=iter(batches))


def test_infer_with_and_without_graph_replay_writes_the_same_files(small_cfg, tmp_path):
    from vpho_amd.trainer import Trainer
    old = os.environ.get('VPHO_GRAPHS')
    got = {}
    try:
        for graphs in ('1', '0'):
            os.environ['VPHO_GRAPHS'] = graphs
            t = Trainer(small_cfg)
            torch.manual_seed(5)
            got[graphs] = _read(t.infer(save_dir=str(tmp_path / f'graphs{graphs}')))          # the synthetic batches of cfg.num_batches
    finally:
        if old is None:
            del os.environ['VPHO_GRAPHS']
        else:
            os.environ['VPHO_GRAPHS'] = old
    assert got['1'][0] == got['0'][0] and got['1'][1] == got['0'][1]
    _same_pickle(got['1'][2], got['0'][2])
    assert [d['index'].tolist() for d in got['1'][2]] == [[0, 1], [2, 3], [4, 5]] and got['1'][2][0]['path'] == ['', '']


def _run_main(mode, extra, cwd_out):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--mode', mode, '--model', 'vpho_net', '--output_dir', cwd_out] + ARGS + extra,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_main_infer_and_main_eval_in_child_processes(tmp_path):
    out_dir = str(tmp_path / 'out')
    stdout = _run_main('infer', ['--clean_data_mode', 'stable_grasping', '--mark', 'tst'], out_dir)
    line = [l for l in stdout.splitlines() if l.startswith('INFER_JSON ')]
    assert len(line) == 1 and 'EVAL_JSON' not in stdout, stdout[-2000:]
    res = json.loads(line[0][len('INFER_JSON '):])
    assert res['images'] == 4 and res['world'] == 1 and res['object'] is not None
    for p in res['files'].values():
        assert os.path.isfile(p) and os.path.getsize(p) > 0 and os.path.abspath(p).startswith(os.path.abspath(out_dir))
    runs = os.listdir(out_dir)
    assert len(runs) == 1 and runs[0].endswith('_tst_infer_vpho_net')
    assert os.path.basename(res['files']['prediction']) == 'my-prediction_align-stable_grasping.pkl'
    xyz, verts = json.loads(__import__('vpho_amd.infer', fromlist=['x']).read_submission_zip(res['files']['hand_diff'])[1])
    assert np.asarray(xyz).shape == (4, 21, 3) and np.asarray(verts).shape == (4, 778, 3)
    # eval is untouched: its line, and nothing written under output_dir
    eval_dir = str(tmp_path / 'out_eval')
    stdout = _run_main('eval', [], eval_dir)
    assert len([l for l in stdout.splitlines() if l.startswith('EVAL_JSON ')]) == 1 and 'INFER_JSON' not in stdout
    assert not os.path.exists(eval_dir) or not os.listdir(eval_dir)

"""Multi-hypothesis evaluation (--eval_best) without a GPU: the wide row layout, its tables, its ragged world-2 gather, the flag,
and the compiler's resource report of the new kernels."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _wide_rows(n, seed=0):
    from vpho_amd import evaluate as E
    g = torch.Generator().manual_seed(seed)
    rows = torch.rand((n, E.ROW_BEST), generator=g)
    rows[:, 7] = (torch.arange(n) % 2).float()
    return rows


def test_row_layout_and_column_names():
    from vpho_amd import evaluate as E
    from vpho_amd.ops_names import HAND_METRIC_NAMES, MULTI_COLUMNS, MULTI_TABLES, OBJ_METRIC_NAMES
    assert E.ROW == 28 and E.RowLayout.resolve(eval_best=False).width == E.ROW and E.RowLayout.resolve(eval_best=True).width == E.ROW_BEST == E.ROW + E.MULTI
    assert len(MULTI_COLUMNS) == E.MULTI == 3 * len(HAND_METRIC_NAMES) + 3 * len(OBJ_METRIC_NAMES)
    assert MULTI_COLUMNS[0] == 'one_candidate/hand/MJE' and MULTI_COLUMNS[4] == 'best_of_S/hand/MJE'
    assert MULTI_COLUMNS[12] == 'one_candidate/object/MCE' and MULTI_COLUMNS[28] == 'best_of_S/object/MCE'
    assert MULTI_COLUMNS[-1] == 'mean_of_S/object/FSCORE@10cm' and MULTI_TABLES == E.MULTI_TABLES


def test_summarize_wide_rows_adds_three_tables_and_keeps_the_rest():
    from vpho_amd import evaluate as E
    from vpho_amd.ops_names import MULTI_COLUMNS
    rows = _wide_rows(7)
    narrow = E.summarize(rows[:, :E.ROW])
    wide = E.summarize(rows)
    assert set(wide) == set(narrow) | {'one_candidate', 'best_of_S', 'mean_of_S'}
    for k in narrow:
        assert wide[k] == narrow[k]
    mean = rows.double().mean(0)
    for j, name in enumerate(MULTI_COLUMNS):
        table, part, metric = name.split('/')
        scale = 1.0 if part == 'hand' else (1000.0 if metric in ('MCE', 'OCE', 'MCE2', 'ADD', 'ADDS', 'CD') else 1.0 if metric == 'REP' else 100.0)
        assert wide[table][part][metric] == pytest.approx(float(mean[E.ROW + j]) * scale, rel=1e-12), name


def test_eval_best_flag_defaults_off_and_parses():
    from vpho_amd.configs import args
    assert args.Config().eval_best is False
    assert args._parser().parse_args(['--eval_best']).eval_best is True
    assert args._parser().parse_args([]).eval_best is False


def test_multi_hypothesis_block_has_no_cpu_path():
    from vpho_amd import evaluate as E
    n, S = 2, 3
    out = {'diff_final_hand_joint': torch.zeros(n, S, 21, 3), 'diff_final_hand_vert': torch.zeros(n, S, 778, 3)}
    data = {'root_joint': torch.zeros(n, 3), 'is_right': torch.ones(n, dtype=torch.bool)}
    with pytest.raises(RuntimeError, match='GPU only'):
        E.multi_hypothesis_block(out, data, torch.zeros(n, 21, 3), torch.zeros(n, 778, 3))


def _worker_ragged_wide(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from vpho_amd import evaluate as E
    n = 4 if rank == 0 else 1
    rows = _wide_rows(n, seed=rank)
    rows[:, 0] = torch.arange(n) + 100 * rank
    q.put((rank, E.gather_rows(rows).clone()))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_wide_rows_world2_gloo_ragged():
    """the wide rows travel in the one all-gather of the 28-column rows: ragged counts, rank order, every column intact"""
    from vpho_amd import evaluate as E
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_ragged_wide, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = torch.cat([_wide_rows(4, seed=0), _wide_rows(1, seed=1)], 0)
    want[:, 0] = torch.tensor([0.0, 1.0, 2.0, 3.0, 100.0])
    for r in range(2):
        assert got[r].shape == (5, E.ROW_BEST)
        assert torch.equal(got[r], want)
    assert set(E.summarize(got[0])) >= {'one_candidate', 'best_of_S', 'mean_of_S'}


@pytest.mark.parametrize('name', ['hand_metrics_multi_kernel', 'obj_multi_nn_kernel', 'obj_multi_metrics_kernel', 'obj_multi_reduce_kernel'])
def test_multi_hypothesis_kernels_use_no_scratch(name):
    """the new kernels in the compiler's resource report (parsed like tests/test_kernel_resources.py): no scratch, no spills; the NN
    kernel keeps the occupancy its LDS tile allows (4 workgroups of 33 KB per CU, 4 waves per SIMD)"""
    import glob
    import re
    import subprocess
    from vpho_amd.build import OBJ, build_extension
    build_extension()
    raw, cur = {}, None
    for f in glob.glob(os.path.join(OBJ, '*.usage.txt')):
        for line in open(f):
            m = re.search(r'Function Name: (\S+)', line)
            if m:
                cur = m.group(1)
                raw[cur] = {}
            for key, pat in (('vgpr', r' VGPRs: (\d+)'), ('spill', r'VGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                             ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)')):
                m = re.search(pat, line)
                if m and cur:
                    raw[cur][key] = int(m.group(1))
    names = list(raw)
    dem = subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.strip().split('\n')
    kernels = {re.sub(r'\(anonymous namespace\)::', '', d).split('(')[0].replace('void ', ''): raw[n] for n, d in zip(names, dem)}
    assert name in kernels, sorted(kernels)[:20]
    k = kernels[name]
    assert k['scratch'] == 0 and k.get('spill', 0) == 0, (name, k)
    if name == 'obj_multi_nn_kernel':
        assert k['occupancy'] >= 4 and k['vgpr'] <= 128, k

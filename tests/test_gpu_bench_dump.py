"""bench.py --dump-outputs: what the last timed step returned, as float32 / float64 .npy files within the size budget, the same from
run to run at the same arguments (two builds are compared output for output that way)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = 2
ARGS = ['--gpus', '1', '--steps', '3', '--warmup', '1', '--bs', str(BS), '--sample_num', '4', '--sampling_steps', '5', '--topk_hand', '8',
        '--topk_obj', '3', '--sample_T0', '0.2', '--no_cpu_baseline', '--no_kernel_timing', '--no_opt_in']


def _bench(out):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + ARGS + ['--dump-outputs', str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])


def test_dump_outputs_of_the_last_timed_step(tmp_path):
    a, b = tmp_path / 'a', tmp_path / 'b'
    line = _bench(a)
    _bench(b)
    assert line['steps'] == 3 and line['ms_per_step'] > 0
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {'agg_hand_joint.npy', 'agg_hand_vert.npy', 'agg_obj_6d.npy', 'diff_final_obj_6d.npy', 'metric_rows.npy'} <= set(names)
    total = 0
    for n in names:
        x = np.load(a / n)
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, np.load(b / n), equal_nan=True), n
        total += os.path.getsize(a / n)
    assert total <= 64_000_000
    assert np.load(a / 'metric_rows.npy').shape[0] == BS                 # the last step's rows only
    assert np.load(a / 'agg_hand_joint.npy').shape == (BS, 21, 3)
    assert np.load(a / 'diff_final_obj_6d.npy').dtype == np.float64     # the object hypotheses stay fp64

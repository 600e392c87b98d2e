"""Which kernel a convolution launch reaches, pinned without a device: vpho_amd/csrc/conv_plan.h is host-only, tests/_conv_plan_probe.cpp
prints its plans, tests/_conv_plan_cases.py holds what they must be.  The GPU tests whose shapes were chosen for a kernel or a tile class
(test_gpu_conv.py, test_gpu_bn_fuse.py, test_gpu_bn_stats_fp64.py) point here: a moved threshold changes a literal of this table instead of
silently taking a class out of their coverage."""
import os
import shutil
import subprocess

import pytest

from tests._conv_plan_cases import CASES, GPU_CASES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _cxx():
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'a host C++ compiler is needed'
    return cxx


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    """id -> the probe's line, from ONE run over all cases; the header compiles with -Wall -Werror and no ROCm include path"""
    exe = str(tmp_path_factory.mktemp('conv_plan') / 'probe')
    r = subprocess.run([_cxx(), '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(HERE, '_conv_plan_probe.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ids = list(CASES)
    r = subprocess.run([exe], input=''.join(CASES[i][0] + '\n' for i in ids), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(ids)
    return dict(zip(ids, lines))


@pytest.mark.parametrize('case', list(CASES))
def test_plan_is_the_recorded_one(plans, case):
    assert plans[case] == CASES[case][1], CASES[case][0]


def _fields(line):
    return dict(t.split('=', 1) for t in line.split() if '=' in t)


def test_the_table_reaches_every_family_tile_and_switch():
    """the table is only worth something while it covers the decisions: every kernel family on every tile it exists for, every switch
    value, ten refusals, the three weight-gradient tiles and slice sums, every Winograd kernel"""
    conv = [_fields(p) for d, p in CASES.values() if d.startswith('conv') and p.startswith('rc=0')]
    reached = {(f['family'], f['tile'], f['threads']) for f in conv}
    tiles = [('128x128', '512'), ('128x64', '512'), ('64x64', '256')]
    want = {(fam, t, n) for fam in ('reg', 'glds', 'glds_pre') for t, n in tiles} | {('reg', '128x128', '256'), ('pers', '128x128', '512'), ('pers_bn', '128x128', '512')}
    want |= {(fam, t, n) for fam, (t, n) in [('split6', tiles[0]), ('split9', tiles[1]), ('split9', tiles[2]), ('split6', tiles[1]), ('split6', tiles[2])]}
    assert want <= reached, want - reached
    descs = [d for d, p in CASES.values()]
    for sw in ['pers=0', 'pers=1', 'pers=2', 'tile=128', 'tile=1288', 'tile=12864', 'tile=64', 'no_glds=1', 'no_uni=1', 'dbg=8', 'dbg=16']:
        assert any(sw in d.split() for d in descs), sw
    refusals = {p.split('error=', 1)[1] for d, p in CASES.values() if p.startswith('rc=1') and 'need_slots=0' in p}
    assert len(refusals) >= 10
    wg = [_fields(p) for d, p in CASES.values() if d.startswith('wgrad')]
    assert {f['tile'] for f in wg} == {'64x64', '128x64', '128x128'} and {f['reduce_groups'] for f in wg} == {'0', '1', '4', '16'}
    assert {'1', '8'} <= {f['splits'] for f in wg} and any(int(f['splits']) > 8 and int(f['splits']) % 8 == 0 for f in wg)
    wino = {(f['epilogue'], f['mode']) for f in (_fields(p) for d, p in CASES.values() if d.startswith('wino'))}
    assert wino == {('plain', '0'), ('plain', '1'), ('plain', '2'), ('bn_fwd', '0'), ('bn_fwd', '1'), ('bn_bwd', '0'), ('bn_bwd', '1')}
    assert any(_fields(p)['staged_ok'] == '0' for d, p in CASES.values() if d.startswith('wino'))


def test_the_forced_register_staged_tile_refuses_bn_x_without_a_stored_gate():
    """VPHO_CONV_TILE=128 has no BatchNorm epilogue; with bn_x and no stored gate the call fails instead of dropping the gate"""
    d, p = CASES['c_tile128_bn_x_without_gate_refused']
    assert 'tile=128' in d.split() and 'bn_x=1' in d.split() and 'gate=1' not in d.split()
    assert p.startswith('rc=1 stats_rows=0 ') and 'runs a kernel without the BatchNorm epilogue (tile 128)' in p


def test_weight_gradient_workspace_is_one_dw_per_slice():
    for d, p in CASES.values():
        if d.startswith('wgrad'):
            f, g = _fields(d), _fields(p)
            k = int(f['K']) ** 2 * int(f['Cin'])
            assert int(g['workspace']) == (int(g['splits']) * int(f['Cout']) * k * 4 if int(g['splits']) > 1 else 0), d


def test_the_gpu_cases_name_a_profiling_class_each():
    classes = {'conv_igemm_128x128', 'conv_igemm_128x64', 'conv_igemm_64x64', 'conv_wgrad_64x64', 'conv_wgrad_128x128'}
    seen = set()
    for i in GPU_CASES:
        d, p = CASES[i]
        seen.add('conv_winograd' if d.startswith('wino') else _fields(p)['prof'])
    assert seen == classes | {'conv_winograd'}

"""Which kernels one evaluation of the score network launches, pinned without a device: vpho_amd/csrc/score_plan.h is host-only,
tests/_score_plan_probe.cpp prints its plans, tests/_score_plan_cases.py holds what they must be.  The GPU tests whose shapes were chosen
for a kernel or a tile split (tests/test_gpu_sampler.py) point here: a moved threshold changes a literal of this table instead of silently
taking a kernel out of their coverage."""
import os
import shutil
import subprocess

import pytest

from tests._score_plan_cases import CASES, GPU_CASES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _cxx():
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'a host C++ compiler is needed'
    return cxx


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    """id -> the probe's line, from ONE run over all cases; the header compiles with -Wall -Werror and no ROCm include path (the stamps
    are printed to 17 digits: no contraction of i * step + T0, as in the library's own build)"""
    exe = str(tmp_path_factory.mktemp('score_plan') / 'probe')
    r = subprocess.run([_cxx(), '-std=c++17', '-O1', '-ffp-contract=off', '-Wall', '-Werror', os.path.join(HERE, '_score_plan_probe.cpp'), '-o', exe],
                       capture_output=True, text=True)
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


def _of(kind, ok=True):
    return [(d, _fields(p)) for d, p in CASES.values() if d.split()[0] == kind and p.startswith('rc=0' if ok else 'rc=1')]


def test_the_table_reaches_every_kernel_switch_and_refusal():
    """the table is only worth something while it covers the decisions: the eight pose-encoder kernels, the six head kernels, every switch
    value, both outcomes of the tail-tile rule on two slot counts, each refusal and the unknown slot count"""
    assert {(f['rows'], f['n1']) for d, f in _of('pe')} == {(r, n) for r in ('32', '64') for n in '1234'}
    assert {(f['family'], f['cb']) for d, f in _of('head')} == {('plain', '0'), ('plain', '1'), ('epi0', '0'), ('epi0', '1'), ('split6', '0'), ('split9', '0')}
    descs = [d.split() for d, p in CASES.values()]
    for sw in ['pe_rows=32', 'pe_rows=64', 'pe_rows=48', 'head_tail=0', 'head_tail=1', 'head_cb=0', 'head_cb=1', 'head_epi=0', 'head_epi=1',
               'slots=208', 'slots=608', 'slots=16', 'slots=-1']:
        assert any(sw in d for d in descs), sw
    for slots in (None, 'slots=208'):
        tails = {f['tail'] != '0' for d, f in _of('head') if (slots in d.split() if slots else 'slots=' not in d)}
        assert tails == {False, True}, slots
    refusals = {p.split('error=', 1)[1] for d, p in CASES.values() if p.startswith('rc=1') and 'need_slots=1' not in p}
    assert len(refusals) == 3 and all(refusals)
    assert any(p == 'rc=1 need_slots=1 error=' for d, p in CASES.values())


def test_lds_and_names_follow_the_kernel():
    for d, f in _of('pe'):
        assert (f['lds'], f['name']) == {'32': ('35328', 'pose_encoder_reg_kernel'), '64': ('68608', 'pose_encoder_reg64_kernel')}[f['rows']], d
        R = int(_fields(d)['R'])
        assert int(f['grid']) == -(-R // int(f['rows'])), d
    for d, f in _of('head'):
        split = f['family'].startswith('split')
        assert (f['lds'], f['name']) == (('73728', 'score_head_split_kernel') if split else ('57344', 'score_head_kernel')), d
        g, R = _fields(d), int(_fields(d)['R'])
        full, tail = int(f['full']), int(f['tail'])
        assert int(f['grid']) == int(g['nheads']) * (full + tail), d
        # the tiles cover the rows exactly once: ordinary tiles first, then 32-row tiles for what is left
        assert (full == -(-R // 128) and tail == 0) or (0 < 128 * full < R and tail == -(-(R - 128 * full) // 32)), d


def test_workspace_slices_start_on_256_bytes():
    ws = [(d, _fields(p)) for d, p in CASES.values() if d.startswith('ws')]
    assert len(ws) >= 3
    for d, f in ws:
        assert f['aligned'] == '1' and f['ascending'] == '1' and f['bytes'] == f['sizing'] and int(f['bytes']) % 256 == 0 and f['first'] == '0', d
        # the last slice is the step log: CTL_LOG_CAP entries of four doubles
        assert int(f['bytes']) - int(f['last']) == 512 * 32, d


def test_the_gpu_cases_are_one_pose_encoder_and_one_head_plan_each():
    for net, bs, S, pe, head in GPU_CASES:
        (dp, pp), (dh, ph) = CASES[pe], CASES[head]
        fp, fh = _fields(dp), _fields(dh)
        assert dp.startswith('pe ') and dh.startswith('head ') and pp.startswith('rc=0') and ph.startswith('rc=0')
        assert int(fp['R']) == int(fh['R']) == bs * S and int(fh['S']) == S
        assert (int(fp['D']), int(fh['nheads'])) == {'hand': (96, 32), 'obj': (9, 3)}[net]

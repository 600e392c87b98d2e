"""tests/_rk_replay.py on the CPU oracle alone: the cases reach the controller branches they are there for, check_log accepts the
oracle's logs and refuses logs of a controller that breaks one rule, forced_replay on the oracle's own log IS the free run, and the
rounding spread that the GPU tests (tests/test_gpu_sampler_rejects.py) take their tolerances from is the recorded one."""
import numpy as np
import pytest
import torch

from tests import _rk_replay as RR

NAMES = list(RR.CASES)
REJECTING = [n for n in NAMES if RR.CASES[n]['rejects']]


@pytest.fixture(scope='module')
def weights(sd, sd_contrast):
    return {'sd': sd, 'sd_contrast': sd_contrast}


def _log(weights, name):
    xs, x, info = RR.cached_free_run(weights, name)
    return info['steps'], info


def _check(weights, name, steps=None, nfev=None):
    case = RR.CASES[name]
    s, info = _log(weights, name)
    return RR.check_log(s if steps is None else steps, dict(nfev=info['nfev'] if nfev is None else nfev), case['T0'], RR.EPS, case['stamps'])


# ---------------------------------------------------------------------------------------------------- branch coverage
def test_cases_are_small():
    for case in RR.CASES.values():
        assert RR.BS * RR.S <= 21 and case['T0'] > RR.EPS


def test_every_case_reaches_its_branches(weights):
    summ = {n: _check(weights, n) for n in NAMES}
    logs = {n: _log(weights, n)[0] for n in NAMES}
    for n in NAMES:
        assert summ[n]['attempts'] <= 120, (n, summ[n])             # far below the device's cap of 512 attempts
    assert summ['obj_1e-4']['n_rejected'] >= 2 and summ['obj_1e-4']['max_consecutive_rejects'] >= 2
    assert summ['obj_1e-5']['n_rejected'] >= 2 and summ['obj_1e-5']['clamped_to_one'] >= 1
    assert summ['obj_1e-5']['attempts'] > 18 + 2 * 20                 # after an 18-attempt solve on the same workspace: > 20 extra rounds of two
    assert summ['hand_1e-4']['n_rejected'] >= 1 and RR.CASES['hand_1e-4']['D'] == 96
    assert summ['hand_contrast_1e-4']['n_rejected'] >= 1 and summ['hand_contrast_1e-4']['clamped_to_one'] >= 1
    for n in ('obj_zeros', 'hand_zeros'):
        assert summ[n]['max_factor'] >= 1                             # factor = MAX_FACTOR
        assert abs(logs[n][0][1]) <= 100 * 1e-6 * (1 + 1e-9)          # h0 = 1e-6: the first step is min(100 * h0, ...)
        assert min(s[2] for s in logs[n]) < 5.9e-6                    # 0.9 * err ** -0.2 > 10
    for n in REJECTING:
        assert RR.has_accept_after_reject(logs[n]), n
    # together
    assert any(s['n_rejected'] >= 2 for s in summ.values())
    assert any(s['max_consecutive_rejects'] >= 2 for s in summ.values())
    assert any(s['clamped_to_one'] >= 1 for s in summ.values())
    per = [k for n in NAMES for k in RR.stamps_per_accept(logs[n], RR.CASES[n]['T0'], RR.EPS, RR.CASES[n]['stamps'])]
    assert min(per) == 0 and max(per) >= 2
    for n in NAMES:                                                   # every stamp is written exactly once
        assert sum(RR.stamps_per_accept(logs[n], RR.CASES[n]['T0'], RR.EPS, RR.CASES[n]['stamps'])) == RR.CASES[n]['stamps']


@pytest.mark.parametrize('name', REJECTING)
def test_rejections_survive_a_perturbed_start(weights, name):
    """the controller is chaotic at these tolerances (the attempt count moves), the rejections are not an accident of one rounding"""
    case = RR.CASES[name]
    _, init = RR.case_inputs(case)
    for seed in (1, 2, 3):
        _, _, info = RR.free_run(weights[case['weights']], case, RR.perturbed(init, seed))
        assert any(not s[3] for s in info['steps']), (name, seed)
        assert len(info['steps']) <= 120


# ---------------------------------------------------------------------------------------------------- check_log
@pytest.mark.parametrize('name', NAMES)
def test_check_log_accepts_the_oracle(weights, name):
    summ = _check(weights, name)
    steps, info = _log(weights, name)
    assert summ['attempts'] == len(steps) and summ['n_rejected'] == sum(not s[3] for s in steps)
    # the log made by the test-side controller from the oracle's error norms is the oracle's log
    sim = RR.simulate_log([s[2] for s in steps], RR.CASES[name]['T0'], RR.EPS, abs(steps[0][1]))
    assert [(s[0], s[3]) for s in sim] == [(s[0], s[3]) for s in steps]
    np.testing.assert_allclose([s[1] for s in sim], [s[1] for s in steps], rtol=1e-13)


def _with(steps, i, **kw):
    t, h, e, a = steps[i]
    d = dict(t=t, h=h, err=e, acc=a)
    d.update(kw)
    return steps[:i] + [(d['t'], d['h'], d['err'], d['acc'])] + steps[i + 1:]


def test_check_log_refuses_a_missing_clamp_to_one(weights):
    steps, _ = _log(weights, 'obj_1e-5')
    # the attempt after an accept-after-reject whose growth factor exceeds 1: as long as the unclamped controller would make it
    idx = [i for i in range(1, len(steps) - 1) if not steps[i - 1][3] and steps[i][3] and 0.9 * steps[i][2] ** -0.2 > 1.0]
    assert idx
    i = idx[0]
    bad = _with(steps, i + 1, h=steps[i][1] * min(10.0, 0.9 * steps[i][2] ** -0.2))
    with pytest.raises(AssertionError, match='step size'):
        _check(weights, 'obj_1e-5', bad)
    # and a whole self-consistent log of such a controller
    errs = [0.5, 3.0, 0.2, 0.5, 0.5]
    good = RR.simulate_log(errs, 0.65, RR.EPS, 0.05)
    RR.check_log(good, dict(nfev=3 + 6 * len(good)), 0.65, RR.EPS, 5)
    bad = RR.simulate_log(errs, 0.65, RR.EPS, 0.05, clamp_after_reject=False)
    with pytest.raises(AssertionError, match='attempt 3: step size'):
        RR.check_log(bad, dict(nfev=3 + 6 * len(bad)), 0.65, RR.EPS, 5)


def test_check_log_refuses_another_min_factor():
    """no case reaches MIN_FACTOR (err > 1845), so the rule is exercised on logs the controller itself makes from given error norms"""
    errs = [0.5, 5000.0, 0.5]
    good = RR.simulate_log(errs, 0.65, RR.EPS, 0.05)
    assert not good[1][3] and abs(good[2][1] / good[1][1] - 0.2) < 1e-12
    RR.check_log(good, dict(nfev=3 + 6 * len(good)), 0.65, RR.EPS, 5)
    bad = RR.simulate_log(errs, 0.65, RR.EPS, 0.05, min_factor=0.1)
    with pytest.raises(AssertionError, match='attempt 2: step size'):
        RR.check_log(bad, dict(nfev=3 + 6 * len(bad)), 0.65, RR.EPS, 5)


def test_check_log_refuses_an_unclipped_last_step(weights):
    steps, _ = _log(weights, 'obj_1e-4')
    prev = steps[-2]
    assert prev[3]
    bad = _with(steps, len(steps) - 1, h=prev[1] * min(10.0, 0.9 * prev[2] ** -0.2))
    assert bad[-1][0] + bad[-1][1] < RR.EPS
    with pytest.raises(AssertionError, match='not clipped'):
        _check(weights, 'obj_1e-4', bad)
    bad = RR.simulate_log([0.5] * 4, 0.65, RR.EPS, 0.05, clip=False)
    with pytest.raises(AssertionError, match='not clipped'):
        RR.check_log(bad, dict(nfev=3 + 6 * len(bad)), 0.65, RR.EPS, 5)
    # stopping short of eps is refused too
    with pytest.raises(AssertionError):
        _check(weights, 'obj_1e-4', steps[:-1], nfev=3 + 6 * (len(steps) - 1))


def test_check_log_refuses_a_flipped_accept_flag(weights):
    steps, _ = _log(weights, 'obj_1e-4')
    rej = [i for i, s in enumerate(steps) if not s[3]][0]
    for i in (rej, 3):
        with pytest.raises(AssertionError, match='accept flag'):
            _check(weights, 'obj_1e-4', _with(steps, i, acc=not steps[i][3]))


def test_check_log_refuses_a_wrong_nfev_and_wrong_counts(weights):
    steps, info = _log(weights, 'obj_1e-4')
    for d in (6, -6):
        with pytest.raises(AssertionError, match='nfev'):
            _check(weights, 'obj_1e-4', nfev=info['nfev'] + d)
    case = RR.CASES['obj_1e-4']
    n_rej = sum(not s[3] for s in steps)
    RR.check_log(steps, dict(nfev=info['nfev'], n_accepted=len(steps) - n_rej, n_rejected=n_rej), case['T0'], RR.EPS, case['stamps'])
    with pytest.raises(AssertionError, match='n_rejected'):
        RR.check_log(steps, dict(nfev=info['nfev'], n_accepted=len(steps) - n_rej, n_rejected=n_rej - 1), case['T0'], RR.EPS, case['stamps'])


def test_check_log_refuses_a_moved_time_after_a_reject(weights):
    steps, _ = _log(weights, 'obj_1e-4')
    rej = [i for i, s in enumerate(steps) if not s[3]][0]
    with pytest.raises(AssertionError, match='time bookkeeping'):
        _check(weights, 'obj_1e-4', _with(steps, rej + 1, t=steps[rej][0] + steps[rej][1]))


# ---------------------------------------------------------------------------------------------------- forced_replay
@pytest.fixture(scope='module')
def replays(weights):
    out = {}

    def get(name):
        if name not in out:
            case = RR.CASES[name]
            steps, _ = _log(weights, name)
            _, init = RR.case_inputs(case)
            out[name] = RR.forced_replay(RR.rhs_of(weights, name), case['T0'], RR.EPS, init, steps, case['rtol'], case['atol'], case['stamps'])
        return out[name]
    return get


@pytest.mark.parametrize('name', NAMES)
def test_forced_replay_of_the_oracles_own_log_is_the_free_run(weights, replays, name):
    xs, x, info = RR.cached_free_run(weights, name)
    rep = replays(name)
    assert np.array_equal(rep['err'], np.array([s[2] for s in info['steps']]))
    assert np.array_equal(rep['xs'].numpy(), xs.numpy()) and np.array_equal(rep['x'].numpy(), x.numpy())
    assert rep['nfev'] == info['nfev']
    # the logged first h is (T0 - h_init) - T0, rounded on the grid of T0
    assert abs(rep['h_init'] - abs(info['steps'][0][1])) <= np.spacing(RR.CASES[name]['T0'])


@pytest.mark.parametrize('name', NAMES)
def test_rounding_spread(weights, replays, name):
    """How far two roundings of the same exact right-hand side lie apart ON A FORCED STEP SEQUENCE: the fp32 denoiser against the same
    denoiser evaluated in float64 and rounded to float32 at its output.  The GPU tests allow the device 4 x this spread; the recorded
    constants (tests/_rk_replay.py CASES) must be within a factor of 2 of what this machine measures."""
    case = RR.CASES[name]
    steps, _ = _log(weights, name)
    _, init = RR.case_inputs(case)
    a = replays(name)
    b = RR.forced_replay(RR.rhs_of(weights, name, fp64=True), case['T0'], RR.EPS, init, steps, case['rtol'], case['atol'], case['stamps'])
    r_err = float(np.max(np.abs(a['err'] - b['err']) / np.maximum(a['err'], 1e-3)))
    r_x = max(float((a['xs'] - b['xs']).abs().max()), float((a['x'] - b['x']).abs().max()))
    print(f'{name}: r_err {r_err:.3g} (recorded {case["r_err"]:.3g})  r_x {r_x:.3g} (recorded {case["r_x"]:.3g})')
    assert case['r_err'] / 2 <= r_err <= case['r_err'] * 2
    assert case['r_x'] / 2 <= r_x <= case['r_x'] * 2
    assert 4 * case['r_err'] <= 0.05                                 # sharp enough to see a stale K slot or a swapped buffer (order 1)

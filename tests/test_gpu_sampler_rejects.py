"""The on-device RK45 step controller (vpho_amd/csrc/score_ode.hip: rk_begin_kernel / rk_end_kernel, the host loop ode_sample_host, the
enqueue-ahead loop of ode_sample_device) on solves that REJECT steps, checked by forced-step replay (tests/_rk_replay.py):

  * controller logic: every attempt of the device's own log follows from the previous one by scipy's rules (check_log);
  * state handling: the CPU oracle, made to take the device's (h, accepted) sequence, gets the same error norm for every attempt and
    the same stamps and sample -- a stale K slot, a swapped y buffer or a dense output written after a rejection changes them by order 1.

Tolerances: 4 x the rounding spread recorded per case (CASES r_err, r_x: fp32 against fp64 evaluation of the network on a forced
sequence).  The device is another fp32 evaluation of the same exact function, so it lies about as far from the exact value as the
oracle does: a factor 2 by the triangle inequality, another factor 2 of margin; never looser than the suite's 1e-3 on the samples.

Observed on an MI355X (device against the replay of its own steps; d_err = max |d err| / max(err, 1e-3), d_xs / d_x = max abs), next to
the tolerances: obj_1e-4 2.3e-5 (2.8e-4), 5.7e-7 / 5.7e-7 (2.5e-6); obj_1e-5 1.6e-4 (1.3e-3), 5.8e-7 / 5.8e-7 (1.8e-6); hand_1e-4 9.9e-6
(1.4e-4), 6.1e-7 / 6.1e-7 (3.0e-6); hand_contrast_1e-4 8.2e-6 (3.7e-4), 1.2e-6 / 5.5e-8 (4.0e-6); obj_zeros 2.7e-5 (1.2e-3), 4.3e-7 / 4.2e-7
(1.8e-6); hand_zeros 8.2e-6 (5.8e-4), 5.1e-7 / 5.1e-7 (2.4e-6).  docs/LOG.md, "RK45 solves that reject steps".
"""
import numpy as np
import pytest
import torch

from tests import _rk_replay as RR

pytestmark = pytest.mark.gpu
NAMES = list(RR.CASES)
STEP_RTOL = 2e-4                   # the first step against the oracle's select_initial_step: the step tolerance of test_gpu_sampler.py


@pytest.fixture(scope='module')
def weights(sd, sd_contrast):
    return {'sd': sd, 'sd_contrast': sd_contrast}


@pytest.fixture(scope='module')
def nets(weights):
    from vpho_amd import ops
    made = {}

    def get(name):
        case = RR.CASES[name]
        key = (case['weights'], case['net'])
        if key not in made:
            made[key] = ops.ScoreNet(weights[case['weights']], f"denoiser_{case['net']}", 'cuda')
        return made[key]
    return get


def _solve(net, name, num_steps=None, **kw):
    case = RR.CASES[name]
    feat, init = RR.case_inputs(case)
    kw.setdefault('xs_f64', True)
    xs, x, st = net.sample(feat.cuda(), init.cuda(), RR.S, case['T0'], num_steps or case['stamps'], rtol=case['rtol'], atol=case['atol'], **kw)
    torch.cuda.synchronize()
    return xs.cpu(), x.cpu(), st


def _verify(weights, name, h_init, xs, x, st, num_steps=None):
    """both checks of one device solve; returns the distances (device against forced replay)"""
    case = RR.CASES[name]
    num_steps = num_steps or case['stamps']
    steps = st['steps']
    # controller logic
    assert st['nan_count'] == 0
    summ = RR.check_log(steps, st, case['T0'], RR.EPS, num_steps)
    if case['rejects']:
        assert summ['n_rejected'] >= 1 and RR.has_accept_after_reject(steps), summ
    assert abs(abs(steps[0][1]) - h_init) <= STEP_RTOL * h_init, (steps[0][1], h_init)
    # state handling
    _, init = RR.case_inputs(case)
    rep = RR.forced_replay(RR.rhs_of(weights, name), case['T0'], RR.EPS, init, steps, case['rtol'], case['atol'], num_steps)
    err_dev = np.array([s[2] for s in steps])
    d_err = float(np.max(np.abs(err_dev - rep['err']) / np.maximum(rep['err'], 1e-3)))
    d_xs, d_x = float((xs.double() - rep['xs']).abs().max()), float((x.double() - rep['x']).abs().max())
    tol_x = min(4 * case['r_x'], 1e-3)
    print(f"{name} stamps {num_steps}: attempts {summ['attempts']} rejected {summ['n_rejected']} clamped_to_one {summ['clamped_to_one']} "
          f"max_factor {summ['max_factor']} | d_err {d_err:.3g} (tol {4 * case['r_err']:.3g})  d_xs {d_xs:.3g} d_x {d_x:.3g} (tol {tol_x:.3g})")
    assert 4 * case['r_err'] <= 0.05
    assert rep['nfev'] == st['nfev']
    assert d_err <= 4 * case['r_err'], (d_err, 4 * case['r_err'])
    assert d_xs <= tol_x and d_x <= tol_x, (d_xs, d_x, tol_x)
    return dict(d_err=d_err, d_xs=d_xs, d_x=d_x, summ=summ)


def _h_init(weights, name):
    case = RR.CASES[name]
    _, init = RR.case_inputs(case)
    return RR.initial_step(RR.rhs_of(weights, name), case['T0'], RR.EPS, init, case['rtol'], case['atol'])[0]


@pytest.mark.parametrize('name', NAMES)
def test_device_solve_follows_the_controller_and_the_forced_replay(weights, nets, name):
    h_init = _h_init(weights, name)                                  # CPU reference first
    xs, x, st = _solve(nets(name), name)
    _verify(weights, name, h_init, xs, x, st)


def test_device_loop_with_full_arrays_and_host_loop(weights, nets):
    """num_steps = 1024: the device loop with its te / dense_p arrays exactly full; 1025: the host loop (ode_sample_host), whose dense
    output goes out in several chunks.  The two loops differ by the last bit of pow() (device library against libm, ~2e-16); the
    controller amplifies a 2e-7 perturbation to 0.35 over such a solve (~2e6), so |h| agrees to far better than 1e-6."""
    name = 'obj_1e-4'
    h_init = _h_init(weights, name)
    res = {}
    for n in (1024, 1025):
        xs, x, st = _solve(nets(name), name, num_steps=n)
        assert xs.shape[1] == n
        _verify(weights, name, h_init, xs, x, st, num_steps=n)
        res[n] = st['steps']
    assert [s[3] for s in res[1024]] == [s[3] for s in res[1025]]
    h_dev, h_host = np.array([s[1] for s in res[1024]]), np.array([s[1] for s in res[1025]])
    worst = float(np.max(np.abs(h_dev / h_host - 1)))
    print(f'device loop against host loop: max relative |h| difference {worst:.3g}')
    assert worst <= 1e-6                                              # observed on an MI355X: 0 (every |h| of the 32 attempts bit-equal)


def _result(net, name):
    xs, x, st = _solve(net, name)
    return xs, x, st['steps'], st['nfev']


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


def test_enqueue_hint_does_not_change_a_solve(weights):
    """A solve enqueues as many attempts as the previous solve on its workspace needed, then rounds of two.  A (76 attempts) after
    anything shorter: a shortfall and ~30 rounds of two; B (18 attempts) after A: 58 surplus attempts enqueued behind ``done``, which
    must be no-ops; B after B and A after A: the hint is exact.  Every order gives the same bits."""
    from vpho_amd import ops
    A, B = 'obj_1e-5', 'obj_zeros'
    assert RR.CASES[A]['weights'] == RR.CASES[B]['weights'] and RR.CASES[A]['net'] == RR.CASES[B]['net']
    first = ops.ScoreNet(weights['sd'], 'denoiser_obj', 'cuda')
    ra, rb = [], []
    ra.append(_result(first, A)); rb.append(_result(first, B)); rb.append(_result(first, B))
    fresh = ops.ScoreNet(weights['sd'], 'denoiser_obj', 'cuda')      # ``first`` stays alive: another workspace
    rb.append(_result(fresh, B)); ra.append(_result(fresh, A)); ra.append(_result(fresh, A))
    assert len(ra[0][2]) > len(rb[0][2]) + 40 and ra[0][3] == 3 + 6 * len(ra[0][2]) and rb[0][3] == 3 + 6 * len(rb[0][2])
    for r in ra[1:]:
        assert _same(ra[0], r)
    for r in rb[1:]:
        assert _same(rb[0], r)
    for r in ra + rb:
        assert torch.isfinite(r[0]).all() and torch.isfinite(r[1]).all()


def test_float32_outputs_are_the_rounded_float64_outputs(nets):
    name = 'obj_1e-4'
    xs64, x64, st64 = _solve(nets(name), name)
    xs32, x32, st32 = _solve(nets(name), name, xs_f64=False, x_f64=False)
    assert xs32.dtype == torch.float32 and x32.dtype == torch.float32
    assert st32['n_rejected'] >= 1 and st32['steps'] == st64['steps'] and st32['nfev'] == st64['nfev']
    assert torch.equal(xs32, xs64.float()) and torch.equal(x32, x64.float())

"""RK45 solves that reject steps: a verifier of the scalar step controller and a forced-step replay of the oracle (CPU only: numpy
and torch, no HIP library).

Why not compare a device solve with the oracle's own free run: at the tolerances that make the controller reject, the controller is
chaotic under fp32 rounding.  Two oracle runs at rtol 1e-5 / atol 1e-6 whose start states differed by 2e-7 (relative) had error
norms that differed by up to 0.42, step sizes by up to 30 %, and a different accept / reject sequence in 3 of 20 configurations.
What is robust is to make the oracle take the steps of the solve under test:

  * check_log      -- every attempt of a step log follows from the previous attempt's OWN logged values by scipy's controller
                      (rk.py _step_impl), restated in fp64 independently of oracle/rk45.py and of the kernels;
  * forced_replay  -- the oracle's RK45 stage algebra (the tableau of oracle/rk45.py, fp64) on the oracle's right-hand side (the ``fun``
                      of oracle/nets.py::ode_sample with its float32 casts), through a GIVEN (h, accepted) sequence: the error norm
                      of every attempt, the dense-output stamps, the final state and the denoised sample.  With the step sequence
                      forced, a 2e-7 perturbation moves the error norms by <= 1.8e-4 (relative) and the final state by <= 5e-6.

CASES are the configurations (21 rows, eps 1e-5) whose free run on the CPU oracle reaches the controller's branches.  The MIN_FACTOR
clamp (0.9 * err ** -0.2 < 0.2) needs err > 1845; none of roughly 60 configurations of these networks reached it, so no case covers
it (check_log itself is tested for it on synthetic logs).
"""
import math

import numpy as np
import torch

from oracle import nets as N
from oracle.rk45 import A, B, C, E, P, select_initial_step

EPS = N.EPS_T
BS, S = 3, 7                       # 21 rows
MAX_STEP = 10.0
H_RTOL = 1e-12                     # a predicted |h| against the logged one: only the last bits of pow() differ


def seeded(shape, seed, scale=1.0):
    """the ``seeded`` of tests/test_gpu_sampler.py"""
    return torch.from_numpy((np.random.default_rng(seed).normal(size=shape) * scale).astype(np.float32))


# r_err, r_x: the rounding spread of the forced replay, recorded on the CPU oracle by tests/test_rk_replay_cpu.py::test_rounding_spread
# (forced_replay on the oracle's own log, fp32 denoiser against the same denoiser evaluated in float64 and rounded to float32 at its
# output):  r_err = max |d err| / max(err, 1e-3) over the attempts,  r_x = max |d xs|, |d x|.  Both are maxima and move with the order in
# which the CPU's matrix products sum, i.e. with the oracle's thread count (1, 2, 4, 8 threads: up to 1.9 x apart); recorded is the
# geometric middle of the smallest and the largest of those four measurements.  The test recomputes them and requires the stored
# value within a factor of 2.  attempts / rejected: the oracle's free run (informative; the tests assert the branches).
CASES = {
    # consecutive rejections
    'obj_1e-4': dict(weights='sd', net='obj', D=9, T0=0.65, stamps=40, rtol=1e-4, atol=1e-5, init='prior', rejects=True,
                     attempts=33, rejected=2, r_err=7.1e-05, r_x=6.3e-07),
    # clamp to 1 after a reject (3 times), more than 30 rounds past the first enqueue
    'obj_1e-5': dict(weights='sd', net='obj', D=9, T0=0.65, stamps=40, rtol=1e-5, atol=1e-6, init='prior', rejects=True,
                     attempts=76, rejected=7, r_err=0.00032, r_x=4.6e-07),
    # D = 96
    'hand_1e-4': dict(weights='sd', net='hand', D=96, T0=0.65, stamps=40, rtol=1e-4, atol=1e-5, init='prior', rejects=True,
                      attempts=33, rejected=2, r_err=3.5e-05, r_x=7.6e-07),
    # clamp to 1 after a reject
    'hand_contrast_1e-4': dict(weights='sd_contrast', net='hand', D=96, T0=0.9, stamps=40, rtol=1e-4, atol=1e-5, init='prior',
                               rejects=True, attempts=67, rejected=1, r_err=9.3e-05, r_x=9.9e-07),
    # MAX_FACTOR, h0 = 1e-6
    'obj_zeros': dict(weights='sd', net='obj', D=9, T0=0.65, stamps=12, rtol=3e-3, atol=3e-4, init='zeros', rejects=False,
                      attempts=18, rejected=0, r_err=0.00029, r_x=4.4e-07),
    'hand_zeros': dict(weights='sd', net='hand', D=96, T0=0.65, stamps=12, rtol=3e-3, atol=3e-4, init='zeros', rejects=False,
                       attempts=18, rejected=0, r_err=0.000145, r_x=6.1e-07),
}


def case_inputs(case):
    """feat (BS,1024) per image, init (BS*S, D): the prior draw (or zeros)"""
    feat = seeded((BS, 1024), 22, 0.3)
    init = seeded((BS * S, case['D']), 41) * N.ve_prior_sigma(case['T0'])
    if case['init'] == 'zeros':
        init = torch.zeros_like(init)
    return feat, init


def perturbed(init, seed, rel=2e-7):
    """the start state under ``rel`` relative noise, rounded to float32 again"""
    noise = np.random.default_rng(seed).normal(size=tuple(init.shape))
    return torch.from_numpy((init.double().numpy() * (1.0 + rel * noise)).astype(np.float32))


class Rhs:
    """The right-hand side of oracle/nets.py::ode_sample (``fun``) and its denoise step, float32 casts included.  ``fp64``: the same
    network evaluated in float64 (weights, features, activations) and rounded to float32 at its output; everything around it unchanged."""

    def __init__(self, sd, prefix, feat_img, D, fp64=False):
        self.p, self.D, self.R, self.fp64 = prefix, D, feat_img.shape[0] * S, fp64
        feat = feat_img[:, None].repeat(1, S, 1).reshape(-1, 1024)
        if fp64:
            self.sd = {k: v.double() for k, v in sd.items() if k.startswith(prefix + '.')}
            self.feat = feat.double()
        else:
            self.sd, self.feat = sd, feat
        self.nfev = 0

    def _score(self, x32, ts32):
        if self.fp64:
            return N.denoiser(self.sd, self.p, self.feat, x32.double(), ts32.double()).float()
        return N.denoiser(self.sd, self.p, self.feat, x32, ts32)

    def __call__(self, t, y):
        self.nfev += 1
        x = torch.tensor(y.reshape(-1, self.D)).float()
        ts = torch.ones(self.R).unsqueeze(-1) * t
        g = N.ve_diffusion(torch.tensor(t)).numpy()
        s = self._score(x, ts)
        s = torch.nan_to_num(s, nan=0.0, posinf=0.0, neginf=0.0) if torch.isnan(s).any() else s
        c = np.float32(0.5 * (g ** 2))
        return np.asarray(0 - c * s.numpy().reshape(-1), dtype=np.float64)

    def denoise(self, y_final, num_steps):
        """score_based_model.py:95-104 as oracle/nets.py::ode_sample states it; y_final (R*D,) f64 -> x (R,D) f64"""
        x = torch.tensor(y_final).reshape(self.R, self.D)
        vec = torch.ones((self.R, 1)) * EPS
        g = N.ve_diffusion(vec)
        grad = self._score(x.float(), vec)
        return x + (0 - g ** 2 * grad) * ((1 - EPS) / num_steps)


def _norm(x):
    return np.linalg.norm(x) / x.size ** 0.5


def initial_step(fun, T0, eps, y0, rtol, atol):
    """the oracle's select_initial_step for the solve T0 -> eps from y0 (R, D) float32: (|h| of the first attempt, f(T0, y0))"""
    y = np.asarray(y0.reshape(-1).numpy(), dtype=np.float64).copy()
    t = float(T0)
    f0 = fun(t, y)
    return float(select_initial_step(fun, t, y, eps, MAX_STEP, f0, -1.0, 4, rtol, atol)), f0


def forced_replay(fun, T0, eps, y0, steps, rtol, atol, num_steps):
    """The oracle's RK45 (oracle/rk45.py::solve_rk45: same stages, same error norm, same t_eval loop and dense-output polynomial) with
    the controller's decisions taken from ``steps`` = [(t, h, err, accepted)]: attempt i starts at the logged t_i with the logged h_i
    and is kept iff its logged flag says so (a rejected attempt keeps y and K[0]); an accepted attempt ends at the next attempt's t
    (the last one at eps).  ``fun``: an Rhs.  y0 (R, D) float32 tensor.
    Returns dict(err (n_attempts,), xs (R, num_steps, D) f64, y (R, D) f64, x (R, D) f64 after the denoise step, h_init = the
    oracle's select_initial_step, nfev)."""
    y = np.asarray(y0.reshape(-1).numpy(), dtype=np.float64).copy()
    n = y.size
    fun.nfev = 0
    t = float(T0)
    h_init, fcur = initial_step(fun, T0, eps, y0, rtol, atol)
    K = np.empty((7, n))
    te = np.linspace(T0, eps, num_steps)[::-1]
    te_i = te.shape[0]
    ys, errs = [], []
    for i, (t_log, h, _e, accepted) in enumerate(steps):
        t, h = np.float64(t_log), np.float64(h)
        K[0] = fcur
        for s in range(1, 6):
            dy = np.dot(K[:s].T, A[s, :s]) * h
            K[s] = fun(t + C[s] * h, y + dy)
        y_new = y + h * np.dot(K[:-1].T, B)
        f_new = fun(t + h, y_new)
        K[-1] = f_new
        scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
        errs.append(_norm(np.dot(K.T, E) * h / scale))
        if not accepted:
            continue
        t_new = np.float64(steps[i + 1][0]) if i + 1 < len(steps) else np.float64(eps)
        te_new = np.searchsorted(te, t_new, side='left')
        step = te[te_new:te_i][::-1]
        if step.size > 0:
            Q = K.T.dot(P)
            x = (step - t) / h
            p = np.cumprod(np.tile(x, (4, 1)), axis=0)
            ys.append(h * np.dot(Q, p) + y[:, None])
            te_i = te_new
        y, fcur = y_new, f_new
    yy = np.hstack(ys) if ys else np.zeros((n, 0))
    xs = torch.tensor(yy).T.reshape(-1, fun.R, fun.D).permute(1, 0, 2)
    nfev = fun.nfev
    x = fun.denoise(yy[:, -1], num_steps)                    # the oracle denoises the LAST STAMP (dense output at eps), not y
    return dict(err=np.asarray(errs), xs=xs, y=torch.tensor(y).reshape(fun.R, fun.D), x=x, h_init=float(h_init), nfev=nfev + 1)


def free_run(sd, case, init=None):
    """the oracle's own solve of a case: (xs (R,stamps,D), x (R,D), info) of oracle/nets.py::ode_sample"""
    feat, init0 = case_inputs(case)
    init = init0 if init is None else init
    rows = feat[:, None].repeat(1, S, 1).reshape(-1, 1024)
    return N.ode_sample(sd, f"denoiser_{case['net']}", rows, init, case['T0'], case['stamps'], rtol=case['rtol'], atol=case['atol'])


_FREE = {}


def cached_free_run(weights, name):
    """one free run per case and process, shared by the tests (nobody changes it)"""
    if name not in _FREE:
        _FREE[name] = free_run(weights[CASES[name]['weights']], CASES[name])
    return _FREE[name]


def rhs_of(weights, name, fp64=False):
    case = CASES[name]
    return Rhs(weights[case['weights']], f"denoiser_{case['net']}", case_inputs(case)[0], case['D'], fp64)


# ----------------------------------------------------------------------------------------------- the controller, restated
def _growth(err):
    return math.inf if err == 0 else 0.9 * err ** -0.2


def check_log(steps, stats, T0, eps, num_steps):
    """scipy's scalar step controller (RungeKutta._step_impl) on a step log [(t, h, err, accepted)] of a backward solve T0 -> eps:
    raises AssertionError naming the rule an attempt breaks.  Every attempt is predicted from the previous attempt's own logged
    (t, h, err), so a correct log differs from the prediction by the last bits of pow() only.  ``stats``: nfev (with the denoise call),
    and n_accepted / n_rejected where the solver reports them.  Returns a summary dict of what the log contains."""
    assert num_steps >= 1 and T0 > eps
    n = len(steps)
    assert n > 0, 'empty log'
    t_expect, rejected, h_pred = float(T0), False, None
    out = dict(attempts=n, n_accepted=0, n_rejected=0, max_consecutive_rejects=0, clamped_to_one=0, max_factor=0, landed=False)
    run = 0
    for i, (t, h, err, acc) in enumerate(steps):
        t, h, err, acc = float(t), float(h), float(err), bool(acc)
        assert not out['landed'], f'attempt {i}: an attempt after the solve landed on eps'
        assert t == t_expect, f'attempt {i}: t {t!r} != {t_expect!r} (time bookkeeping)'
        assert h < 0 and math.isfinite(h), f'attempt {i}: h {h!r} is not a backward step'
        assert math.isfinite(err) and err >= 0, f'attempt {i}: error norm {err!r}'
        assert acc == (err < 1), f'attempt {i}: accept flag {acc} with error norm {err!r}'
        ulp = abs(math.nextafter(t, -math.inf) - t)
        # h = eps - t is rounded on the grid of t when eps < t / 2, so t + h may miss eps by less than ulp(t)
        assert t + h >= eps - ulp, f'attempt {i}: t + h = {t + h!r} passes eps (not clipped)'
        min_step = 10 * ulp
        if h_pred is not None:
            if not rejected:                                     # first attempt of a step: clamp (never on a retry)
                h_pred = MAX_STEP if h_pred > MAX_STEP else (min_step if h_pred < min_step else h_pred)
            else:
                assert h_pred >= min_step, f'attempt {i}: step size underflow'
            want = min(h_pred, t - eps)                          # t + h clipped to eps
            # t_new = t + h is rounded to the grid of t before h = t_new - t is logged: one ulp(t) on top of the relative tolerance
            assert abs(-h - want) <= H_RTOL * want + ulp, f'attempt {i}: step size |h| {-h!r}, the controller gives {want!r}'
        else:
            assert -h <= T0 - eps, f'attempt {i}: first step longer than the interval'
        if acc:
            out['n_accepted'] += 1
            run = 0
            t_next = float(steps[i + 1][0]) if i + 1 < n else None
            g = _growth(err)
            factor = min(10.0, g)
            if factor == 10.0:
                out['max_factor'] += 1
            if rejected:
                if g > 1:
                    out['clamped_to_one'] += 1
                factor = min(1.0, factor)
            h_pred = -h * factor
            rejected = False
            if t_next is None or t_next == eps:
                t_next = float(eps)
                assert i + 1 == n, f'attempt {i}: landed on eps but the log goes on'
                out['landed'] = True
            # scipy: h = t_new - t with t_new = t + h_abs * direction (or tf).  t + h == t_new follows wherever t_new - t is exact
            # (Sterbenz: t_new >= t / 2); below that h itself carries a rounding error and only its definition can be asked for.
            assert h == t_next - t, f'attempt {i}: h {h!r} != t_next - t = {t_next - t!r}'
            if t_next >= t / 2:
                assert t_next == t + h, f'attempt {i}: next t {t_next!r} != t + h = {t + h!r}'
            t_expect = t_next
        else:
            out['n_rejected'] += 1
            run += 1
            out['max_consecutive_rejects'] = max(out['max_consecutive_rejects'], run)
            h_pred = -h * max(0.2, _growth(err))
            rejected = True
            t_expect = t
    assert out['landed'], 'the last attempt is not an accepted step onto eps'
    assert stats['nfev'] == 2 + 6 * n + 1, f"nfev {stats['nfev']} != 2 + 6 * {n} + 1"
    for k in ('n_accepted', 'n_rejected'):
        if k in stats:
            assert stats[k] == out[k], f'{k}: {stats[k]} reported, {out[k]} in the log'
    return out


def simulate_log(errs, T0, eps, h0, min_factor=0.2, clamp_after_reject=True, clip=True):
    """A step log made by the controller itself from a GIVEN sequence of error norms (0.5 once they run out): self-consistent by
    construction, and with a switch per rule so that a test can make the log of a controller that breaks exactly one rule."""
    t, h_abs, log, it = float(T0), float(h0), [], iter(errs)
    while t != eps and len(log) < 10000:
        min_step = 10 * abs(math.nextafter(t, -math.inf) - t)
        h_abs = MAX_STEP if h_abs > MAX_STEP else (min_step if h_abs < min_step else h_abs)
        accepted = rejected = False
        while not accepted:
            t_new = t - h_abs
            if t_new < eps:
                t_new = eps if clip else max(t_new, eps / 2)
            h = t_new - t
            h_abs = abs(h)
            err = next(it, 0.5)
            if err < 1:
                factor = min(10.0, _growth(err))
                if rejected and clamp_after_reject:
                    factor = min(1.0, factor)
                accepted = True
            else:
                factor = max(min_factor, _growth(err))
                rejected = True
            log.append((t, h, err, accepted))
            h_abs *= factor
        t = t_new if t_new > eps else eps
    return log


def has_accept_after_reject(steps):
    return any((not a[3]) and b[3] for a, b in zip(steps, steps[1:]))


def stamps_per_accept(steps, T0, eps, num_steps):
    """how many t_eval stamps each accepted attempt writes"""
    te = np.linspace(T0, eps, num_steps)
    out, nxt = [], 0
    for i, (t, h, _e, acc) in enumerate(steps):
        if not acc:
            continue
        t_new = steps[i + 1][0] if i + 1 < len(steps) else eps
        k = nxt
        while k < num_steps and te[k] >= t_new:
            k += 1
        out.append(k - nxt)
        nxt = k
    return out

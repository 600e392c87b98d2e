"""numpy float64 restatement of the hand benchmark metrics (--eval_hand_bench): the FreiHAND / HO3D leaderboard
definitions written out plainly, by another route than csrc/hand_bench.hip wherever there is one -- the alignment by ``np.linalg.svd``
(the kernel: eigen-decomposition of H^T H), the AUC count by comparing against the whole table (the kernel: binary search), the nearest
neighbours by brute force on the uncentred float64 points (the kernel: fp32 on centred points).  No GPU, no torch."""
import numpy as np

F_THRESH = (0.005, 0.015)
AUC = (0.0, 0.05, 100)
BAND = 2e-7            # m: the rounding of an fp32 point at camera depth (0.7 m: ulp 6e-8 per coordinate, two points, three coordinates)


def thresholds():
    return np.linspace(AUC[0], AUC[1], AUC[2])


def g_table(t):
    """G[c], c = 0 .. n_t: the trapezoid integral over the table of the step 1[e <= t] of a point with c = #{j : e <= t_j}, divided by
    t[-1] - t[0]; with j0 = n_t - c: ((t[-1] - t[j0]) + (t[j0] - t[j0-1]) / 2 if j0 >= 1) / (t[-1] - t[0]), G[0] = 0"""
    n = t.shape[0]
    g = np.zeros(n + 1)
    for c in range(1, n + 1):
        j0 = n - c
        g[c] = ((t[-1] - t[j0]) + ((t[j0] - t[j0 - 1]) / 2 if j0 >= 1 else 0.0)) / (t[-1] - t[0])
    return g


def postprocess(pd_model, root, is_right):
    """the reference's postprocess in fp32 (x un-flipped for left hands, root added): pd_model (n,S,P,3) -> camera frame, the bits the
    kernel forms as it loads"""
    sgn = np.where(np.asarray(is_right).astype(bool), 1.0, -1.0).astype(np.float32)[:, None, None]
    v = np.asarray(pd_model, np.float32).copy()
    v[..., 0] = v[..., 0] * sgn
    return (v + np.asarray(root, np.float32)[:, None, None]).astype(np.float32)


def align(A, B):
    """rigid_align_AtoB (similarity with scale and the reflection fix) in float64 by np.linalg.svd: A, B (P,3) -> c R A + t"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ca, cb = A.mean(0), B.mean(0)
    H = (A - ca).T @ (B - cb) / A.shape[0]
    U, s, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        s = s.copy()
        s[-1] = -s[-1]
        Vt = Vt.copy()
        Vt[2] = -Vt[2]
        R = Vt.T @ U.T
    c = s.sum() / ((A - ca) ** 2).sum(1).mean()
    return (c * R @ A.T).T + (cb - c * R @ ca)


def errors(X, B):
    return np.sqrt(((np.asarray(X, np.float64) - np.asarray(B, np.float64)) ** 2).sum(-1))


def pck_counts(e, t):
    return (e[:, None] <= t[None, :]).sum(1)


def nn_dists(X, B):
    """d1 (each point of B to its nearest of X), d2 (each point of X to its nearest of B): brute force, float64"""
    X, B = np.asarray(X, np.float64), np.asarray(B, np.float64)
    d = np.sqrt(((X[:, None, :] - B[None, :, :]) ** 2).sum(-1))          # [p of X][q of B]
    return d.min(0), d.min(1)


def f_score(n1, n2, P):
    p, r = n1 / P, n2 / P
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def pair(A, B, with_fscore=True, t=None, g=None):
    """one (hand, ground truth) pair, A and B (P,3) camera-frame fp32 points -> values (6,) [AUC, PA AUC, F@lo, F@hi, PA F@lo, PA F@hi]
    (the F entries NaN without with_fscore), counts (10,) int as the kernel's, band (8,): the number of nearest-neighbour distances of
    each of the eight counts within BAND of its threshold, margin: (smallest |e - t_j| over points and table entries, smallest
    |d - th| over distances and thresholds)"""
    t = thresholds() if t is None else t
    g = g_table(t) if g is None else g
    P = A.shape[0]
    values, counts, band = np.full(6, np.nan), np.zeros(10, np.int64), np.zeros(8, np.int64)
    m_e, m_d = np.inf, np.inf
    if not (np.isfinite(A).all() and np.isfinite(B).all()):
        return values, counts, band, (m_e, m_d)
    H = align(A, B)
    for k, X in enumerate((A, H)):
        e = errors(X, B)
        c = pck_counts(e, t)
        values[k] = g[c].sum() / P
        counts[8 + k] = c.sum()
        m_e = min(m_e, np.abs(e[:, None] - t[None, :]).min())
        if with_fscore:
            d1, d2 = nn_dists(X, B)
            for j, d in enumerate((d1, d2)):
                for i, th in enumerate(F_THRESH):
                    counts[k * 4 + j * 2 + i] = (d < th).sum()
                    band[k * 4 + j * 2 + i] = (np.abs(d - th) <= BAND).sum()
                    m_d = min(m_d, np.abs(d - th).min())
            for i in range(2):
                values[2 + k * 2 + i] = f_score(counts[k * 4 + i], counts[k * 4 + 2 + i], P)
    return values, counts, band, (m_e, m_d)


def bench_multi(pd_model, gt, root, is_right, with_fscore=True):
    """pd_model (n,S,P,3) model frame, gt (n,P,3), root (n,3), is_right (n,) -> values (n,S,6), counts (n,S,10), band (n,S,8), margins"""
    cam = postprocess(pd_model, root, is_right)
    n, S = cam.shape[:2]
    t = thresholds()
    g = g_table(t)
    values, counts, band = np.zeros((n, S, 6)), np.zeros((n, S, 10), np.int64), np.zeros((n, S, 8), np.int64)
    m_e, m_d = np.inf, np.inf
    for b in range(n):
        for s in range(S):
            values[b, s], counts[b, s], band[b, s], m = pair(cam[b, s], np.asarray(gt[b], np.float32), with_fscore, t, g)
            m_e, m_d = min(m_e, m[0]), min(m_d, m[1])
    return values, counts, band, (m_e, m_d)


def values_from_counts(counts, P, auc):
    """the F entries recomputed from integer counts (n,S,10) by the F rule; ``auc`` (n,S,2) is passed through"""
    out = np.zeros(counts.shape[:2] + (6,))
    out[..., :2] = auc
    for idx in np.ndindex(*counts.shape[:2]):
        c = counts[idx]
        for k in range(2):
            for i in range(2):
                out[idx + (2 + k * 2 + i,)] = f_score(int(c[k * 4 + i]), int(c[k * 4 + 2 + i]), P)
    return out


def table_rule(per):
    """per (n,S,8) -> one, best, mean (n,8): hypothesis 0, the per-value maximum, the mean (sum in ascending s); NaN propagates"""
    one = per[:, 0].copy()
    best = per.max(1)                                  # np.max propagates NaN
    mean = np.zeros_like(one)
    for s in range(per.shape[1]):
        mean = mean + per[:, s]
    return one, best, mean / per.shape[1]


def synthetic(n, S, P, seed):
    """points on a bumpy 0.1 m ellipsoid at depth 0.6 m as ground truth (camera frame, fp32); hypotheses rotated, scaled and noised at
    2 / 8 / 30 mm (cycling over s), returned in the MODEL frame with roots and handedness (every other hand is a left one)"""
    rng = np.random.default_rng(seed)
    is_right = (np.arange(n) % 2) == 0
    root = (rng.normal(size=(n, 3)) * 0.03 + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    u = rng.normal(size=(n, P, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    bump = 1.0 + 0.15 * np.sin(7.0 * u[..., :1]) * np.cos(5.0 * u[..., 1:2])
    shape = u * bump * np.array([0.05, 0.035, 0.02])
    gt = (shape + root[:, None]).astype(np.float32)
    pd = np.zeros((n, S, P, 3), np.float32)
    noise = (0.002, 0.008, 0.030)
    for b in range(n):
        for s in range(S):
            w = rng.normal(size=3) * 0.2
            th = np.linalg.norm(w)
            K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
            R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
            cam = (1.0 + 0.1 * rng.normal()) * shape[b] @ R.T + root[b] + rng.normal(size=(P, 3)) * noise[s % 3] + rng.normal(size=3) * noise[s % 3]
            m = (cam.astype(np.float32) - root[b]).astype(np.float32)
            if not is_right[b]:
                m[:, 0] = -m[:, 0]
            pd[b, s] = m
    return pd, gt, root, is_right


def find_seed(n, S, P, start=0, margin_e=1e-9, margin_d=BAND, tries=64):
    """the first seed from ``start`` whose synthetic case keeps every error margin_e and every nearest-neighbour distance margin_d away
    from its thresholds (run on the CPU when a shape is added; the seeds are recorded in tests/test_gpu_hand_bench.py)"""
    for seed in range(start, start + tries):
        m = bench_multi(*synthetic(n, S, P, seed))[3]
        if m[0] > margin_e and m[1] > margin_d:
            return seed, m
    raise RuntimeError('no seed found')

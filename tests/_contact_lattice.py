"""Contact-detection inputs on which the fp32 arithmetic of csrc/contact.hip is exact, so that a float64 reference is exact too and a test
can ask for equality on every element.  Every coordinate, offset and threshold is a multiple of U = 2^-12 m with magnitude below 2^-2 m:
differences are multiples of U below 2^-2, squared distances multiples of U^2 = 2^-24 below 2^-2 -- 22 bits, inside fp32's 24 -- the
normals are +-e_z, so the signed normal distance is a coordinate difference, and the tangential distance sqrt(k U^2) is compared with a
threshold T = m U, where a correctly rounded sqrt decides as k < m^2 does.  No GPU, no torch."""
import numpy as np

U = 2.0 ** -12
PITCH = 2.0 ** -7                                   # 32 U
NORMAL_THRESH = (-2.0 ** -6, 2.0 ** -7)             # (-64 U, 32 U)
VERTICAL_THRESH = 2.0 ** -7                         # 32 U
DECAY = (-2.0 ** -8, 2.0 ** -8)                     # (-16 U, 16 U): the sigmoid flanks are centred on -40 U and 24 U
KW = dict(normal_thresh=NORMAL_THRESH, vertical_thresh=VERTICAL_THRESH, decay=DECAY)
SEAM_SIZES = ((1, 1), (255, 1023), (256, 1024), (257, 1025), (513, 2049), (300, 3000), (1100, 2))      # (queries, targets)
_SIDE = 16                                          # the lattice has 16^3 = 4096 sites


def is_exact(a):
    """every value an fp32 multiple of U below 2^-2 in magnitude"""
    a = np.asarray(a)
    k = np.asarray(a, np.float64) / U
    return bool(a.dtype == np.float32 and (k == np.round(k)).all() and (np.abs(k) < 2 ** 10).all())


def _sites(rng, nt):
    idx = rng.permutation(_SIDE ** 3)[:nt]
    return (np.stack([idx // (_SIDE * _SIDE), (idx // _SIDE) % _SIDE, idx % _SIDE], -1) * PITCH).astype(np.float32)


def seam_case(nq, nt, seed):
    """targets: ``nt`` sites of the lattice k * 2^-7 in shuffled order, normals +-e_z; query i sits at target own[i], displaced by d_i U
    along z (|d_i| <= 7) and tau_i U along x (0 <= tau_i <= 7), normal sign_i e_z.  own includes 0, 1023, 1024 and nt - 1 (clipped to
    nt - 1) as far as nq allows, and those queries have tau = 0: whichever other target a kernel took for them, it lies >= 32 U away
    tangentially (outside the gate: weight 0) or +-32 U away along the normal (another weight).  The squared distance to the own target is
    at most 98 U^2, to any other at least 25^2 U^2: the runner-up is 576 U^2 = 3.4e-5 m^2 behind in fp32 and in fp64.
    -> dict(targets (nt,3), target_normals, queries (nq,3), query_normals, own (nq,), nd (nq,) float64 signed normal distance)"""
    rng = np.random.default_rng([seed, nq, nt])
    targets = _sites(rng, nt)
    own = rng.integers(0, nt, size=nq)
    special = np.unique(np.clip([0, 1023, 1024, nt - 1], 0, nt - 1))
    pos = rng.permutation(nq)[:len(special)]
    own[pos] = special[:len(pos)]
    d = rng.integers(-7, 8, size=nq)
    tau = rng.integers(0, 8, size=nq)
    tau[pos] = 0
    sign = rng.choice([-1.0, 1.0], size=nq)
    queries = targets[own].astype(np.float64)
    queries[:, 2] += d * U
    queries[:, 0] += tau * U
    qn = np.zeros((nq, 3), np.float32)
    qn[:, 2] = sign
    tn = np.zeros((nt, 3), np.float32)
    tn[:, 2] = rng.choice([-1.0, 1.0], size=nt)
    return dict(targets=targets, target_normals=tn, queries=queries.astype(np.float32), query_normals=qn, own=own.astype(np.int32),
                nd=d * U * sign, seam_queries=pos)


def gate_case():
    """four targets 2^-4 apart along x; queries above them with the signed normal distance nd and the tangential distance vd (along y) on
    and next to every strict gate, and nd swept in steps of U over (-64 U, 32 U), i.e. across both sigmoid flanks.
    -> dict(targets, target_normals, queries, query_normals, own, nd, vd, inside (nq,) bool by construction)"""
    nlo, nhi, vt = NORMAL_THRESH[0] / U, NORMAL_THRESH[1] / U, VERTICAL_THRESH / U
    rows = [(nlo, 0, False), (nlo + 1, 0, True), (nhi - 1, 0, True), (nhi, 0, False),
            (0, vt - 1, True), (0, vt, False), (nlo + 1, vt - 1, True), (nhi - 1, vt, False)]
    rows += [(k, 0, True) for k in range(int(nlo) + 1, int(nhi))]
    nd = np.array([r[0] for r in rows], np.float64) * U
    vd = np.array([r[1] for r in rows], np.float64) * U
    inside = np.array([r[2] for r in rows])
    nq = len(rows)
    targets = np.zeros((4, 3), np.float32)
    targets[:, 0] = np.arange(4) * 2.0 ** -4
    own = np.arange(nq) % 4
    sign = np.where(np.arange(nq) % 3 == 0, -1.0, 1.0)
    queries = targets[own].astype(np.float64)
    queries[:, 2] += nd * sign                      # (q - t) . (sign e_z) = nd
    queries[:, 1] += vd
    qn = np.zeros((nq, 3), np.float32)
    qn[:, 2] = sign
    tn = np.zeros((4, 3), np.float32)
    tn[:, 2] = 1.0
    return dict(targets=targets, target_normals=tn, queries=queries.astype(np.float32), query_normals=qn, own=own.astype(np.int32), nd=nd, vd=vd,
                inside=inside)


def tie_case(second):
    """1100 lattice targets with the point of index 5 stored again at index ``second`` (9: the same LDS tile, 1030: across the seam at 1024);
    32 queries next to that point, the rest spread as in seam_case.  The smaller index, 5, must be reported."""
    c = seam_case(64, 1100, 17)
    assert second != 5 and not (c['own'] == second).any()
    c['targets'][second] = c['targets'][5]
    c['own'][:32] = 5
    q = c['targets'][c['own']].astype(np.float64)
    rng = np.random.default_rng(second)
    d, tau = rng.integers(-7, 8, size=64), rng.integers(0, 8, size=64)
    q[:, 2] += d * U
    q[:, 0] += tau * U
    c['queries'] = q.astype(np.float32)
    c['nd'] = d * U * c['query_normals'][:, 2].astype(np.float64)
    del c['seam_queries']
    return c


def closed_form_weight(nd):
    """the double sigmoid of physics_fn.py:47-117 at the thresholds above, normalised by its value at 0, float64"""
    mid1, mid2 = (DECAY[0] + NORMAL_THRESH[0]) / 2, (DECAY[1] + NORMAL_THRESH[1]) / 2
    f = lambda x: 1.0 / ((1.0 + np.exp(-1600.0 * (x - mid1))) * (1.0 + np.exp(1600.0 * (x - mid2))) + 1e-10)
    return f(np.asarray(nd, np.float64)) / f(0.0)


# ------------------------------------------------------------------------------------------------------------ force_contact inputs
GROUPS = ('palm', 'thumb', 'index', 'middle', 'ring', 'pinky')


def private_anchors(anchor):
    """{group: anchors of the group whose three face vertices no other anchor's face uses}: contact on them reaches that group alone"""
    from oracle.contact import FINGER_LABEL
    face = np.asarray(anchor['face_vert_idx']).reshape(32, 3)
    uses = np.bincount(face.reshape(-1), minlength=778)
    return {g: [a for a in FINGER_LABEL[g] if (uses[face[a]] == 1).all()] for g in GROUPS}


def force_inputs(anchor, n, ld, positive_groups, seed, levels=None):
    """hand_contact (n, ld) fp32, zero except on the three face vertices of one private anchor of each of the first positive_groups[i]
    finger groups of sample i; columns 778.. hold NaN.  The touched vertices get seeded values in (0.25, 1), or levels[k] for the k-th
    group.  -> hand_contact, chosen (n, 6) int: the anchor touched per group, -1 for none"""
    rng = np.random.default_rng(seed)
    face = np.asarray(anchor['face_vert_idx']).reshape(32, 3)
    private = private_anchors(anchor)
    hc = np.zeros((n, ld), np.float32)
    hc[:, 778:] = np.nan
    chosen = np.full((n, 6), -1)
    for i in range(n):
        for k, g in enumerate(GROUPS[:positive_groups[i]]):
            a = private[g][int(rng.integers(0, len(private[g])))] if levels is None else private[g][0]      # levels: the same anchors in every sample
            chosen[i, k] = a
            hc[i, face[a]] = np.float32(levels[k]) if levels is not None else rng.uniform(0.25, 1.0, size=3).astype(np.float32)
    return hc, chosen

"""NumPy fp64 restatement of csrc/contact_multi.hip by brute force: the hand -> object contact map of (hand, object pose) pairs in the
object's model frame over ALL object vertices, the agreement columns and the S-reduction -- and the seeded scenes its tests share.
Operation for operation the kernel's expressions (sums left to right, no fused multiply-add), so nd / vd agree to rounding of exp alone."""
import numpy as np

GATES = dict(normal_thresh=(-0.01, 0.01), vertical_thresh=0.005, decay=(-0.005, 0.005))      # Config's defaults and PhysicsLabeler.DECAY
SIZES = (1, 31, 32, 33, 300, 4500)


def _f32(x):
    return float(np.float32(x))


def contact_weight(nd, normal_thresh, decay):
    """contact_weight(nd) / w0 of contact.hip, clamped to [0, 1]; the gates are fp32 numbers widened to fp64, as the entry point takes them"""
    mid1 = (_f32(decay[0]) + _f32(normal_thresh[0])) / 2
    mid2 = (_f32(decay[1]) + _f32(normal_thresh[1])) / 2

    def fn(x):
        with np.errstate(over='ignore'):
            m1 = 1.0 + np.exp(-1600.0 * (x - mid1))
            m2 = 1.0 + np.exp(1600.0 * (x - mid2))
            w = 1.0 / (m1 * m2 + 1e-10)
        return np.where(np.isfinite(m1) & np.isfinite(m2), w, 0.0)
    return np.clip(fn(np.asarray(nd, np.float64)) / fn(np.zeros(1))[0], 0.0, 1.0)


def _rt_dot(R, x, transpose):
    """R^T x (or R x) of (3, 3) with (P, 3), each component a sum of three products left to right"""
    M = R.T if transpose else R
    return np.stack([M[k, 0] * x[:, 0] + M[k, 1] * x[:, 1] + M[k, 2] * x[:, 2] for k in range(3)], -1)


def model_frame(h, g, root, right, rt):
    """filled hand vertices h and normals g (Nh, 3) fp32 of one pair -> p, m (Nh, 3) fp64 in the object's model frame"""
    sg = 1.0 if right else -1.0
    h, g = np.asarray(h, np.float32).astype(np.float64), np.asarray(g, np.float32).astype(np.float64)
    d = np.stack([(h[:, 0] * sg + root[0]) - rt[0, 3], (h[:, 1] + root[1]) - rt[1, 3], (h[:, 2] + root[2]) - rt[2, 3]], -1)
    return _rt_dot(rt[:, :3], d, True), _rt_dot(rt[:, :3], np.stack([g[:, 0] * sg, g[:, 1], g[:, 2]], -1), True)


def contact_multi(vf, nf, root, is_right, rt, objects, obj_id, normal_thresh, vertical_thresh, decay):
    """vf, nf (n, S, Nh, 3) fp32, root (n, 3), is_right (n,), rt (n, S, 3, 4) fp64, objects: list of (N_o, 3) vertex arrays, obj_id (n,).
    -> dict: weight (n, S, Nh) fp64 (before the fp32 store), contact bool, nearest (the brute-force index of EVERY vertex), nn (-1 without
    contact), nd, vd, gap (n, S, Nh): (second smallest d2 - smallest d2) / smallest d2 (inf with one vertex, nan for 0 / 0).
    A pair with a non-finite input or an obj_id outside the list: NaN weight / nd / vd, nn = nearest = -1."""
    vf, nf = np.asarray(vf, np.float32), np.asarray(nf, np.float32)
    n, S, Nh = vf.shape[:3]
    lo, hi, vt = _f32(normal_thresh[0]), _f32(normal_thresh[1]), _f32(vertical_thresh)
    out = dict(weight=np.full((n, S, Nh), np.nan), contact=np.zeros((n, S, Nh), bool), nearest=np.full((n, S, Nh), -1, np.int64),
               nn=np.full((n, S, Nh), -1, np.int64), nd=np.full((n, S, Nh), np.nan), vd=np.full((n, S, Nh), np.nan), gap=np.full((n, S, Nh), np.nan))
    for i in range(n):
        o = int(obj_id[i])
        for s in range(S):
            if not (0 <= o < len(objects)) or not all(np.isfinite(np.asarray(a, np.float64)).all() for a in (vf[i, s], nf[i, s], root[i], rt[i, s])):
                continue
            v = np.asarray(objects[o], np.float64).reshape(-1, 3)
            p, m = model_frame(vf[i, s], nf[i, s], np.asarray(root[i], np.float64), bool(is_right[i]), np.asarray(rt[i, s], np.float64))
            d = p[:, None, :] - v[None, :, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            nn = d2.argmin(1)                                             # the first minimum: the smaller index on a tie
            if v.shape[0] > 1:
                two = np.partition(d2, 1, axis=1)[:, :2]
                with np.errstate(invalid='ignore', divide='ignore'):
                    out['gap'][i, s] = (two[:, 1] - two[:, 0]) / two[:, 0]
            else:
                out['gap'][i, s] = np.inf
            e = p - v[nn]
            nd = e[:, 0] * m[:, 0] + e[:, 1] * m[:, 1] + e[:, 2] * m[:, 2]
            r = e - nd[:, None] * m
            vd = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
            c = (nd > lo) & (nd < hi) & (vd < vt)
            out['nd'][i, s], out['vd'][i, s], out['contact'][i, s], out['nearest'][i, s] = nd, vd, c, nn
            out['nn'][i, s] = np.where(c, nn, -1)
            out['weight'][i, s] = np.where(c, contact_weight(nd, normal_thresh, decay), 0.0)
    return out


def gate_distance(ref, normal_thresh, vertical_thresh):
    """how far (m) each vertex of a contact_multi result is from the nearest of the three gates"""
    lo, hi, vt = _f32(normal_thresh[0]), _f32(normal_thresh[1]), _f32(vertical_thresh)
    return np.minimum(np.minimum(np.abs(ref['nd'] - lo), np.abs(ref['nd'] - hi)), np.abs(ref['vd'] - vt))


def agreement(w, w_gt, fc, gr, fc_gt, gr_gt):
    """w (n, S, Nh), w_gt (n, Nh) fp32 maps, fc (n, S, 32) / gr (n, S) against fc_gt (n, 32) / gr_gt (n,) -> counts (n, S, 3) int,
    values (n, S, 8) fp64: IoU, precision, recall, F1, MAE, anchor_agree, grasped, grasp_agree; a pair with a NaN in either map: NaN, 0"""
    w, w_gt = np.asarray(w, np.float32), np.asarray(w_gt, np.float32)
    n, S, Nh = w.shape
    counts, values = np.zeros((n, S, 3), np.int64), np.full((n, S, 8), np.nan)
    div = lambda a, b: a / b if b else np.nan
    for i in range(n):
        for s in range(S):
            if np.isnan(w[i, s]).any() or np.isnan(w_gt[i]).any():
                continue
            c, g = w[i, s] > 0, w_gt[i] > 0
            TP, P, G = int((c & g).sum()), int(c.sum()), int(g.sum())
            counts[i, s] = TP, P, G
            same = int(((np.asarray(fc[i, s]) > 0) == (np.asarray(fc_gt[i]) > 0)).sum())
            values[i, s] = (div(TP, P + G - TP), div(TP, P), div(TP, G), div(2 * TP, P + G),
                            np.abs(w[i, s].astype(np.float64) - w_gt[i].astype(np.float64)).sum() / Nh, same / 32.0,
                            float(bool(gr[i, s])), float(bool(gr[i, s]) == bool(gr_gt[i])))
    return counts, values


def table(values):
    """(n, S, 8) -> (n, 24): hypothesis 0 | best-of-S (max, MAE min) | mean-of-S, NaNs left out, NaN where a value never is defined"""
    n, S, _ = values.shape
    out = np.full((n, 24), np.nan)
    out[:, :8] = values[:, 0]
    for i in range(n):
        for j in range(8):
            v = values[i, :, j]
            v = v[~np.isnan(v)]
            if len(v):
                out[i, 8 + j] = v.min() if j == 4 else v.max()
                acc = 0.0
                for x in v:
                    acc += x
                out[i, 16 + j] = acc / len(v)
    return out


# ------------------------------------------------------------------------------------------------------------------ seeded scenes
def ellipsoid(n_verts, seed):
    """n_verts points on an ellipsoid of half-axes 4 x 5 x 6 cm about (1, -2, 0.5) cm: an object's full vertices in its model frame"""
    r = np.random.default_rng(seed)
    u = r.normal(size=(n_verts, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u * np.array([0.04, 0.05, 0.06]) + np.array([0.01, -0.02, 0.005])


def objects(seed=0):
    """one ellipsoid per entry of SIZES"""
    return [ellipsoid(k, seed + 17 * i) for i, k in enumerate(SIZES)]


def rotation(r):
    q = r.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(seed, n, S, obj_id, objs, Nh=1080, spread=0.012, tangent=0.002):
    """Seeded near-contact pairs: every hand vertex sits within ``spread`` of an object vertex along the direction away from the object's
    centre, moved sideways by ~``tangent``, its normal pointing roughly back at the object; poses at arm's length from the camera, left
    and right hands alternating.  -> vf, nf (n, S, Nh, 3) fp32 in the flipped, root-relative frame, root (n, 3), is_right (n,) uint8,
    rt (n, S, 3, 4) fp64"""
    r = np.random.default_rng(seed)
    vf, nf = np.zeros((n, S, Nh, 3), np.float32), np.zeros((n, S, Nh, 3), np.float32)
    root = r.normal(size=(n, 3)) * 0.05 + np.array([0.03, -0.02, 0.6])
    is_right = (np.arange(n) % 2 == 0).astype(np.uint8) if n > 1 else np.array([seed % 2], np.uint8)
    rt = np.zeros((n, S, 3, 4))
    for i in range(n):
        v = np.asarray(objs[int(obj_id[i])], np.float64)
        centre = v.mean(0)
        sg = 1.0 if is_right[i] else -1.0
        for s in range(S):
            R = rotation(r)
            t = root[i] + r.normal(size=3) * 0.03
            rt[i, s, :, :3], rt[i, s, :, 3] = R, t
            pick = v[r.integers(0, len(v), Nh)]
            u = pick - centre
            bad = np.linalg.norm(u, axis=1) < 1e-9
            u[bad] = r.normal(size=(int(bad.sum()), 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            p = pick + u * r.uniform(-spread, spread, (Nh, 1)) + r.normal(size=(Nh, 3)) * tangent
            m = -u + r.normal(size=(Nh, 3)) * 0.2
            m /= np.linalg.norm(m, axis=1, keepdims=True)
            c = p @ R.T + t - root[i]
            g = m @ R.T
            c[:, 0] *= sg
            g[:, 0] *= sg
            vf[i, s], nf[i, s] = c.astype(np.float32), g.astype(np.float32)
    return vf, nf, root, is_right, rt

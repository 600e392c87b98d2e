"""A numpy referee for csrc/raster.hip that restates the rules of include/vpho_hip.h (vpho_mesh_raster_f32, vpho_render_overlay_u8), and the
scenes the raster tests share.  Projection and snapping follow the header's operation order; coverage is decided in 64-bit integers; depth
goes by ANOTHER route than the kernel's barycentric sum: the plane of 1/z over the three snapped corners is fitted by solving the 3x3
system in float64 (corners taken relative to corner 0, an exact integer shift) and evaluated at the pixel centre.  Same tie rules: front =
smallest float64 z, back = largest, the smaller face index among equals.  No GPU."""
import numpy as np

SNAP, SNAP_MAX = 256, 2 ** 30
TIE_REL = 1e-9
FULL_PIXEL_AREA = 2 * 256 ** 2            # integer doubled area of a face of one pixel of screen area


def project_snap(verts, K, z_near=0.01):
    """verts (V,3) float32, K (3,3) float64 -> snapped (V,2) int64, usable (V,) bool.  u = (K00 X + K01 Y) / Z + K02, v = (K11 Y) / Z + K12 in
    float64, every operation rounded once; rint(. * 256), ties to even."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    K = np.asarray(K, np.float64)
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all='ignore'):
        u = (K[0, 0] * X + K[0, 1] * Y) / Z + K[0, 2]
        w = (K[1, 1] * Y) / Z + K[1, 2]
        su, sw = np.rint(u * 256.0), np.rint(w * 256.0)
        ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z > z_near) & (np.abs(su) <= SNAP_MAX) & (np.abs(sw) <= SNAP_MAX)
    snapped = np.stack([np.where(ok, su, 0.0), np.where(ok, sw, 0.0)], -1).astype(np.int64)
    return snapped, ok


def _owns(dx, dy):
    return dy < 0 or (dy == 0 and dx > 0)


def face_setup(snapped, ok, face, H, W):
    """-> None for a dropped face, else ((x0,y0),(x1,y1),(x2,y2)) oriented to positive doubled area, the order of the corners, the doubled
    area and the pixel box (xlo, xhi, ylo, yhi, inclusive, clipped to the image)"""
    i0, i1, i2 = (int(i) for i in face)
    if not (ok[i0] and ok[i1] and ok[i2]):
        return None
    p = [tuple(int(c) for c in snapped[i]) for i in (i0, i1, i2)]
    order = [i0, i1, i2]
    A = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0])
    if A == 0:
        return None
    if A < 0:
        p[1], p[2] = p[2], p[1]
        order[1], order[2] = order[2], order[1]
        A = -A
    xs, ys = [c[0] for c in p], [c[1] for c in p]
    xlo, xhi = max((min(xs) + 127) >> 8, 0), min((max(xs) - 128) >> 8, W - 1)
    ylo, yhi = max((min(ys) + 127) >> 8, 0), min((max(ys) - 128) >> 8, H - 1)
    if xlo > xhi or ylo > yhi:
        return None
    return p, order, A, (xlo, xhi, ylo, yhi)


def face_cover(p, box):
    """exact coverage of the pixel centres of the box by the oriented face: (cover (h,w) bool, CX, CY int64 lattice centres)"""
    xlo, xhi, ylo, yhi = box
    CX, CY = np.meshgrid(np.arange(xlo, xhi + 1, dtype=np.int64) * 256 + 128, np.arange(ylo, yhi + 1, dtype=np.int64) * 256 + 128)
    cover = np.ones(CX.shape, bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = p[b][0] - p[a][0], p[b][1] - p[a][1]
        assert abs(dx) <= 2 ** 31 and abs(dy) <= 2 ** 31
        E = np.int64(dx) * (CY - np.int64(p[a][1])) - np.int64(dy) * (CX - np.int64(p[a][0]))
        cover &= (E > 0) | ((E == 0) & _owns(dx, dy))
    return cover, CX, CY


def raster_image(verts, faces, K, H, W, z_near=0.01):
    """one image -> dict: depth_front / depth_back (H,W) float32 (0 where empty), face_front / face_back int32 (-1), count (covering faces),
    tie (the two best depths of the front OR of the back differ by less than 1e-9 relative), area_front / area_back (int64 doubled area
    of the winning face, 0 where empty), z64_front / z64_back (the float64 depths)."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    snapped, ok = project_snap(verts, K, z_near)
    zf, zb = np.full((H, W), np.inf), np.full((H, W), -np.inf)
    zf2, zb2 = np.full((H, W), np.inf), np.full((H, W), -np.inf)              # the runners-up
    ff, fb = np.full((H, W), -1, np.int32), np.full((H, W), -1, np.int32)
    af, ab = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    count = np.zeros((H, W), np.int32)
    for f, face in enumerate(faces):
        st = face_setup(snapped, ok, face, H, W)
        if st is None:
            continue
        p, order, A, box = st
        cover, CX, CY = face_cover(p, box)
        if not cover.any():
            continue
        M = np.array([[0.0, 0.0, 1.0], [p[1][0] - p[0][0], p[1][1] - p[0][1], 1.0], [p[2][0] - p[0][0], p[2][1] - p[0][1], 1.0]])
        rhs = 1.0 / verts[order, 2].astype(np.float64)
        a, b, c = np.linalg.solve(M, rhs)
        z = 1.0 / (a * (CX - p[0][0]).astype(np.float64) + b * (CY - p[0][1]).astype(np.float64) + c)
        xlo, xhi, ylo, yhi = box
        sl = (slice(ylo, yhi + 1), slice(xlo, xhi + 1))
        count[sl] += cover
        # front: strictly nearer replaces the best, which becomes the runner-up; otherwise the face may still be the runner-up
        better = cover & (z < zf[sl])
        zf2[sl] = np.where(better, zf[sl], np.where(cover, np.minimum(zf2[sl], z), zf2[sl]))
        zf[sl] = np.where(better, z, zf[sl])
        ff[sl] = np.where(better, f, ff[sl])
        af[sl] = np.where(better, A, af[sl])
        farther = cover & (z > zb[sl])
        zb2[sl] = np.where(farther, zb[sl], np.where(cover, np.maximum(zb2[sl], z), zb2[sl]))
        zb[sl] = np.where(farther, z, zb[sl])
        fb[sl] = np.where(farther, f, fb[sl])
        ab[sl] = np.where(farther, A, ab[sl])
    covered = ff >= 0
    with np.errstate(invalid='ignore'):
        tie = covered & (count > 1) & ((np.abs(zf2 - zf) < TIE_REL * np.abs(zf)) | (np.abs(zb - zb2) < TIE_REL * np.abs(zb)))
    return dict(depth_front=np.where(covered, zf, 0.0).astype(np.float32), depth_back=np.where(covered, zb, 0.0).astype(np.float32), face_front=ff,
                face_back=fb, count=count, tie=tie, area_front=af, area_back=ab, z64_front=np.where(covered, zf, 0.0), z64_back=np.where(covered, zb, 0.0))


def raster(verts, mesh_id, K, meshes, H, W, z_near=0.01):
    """a batch: verts (n,Vmax,3), mesh_id (n,), K (n,3,3), meshes = [(vertex count, faces)] -> dict of stacked maps"""
    outs = [raster_image(verts[i][:meshes[m][0]], meshes[m][1], K[i], H, W, z_near) for i, m in enumerate(mesh_id)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def face_z_range(verts, faces, face_map):
    """(lo, hi) float32 maps: the smallest and largest corner depth of the face each pixel names (0 where face_map is -1)"""
    z = np.asarray(verts, np.float32)[:, 2][np.asarray(faces, np.int64)]
    f = np.where(face_map >= 0, face_map, 0)
    return np.where(face_map >= 0, z.min(1)[f], 0).astype(np.float32), np.where(face_map >= 0, z.max(1)[f], 0).astype(np.float32)


def ulp_distance(a, b):
    """distance in float32 units in the last place between two positive float32 arrays"""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def overlay(image, mean, std, K, hand, obj, meshes, ambient):
    """the compositing formula of vpho_render_overlay_u8 in float64, on given maps.  image (n,3,H,W) float32; hand / obj: None or a dict
    with depth_front, face_front (n,H,W), verts (n,Vmax,3), mesh_id (n,), colour (3), opacity; the float parameters are the float32 values
    the kernel receives.  -> (n,H,W,3) float64 BEFORE clamping and rounding, and the uint8 image."""
    image = np.asarray(image, np.float32).astype(np.float64)
    n, _, H, W = image.shape
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    mean, std, ambient = f32(mean), f32(std), float(np.float32(ambient))
    bg = (image * std[None, :, None, None] + mean[None, :, None, None]) * 255.0
    out = np.transpose(bg, (0, 2, 3, 1)).copy()
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing='ij')
    for i in range(n):
        k = np.asarray(K[i], np.float64)
        ry = (ys - k[1, 2]) / k[1, 1]
        rx = ((xs - k[0, 2]) - k[0, 1] * ry) / k[0, 0]
        hf = hand['face_front'][i] if hand is not None else np.full((H, W), -1)
        of = obj['face_front'][i] if obj is not None else np.full((H, W), -1)
        hd = hand['depth_front'][i] if hand is not None else np.zeros((H, W), np.float32)
        od = obj['depth_front'][i] if obj is not None else np.zeros((H, W), np.float32)
        use_hand = (hf >= 0) & ((of < 0) | (hd <= od))
        use_obj = ~use_hand & (of >= 0)
        for layer, use, fmap in ((hand, use_hand, hf), (obj, use_obj, of)):
            if layer is None or not use.any():
                continue
            faces = np.asarray(meshes[int(layer['mesh_id'][i])][1], np.int64)
            v = np.asarray(layer['verts'][i], np.float32).astype(np.float64)
            tri = v[faces[fmap[use]]]                                         # (P,3,3)
            a, b = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
            nx, ny, nz = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
            n2 = (nx * nx + ny * ny) + nz * nz
            dx, dy = rx[use], ry[use]
            dot = (nx * dx + ny * dy) + nz
            d2 = (dx * dx + dy * dy) + 1.0
            with np.errstate(all='ignore'):
                shade = np.where(n2 > 0, ambient + (1.0 - ambient) * (np.abs(dot) / (np.sqrt(n2) * np.sqrt(d2))), ambient)
            op, col = float(np.float32(layer['opacity'])), f32(layer['colour'])
            out[i][use] = (op * shade)[:, None] * col[None, :] + (1.0 - op) * out[i][use]
    with np.errstate(invalid='ignore'):
        u8 = np.where(out > 0, np.rint(np.minimum(out, 255.0)), 0.0).astype(np.uint8)
    return out, u8


# ------------------------------------------------------------------------------------------------------------------ scenes
def dyadic_K(f=32.0, cx=16.0, cy=12.0, skew=0.0):
    return np.array([[f, skew, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


def unproject(px, py, z, K):
    """camera-frame points whose projection is the pixel coordinate (px, py) at depth z (no skew); exact for dyadic inputs"""
    px, py, z = np.broadcast_arrays(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(z, np.float64))
    return np.stack([(px - K[0, 2]) * z / K[0, 0], (py - K[1, 2]) * z / K[1, 1], z], -1).astype(np.float32)


def quad_scene(x0=3.5, x1=11.5, y0=2.5, y1=10.5, z=2.0, K=None):
    """an axis-aligned quad at constant depth as two triangles sharing the diagonal (x0,y0)-(x1,y1), which runs through pixel centres when
    the corners lie on centres and the quad is square.  -> verts (4,3) float32, faces (2,3), K"""
    K = dyadic_K() if K is None else K
    v = unproject([x0, x1, x1, x0], [y0, y0, y1, y1], z, K)
    return v, np.array([[0, 1, 2], [0, 2, 3]]), K


def fan_scene(hub=(8.5, 8.5), z=2.0, K=None):
    """eight triangles around a hub that lies ON a pixel centre, rim corners on centres too (edges through centres), mixed windings"""
    K = dyadic_K() if K is None else K
    rim = [(12.5, 8.5), (12.5, 12.5), (8.5, 13.5), (4.5, 12.5), (3.5, 8.5), (4.5, 4.5), (8.5, 2.5), (12.5, 4.5)]
    v = unproject([hub[0]] + [r[0] for r in rim], [hub[1]] + [r[1] for r in rim], z, K)
    f = [[0, 1 + i, 1 + (i + 1) % 8] if i % 2 == 0 else [0, 1 + (i + 1) % 8, 1 + i] for i in range(8)]
    return v, np.array(f), K


def tetra_scene(K=None):
    """a tetrahedron seen from above its apex: base (faces 0) far, three side faces near.  Corner depths are powers of two.  Front ids are the
    side faces 1, 2, 3, the back id is the base face 0 wherever the tetrahedron covers a pixel."""
    K = dyadic_K() if K is None else K
    v = np.concatenate([unproject([4.0, 28.0, 16.0], [3.0, 3.0, 22.0], 4.0, K), unproject([16.0], [9.0], 2.0, K)])
    return v, np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3], [2, 0, 3]]), K


def border_scene(K=None):
    """one face partly off every border of a 24 x 32 image, one face behind z_near, one face with a NaN vertex, one ordinary face"""
    K = dyadic_K() if K is None else K
    big = unproject([-6.0, 40.0, 10.0], [-4.0, 6.0, 30.0], 2.0, K)
    behind = unproject([2.0, 10.0, 6.0], [2.0, 2.0, 9.0], [1.0, 1.0, 0.0078125], K)        # one corner at Z = 2^-7 < z_near
    nan = unproject([20.0, 30.0, 25.0], [14.0, 14.0, 22.0], 1.0, K)
    nan[1, 0] = np.nan
    plain = unproject([18.0, 30.0, 24.0], [2.0, 4.0, 11.0], 1.0, K)
    v = np.concatenate([big, behind, nan, plain])
    return v, np.arange(12).reshape(4, 3), K


def box_faces():
    """a closed box of 8 corners, 12 triangles"""
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))])


def box_verts(half=(0.05, 0.03, 0.04)):
    return np.array([[sx * half[0], sy * half[1], sz * half[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)


def pose(v, seed, centre=(0.0, 0.0, 0.6)):
    """a seeded rigid motion of a mesh, rounded to float32 as the kernel reads it"""
    r = np.random.default_rng(seed)
    q = r.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return (np.asarray(v, np.float64) @ R.T + np.asarray(centre) + r.normal(0, 0.005, 3)).astype(np.float32)


def skew_K(H, W, f=None, skew=1.75):
    f = 1.9 * max(H, W) if f is None else f
    return np.array([[f, skew, W / 2 + 0.37], [0.0, f * 1.03, H / 2 - 0.61], [0.0, 0.0, 1.0]])


def pad_verts(vs, Vmax=None):
    Vmax = max(len(v) for v in vs) if Vmax is None else Vmax
    out = np.zeros((len(vs), Vmax, 3), np.float32)
    for i, v in enumerate(vs):
        out[i, :len(v)] = v
    return out


# the generic scenes of tests/test_gpu_render.py: seeded float32 vertices, a K with skew.  The seeds are chosen so that the referee finds no
# `tie` pixel (tests/test_raster_cpu.py confirms the share stays within TIE_CAP without a GPU)
TIE_CAP = 0.001
GENERIC = {
    # name: (H, W, [(mesh, seed)] per image): mesh 0 = the 1 552-face ellipsoid (1 552 = 24 * 64 + 16: not a multiple of the kernel's chunk),
    # mesh 1 = the 12-face box
    'mixed_40x56': (40, 56, [(0, 11), (1, 12)]),
    'ellipsoid_256': (256, 256, [(0, 21)]),
    'many_images_20x24': (20, 24, [(0, 31), (1, 32), (1, 33), (0, 34), (1, 35), (0, 36)]),       # 6 images, 2 x 2 tiles of 16 x 16
}
_SCENES = {}


def generic_meshes():
    from _hand_surface_fp64 import ellipsoid
    ev, ef = ellipsoid()
    return [(len(ev), np.asarray(ef, np.int64)), (8, box_faces())], [np.asarray(ev, np.float64), box_verts()]


def generic_scene(name):
    """-> dict(verts (n,Vmax,3) float32, mesh_id, K (n,3,3), meshes, H, W, ref = the referee's maps), computed once per process"""
    if name not in _SCENES:
        H, W, images = GENERIC[name]
        meshes, rest = generic_meshes()
        verts = pad_verts([pose(rest[m], seed) for m, seed in images], max(len(r) for r in rest))
        mesh_id = [m for m, _ in images]
        K = np.stack([skew_K(H, W) for _ in images])
        _SCENES[name] = dict(verts=verts, mesh_id=mesh_id, K=K, meshes=meshes, H=H, W=W, ref=raster(verts, mesh_id, K, meshes, H, W))
    return _SCENES[name]

"""The rasteriser without a GPU: the numpy referee of tests/_raster_fp64.py against closed forms (the fill rule, shared edges, a vertex fan,
a tetrahedron, dropped faces), the tie share of the generic scenes the GPU test uses, the PNG writer, the --infer_render flag, the header
and the compiler's report of csrc/raster.hip, and that --infer_render 0 never loads vpho_amd.render."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raster_fp64 as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 32


# ---------------------------------------------------------------------------------------------------------------------- closed forms
def test_dyadic_quad_covers_the_half_open_box_at_its_depth():
    v, f, K = R.quad_scene(3.5, 11.5, 2.5, 10.5, 2.0)
    out = R.raster_image(v, f, K, H, W)
    want = np.zeros((H, W), bool)
    want[2:10, 3:11] = True                                  # centres 3.5 .. 10.5 lie in [3.5, 11.5): the left / top edges own theirs
    assert np.array_equal(out['face_front'] >= 0, want) and np.array_equal(out['count'], want.astype(np.int32))
    assert (out['depth_front'][want] == 2.0).all() and (out['depth_back'][want] == 2.0).all() and not out['depth_front'][~want].any()
    assert np.array_equal(out['face_front'], out['face_back']) and (out['face_front'][~want] == -1).all()
    # corners off the centres: [4.25, 9.75) x [3.0, 7.0) holds the centres 4.5 .. 9.5 and 3.5 .. 6.5
    v, f, K = R.quad_scene(4.25, 9.75, 3.0, 7.0, 0.5)
    out = R.raster_image(v, f, K, H, W)
    want = np.zeros((H, W), bool)
    want[3:7, 4:10] = True
    assert np.array_equal(out['count'], want.astype(np.int32)) and (out['depth_front'][want] == 0.5).all()
    # one pixel, one face pair over it
    out = R.raster_image(*R.quad_scene(-3.0, 5.0, -3.0, 5.0, 1.0, R.dyadic_K(32.0, 0.5, 0.5))[:2], R.dyadic_K(32.0, 0.5, 0.5), 1, 1)
    assert out['count'].tolist() == [[1]] and out['depth_front'][0, 0] == 1.0


@pytest.mark.parametrize('flip', [False, True])
def test_an_edge_through_pixel_centres_gives_each_centre_to_one_face(flip):
    v, f, K = R.quad_scene()
    if flip:
        f = f[:, ::-1].copy()                                # the other winding: the same coverage
    a, b = R.raster_image(v, f[:1], K, H, W)['count'], R.raster_image(v, f[1:], K, H, W)['count']
    on_diagonal = [(x - 1, x) for x in range(4, 11)]         # centre (x + 0.5, x - 0.5) lies on the diagonal from (3.5, 2.5) to (11.5, 10.5)
    assert all(a[y, x] + b[y, x] == 1 for y, x in on_diagonal)
    assert len({int(a[y, x]) for y, x in on_diagonal}) == 1  # ... and the rule gives them all to the same face
    both = R.raster_image(v, f, K, H, W)['count']
    assert np.array_equal(a + b, both) and both.max() == 1 and both.sum() == 64


def test_a_fan_around_a_pixel_centre_covers_it_once():
    v, f, K = R.fan_scene()
    out = R.raster_image(v, f, K, H, W)
    assert out['count'][8, 8] == 1 and out['count'].max() == 1 and out['count'].sum() > 60
    assert (out['depth_front'][out['count'] == 1] == 2.0).all()
    alone = sum(R.raster_image(v, f[i:i + 1], K, H, W)['count'] for i in range(len(f)))
    assert np.array_equal(alone, out['count'])               # the spokes run through centres too: every one is covered exactly once


def test_tetrahedron_front_and_back_ids():
    v, f, K = R.tetra_scene()
    out = R.raster_image(v, f, K, H, W)
    ff, fb = out['face_front'], out['face_back']
    covered = ff >= 0
    assert covered.sum() > 150 and (out['count'][covered] == 2).all()
    assert (fb[covered] == 0).all() and set(np.unique(ff[covered])) == {1, 2, 3}
    assert ff[5, 16] == 1 and ff[12, 20] == 2 and ff[12, 11] == 3 and ff[0, 0] == -1 and ff[23, 31] == -1
    assert (out['depth_back'][covered] == 4.0).all()
    d = out['depth_front'][covered]
    assert (d > 2.0).all() and (d < 4.0).all() and not out['tie'].any()


def test_dropped_faces_and_faces_off_the_borders():
    v, f, K = R.border_scene()
    out = R.raster_image(v, f, K, H, W)
    seen = set(np.unique(out['face_front'])) | set(np.unique(out['face_back']))
    assert seen == {-1, 0, 3}                                # behind z_near and NaN: dropped whole, and nothing else
    # the big face reaches all four borders
    c = out['face_back'] == 0
    assert c[0].any() and c[-1].any() and c[:, 0].any() and c[:, -1].any()
    snapped, ok = R.project_snap(v, K)
    assert ok.tolist() == [True] * 5 + [False] + [True, False, True] + [True] * 3
    # a coordinate beyond 2^30 lattice units drops the face
    far = v.copy()
    far[0, 0] = 3.0e5
    assert not R.project_snap(far, K)[1][0]
    # zero area
    line = R.unproject([2.0, 4.0, 6.0], [2.0, 4.0, 6.0], 1.0, K)
    assert R.raster_image(line, [[0, 1, 2]], K, H, W)['count'].sum() == 0


def test_the_generic_scenes_stay_within_the_tie_cap():
    """the seeds of the GPU test's generic scenes: the referee alone finds (almost) no pixel whose two best depths agree to 1e-9"""
    for name in R.GENERIC:
        ref = R.generic_scene(name)['ref']
        covered = ref['face_front'] >= 0
        share = float(ref['tie'].sum()) / max(int(covered.sum()), 1)
        whole = int(((ref['area_front'] >= R.FULL_PIXEL_AREA) & covered).sum())
        print(f'{name}: {int(covered.sum())} covered pixels, tie share {share:.5f}, {whole} with a front face of a pixel or more')
        assert covered.sum() > 100 and share <= R.TIE_CAP and whole > 0
        assert covered.reshape(covered.shape[0], -1).any(1).all()          # every image shows its mesh


def test_overlay_restatement_on_a_hand_made_case():
    v, f, K = R.quad_scene()
    maps = R.raster_image(v, f, K, H, W)
    layer = dict(depth_front=maps['depth_front'][None], face_front=maps['face_front'][None], verts=v[None], mesh_id=[0], colour=(64.0, 128.0, 192.0), opacity=1.0)
    image = np.zeros((1, 3, H, W), np.float32)
    full, u8 = R.overlay(image, (0.5, 0.25, 0.125), (1.0, 1.0, 1.0), K[None], layer, None, [(4, f)], 1.0)
    assert (u8[0, 5, 5] == [64, 128, 192]).all()                            # ambient 1: the colour itself
    assert (u8[0, 0, 0] == [128, 64, 32]).all()                             # background: 127.5 -> 128 (half to even), 63.75 -> 64, 31.875 -> 32
    # a fronto-parallel face seen along the axis has |n . d| / (|n| |d|) = 1 / |d|
    full, _ = R.overlay(image, (0, 0, 0), (1, 1, 1), K[None], dict(layer, colour=(256.0,) * 3), None, [(4, f)], 0.0)
    d = np.array([(5.5 - K[0, 2]) / K[0, 0], (5.5 - K[1, 2]) / K[1, 1], 1.0])
    assert abs(full[0, 5, 5, 0] - 256.0 / np.linalg.norm(d)) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------- PNG
def test_png_round_trip_and_chunk_crcs(tmp_path):
    from vpho_amd import render
    r = np.random.default_rng(5)
    for shape in ((7, 5, 3), (1, 1, 3), (64, 33, 3)):
        img = r.integers(0, 256, shape, dtype=np.uint8)
        p = str(tmp_path / f'{shape[0]}x{shape[1]}.png')
        render.write_png(p, img)
        assert np.array_equal(render.read_png(p), img)
        data = open(p, 'rb').read()
        assert data[:8] == b'\x89PNG\r\n\x1a\n'
        pos, kinds, idat = 8, [], b''
        while pos < len(data):
            n, kind = struct.unpack('>I', data[pos:pos + 4])[0], data[pos + 4:pos + 8]
            body = data[pos + 8:pos + 8 + n]
            crc = 0xFFFFFFFF                                                 # the CRC of the PNG specification, bit by bit
            for byte in kind + body:
                crc ^= byte
                for _ in range(8):
                    crc = (crc >> 1) ^ (0xEDB88320 if crc & 1 else 0)
            assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == crc ^ 0xFFFFFFFF, kind
            kinds.append(kind)
            idat += body if kind == b'IDAT' else b''
            if kind == b'IHDR':
                assert struct.unpack('>IIBBBBB', body) == (shape[1], shape[0], 8, 2, 0, 0, 0)
            pos += 12 + n
        assert kinds[0] == b'IHDR' and kinds[-1] == b'IEND' and pos == len(data)
        raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
        assert not raw[:, 0].any() and np.array_equal(raw[:, 1:].reshape(shape), img)        # filter type 0 on every line
    with pytest.raises(ValueError, match='uint8'):
        render.write_png(str(tmp_path / 'bad.png'), np.zeros((4, 4, 3), np.float32))
    bad = bytearray(open(p, 'rb').read())
    bad[40] ^= 1
    open(p, 'wb').write(bytes(bad))
    with pytest.raises(ValueError, match='CRC'):
        render.read_png(p)


# ---------------------------------------------------------------------------------------------------------------------- flag, header, report
def test_infer_render_flag_default_and_parsing():
    from vpho_amd.configs import args as A
    p = A._parser()
    assert p.parse_args([]).infer_render == 0 and A.Config().infer_render == 0
    assert p.parse_args(['--mode', 'infer', '--infer_render', '12']).infer_render == 12
    with pytest.raises(SystemExit):
        p.parse_args(['--infer_render', 'all'])


def test_header_declares_the_raster_entry_points_at_abi_13():
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert re.search(r'VPHO_API int vpho_mesh_raster_f32\(const vpho_mesh_table\* t, const float\* verts, int Vmax, const int\* mesh_id, const double\* K,'
                     r'[^;]*void\* workspace, void\* stream\);', hdr)
    assert re.search(r'VPHO_API int vpho_render_overlay_u8\(const float\* image,[^;]*unsigned char\* out, void\* stream\);', hdr)
    assert re.search(r'VPHO_API long long vpho_mesh_raster_bytes\(int n, int face_stride\);', hdr)
    assert 'render_fn.py' in hdr and 'base.py:472-500,632-688' in hdr
    for rule in ('rint(u * 256)', '2^30', 'Z <= z_near', 'Top-left', '(w0 / z0 + w1 / z1) + w2 / z2', 'smaller face index', 'the hand wins an exact tie'):
        assert rule in hdr, rule
    count = hdr.count('VPHO_API ') - 1
    assert count >= 124
    for doc in ('README.md', 'INTEGRATION.md'):
        assert f'{count} ' in open(os.path.join(ROOT, doc)).read(), (doc, count)
    from vpho_amd import ops
    for name in ('vpho_mesh_raster_f32', 'vpho_render_overlay_u8', 'vpho_mesh_raster_bytes'):
        assert hasattr(ops.lib, name), name
    assert ops.lib.vpho_mesh_raster_bytes(3, 10) == 3 * 10 * 56 and ops.lib.vpho_mesh_raster_bytes(-1, 1) == -1


def test_ctypes_structures_of_the_raster_mirror_the_header():
    import ctypes
    from vpho_amd import ops
    txt = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read(), flags=re.S)
    kind = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float'}
    for name, cls in (('vpho_mesh_table', ops.MeshTable), ('vpho_render_layer', ops.RenderLayer)):
        body = re.search(r'typedef\s+struct\s*\{([^{}]*)\}\s*' + name + r'\s*;', txt).group(1)
        fields = []
        for decl in body.split(';'):
            decl = ' '.join(decl.split())
            if decl:
                m = re.match(r'^(const\s+)?(\w+)\s*(.*)$', decl)
                fields += [(item.strip().lstrip('* '), 'ptr' if item.strip().startswith('*') else m.group(2)) for item in m.group(3).split(',')]
        assert fields == [(f[0], kind[f[1]]) for f in cls._fields_], (name, fields)


def test_raster_kernels_report_no_spill_and_no_scratch():
    from vpho_amd.build import build_extension
    build_extension()
    seen, name = {}, None
    for line in open(os.path.join(ROOT, 'vpho_amd', 'csrc', '_obj', 'raster.hip.usage.txt')):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (('spill', r'VGPRs Spill: (\d+)'), ('sspill', r'SGPRs Spill: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('lds', r'LDS Size \[bytes/block\]: (\d+)'), ('vgpr', r' VGPRs: (\d+)')):
            m = re.search(pat, line)
            if m and name:
                seen[name][key] = int(m.group(1))
    assert len(seen) == 3 and all(any(k in n for n in seen) for k in ('raster_setup_kernel', 'raster_tile_kernel', 'render_overlay_kernel')), sorted(seen)
    for k, v in seen.items():
        assert v['spill'] == 0 and v['sspill'] == 0 and v['scratch'] == 0 and v['vgpr'] <= 128, (k, v)
        # the tile kernel keeps 256 records of 48 bytes, their face indices and four wave counts in LDS, the other two use none
        assert v['lds'] == (256 * 48 + 256 * 4 + 4 * 4 if 'raster_tile_kernel' in k else 0), (k, v)


def test_infer_render_0_never_loads_the_render_module():
    code = ('import sys\n'
            'import vpho_amd.trainer, vpho_amd.infer, vpho_amd.ops, vpho_amd.evaluate, vpho_amd.configs.args as A\n'
            'assert A.cfg.infer_render == 0\n'
            "assert 'vpho_amd.render' not in sys.modules, 'vpho_amd.render was imported'\n"
            "print('clean')\n")
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('clean'), r.stdout[-1000:] + r.stderr[-2000:]
    src = open(os.path.join(ROOT, 'vpho_amd', 'trainer.py')).read()
    assert src.count('import render') == 1 and re.search(r'if n_render:\n\s+from \. import render as RND', src)
    for mod in ('ops.py', 'evaluate.py', 'infer.py', '__init__.py', 'model/engine.py'):
        assert not re.search(r'import render|vpho_amd\.render', open(os.path.join(ROOT, 'vpho_amd', mod)).read()), mod

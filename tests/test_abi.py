"""CPU-side checks: the C-ABI library loads and exports every symbol include/vpho_hip.h declares; host-side packing.

The ABI version and the number of entry points are spelled in this file and in no other test: a pull request that adds an entry point
changes the two numbers below, the header, common.cpp, ops.py and the two documents, and nothing else that counts."""
import ctypes
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_VERSION = 14
ENTRY_POINTS = 134


def _declared():
    src = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(vpho_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol_at_the_pinned_abi_version():
    import __graft_entry__ as g
    g.build()
    lib = ctypes.CDLL(os.path.join(ROOT, 'vpho_amd', 'libvpho_hip.so'))
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/vpho_hip.h but not exported'
    lib.vpho_abi_version.restype = ctypes.c_int
    assert lib.vpho_abi_version() == ABI_VERSION


def test_the_abi_version_is_one_number_in_the_header_the_library_and_the_binding():
    """the header's comment, common.cpp, ops.ABI_VERSION and the library that ops loaded: a stale library is refused when ops is imported
    (abi.py, which ops imports, compares the two), not found out by a missing symbol halfway through a run"""
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    m = re.search(r'vpho_abi_version\(void\);\s*/\* (\d+) \*/', hdr)
    assert m and int(m.group(1)) == ABI_VERSION
    src = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'common.cpp')).read()
    m = re.search(r'vpho_abi_version\((void)?\)\s*\{\s*return (\d+);', src)
    assert m and int(m.group(2)) == ABI_VERSION
    from vpho_amd import ops
    assert ops.ABI_VERSION == ABI_VERSION and ops.lib.vpho_abi_version() == ABI_VERSION
    binding = open(os.path.join(ROOT, 'vpho_amd', 'abi.py')).read()
    assert re.search(r'if lib\.vpho_abi_version\(\) != ABI_VERSION:\s*raise ImportError', binding)
    for doc in ('README.md', 'INTEGRATION.md'):
        assert re.search(r'version %d\b' % ABI_VERSION, open(os.path.join(ROOT, doc)).read()), doc


def test_the_entry_point_count_is_one_number_in_the_header_the_library_and_the_documents():
    import subprocess
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert hdr.count('VPHO_API ') - 1 == ENTRY_POINTS == len(_declared())          # the #define aside: one per declaration
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(ROOT, 'vpho_amd', 'libvpho_hip.so')], capture_output=True, text=True, check=True).stdout
    assert len([l for l in out.splitlines() if l.strip()]) == ENTRY_POINTS
    assert f'{ENTRY_POINTS} entry points' in open(os.path.join(ROOT, 'README.md')).read()
    assert f'exactly the {ENTRY_POINTS} `vpho_*` entry points' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_library_exports_nothing_but_the_header():
    """-fvisibility=hidden + VPHO_API + the linker version script (vpho_amd/build.py): the dynamic symbol table IS the C ABI --
    no C++ helper (vpho::fail, prof_record), kernel host stub, __hip_cuid_* or weak STL instantiation leaks out of the library"""
    import subprocess
    import __graft_entry__ as g
    g.build()
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(ROOT, 'vpho_amd', 'libvpho_hip.so')], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if l.strip())
    assert exported == _declared(), (sorted(set(exported) - set(_declared())), sorted(set(_declared()) - set(exported)))
    hdr = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    assert hdr.count('VPHO_API ') - 1 == len(exported)            # every declaration carries the export attribute (+ the #define)


def test_product_library_carries_no_ablation_or_stamp_code():
    """Switches that make a kernel produce WRONG results (timing ablations: skipped loads / barriers / stores) and the in-kernel clock
    stamps exist only as compile-time macros of diagnostic builds (scripts/kernel_ablate.sh, scripts/build_stamps.sh): the product
    library reads no such environment variable, exports no diagnostic entry point, and its build defines none of the macros
    (VPHO_CONV_DBG bits 1 / 2 / 4 and VPHO_WINO_ABL used to be one stray environment variable away)."""
    import subprocess
    import __graft_entry__ as g
    from vpho_amd import build as B
    g.build()
    lib = os.path.join(ROOT, 'vpho_amd', 'libvpho_hip.so')
    strs = subprocess.run(['strings', '-n', '6', lib], capture_output=True, text=True, check=True).stdout
    env = sorted(set(re.findall(r'VPHO_[A-Z0-9_]+', strs)))
    assert 'VPHO_WINO_ABL' not in env and not [e for e in env if 'ABL' in e or 'STAMP' in e], env
    assert 'vpho_diag_' not in strs
    macros = ('CONV_ABLATE', 'WINO_ABLATE', 'FK_ABLATE', 'VPHO_CLOCK_STAMPS')
    assert not [f for f in B.FLAGS if any(m in f for m in macros)], B.FLAGS
    src = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'conv_igemm.hip')).read()
    plan = open(os.path.join(ROOT, 'vpho_amd', 'csrc', 'conv_plan.h')).read()
    # the run-time VPHO_CONV_DBG keeps only its two bit-identical A/B orders: Geo::dbg has ONE writer, the plan, and it masks
    assert re.search(r'g\.dbg\s*=\s*sw\.dbg & \(8 \| 16\);', plan), 'VPHO_CONV_DBG must be masked to its bit-identical bits'
    assert len(re.findall(r'\bdbg\s*=[^=]', plan + src)) == 1 and 'env_int("VPHO_CONV_DBG", 0)' in plan
    assert not re.search(r'g\.dbg & (1|2|4)\b', src + plan)


def test_library_reads_the_kept_ab_switches_and_none_of_the_retired_ones():
    """The A/B switches of kernels that were measured, lost and removed must not come back silently, and the switches whose two sides
    both still run (each has a bit-identity test of live code against live code) must not be lost by accident: the environment
    variables the built library names."""
    import subprocess
    import __graft_entry__ as g
    g.build()
    lib = os.path.join(ROOT, 'vpho_amd', 'libvpho_hip.so')
    strs = subprocess.run(['strings', '-n', '6', lib], capture_output=True, text=True, check=True).stdout
    env = set(re.findall(r'VPHO_[A-Z0-9_]+', strs))
    retired = ('VPHO_PE_RING', 'VPHO_HEAD_PERS', 'VPHO_HEAD_LDS', 'VPHO_WINO8')
    assert not [e for e in retired if e in env], sorted(env)
    kept = ('VPHO_HEAD_EPI', 'VPHO_PE_ROWS', 'VPHO_HEAD_CB', 'VPHO_WINO_STAGED')
    assert not [e for e in kept if e not in env], sorted(env)


def test_state_dict_layout_matches_reference_contract(model_cpu):
    sd = model_cpu.state_dict()
    assert len([k for k in sd if k.startswith('feature_extractor.')]) == 530
    assert len([k for k in sd if k.startswith('encoder_hand.')]) == 170
    assert sd['denoiser_hand.head.head.0.weight'].shape == (32, 1408, 256)
    assert sd['denoiser_obj.head.head.2.weight'].shape == (3, 256, 3)
    assert sd['head_hm_hand.deconv_layers.0.weight'].shape == (128, 64, 4, 4)
    assert sd['cross_hand.pose_embedder.pe'].shape == (5000, 1, 512)
    assert sd['cross_obj.attn.layers.0.self_attn.in_proj_weight'].shape == (1536, 512)
    assert sd['head_physics.anchor'].shape == (8, 3)
    assert 'head_obj.point_002_master_chef_can' in sd and 'head_mano.mano_layer.th_posedirs' in sd


def test_deconv_phase_packing_is_equivalent_on_cpu():
    """pack_deconv4x4s2 (host logic) reproduces ConvTranspose2d(k4,s2,p1) with four stride-1 2x2 convolutions."""
    from vpho_amd.model.pack import pack_deconv4x4s2
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(1, 6, 5, 5, generator=g), torch.randn(6, 4, 4, 4, generator=g)
    ref = F.conv_transpose2d(x, w, None, 2, 1)
    out = torch.zeros_like(ref)
    for (py, px), (wp, pady, padx) in pack_deconv4x4s2(w).items():
        wk = wp.view(4, 2, 2, 6).permute(0, 3, 1, 2)
        xp = F.pad(x, (padx, 1 - padx, pady, 1 - pady))
        out[:, :, py::2, px::2] = F.conv2d(xp, wk)
    assert torch.allclose(out, ref, atol=1e-5)


def test_bn_folding_on_cpu(sd):
    from vpho_amd.model.pack import fold_conv_bn
    p = 'feature_extractor.layer1_h.0.0'
    w, b = fold_conv_bn(sd, p + '.conv1', p + '.bn1')
    x = torch.randn(2, 64, 5, 5)
    ref = F.batch_norm(F.conv2d(x, sd[p + '.conv1.weight']), sd[p + '.bn1.running_mean'], sd[p + '.bn1.running_var'],
                       sd[p + '.bn1.weight'], sd[p + '.bn1.bias'], False, 0.0, 1e-5)
    got = F.conv2d(x, w.view(64, 1, 1, 64).permute(0, 3, 1, 2), b)
    assert torch.allclose(got, ref, atol=1e-5)


def _header_structs():
    """{struct name: [(field name, 'ptr' | 'int' | 'float' | 'double' | 'longlong'), ...]} from include/vpho_hip.h"""
    import re
    txt = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    out = {}
    for body, name in re.findall(r'typedef\s+struct(?:\s+\w+)?\s*\{(.*?)\}\s*(\w+)\s*;', txt, flags=re.S):
        fields = []
        for decl in body.split(';'):
            decl = ' '.join(decl.split())
            if not decl:
                continue
            m = re.match(r'^(const\s+)?(unsigned\s+char|long\s+long|\w+)\s*(.*)$', decl)
            base, rest = m.group(2), m.group(3)
            for item in rest.split(','):
                item = item.strip()
                ptr = item.startswith('*') or base.endswith('*')
                fields.append((item.lstrip('* '), 'ptr' if ptr else {'int': 'int', 'float': 'float', 'double': 'double', 'long long': 'longlong'}[base]))
        out[name] = fields
    return out


def test_ctypes_structures_mirror_the_header_field_for_field():
    """A binding whose Structure is one field short makes the C side read past it (found in INTEGRATION.md's example): names, order and
    kind of every field of every struct the ABI passes by pointer, header against vpho_amd/ops.py."""
    from vpho_amd import ops
    hs = _header_structs()
    pairs = {'vpho_conv_desc': ops.ConvDesc, 'vpho_score_weights': ops.ScoreWeights, 'vpho_ode_stats': ops.OdeStats,
             'vpho_mano_tables': ops.ManoTables, 'vpho_obj_tables': ops.ObjTables, 'vpho_anchor_tables': ops.AnchorTables,
             'vpho_obj_metric_tables': ops.ObjMetricTables, 'vpho_obj_symmetry_tables': ops.ObjSymmetryTables,
             'vpho_obj_mesh_tables': ops.ObjMeshTables, 'vpho_obj_mesh_accel': ops.ObjMeshAccel, 'vpho_obj_solids': ops.ObjSolids,
             'vpho_obj_solid_columns': ops.ObjSolidColumns, 'vpho_hand_surface_table': ops.HandSurfaceTable,
             'vpho_obj_vertex_accel': ops.ObjVertexAccel, 'vpho_mesh_table': ops.MeshTable, 'vpho_render_layer': ops.RenderLayer}
    # every struct the header defines has its mirror here: a new one cannot be added without it
    assert set(pairs) == set(hs) and len(hs) == 16, sorted(set(pairs) ^ set(hs))
    kind = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_double: 'double', ctypes.c_longlong: 'longlong'}
    for name, cls in pairs.items():
        assert name in hs, name
        got = [(f[0], kind[f[1]]) for f in cls._fields_]
        assert got == hs[name], f'{name}: header {hs[name]} vs ctypes {got}'
    # the example a maintainer would copy out of INTEGRATION.md names the same fields of the sampler's weight struct
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for f, _ in hs['vpho_score_weights']:
        assert f"'{f}'" in doc, f'INTEGRATION.md example lacks vpho_score_weights.{f}'


_ELEMENTS = {'float': torch.float32, 'double': torch.float64, 'int': torch.int32, 'unsigned int': torch.int32, 'unsigned char': torch.uint8,
             'long long': torch.int64, 'void': None}
_SCALARS = {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'float': ctypes.c_float, 'double': ctypes.c_double}


def _header_prototypes(txt=None):
    """{function: (return type, [parameter])} by this file's own reading of the header; a parameter is ('scalar', C type, name) or
    ('ptr', element type, name) with the element type one of _ELEMENTS or a struct name"""
    txt = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read() if txt is None else txt
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    txt = re.sub(r'typedef\s+struct(?:\s+\w+)?\s*\{.*?\}\s*\w+\s*;', ' ', txt, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r'\b(int|long long|const char\s*\*|void)\s+(vpho_\w+)\s*\(([^)]*)\)\s*;', txt):
        params = []
        for a in args.split(','):
            a = ' '.join(a.replace('*', ' * ').split())
            if not a or a == 'void':
                continue
            *words, pname = [w for w in a.split() if w != 'const']          # the last word is the parameter's name
            if words[-1] == '*':
                params.append(('ptr', ' '.join(words[:-1]), pname))
            else:
                params.append(('scalar', ' '.join(words), pname))
        protos[name] = (' '.join(ret.replace('*', ' *').split()), params)
    return protos


def _call_sites():
    """(file, line, 'call' | 'query', entry point, number of arguments) of every `_call('vpho_x', ...)`, `abi.call(...)` and
    `abi.query(...)` in vpho_amd/, tests/ and scripts/"""
    import ast
    import glob
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, 'vpho_amd', '**', '*.py'), recursive=True) + glob.glob(os.path.join(ROOT, 'tests', '*.py'))
                       + glob.glob(os.path.join(ROOT, 'scripts', '*.py'))):
        if os.path.abspath(path) == os.path.abspath(__file__):             # miscounts on purpose, to see the refusal
            continue
        for node in ast.walk(ast.parse(open(path).read())):
            if not isinstance(node, ast.Call):
                continue
            f = node.func
            what = f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None
            if isinstance(f, ast.Attribute) and what in ('call', 'query'):
                owner = f.value.id if isinstance(f.value, ast.Name) else f.value.attr if isinstance(f.value, ast.Attribute) else None
                if owner != 'abi':
                    continue
            elif what != '_call':
                continue
            if not (node.args and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str)):
                assert os.path.basename(path) == 'abi.py', f'{path}:{node.lineno}: the entry point must be a string literal'
                continue
            assert not any(isinstance(a, ast.Starred) for a in node.args) and not node.keywords, \
                f'{path}:{node.lineno}: a starred argument list cannot be counted against the header: spell the arguments out'
            out.append((os.path.relpath(path, ROOT), node.lineno, 'query' if what == 'query' else 'call', node.args[0].value, len(node.args) - 1))
    return out


def test_every_call_site_names_a_declared_function_and_passes_the_declared_number_of_arguments():
    """The static half of the binding's check, over vpho_amd/, tests/ and scripts/: each `_call('vpho_x', ...)` / `abi.call` passes as many
    arguments as the prototype has before its trailing stream, each `abi.query` as many as the prototype has, and none hides its
    arguments behind a star -- a missing argument would otherwise only show when that line runs."""
    protos = _header_prototypes()
    assert len(protos) == ENTRY_POINTS
    sites = _call_sites()
    for path, line, how, name, n in sites:
        assert name in protos, f'{path}:{line}: {name} is called but not declared in include/vpho_hip.h'
        params = protos[name][1]
        streamed = bool(params) and params[-1] == ('ptr', 'void', 'stream')
        if how == 'call':
            assert streamed, f'{path}:{line}: {name} takes no stream: abi.query'
            assert n == len(params) - 1, f'{path}:{line}: {name} with {n} arguments, the header has {len(params) - 1} before the stream'
        else:
            assert n == len(params), f'{path}:{line}: {name} with {n} arguments, the header has {len(params)}'
    # ops.py reaches every entry point but the two abi.py calls itself and the two aliases that have no wrapper (tests/test_leaf_coverage_cpu.py)
    in_ops = {name for path, _, _, name, _ in sites if path == os.path.join('vpho_amd', 'ops.py')}
    assert in_ops == set(protos) - {'vpho_last_error', 'vpho_abi_version', 'vpho_mha_f32', 'vpho_mha_bwd_f32'}, sorted(in_ops ^ set(protos))
    assert {'vpho_mha_f32', 'vpho_mha_bwd_f32'} <= {name for path, _, _, name, _ in sites if path.startswith('tests')}
    # nothing in the binding's one user goes round abi.call / abi.query to the library
    src = open(os.path.join(ROOT, 'vpho_amd', 'ops.py')).read()
    assert re.findall(r'\blib\.(vpho_\w+)', src) in ([], ['vpho_last_error']) and 'argtypes' not in src and 'restype' not in src


def test_argtypes_and_restype_of_every_entry_point_are_the_header_s():
    """Every one of the 134 functions is typed, from the header, element types included: what abi.py set on the loaded library against
    this file's own reading of include/vpho_hip.h.  (Before abi.py four functions had argtypes and a pointer was just 'a pointer'.)"""
    from vpho_amd import abi
    protos = _header_prototypes()
    assert len(protos) == ENTRY_POINTS
    rets = {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'const char *': ctypes.c_char_p}
    structs = set(_header_structs())
    n_ptr = n_stream = 0
    for name, (ret, params) in protos.items():
        fn = getattr(abi.lib, name)
        assert fn.restype is rets[ret], f'{name}: restype {fn.restype}, header {ret}'
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), f'{name}: {fn.argtypes} vs {params}'
        for i, ((kind, what, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = f'{name} parameter {i} ({what} {pname})'
            if kind == 'scalar':
                assert at is _SCALARS[what], f'{where}: {at}'
            elif (kind, what, pname) == ('ptr', 'void', 'stream'):
                # the stream is the one pointer no caller passes: abi.call appends torch's integer handle itself
                assert at is ctypes.c_void_p and i == len(params) - 1, f'{where}: {at}'
                n_stream += 1
            elif what in structs:
                assert at is ctypes.POINTER(abi.struct(what)), f'{where}: {at}'
            else:
                assert issubclass(at, abi._Pointer) and at.element == what and at.dtype == _ELEMENTS[what], f'{where}: {at} {at.element} {at.dtype}'
                n_ptr += 1
    # every entry point launches on a stream but the version / error / profiling queries and the twelve size queries
    host_only = [n for n in protos if n in ('vpho_last_error', 'vpho_abi_version') or n.startswith('vpho_prof_') or n.endswith('_bytes')]
    assert n_stream == ENTRY_POINTS - len(host_only) == 118, (n_stream, host_only)
    assert n_ptr >= 4 * n_stream, n_ptr                      # a launch reads and writes tensors: the element types judged above are the bulk


class _Tensor:
    """what a converter looks at of a tensor"""
    def __init__(self, dtype, cuda=True, contiguous=True, address=0x7F0012345000):
        self.dtype, self.is_cuda, self._c, self._a = dtype, cuda, contiguous, address

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return self._a


def test_the_converters_refuse_what_the_static_check_used_to_judge_and_more():
    """The run-time refusals that replace the static per-argument judgement of the I / F / LL / _f32 ... wrappers (those are gone):
      * 'a tensor pointer where the header has a pointer' -> the converter of the declared ELEMENT type: a wrong dtype, a CPU tensor, a
        non-contiguous tensor and a bare int are refused (the static check knew 'ptr' only, and only for arguments built by a wrapper);
      * 'I(...) where the header has int, F(...) where it has float' -> c_int refuses a float, c_float / c_double take an int, c_int takes
        numpy integers and bool (as the wrappers did);
      * 'byref(...) is a pointer' -> POINTER(mirror) refuses byref of another struct, a data pointer refuses byref / an array of another
        element type;
      * 'as many arguments as the header has' (static, kept above) -> abi.call / abi.query count again at run time, since ctypes itself
        lets surplus arguments through."""
    import pytest
    from vpho_amd import abi
    dtypes = [torch.float32, torch.float64, torch.int32, torch.uint8, torch.int64, torch.float16, torch.bool, torch.int16]
    elements = {'float': ctypes.c_float, 'double': ctypes.c_double, 'int': ctypes.c_int, 'unsigned int': ctypes.c_uint,
                'unsigned char': ctypes.c_ubyte, 'long long': ctypes.c_longlong}
    assert set(elements) | {'void'} == set(abi._POINTERS) == set(_ELEMENTS)
    for el, ctype in elements.items():
        conv = abi._POINTERS[el]
        got = conv.from_param(_Tensor(_ELEMENTS[el]))
        assert isinstance(got, ctypes.c_void_p) and got.value == 0x7F0012345000
        assert conv.from_param(None) is None
        off = ctypes.c_void_p(0x7F0012345010)
        assert conv.from_param(off) is off
        for wrong in dtypes:
            if wrong != _ELEMENTS[el]:
                with pytest.raises(abi.VphoError, match=f'expected {_ELEMENTS[el]}, got {wrong}'.replace('.', r'\.')):
                    conv.from_param(_Tensor(wrong))
        with pytest.raises(abi.VphoError, match='GPU tensors only'):
            conv.from_param(_Tensor(_ELEMENTS[el], cuda=False))
        with pytest.raises(abi.VphoError, match='contiguous'):
            conv.from_param(_Tensor(_ELEMENTS[el], contiguous=False))
        for bare in (0x7F0012345000, 0, 1.0, 'x'):
            with pytest.raises(abi.VphoError, match='expected'):
                conv.from_param(bare)
        arr, one = (ctype * 3)(), ctype()
        assert conv.from_param(arr) is arr and conv.from_param(ctypes.byref(one))._obj is one
        other = ctypes.c_double if ctype is not ctypes.c_double else ctypes.c_float
        with pytest.raises(abi.VphoError, match='expected'):
            conv.from_param((other * 3)())
        with pytest.raises(abi.VphoError, match='expected'):
            conv.from_param(ctypes.byref(other()))
    void = abi._POINTERS['void']
    for any_dtype in dtypes:
        assert void.from_param(_Tensor(any_dtype)).value == 0x7F0012345000
    with pytest.raises(abi.VphoError, match='GPU tensors only'):
        void.from_param(_Tensor(torch.uint8, cuda=False))
    with pytest.raises(abi.VphoError, match='contiguous'):
        void.from_param(_Tensor(torch.uint8, contiguous=False))
    with pytest.raises(abi.VphoError, match='expected'):
        void.from_param(4096)
    # scalars, through a host-only function and through the types the header gives float and double parameters
    eight = abi.query('vpho_bn_workspace_bytes', 8)
    assert eight > 0 and abi.query('vpho_bn_workspace_bytes', np.int64(8)) == eight == abi.query('vpho_bn_workspace_bytes', np.int32(8))
    assert abi.query('vpho_bn_workspace_bytes', True) == abi.query('vpho_bn_workspace_bytes', 1)
    with pytest.raises(abi.VphoError, match=r'vpho_bn_workspace_bytes\(C\)'):
        abi.query('vpho_bn_workspace_bytes', 8.0)
    ode = abi.lib.vpho_ode_sample.argtypes
    assert abi.lib.vpho_score_eval.argtypes[5] is ctypes.c_float and ode[5] is ctypes.c_double
    assert ode[5].from_param(3) is not None and abi.lib.vpho_score_eval.argtypes[5].from_param(3) is not None      # an int for double / float
    with pytest.raises(TypeError):
        ode[7].from_param(50.0)                                                                                     # a float for int
    # struct pointers
    from vpho_amd import ops
    with pytest.raises(abi.VphoError, match=r'vpho_score_workspace_bytes\(w\)'):
        abi.query('vpho_score_workspace_bytes', ctypes.byref(ops.OdeStats()), 1, 1)
    with pytest.raises(TypeError):
        ode[16].from_param(ctypes.byref(ops.ScoreWeights()))
    assert ode[16].from_param(ctypes.byref(ops.OdeStats())) is not None
    # the count, with the function's name, before anything is touched (no GPU here: a launch would fail differently)
    x = _Tensor(torch.float32)
    with pytest.raises(abi.VphoError, match=r'vpho_maxpool_nhwc_f32: 8 arguments, .* 9 before the stream'):
        abi.call('vpho_maxpool_nhwc_f32', x, 1, 4, 4, 4, 2, 2, 0)
    with pytest.raises(abi.VphoError, match=r'vpho_maxpool_nhwc_f32: 10 arguments, .* 9 before the stream'):
        abi.call('vpho_maxpool_nhwc_f32', x, 1, 4, 4, 4, 2, 2, 0, x, x)
    with pytest.raises(abi.VphoError, match=r'vpho_bn_workspace_bytes: 2 arguments'):
        abi.query('vpho_bn_workspace_bytes', 8, 8)
    with pytest.raises(abi.VphoError, match=r'vpho_bn_workspace_bytes: 0 arguments'):
        abi.query('vpho_bn_workspace_bytes')


def test_the_header_parser_refuses_what_it_does_not_know():
    """abi.parse_header skips nothing silently: an unknown element type, an unknown scalar, an unknown return type, a prototype without
    VPHO_API and a stray statement each raise and name the line"""
    import pytest
    from vpho_amd import abi
    good = 'typedef struct { const float* x; int n; } vpho_t;\nVPHO_API int vpho_f(const vpho_t* t, const float* x, long long n, void* stream);\n'
    structs, protos = abi.parse_header(good)
    assert structs == {'vpho_t': [('x', ctypes.c_void_p), ('n', ctypes.c_int)]}
    assert protos['vpho_f'][1] == [('t', 'vpho_t', True), ('x', 'float', True), ('n', 'long long', False), ('stream', 'void', True)]
    for bad, line in (('VPHO_API int vpho_f(const short* x, void* stream);', 3), ('VPHO_API int vpho_f(unsigned n, void* stream);', 3),
                      ('VPHO_API int vpho_f(size_t n);', 3), ('VPHO_API float vpho_f(int n);', 3), ('int vpho_f(int n);', 3),
                      ('VPHO_API int vpho_f(const vpho_other* t);', 3), ('typedef struct { short n; } vpho_u;', 3), ('static int x = 3;', 3),
                      ('VPHO_API int vpho_f(float** x);', 3)):
        with pytest.raises(abi.VphoError, match=r'vpho_hip\.h:%d: ' % line):
            abi.parse_header(good + bad + '\n')

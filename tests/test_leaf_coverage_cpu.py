"""Keeps the leaf-test gap closed: every compute entry point of include/vpho_hip.h must be reachable from an ``ops`` wrapper that some
tests/test_gpu_*.py calls BY NAME (a direct test, not only the end-to-end fixtures).  A call counts by its receiver: ``ops.f(...)`` on the
imported module, ``v.m(...)`` on an object built from an ops class -- not any ``x.transpose(...)`` or ``tr.step(...)`` (ops_calls_in).
Static: the header is read with a regular expression and vpho_amd/ops.py and the test files with ``ast``, as tests/test_abi.py does.  No GPU."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry points with no wrapper named in a GPU test file, each with the reason it is acceptable.  The test fails on an entry that is no
# longer needed, and none of the kernels of the leaf-test issues may ever be listed here (LEAF_KERNELS, CASCADE_KERNELS,
# SPATIAL_BWD_KERNELS, MANO_FK_KERNELS below).
EXCEPTIONS = {
    'vpho_conv3x3_winograd_gate_nhwc_f32': 'gated Winograd input gradient of the training blocks: compared through the bottleneck / FPN / encoder training goldens only',
    'vpho_mha_f32': 'alias of vpho_mha_dropout_f32 without a mask (no wrapper): called through ops._call in test_gpu_attention.py, every forward form, the bits of ops.mha',
    'vpho_mha_bwd_f32': 'alias of vpho_mha_bwd_ws_f32 for short sequences (no wrapper): called through ops._call in test_gpu_attention.py, the bits of ops.mha_bwd and its S <= 64 refusal',
}

# the glue and training leaf kernels that tests/test_gpu_leaf_forward.py / test_gpu_leaf_train.py cover one by one
LEAF_KERNELS = {
    'vpho_nchw_to_nhwc_f32', 'vpho_nhwc_to_nchw_f32', 'vpho_maxpool_nhwc_f32', 'vpho_align_heatmap_nhwc_f32', 'vpho_nerf_embed_f32',
    'vpho_cross_tokens_f32', 'vpho_add_layernorm_f32', 'vpho_force_local_f32', 'vpho_append_betas_f32', 'vpho_dsm_prepare_f32',
    'vpho_plinear2_fwd_f32', 'vpho_plinear2_bwd_f32', 'vpho_dsm_loss_f32', 'vpho_mse_loss_f32', 'vpho_relu_bwd_f32', 'vpho_sum_repeats_f32',
    'vpho_transpose_f32', 'vpho_im2col_t_f32', 'vpho_add_lrelu_f32', 'vpho_adamw_f32', 'vpho_adamw_multi_f32', 'vpho_cross_tokens_bwd_f32',
    'vpho_layernorm_bwd_f32', 'vpho_physics_loss_f32', 'vpho_resize_bilinear_nhwc_f32', 'vpho_resize_bilinear_rows_nhwc_f32',
    'vpho_lrelu_bwd_f32'}
LEAF_WRAPPERS = {
    'nchw_to_nhwc', 'nhwc_to_nchw', 'maxpool_nhwc', 'align_heatmap_nhwc', 'nerf_embed', 'cross_tokens', 'add_layernorm', 'force_local',
    'append_betas', 'dsm_prepare', 'plinear2_fwd', 'plinear2_bwd', 'dsm_loss', 'mse_loss', 'relu_bwd', 'sum_repeats', 'transpose', 'im2col_t',
    'add_lrelu', 'adamw_', 'AdamWList', 'AdamWList.step', 'cross_tokens_bwd', 'layernorm_bwd', 'physics_loss', 'resize_bilinear_nhwc', 'lrelu_bwd'}

# the aggregation-cascade kernels that tests/test_gpu_cascade_leaves.py covers one by one
CASCADE_KERNELS = {
    'vpho_hand_candidates_f32', 'vpho_hand_heat_f32', 'vpho_topk_weights_f32', 'vpho_obj_heat_score', 'vpho_obj_cross_candidates',
    'vpho_obj_physics_score', 'vpho_obj_verts_f32', 'vpho_force_anchor_f32', 'vpho_hand_phys_candidates_f32', 'vpho_hand_pt2d_score_f32',
    'vpho_obj_pt2d_score', 'vpho_hand_pose_fuse_f32', 'vpho_hand_joint_gather_mean_f32', 'vpho_obj_fuse_f64', 'vpho_hand_phys_score_f32',
    'vpho_hand_phys_fuse_f32'}
CASCADE_WRAPPERS = {'Aggregation.' + m for m in (
    'hand_candidates', 'hand_heat', 'topk_weights', 'obj_heat_score', 'obj_cross', 'obj_physics_score', 'obj_verts', 'force_anchor',
    'hand_phys_candidates', 'hand_pt2d_score', 'obj_pt2d_score', 'hand_pose_fuse', 'hand_joint_gather_mean', 'obj_fuse', 'hand_phys_score',
    'hand_phys_fuse')}
# of these, the three that other GPU test files also call by name (weakly: equality with the engine, an error message, finiteness)
CASCADE_CALLED_ELSEWHERE = {'vpho_obj_fuse_f64', 'vpho_hand_phys_score_f32', 'vpho_hand_phys_fuse_f32'}

# the spatial backward entry points whose every launch form tests/test_gpu_spatial_bwd.py covers (maxpool_bwd reaches both pool entries:
# the workspace form by default, the one-pass form with one_pass=True)
SPATIAL_BWD_KERNELS = {'vpho_maxpool_bwd_nhwc_f32', 'vpho_maxpool_bwd_ws_nhwc_f32', 'vpho_resize_bilinear_bwd_nhwc_f32',
                       'vpho_roi_align_bwd_nhwc_f32', 'vpho_align_heatmap_bwd_nhwc_f32'}
SPATIAL_BWD_WRAPPERS = {'maxpool_bwd', 'resize_bilinear_bwd', 'roi_align_bwd', 'align_heatmap_bwd'}

# the MANO shape blend and forward kinematics, whose every launch form tests/test_gpu_mano_fk.py covers
MANO_FK_KERNELS = {'vpho_mano_shape_f32', 'vpho_mano_fk_f32'}
MANO_FK_WRAPPERS = {'Mano.shape', 'Mano.fk'}


def _declared():
    src = open(os.path.join(ROOT, 'include', 'vpho_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(vpho_[a-z0-9_]+)\s*\(', src)))


def _is_compute(name):
    """everything that launches work; not the ABI / error / profiling queries nor the size queries"""
    return not (name in ('vpho_abi_version', 'vpho_last_error') or name.endswith('_bytes') or name.startswith('vpho_prof_'))


def _entry_points_of(node):
    """vpho_* names a function body reaches directly: _call('vpho_x', ...) and lib.vpho_x"""
    out = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == '_call' and n.args and isinstance(n.args[0], ast.Constant):
            out.add(n.args[0].value)
        if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == 'lib' and n.attr.startswith('vpho_'):
            out.add(n.attr)
    return out


def _ops_calls(fn, cls=None):
    """what a function body of vpho_amd/ops.py calls in its own module: f(...) -> 'f' (a wrapper or a class), self.m(...) -> 'Class.m'.
    Attribute calls on anything else (tensor methods such as x.transpose(...)) are NOT calls of a wrapper."""
    out = set()
    for n in ast.walk(fn):
        if isinstance(n, ast.Call):
            if isinstance(n.func, ast.Name):
                out.add(n.func.id)
            elif cls and isinstance(n.func, ast.Attribute) and isinstance(n.func.value, ast.Name) and n.func.value.id == 'self':
                out.add(f'{cls}.{n.func.attr}')
    return out


_CTOR = ('__init__', '__call__', '__enter__', '__exit__')


def _ops_tree():
    return ast.parse(open(os.path.join(ROOT, 'vpho_amd', 'ops.py')).read())


def ops_classes():
    return {n.name for n in _ops_tree().body if isinstance(n, ast.ClassDef)}


def wrappers():
    """{wrapper: set of entry points it reaches}.  A function is known by its name, a method as 'Class.method', __init__ / __call__ by
    the class name; calls of one wrapper from another are followed"""
    direct, calls = {}, {}

    def add(name, fn, cls=None):
        direct.setdefault(name, set()).update(_entry_points_of(fn))
        calls.setdefault(name, set()).update(_ops_calls(fn, cls))

    for node in _ops_tree().body:
        if isinstance(node, ast.FunctionDef):
            add(node.name, node)
        elif isinstance(node, ast.ClassDef):
            for m in node.body:
                if isinstance(m, ast.FunctionDef):
                    add(node.name if m.name in _CTOR else f'{node.name}.{m.name}', m, node.name)
    reach = {k: set(v) for k, v in direct.items()}
    changed = True
    while changed:
        changed = False
        for k in reach:
            for c in calls[k]:
                if c in reach and c != k and not reach[c] <= reach[k]:
                    reach[k] |= reach[c]
                    changed = True
    reach = {k: {e for e in v if _is_compute(e)} for k, v in reach.items()}
    return {k: v for k, v in reach.items() if v and not k.rpartition('.')[2].startswith('_')}


def ops_factories():
    """ops functions that hand back an object of an ops class (``return Class(...)``), e.g. roi_windows -> RoiWindows"""
    classes, out = ops_classes(), {}
    for f in _ops_tree().body:
        if isinstance(f, ast.FunctionDef):
            for r in ast.walk(f):
                if isinstance(r, ast.Return) and isinstance(r.value, ast.Call) and isinstance(r.value.func, ast.Name) and r.value.func.id in classes:
                    out[f.name] = r.value.func.id
    return out


def package_attributes():
    """attributes in which the package keeps an object of an ops class (``self.agg = ops.Aggregation(...)`` in vpho_amd/model/engine.py):
    {attribute: Class}, so that ``eng.agg.obj_fuse(...)`` in a test is a call of Aggregation.obj_fuse"""
    classes, out = ops_classes(), {}
    for path in glob.glob(os.path.join(ROOT, 'vpho_amd', '**', '*.py'), recursive=True):
        for n in ast.walk(ast.parse(open(path).read())):
            if (isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Attribute) and isinstance(n.value, ast.Call)
                    and isinstance(n.value.func, ast.Attribute) and isinstance(n.value.func.value, ast.Name) and n.value.func.value.id == 'ops'
                    and n.value.func.attr in classes):
                out[n.targets[0].attr] = n.value.func.attr
    return out


def _returned_name(fn):
    return {n.value.id for n in ast.walk(fn) if isinstance(n, ast.Return) and isinstance(n.value, ast.Name)}


def ops_calls_in(src, classes, factories=None, attrs=None):
    """the ops wrappers one test file calls, judged by the RECEIVER:
      * ``A.f(...)`` counts as 'f' only if A is the imported module (``from vpho_amd import ops [as A]``, ``import vpho_amd.ops as A``, or
        ``A = helper()`` where the file's own helper returns that import);
      * ``f(...)`` counts only if f came from ``from vpho_amd.ops import f``: names the test file defines itself never count;
      * ``v.m(...)`` counts as 'Class.m' only if v was bound to ``A.Class(...)`` in this file (an assignment, or a fixture function of that
        name that returns one) or to an ops function that returns one (``factories``); ``x.attr.m(...)`` only if the package keeps an
        object of an ops class in ``attr`` (``attrs``).  Names are tracked per file, without regard to scope.
    So ``k.transpose(-1, -2)`` on a tensor or ``tr.step(...)`` on a trainer are not calls of ops.transpose / AdamWList.step."""
    tree = ast.parse(src)
    factories, attrs = factories or {}, attrs or {}
    mod, direct = set(), {}
    for n in ast.walk(tree):
        if isinstance(n, ast.ImportFrom) and n.module == 'vpho_amd':
            mod |= {a.asname or a.name for a in n.names if a.name == 'ops'}
        elif isinstance(n, ast.ImportFrom) and n.module == 'vpho_amd.ops':
            direct.update({a.asname or a.name: a.name for a in n.names})
        elif isinstance(n, ast.Import):
            mod |= {a.asname for a in n.names if a.name == 'vpho_amd.ops' and a.asname}
    helpers = {f.name for f in ast.walk(tree) if isinstance(f, ast.FunctionDef) and _returned_name(f) & mod}

    def is_mod(e):
        return isinstance(e, ast.Name) and e.id in mod

    def ctor_class(e):
        """e is ``A.Class(...)`` or a name already bound to one -> Class"""
        if isinstance(e, ast.Call) and isinstance(e.func, ast.Attribute) and is_mod(e.func.value):
            return e.func.attr if e.func.attr in classes else factories.get(e.func.attr)
        if isinstance(e, ast.Call) and isinstance(e.func, ast.Name) and direct.get(e.func.id) in classes:
            return direct[e.func.id]
        return inst.get(e.id) if isinstance(e, ast.Name) else None

    inst = {}
    for _ in range(3):                                                 # module aliases through helpers, then instances, then fixtures
        for n in ast.walk(tree):
            if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
                t, v = n.targets[0].id, n.value
                if is_mod(v) or (isinstance(v, ast.Call) and isinstance(v.func, ast.Name) and v.func.id in helpers):
                    mod.add(t)
                elif ctor_class(v):
                    inst[t] = ctor_class(v)
            elif isinstance(n, ast.FunctionDef):
                for r in ast.walk(n):
                    if isinstance(r, ast.Return) and r.value is not None and ctor_class(r.value):
                        inst[n.name] = ctor_class(r.value)
    out = set()
    for n in ast.walk(tree):
        if not isinstance(n, ast.Call):
            continue
        f = n.func
        if isinstance(f, ast.Name) and f.id in direct:
            out.add(direct[f.id])
        elif isinstance(f, ast.Attribute) and is_mod(f.value):
            out.add(f.attr)
        elif isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id in inst:
            out.add(f'{inst[f.value.id]}.{f.attr}')
        elif isinstance(f, ast.Attribute) and isinstance(f.value, ast.Attribute) and f.value.attr in attrs:
            out.add(f'{attrs[f.value.attr]}.{f.attr}')
    return out


def _gpu_test_files():
    return sorted(glob.glob(os.path.join(ROOT, 'tests', 'test_gpu_*.py')))


def names_called_in_gpu_tests(skip=()):
    classes, factories, attrs, out = ops_classes(), ops_factories(), package_attributes(), set()
    for path in _gpu_test_files():
        if os.path.basename(path) not in skip:
            out |= ops_calls_in(open(path).read(), classes, factories, attrs)
    return out


def uncovered(skip=()):
    called = names_called_in_gpu_tests(skip)
    W = wrappers()
    by_entry = {}
    for w, eps in W.items():
        for e in eps:
            by_entry.setdefault(e, set()).add(w)
    missing = {}
    for e in _declared():
        if _is_compute(e) and not (by_entry.get(e, set()) & called):
            missing[e] = sorted(by_entry.get(e, set()))
    return missing


def test_every_compute_entry_point_has_a_wrapper_called_by_name_in_a_gpu_test():
    missing = uncovered()
    new = {e: w for e, w in missing.items() if e not in EXCEPTIONS}
    assert not new, ('compute entry points no tests/test_gpu_*.py reaches through a wrapper it calls by name (entry point: its wrappers) -- '
                     f'add a direct test, or an EXCEPTIONS entry with a reason: {new}')
    stale = sorted(set(EXCEPTIONS) - set(missing))
    assert not stale, f'EXCEPTIONS entries that are no longer needed (the entry point is covered, or gone): {stale}'
    assert all(isinstance(r, str) and r.strip() and '\n' not in r for r in EXCEPTIONS.values())


def test_the_leaf_kernels_are_never_an_exception_and_each_wrapper_is_called_directly():
    assert not (set(EXCEPTIONS) & LEAF_KERNELS)
    declared = set(_declared())
    assert LEAF_KERNELS <= declared, sorted(LEAF_KERNELS - declared)
    W = wrappers()
    assert LEAF_WRAPPERS - {'AdamWList'} <= set(W), sorted(LEAF_WRAPPERS - set(W))                        # the constructor launches nothing
    reached = set().union(*(W.get(w, set()) for w in LEAF_WRAPPERS))
    assert LEAF_KERNELS <= reached, sorted(LEAF_KERNELS - reached)
    classes, leaf_calls = ops_classes(), set()
    for f in ('test_gpu_leaf_forward.py', 'test_gpu_leaf_train.py'):
        leaf_calls |= ops_calls_in(open(os.path.join(ROOT, 'tests', f)).read(), classes, ops_factories(), package_attributes())
    assert LEAF_WRAPPERS <= leaf_calls, sorted(LEAF_WRAPPERS - leaf_calls)


def test_without_the_leaf_files_the_gap_of_the_issue_is_back():
    """the other GPU test files do not cover the leaf kernels by accident (a tensor's .transpose(), a trainer's .step()): with the two
    leaf files left out, exactly the kernels that had no direct call come back as uncovered.  resize_bilinear (both forms) and lrelu_bwd
    are called elsewhere as helpers of other comparisons.  (tests/test_gpu_binding.py calls maxpool_nhwc and nhwc_to_nchw directly, on
    purpose, to see the typed binding refuse their arguments: it is left out with the leaf files.)"""
    back = set(uncovered(skip=('test_gpu_leaf_forward.py', 'test_gpu_leaf_train.py', 'test_gpu_binding.py'))) - set(EXCEPTIONS)
    assert back == LEAF_KERNELS - {'vpho_resize_bilinear_nhwc_f32', 'vpho_resize_bilinear_rows_nhwc_f32', 'vpho_lrelu_bwd_f32'}, sorted(back ^ LEAF_KERNELS)


def test_the_cascade_kernels_are_never_an_exception_and_each_wrapper_is_called_directly():
    assert not (set(EXCEPTIONS) & CASCADE_KERNELS) and len(CASCADE_KERNELS) == len(CASCADE_WRAPPERS) == 16
    declared = set(_declared())
    assert CASCADE_KERNELS <= declared, sorted(CASCADE_KERNELS - declared)
    W = wrappers()
    assert CASCADE_WRAPPERS <= set(W), sorted(CASCADE_WRAPPERS - set(W))
    assert all(len(W[w]) == 1 for w in CASCADE_WRAPPERS)                                                # one wrapper, one entry point
    reached = set().union(*(W[w] for w in CASCADE_WRAPPERS))
    assert reached == CASCADE_KERNELS, sorted(reached ^ CASCADE_KERNELS)
    src = open(os.path.join(ROOT, 'tests', 'test_gpu_cascade_leaves.py')).read()
    calls = ops_calls_in(src, ops_classes(), ops_factories(), package_attributes())
    assert CASCADE_WRAPPERS <= calls, sorted(CASCADE_WRAPPERS - calls)


def test_without_the_cascade_file_the_gap_of_the_issue_is_back():
    """the other GPU test files reach the cascade stages through the engine only: with tests/test_gpu_cascade_leaves.py left out, exactly
    the thirteen kernels that had no direct call come back as uncovered (the other three are called by name elsewhere)"""
    back = set(uncovered(skip=('test_gpu_cascade_leaves.py',))) - set(EXCEPTIONS)
    assert back == CASCADE_KERNELS - CASCADE_CALLED_ELSEWHERE, sorted(back ^ (CASCADE_KERNELS - CASCADE_CALLED_ELSEWHERE))


def test_the_spatial_backward_kernels_are_never_an_exception_and_each_wrapper_is_called_directly():
    assert not (set(EXCEPTIONS) & SPATIAL_BWD_KERNELS)
    declared = set(_declared())
    assert SPATIAL_BWD_KERNELS <= declared, sorted(SPATIAL_BWD_KERNELS - declared)
    W = wrappers()
    assert SPATIAL_BWD_WRAPPERS <= set(W), sorted(SPATIAL_BWD_WRAPPERS - set(W))
    assert W['maxpool_bwd'] == {'vpho_maxpool_bwd_nhwc_f32', 'vpho_maxpool_bwd_ws_nhwc_f32'}
    reached = set().union(*(W[w] for w in SPATIAL_BWD_WRAPPERS))
    assert reached == SPATIAL_BWD_KERNELS, sorted(reached ^ SPATIAL_BWD_KERNELS)
    src = open(os.path.join(ROOT, 'tests', 'test_gpu_spatial_bwd.py')).read()
    calls = ops_calls_in(src, ops_classes(), ops_factories(), package_attributes())
    assert SPATIAL_BWD_WRAPPERS <= calls, sorted(SPATIAL_BWD_WRAPPERS - calls)
    tree = ast.parse(src)                                            # and the one-pass pool form is asked for by its keyword there
    assert any(isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'maxpool_bwd'
               and any(k.arg == 'one_pass' for k in n.keywords) for n in ast.walk(tree))


def test_the_mano_fk_kernels_are_never_an_exception_and_each_wrapper_is_called_directly():
    assert not (set(EXCEPTIONS) & MANO_FK_KERNELS)
    declared = set(_declared())
    assert MANO_FK_KERNELS <= declared, sorted(MANO_FK_KERNELS - declared)
    W = wrappers()
    assert MANO_FK_WRAPPERS <= set(W), sorted(MANO_FK_WRAPPERS - set(W))
    assert W['Mano.shape'] == {'vpho_mano_shape_f32'} and W['Mano.fk'] == {'vpho_mano_fk_f32'}
    src = open(os.path.join(ROOT, 'tests', 'test_gpu_mano_fk.py')).read()
    calls = ops_calls_in(src, ops_classes(), ops_factories(), package_attributes())
    assert MANO_FK_WRAPPERS <= calls, sorted(MANO_FK_WRAPPERS - calls)
    tree = ast.parse(src)                                            # and the joints-only launch and the HO3D flags are asked for there
    fk = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'fk']
    assert any(any(k.arg == 'ho3d' for k in n.keywords) for n in fk)
    assert any(len(n.args) >= 4 and isinstance(n.args[3], ast.Constant) and n.args[3].value is False for n in fk)


_SAMPLE = '''
import torch
from vpho_amd import ops as O
from vpho_amd.ops import nerf_embed as ne

def _ops():
    from vpho_amd import ops
    return ops

def transpose(x):                       # the file's own function
    return x.t()

@pytest.fixture
def hands(assets):
    return O.Mano(assets, 'cuda')

def test_a(hands, eng):
    ops = _ops()
    k = torch.zeros(2, 3)
    k.transpose(-1, -2)                 # a tensor method
    transpose(k)
    tr = make_trainer()
    tr.step(1)                          # not an ops object
    lst = ops.AdamWList([])
    lst.step(1)
    ops.maxpool_nhwc(k, 2, 2, 0)
    ne(k)
    hands.fk(k, k, 1)
    win = O.roi_windows(k, None, 1, 2, 2, 0.25)
    win.tiles()
    eng.agg.obj_fuse(k, k, None)
    eng.other.hand_heat(k)
'''


def test_the_scan_sees_what_it_should():
    """the parser is not vacuous, and a call counts by its receiver: the header's entry points, methods as Class.method, wrapper-to-wrapper
    calls, and -- on a sample file -- exactly the calls made on the ops module, on objects of its classes and on imported names"""
    W = wrappers()
    assert len([e for e in _declared() if _is_compute(e)]) >= 80
    assert W['AdamWList.step'] == {'vpho_adamw_multi_f32'} and W['nerf_embed'] == {'vpho_nerf_embed_f32'} and 'step' not in W
    assert W['transpose'] == {'vpho_transpose_f32'}
    assert W['linear_into'] == W['conv2d_nhwc'] and 'vpho_conv2d_nhwc_f32' in W['conv2d_nhwc']           # linear_into -> conv2d_nhwc, followed
    assert not _is_compute('vpho_bn_workspace_bytes') and _is_compute('vpho_colsum_f32')
    assert ops_factories()['roi_windows'] == 'RoiWindows' and package_attributes()['agg'] == 'Aggregation'
    got = ops_calls_in(_SAMPLE, ops_classes(), ops_factories(), package_attributes())
    assert got == {'AdamWList', 'AdamWList.step', 'maxpool_nhwc', 'nerf_embed', 'Mano', 'Mano.fk', 'roi_windows', 'RoiWindows.tiles',
                   'Aggregation.obj_fuse'}, sorted(got)

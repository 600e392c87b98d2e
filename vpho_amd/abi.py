"""The one typed binding of ``include/vpho_hip.h``: the header is parsed once at import and every struct mirror, ``restype`` and
``argtypes`` of ``libvpho_hip.so`` comes from it.  No other module spells a C type of the library.  There is NO fallback: importing this
module without the built extension raises.

``call(name, *args)`` passes plain values (tensors, ints, floats, ``None``, ``byref`` of a mirror) + the current HIP stream and raises
``VphoError`` on a non-zero return; ``query`` serves the host-only functions (no stream: the ``*_bytes`` sizes, the profiler).
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'vpho_hip.h')
LIB_PATH = os.environ.get('VPHO_HIP_LIB') or os.path.join(_HERE, 'libvpho_hip.so')   # override: A/B kernel builds
ABI_VERSION = 14                        # include/vpho_hip.h; a stale library must not be found out by a missing symbol halfway through a run


class VphoError(RuntimeError):
    pass


SCALARS = {'int': C.c_int, 'long long': C.c_longlong, 'float': C.c_float, 'double': C.c_double}
RETURNS = {'int': C.c_int, 'long long': C.c_longlong, 'const char*': C.c_char_p}
# element type of a data pointer: the tensor dtype it takes (None: any) and the ctypes type of a host array / byref it takes
ELEMENTS = {'float': (torch.float32, C.c_float), 'double': (torch.float64, C.c_double), 'int': (torch.int32, C.c_int),
            'unsigned int': (torch.int32, C.c_uint),         # the two words of a Philox key travel in an int32 tensor
            'unsigned char': (torch.uint8, C.c_ubyte), 'long long': (torch.int64, C.c_longlong), 'void': (None, None)}
_BYREF = type(C.byref(C.c_int()))


class _Pointer:
    """argtypes entry of a data pointer: one subclass per element type (``_POINTERS``)"""
    element, dtype, ctype = 'void', None, None

    @classmethod
    def from_param(cls, v):
        if v is None:
            return None
        try:                                                 # a tensor, nearly always
            if not v.is_cuda:
                raise VphoError('vpho_amd ops take GPU tensors only (no CPU path)')
        except AttributeError:
            pass
        else:
            if v.dtype != cls.dtype and cls.dtype is not None:
                raise VphoError(f'expected {cls.dtype}, got {v.dtype}')
            if not v.is_contiguous():
                raise VphoError('expected a contiguous tensor')
            return C.c_void_p(v.data_ptr())
        if isinstance(v, C.c_void_p):                        # an address with an offset, which its maker vouches for (``at``)
            return v
        host = v._obj if isinstance(v, _BYREF) else v
        if isinstance(v, (_BYREF, C.Array)) and (cls.ctype is None or isinstance(host, cls.ctype) or getattr(host, '_type_', None) is cls.ctype):
            return v
        raise VphoError(f'expected a {cls.element}* (tensor, None, c_void_p, ctypes array or byref), got {type(v).__name__}'
                        + (': a bare int is never taken for a pointer' if isinstance(v, int) else ''))


_POINTERS = {k: type('_' + k.replace(' ', '_') + '_p', (_Pointer,), dict(element=k, dtype=d, ctype=c)) for k, (d, c) in ELEMENTS.items()}
_OF_DTYPE = {p.dtype: p for p in _POINTERS.values() if p.element != 'unsigned int'}


def addr(t, dtype=None):
    """device address of a contiguous GPU tensor of the given dtype (None: any), None for None: the converter's checks for what travels
    as an integer -- descriptor fields and table records"""
    p = _OF_DTYPE[dtype].from_param(t)
    return None if p is None else p.value


def at(t, dtype, offset=0):
    """a pointer argument with the converter's checks for ``dtype`` (where the header says ``void*``), ``offset`` elements into the tensor"""
    p = _OF_DTYPE[dtype].from_param(t)
    return C.c_void_p(p.value + offset * t.element_size()) if offset else p


_TYPE = r'(?:const\s+)?(unsigned\s+int|unsigned\s+char|long\s+long|\w+)'


def parse_header(text):
    """-> ({struct: [(field, ctypes type)]}, {function: (restype, [(parameter, element | scalar | struct, is_pointer)])}); anything that is
    neither a struct typedef, a VPHO_API prototype, a preprocessor line nor the extern "C" braces raises, naming the line"""
    text = re.sub(r'/\*.*?\*/', lambda m: '\n' * m.group().count('\n'), text, flags=re.S)
    structs, protos = {}, {}

    def line(pos):
        return text.count('\n', 0, pos) + 1

    def declarators(decl, pos, known):
        m = re.match(r'^%s\s*(.*)$' % _TYPE, decl, flags=re.S)
        if not m:
            raise VphoError(f'{HEADER}:{line(pos)}: cannot parse "{decl}"')
        base = ' '.join(m.group(1).split())
        for item in m.group(2).split(','):
            d = re.match(r'^\s*(\*?)\s*(\w+)\s*$', item)
            ok = d and (base in ELEMENTS or base in known if d.group(1) else base in SCALARS)
            if not ok:
                raise VphoError(f'{HEADER}:{line(pos)}: unknown type in "{" ".join(decl.split())}"')
            yield d.group(2), base, bool(d.group(1))

    def struct(m):
        fields = []
        for d in re.finditer(r'[^;]+', m.group(1)):
            if d.group().strip():
                fields += [(n, C.c_void_p if p else SCALARS[b]) for n, b, p in declarators(d.group().strip(), m.start(1) + d.start(), ())]
        structs[m.group(2)] = fields
        return '\n' * m.group().count('\n')

    def proto(m):
        ret = re.sub(r'\s*\*', '*', ' '.join(m.group(1).split()))
        if ret not in RETURNS:
            raise VphoError(f'{HEADER}:{line(m.start())}: unknown return type "{ret}" of {m.group(2)}')
        params = [] if m.group(3).strip() == 'void' else [next(declarators(p.strip(), m.start(3), structs)) for p in m.group(3).split(',')]
        protos[m.group(2)] = (RETURNS[ret], params)
        return '\n' * m.group().count('\n')

    text = re.sub(r'typedef\s+struct(?:\s+\w+)?\s*\{(.*?)\}\s*(\w+)\s*;', struct, text, flags=re.S)
    text = re.sub(r'VPHO_API\s+([\w\s]+?\*?)\s*(vpho_\w+)\s*\(([^()]*)\)\s*;', proto, text)
    rest = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|^\}', '', text, flags=re.M)
    m = re.search(r'\S', rest)
    if m:
        n = rest.count('\n', 0, m.start())
        raise VphoError(f'{HEADER}:{n + 1}: not a struct, a VPHO_API prototype or a preprocessor line: "{rest.splitlines()[n].strip()}"')
    return structs, protos


STRUCTS, PROTOTYPES = parse_header(open(HEADER).read())
_MIRRORS = {name: type(name, (C.Structure,), {'_fields_': fields}) for name, fields in STRUCTS.items()}


def struct(name):
    """the ctypes.Structure mirror of a struct of the header"""
    return _MIRRORS[name]


if not os.path.exists(LIB_PATH):
    raise ImportError(f'{LIB_PATH} is missing: build the HIP extension first (python -m vpho_amd.build or '
                      f'__graft_entry__.build()); vpho_amd has no CPU fallback')
lib = C.CDLL(LIB_PATH)
_FN = {}                                # name -> (typed function, number of parameters)
for _name, (_ret, _params) in PROTOTYPES.items():
    _f = getattr(lib, _name)
    _f.restype = _ret
    _f.argtypes = [(C.POINTER(_MIRRORS[b]) if b in _MIRRORS else _POINTERS[b]) if p else SCALARS[b] for _, b, p in _params]
    if _params and _params[-1] == ('stream', 'void', True):
        _f.argtypes = _f.argtypes[:-1] + [C.c_void_p]         # the stream is a handle ``call`` itself appends, as an integer
    _FN[_name] = (_f, len(_params))
if lib.vpho_abi_version() != ABI_VERSION:
    raise ImportError(f'{LIB_PATH} implements ABI version {lib.vpho_abi_version()}, this binding expects {ABI_VERSION}: rebuild the '
                      f'extension (python -m vpho_amd.build --force)')


def _refused(name, fn, args, e):
    """ctypes' ArgumentError as a VphoError that names the parameter: ask the converters again, one by one"""
    for (pname, _, _), t, a in zip(PROTOTYPES[name][1], fn.argtypes, args):
        try:
            t.from_param(a)
        except Exception as why:
            return VphoError(f'{name}({pname}): {why}')
    return VphoError(f'{name}: {e}')


def check(rc):
    if rc != 0:
        raise VphoError(lib.vpho_last_error().decode())


def query(name, *args):
    """a host-only function (no stream): returns its value"""
    fn, n = _FN[name]
    if len(args) != n:
        raise VphoError(f'{name}: {len(args)} arguments, include/vpho_hip.h declares {n}')
    try:
        return fn(*args)
    except C.ArgumentError as e:
        raise _refused(name, fn, args, e) from None


def call(name, *args):
    """a launching function: the arguments before the stream; the current stream is appended, a non-zero return raises"""
    fn, n = _FN[name]
    if len(args) + 1 != n:
        raise VphoError(f'{name}: {len(args)} arguments, include/vpho_hip.h declares {n - 1} before the stream')
    try:
        rc = fn(*args, torch.cuda.current_stream().cuda_stream)
    except C.ArgumentError as e:
        raise _refused(name, fn, args, e) from None
    check(rc)

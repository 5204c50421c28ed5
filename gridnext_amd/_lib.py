"""ctypes binding of libgridnext_hip.so, derived from include/gridnext_hip.h - the one statement of the C ABI.

Nothing about an entry point is restated here: SIGNATURES, PARAMS, CONSTANTS and struct() are parsed out of the header when this
module is first imported, so an entry point exists for Python as soon as the header declares it.  A declaration this parser
cannot type raises and names itself - nothing is guessed, and there is no fallback table.

There is deliberately NO fallback for the kernels either: if the shared library is missing, or a tensor is not on a HIP
device, the call raises.  The product path never computes on the CPU.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GNX_LIB') or os.path.join(_HERE, 'libgridnext_hip.so')   # GNX_LIB: debug builds only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'gridnext_hip.h')

_BY_VALUE = {'int': ctypes.c_int, 'long': ctypes.c_long, 'long long': ctypes.c_longlong, 'float': ctypes.c_float,
             'double': ctypes.c_double, 'size_t': ctypes.c_size_t}


class HipExtensionMissing(RuntimeError):
    pass


def _ctype(ctype, where):
    """The ctypes type of a C type as the header writes it; pointers and the stream handle travel as addresses."""
    if '*' in ctype or ctype == 'gnx_stream_t':
        return ctypes.c_void_p
    if ctype not in _BY_VALUE:
        raise TypeError("%s: no ctypes type for `%s` in `%s`" % (HEADER_PATH, ctype, ' '.join(where.split())))
    return _BY_VALUE[ctype]


def _declarators(text):
    """`const float* x` -> [('const float*', 'x')]; `int B, H` -> [('int', 'B'), ('int', 'H')]."""
    first, *more = [d.strip() for d in text.split(',')]
    ctype, name = re.fullmatch(r'(.*?)\s*(\w+)', first, re.S).groups()
    if more and '*' in ctype:
        raise TypeError("%s: one pointer per declaration, please: `%s`" % (HEADER_PATH, ' '.join(text.split())))
    return [(' '.join(ctype.split()), n) for n in [name] + more]


def _parse_header(path):
    """name -> (restype, [argtypes]), name -> [parameter names], GNX_* -> int, typedef name -> ctypes.Structure."""
    try:
        text = open(path).read()
    except OSError:
        raise HipExtensionMissing("gridnext_amd: %s not found; the ctypes binding is derived from it" % path)
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    constants = {k: int(v) for k, v in re.findall(r'^#define (GNX_\w+) \(?(-?\d+)\)?\s*$', text, re.M)}
    text = re.sub(r'^#.*$', '', text, flags=re.M)
    structs = {}
    for body, name in re.findall(r'typedef struct \{(.*?)\} (\w+);', text, re.S):
        fields = [(n, _ctype(t, name)) for stmt in body.split(';') if stmt.strip() for t, n in _declarators(stmt)]
        structs[name] = type(name, (ctypes.Structure,), {'_fields_': fields})
    text = re.sub(r'typedef struct \{.*?\} \w+;', '', text, flags=re.S)
    signatures, params = {}, {}
    for decl in re.finditer(r'^([a-z ]+?) (gnx_\w+)\(([^()]*)\);', text, re.M):
        res, name, plist = decl.groups()
        plist = [] if plist.strip() in ('', 'void') else [_declarators(p)[0] for p in plist.split(',')]
        signatures[name] = (_ctype(res, decl[0]), [_ctype(t, decl[0]) for t, _ in plist])
        params[name] = [n for _, n in plist]
    stray = set(re.findall(r'\b(gnx_\w+)\s*\(', text)) - set(signatures)
    if stray:
        raise TypeError("%s: cannot read the declaration of %s" % (path, ', '.join(sorted(stray))))
    return signatures, params, constants, structs


# name -> (restype, [argtypes]); name -> [parameter names]; every `#define GNX_<NAME> <integer>`
SIGNATURES, PARAMS, CONSTANTS, _STRUCTS = _parse_header(HEADER_PATH)

_lib = None
ERR_UNSUPPORTED = CONSTANTS['GNX_ERR_UNSUPPORTED']
_ERRORS = {CONSTANTS['GNX_ERR_BAD_ARG']: 'bad argument', CONSTANTS['GNX_ERR_LAUNCH']: 'kernel launch failed',
           ERR_UNSUPPORTED: 'unsupported shape'}


def struct(name):
    """The ctypes.Structure of one of the header's `typedef struct` blocks, fields in the header's order."""
    return _STRUCTS[name]


def lib():
    """The loaded library; raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionMissing(
                "gridnext_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C gridnext_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError here = header/library mismatch: fail loudly
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t, dtype=torch.float32):
    """Device pointer of a tensor that must live on a HIP device; None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("gridnext_amd kernels need tensors on a HIP device (got %s); there is no CPU path"
                           % t.device)
    if dtype is not None and t.dtype != dtype:
        raise TypeError("expected %s, got %s" % (dtype, t.dtype))
    return t.data_ptr()


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError("%s failed: %s (%d)" % (name, _ERRORS.get(rc, 'error'), rc))


def try_call(name, *args):
    """`call` for an entry point that may decline a shape: True when it ran, False when it returned ERR_UNSUPPORTED (the
    caller then takes its general form); any other error raises."""
    rc = getattr(lib(), name)(*args)
    if rc == ERR_UNSUPPORTED:
        return False
    if rc != 0:
        raise RuntimeError("%s failed: %s (%d)" % (name, _ERRORS.get(rc, 'error'), rc))
    return True


def query(name, *args):
    return getattr(lib(), name)(*args)

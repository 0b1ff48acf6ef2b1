"""ctypes binding of libsegan_hip.so (the C ABI declared in include/segan_hip.h, and the additive
exports of the extension headers include/segan_dereverb.h, include/segan_pyin.h,
include/segan_omlsa.h and include/segan_rir.h).

The signatures and the integer macros are read from the header itself, so the binding cannot
drift from the declarations the HIP sources are compiled against.

The product path has no fallback: if the library is missing or a call fails, a
RuntimeError carrying ``segan_last_error()`` is raised.
"""
import ctypes
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SEGAN_HIP_LIB') or os.path.join(_HERE, 'libsegan_hip.so')   # override: A/B of two builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'segan_hip.h')
# exports added beside ABI 17 without touching the main header (the WPE dereverberation baseline)
EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'segan_dereverb.h')
# the same for the Viterbi-smoothed pitch tracker
PYIN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'segan_pyin.h')
# and for the OM-LSA enhancer
OMLSA_HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'segan_omlsa.h')
# and for the room-impulse-response synthesis
RIR_HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'segan_rir.h')


class SeganSrc(Structure):
    """Mirror of ``segan_src`` (include/segan_hip.h)."""
    _fields_ = [('p0', c_void_p), ('p1', c_void_p), ('C0', c_int32), ('C1', c_int32),
                ('scale', c_void_p), ('shift', c_void_p), ('slope', c_void_p)]


_SCALARS = {'int': c_int, 'float': c_float, 'double': c_double, 'size_t': c_size_t,
            'int64_t': c_int64, 'long long': c_int64}


class _Defines(dict):
    """name -> int of the header's integer macros; asking for any other name raises."""

    def __init__(self, where):
        dict.__init__(self)
        self.where, self.unread = where, {}

    def __missing__(self, name):
        raise RuntimeError('{}: no integer `#define {}` ({})'.format(
            self.where, name, self.unread.get(name, 'not defined')))


def _ctype(text, decl, ret=False):
    tok = [w for w in re.findall(r'\w+|\S', text) if w != 'const']
    if not ret:
        if len(tok) < 2 or not re.match(r'[A-Za-z_]\w*$', tok[-1]):
            raise RuntimeError('unnamed or unreadable argument `{}` in `{}`'.format(text.strip(), decl))
        tok.pop()                    # the argument's name
    stars = tok.count('*')
    base = tok[:len(tok) - stars]    # the stars follow the type's words, or the type is not read
    if stars and base and '*' not in base:
        if not ret:
            return POINTER(SeganSrc) if tok == ['segan_src', '*'] else c_void_p
        if tok == ['char', '*']:
            return c_char_p
    elif ret and tok == ['void']:
        return None
    elif ' '.join(tok) in _SCALARS:
        return _SCALARS[' '.join(tok)]
    raise RuntimeError('unknown type `{}` in `{}`'.format(text.strip(), decl))


def read_header(text, where='<text>'):
    """(SIGNATURES, DEFINES) of a header given as text: every ``ret segan_name(args);`` as name ->
    (restype, argtypes) in header order, and every ``#define SEGAN_NAME <integer literal>``.  Not a
    C parser: whatever it cannot map raises with the declaration, it never guesses."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    defines = _Defines(where)
    seen = {}
    for name, val in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SEGAN_\w+)[ \t]+(\S.*?)[ \t]*$', text, flags=re.M):
        seen.setdefault(name, []).append(val)
    for name, vals in seen.items():
        if len(set(vals)) == 1 and re.match(r'-?(0[xX][0-9a-fA-F]+|[1-9]\d*|0)$', vals[0]):
            defines[name] = int(vals[0], 0)
        else:                        # an expression, or definitions that differ: not ours to evaluate
            defines.unread[name] = ' / '.join('#define {} {}'.format(name, v) for v in vals)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    signatures = {}
    for m in re.finditer(r'[^;{}]*\bsegan_\w+\s*\([^;]*(;|$)', text):
        decl = ' '.join(m.group().split())
        d = re.match(r'([\w\s*]+?)\s*\b(segan_\w+)\s*\(([^()]*)\)\s*;$', decl)
        if not d or d.group(2) in signatures:
            raise RuntimeError('{}: cannot read the declaration `{}`'.format(where, decl))
        args = [] if d.group(3).strip() == 'void' else d.group(3).split(',')
        signatures[d.group(2)] = (_ctype(d.group(1), decl, ret=True), [_ctype(a, decl) for a in args])
    return signatures, defines


def _read_header_file(path=HEADER_PATH):
    if not os.path.exists(path):
        raise RuntimeError('segan_pytorch_amd: {} not found. The ctypes binding is read from the '
                           'header the library is built against.'.format(path))
    with open(path) as f:
        return read_header(f.read(), path)


# name -> (restype, argtypes) of every entry point, and name -> int of every SEGAN_* macro
SIGNATURES, DEFINES = _read_header_file()
# the same of the extension header, in tables of their own: SIGNATURES and DEFINES are ABI 17's
EXT_SIGNATURES, EXT_DEFINES = _read_header_file(EXT_HEADER_PATH)
PYIN_SIGNATURES, PYIN_DEFINES = _read_header_file(PYIN_HEADER_PATH)
OMLSA_SIGNATURES, OMLSA_DEFINES = _read_header_file(OMLSA_HEADER_PATH)
RIR_SIGNATURES, RIR_DEFINES = _read_header_file(RIR_HEADER_PATH)

PAD_REFLECT = DEFINES['SEGAN_PAD_REFLECT']
PAD_ZERO = DEFINES['SEGAN_PAD_ZERO']
ACT_NONE = DEFINES['SEGAN_ACT_NONE']
ACT_TANH = DEFINES['SEGAN_ACT_TANH']
ABI_VERSION = DEFINES['SEGAN_ABI_VERSION']

_lib = None


def load():
    """Load (once) and return the ctypes handle; raises if the .so is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'segan_pytorch_amd: {} not found. Build it with `make` (or '
            '`python -c "import __graft_entry__ as g; g.build()"`) at the repo root. '
            'There is no non-HIP fallback.'.format(LIB_PATH))
    # torch bundles its own HIP runtime; it has to be up before this library (linked against
    # /opt/rocm's) is mapped, otherwise the library's first launch finds no device
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:     # pragma: no cover
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (list(SIGNATURES.items()) + list(EXT_SIGNATURES.items()) +
                              list(PYIN_SIGNATURES.items()) + list(OMLSA_SIGNATURES.items()) +
                              list(RIR_SIGNATURES.items())):
        fn = getattr(lib, name)      # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    ver = lib.segan_abi_version()
    if ver != ABI_VERSION:
        raise RuntimeError('libsegan_hip ABI {} != expected {}'.format(ver, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().segan_last_error()
        raise RuntimeError('libsegan_hip {} failed ({}): {}'.format(
            what, rc, msg.decode() if msg else '?'))

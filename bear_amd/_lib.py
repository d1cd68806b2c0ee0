"""ctypes binding of libbear_hip.so (C ABI: include/bear_hip.h).

Fails loudly: a missing library raises ImportError with the build command, and every
non-zero status from the library raises BearError.  No compute path exists outside the
library.
"""
import ctypes
import os
import re

# torch ships its own libamdhip64 (SONAME libamdhip64.so.7); importing it first makes the
# dynamic loader bind libbear_hip.so to that same runtime instance, so device pointers and
# streams are shared with torch.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
def _deterministic_requested():
    v = os.environ.get("BEAR_AMD_DETERMINISTIC", "")
    return bool(v) and v != "0"


# BEAR_AMD_DETERMINISTIC set when the package is first used: the deterministic build of the same sources (libbear_hip_det.so:
# every sum of a launch bit-identical from run to run, include/bear_hip.h).  Set later, the regular library still switches its
# parameter gradients over per call; BEAR_AMD_LIB: developer A/B builds.
LIB_PATH = os.environ.get("BEAR_AMD_LIB") or os.path.join(_HERE, "libbear_hip_det.so" if _deterministic_requested() else "libbear_hip.so")

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bear_hip.h")

_SCALARS = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "double": ctypes.c_double}
_RESULTS = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "const char *": ctypes.c_char_p}


def _param_type(param, decl, path):
    """The ctypes type of one parameter of the declaration ``decl`` ("The binding"); anything else is refused."""
    words = param.replace("*", " ").split()
    stars = param.count("*")
    if stars == 2:
        return ctypes.POINTER(ctypes.c_void_p)          # T **: an out-handle
    if stars == 1:                                       # file names travel as bytes, every other pointer as an address
        return ctypes.c_char_p if words == ["const", "char", "path"] else ctypes.c_void_p
    if stars == 0 and len(words) == 2 and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    raise ImportError(f"{path}: no ctypes type for parameter `{param.strip()}` of `{decl}`")


def read_header(path):
    """(BEAR_ABI_VERSION, {name: (restype, argtypes)}) of every function ``path`` declares, in the header's order.  The header is
    plain C, one declaration per statement; what this reader does not understand is an ImportError, never a guess."""
    try:
        text = open(path).read()
    except OSError as e:
        raise ImportError(f"the C ABI's header was looked for at {path}: {e}; the binding takes every signature from it") from None
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    version = re.search(r"^#define BEAR_ABI_VERSION (\d+)\s*$", text, flags=re.M)
    if version is None or 'extern "C" {' not in text:
        raise ImportError(f"{path}: no BEAR_ABI_VERSION or no extern \"C\" block")
    body = re.sub(r"^\s*#.*$", "", text.split('extern "C" {', 1)[1], flags=re.M)
    sigs = {}
    for stmt in body.split(";"):
        if not re.search(r"\bbear_[a-z0-9_]+\s*\(", stmt):
            continue
        decl = " ".join(stmt.split())
        m = re.fullmatch(r"(.*?)\b(bear_[a-z0-9_]+) ?\(([^()]*)\)", decl)
        result = m and re.sub(r"\s*\*\s*", " *", m.group(1)).strip()
        if not m or result not in _RESULTS:
            raise ImportError(f"{path}: cannot bind `{decl}`: not a declaration with a result type among {sorted(_RESULTS)}")
        params = m.group(3).strip()
        sigs[m.group(2)] = (_RESULTS[result], [] if params == "void" else [_param_type(q, decl, path) for q in params.split(",")])
    unread = sorted(set(re.findall(r"\b(bear_[a-z0-9_]+)\s*\(", text)) - set(sigs))
    if unread:
        raise ImportError(f"{path} mentions {unread} outside a declaration this binding reads")
    return int(version.group(1)), sigs


# read when the package is first used (the header alone, no library needed): the loader below binds exactly these
ABI_VERSION, _SIGNATURES = read_header(HEADER_PATH)
SYMBOLS = list(_SIGNATURES)


ERR_NOMEM = -5   # BEAR_ERR_NOMEM (include/bear_hip.h)


class BearError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = _lib.bear_strerror(status).decode() if _lib is not None else "?"
        hip = _lib.bear_last_hip_error() if (_lib is not None and status == -4) else 0
        super().__init__(f"{where}: {msg} (status {status}" + (f", hipError {hip})" if hip else ")"))


_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). bear_amd has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    rebuild = f"rebuild it with `make -C {os.path.join(_HERE, 'csrc')}`"
    L.bear_abi_version.restype = ctypes.c_int
    if L.bear_abi_version() != ABI_VERSION:
        # a library from another tree may export every symbol and still take its arguments in another order
        raise ImportError(f"{LIB_PATH} speaks ABI version {L.bear_abi_version()}, {HEADER_PATH} declares {ABI_VERSION}: {rebuild}")
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(L, name, None)      # (symbols are added without a new ABI version: a library built before them still answers it)
        if fn is None:
            raise ImportError(f"{LIB_PATH} is stale: it does not export {name}; {rebuild}")
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def lib():
    return _load()


def check(status, where):
    if status != 0:
        raise BearError(status, where)


def call(name, *args):
    """Calls the entry point ``name`` and raises BearError, naming it, on any status but BEAR_OK."""
    check(getattr(lib(), name)(*args), name)

"""ctypes loader for libnfs_hip.so.

include/nfs_hip.h is the only declaration of the C ABI: ``read_header`` derives the argtypes, the return types, the
struct layouts, the NFS_E* codes and the ABI version from it at import time (no compiler, no library, no GPU).

The HIP library is the product path: there is NO CPU fallback.  If the shared
object is missing, importing an op raises immediately (``NfsLibraryError``).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# NFS_LIB_PATH: load another build of the same library (measurement builds made with -DNFS_ABLATE; never the product)
LIB_PATH = os.environ.get("NFS_LIB_PATH") or os.path.join(_HERE, "libnfs_hip.so")
CSRC_DIR = os.path.join(_HERE, "csrc")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "nfs_hip.h"))    # as csrc/common.h includes it


class NfsLibraryError(RuntimeError):
    pass


class NfsError(RuntimeError):
    """an entry point returned non-zero: ``code`` is its NFS_E* value, the message carries nfs_last_error()"""

    def __init__(self, name, code, msg):
        RuntimeError.__init__(self, "%s failed (%d): %s" % (name, code, msg))
        self.name, self.code = name, int(code)


# The closed type vocabulary of the header.  A new type is one line here.
_VALUE = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "int64_t": C.c_int64, "nfs_stream_t": C.c_void_p}
# tensors cross as data_ptr() integers: a pointer to one of these (const or not) is a c_void_p
_POINTEE = {"float", "int", "double", "uint8_t", "uint32_t", "long long", "unsigned long long"}


def read_header(text):
    """(signatures, restypes, structs, constants) of a header in the shape of include/nfs_hip.h: name -> argtypes list,
    name -> return type, typedef name -> ctypes.Structure class, NFS_* macro -> int.  Not a C parser: every statement is
    the stream typedef, a ``typedef struct``, or an ``nfs_*`` declaration over the vocabulary above, or it raises."""
    signatures, restypes, structs, constants = {}, {}, {}, {}

    def ctype(spelling, where, returned=False):
        words = spelling.replace("*", " * ").split()
        if words[-1:] != ["*"]:
            if " ".join(words) in _VALUE:
                return _VALUE[" ".join(words)]
        else:
            base = " ".join(w for w in words[:-1] if w != "const")
            if base in _POINTEE:
                return C.c_void_p
            if base in structs:
                return C.POINTER(structs[base])
            if returned and words == ["const", "char", "*"]:
                return C.c_char_p
        raise NfsLibraryError("nfs_hip.h: type '%s' in '%s' is outside the binding's vocabulary (_lib.read_header)"
                              % (" ".join(words), where))

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(NFS_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M):
        constants[name] = int(value)
    text = re.sub(r'^[ \t]*(#.*|extern[ \t]+"C"[ \t]*\{[ \t]*|\}[ \t]*)$', "", text, flags=re.M)
    statement = r"((?:[^;{}]|\{[^{}]*\})*);"
    rest = re.sub(statement, "", text).strip()
    if rest:
        raise NfsLibraryError("nfs_hip.h: not a statement: '%s'" % rest)
    for st in re.findall(statement, text):
        st = " ".join(st.split())
        m = re.fullmatch(r"typedef struct \{((?:[^;]*;)*) ?\} ?(\w+)", st)
        if m:
            fields = []
            for decl in m.group(1).split(";")[:-1]:
                f = re.fullmatch(r"(.*?)(\w+(?: ?\[\d+\])?(?: ?, ?\w+(?: ?\[\d+\])?)*)", decl.strip())
                if not f:
                    raise NfsLibraryError("nfs_hip.h: not a field: '%s' in '%s'" % (decl.strip(), st))
                t = ctype(f.group(1), st)
                for name, n in re.findall(r"(\w+)(?: ?\[(\d+)\])?", f.group(2)):
                    fields.append((name, t * int(n) if n else t))
            structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
            continue
        m = re.fullmatch(r"(.*?)\b(nfs_\w+) ?\((.*)\)", st)
        if m:
            args = []
            for param in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
                p = re.fullmatch(r"(.*\W)\w+", param.strip())
                if not p:
                    raise NfsLibraryError("nfs_hip.h: not a parameter: '%s' in '%s'" % (param.strip(), st))
                args.append(ctype(p.group(1), st))
            signatures[m.group(2)], restypes[m.group(2)] = args, ctype(m.group(1), st, returned=True)
            continue
        if st != "typedef void* nfs_stream_t":
            raise NfsLibraryError("nfs_hip.h: neither the stream typedef, a struct nor an nfs_* declaration: '%s'" % st)
    return signatures, restypes, structs, constants


try:
    with open(HEADER_PATH) as _f:
        SIGNATURES, RESTYPES, _structs, _constants = read_header(_f.read())
except OSError as e:
    raise NfsLibraryError("the binding is derived from %s, which cannot be read: %s" % (HEADER_PATH, e))
SplatCfg, GramLayer, ConvDesc = _structs["nfs_splat_cfg"], _structs["nfs_gram_layer_t"], _structs["nfs_conv2d_desc_t"]
NFS_EINVAL, NFS_ELAUNCH = _constants["NFS_EINVAL"], _constants["NFS_ELAUNCH"]
ABI_VERSION = _constants["NFS_ABI_VERSION"]          # what nfs_version() of a library built from this header returns

# libnfs_grid2d.so (the 2-D grid stylizer's operators): a library and a header of its own, bound the same way
GRID2D_LIB_PATH = os.path.join(_HERE, "libnfs_grid2d.so")
GRID2D_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "nfs_grid2d.h"))
try:
    with open(GRID2D_HEADER_PATH) as _f:
        GRID2D_SIGNATURES, GRID2D_RESTYPES, _, _c2 = read_header(_f.read())
except OSError as e:
    raise NfsLibraryError("the binding is derived from %s, which cannot be read: %s" % (GRID2D_HEADER_PATH, e))
GRID2D_ABI_VERSION = _c2["NFS_GRID2D_ABI_VERSION"]

# libnfs_descent.so (the update kernels of optimizer 'lapnorm'): the third library and header, bound the same way
DESCENT_LIB_PATH = os.path.join(_HERE, "libnfs_descent.so")
DESCENT_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "nfs_descent.h"))
try:
    with open(DESCENT_HEADER_PATH) as _f:
        DESCENT_SIGNATURES, DESCENT_RESTYPES, _, _c3 = read_header(_f.read())
except OSError as e:
    raise NfsLibraryError("the binding is derived from %s, which cannot be read: %s" % (DESCENT_HEADER_PATH, e))
DESCENT_ABI_VERSION = _c3["NFS_DESCENT_ABI_VERSION"]

# libnfs_colour.so (colour rendering through the views: target_field 'c' of the 3-D particle stylizer): the fourth
COLOUR_LIB_PATH = os.path.join(_HERE, "libnfs_colour.so")
COLOUR_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "nfs_colour.h"))
try:
    with open(COLOUR_HEADER_PATH) as _f:
        COLOUR_SIGNATURES, COLOUR_RESTYPES, _, _c4 = read_header(_f.read())
except OSError as e:
    raise NfsLibraryError("the binding is derived from %s, which cannot be read: %s" % (COLOUR_HEADER_PATH, e))
COLOUR_ABI_VERSION = _c4["NFS_COLOUR_ABI_VERSION"]

# libnfs_emission.so (the emission model of a colour grid: grid_variable 'c' of the grid-sequence stylizer): the fifth
EMISSION_LIB_PATH = os.path.join(_HERE, "libnfs_emission.so")
EMISSION_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "nfs_emission.h"))
try:
    with open(EMISSION_HEADER_PATH) as _f:
        EMISSION_SIGNATURES, EMISSION_RESTYPES, _, _c5 = read_header(_f.read())
except OSError as e:
    raise NfsLibraryError("the binding is derived from %s, which cannot be read: %s" % (EMISSION_HEADER_PATH, e))
EMISSION_ABI_VERSION = _c5["NFS_EMISSION_ABI_VERSION"]

# libnfs_liquid.so (the ray weights of a liquid colour render: --colour_render liquid of the two colour stylizers): the sixth
LIQUID_LIB_PATH = os.path.join(_HERE, "libnfs_liquid.so")
LIQUID_HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "nfs_liquid.h"))
try:
    with open(LIQUID_HEADER_PATH) as _f:
        LIQUID_SIGNATURES, LIQUID_RESTYPES, _, _c6 = read_header(_f.read())
except OSError as e:
    raise NfsLibraryError("the binding is derived from %s, which cannot be read: %s" % (LIQUID_HEADER_PATH, e))
LIQUID_ABI_VERSION = _c6["NFS_LIQUID_ABI_VERSION"]

_lib = None
_lib2d = None
_libdescent = None
_libcolour = None
_libemission = None
_libliquid = None


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libnfs_hip.so, libnfs_grid2d.so, libnfs_descent.so, libnfs_colour.so,
    libnfs_emission.so and libnfs_liquid.so (in-tree)."""
    # (MAX_JOBS when set, else at most 16: the core count of a shared host is not this build's to take)
    jobs = os.environ.get("MAX_JOBS") or str(min(os.cpu_count() or 4, 16))
    r = subprocess.run(["make", "-C", CSRC_DIR, "-j", jobs],
                       capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode != 0:
        raise NfsLibraryError("building libnfs_hip.so failed")
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NfsLibraryError(
                "libnfs_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                "-- there is no CPU fallback for the product path" % LIB_PATH)
        # PyTorch-ROCm ships its own HIP runtime; it must be the one already resident when libnfs_hip.so resolves
        # libamdhip64 -- loading this library first leaves the process with two runtimes and every later launch
        # fails with "no ROCm-capable device is detected" (seen when build() and smoke() shared a process)
        import torch  # noqa: F401
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise NfsLibraryError("cannot load %s: %s" % (LIB_PATH, e))
        for name, argt in SIGNATURES.items():
            try:
                f = getattr(L, name)
            except AttributeError:
                raise NfsLibraryError("libnfs_hip.so does not export %s (stale build?)" % name)
            f.argtypes = argt
            f.restype = RESTYPES[name]
        # the binding is the header at hand, and the library moves with it (entry points, packed-filter sizes, the default
        # GEMM arithmetic): a .so built from another header, with every symbol present, must not be driven by this one
        if L.nfs_version() != ABI_VERSION:
            stale = ("the library is stale: rebuild (make -C %s)" % CSRC_DIR if L.nfs_version() < ABI_VERSION else
                     "the header is stale: %s is older than the library" % HEADER_PATH)
            raise NfsLibraryError("%s reports ABI %d, the header this binding is read from declares %d; %s"
                                  % (LIB_PATH, L.nfs_version(), ABI_VERSION, stale))
        _lib = L
    return _lib


def _load_beside(path, signatures, restypes, version_fn, abi):
    """a library that links against libnfs_hip.so (one error channel, one HIP runtime), loaded after it and checked
    against its own header: every declared symbol present, the version the header's"""
    lib()
    so = os.path.basename(path)
    if not os.path.exists(path):
        raise NfsLibraryError(
            "%s is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
            "-- there is no CPU fallback for the product path" % (so, path))
    try:
        L = C.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise NfsLibraryError("cannot load %s: %s" % (path, e))
    for name, argt in signatures.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            raise NfsLibraryError("%s does not export %s (stale build?)" % (so, name))
        f.argtypes = argt
        f.restype = restypes[name]
    if getattr(L, version_fn)() != abi:
        raise NfsLibraryError("%s reports ABI %d, the header this binding is read from declares %d: rebuild (make -C %s)"
                              % (path, getattr(L, version_fn)(), abi, CSRC_DIR))
    return L


def lib2d():
    """libnfs_grid2d.so, loaded after libnfs_hip.so (it links against it: one error channel, one HIP runtime)"""
    global _lib2d
    if _lib2d is None:
        _lib2d = _load_beside(GRID2D_LIB_PATH, GRID2D_SIGNATURES, GRID2D_RESTYPES, "nfs_grid2d_version", GRID2D_ABI_VERSION)
    return _lib2d


def libdescent():
    """libnfs_descent.so, loaded the same way"""
    global _libdescent
    if _libdescent is None:
        _libdescent = _load_beside(DESCENT_LIB_PATH, DESCENT_SIGNATURES, DESCENT_RESTYPES, "nfs_descent_version",
                                   DESCENT_ABI_VERSION)
    return _libdescent


def libcolour():
    """libnfs_colour.so, loaded the same way"""
    global _libcolour
    if _libcolour is None:
        _libcolour = _load_beside(COLOUR_LIB_PATH, COLOUR_SIGNATURES, COLOUR_RESTYPES, "nfs_colour_version",
                                  COLOUR_ABI_VERSION)
    return _libcolour


def libemission():
    """libnfs_emission.so, loaded the same way"""
    global _libemission
    if _libemission is None:
        _libemission = _load_beside(EMISSION_LIB_PATH, EMISSION_SIGNATURES, EMISSION_RESTYPES, "nfs_emission_version",
                                    EMISSION_ABI_VERSION)
    return _libemission


def libliquid():
    """libnfs_liquid.so, loaded the same way"""
    global _libliquid
    if _libliquid is None:
        _libliquid = _load_beside(LIQUID_LIB_PATH, LIQUID_SIGNATURES, LIQUID_RESTYPES, "nfs_liquid_version",
                                  LIQUID_ABI_VERSION)
    return _libliquid


# Optional live profiling (used by bench.py --full): when PROFILE is a dict, every call is bracketed by
# two events recorded on the SAME stream the kernel is enqueued on; entries are
# name -> [(start_event, end_event, args)].  Costs two event records per call, so it is off by
# default and the headline timing in bench.py is taken with it off.
PROFILE = None


def call(name, *args):
    """Call an int-returning entry point; raise with nfs_last_error() on failure."""
    L = lib()
    if name in GRID2D_SIGNATURES:            # (the error text stays libnfs_hip.so's: the libraries share nfs::set_error)
        L, L0 = lib2d(), L
    elif name in DESCENT_SIGNATURES:
        L, L0 = libdescent(), L
    elif name in COLOUR_SIGNATURES:
        L, L0 = libcolour(), L
    elif name in EMISSION_SIGNATURES:
        L, L0 = libemission(), L
    elif name in LIQUID_SIGNATURES:
        L, L0 = libliquid(), L
    else:
        L0 = L
    if PROFILE is not None:
        import torch
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = getattr(L, name)(*args)
        e1.record()
        PROFILE.setdefault(name, []).append((e0, e1, args))
    else:
        rc = getattr(L, name)(*args)
    if rc != 0:
        raise NfsError(name, rc, L0.nfs_last_error().decode())
    return rc

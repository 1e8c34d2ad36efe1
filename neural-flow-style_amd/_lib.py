"""ctypes loader for libnfs_hip.so and the side libraries beside it.

include/nfs_hip.h is the only declaration of the C ABI: ``read_header`` derives the argtypes, the return types, the
struct layouts, the NFS_E* codes and the ABI version from it at import time (no compiler, no library, no GPU).

A side library is a key of ``SIDE``, of ``SIDE_LATER`` or of ``SIDE_OPEN``: libnfs_<key>.so beside the package, declared in
include/nfs_<key>.h (read by the same ``read_header``), versioned by NFS_<KEY>_ABI_VERSION / nfs_<key>_version().  It links
against libnfs_hip.so (one error channel, one HIP runtime).  The three tables hold one record per key (``SIDE`` the first five
libraries, ``SIDE_LATER`` the sixth, ``SIDE_OPEN`` every one since: a new key goes THERE, and no test pins what that table
holds), ``side(key)`` returns the loaded library of a key of any of them, and ``call`` finds the library that owns a name.

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


def _read(path):
    try:
        with open(path) as f:
            return read_header(f.read())
    except OSError as e:
        raise NfsLibraryError("the binding is derived from %s, which cannot be read: %s" % (path, e))


SIGNATURES, RESTYPES, _structs, _constants = _read(HEADER_PATH)
SplatCfg, GramLayer, ConvDesc = _structs["nfs_splat_cfg"], _structs["nfs_gram_layer_t"], _structs["nfs_conv2d_desc_t"]
NFS_EINVAL, NFS_ELAUNCH = _constants["NFS_EINVAL"], _constants["NFS_ELAUNCH"]
ABI_VERSION = _constants["NFS_ABI_VERSION"]          # what nfs_version() of a library built from this header returns


class SideLibrary:
    """what the binding knows of libnfs_<key>.so: everything but ``handle`` (the loaded library, see ``side``) is derived
    from the key and from include/nfs_<key>.h at import"""

    def __init__(self, key):
        self.key, self.handle = key, None
        self.path = os.path.join(_HERE, "libnfs_%s.so" % key)
        self.header_path = os.path.join(os.path.dirname(HEADER_PATH), "nfs_%s.h" % key)
        self.signatures, self.restypes, _, constants = _read(self.header_path)
        self.abi, self.version_fn = constants["NFS_%s_ABI_VERSION" % key.upper()], "nfs_%s_version" % key


def _owners(records):
    """entry point -> the record of the side library that declares it; a name of nfs_hip.h is in none of them"""
    owners = {}
    for r in records:
        for name in r.signatures:
            if name in owners or name in SIGNATURES:
                raise NfsLibraryError("%s declares %s, which %s declares too: call() could not tell whose it is"
                                      % (r.header_path, name, owners[name].header_path if name in owners else HEADER_PATH))
            owners[name] = r
    return owners


# grid2d: the 2-D grid stylizer's operators; descent: the update kernels of optimizer 'lapnorm'; colour: colour rendering
# through the views (target_field 'c' of the 3-D particle stylizer); emission: the emission model of a colour grid
# (grid_variable 'c' of the grid-sequence stylizer); liquid: the ray weights of a liquid colour render (colour_render
# 'liquid')
SIDE = {k: SideLibrary(k) for k in ("grid2d", "descent", "colour", "emission", "liquid")}
# Two tables, one kind of record: tests/test_side_libraries_cpu.py pins SIDE to the five keys above (and each one's names),
# so a library added since is a record of SIDE_LATER, built after SIDE and bound, owned and loaded in the same way.
# absorb: the derivative of the liquid colour render in the density it is seen through (target_field 'pc')
SIDE_LATER = {k: SideLibrary(k) for k in ("absorb",)}
_OWNER = _owners(list(SIDE.values()) + list(SIDE_LATER.values()))
# THE OPEN TABLE: tests pin SIDE_LATER to ["absorb"] and the names of _OWNER to those six libraries, so every library added
# since is a record here -- append the key; nothing else in this file changes, and no test may assert what this table holds
# as a whole (only that its own key is in it and bound).  Its names are a second lookup that call() consults after _OWNER.
# exposure: the smoke colour render at a fixed exposure and its derivative in the density (colour_render 'exposure')
# carrier: particles moved by a displacement field on a coarse grid, and the transpose of that sampling (target_field 'g')
# flow: particles carried along a flow of the carrier field in K Euler steps, and the sweep back along the path
# (--carrier_steps of target_field 'g')
SIDE_OPEN = {k: SideLibrary(k) for k in ("exposure", "carrier", "flow")}


def _owners_open(records, taken):
    """``_owners`` of the open table; a name that ``taken`` (the names of the two closed tables) holds raises as well"""
    owners = _owners(records)
    for name, r in owners.items():
        if name in taken:
            raise NfsLibraryError("%s declares %s, which %s declares too: call() could not tell whose it is"
                                  % (r.header_path, name, taken[name].header_path))
    return owners


_OWNER_OPEN = _owners_open(list(SIDE_OPEN.values()), _OWNER)
_lib = None


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libnfs_hip.so and one libnfs_<key>.so per side library (in-tree)."""
    # (MAX_JOBS when set, else at most 16: the core count of a shared host is not this build's to take)
    jobs = os.environ.get("MAX_JOBS") or str(min(os.cpu_count() or 4, 16))
    r = subprocess.run(["make", "-C", CSRC_DIR, "-j", jobs],
                       capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode != 0:
        raise NfsLibraryError("building libnfs_hip.so failed")
    return LIB_PATH


def _open(so, path, header_path, signatures, restypes, version_fn, abi):
    """the shared object at ``path``, every declared symbol bound, its version the header's"""
    if not os.path.exists(path):
        raise NfsLibraryError(
            "%s is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
            "-- there is no CPU fallback for the product path" % (so, path))
    # PyTorch-ROCm ships its own HIP runtime; it must be the one already resident when libnfs_hip.so resolves
    # libamdhip64 -- loading this library first leaves the process with two runtimes and every later launch
    # fails with "no ROCm-capable device is detected" (seen when build() and smoke() shared a process)
    import torch  # noqa: F401
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
    # the binding is the header at hand, and the library moves with it (entry points, packed-filter sizes, the default
    # GEMM arithmetic): a .so built from another header, with every symbol present, must not be driven by this one
    got = getattr(L, version_fn)()
    if got != abi:
        stale = ("the library is stale: rebuild (make -C %s)" % CSRC_DIR if got < abi else
                 "the header is stale: %s is older than the library" % header_path)
        raise NfsLibraryError("%s reports ABI %d, the header this binding is read from declares %d; %s"
                              % (path, got, abi, stale))
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = _open("libnfs_hip.so", LIB_PATH, HEADER_PATH, SIGNATURES, RESTYPES, "nfs_version", ABI_VERSION)
    return _lib


def side(key):
    """libnfs_<key>.so, loaded after libnfs_hip.so (it links against it: one error channel, one HIP runtime)"""
    r = SIDE[key] if key in SIDE else SIDE_LATER[key] if key in SIDE_LATER else SIDE_OPEN[key]
    if r.handle is None:
        lib()
        r.handle = _open(os.path.basename(r.path), r.path, r.header_path, r.signatures, r.restypes, r.version_fn, r.abi)
    return r.handle


# Optional live profiling (used by bench.py --full): when PROFILE is a dict, every call is bracketed by
# two events recorded on the SAME stream the kernel is enqueued on; entries are
# name -> [(start_event, end_event, args)].  Costs two event records per call, so it is off by
# default and the headline timing in bench.py is taken with it off.
PROFILE = None


def call(name, *args):
    """Call an int-returning entry point; raise with nfs_last_error() on failure."""
    L0 = lib()                       # (the error text stays libnfs_hip.so's: the libraries share nfs::set_error)
    r = _OWNER.get(name) or _OWNER_OPEN.get(name)
    L = L0 if r is None else side(r.key)
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

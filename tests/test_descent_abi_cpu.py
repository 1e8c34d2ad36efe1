"""libnfs_descent.so against include/nfs_descent.h, without a GPU: every declared symbol is exported and nothing else is, the
version matches, the binding is what the header says, arguments are refused before any launch -- and the other two
libraries' ABIs are what they were (their headers declare none of the descent entry points)."""
import ctypes as C
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I, _F, _L = C.c_void_p, C.c_int, C.c_float, C.c_int64


def _lib():
    from neural_flow_style_amd import _lib
    if not all(os.path.exists(p) for p in (_lib.LIB_PATH, _lib.GRID2D_LIB_PATH, _lib.DESCENT_LIB_PATH)):
        _lib.build()
    return _lib


def _defined(path):
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-nm")
    nm = nm if os.path.exists(nm) else shutil.which("nm")
    assert nm
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    return {n for n in names if re.fullmatch(r"nfs_\w+", n)}


def test_library_and_header_declare_the_same_symbols():
    _l = _lib()
    hdr = open(os.path.join(ROOT, "include", "nfs_descent.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nfs_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_l.DESCENT_SIGNATURES) and len(declared) == 4
    assert _defined(_l.DESCENT_LIB_PATH) == declared
    L = _l.libdescent()
    assert L.nfs_descent_version() == _l.DESCENT_ABI_VERSION == 100


def test_no_symbol_is_shared_with_the_other_two_libraries():
    _l = _lib()
    declared = set(_l.DESCENT_SIGNATURES)
    assert not declared & set(_l.SIGNATURES) and not declared & set(_l.GRID2D_SIGNATURES)
    assert not declared & _defined(_l.LIB_PATH) and not declared & _defined(_l.GRID2D_LIB_PATH)
    assert not _defined(_l.DESCENT_LIB_PATH) & (_defined(_l.LIB_PATH) | _defined(_l.GRID2D_LIB_PATH))


def test_derived_binding_equals_the_rows_typed_by_hand():
    _l = _lib()
    rows = {
        "nfs_descent_version": [],
        "nfs_descent_step": [_P, _P, _L, _F, _P],
        "nfs_advect_descent_fwd": [_P, _P, _P, _F, _P, _P, _I, _I, _I, _P],
        "nfs_advect2d_descent_fwd": [_P, _P, _P, _F, _P, _I, _I, _P],
    }
    assert _l.DESCENT_SIGNATURES == rows
    assert all(t is C.c_int for t in _l.DESCENT_RESTYPES.values())


def test_call_dispatches_on_the_name():
    _l = _lib()
    import pytest
    with pytest.raises(_l.NfsError, match="nfs_descent_step: null pointer") as e:
        _l.call("nfs_descent_step", None, None, 4, 0.1, None)
    assert e.value.code == _l.NFS_EINVAL


def test_arguments_are_refused_before_any_launch_and_reported_through_the_shared_channel():
    _l = _lib()
    L, L0 = _l.libdescent(), _l.lib()
    E = _l.NFS_EINVAL
    # null pointers
    assert L.nfs_descent_step(None, 8, 4, 0.1, None) == E and b"nfs_descent_step: null pointer" in L0.nfs_last_error()
    assert L.nfs_advect_descent_fwd(8, 16, None, 0.1, 32, None, 4, 4, 4, None) == E
    assert b"nfs_advect_descent_fwd: null pointer" in L0.nfs_last_error()
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, None, None, 4, 4, 4, None) == E
    assert b"nfs_advect_descent_fwd: null pointer" in L0.nfs_last_error()
    assert L.nfs_advect2d_descent_fwd(None, 16, 24, 0.1, 32, 4, 4, None) == E
    assert b"nfs_advect2d_descent_fwd: null pointer" in L0.nfs_last_error()
    # an axis shorter than 2
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, 32, None, 4, 1, 4, None) == E and b"at least 2" in L0.nfs_last_error()
    assert L.nfs_advect2d_descent_fwd(8, 16, 24, 0.1, 32, 1, 9, None) == E and b"at least 2" in L0.nfs_last_error()
    # D * H * W >= 2^30
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, 32, None, 1 << 10, 1 << 10, 1 << 10, None) == E
    assert b"2^30" in L0.nfs_last_error()
    assert L.nfs_advect2d_descent_fwd(8, 16, 24, 0.1, 32, 1 << 15, 1 << 15, None) == E and b"2^30" in L0.nfs_last_error()
    # aliases, a negative count, a mask on a voxel count nfs_advect_fwd_live does not take
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, 16, None, 4, 4, 4, None) == E and b"alias" in L0.nfs_last_error()
    assert L.nfs_descent_step(8, 8, 4, 0.1, None) == E and b"alias" in L0.nfs_last_error()
    assert L.nfs_descent_step(8, 16, -1, 0.1, None) == E and b"negative" in L0.nfs_last_error()
    assert L.nfs_advect_descent_fwd(8, 16, 24, 0.1, 32, 40, 5, 6, 7, None) == E and b"multiple of 4" in L0.nfs_last_error()

"""libnfs_grid2d.so against include/nfs_grid2d.h, without a GPU: every declared symbol is exported and nothing else is, the
version matches, the binding is what the header says, arguments are refused before any launch -- and libnfs_hip.so's
own ABI is what it was (its header declares none of the 2-D entry points)."""
import ctypes as C
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I, _F = C.c_void_p, C.c_int, C.c_float


def _lib():
    from neural_flow_style_amd import _lib
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.GRID2D_LIB_PATH)):
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
    hdr = open(os.path.join(ROOT, "include", "nfs_grid2d.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nfs_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_l.GRID2D_SIGNATURES) and len(declared) == 7
    assert _defined(_l.GRID2D_LIB_PATH) == declared
    L = _l.lib2d()
    assert L.nfs_grid2d_version() == _l.GRID2D_ABI_VERSION == 100
    assert not declared & set(_l.SIGNATURES) and not declared & _defined(_l.LIB_PATH)


def test_derived_binding_equals_the_rows_typed_by_hand():
    _l = _lib()
    rows = {
        "nfs_grid2d_version": [],
        "nfs_source2d_velocity_fwd": [_P, _I, _P, _I, _I, _P],
        "nfs_source2d_velocity_bwd": [_P, _I, _P, _I, _I, _P],
        "nfs_advect2d_source_fwd": [_P, _P, _I, _P, _I, _I, _P],
        "nfs_advect2d_source_bwd": [_P, _P, _I, _P, _P, _I, _I, _P],
        "nfs_advect2d_bwd_adam_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _F, _F, _F, _F, _P],
        "nfs_transport_step2d": [_P, _P, _F, _F, _P, _F, _P, _I, _I, _I, _P],
    }
    assert _l.GRID2D_SIGNATURES == rows
    assert all(t is C.c_int for t in _l.GRID2D_RESTYPES.values())


def test_arguments_are_refused_before_any_launch_and_reported_through_the_shared_channel():
    _l = _lib()
    L, L0 = _l.lib2d(), _l.lib()
    assert L.nfs_advect2d_source_fwd(None, None, 0, None, 4, 4, None) == _l.NFS_EINVAL
    assert b"nfs_advect2d_source_fwd: null pointer" in L0.nfs_last_error()
    assert L.nfs_source2d_velocity_fwd(8, 4, 16, 4, 4, None) == _l.NFS_EINVAL and b"src 4" in L0.nfs_last_error()
    assert L.nfs_transport_step2d(8, 8, 1.0, 1.0, None, 0.0, 16, 1, 4, 1, None) == _l.NFS_EINVAL
    assert b"at least 2" in L0.nfs_last_error()
    assert L.nfs_advect2d_bwd_adam_fwd(8, 16, 24, 32, 40, None, 1 << 15, 1 << 15, 0.1, 0.9, 0.999, 1e-8, None) == _l.NFS_EINVAL
    assert b"2^30" in L0.nfs_last_error()

"""The boundary of libnfs_colour.so without a GPU: it exports exactly what include/nfs_colour.h declares, the three
libraries beside it export what they did, and every entry point refuses bad arguments before any launch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    from neural_flow_style_amd import _lib
    if not all(os.path.exists(p) for p in (_lib.LIB_PATH, _lib.GRID2D_LIB_PATH, _lib.DESCENT_LIB_PATH,
                                           _lib.COLOUR_LIB_PATH)):
        _lib.build()
    return _lib


def _defined(path):
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-nm")
    nm = nm if os.path.exists(nm) else shutil.which("nm")
    assert nm, "neither llvm-nm of the ROCm toolchain that built the library nor nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    return {n for n in names if re.fullmatch(r"nfs_\w+", n)}


def test_exported_symbols_equal_the_header():
    _lib = _built()
    hdr = open(os.path.join(ROOT, "include", "nfs_colour.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nfs_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"nfs_colour_version", "nfs_ray_weights", "nfs_colour_project_fwd", "nfs_colour_project_bwd"}
    assert declared == set(_lib.COLOUR_SIGNATURES)
    assert _defined(_lib.COLOUR_LIB_PATH) == declared
    assert _lib.libcolour().nfs_colour_version() == _lib.COLOUR_ABI_VERSION == 100


def test_the_other_libraries_export_what_they_did():
    """libnfs_hip.so keeps its 134 entry points, and each library defines exactly its own header's names: nothing moved
    between them"""
    _lib = _built()
    hip = _defined(_lib.LIB_PATH)
    assert hip == set(_lib.SIGNATURES) and len(hip) == 134
    assert _defined(_lib.GRID2D_LIB_PATH) == set(_lib.GRID2D_SIGNATURES)
    assert _defined(_lib.DESCENT_LIB_PATH) == set(_lib.DESCENT_SIGNATURES)
    assert _lib.ABI_VERSION == _lib.lib().nfs_version()
    assert _lib.lib2d().nfs_grid2d_version() == _lib.GRID2D_ABI_VERSION
    assert _lib.libdescent().nfs_descent_version() == _lib.DESCENT_ABI_VERSION
    names = [set(_lib.SIGNATURES), set(_lib.GRID2D_SIGNATURES), set(_lib.DESCENT_SIGNATURES), set(_lib.COLOUR_SIGNATURES)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not (names[i] & names[j]), names[i] & names[j]


def test_the_binding_routes_a_call_to_the_fourth_library():
    _lib = _built()
    with pytest.raises(_lib.NfsError, match="nfs_ray_weights: null pointer") as e:
        _lib.call("nfs_ray_weights", None, 0.1, None, 1, None, 1, 1, 1, 1, None)
    assert e.value.code == _lib.NFS_EINVAL


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch; tests/test_colour_kernels_gpu.py repeats the refusals on device buffers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
def test_every_argument_refusal():
    _lib = _built()
    bufs = [ctypes.create_string_buffer(64) for _ in range(4)]                # distinct, non-null, never dereferenced
    a, b, c, d = [ctypes.addressof(x) for x in bufs]
    BIG = (1 << 10, 1 << 10, 1 << 10)                                          # V D H W = 2^30 at V = 1

    def refused(name, args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg

    # nfs_ray_weights(d_rot, tau, gmax, G, w, V, D, H, W)
    n = "nfs_ray_weights"
    for i in (0, 2, 4):
        args = [a, 0.1, b, 1, c, 2, 3, 4, 5]
        args[i] = None
        refused(n, args, "null pointer")
    for dims in ((0, 3, 4, 5), (2, 0, 4, 5), (2, 3, 0, 5), (2, 3, 4, 0), (-1, 3, 4, 5)):
        refused(n, [a, 0.1, b, 1, c, *dims], "must be at least 1")
    refused(n, [a, 0.1, b, 1, c, 1, *BIG], "below 2^30")
    for G in (0, -1, 3, 5):                                                    # G must divide V = 4
        refused(n, [a, 0.1, b, G, c, 4, 3, 4, 5], "G must divide V")
    refused(n, [a, 0.1, b, 1, b, 2, 3, 4, 5], "gmax must not alias")
    refused(n, [a, 0.1, a, 1, c, 2, 3, 4, 5], "gmax must not alias")

    # nfs_colour_project_fwd(q, rot, w, img, V, D, H, W, C) / nfs_colour_project_bwd(g_img, rot, w, g_q, overwrite, V, ...)
    for n, pre in (("nfs_colour_project_fwd", ()), ("nfs_colour_project_bwd", (1,))):
        for i in range(4):
            ptrs = [a, b, c, d]
            ptrs[i] = None
            refused(n, [*ptrs, *pre, 2, 3, 4, 5, 3], "null pointer")
        for dims in ((0, 3, 4, 5), (2, 0, 4, 5), (2, 3, 0, 5), (2, 3, 4, 0)):
            refused(n, [a, b, c, d, *pre, *dims, 3], "must be at least 1")
        refused(n, [a, b, c, d, *pre, 1, *BIG, 3], "below 2^30")
        for C in (0, 5, -2):
            refused(n, [a, b, c, d, *pre, 2, 3, 4, 5, C], "C must be 1..4")
        for i in range(3):                                                     # the output on any input
            ptrs = [a, b, c, d]
            ptrs[3] = ptrs[i]
            refused(n, [*ptrs, *pre, 2, 3, 4, 5, 3], "must not alias")

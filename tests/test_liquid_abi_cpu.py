"""The boundary of libnfs_liquid.so without a GPU: it exports exactly what include/nfs_liquid.h declares and reports version
100, the binding has the same names and routes to it, the entry point refuses every bad argument and every aliasing before
any launch, and the other five libraries export what they did."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"nfs_liquid_version", "nfs_liquid_weights"}


def _built():
    from neural_flow_style_amd import _lib
    if not all(os.path.exists(p) for p in (_lib.LIB_PATH, _lib.LIQUID_LIB_PATH)):
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
    hdr = open(os.path.join(ROOT, "include", "nfs_liquid.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nfs_[a-z0-9_]+)\s*\(", hdr))
    assert declared == NAMES
    assert declared == set(_lib.LIQUID_SIGNATURES)
    assert _defined(_lib.LIQUID_LIB_PATH) == declared
    assert _lib.libliquid().nfs_liquid_version() == _lib.LIQUID_ABI_VERSION == 100


def test_the_other_five_libraries_export_what_they_did():
    """every name their headers declare and nothing else; libnfs_hip.so keeps its 134 entry points, libnfs_colour.so and
    libnfs_emission.so their version 100 and their names; no name is shared with the sixth"""
    _lib = _built()
    five = [(_lib.LIB_PATH, _lib.SIGNATURES), (_lib.GRID2D_LIB_PATH, _lib.GRID2D_SIGNATURES),
            (_lib.DESCENT_LIB_PATH, _lib.DESCENT_SIGNATURES), (_lib.COLOUR_LIB_PATH, _lib.COLOUR_SIGNATURES),
            (_lib.EMISSION_LIB_PATH, _lib.EMISSION_SIGNATURES)]
    for path, signatures in five:
        assert _defined(path) == set(signatures), path
        assert not (set(signatures) & NAMES)
    assert len(_lib.SIGNATURES) == 134
    assert set(_lib.COLOUR_SIGNATURES) == {"nfs_colour_version", "nfs_ray_weights", "nfs_colour_project_fwd",
                                           "nfs_colour_project_bwd"}
    assert set(_lib.EMISSION_SIGNATURES) == {"nfs_emission_version", "nfs_emission_fwd", "nfs_emission_bwd",
                                             "nfs_emission_bwd_adam"}
    assert _lib.libcolour().nfs_colour_version() == 100 and _lib.libemission().nfs_emission_version() == 100


def test_the_ops_and_engine_layers_have_the_liquid_render():
    from neural_flow_style_amd import engine, ops
    assert callable(ops.liquid_weights)
    assert "liquid" in engine.ColourRenderLoss.RENDERS


def test_the_binding_routes_a_call_to_the_sixth_library():
    _lib = _built()
    with pytest.raises(_lib.NfsError, match="nfs_liquid_weights: null pointer") as e:
        _lib.call("nfs_liquid_weights", None, None, 0.2, None, None, None, 1, 1, 1, 1, None)
    assert e.value.code == _lib.NFS_EINVAL


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch; tests/test_liquid_kernels_gpu.py repeats the refusals on device buffers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
def test_every_argument_refusal():
    _lib = _built()
    # one block of host memory, never dereferenced: d, rot, w, grey, t_total far enough apart for V = 2, D x H x W = 3 x 4 x 5
    V, D, H, W = 2, 3, 4, 5
    block = ctypes.create_string_buffer(8192)
    base = ctypes.addressof(block)
    d, rot, w, grey, t = [base + 1024 * i for i in range(5)]        # (w needs 480 bytes, d 240, rot 72, the images 160)

    def refused(args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call("nfs_liquid_weights", *args, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith("nfs_liquid_weights:") and text in msg, msg

    for i in range(3):                                               # d, rot and w are required
        ptrs = [d, rot, w]
        ptrs[i] = None
        refused([ptrs[0], ptrs[1], 0.2, ptrs[2], grey, t, V, D, H, W], "null pointer")
    for i in range(4):                                               # every size below 1
        for bad in (0, -1):
            dims = [V, D, H, W]
            dims[i] = bad
            refused([d, rot, 0.2, w, grey, t, *dims], "at least 1")
    refused([d, rot, 0.2, w, grey, t, 1, 1024, 1024, 1024], "below 2^30")
    refused([d, rot, 0.2, w, grey, t, 4, 1024, 512, 512], "below 2^30")
    # every output on every input, and on every other output: the same address, and a range that only overlaps
    for out in range(3):
        for other, who in ((d, "d or rot"), (rot, "d or rot"), (d + 8, "d or rot")):
            ptrs = [w, grey, t]
            ptrs[out] = other
            refused([d, rot, 0.2, *ptrs, V, D, H, W], "must not alias " + who)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        ptrs = [w, grey, t]
        ptrs[b] = ptrs[a]
        refused([d, rot, 0.2, *ptrs, V, D, H, W], "must not alias one another")
        ptrs = [w, grey, t]
        ptrs[b] = ptrs[a] + 16
        refused([d, rot, 0.2, *ptrs, V, D, H, W], "must not alias one another")
    # (that buffers which only touch end to end are NOT refused needs a call that goes through, so a device:
    # tests/test_liquid_kernels_gpu.py::test_buffers_that_touch_end_to_end_are_no_overlap)

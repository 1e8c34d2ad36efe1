"""The boundary of libnfs_liquid.so without a GPU: the ops and engine layers have the liquid render, and the entry point
refuses every bad argument and every aliasing before any launch (what it exports, its version and the routing of its names:
tests/test_side_libraries_cpu.py)."""
import ctypes

import pytest
import torch

from tests.test_side_libraries_cpu import _built


def test_the_ops_and_engine_layers_have_the_liquid_render():
    from neural_flow_style_amd import engine, ops
    assert callable(ops.liquid_weights)
    assert "liquid" in engine.ColourRenderLoss.RENDERS


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

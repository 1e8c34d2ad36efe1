"""The boundary of libnfs_colour.so without a GPU: every entry point refuses bad arguments before any launch
(what it exports, its version and the routing of its names: tests/test_side_libraries_cpu.py)."""
import ctypes

import pytest
import torch

from tests.test_side_libraries_cpu import _built


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

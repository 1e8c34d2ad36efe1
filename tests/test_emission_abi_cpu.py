"""The boundary of libnfs_emission.so without a GPU: the ops layer has its three forms and every entry point refuses bad
arguments before any launch (what it exports, its version and the routing of its names: tests/test_side_libraries_cpu.py)."""
import ctypes

import pytest
import torch

from tests.test_side_libraries_cpu import _built


def test_the_ops_layer_has_the_three_forms():
    from neural_flow_style_amd import engine, ops
    assert callable(ops.emission_fwd) and callable(ops.emission_bwd) and callable(ops.emission_bwd_adam)
    assert callable(engine.TFAdamState.step_through_emission)


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch; tests/test_emission_kernels_gpu.py repeats the refusals on device buffers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
def test_every_argument_refusal():
    _lib = _built()
    bufs = [ctypes.create_string_buffer(64) for _ in range(5)]                # distinct, non-null, never dereferenced
    a, b, c, d, e_ = [ctypes.addressof(x) for x in bufs]

    def refused(name, args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg

    # nfs_emission_fwd(c, e, q, n, C)
    n = "nfs_emission_fwd"
    for i in range(3):
        ptrs = [a, b, c]
        ptrs[i] = None
        refused(n, [*ptrs, 5, 3], "null pointer")
    for bad in (0, -1):
        refused(n, [a, b, c, bad, 3], "n must be at least 1")
    refused(n, [a, b, c, 1 << 36, 3], "below 2^36")
    for C in (0, 5, -2):
        refused(n, [a, b, c, 5, C], "C must be 1..4")
    refused(n, [a, b, a, 5, 3], "must not alias")
    refused(n, [a, b, b, 5, 3], "must not alias")

    # nfs_emission_bwd(g_q, c, e, g_c, n, C)
    n = "nfs_emission_bwd"
    for i in range(4):
        ptrs = [a, b, c, d]
        ptrs[i] = None
        refused(n, [*ptrs, 5, 3], "null pointer")
    for bad in (0, -1):
        refused(n, [a, b, c, d, bad, 3], "n must be at least 1")
    refused(n, [a, b, c, d, 1 << 36, 3], "below 2^36")
    for C in (0, 5, -2):
        refused(n, [a, b, c, d, 5, C], "C must be 1..4")
    for i in range(3):                                                         # the output on any input
        ptrs = [a, b, c, d]
        ptrs[3] = ptrs[i]
        refused(n, [*ptrs, 5, 3], "must not alias")

    # nfs_emission_bwd_adam(g_q, c, e, m, v, n, C, lr_t, beta1, beta2, eps)
    n = "nfs_emission_bwd_adam"
    hyper = [1e-3, 0.9, 0.999, 1e-8]
    for i in range(5):
        ptrs = [a, b, c, d, e_]
        ptrs[i] = None
        refused(n, [*ptrs, 5, 3, *hyper], "null pointer")
    for bad in (0, -1):
        refused(n, [a, b, c, d, e_, bad, 3, *hyper], "n must be at least 1")
    refused(n, [a, b, c, d, e_, 1 << 36, 3, *hyper], "below 2^36")
    for C in (0, 5, -2):
        refused(n, [a, b, c, d, e_, 5, C, *hyper], "C must be 1..4")
    # the written arrays c (1), m (3), v (4): pairwise different, and none of them g_q (0) or e (2)
    for i, j in ((1, 3), (1, 4), (3, 4), (1, 0), (3, 0), (4, 0), (1, 2), (3, 2), (4, 2)):
        ptrs = [a, b, c, d, e_]
        ptrs[i] = ptrs[j]
        refused(n, [*ptrs, 5, 3, *hyper], "must not alias")

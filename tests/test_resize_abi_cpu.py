"""nfs_resize3d refuses what it cannot serve before any launch (NFS_EINVAL, nfs_last_error set)."""
import ctypes

import pytest
import torch

from tests.test_abi_cpu import _ensure_built


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
def test_resize3d_refuses_before_any_launch():
    _lib = _ensure_built()
    bufs = [ctypes.create_string_buffer(64) for _ in range(2)]              # distinct, non-null, never dereferenced
    x, out = (ctypes.addressof(b) for b in bufs)
    good = dict(x=x, out=out, D=2, H=2, W=2, C=1, oD=3, oH=3, oW=3, method=1, align=0)

    def refused(text, **over):
        a = dict(good, **over)
        with pytest.raises(_lib.NfsError) as e:
            _lib.call("nfs_resize3d", a["x"], a["out"], a["D"], a["H"], a["W"], a["C"], a["oD"], a["oH"], a["oW"],
                      a["method"], a["align"], 1.0, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith("nfs_resize3d:") and text in msg, msg

    refused("null pointer", x=None)
    refused("null pointer", out=None)
    for k in ("D", "H", "W", "C"):
        refused("non-positive input dimension", **{k: 0})
        refused("non-positive input dimension", **{k: -3})
    for k in ("oD", "oH", "oW"):
        refused("non-positive output dimension", **{k: 0})
    refused("method must be 0 (nearest) or 1 (bilinear)", method=2)
    refused("method must be 0 (nearest) or 1 (bilinear)", method=-1)
    refused("out must not alias x", out=x)
    refused("below 2^31 voxels", oH=1 << 16, oW=1 << 15)


def test_binding_is_in_the_table_at_this_abi():
    _lib = _ensure_built()
    assert "nfs_resize3d" in _lib.SIGNATURES and len(_lib.SIGNATURES["nfs_resize3d"]) == 13
    assert _lib.ABI_VERSION >= 157 and _lib.lib().nfs_version() >= 157
    assert _lib.ABI_VERSION == _lib.lib().nfs_version()

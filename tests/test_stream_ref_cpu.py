"""The stream-function variable without a GPU: tests/stream_ref.py against the oracle's curl lines and autograd of them,
the divergence-free convention (which the channel reversal decides), and the argument checks of the three entry points."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import stream_ref as SR

SHAPES = [(5, 6, 7), (2, 2, 2), (1, 4, 3), (4, 1, 1)]


def oracle_velocity(s):
    """O.curl(s, is_2d=False).flip(-1) for s [D,H,W,3] (a torch tensor).  The oracle's lines have no value on an axis of
    length 1 (their torch.stack fails on the empty differences); the kernels define the difference as zero there, which
    is what the same lines give on the field replicated to two slices along that axis -- evaluated that way, first slice
    taken."""
    x = s[None]
    for ax in (1, 2, 3):
        if x.shape[ax] == 1:
            x = torch.cat([x, x], dim=ax)
    c = O.curl(x, is_2d=False).flip(-1)
    return c[0, :s.shape[0], :s.shape[1], :s.shape[2]]


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_is_the_reversed_oracle_curl_and_its_autograd(shape):
    rng = np.random.RandomState(sum(shape))
    s = rng.randn(*shape, 3)
    g = rng.randn(*shape, 3)
    st = torch.tensor(s, requires_grad=True)
    vo = oracle_velocity(st)
    (vo * torch.tensor(g)).sum().backward()
    assert np.abs(SR.velocity(s) - vo.detach().numpy()).max() <= 1e-12
    assert np.abs(SR.velocity_T(g) - st.grad.numpy()).max() <= 1e-12
    # <velocity(s), g> == <s, velocity_T(g)>, and the all-positive transpose bounds the signed one
    assert abs((SR.velocity(s) * g).sum() - (s * SR.velocity_T(g)).sum()) <= 1e-10
    A = SR.velocity_T(g, absolute=True)
    assert (np.abs(SR.velocity_T(g)) <= A + 1e-12).all()
    ones = SR.velocity_T(np.ones_like(g), absolute=True)
    assert ones.max() <= 8.0          # at most eight terms meet in one element (n - 2 on two axes)


def test_only_the_reversed_curl_is_divergence_free():
    """24^3, psi in float32 at 1 cell, the velocity in float32 as the kernels form it, the divergence in float64:
    max |div| <= 12 * 2^-23 * M (stream_ref.divergence_bound); the curl in its own channel order misses that by more
    than 1e4 -- the convention is not a matter of taste"""
    s = SR.make_psi((24, 24, 24), 1.0, seed=3)
    assert s.dtype == np.float32
    bound = SR.divergence_bound(s)
    vel = SR.velocity(s)
    assert vel.dtype == np.float32
    div = np.abs(SR.divergence(vel)).max()
    div64 = np.abs(SR.divergence(SR.velocity(s.astype(np.float64)))).max()
    wrong = np.abs(SR.divergence(SR.velocity(s, reverse=False))).max()
    print("24^3, 1 cell: max|div| %.3e (float64 arithmetic %.3e), bound %.3e, unreversed %.3e" % (div, div64, bound, wrong))
    assert div <= bound and div64 <= bound
    assert wrong > 1e4 * bound
    assert abs(np.abs(vel / (2.0 / 23)).max() - 1.0) < 1e-5
    # the oracle's float32 lines say the same
    vo = oracle_velocity(torch.tensor(s)).numpy()
    assert np.array_equal(vo, vel)
    assert SR.divergence(np.zeros((2, 5, 5, 3))).size == 0


def test_psi_generator_is_seeded_smooth_and_scaled():
    a, b = SR.make_psi((9, 12, 10), 2.5, seed=1), SR.make_psi((9, 12, 10), 2.5, seed=1)
    assert np.array_equal(a, b) and not np.array_equal(a, SR.make_psi((9, 12, 10), 2.5, seed=2))
    cell = np.asarray([2.0 / 8, 2.0 / 11, 2.0 / 9])
    assert abs(np.abs(SR.velocity(a.astype(np.float64)) / cell).max() - 2.5) < 1e-4
    assert np.abs(a).min() > 0


# ---- the C ABI refuses before any launch (host pointers that must never reach a kernel: only where nothing can be launched)
_ADVECT = {"nfs_advect_stream_fwd": 4, "nfs_advect_stream_bwd": 4}      # pointer arguments before D, H, W
no_device = pytest.mark.skipif(torch.cuda.is_available(),
                               reason="passes dummy host pointers: only where nothing can be launched")


def _library():
    import os
    from neural_flow_style_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _refused(_lib, name, args, text):
    with pytest.raises(_lib.NfsError) as e:
        _lib.call(name, *args)
    assert e.value.code == _lib.NFS_EINVAL
    msg = _lib.lib().nfs_last_error().decode()
    assert msg.startswith(name + ":") and text in msg, msg


@no_device
@pytest.mark.parametrize("name", sorted(_ADVECT))
def test_stream_advect_entry_points_refuse_before_any_launch(name):
    _lib = _library()
    bufs = [ctypes.create_string_buffer(64) for _ in range(4)]
    p = [ctypes.addressof(b) for b in bufs]
    for shape in ((3, 3, 3), (1, 4, 4), (4, 1, 4), (4, 4, 1)):
        _refused(_lib, name, p + list(shape) + [None], "needs D, H, W >= 2")
    if name.endswith("_fwd"):
        # d, s, out, live (nullable)
        for i in range(3):
            _refused(_lib, name, p[:i] + [None] + p[i + 1:] + [4, 4, 4, None], "null pointer")
        _refused(_lib, name, [p[0], p[1], p[0], p[3], 4, 4, 4, None], "out must not alias d or s")
        _refused(_lib, name, [p[0], p[1], p[1], None, 4, 4, 4, None], "out must not alias d or s")
        _refused(_lib, name, p[:3] + [None, 3, 3, 3, None], "needs D, H, W >= 2")       # the mask is optional
    else:
        # d, s, g_out, g_vel
        for i in range(4):
            _refused(_lib, name, p[:i] + [None] + p[i + 1:] + [4, 4, 4, None], "null pointer")
        for i in range(3):
            _refused(_lib, name, p[:3] + [p[i], 4, 4, 4, None], "g_vel must not alias")


@no_device
def test_stream_update_entry_point_checks_its_arguments_and_takes_degenerate_shapes():
    _lib = _library()
    name = "nfs_stream_bwd_adam"
    bufs = [ctypes.create_string_buffer(64) for _ in range(4)]
    p = [ctypes.addressof(b) for b in bufs]
    adam = [1e-3, 0.9, 0.999, 1e-8, None]
    for i in range(4):
        _refused(_lib, name, p[:i] + [None] + p[i + 1:] + [4, 4, 4] + adam, "null pointer")
    for i in (1, 2, 3):
        _refused(_lib, name, [p[i]] + p[1:] + [4, 4, 4] + adam, "g_vel must not alias s, m or v")
    _refused(_lib, name, p + [0, 4, 3] + adam, "non-positive dimension")
    # (1, 4, 3) is a shape it takes: the arguments pass every check, and what comes back is the launch's status -- without a
    # device that is NFS_ELAUNCH, never NFS_EINVAL
    try:
        _lib.call(name, *p, 1, 4, 3, *adam)
    except _lib.NfsError as e:
        assert e.code != _lib.NFS_EINVAL, _lib.lib().nfs_last_error().decode()

"""The potential and Helmholtz variables without a GPU: tests/potential_ref.py against a torch restatement of the reference's
gradient lines and autograd of it, the adjoint identity, what each part of the Helmholtz velocity contributes (rotation
from the stream part only, divergence from the potential part only), the irrotationality bound of a float32 potential
velocity, and the argument checks of the four fused advect entry points."""
import ctypes

import numpy as np
import pytest
import torch

from tests import potential_ref as PR
from tests.potential_torch import torch_grad_reversed, torch_stream_part

SHAPES = [(5, 6, 7), (2, 2, 2), (1, 4, 3), (4, 1, 1), (3, 1, 5)]


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_is_the_reversed_gradient_and_its_autograd(shape):
    rng = np.random.RandomState(sum(shape))
    phi, a = rng.randn(*shape), rng.randn(*shape, 4)
    g = rng.randn(*shape, 3)
    pt = torch.tensor(phi, requires_grad=True)
    vt = torch_grad_reversed(pt)
    (vt * torch.tensor(g)).sum().backward()
    assert np.abs(PR.velocity(phi) - vt.detach().numpy()).max() <= 1e-12
    assert np.abs(PR.velocity_T(g) - pt.grad.numpy()).max() <= 1e-12
    at = torch.tensor(a, requires_grad=True)
    va = torch_stream_part(at[..., :3]) + torch_grad_reversed(at[..., 3])
    (va * torch.tensor(g)).sum().backward()
    assert np.abs(PR.helmholtz_velocity(a) - va.detach().numpy()).max() <= 1e-12
    assert np.abs(PR.helmholtz_velocity_T(g) - at.grad.numpy()).max() <= 1e-12
    # <velocity(x), g> == <x, velocity_T(g)> to 1e-12 relative, for phi and for a
    for v, x, xt in ((PR.velocity(phi), phi, PR.velocity_T(g)), (PR.helmholtz_velocity(a), a, PR.helmholtz_velocity_T(g))):
        lhs, rhs, terms = (v * g).sum(), (x * xt).sum(), np.abs(v * g).sum()
        print("%-10s <v, g> %+.15e  <x, v^T g> %+.15e  difference / |<v, g>| %.1e, / sum|terms| %.1e" % (
            shape, lhs, rhs, abs(lhs - rhs) / abs(lhs), abs(lhs - rhs) / terms))
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    # the all-positive transpose bounds the signed one; at most nine terms meet in one element of the potential's
    A = PR.velocity_T(g, absolute=True)
    assert (np.abs(PR.velocity_T(g)) <= A + 1e-12).all()
    assert (np.abs(PR.helmholtz_velocity_T(g)) <= PR.helmholtz_velocity_T(g, absolute=True) + 1e-12).all()
    assert PR.velocity_T(np.ones_like(g), absolute=True).max() <= 9.0
    assert PR.helmholtz_velocity_T(np.ones_like(g), absolute=True)[..., :3].max() <= 8.0


@pytest.mark.parametrize("shape", [(5, 6, 7), (9, 12, 10)])
def test_each_part_of_the_helmholtz_velocity_contributes_its_own_half(shape):
    """float64: rot(v) = rot(stream part), div(v) = div(potential part), both to 1e-12 relative"""
    a = np.random.RandomState(1).randn(*shape, 4)
    v, vs, vp = PR.helmholtz_velocity(a), PR.stream_part(a), PR.velocity(a[..., 3])
    rot, rot_s = PR.rotation(v), PR.rotation(vs)
    div, div_p = PR.divergence(v), PR.divergence(vp)
    assert rot.size and div.size
    assert np.abs(rot - rot_s).max() <= 1e-12 * np.abs(rot_s).max()
    assert np.abs(div - div_p).max() <= 1e-12 * np.abs(div_p).max()
    assert np.abs(rot_s).max() > 0.1 and np.abs(div_p).max() > 0.1
    assert PR.rotation(np.zeros((2, 5, 5, 3))).size == 0 and PR.divergence(np.zeros((5, 2, 5, 3))).size == 0


@pytest.mark.parametrize("shape", [(4, 6, 10), (9, 12, 10), (24, 24, 24)])
def test_a_float32_potential_velocity_is_irrotational_to_rounding(shape):
    """phi in float32 at 0.5 cell, the velocity in float32 as the kernels form it, the rotation in float64: every component
    within 2^-22 * M, M = max |D_A phi| -- four rounded differences enter each, each within 2^-24 * M.  (NumPy on these
    shapes: the worst ratio to the bound is 0.36.)  A stream velocity of the same size sits about 1e6 above the bound."""
    phi = PR.make_phi(shape, 0.5, seed=3)
    assert phi.dtype == np.float32
    vel = PR.velocity(phi)
    assert vel.dtype == np.float32
    bound = PR.rotation_bound(phi)
    rot = np.abs(PR.rotation(vel)).max()
    rot64 = np.abs(PR.rotation(PR.velocity(phi.astype(np.float64)))).max()
    a = PR.make_a(shape, 1.0, seed=3)
    stream = PR.stream_part(a)
    stream *= np.abs(vel).max() / np.abs(stream).max()
    rot_s = np.abs(PR.rotation(stream)).max()
    print("%-12s 0.5 cell: max|rot| %.3e (%.2f of the bound %.3e; float64 arithmetic %.3e), stream velocity %.3e" % (
        shape, rot, rot / bound, bound, rot64, rot_s))
    assert rot <= bound and rot64 <= bound
    assert rot_s > 1e4 * bound
    cell = np.asarray([2.0 / (n - 1) for n in shape])
    assert abs(np.abs(vel / cell).max() - 0.5) < 1e-5


def test_generators_are_seeded_smooth_and_scaled():
    a, b = PR.make_phi((9, 12, 10), 2.5, seed=1), PR.make_phi((9, 12, 10), 2.5, seed=1)
    assert np.array_equal(a, b) and not np.array_equal(a, PR.make_phi((9, 12, 10), 2.5, seed=2))
    cell = np.asarray([2.0 / 8, 2.0 / 11, 2.0 / 9])
    assert abs(np.abs(PR.velocity(a.astype(np.float64)) / cell).max() - 2.5) < 1e-4
    assert np.abs(PR.velocity(a)).max(axis=-1).min() > 0                            # never flat
    h = PR.make_a((9, 12, 10), 2.5, seed=1)
    assert h.shape == (9, 12, 10, 4) and h.dtype == np.float32
    assert abs(np.abs(PR.helmholtz_velocity(h.astype(np.float64)) / cell).max() - 2.5) < 1e-4
    ps = np.abs(PR.stream_part(h) / cell).max()
    pp = np.abs(PR.velocity(h[..., 3]) / cell).max()
    assert abs(ps / pp - 1.0) < 1e-4                                                # both parts carry the same weight
    for shape in ((1, 4, 3), (4, 1, 1)):                                            # degenerate axes: still a usable start
        assert np.abs(PR.velocity(PR.make_phi(shape, 1.0, seed=5))).max() > 0


# ---- the C ABI refuses before any launch (host pointers that must never reach a kernel: only where nothing can be launched)
_ADVECT = ["nfs_advect_helmholtz_bwd", "nfs_advect_helmholtz_fwd", "nfs_advect_potential_bwd", "nfs_advect_potential_fwd"]
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
@pytest.mark.parametrize("name", _ADVECT)
def test_potential_advect_entry_points_refuse_before_any_launch(name):
    _lib = _library()
    bufs = [ctypes.create_string_buffer(64) for _ in range(4)]
    p = [ctypes.addressof(b) for b in bufs]
    for shape in ((3, 3, 3), (1, 4, 4), (4, 1, 4), (4, 4, 1)):
        _refused(_lib, name, p + list(shape) + [None], "needs D, H, W >= 2")
    if name.endswith("_fwd"):
        # d, variable, out, live (nullable)
        for i in range(3):
            _refused(_lib, name, p[:i] + [None] + p[i + 1:] + [4, 4, 4, None], "null pointer")
        _refused(_lib, name, [p[0], p[1], p[0], p[3], 4, 4, 4, None], "out must not alias d or the variable")
        _refused(_lib, name, [p[0], p[1], p[1], None, 4, 4, 4, None], "out must not alias d or the variable")
        _refused(_lib, name, p[:3] + [None, 3, 3, 3, None], "needs D, H, W >= 2")       # the mask is optional
    else:
        # d, variable, g_out, g_vel
        for i in range(4):
            _refused(_lib, name, p[:i] + [None] + p[i + 1:] + [4, 4, 4, None], "null pointer")
        for i in range(3):
            _refused(_lib, name, p[:3] + [p[i], 4, 4, 4, None], "g_vel must not alias")
    if "helmholtz" in name:                                                          # float4 accesses
        _refused(_lib, name, [p[0], p[1] + 4] + p[2:] + [4, 4, 4, None], "16-byte aligned")


@no_device
@pytest.mark.parametrize("name", ["nfs_potential_bwd_adam", "nfs_helmholtz_bwd_adam"])
def test_update_entry_points_refuse_before_any_launch(name):
    _lib = _library()
    bufs = [ctypes.create_string_buffer(64) for _ in range(4)]
    p = [ctypes.addressof(b) for b in bufs]
    adam = [1e-3, 0.9, 0.999, 1e-8, None]
    for i in range(4):
        _refused(_lib, name, p[:i] + [None] + p[i + 1:] + [4, 4, 4] + adam, "null pointer")
    for i in (1, 2, 3):
        _refused(_lib, name, [p[i]] + p[1:] + [4, 4, 4] + adam, "g_vel must not alias the variable, m or v")
    _refused(_lib, name, p + [0, 4, 3] + adam, "non-positive dimension")
    if "helmholtz" in name:                                                          # float4 accesses
        for i in (1, 2, 3):
            _refused(_lib, name, p[:i] + [p[i] + 4] + p[i + 1:] + [4, 4, 4] + adam, "16-byte aligned")

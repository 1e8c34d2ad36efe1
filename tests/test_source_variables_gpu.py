"""Stylising through a stream function (grid variable 's'), a velocity potential ('p') and the Helmholtz pair ('sp') on
the GPU: the nine kernels against the compositions they replace (bit for bit) and against tests/stream_ref.py /
tests/potential_ref.py, then engine.GridStylizer(target='s' | 'p' | 'sp') and styler_grid.Styler on top of them -- gradient
parity with the oracle chain, steps, graph replay, dead-region skipping, order 2, two ranks, and the properties the
variables exist for: the stream function's flow stays divergence-free, the potential's irrotational, and the pair's velocity
is the sum of its two parts.

The checks are written once here over the three kinds (``check_*``: plain functions).  tests/test_stream_function_gpu.py
('s') and tests/test_potential_gpu.py ('p', 'sp') run them under the test names and cases they have always had; the cases
the three-kind form adds are collected here."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import potential_ref as PR
from tests import stream_ref as SR
from tests.potential_torch import torch_grad_reversed, torch_stream_part

pytestmark = pytest.mark.gpu
LAYERS5 = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (2,2,2): one cell; 240 voxels: one partial wave; (9,12,10); W > 64: the lane walk wraps inside a row; (16,16,16): several blocks
KERNEL_SHAPES = [(2, 2, 2), (4, 6, 10), (9, 12, 10), (12, 20, 68), (16, 16, 16)]
# ... and for the updates additionally: axes of length 1, a voxel count that is no multiple of 4
DEGENERATE_SHAPES = [(1, 4, 3), (4, 1, 1)]
UPDATE_SHAPES = KERNEL_SHAPES + DEGENERATE_SHAPES + [(5, 6, 7)]
KINDS = ["s", "p", "sp"]
B1, B2, EPS = 0.9, 0.999, 1e-8


class Kind(object):
    """what differs between the three variables: the reference functions, the generator and the named ops"""

    def __init__(self, kind):
        from neural_flow_style_amd import ops
        self.kind = kind
        if kind == "s":
            self.make, self.ref_velocity, self.ref_T = SR.make_psi, SR.velocity, SR.velocity_T
            self.velocity, self.velocity_bwd = ops.stream_velocity, ops.stream_velocity_bwd
            self.advect_fwd, self.advect_bwd = ops.advect_stream_fwd, ops.advect_stream_bwd
            self.bwd_adam, self.entry = ops.stream_bwd_adam, "nfs_advect_stream_fwd"
            self.torch_velocity = lambda s: O.curl(s[None], False).flip(-1)[0]
        elif kind == "p":
            self.make, self.ref_velocity, self.ref_T = PR.make_phi, PR.velocity, PR.velocity_T
            self.velocity, self.velocity_bwd = ops.potential_velocity, ops.potential_velocity_bwd
            self.advect_fwd, self.advect_bwd = ops.advect_potential_fwd, ops.advect_potential_bwd
            self.bwd_adam, self.entry = ops.potential_bwd_adam, "nfs_advect_potential_fwd"
            self.torch_velocity = torch_grad_reversed
        else:
            self.make, self.ref_velocity, self.ref_T = PR.make_a, PR.helmholtz_velocity, PR.helmholtz_velocity_T
            self.velocity, self.velocity_bwd = ops.helmholtz_velocity, ops.helmholtz_velocity_bwd
            self.advect_fwd, self.advect_bwd = ops.advect_helmholtz_fwd, ops.advect_helmholtz_bwd
            self.bwd_adam, self.entry = ops.helmholtz_bwd_adam, "nfs_advect_helmholtz_fwd"
            self.torch_velocity = lambda a: torch_stream_part(a[..., :3]) + torch_grad_reversed(a[..., 3])

    def shape(self, D, H, W):
        return {"s": (D, H, W, 3), "p": (D, H, W), "sp": (D, H, W, 4)}[self.kind]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _case(K, shape, cells=2.5):
    """(density [D,H,W,1] random with a zeroed block -- the live mask then has both values --, the variable at ``cells``
    cells, so that back-traced points leave the volume on every face, a random incoming gradient)"""
    rng = np.random.RandomState(sum(shape) + 7)
    D, H, W = shape
    d = rng.rand(D, H, W).astype(np.float32)
    d[: max(D // 2, 1), : max(H // 2, 1), : max(W // 2, 1)] = 0.0
    x = K.make(shape, cells, seed=sum(shape))
    g = rng.randn(D, H, W, 1).astype(np.float32)
    return torch.tensor(d).cuda().unsqueeze(-1), torch.tensor(x).cuda(), torch.tensor(g).cuda()


# ---- 1, 2. velocity and forward kernel ----------------------------------------------------------------------------------
def check_forward_kernel_is_the_composition_bit_for_bit(kind, shape):
    from neural_flow_style_amd import ops
    K = Kind(kind)
    d, x, _ = _case(K, shape)
    assert ops.advect_stream_takes(*shape) and tuple(x.shape) == K.shape(*shape) == ops.source_shape(kind, *shape)
    vel = K.velocity(x)
    assert np.array_equal(vel.cpu().numpy(), K.ref_velocity(x.cpu().numpy()))      # the convention, on the device too
    if kind == "s":                                                               # the operator in the reference's order
        assert torch.equal(ops.curl_fwd(x).flip(-1), vel)
    elif kind == "p":
        assert torch.equal(ops.grad_fwd(x).flip(-1), vel)
    else:
        assert torch.equal(vel, ops.stream_velocity(x[..., :3].contiguous()) + ops.potential_velocity(x[..., 3].contiguous()))
    cell = np.asarray([2.0 / (n - 1) for n in shape], np.float32)
    assert float((vel.cpu() / torch.tensor(cell)).abs().max()) > 2.4
    want = ops.advect_fwd(d, vel)
    assert torch.equal(_bits(K.advect_fwd(d, x)), _bits(want))
    live, live_ref = ops.live_mask(*shape, d), ops.live_mask(*shape, d)
    got = K.advect_fwd(d, x, live=live)
    ops.advect_fwd(d, vel, live=live_ref)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(live.view(torch.int64), live_ref.view(torch.int64))
    n = shape[0] * shape[1] * shape[2]
    words = live.view(torch.int64).cpu().numpy().view(np.uint64)
    on = int(np.unpackbits(words.view(np.uint8), bitorder="little")[:n].sum())
    if n > 8:                                  # (2,2,2) is one cell: every voxel reads the same eight corners
        assert 0 < on < n                                                          # both values occur


def check_velocity_is_zero_along_an_axis_of_length_1(kind, shape):
    """the shapes only the operators and the updates take: the velocity against the float32 reference, bit for bit"""
    K = Kind(kind)
    x = torch.tensor(K.make(shape, 1.0, seed=sum(shape))).cuda()
    vel = K.velocity(x).cpu().numpy()
    assert np.array_equal(vel, K.ref_velocity(x.cpu().numpy())) and np.abs(vel).max() > 0
    if kind == "p":
        for ax, n in enumerate(shape):
            assert n > 1 or not vel[..., ax].any()


def check_transform_grad_is_the_reference_operator_and_differentiable():
    """transform.grad: [B,D,H,W] -> [B,D,H,W,3] in the reference's (dx, dy, dz) order, bit-equal to the torch restatement
    (reversed back) in float32; its autograd gradient is the transpose -- against tests/potential_ref.py in float64 within
    9 * 2^-23 * A (at most nine float32 terms summed; A = the all-positive transpose of |g|)"""
    import neural_flow_style_amd.transform as T
    shape = (5, 6, 7)
    rng = np.random.RandomState(4)
    p = torch.tensor(rng.randn(2, *shape).astype(np.float32)).cuda().requires_grad_()
    g = rng.randn(2, *shape, 3).astype(np.float32)
    out = T.grad(p)
    assert tuple(out.shape) == (2,) + shape + (3,)
    for b in range(2):
        assert torch.equal(out[b].detach().cpu(), torch_grad_reversed(p[b].detach().cpu()).flip(-1))
    (out * torch.tensor(g).cuda()).sum().backward()
    for b in range(2):
        g_rev = g[b][..., ::-1].astype(np.float64)
        err = np.abs(p.grad[b].double().cpu().numpy() - PR.velocity_T(g_rev))
        assert (err <= 9 * 2.0 ** -23 * PR.velocity_T(g_rev, absolute=True)).all()


# ---- 3. adjoint kernel ------------------------------------------------------------------------------------------------
def check_adjoint_kernel_is_the_composition_bit_for_bit(kind, shape):
    from neural_flow_style_amd import ops
    K = Kind(kind)
    d, x, g = _case(K, shape)
    want = ops.advect_bwd(d, K.velocity(x), g, need_d=False)[1]
    a, b = K.advect_bwd(d, x, g), K.advect_bwd(d, x, g)
    assert torch.equal(_bits(a), _bits(want)) and torch.equal(_bits(a), _bits(b))
    assert float(a.abs().max()) > 0


# ---- 4. refused shape -------------------------------------------------------------------------------------------------
def check_shapes_the_fused_advect_refuses_take_the_composition(kind):
    from neural_flow_style_amd import _lib, ops
    K = Kind(kind)
    shape = (7, 6, 11)                                                             # 462 voxels: not a multiple of 4
    d, x, g = _case(K, shape)
    assert not ops.advect_stream_takes(*shape)
    out, g_vel = torch.empty_like(d), torch.empty(*shape, 3).cuda()
    with pytest.raises(_lib.NfsError):
        _lib.call(K.entry, d.data_ptr(), x.data_ptr(), out.data_ptr(), None, *shape, ops._stream())
    with pytest.raises(_lib.NfsError):
        _lib.call(K.entry.replace("_fwd", "_bwd"), d.data_ptr(), x.data_ptr(), g.data_ptr(), g_vel.data_ptr(), *shape,
                  ops._stream())
    vel = K.velocity(x)
    assert torch.equal(_bits(K.advect_fwd(d, x)), _bits(ops.advect_fwd(d, vel)))
    assert torch.equal(_bits(K.advect_bwd(d, x, g)), _bits(ops.advect_bwd(d, vel, g, need_d=False)[1]))


# ---- 5, 6. update kernels -----------------------------------------------------------------------------------------------
def check_update_kernel_gathers_the_transpose_and_applies_adam(kind, shape):
    """first step from zero moments: m = fl(fl(1 - b1) g_x) and v = fl(fl(fl(1 - b2) g_x) g_x) are chains of single
    roundings whichever way the compiler contracts b m + (1 - b) g with m = 0, so their bits pin the gather and its
    summation order (g_x from the stand-alone adjoint); m / (1 - b1) against the float64 transpose within 16 * 2^-23 * A
    (at most nine terms summed -- eight for 's' --, two roundings from the factor; A = the all-positive transpose of |g|); three further steps
    against the unfused pair to the fused-vs-unfused bar of tests/test_engine_gpu.py (rel-L2 < 1e-6)"""
    from neural_flow_style_amd import ops
    K = Kind(kind)
    rng = np.random.RandomState(sum(shape))
    x0 = torch.tensor(K.make(shape, 1.0, seed=5)).cuda()
    g_np = rng.randn(*shape, 3).astype(np.float32)
    g = torch.tensor(g_np).cuda()
    g_x = K.velocity_bwd(g)
    assert tuple(g_x.shape) == tuple(x0.shape)
    if kind == "s":
        assert torch.equal(_bits(g_x), _bits(ops.curl_bwd(g.flip(-1).contiguous())))
    elif kind == "p":
        assert torch.equal(_bits(g_x), _bits(ops.grad_bwd(g.flip(-1).contiguous())))
    x, m, v = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0)
    K.bwd_adam(g, x, m, v, 1e-3, B1, B2, EPS)
    one_b1 = torch.tensor(np.float32(1) - np.float32(B1)).cuda()
    one_b2 = torch.tensor(np.float32(1) - np.float32(B2)).cuda()
    assert torch.equal(_bits(m), _bits(one_b1 * g_x))
    assert torch.equal(_bits(v), _bits((one_b2 * g_x) * g_x))
    got = m.double().cpu().numpy() / float(np.float32(1) - np.float32(B1))
    want = K.ref_T(g_np.astype(np.float64))
    A = K.ref_T(g_np.astype(np.float64), absolute=True)
    err = np.abs(got - want)
    print("update %-2s %-12s first step: max |m/(1-b1) - transpose| %.3e, worst err/bound %.3f" % (
        kind, shape, err.max(), float((err / np.maximum(16 * 2.0 ** -23 * A, 1e-300)).max()) if A.max() > 0 else 0.0))
    assert (err <= 16 * 2.0 ** -23 * A).all()
    # the unfused pair from the same start, then three further steps with fresh gradients
    x_u, m_u, v_u = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0)
    ops.adam_tf_step(x_u, m_u, v_u, g_x, 1e-3, B1, B2, EPS)
    for k in range(3):
        gk = torch.tensor(rng.randn(*shape, 3).astype(np.float32)).cuda()
        K.bwd_adam(gk, x, m, v, 1e-3, B1, B2, EPS)
        ops.adam_tf_step(x_u, m_u, v_u, K.velocity_bwd(gk), 1e-3, B1, B2, EPS)
    for name, a, b in (("var", x, x_u), ("m", m, m_u), ("v", v, v_u)):
        ulp = int((_bits(a).long() - _bits(b).long()).abs().max())
        print("update %-2s %-12s %-3s after 4 steps: rel-L2 %.2e, largest difference %d ulp" % (kind, shape, name, rel(a, b), ulp))
        assert rel(a, b) < 1e-6
    assert float((x - x0).abs().max()) > 0


# ---- 7 - 11. the stylizer -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engine_case(n_layers, V=3, G=24):
    """computed once per layer set and shared (read only): density, views, loss, oracle pieces"""
    from tests.test_engine_gpu import _setup
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, LAYERS5[:n_layers])
    return d0, mats, loss, cfg, w_or, sfe, T, eng


@functools.lru_cache(maxsize=None)
def _start(kind, G=24, cells=0.5):
    return Kind(kind).make((G, G, G), cells, seed=11)


def _stylizer(eng, loss, d0, var, target, **kw):
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target=target, **kw)
    assert tuple(gs.var.shape) == tuple(np.shape(var)) and float(gs.var.abs().max()) == 0       # starts from zero
    gs.var.copy_(torch.as_tensor(var))
    return gs


def check_gradient_parity_with_the_oracle_chain(kind):
    """24^3, 3 views, conv1_1..conv5_1, the variable at 0.5 cell: gradient() against autograd through the torch
    restatement of the velocity -> O.grid_forward; the bars of test_gradient_parity_grid_velocity"""
    K = Kind(kind)
    G, V = 24, 3
    d0, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(5, V, G)
    x0 = _start(kind)
    x_o = torch.tensor(x0).requires_grad_()
    vel_o = K.torch_velocity(x_o)[None]
    rot_o = torch.tensor(np.asarray(mats, np.float32))
    total, per_view, d_out = O.grid_forward(torch.tensor(d0)[None, ..., None], vel_o, rot_o, cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, x_o)
    rot = T.rot_to_device(mats, "cuda")
    gs = _stylizer(eng, loss, d0, x0, kind)
    losses, g_h = gs.gradient(rot)
    print("%s gradient: d_s rel %.2e, losses rel %.2e, gradient rel %.2e" % (
        kind, rel(gs.d_s, d_out[0, ..., 0]), rel(losses, torch.stack(per_view)), rel(g_h, g_o)))
    assert rel(gs.d_s, d_out[0, ..., 0]) < 1e-5
    assert rel(losses, torch.stack(per_view)) < 1e-4
    assert rel(g_h, g_o) < 1e-3
    assert torch.equal(gs.velocity(), K.velocity(gs.var))
    # ... and not the velocity variable's gradient at the same velocity handed through
    gv = _stylizer(eng, loss, d0, gs.velocity().cpu(), "v")
    _, g_vel = gv.gradient(rot)
    assert tuple(g_h.shape) == K.shape(G, G, G) and tuple(g_vel.shape) == (G, G, G, 3)
    handed = {"s": g_vel, "p": g_vel[..., 0]}.get(kind, torch.cat([g_vel, g_vel[..., :1]], dim=-1))
    assert rel(g_h, handed) > 1e-2
    assert rel(g_h, K.velocity_bwd(g_vel)) < 1e-5


def _masked_steps(eng, loss, d0, x0, kind, rot, skip, n=4):
    gs = _stylizer(eng, loss, d0, x0, kind, lr=1e-3, graph=False)
    gs.dead_skip = skip
    gs.step(rot)
    taken = bool(gs._live_kw())
    for _ in range(n - 1):
        gs.step(rot)
    return gs, taken


def _step_case(kind):
    d0, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(3)
    x0 = _start(kind)
    return x0, T.rot_to_device(mats, "cuda"), (lambda **kw: _stylizer(eng, loss, d0, x0, kind, lr=1e-3, **kw))


@functools.lru_cache(maxsize=None)
def _eager_steps(kind):
    """five eager steps from the shared start: (losses, the stylizer) -- read only"""
    x0, rot, make = _step_case(kind)
    a = make(graph=False)
    return [float(a.step(rot)) for _ in range(5)], a


def check_step_is_adam_on_the_gradient_and_lowers_the_loss(kind):
    from neural_flow_style_amd import ops
    x0, rot, make = _step_case(kind)
    a, b = make(graph=False), make(graph=False)
    assert a.slab is None and a._adv_target() is not None and not a._fused_step_ok()
    first = float(a.step(rot))
    _, g = b.gradient(rot)
    b.adam.step(b.var, g, b.lr)
    for x, y in ((a.var, b.var), (a.adam.m, b.adam.m), (a.adam.v, b.adam.v)):
        assert rel(x, y) < 1e-6
    assert float((a.var - torch.tensor(x0).cuda()).abs().max()) > 0
    # the stored forward sample is that of the updated variable
    assert a._adv_valid() and torch.equal(_bits(a._adv_buf),
                                          _bits(ops.advect_fwd(a.d0.unsqueeze(-1), a.velocity()).squeeze(-1)))
    ls, _ = _eager_steps(kind)
    print("%s steps, loss:" % kind, ls)
    assert abs(ls[0] - first) <= 1e-6 * abs(first) and ls[4] < ls[0]
    # L-BFGS only needs gradient(): two finite steps
    lb = make(graph=False, optimizer="lbfgs")
    assert np.isfinite(float(lb.step(rot))) and np.isfinite(float(lb.step(rot)))
    assert float((lb.var - torch.tensor(x0).cuda()).abs().max()) > 0


def check_graph_replay_reads_the_moved_variable_and_follows_the_eager_steps(kind):
    """warm, capture, then move the variable in place: the replayed gradient is that of the new variable; whole steps
    through the graph follow the eager trajectory"""
    x0, rot, make = _step_case(kind)
    ls, a = _eager_steps(kind)
    c = make(graph=True)
    for _ in range(2):
        c._field_gradient_graphed(rot)
    assert c._graph is not None
    x1 = a.var.clone()
    c.var.copy_(x1)
    _, g_ds = c._field_gradient_graphed(rot)
    g_replay = c.variable_gradient(g_ds)
    e = make(graph=False)
    e.var.copy_(x1)
    _, g_eager = e.gradient(rot)
    assert rel(g_replay, g_eager) < 1e-5
    cg = make(graph=True)
    lg = [float(cg.step(rot)) for _ in range(5)]
    assert cg._graph is not None
    np.testing.assert_allclose(lg, ls, rtol=1e-6)
    assert rel(cg.var, a.var) < 1e-6


def check_dead_region_skipping_leaves_every_bit_of_the_update(kind):
    """dead_skip on and off: the variable, m and v bit-identical after four steps (g_vel is an exact +-0 at dead voxels,
    which leaves the gathered sums and ApplyAdam unchanged), and the masked path was actually taken"""
    d0, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(3)
    rot = T.rot_to_device(mats, "cuda")
    on, taken_on = _masked_steps(eng, loss, d0, _start(kind), kind, rot, True)
    off, taken_off = _masked_steps(eng, loss, d0, _start(kind), kind, rot, False)
    assert taken_on and not taken_off
    for x, y in ((on.var, off.var), (on.adam.m, off.adam.m), (on.adam.v, off.adam.v)):
        assert torch.equal(_bits(x), _bits(y))


def check_the_flow_stays_divergence_free_and_a_free_velocity_does_not():
    d0, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(3)
    rot = T.rot_to_device(mats, "cuda")
    psi = _start("s")
    gs = _stylizer(eng, loss, d0, psi, "s", lr=1e-3, graph=False)
    vel_start = gs.velocity().clone()
    gv = _stylizer(eng, loss, d0, vel_start.cpu(), "v", lr=1e-3, graph=False)
    for _ in range(4):
        gs.step(rot)
        gv.step(rot)
    psi_fin = gs.var.cpu().numpy()
    bound = SR.divergence_bound(psi_fin)
    div_s = float(np.abs(SR.divergence(gs.velocity().cpu().numpy())).max())
    div_v = float(np.abs(SR.divergence(gv.var.cpu().numpy())).max())
    print("after 4 steps: max|div| stream %.3e (bound %.3e), free velocity %.3e" % (div_s, bound, div_v))
    assert float((gs.var - torch.tensor(psi).cuda()).abs().max()) > 0
    assert div_s <= bound
    assert div_v > 100 * bound


def check_the_potential_flow_stays_irrotational_and_a_free_velocity_does_not():
    d0, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(3)
    rot = T.rot_to_device(mats, "cuda")
    phi = _start("p")
    gs = _stylizer(eng, loss, d0, phi, "p", lr=1e-3, graph=False)
    vel_start = gs.velocity().clone()
    gv = _stylizer(eng, loss, d0, vel_start.cpu(), "v", lr=1e-3, graph=False)
    for _ in range(4):
        gs.step(rot)
        gv.step(rot)
    bound = PR.rotation_bound(gs.var.cpu().numpy())
    rot_p = float(np.abs(PR.rotation(gs.velocity().cpu().numpy())).max())
    rot_v = float(np.abs(PR.rotation(gv.var.cpu().numpy())).max())
    print("after 4 steps: max|rot| potential %.3e (bound %.3e), free velocity %.3e" % (rot_p, bound, rot_v))
    assert float((gs.var - torch.tensor(phi).cuda()).abs().max()) > 0
    assert rot_p <= bound
    assert rot_v > 100 * bound


def check_the_helmholtz_velocity_is_the_sum_of_its_parts_and_both_move():
    from neural_flow_style_amd import ops
    d0, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(3)
    rot = T.rot_to_device(mats, "cuda")
    a0 = _start("sp")
    gs = _stylizer(eng, loss, d0, a0, "sp", lr=1e-3, graph=False)
    for _ in range(4):
        gs.step(rot)
    psi, phi = gs.var[..., :3].contiguous(), gs.var[..., 3].contiguous()
    assert torch.equal(_bits(gs.velocity()), _bits(ops.stream_velocity(psi) + ops.potential_velocity(phi)))
    start = torch.tensor(a0).cuda()
    assert float((psi - start[..., :3]).abs().max()) > 0 and float((phi - start[..., 3]).abs().max()) > 0


# ---- 12. order 2 ------------------------------------------------------------------------------------------------------
def check_order_2_runs_through_the_materialised_velocity(kind):
    import neural_flow_style_amd.engine as eng
    import neural_flow_style_amd.transform as T
    import neural_flow_style_amd.vgg as vgg
    from neural_flow_style_amd import ops
    from tests.synth import style_image, uniform_views
    K = Kind(kind)
    shape = (9, 12, 10)
    rng = np.random.RandomState(3)
    d0 = np.clip(rng.rand(*shape).astype(np.float32) - 0.4, 0, 1)
    x0 = K.make(shape, 0.5, seed=2)
    layers = ["conv1_1", "conv2_1"]
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv2_1"), "cuda")
    loss = eng.RenderStyleLoss(net, layers, [1.0, 1.0], 1.0, transmit=0.05)
    loss.set_style_image(style_image(shape[1], shape[2], rng))
    rot = T.rot_to_device(uniform_views(2), "cuda")
    gs = _stylizer(eng, loss, d0, x0, kind, lr=1e-3, graph=False, adv_order=2)
    assert gs._adv_target() is None and gs._live_target() is None
    _, g = gs.gradient(rot)
    vel = K.velocity(gs.var)
    assert torch.equal(_bits(gs._mc_vel), _bits(vel))
    g_adv = ops.smooth3d_relu_bwd(gs.d_s, gs.g_ds, gs.k)
    _, g_vel = ops.advect_maccormack_bwd(gs.d0.unsqueeze(-1), vel, gs._mc_fwd, gs._mc_keep, g_adv.unsqueeze(-1),
                                         need_d=False)
    assert torch.equal(_bits(g), _bits(K.velocity_bwd(g_vel)))
    assert float(g.abs().max()) > 0
    gs1 = _stylizer(eng, loss, d0, x0, kind, lr=1e-3, graph=False)
    assert not torch.equal(gs1.gradient(rot)[1], g)                                 # not the first-order gradient
    assert np.isfinite(float(gs.step(rot)))
    assert float((gs.var - torch.tensor(x0).cuda()).abs().max()) > 0


# ---- 13. two ranks ----------------------------------------------------------------------------------------------------
_RANK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from neural_flow_style_amd import engine, vgg
from neural_flow_style_amd import synthetic as S, transform as T
from tests import potential_ref as PR, stream_ref as SR
kind = sys.argv[2]
world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) %% torch.cuda.device_count())
torch.cuda.set_device(dev)
if world > 1:
    dist.init_process_group("gloo")
G, V = 24, 6
rng = np.random.RandomState(5)
d0 = S.blob_density(G, rng)
simg = S.style_image(G, G, rng)
net = vgg.VGG(vgg.synthetic_weights(123, upto="conv3_1"), dev)
loss = engine.RenderStyleLoss(net, ["conv1_1", "conv2_1", "conv3_1"], [1.0] * 3, 1.0, transmit=0.02)
loss.set_style_image(simg)
gs = engine.GridStylizer(loss, torch.tensor(d0, device=dev), k=3, target=kind, lr=1e-3,
                         process_group=dist.group.WORLD if world > 1 else None)
assert gs.slab is None
make = {"s": SR.make_psi, "p": PR.make_phi, "sp": PR.make_a}[kind]
gs.var.copy_(torch.tensor(make((G, G, G), 0.5, seed=11)))
rot = T.rot_to_device(S.uniform_views(V), dev)[rank::world].contiguous()
ls = [float(gs.step(rot)) for _ in range(4)]
np.savez(sys.argv[1] + ".%%d.npz" %% rank, l=np.asarray(ls), var=gs.var.cpu().numpy())
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


def check_two_ranks_sharing_the_views_keep_bit_identical_replicas(kind, tmp_path):
    """views sharded over two gloo ranks in the all-reduce mode (these variables have no slab form): after four steps both
    replicas of the variable are bit-identical -- every rank repeats deterministic field work on the summed density gradient -- and
    the first loss is the one-rank run's to rtol 2e-6"""
    from tests.ranks import require_gpus_for, run_ranks
    require_gpus_for(2)
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NFS_SLAB_SHARD"):
        env.pop(k, None)
    subprocess.run([sys.executable, str(script), str(tmp_path / "one"), kind], check=True, env=env, timeout=600)
    run_ranks([sys.executable, str(script), str(tmp_path / "two"), kind], 2, env, timeout=900)
    one = np.load(str(tmp_path / "one") + ".0.npz")
    r0, r1 = (np.load(str(tmp_path / "two") + ".%d.npz" % r) for r in (0, 1))
    assert np.array_equal(r0["var"].view(np.int32), r1["var"].view(np.int32))
    assert np.array_equal(r0["l"], r1["l"])
    np.testing.assert_allclose(r0["l"][0], one["l"][0], rtol=2e-6)
    print("%s losses, one rank:" % kind, one["l"], "two ranks:", r0["l"])


# ---- 14. styler_grid --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _velocity_run(G, F):
    """the 'v' run the variables are compared with, once"""
    from neural_flow_style_amd.styler_grid import Styler
    from tests.test_sequence_gpu import _cfg_for, sequence_case, v_init_for
    d, u, simg = sequence_case(G, F)
    sv = Styler(_cfg_for(G, F, simg, grid_variable="v", iter=4))
    sv.load_img([G, G])
    return sv.run({"d": d, "v": u, "v_init": v_init_for(G, F)})


def check_styler_grid_optimises_the_variable_per_frame(kind):
    from neural_flow_style_amd import ops
    from neural_flow_style_amd.styler_grid import Styler
    from tests.test_sequence_gpu import _cfg_for, sequence_case
    K = Kind(kind)
    G, F = 16, 3
    d, u, simg = sequence_case(G, F)
    init = [K.make((G, G, G), 0.5, seed=20 + t) for t in range(F)]
    st = Styler(_cfg_for(G, F, simg, grid_variable=kind, iter=4))
    st.load_img([G, G])
    r = st.run({"d": d, "v": u, kind + "_init": init})
    hist = np.asarray(r["l_frames"])
    print("styler_grid grid_variable=%s losses per iteration:" % kind, hist.sum(1))
    assert hist.shape[0] == 4 and np.isfinite(hist).all() and hist[-1].sum() < hist[0].sum()
    assert len(r["v"]) == len(r["opt"]) == F
    assert r["p"] is None                                       # the reference's particle-position key
    assert (r["s"] is None) if kind == "p" else len(r["s"]) == F
    assert (r["phi"] is None) if kind == "s" else len(r["phi"]) == F
    for t in range(F):
        opt = r["opt"][t]
        assert opt.shape == K.shape(G, G, G) and not np.array_equal(opt, init[t])
        if kind == "s":
            assert np.array_equal(r["s"][t], opt)
        elif kind == "p":
            assert np.array_equal(r["phi"][t], opt)
        else:
            assert np.array_equal(r["s"][t], opt[..., :3]) and np.array_equal(r["phi"][t], opt[..., 3])
        vt = K.velocity(torch.tensor(opt).cuda())
        assert np.array_equal(r["v"][t], vt.cpu().numpy()), t
        dt = torch.tensor(d[t]).cuda().unsqueeze(-1)
        want = ops.smooth3d_relu_fwd(ops.advect_fwd(dt, torch.tensor(r["v"][t]).cuda()).squeeze(-1).contiguous(), 3.0).abs()
        assert np.array_equal(r["d"][t][..., 0], want.cpu().numpy()), t
    rv = _velocity_run(G, F)
    assert not np.array_equal(rv["v"][0], r["v"][0]) and not np.array_equal(rv["d"][0], r["d"][0])


def check_styler_grid_starts_from_zero_without_an_init(kind):
    """no ``s_init`` / ``p_init`` / ``sp_init``: the variable starts flat and one iteration moves it"""
    from neural_flow_style_amd.styler_grid import Styler
    from tests.test_sequence_gpu import _cfg_for, sequence_case
    G, F = 16, 3
    d, u, simg = sequence_case(G, F)
    st = Styler(_cfg_for(G, F, simg, grid_variable=kind, iter=1))
    st.load_img([G, G])
    st.prepare({"d": d, "v": u})
    C = {"s": 3, "p": 1, "sp": 4}[kind]
    assert all(float(x.abs().max()) == 0 and tuple(x.shape) == (G, G, G, C) for x in st._st.g_opt.values())
    st.iterate()
    r = st.finish()
    assert np.isfinite(np.asarray(r["l_frames"])).all() and any(np.abs(x).max() > 0 for x in r["opt"])
    assert all(x.shape == Kind(kind).shape(G, G, G) for x in r["opt"])


# ---- the cases the three kinds add to the two older files' ------------------------------------------------------------
@pytest.mark.parametrize("shape", DEGENERATE_SHAPES)
def test_stream_velocity_is_zero_along_an_axis_of_length_1(shape):
    check_velocity_is_zero_along_an_axis_of_length_1("s", shape)


@pytest.mark.parametrize("shape", [(4, 6, 10), (12, 20, 68), (16, 16, 16)])
def test_stream_update_kernel_on_the_shapes_of_the_other_updates(shape):
    assert shape in UPDATE_SHAPES
    check_update_kernel_gathers_the_transpose_and_applies_adam("s", shape)


def test_styler_grid_starts_a_stream_function_from_zero_without_an_init():
    check_styler_grid_starts_from_zero_without_an_init("s")


def test_two_ranks_keep_bit_identical_replicas_of_the_helmholtz_pair(tmp_path):
    check_two_ranks_sharing_the_views_keep_bit_identical_replicas("sp", tmp_path)

"""Stylising through a stream function (grid variable 's') on the GPU: the three kernels against the compositions they
replace (bit for bit) and against tests/stream_ref.py, then engine.GridStylizer(target='s') and styler_grid.Styler on top
of them -- gradient parity with the oracle chain, steps, graph replay, dead-region skipping, order 2, two ranks, and the
property the variable exists for: the flow stays divergence-free."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import stream_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS5 = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]
# (2,2,2); 240 voxels: one partial wave; (9,12,10); W > 64: the lane walk wraps inside a row; (16,16,16): several blocks
KERNEL_SHAPES = [(2, 2, 2), (4, 6, 10), (9, 12, 10), (12, 20, 68), (16, 16, 16)]
B1, B2, EPS = 0.9, 0.999, 1e-8


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _case(shape, cells=2.5):
    """(density [D,H,W,1] random with a zeroed block -- the live mask then has both values --, psi at ``cells`` cells, so
    that back-traced points leave the volume on every face, a random incoming gradient)"""
    rng = np.random.RandomState(sum(shape) + 7)
    D, H, W = shape
    d = rng.rand(D, H, W).astype(np.float32)
    d[: max(D // 2, 1), : max(H // 2, 1), : max(W // 2, 1)] = 0.0
    s = SR.make_psi(shape, cells, seed=sum(shape))
    g = rng.randn(D, H, W, 1).astype(np.float32)
    return torch.tensor(d).cuda().unsqueeze(-1), torch.tensor(s).cuda(), torch.tensor(g).cuda()


# ---- 1. forward kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_forward_kernel_is_the_composition_bit_for_bit(shape):
    from neural_flow_style_amd import ops
    d, s, _ = _case(shape)
    assert ops.advect_stream_takes(*shape)
    vel = ops.stream_velocity(s)
    assert np.array_equal(vel.cpu().numpy(), SR.velocity(s.cpu().numpy()))        # the convention, on the device too
    cell = np.asarray([2.0 / (n - 1) for n in shape], np.float32)
    assert float((vel.cpu() / torch.tensor(cell)).abs().max()) > 2.4
    want = ops.advect_fwd(d, vel)
    assert torch.equal(_bits(ops.advect_stream_fwd(d, s)), _bits(want))
    live, live_ref = ops.live_mask(*shape, d), ops.live_mask(*shape, d)
    got = ops.advect_stream_fwd(d, s, live=live)
    ops.advect_fwd(d, vel, live=live_ref)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(live.view(torch.int64), live_ref.view(torch.int64))
    n = shape[0] * shape[1] * shape[2]
    words = live.view(torch.int64).cpu().numpy().view(np.uint64)
    on = int(np.unpackbits(words.view(np.uint8), bitorder="little")[:n].sum())
    if n > 8:                                  # (2,2,2) is one cell: every voxel reads the same eight corners)
        assert 0 < on < n                                                          # both values occur


def test_shapes_the_fused_advect_refuses_take_the_composition():
    from neural_flow_style_amd import _lib, ops
    shape = (7, 6, 11)                                                             # 462 voxels: not a multiple of 4
    d, s, g = _case(shape)
    assert not ops.advect_stream_takes(*shape)
    with pytest.raises(_lib.NfsError):
        _lib.call("nfs_advect_stream_fwd", d.data_ptr(), s.data_ptr(), torch.empty_like(d).data_ptr(), None, *shape,
                  ops._stream())
    vel = ops.stream_velocity(s)
    assert torch.equal(_bits(ops.advect_stream_fwd(d, s)), _bits(ops.advect_fwd(d, vel)))
    assert torch.equal(_bits(ops.advect_stream_bwd(d, s, g)), _bits(ops.advect_bwd(d, vel, g, need_d=False)[1]))


# ---- 2. adjoint kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_adjoint_kernel_is_the_composition_bit_for_bit(shape):
    from neural_flow_style_amd import ops
    d, s, g = _case(shape)
    want = ops.advect_bwd(d, ops.stream_velocity(s), g, need_d=False)[1]
    a, b = ops.advect_stream_bwd(d, s, g), ops.advect_stream_bwd(d, s, g)
    assert torch.equal(_bits(a), _bits(want)) and torch.equal(_bits(a), _bits(b))
    assert float(a.abs().max()) > 0


# ---- 3. update kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 2), (1, 4, 3), (4, 1, 1), (5, 6, 7), (9, 12, 10)])
def test_update_kernel_gathers_the_transpose_and_applies_adam(shape):
    """first step from zero moments: m = fl(fl(1 - b1) g_s) and v = fl(fl(fl(1 - b2) g_s) g_s) are chains of single
    roundings whichever way the compiler contracts b m + (1 - b) g with m = 0, so their bits pin the gather; m / (1 - b1)
    against the float64 transpose within 16 * 2^-23 * A (at most eight terms summed, two roundings from the factor; A = the
    all-positive transpose of |g|); three further steps against curl_bwd + adam_tf_step to the fused-vs-unfused bar of
    tests/test_engine_gpu.py (rel-L2 < 1e-6)"""
    from neural_flow_style_amd import ops
    rng = np.random.RandomState(sum(shape))
    s0 = torch.tensor(SR.make_psi(shape, 1.0, seed=5)).cuda()
    g_np = rng.randn(*shape, 3).astype(np.float32)
    g = torch.tensor(g_np).cuda()
    g_s = ops.stream_velocity_bwd(g)
    s, m, v = s0.clone(), torch.zeros_like(s0), torch.zeros_like(s0)
    ops.stream_bwd_adam(g, s, m, v, 1e-3, B1, B2, EPS)
    one_b1 = torch.tensor(np.float32(1) - np.float32(B1)).cuda()
    one_b2 = torch.tensor(np.float32(1) - np.float32(B2)).cuda()
    assert torch.equal(_bits(m), _bits(one_b1 * g_s))
    assert torch.equal(_bits(v), _bits((one_b2 * g_s) * g_s))
    got = m.double().cpu().numpy() / float(np.float32(1) - np.float32(B1))
    want = SR.velocity_T(g_np.astype(np.float64))
    A = SR.velocity_T(g_np.astype(np.float64), absolute=True)
    err = np.abs(got - want)
    print("update %-12s first step: max |m/(1-b1) - transpose| %.3e, worst err/bound %.3f" % (
        shape, err.max(), float((err / np.maximum(16 * 2.0 ** -23 * A, 1e-300)).max()) if A.max() > 0 else 0.0))
    assert (err <= 16 * 2.0 ** -23 * A).all()
    # the unfused pair from the same start, then three further steps with fresh gradients
    s_u, m_u, v_u = s0.clone(), torch.zeros_like(s0), torch.zeros_like(s0)
    ops.adam_tf_step(s_u, m_u, v_u, g_s, 1e-3, B1, B2, EPS)
    for k in range(3):
        gk = torch.tensor(rng.randn(*shape, 3).astype(np.float32)).cuda()
        ops.stream_bwd_adam(gk, s, m, v, 1e-3, B1, B2, EPS)
        ops.adam_tf_step(s_u, m_u, v_u, ops.curl_bwd(gk.flip(-1).contiguous()), 1e-3, B1, B2, EPS)
    for name, a, b in (("psi", s, s_u), ("m", m, m_u), ("v", v, v_u)):
        ulp = int((_bits(a).long() - _bits(b).long()).abs().max())
        print("update %-12s %-3s after 4 steps: rel-L2 %.2e, largest difference %d ulp" % (shape, name, rel(a, b), ulp))
        assert rel(a, b) < 1e-6
    assert float((s - s0).abs().max()) > 0


# ---- 4 - 6. the stylizer ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engine_case(n_layers, V=3, G=24, cells=0.5):
    """computed once per layer set and shared (read only): density, psi at ``cells`` cells, views, loss, oracle pieces"""
    from tests.test_engine_gpu import _setup
    layers = LAYERS5[:n_layers]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, layers)
    psi = SR.make_psi((G, G, G), cells, seed=11)
    return d0, psi, mats, loss, cfg, w_or, sfe, T, eng


def _stylizer(eng, loss, d0, var, target="s", **kw):
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target=target, **kw)
    gs.var.copy_(torch.as_tensor(var))
    return gs


def test_gradient_parity_with_the_oracle_chain():
    """24^3, 3 views, conv1_1..conv5_1, psi at 0.5 cell: gradient() against autograd through O.curl(s).flip(-1) ->
    O.grid_forward; the bars of test_gradient_parity_grid_velocity"""
    from neural_flow_style_amd import ops
    G, V = 24, 3
    d0, psi, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(5, V, G)
    s_o = torch.tensor(psi)[None].requires_grad_()
    vel_o = O.curl(s_o, False).flip(-1)
    rot_o = torch.tensor(np.asarray(mats, np.float32))
    total, per_view, d_out = O.grid_forward(torch.tensor(d0)[None, ..., None], vel_o, rot_o, cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, s_o)
    rot = T.rot_to_device(mats, "cuda")
    gs = _stylizer(eng, loss, d0, psi)
    losses, g_h = gs.gradient(rot)
    print("stream gradient: d_s rel %.2e, losses rel %.2e, gradient rel %.2e" % (
        rel(gs.d_s, d_out[0, ..., 0]), rel(losses, torch.stack(per_view)), rel(g_h, g_o[0])))
    assert rel(gs.d_s, d_out[0, ..., 0]) < 1e-5
    assert rel(losses, torch.stack(per_view)) < 1e-4
    assert rel(g_h, g_o[0]) < 1e-3
    assert torch.equal(gs.velocity(), ops.stream_velocity(gs.var))
    # ... and not the velocity variable's gradient at the same velocity handed through
    gv = _stylizer(eng, loss, d0, gs.velocity(), target="v")
    _, g_vel = gv.gradient(rot)
    assert tuple(g_h.shape) == (G, G, G, 3) == tuple(g_vel.shape)
    assert rel(g_h, g_vel) > 1e-2
    assert rel(g_h, ops.stream_velocity_bwd(g_vel)) < 1e-5


def _masked_steps(eng, loss, d0, psi, rot, skip, n=4):
    gs = _stylizer(eng, loss, d0, psi, lr=1e-3, graph=False)
    gs.dead_skip = skip
    gs.step(rot)
    taken = bool(gs._live_kw())
    for _ in range(n - 1):
        gs.step(rot)
    return gs, taken


def _step_case():
    d0, psi, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(3)
    return psi, T.rot_to_device(mats, "cuda"), (lambda **kw: _stylizer(eng, loss, d0, psi, lr=1e-3, **kw))


@functools.lru_cache(maxsize=None)
def _eager_steps():
    """five eager steps from the shared start: (losses, the stylizer) -- read only"""
    psi, rot, make = _step_case()
    a = make(graph=False)
    return [float(a.step(rot)) for _ in range(5)], a


def test_step_is_adam_on_the_gradient_and_lowers_the_loss():
    from neural_flow_style_amd import ops
    psi, rot, make = _step_case()
    a, b = make(graph=False), make(graph=False)
    assert a.slab is None and a._adv_target() is not None and not a._fused_step_ok()
    first = float(a.step(rot))
    _, g = b.gradient(rot)
    b.adam.step(b.var, g, b.lr)
    for x, y in ((a.var, b.var), (a.adam.m, b.adam.m), (a.adam.v, b.adam.v)):
        assert rel(x, y) < 1e-6
    assert float((a.var - torch.tensor(psi).cuda()).abs().max()) > 0
    # the stored forward sample is that of the updated variable
    assert a._adv_valid() and torch.equal(a._adv_buf, ops.advect_fwd(a.d0.unsqueeze(-1), a.velocity()).squeeze(-1))
    ls, _ = _eager_steps()
    print("stream-function steps, loss:", ls)
    assert abs(ls[0] - first) <= 1e-6 * abs(first) and ls[4] < ls[0]
    # L-BFGS only needs gradient(): two finite steps
    lb = make(graph=False, optimizer="lbfgs")
    assert np.isfinite(float(lb.step(rot))) and np.isfinite(float(lb.step(rot)))
    assert float((lb.var - torch.tensor(psi).cuda()).abs().max()) > 0


def test_graph_replay_reads_the_moved_variable_and_follows_the_eager_steps():
    """warm, capture, then move psi in place: the replayed gradient is that of the new variable; whole steps through the
    graph follow the eager trajectory"""
    psi, rot, make = _step_case()
    ls, a = _eager_steps()
    c = make(graph=True)
    for _ in range(2):
        c._field_gradient_graphed(rot)
    assert c._graph is not None
    psi1 = a.var.clone()
    c.var.copy_(psi1)
    _, g_ds = c._field_gradient_graphed(rot)
    g_replay = c.variable_gradient(g_ds)
    e = make(graph=False)
    e.var.copy_(psi1)
    _, g_eager = e.gradient(rot)
    assert rel(g_replay, g_eager) < 1e-5
    # whole steps through the graph follow the eager trajectory
    cg = make(graph=True)
    lg = [float(cg.step(rot)) for _ in range(5)]
    assert cg._graph is not None
    np.testing.assert_allclose(lg, ls, rtol=1e-6)
    assert rel(cg.var, a.var) < 1e-6


def test_dead_region_skipping_leaves_every_bit_of_the_update():
    """dead_skip on and off: psi, m and v bit-identical after four steps (g_vel is an exact +-0 at dead voxels, which
    leaves the gathered sums and ApplyAdam unchanged), and the masked path was actually taken"""
    d0, psi, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(3)
    rot = T.rot_to_device(mats, "cuda")
    on, taken_on = _masked_steps(eng, loss, d0, psi, rot, True)
    off, taken_off = _masked_steps(eng, loss, d0, psi, rot, False)
    assert taken_on and not taken_off
    for x, y in ((on.var, off.var), (on.adam.m, off.adam.m), (on.adam.v, off.adam.v)):
        assert torch.equal(_bits(x), _bits(y))


def test_the_flow_stays_divergence_free_and_a_free_velocity_does_not():
    d0, psi, mats, loss, cfg, w_or, sfe, T, eng = _engine_case(3)
    rot = T.rot_to_device(mats, "cuda")
    gs = _stylizer(eng, loss, d0, psi, lr=1e-3, graph=False)
    vel_start = gs.velocity().clone()
    gv = _stylizer(eng, loss, d0, vel_start, target="v", lr=1e-3, graph=False)
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


# ---- 7. order 2 -------------------------------------------------------------------------------------------------------
def test_order_2_runs_through_the_materialised_velocity():
    import neural_flow_style_amd.engine as eng
    import neural_flow_style_amd.transform as T
    import neural_flow_style_amd.vgg as vgg
    from neural_flow_style_amd import ops
    from tests.synth import style_image, uniform_views
    shape = (9, 12, 10)
    rng = np.random.RandomState(3)
    d0 = np.clip(rng.rand(*shape).astype(np.float32) - 0.4, 0, 1)
    psi = SR.make_psi(shape, 0.5, seed=2)
    layers = ["conv1_1", "conv2_1"]
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv2_1"), "cuda")
    loss = eng.RenderStyleLoss(net, layers, [1.0, 1.0], 1.0, transmit=0.05)
    loss.set_style_image(style_image(shape[1], shape[2], rng))
    rot = T.rot_to_device(uniform_views(2), "cuda")
    gs = _stylizer(eng, loss, d0, psi, lr=1e-3, graph=False, adv_order=2)
    assert gs._adv_target() is None and gs._live_target() is None
    _, g = gs.gradient(rot)
    vel = ops.stream_velocity(gs.var)
    assert torch.equal(_bits(gs._mc_vel), _bits(vel))
    g_adv = ops.smooth3d_relu_bwd(gs.d_s, gs.g_ds, gs.k)
    _, g_vel = ops.advect_maccormack_bwd(gs.d0.unsqueeze(-1), vel, gs._mc_fwd, gs._mc_keep, g_adv.unsqueeze(-1),
                                         need_d=False)
    assert torch.equal(_bits(g), _bits(ops.stream_velocity_bwd(g_vel)))
    assert float(g.abs().max()) > 0
    gs1 = _stylizer(eng, loss, d0, psi, lr=1e-3, graph=False)
    assert not torch.equal(gs1.gradient(rot)[1], g)                                 # not the first-order gradient
    assert np.isfinite(float(gs.step(rot)))
    assert float((gs.var - torch.tensor(psi).cuda()).abs().max()) > 0


# ---- 8. two ranks -----------------------------------------------------------------------------------------------------
_RANK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from neural_flow_style_amd import engine, vgg
from neural_flow_style_amd import synthetic as S, transform as T
from tests import stream_ref as SR
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
gs = engine.GridStylizer(loss, torch.tensor(d0, device=dev), k=3, target="s", lr=1e-3,
                         process_group=dist.group.WORLD if world > 1 else None)
assert gs.slab is None
gs.var.copy_(torch.tensor(SR.make_psi((G, G, G), 0.5, seed=11)))
rot = T.rot_to_device(S.uniform_views(V), dev)[rank::world].contiguous()
ls = [float(gs.step(rot)) for _ in range(4)]
np.savez(sys.argv[1] + ".%%d.npz" %% rank, l=np.asarray(ls), var=gs.var.cpu().numpy())
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


def test_two_ranks_sharing_the_views_keep_bit_identical_replicas(tmp_path):
    """views sharded over two gloo ranks in the all-reduce mode (the stream function has no slab form): after four steps
    both replicas of psi are bit-identical -- every rank repeats deterministic field work on the summed density gradient
    -- and the first loss is the one-rank run's to rtol 2e-6"""
    from tests.ranks import require_gpus_for, run_ranks
    require_gpus_for(2)
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NFS_SLAB_SHARD"):
        env.pop(k, None)
    subprocess.run([sys.executable, str(script), str(tmp_path / "one")], check=True, env=env, timeout=600)
    run_ranks([sys.executable, str(script), str(tmp_path / "two")], 2, env, timeout=900)
    one = np.load(str(tmp_path / "one") + ".0.npz")
    r0, r1 = (np.load(str(tmp_path / "two") + ".%d.npz" % r) for r in (0, 1))
    assert np.array_equal(r0["var"].view(np.int32), r1["var"].view(np.int32))
    assert np.array_equal(r0["l"], r1["l"])
    np.testing.assert_allclose(r0["l"][0], one["l"][0], rtol=2e-6)
    print("stream-function losses, one rank:", one["l"], "two ranks:", r0["l"])


# ---- 9. styler_grid ---------------------------------------------------------------------------------------------------
def test_styler_grid_optimises_a_stream_function_per_frame():
    from neural_flow_style_amd import ops
    from neural_flow_style_amd.styler_grid import Styler
    from tests.test_sequence_gpu import _cfg_for, sequence_case, v_init_for
    G, F = 16, 3
    d, u, simg = sequence_case(G, F)
    s_init = [SR.make_psi((G, G, G), 0.5, seed=20 + t) for t in range(F)]
    st = Styler(_cfg_for(G, F, simg, grid_variable="s", iter=4))
    st.load_img([G, G])
    r = st.run({"d": d, "v": u, "s_init": s_init})
    hist = np.asarray(r["l_frames"])
    print("styler_grid grid_variable=s losses per iteration:", hist.sum(1))
    assert hist.shape[0] == 4 and np.isfinite(hist).all() and hist[-1].sum() < hist[0].sum()
    assert len(r["s"]) == len(r["v"]) == len(r["opt"]) == F
    for t in range(F):
        assert np.array_equal(r["s"][t], r["opt"][t]) and not np.array_equal(r["s"][t], s_init[t])
        st_ = torch.tensor(r["s"][t]).cuda()
        vt = ops.stream_velocity(st_)
        assert np.array_equal(r["v"][t], vt.cpu().numpy()), t
        dt = torch.tensor(d[t]).cuda().unsqueeze(-1)
        want = ops.smooth3d_relu_fwd(ops.advect_fwd(dt, torch.tensor(r["v"][t]).cuda()).squeeze(-1).contiguous(), 3.0).abs()
        assert np.array_equal(r["d"][t][..., 0], want.cpu().numpy()), t
    sv = Styler(_cfg_for(G, F, simg, grid_variable="v", iter=4))
    sv.load_img([G, G])
    rv = sv.run({"d": d, "v": u, "v_init": v_init_for(G, F)})
    assert not np.array_equal(rv["v"][0], r["v"][0]) and not np.array_equal(rv["d"][0], r["d"][0])

"""Differentiable MacCormack advection (adv_order = 2) on the GPU: the forward's keep mask, the adjoint element by element
against tests/maccormack_ref.py on the kernel's own decisions, its bit-reproducibility, and the layers above it
(transform.advect, engine.GridStylizer, styler_grid.Styler)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import maccormack_ref as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a = torch.as_tensor(np.asarray(a)).double(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _forward(d, v):
    """(d, v as CUDA tensors, out, d_fwd, keep tensor, keep as a bool array shaped like d)"""
    from neural_flow_style_amd import ops
    dt, vt = torch.tensor(d).cuda(), torch.tensor(v).cuda()
    keep = ops.maccormack_mask(d.shape, dt)
    d_fwd = torch.empty_like(dt)
    out = ops.advect_maccormack(dt, vt, keep=keep, d_fwd=d_fwd)
    kb = MR.unpack_mask(keep.view(torch.int64).cpu().numpy(), d.shape)
    return dt, vt, out, d_fwd, keep, kb


@pytest.mark.parametrize("case", MR.CASES, ids=lambda c: c[0])
def test_forward_with_mask_is_the_plain_forward_and_the_mask_is_the_float64_decision(case):
    """out with the mask == out without it, bit for bit; where keep is set out IS d_fwd; on the voxels the float64
    scheme calls settled (test_grid_ops_gpu's rule) keep is the float64 decision"""
    from neural_flow_style_amd import ops
    from tests.test_grid_ops_gpu import _maccormack_f64
    d, v, _ = MR.make_case(case)
    dt, vt, out, d_fwd, keep, kb = _forward(d, v)
    plain = ops.advect_maccormack(dt, vt)
    assert torch.equal(_bits(out), _bits(plain))
    k = torch.tensor(kb).cuda()
    assert torch.equal(_bits(out)[k], _bits(d_fwd)[k])
    # no bit set beyond the field
    words = keep.view(torch.int64).cpu().numpy().view(np.uint64)
    n = d.size
    assert not words[(n + 63) // 64:].any() and (n % 64 == 0 or words[n // 64] >> np.uint64(n % 64) == 0)
    _, d_adv, lo, hi, tol, cell_sure = _maccormack_f64(d, v)
    margin = 2 * tol
    settled = (np.abs(d_adv - lo) > margin) & (np.abs(d_adv - hi) > margin) & cell_sure[..., None]
    want = (d_adv > hi) | (d_adv < lo)
    bad = settled & (kb != want)
    print("keep %-14s fires on %.1f %%, settled %.2f %%" % (case[0], 100 * kb.mean(), 100 * settled.mean()))
    assert not bad.any(), (case[0], np.argwhere(bad)[:4])
    if case[3] == "random":
        assert settled.mean() >= 0.99


def _gradients(rng, shape):
    hot = np.zeros(shape, np.float32)
    hot[(-1,) * (len(shape) - 1) + (0,)] = 1.5                       # a corner voxel: its stencils clamp
    return (("randn", rng.randn(*shape).astype(np.float32)), ("ones", np.ones(shape, np.float32)), ("one-hot", hot))


@pytest.mark.parametrize("case", MR.CASES, ids=lambda c: c[0])
def test_adjoint_every_element_within_the_derived_bound_of_the_float64_adjoint(case):
    """g_d and g_vel from the kernel's own keep and d_fwd against tests/maccormack_ref.adjoint, every element, no
    exemptions: g_d within bound_d; each component of g_vel within bound_vel of a candidate (one and the same value
    except within 1e-4 cells of a cell face).  g in {randn, ones, one-hot at a corner}; both gradients together (g_d
    accumulated onto what its buffer held) and each alone"""
    from neural_flow_style_amd import ops
    d, v, rng = MR.make_case(case)
    dt, vt, out, d_fwd, keep, kb = _forward(d, v)
    F = d_fwd.cpu().numpy()
    for gname, g in _gradients(rng, d.shape):
        gt = torch.tensor(g).cuda()
        init = rng.randn(*d.shape).astype(np.float32)
        ref_i = MR.adjoint(d, v, F, kb, g, init_d=init)
        ref_0 = MR.adjoint(d, v, F, kb, g)
        acc = torch.tensor(init).cuda()
        gd_both, gv_both = ops.advect_maccormack_bwd(dt, vt, d_fwd, keep, gt, g_d_acc=acc)
        assert gd_both is acc
        gd_only, none_v = ops.advect_maccormack_bwd(dt, vt, d_fwd, keep, gt, need_vel=False)
        none_d, gv_only = ops.advect_maccormack_bwd(dt, vt, d_fwd, keep, gt, need_d=False)
        assert none_v is None and none_d is None
        for what, got, ref in (("both", gd_both, ref_i), ("alone", gd_only, ref_0)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref["g_d"])
            worst = float((err / np.maximum(ref["bound_d"], 1e-300)).max()) if err.max() > 0 else 0.0
            print("g_d   %-14s %-7s %-5s max err %.2e (max|g_d| %.2e), worst err/bound %.3f" % (
                case[0], gname, what, err.max(), np.abs(ref["g_d"]).max(), worst))
            bad = err > ref["bound_d"]
            assert not bad.any(), (case[0], gname, what, [(tuple(i), err[tuple(i)], ref["bound_d"][tuple(i)])
                                                          for i in np.argwhere(bad)[:4]])
        for what, got in (("both", gv_both), ("alone", gv_only)):
            gv = got.cpu().numpy()
            ex = MR.vel_excess(ref_0, gv)
            err = np.abs(gv - ref_0["g_vel"])
            print("g_vel %-14s %-7s %-5s max err %.2e (max|g_vel| %.2e), unsure voxels %d, worst excess %.2e" % (
                case[0], gname, what, err[~ref_0["unsure"]].max() if (~ref_0["unsure"]).any() else 0.0,
                np.abs(ref_0["g_vel"]).max(), int(ref_0["unsure"].sum()), ex.max()))
            bad = ex > 0
            assert not bad.any(), (case[0], gname, what, [(tuple(i), gv[tuple(i)], ref_0["g_vel"][tuple(i)],
                                                           ref_0["bound_vel"][tuple(i)]) for i in np.argwhere(bad)[:4]])
        assert torch.equal(_bits(gv_both), _bits(gv_only))


@pytest.mark.parametrize("case", MR.CASES, ids=lambda c: c[0])
def test_velocity_gradient_is_bit_identical_from_call_to_call(case):
    """the fixed-point sums make g_vel independent of the order the atomics arrive in: the same bits in every call, with
    the density gradient asked for or not"""
    from neural_flow_style_amd import ops
    d, v, rng = MR.make_case(case)
    dt, vt, out, d_fwd, keep, kb = _forward(d, v)
    gt = torch.tensor(rng.randn(*d.shape).astype(np.float32)).cuda()
    runs = [ops.advect_maccormack_bwd(dt, vt, d_fwd, keep, gt, need_d=nd_)[1] for nd_ in (True, True, False, False)]
    for other in runs[1:]:
        assert torch.equal(_bits(runs[0]), _bits(other))
    assert float(runs[0].abs().max()) > 0


@pytest.mark.parametrize("dims,C", [((9, 12, 10), 1), ((7, 6, 11), 3), ((14, 17), 1), ((13, 9), 3)])
def test_transform_advect_order_2_is_differentiable_and_order_1_unchanged(dims, C):
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import transform as T
    rng = np.random.RandomState(len(dims) * 10 + C)
    nd = len(dims)
    d = rng.randn(1, *dims, C).astype(np.float32)
    v = (rng.uniform(-2, 2, (1,) + dims + (nd,)) * np.asarray([2.0 / (n - 1) for n in dims])).astype(np.float32)
    w = torch.tensor(rng.randn(1, *dims, C).astype(np.float32)).cuda()
    dh, vh = torch.tensor(d).cuda().requires_grad_(), torch.tensor(v).cuda().requires_grad_()
    out = T.advect(dh, vh, order=2, is_3d=nd == 3)
    assert out.requires_grad
    (out * w).sum().backward()
    dt, vt, out2, d_fwd, keep, _ = _forward(d[0], v[0])
    assert torch.equal(_bits(out[0]), _bits(out2))
    gd, gv = ops.advect_maccormack_bwd(dt, vt, d_fwd, keep, w[0].contiguous())
    assert torch.equal(_bits(vh.grad[0]), _bits(gv))
    assert rel(dh.grad[0].cpu(), gd.cpu()) < 1e-6                                  # (float atomics: not bit for bit)
    # only what asks for a gradient gets one
    v2 = torch.tensor(v).cuda().requires_grad_()
    (T.advect(torch.tensor(d).cuda(), v2, order=2, is_3d=nd == 3) * w).sum().backward()
    assert torch.equal(_bits(v2.grad), _bits(vh.grad))
    # order 1: as before
    d1, v1 = torch.tensor(d).cuda().requires_grad_(), torch.tensor(v).cuda().requires_grad_()
    o1 = T.advect(d1, v1, order=1, is_3d=nd == 3)
    (o1 * w).sum().backward()
    bwd1 = ops.advect_bwd if nd == 3 else ops.advect2d_bwd
    gd1, gv1 = bwd1(torch.tensor(d[0]).cuda(), torch.tensor(v[0]).cuda(), w[0].contiguous())
    assert torch.equal(_bits(v1.grad[0]), _bits(gv1)) and rel(d1.grad[0].cpu(), gd1.cpu()) < 1e-6
    assert not torch.equal(o1, out)


LAYERS5 = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]


def _oracle_order2(d0, vel_o, keep):
    """the oracle's MacCormack pieces with ``keep`` imposed: where(keep, F, A) [1,D,H,W,1], and the oracle's own
    float32 decisions"""
    d0_o = torch.tensor(d0)[None, ..., None]
    D, H, W = d0.shape
    g = O.mgrid(D, H, W).unsqueeze(0)
    vp = vel_o.permute(0, 4, 1, 2, 3)
    F = O.batch_warp3d(d0_o, g - vp, [1, D, H, W])
    B = O.batch_warp3d(F, g + vp, [1, D, H, W])
    A = F + (d0_o - B) * 0.5
    lo, hi = O._stencil_extrema(d0_o, (g - vp).detach())
    own = ((A > hi) | (lo > A)).detach()
    return torch.where(torch.tensor(keep)[None, ..., None], F, A), own


def test_grid_stylizer_order_2_gradient_matches_the_oracle_chain_on_the_engines_own_mask():
    """24^3, 3 views, conv1_1..conv5_1, non-zero initial velocity: GridStylizer(adv_order=2).gradient() against
    smooth3d_relu -> grid_view_loss fed with where(keep, F, A) from the oracle's advect pieces, keep = the engine's
    mask.  Bars of test_gradient_parity_grid_velocity.  The decisions that differ from the float32 oracle's
    own are reported: they sit where both branches agree to rounding"""
    from tests.test_engine_gpu import _setup
    from tests.test_engine_gpu import rel as rel_t
    G, V = 24, 3
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, LAYERS5)
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", adv_order=2)
    gs.var.copy_(torch.tensor(vel0))
    losses, g_h = gs.gradient(T.rot_to_device(mats, "cuda"))
    keep = MR.unpack_mask(gs._mc_keep.view(torch.int64).cpu().numpy(), (G, G, G))
    vel_o = torch.tensor(vel0)[None].requires_grad_()
    adv, own = _oracle_order2(d0, vel_o, keep)
    d_out = O.smooth3d_relu(adv, cfg["k"])
    rot_o = torch.tensor(np.asarray(mats, np.float32))
    per_view = [O.grid_view_loss(d_out, rot_o[v:v + 1], cfg, w_or, sfe) for v in range(V)]
    (g_o,) = torch.autograd.grad(sum(per_view), vel_o)
    differ = int((own[0, ..., 0].numpy() != keep).sum())
    print("order-2 engine: limiter fires on %.1f %% of %d voxels; %d decisions differ from the float32 oracle's own; "
          "d_s rel %.2e, losses rel %.2e, gradient rel %.2e" % (
              100 * keep.mean(), keep.size, differ, rel_t(gs.d_s, d_out[0, ..., 0]), rel_t(losses, torch.stack(per_view)),
              rel_t(g_h, g_o[0])))
    assert rel_t(gs.d_s, d_out[0, ..., 0]) < 1e-5
    assert rel_t(losses, torch.stack(per_view)) < 1e-4
    assert rel_t(g_h, g_o[0]) < 1e-3
    # and it is not the first-order gradient
    gs1 = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v")
    gs1.var.copy_(torch.tensor(vel0))
    _, g_1 = gs1.gradient(T.rot_to_device(mats, "cuda"))
    assert rel_t(g_h, g_1) > 1e-2


def test_grid_stylizer_order_2_step_is_adam_on_its_gradient_and_graph_replay_feeds_the_adjoint():
    from tests.test_engine_gpu import _setup
    from tests.test_engine_gpu import rel as rel_t
    G, V = 24, 3
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, LAYERS5[:3])
    rot = T.rot_to_device(mats, "cuda")

    def make(**kw):
        gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=1e-3, adv_order=2, **kw)
        gs.var.copy_(torch.tensor(vel0))
        return gs
    a, b = make(graph=False), make(graph=False)
    assert not a._fused_step_ok() and a._adv_target() is None and a._live_target() is None and a.slab is None
    first = float(a.step(rot))
    _, g = b.gradient(rot)
    b.adam.step(b.var, g, b.lr)
    assert torch.equal(_bits(a.var), _bits(b.var))
    assert float((a.var - torch.tensor(vel0).cuda()).abs().max()) > 0
    # four steps lower the loss
    ls = [first] + [float(a.step(rot)) for _ in range(4)]
    print("order-2 steps, loss:", ls)
    assert ls[4] < ls[0]
    # the captured forward writes d_fwd and the mask the adjoint outside the capture reads: warm, capture, then replay on
    # ANOTHER variable (moved in place) -- the gradient must be that of the new variable
    c = make(graph=True)
    for _ in range(2):
        c._field_gradient_graphed(rot)
    assert c._graph is not None
    vel1 = a.var.clone()
    c.var.copy_(vel1)
    _, g_ds = c._field_gradient_graphed(rot)
    g_replay = c.variable_gradient(g_ds)
    e = make(graph=False)
    e.var.copy_(vel1)
    _, g_eager = e.gradient(rot)
    assert torch.equal(_bits(c._mc_keep), _bits(e._mc_keep))
    assert rel_t(g_replay, g_eager) < 1e-5
    # L-BFGS only needs gradient(): it runs
    lb = make(graph=False, optimizer="lbfgs")
    l0 = float(lb.step(rot))
    assert np.isfinite(l0) and np.isfinite(float(lb.step(rot)))


_RANK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from neural_flow_style_amd import engine, vgg
from neural_flow_style_amd import synthetic as S, transform as T
world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) %% torch.cuda.device_count())
torch.cuda.set_device(dev)
if world > 1:
    dist.init_process_group("gloo")
G, V = 24, 6
rng = np.random.RandomState(5)
d0 = S.blob_density(G, rng); vel = S.curl_velocity(G, rng, max_cells=1.0)
simg = S.style_image(G, G, rng)
net = vgg.VGG(vgg.synthetic_weights(123, upto="conv3_1"), dev)
loss = engine.RenderStyleLoss(net, ["conv1_1", "conv2_1", "conv3_1"], [1.0] * 3, 1.0, transmit=0.02)
loss.set_style_image(simg)
gs = engine.GridStylizer(loss, torch.tensor(d0, device=dev), k=3, target="v", lr=1e-3, adv_order=2,
                         process_group=dist.group.WORLD if world > 1 else None)
assert gs.slab is None
gs.var.copy_(torch.tensor(vel))
rot = T.rot_to_device(S.uniform_views(V), dev)[rank::world].contiguous()
ls = [float(gs.step(rot)) for _ in range(4)]
np.savez(sys.argv[1] + ".%%d.npz" %% rank, l=np.asarray(ls), var=gs.var.cpu().numpy())
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


def test_two_ranks_sharing_the_views_keep_bit_identical_replicas(tmp_path):
    """views sharded over two gloo ranks, the all-reduce mode (order 2 has no slab form): after four steps the two
    replicas of the variable are bit-identical -- the adjoint every rank repeats on the summed density gradient is
    reproducible -- and the first step's loss is the one-rank run's to rtol 2e-6 (_slab_case's bar for two ranks).
    No multi-step tolerance against the one-rank run is asserted: the limiter is discontinuous in the velocity (where
    it flips, out jumps from A to F), so a last-bit difference between a + b summed on one rank and across two may move
    single voxels by a finite amount a few steps later.  That is the scheme, not an error."""
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
    print("order-2 losses, one rank:", one["l"], "two ranks:", r0["l"])


def test_styler_grid_adv_order_2_optimises_and_finishes_through_maccormack():
    """styler_grid.Styler with adv_order = 2 on a 3-frame 16^3 sequence: it runs, the loss falls, the final density of
    every frame is smooth(MacCormack(d_t, v_t)) of the returned velocity, and the run differs from adv_order = 1"""
    from neural_flow_style_amd import ops
    from neural_flow_style_amd.styler_grid import Styler
    from tests.test_sequence_gpu import _cfg_for, sequence_case, v_init_for
    G, F = 16, 3
    d, u, simg = sequence_case(G, F)
    vi = v_init_for(G, F)
    res = {}
    for order in (2, 1):
        st = Styler(_cfg_for(G, F, simg, adv_order=order, iter=4))
        st.load_img([G, G])
        res[order] = st.run({"d": d, "v": u, "v_init": vi})
    r2 = res[2]
    hist = np.asarray(r2["l_frames"])
    print("styler_grid adv_order=2 losses per iteration:", hist.sum(1))
    assert hist.shape[0] == 4 and np.isfinite(hist).all() and hist[-1].sum() < hist[0].sum()
    for t in range(F):
        dt = torch.tensor(d[t]).cuda().unsqueeze(-1)
        vt = torch.tensor(r2["v"][t]).cuda()
        want = ops.smooth3d_relu_fwd(ops.advect_maccormack(dt, vt).squeeze(-1).contiguous(), 3.0).abs()
        assert np.array_equal(r2["d"][t][..., 0], want.cpu().numpy()), t
        first = ops.smooth3d_relu_fwd(ops.advect_fwd(dt, vt).squeeze(-1).contiguous(), 3.0).abs()
        assert not np.array_equal(r2["d"][t][..., 0], first.cpu().numpy()), t
    assert not np.array_equal(r2["v"][0], res[1]["v"][0])

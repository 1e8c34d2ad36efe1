"""End-to-end parity of the stylisation step (render -> VGG-19 -> Gram loss -> adjoint chain
-> TF-Adam) against the CPU oracle on identical seeded inputs.  Bar (north_star):
relative L2 <= 1e-3 for the field gradient and for the density after K iterations."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests.synth import blob_density, style_image, uniform_views

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _setup(G, V, layers, seed=123, tau=0.05):
    import neural_flow_style_amd.vgg as vgg
    import neural_flow_style_amd.engine as eng
    import neural_flow_style_amd.transform as T
    rng = np.random.RandomState(seed)
    d0 = blob_density(G, rng)
    vel0 = (rng.randn(G, G, G, 3) * 0.3 / (G - 1)).astype(np.float32)   # off-grid start
    mats = uniform_views(V)
    simg = style_image(G, G, rng)
    top = O.last_layer(layers)
    w_np = vgg.synthetic_weights(123, upto=top)
    w_or = O.synthetic_vgg19_weights(123, upto=top)
    for k in w_np:  # the product's weight generator must equal the oracle's
        assert np.array_equal(w_np[k][0], w_or[k][0]) and np.array_equal(w_np[k][1], w_or[k][1])
    net = vgg.VGG(w_np, "cuda")
    loss = eng.RenderStyleLoss(net, layers, [1.0] * len(layers), 1.0, transmit=tau)
    loss.set_style_image(simg)
    cfg = dict(k=3, transmit=tau, style_layer=layers, w_style_layer=[1.0] * len(layers), w_style=1.0, upto=top)
    sfe = O.style_target_features(torch.tensor(simg)[None], w_or, layers, upto=top)
    return d0, vel0, mats, loss, cfg, w_or, sfe, T, eng


@pytest.mark.parametrize("G,V,layers", [(24, 3, ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]),
                                        (32, 2, ["conv2_1", "conv3_1"])])
def test_gradient_parity_grid_velocity(G, V, layers):
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, layers)
    d0_o = torch.tensor(d0)[None, ..., None]
    vel_o = torch.tensor(vel0)[None].requires_grad_()
    rot_o = torch.tensor(np.asarray(mats, np.float32))
    total, per_view, d_out = O.grid_forward(d0_o, vel_o, rot_o, cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, vel_o)

    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v")
    gs.var.copy_(torch.tensor(vel0))
    losses, g_h = gs.gradient(T.rot_to_device(mats, "cuda"))
    assert rel(gs.d_s, d_out[0, ..., 0]) < 1e-5
    lo = torch.stack(per_view)
    assert rel(losses, lo) < 1e-4
    assert rel(g_h, g_o[0]) < 1e-3


def test_gradient_parity_density_variable_and_liquid():
    G, V = 20, 2
    layers = ["conv1_1", "conv2_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, layers, tau=0.2)
    loss.liquid = True
    cfg["render_liquid"] = True
    d_o = torch.tensor(d0)[None, ..., None].requires_grad_()
    rot_o = torch.tensor(np.asarray(mats, np.float32))
    total, per_view, _ = O.grid_forward(d_o, None, rot_o, cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, d_o)
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="d")
    losses, g_h = gs.gradient(T.rot_to_device(mats, "cuda"))
    assert rel(losses, torch.stack(per_view)) < 1e-4
    assert rel(g_h, g_o[0, ..., 0]) < 1e-3


def test_adam_trajectory_parity():
    G, V, K = 24, 2, 4
    layers = ["conv1_1", "conv2_1", "conv3_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, layers)
    lr = 0.002
    d0_o = torch.tensor(d0)[None, ..., None]
    vel_o = torch.tensor(vel0)[None]
    rot_o = torch.tensor(np.asarray(mats, np.float32))
    opt = O.TFAdam()
    lo = []
    for _ in range(K):
        v = vel_o.clone().requires_grad_()
        total, _, _ = O.grid_forward(d0_o, v, rot_o, cfg, w_or, sfe)
        (g,) = torch.autograd.grad(total, v)
        vel_o = opt.step(vel_o, g, lr)
        lo.append(float(total))
    d_fin_o = O.smooth3d_relu(O.advect(d0_o, vel_o), 3)[0, ..., 0]

    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=lr)
    gs.var.copy_(torch.tensor(vel0))
    rot = T.rot_to_device(mats, "cuda")
    lh = [float(gs.step(rot)) for _ in range(K)]
    np.testing.assert_allclose(lh, lo, rtol=2e-3)
    assert lh[-1] < lh[0]
    assert rel(gs.forward_field(), d_fin_o) < 1e-3


def test_view_groups_on_streams_match_single_batch():
    """concurrency modes (NFS_VIEW_GROUPS / NFS_VGG_STREAMS / NFS_GRAM_STREAM): view groups on separate HIP
    streams and the Gram work on a side stream must give the same losses and field gradient as one batch on
    one stream"""
    layers = ["conv1_1", "conv2_1", "conv3_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(24, 4, layers)
    rot = T.rot_to_device(mats, "cuda")
    res = []
    # (the default: one batch, the Gram work of all style layers grouped after the forward pass; then the per-layer
    # chain on the main stream / on a side stream, with and without view groups)
    for grouped, groups, streams, side in ((True, 1, 1, False), (False, 1, 1, False), (False, 2, 2, True),
                                           (False, 2, 1, True), (False, 1, 1, True), (True, 2, 2, False)):
        loss.gram_grouped = grouped
        loss.view_groups, loss.vgg_streams, loss.gram_side_stream = groups, streams, side
        gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v")
        gs.var.copy_(torch.tensor(vel0))
        losses, g = gs.gradient(rot)
        torch.cuda.synchronize()
        res.append((losses.clone(), g.clone()))
    for losses, g in res[1:]:
        assert rel(losses, res[0][0]) < 1e-5
        assert rel(g, res[0][1]) < 1e-5


def test_fused_advect_adam_equals_separate_kernels():
    """GridStylizer.step with the velocity gradient consumed inside the Adam kernel (default) follows the same
    trajectory as advect_bwd + adam_tf_step"""
    layers = ["conv1_1", "conv2_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(24, 2, layers)
    rot = T.rot_to_device(mats, "cuda")
    out = []
    for fuse in (True, False):
        gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=1e-3)
        gs.fuse_adam = fuse
        gs.var.copy_(torch.tensor(vel0))
        ls = [float(gs.step(rot)) for _ in range(4)]
        out.append((ls, gs.var.clone(), gs.adam.m.clone(), gs.adam.v.clone()))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-6)
    for a, b in zip(out[0][1:], out[1][1:]):
        assert rel(a, b) < 1e-6



@pytest.mark.parametrize("graph", [False, True])
def test_next_forward_advect_inside_the_adam_kernel_is_bit_identical(graph):
    """The Adam kernel of iteration i also writes advect(d0, updated velocity), iteration i + 1's forward sample
    (nfs_advect_bwd_adam_fwd): same trajectory, bit for bit, as running the forward advect by itself (NFS_FUSE_ADVECT=0
    semantics); a variable changed by hand, a re-bound frame or a changed density make the stored sample stale."""
    layers = ["conv1_1", "conv2_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(24, 2, layers)
    rot = T.rot_to_device(mats, "cuda")
    out = []
    for fuse in (True, False):
        gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=1e-3, graph=graph)
        gs.fuse_advect = fuse
        gs.var.copy_(torch.tensor(vel0))
        ls = [float(gs.step(rot)) for _ in range(4)]
        assert (gs._adv_buf is not None and gs._adv_valid()) == fuse
        if fuse:    # the stored sample IS the forward advect of the current variable
            assert torch.equal(gs._adv_buf, ops_mod().advect_fwd(gs.d0.unsqueeze(-1), gs.var).squeeze(-1))
        gs.var.mul_(0.5)                                            # by hand: the stored sample is stale now
        assert not gs._adv_valid()
        ls += [float(gs.step(rot)) for _ in range(2)]
        gs.d0.mul_(0.9)                                             # the density it gathers from changed
        assert not gs._adv_valid()
        ls += [float(gs.step(rot)) for _ in range(2)]
        out.append((ls, gs.var.clone(), gs.adam.m.clone(), gs.adam.v.clone(), gs.d_s.clone()))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert torch.equal(a, b)


def ops_mod():
    import neural_flow_style_amd.ops as o
    return o


@pytest.mark.parametrize("graph", [False, True])
def test_stored_forward_advect_never_goes_stale_on_shapes_the_fused_kernel_refuses(graph):
    """9 x 10 x 11 cells (990: not a multiple of 4) cannot take the fused advect-adjoint + Adam kernel: step() updates the
    velocity through TFAdamState.step, which writes no next forward sample -- so none may be kept (round-4 advisor find:
    the stylizer kept advect(d0, OLD velocity) and optimised against a frozen density from step 2 on).  Same trajectory
    with the switch on and off; an external raw-pointer Adam step on gs.var is seen through the version counter."""
    import neural_flow_style_amd.vgg as vgg
    import neural_flow_style_amd.engine as eng
    import neural_flow_style_amd.transform as T
    D, H, W = 9, 10, 11
    rng = np.random.RandomState(3)
    d0 = np.clip(rng.rand(D, H, W).astype(np.float32) - 0.4, 0, 1)
    vel0 = (rng.randn(D, H, W, 3) * 0.05).astype(np.float32)
    layers = ["conv1_1", "conv2_1"]
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv2_1"), "cuda")
    loss = eng.RenderStyleLoss(net, layers, [1.0, 1.0], 1.0, transmit=0.05)
    loss.set_style_image(style_image(H, W, rng))
    rot = T.rot_to_device(uniform_views(2), "cuda")
    out = []
    for fuse in (True, False):
        gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=5e-3, graph=graph)
        gs.fuse_advect = fuse
        assert not gs._fused_step_ok() and gs._adv_target() is None
        gs.var.copy_(torch.tensor(vel0))
        ls = [float(gs.step(rot)) for _ in range(4)]
        assert not gs._adv_valid()
        out.append((ls, gs.var.clone(), gs.d_s.clone()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    assert len(set(out[0][0])) == 4                                 # the density the loss sees does move
    # a fusable shape, updated from OUTSIDE through the raw-pointer Adam kernel: the stored sample is dropped
    d0c, vel0c, mats, lossc, cfg, w_or, sfe, T, eng = _setup(24, 2, layers)
    gs = eng.GridStylizer(lossc, torch.tensor(d0c).cuda(), k=3, target="v", lr=1e-3, graph=graph)
    gs.var.copy_(torch.tensor(vel0c))
    rotc = T.rot_to_device(mats, "cuda")
    for _ in range(3):
        gs.step(rotc)
    assert gs._adv_valid()
    _, g = gs.gradient(rotc)
    eng.TFAdamState().step(gs.var, g.contiguous(), 1e-2)
    assert not gs._adv_valid()
    d_ref = ops_mod().smooth3d_relu_fwd(ops_mod().advect_fwd(gs.d0.unsqueeze(-1), gs.var).squeeze(-1), 3.0)
    assert torch.equal(gs.forward_field(), d_ref)                   # the forward follows the externally updated variable
    assert np.isfinite(float(gs.step(rotc))) and gs._adv_valid()


def test_graph_replay_equals_eager_steps():
    """GridStylizer(graph=True): forward + adjoint replayed as one hipGraph (eager warm-up step, capture, replays)
    follows the eager trajectory; a different view tensor is copied into the captured buffer."""
    layers = ["conv1_1", "conv2_1", "conv3_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(24, 3, layers)
    rot = T.rot_to_device(mats, "cuda")
    out = []
    for graph in (False, True):
        gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=1e-3, graph=graph)
        gs.var.copy_(torch.tensor(vel0))
        ls = [float(gs.step(rot)) for _ in range(5)]
        ls.append(float(gs.step(rot.clone())))                      # not the captured tensor: copied in
        assert (gs._graph is not None) == graph
        out.append((ls, gs.var.clone(), gs.adam.m.clone(), gs.adam.v.clone()))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-6)
    for a, b in zip(out[0][1:], out[1][1:]):
        assert rel(a, b) < 1e-6


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_gradient_parity_with_max_and_mean_ray_modes(mode):
    """north_star's per-ray max / mean render (reduce_max -- the line the reference keeps commented out, styler_3p.py:149
    -- and reduce_mean along the ray, un-normalised) through the whole chain: rotate -> ray reduction -> VGG -> Gram
    losses and the adjoint back to the velocity variable, vs the oracle; the max gradient goes to the arg-max cells"""
    G, V = 24, 3
    layers = ["conv1_1", "conv2_1", "conv3_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, layers)
    loss = eng.RenderStyleLoss(loss.net, layers, [1.0] * 3, 1.0, transmit=cfg["transmit"], ray_mode=mode)
    simg = style_image(G, G, np.random.RandomState(123 + 1))
    loss.set_style_image(simg)
    sfe = O.style_target_features(torch.tensor(simg)[None], w_or, layers, upto=cfg["upto"])
    cfg = dict(cfg, ray_mode=mode)
    d0_o = torch.tensor(d0)[None, ..., None]
    vel_o = torch.tensor(vel0)[None].requires_grad_()
    total, per_view, _ = O.grid_forward(d0_o, vel_o, torch.tensor(np.asarray(mats, np.float32)), cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, vel_o)
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v")
    gs.var.copy_(torch.tensor(vel0))
    losses, g_h = gs.gradient(T.rot_to_device(mats, "cuda"))
    assert rel(losses, torch.stack(per_view)) < 1e-4
    assert rel(g_h, g_o[0]) < 1e-3
    # and the step runs (two-pass adjoint on the kept rotated volume)
    assert np.isfinite(float(gs.step(T.rot_to_device(mats, "cuda"))))


def test_graph_replay_with_large_images_uses_no_memset_nodes():
    """a captured step whose render is >= 16384 pixels per normalisation group (the multi-block max-normalisation with
    its -inf initialisation and float atomics, fused with the loss-net input): the replayed trajectory must equal the
    eager one -- as a memset NODE of the hipGraph that initialisation ran out of order with the atomics behind it"""
    import neural_flow_style_amd.vgg as vgg
    import neural_flow_style_amd.engine as eng
    import neural_flow_style_amd.transform as T
    rng = np.random.RandomState(3)
    D, H = 8, 136
    d0 = blob_density(H, rng)[H // 2 - D // 2: H // 2 + D // 2].copy()          # [8,136,136]
    vel0 = (rng.randn(D, H, H, 3) * 0.3 / (H - 1)).astype(np.float32)
    simg = style_image(H, H, rng)
    layers = ["conv1_1", "conv2_1"]
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv2_1"), "cuda")
    rot = T.rot_to_device(uniform_views(2), "cuda")
    out = []
    for graph in (False, True):
        loss = eng.RenderStyleLoss(net, layers, [1.0, 1.0], 1.0, transmit=0.05)
        loss.set_style_image(simg)
        gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=1e-3, graph=graph)
        gs.var.copy_(torch.tensor(vel0))
        ls = [float(gs.step(rot)) for _ in range(6)]
        assert (gs._graph is not None) == graph
        out.append((ls, gs.var.clone()))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-6)
    assert rel(out[0][1], out[1][1]) < 1e-6


@pytest.mark.parametrize("variant", ["channel", "all", "image", "content_only"])
def test_gradient_parity_with_content_loss(variant):
    """the content term of _loss (styler_base.py:135-150) on a VGG layer, added to the style loss:
    channel maximisation, -mean(feature), distance to a content image's features; and alone on a layer above the
    style layers (the gradient then enters the adjoint chain at the content layer only)."""
    import neural_flow_style_amd.vgg as vgg
    G, V = 24, 2
    layers = ["conv1_1", "conv2_1"]
    clayer = "conv3_1" if variant == "content_only" else "conv2_1"
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, layers + (["conv3_1"] if variant == "content_only" else []))
    net = loss.net
    w_content = 3.0e4                                   # comparable to the style term for this synthetic network
    kw = dict(w_content=w_content, content_layer=clayer, content_channel=0 if variant == "all" else 37,
              w_content_amp=1.5)
    loss = eng.RenderStyleLoss(net, layers, [1.0] * len(layers), 1.0, transmit=cfg["transmit"], **kw)
    simg = style_image(G, G, np.random.RandomState(123 + 1))
    loss.set_style_image(simg)
    cfg = dict(cfg, style_layer=layers, w_style_layer=[1.0] * len(layers), upto=O.last_layer(layers + [clayer]), **kw)
    sfe = O.style_target_features(torch.tensor(simg)[None], w_or, layers, upto=cfg["upto"])
    if variant == "image":
        cimg = style_image(G, G, np.random.RandomState(7))
        cf = loss.set_content_image(cimg)
        cfg["content_feature"] = O.vgg19_features(torch.tensor(cimg)[None], w_or, clayer)[clayer].detach()
        assert rel(cf, cfg["content_feature"]) < 1e-5
    d0_o = torch.tensor(d0)[None, ..., None]
    vel_o = torch.tensor(vel0)[None].requires_grad_()
    rot_o = torch.tensor(np.asarray(mats, np.float32))
    total, per_view, _ = O.grid_forward(d0_o, vel_o, rot_o, cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, vel_o)
    # the content term must matter in this comparison
    cfg0 = dict(cfg, w_content=0)
    total0, _, _ = O.grid_forward(d0_o, vel_o, rot_o, cfg0, w_or, sfe)
    assert abs(float(total.detach() - total0.detach())) > 1e-2 * abs(float(total0.detach()))
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v")
    gs.var.copy_(torch.tensor(vel0))
    losses, g_h = gs.gradient(T.rot_to_device(mats, "cuda"))
    assert rel(losses, torch.stack(per_view)) < 1e-4
    assert rel(g_h, g_o[0]) < 1e-3


@pytest.mark.parametrize("dims", [(20, 28, 36), (18, 25, 27)])
def test_gradient_parity_non_cubic_grid(dims):
    """D != H != W (and a non-square image through the loss network): every tile / wave mapping on the path takes its
    extents from the right axis; odd H, W: VALID pools floor, ragged Winograd tiles and bit-cache words at the edges"""
    import neural_flow_style_amd.vgg as vgg
    import neural_flow_style_amd.engine as eng
    import neural_flow_style_amd.transform as T
    (D, H, W), V = dims, 3
    layers = ["conv1_1", "conv2_1", "conv3_1"]
    rng = np.random.RandomState(77)
    big = blob_density(40, rng)
    d0 = np.ascontiguousarray(big[4:4 + D, 6:6 + H, 2:2 + W])
    vel0 = (rng.randn(D, H, W, 3) * 0.3 / 30).astype(np.float32)
    mats = uniform_views(V)
    simg = style_image(H, W, rng)
    w_np = vgg.synthetic_weights(123, upto="conv3_1")
    w_or = O.synthetic_vgg19_weights(123, upto="conv3_1")
    net = vgg.VGG(w_np, "cuda")
    tau = 0.05
    loss = eng.RenderStyleLoss(net, layers, [1.0] * 3, 1.0, transmit=tau)
    loss.set_style_image(simg)
    cfg = dict(k=3, transmit=tau, style_layer=layers, w_style_layer=[1.0] * 3, w_style=1.0, upto="conv3_1")
    sfe = O.style_target_features(torch.tensor(simg)[None], w_or, layers, upto="conv3_1")
    d0_o = torch.tensor(d0)[None, ..., None]
    vel_o = torch.tensor(vel0)[None].requires_grad_()
    rot_o = torch.tensor(np.asarray(mats, np.float32))
    total, per_view, d_out = O.grid_forward(d0_o, vel_o, rot_o, cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, vel_o)
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v")
    gs.var.copy_(torch.tensor(vel0))
    losses, g_h = gs.gradient(T.rot_to_device(mats, "cuda"))
    assert rel(gs.d_s, d_out[0, ..., 0]) < 1e-5
    assert rel(losses, torch.stack(per_view)) < 1e-4
    assert rel(g_h, g_o[0]) < 1e-3


def test_gradient_parity_at_real_vgg_dynamic_range():
    """f32 Winograd F(4x4,3x3) at the dynamic range of the REAL vgg_19 checkpoint (which cannot be loaded here):
    conv1_1 filters of O(0.5) on 0..255 inputs and biases of O(1) give activations of O(10^2..10^3) through the net --
    the seeded filters are rescaled to reach that range.  Reference = the oracle in float64 on the same float32
    weights.  Error budget, stated: activations <= 2e-5 relative L2 per style layer (Winograd's interpolation points
    0, +-1, +-2 amplify f32 rounding by ~10x over a direct f32 convolution), field gradient <= 2e-4 -- a factor 5
    inside the 1e-3 bar of the metric."""
    import neural_flow_style_amd.vgg as vgg
    import neural_flow_style_amd.engine as eng
    import neural_flow_style_amd.transform as T
    G, V = 32, 2
    layers = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]
    rng = np.random.RandomState(77)
    d0 = blob_density(G, rng)
    simg = style_image(G, G, rng)
    mats = uniform_views(V)
    w = vgg.synthetic_weights(123, upto="conv5_1")
    w["conv1_1"] = ((w["conv1_1"][0] * 8.0).astype(np.float32), (w["conv1_1"][1] * 100.0).astype(np.float32))
    for k in list(w)[1:]:
        w[k] = (w[k][0], (w[k][1] * 100.0).astype(np.float32))           # biases of O(1)
    net = vgg.VGG(w, "cuda")
    # activations: HIP f32 vs oracle f64
    dimg = torch.tensor(simg)[None]
    fo = O.vgg19_features(dimg.double(), {k: (v[0].astype(np.float64), v[1].astype(np.float64)) for k, v in w.items()},
                          "conv5_1")
    mean = torch.tensor(O.VGG_MEAN, dtype=torch.float32)
    acts = net.forward((dimg - mean).cuda().contiguous(), "conv5_1")
    assert float(fo["conv1_1"].max()) > 500 and float(fo["conv3_1"].max()) > 200
    for name in layers:
        assert rel(acts[name], fo[name]) < 2e-5, name
    # field gradient through render -> VGG -> Gram -> adjoints
    loss = eng.RenderStyleLoss(net, layers, [1.0] * 5, 1.0, transmit=0.05)
    loss.set_style_image(simg)
    cfg = dict(k=3, transmit=0.05, style_layer=layers, w_style_layer=[1.0] * 5, w_style=1.0, upto="conv5_1")
    w64 = {k: (v[0].astype(np.float64), v[1].astype(np.float64)) for k, v in w.items()}
    sfe = O.style_target_features(dimg.double(), w64, layers, upto="conv5_1")
    d_o = torch.tensor(d0, dtype=torch.float64)[None, ..., None].requires_grad_()
    total, per_view, _ = O.grid_forward(d_o, None, torch.tensor(np.asarray(mats, np.float64)), cfg, w64, sfe)
    (g_o,) = torch.autograd.grad(total, d_o)
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="d")
    losses, g_h = gs.gradient(T.rot_to_device(mats, "cuda"))
    assert rel(losses, torch.stack(per_view).detach()) < 1e-4
    assert rel(g_h, g_o[0, ..., 0]) < 2e-4


def test_gradient_parity_with_histogram_loss():
    """style + histogram terms (styler_base.py:187-209; hist layers 'input' and conv2_1) through the whole chain vs the
    oracle.  The matching is a staircase in the feature values, so a pixel within float rounding of a bin edge may take
    the neighbouring step; measured on MI355X: loss 1.8e-7, gradient 1.3e-6 relative -- held to the metric's own bar
    (1e-3 on the gradient), the loss to 1e-4"""
    G, V = 24, 2
    layers = ["conv1_1", "conv2_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, V, layers)
    import neural_flow_style_amd.vgg as vgg
    rng = np.random.RandomState(4)
    simg = style_image(G, G, rng)
    net = loss.net
    hl, hw = ["input", "conv2_1"], [1.0, 0.5]
    loss2 = eng.RenderStyleLoss(net, layers, [1.0, 1.0], 1.0, transmit=0.05, w_hist=0.3, hist_layer=hl, w_hist_layer=hw)
    loss2.set_style_image(simg)
    targets = loss2.set_hist_image(simg)
    feats_s = O.vgg19_features(torch.tensor(simg)[None], w_or, "conv2_1")
    assert rel(targets["conv2_1"], feats_s["conv2_1"]) < 1e-5
    sfe = O.style_target_features(torch.tensor(simg)[None], w_or, layers, upto="conv2_1")
    cfg = dict(cfg, w_hist=0.3, hist_layer=hl, w_hist_layer=hw, upto="conv2_1",
               hist_feature={"input": torch.tensor(simg)[None], "conv2_1": feats_s["conv2_1"]})
    d_o = torch.tensor(d0)[None, ..., None].requires_grad_()
    total, per_view, _ = O.grid_forward(d_o, None, torch.tensor(np.asarray(mats, np.float32)), cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, d_o)
    gs = eng.GridStylizer(loss2, torch.tensor(d0).cuda(), k=3, target="d")
    losses, g_h = gs.gradient(T.rot_to_device(mats, "cuda"))
    e_l, e_g = rel(losses, torch.stack(per_view).detach()), rel(g_h, g_o[0, ..., 0])
    print("histogram term: loss rel %.2e, gradient rel-L2 %.2e" % (e_l, e_g))
    assert e_l < 1e-4
    assert e_g < 1e-3


def test_image_style_loss_with_masked_histogram_branch():
    """the 2-D colour loss with style_mask AND the histogram term: the masked branch of _loss (styler_base.py:196-201;
    hist layers 'input' and conv2_1) next to the masked style loss, loss and image gradient vs the oracle"""
    import neural_flow_style_amd.vgg as vgg
    import neural_flow_style_amd.engine as eng
    rng = np.random.RandomState(17)
    H = W = 24
    layers = ["conv1_1", "conv2_1"]
    w_np = vgg.synthetic_weights(123, upto="conv2_1")
    w_or = O.synthetic_vgg19_weights(123, upto="conv2_1")
    net = vgg.VGG(w_np, "cuda")
    simg = style_image(H, W, rng)
    d = rng.rand(1, H, W, 3).astype(np.float32)
    d_gray = np.clip(rng.rand(1, H, W, 1) * 1.6 - 0.5, 0, 1).astype(np.float32)     # ~30 % exact zeros
    hl, hw = ["input", "conv2_1"], [1.0, 0.5]
    loss = eng.ImageStyleLoss(net, layers, [1.0, 1.0], 1.0, w_tv=0.01, style_mask=True, w_hist=0.3, hist_layer=hl,
                              w_hist_layer=hw)
    loss.set_style_image(simg)
    loss.set_hist_image(simg)
    losses, g_h = loss.loss_and_grad(torch.tensor(d).cuda(), torch.tensor(d_gray).cuda())
    # oracle: the same graph from the image on
    d_o = torch.tensor(d, requires_grad=True)
    dg = torch.tensor(d_gray)
    d_img = O.plugin_to_loss_net(d_o, 1.0, is_color=True)
    feats = O.vgg19_features(d_img, w_or, "conv2_1")
    sfe = O.style_target_features(torch.tensor(simg)[None], w_or, layers, upto="conv2_1")
    feats_s = O.vgg19_features(torch.tensor(simg)[None], w_or, "conv2_1")
    total, _ = O.style_loss(feats, sfe, layers, [1.0, 1.0], 1.0, d_gray=dg)
    for name, wl in zip(hl, hw):
        f = d_img if name == "input" else feats[name]
        tpl = torch.tensor(simg)[None] if name == "input" else feats_s[name]
        m = O.tf1_resize_bicubic(dg, f.shape[1], f.shape[2])
        total = total + 0.3 * wl * O.hist_loss(f, tpl, mask=m)
    total = total + 0.01 * O.tv_loss(d_img)
    (g_o,) = torch.autograd.grad(total, d_o)
    e_l = abs(float(losses.sum()) - float(total.detach())) / float(total.detach())
    e_g = rel(g_h, g_o)
    print("masked histogram branch: loss rel %.2e, gradient rel-L2 %.2e" % (e_l, e_g))
    assert e_l < 2e-4          # (measured 2.6e-5 / 1.3e-4: a few pixels on the other side of a bin edge)
    assert e_g < 1e-3


def test_graph_is_recaptured_when_the_histogram_targets_change():
    """a captured hipGraph bakes in the histogram templates' addresses and the hist weights (kernel arguments):
    set_hist_image / a changed weight after the capture must force a re-capture, not a replay against freed tensors"""
    layers = ["conv1_1", "conv2_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(24, 2, layers)
    rot = T.rot_to_device(mats, "cuda")
    rng = np.random.RandomState(4)
    s1, s2 = style_image(24, 24, rng), style_image(24, 24, np.random.RandomState(9))
    out = []
    for graph in (False, True):
        l2 = eng.RenderStyleLoss(loss.net, layers, [1.0, 1.0], 1.0, transmit=0.05, w_hist=0.3, hist_layer=["conv2_1"],
                                 w_hist_layer=[1.0])
        l2.set_style_image(s1)
        keep = l2.set_hist_image(s1)                         # (held: the old templates must not be what is replayed)
        gs = eng.GridStylizer(l2, torch.tensor(d0).cuda(), k=3, target="v", lr=1e-3, graph=graph)
        gs.var.copy_(torch.tensor(vel0))
        ls = [float(gs.step(rot)) for _ in range(3)]
        g_before = gs._graph
        l2.set_hist_image(s2)
        ls += [float(gs.step(rot)) for _ in range(3)]
        if graph:
            assert g_before is not None and gs._graph is not None and gs._graph is not g_before
        g_mid = gs._graph
        l2.w_hist = 0.6
        ls += [float(gs.step(rot)) for _ in range(3)]
        if graph:
            assert gs._graph is not g_mid
        out.append((ls, gs.var.clone()))
        del keep
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-5)
    assert rel(out[0][1], out[1][1]) < 1e-5
    assert abs(out[0][0][3] - out[0][0][2]) > 1e-6 * abs(out[0][0][2])      # the new template does change the loss


_SLAB_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from neural_flow_style_amd import engine, vgg, parallel
from neural_flow_style_amd import synthetic as S, transform as T
world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) %% torch.cuda.device_count())
torch.cuda.set_device(dev)
if world > 1:
    dist.init_process_group("gloo")
D, HW, V = %(D)d, %(HW)d, %(V)d
rng = np.random.RandomState(5)
z = (HW - D) // 2                                 # [D, HW, HW]: the middle D planes of an HW^3 volume
d0 = S.blob_density(HW, rng)[z:z + D].copy(); vel = S.curl_velocity(HW, rng, max_cells=1.0)[z:z + D].copy()
simg = S.style_image(HW, HW, rng)
net = vgg.VGG(vgg.synthetic_weights(123, upto="conv3_1"), dev)
loss = engine.RenderStyleLoss(net, ["conv1_1", "conv2_1", "conv3_1"], [1.0] * 3, 1.0, transmit=0.02)
loss.set_style_image(simg)
gs = engine.GridStylizer(loss, torch.tensor(d0, device=dev), k=3, target="v", lr=1e-3,
                         process_group=dist.group.WORLD if world > 1 else None, graph=%(graph)r)
assert (gs.slab is not None) == (world > 1 and os.environ.get("NFS_SLAB_SHARD") != "0")
gs.var.copy_(torch.tensor(vel))
rot = T.rot_to_device(S.uniform_views(V), dev)[rank::world].contiguous()
ls = [float(gs.step(rot)) for _ in range(5)]
var = gs.gather_variable()
if rank == 0:
    np.savez(sys.argv[1], l=np.asarray(ls), var=var.cpu().numpy(), d_s=gs.d_s.abs().cpu().numpy())
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


@pytest.mark.parametrize("D,world,graph", [(24, 2, False), (28, 3, False), (24, 2, True), (24, 4, False), (24, 8, True)])
def test_slab_sharded_field_work_reproduces_the_single_rank_trajectory(tmp_path, D, world, graph):
    """views sharded over ranks (sharing the GPUs over gloo) with the field work sharded over D-slabs: reduce-scatter of
    the packed gradient chunks (two-plane halos, the loss in an extra plane) -> slab-local smooth adjoint, advect adjoint
    + ApplyAdam, advect, smooth -> all-gather of the smoothed density.  Even (24 / 2) and ragged (28 / 3: slabs of 10,
    10, 8 planes) splits, with and without the hipGraph of the loss chain, against the one-rank run and against the
    replicated all-reduce form of the same ranks.  World 4 and 8 on eight views are the rank counts of a SCALE run (two
    views / one view per rank; 24 / 8 = slabs of 3 planes)"""
    _slab_case(tmp_path, D, D, world, graph)


def test_slab_sharded_field_work_with_an_idle_rank_reproduces_the_single_rank_trajectory(tmp_path):
    """as above with a rank that owns no plane: 9 planes of 24 x 24 over 4 ranks = three slabs of 3 and an IDLE fourth
    rank (it still renders its two views, sends its chunks and receives zeros)"""
    _slab_case(tmp_path, 9, 24, 4, False)


def _slab_case(tmp_path, D, HW, world, graph):
    """the one-rank run, the D-slab sharded ranks and the replicated all-reduce ranks of _SLAB_SCRIPT on a [D, HW, HW]
    volume: the same losses, variable and smoothed density"""
    import os
    import subprocess
    import sys
    from tests.ranks import require_gpus_for, run_ranks
    require_gpus_for(world)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rank.py"
    script.write_text(_SLAB_SCRIPT % {"root": root, "D": D, "HW": HW, "graph": graph,
                                      "V": 8 if world in (4, 8) else 6})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=root)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NFS_SLAB_SHARD"):
        env.pop(k, None)
    one, slab, repl = tmp_path / "one.npz", tmp_path / "slab.npz", tmp_path / "repl.npz"
    subprocess.run([sys.executable, str(script), str(one)], check=True, env=env, timeout=600)
    run_ranks([sys.executable, str(script), str(slab)], world, env, timeout=900)
    run_ranks([sys.executable, str(script), str(repl)], world, dict(env, NFS_SLAB_SHARD="0"), timeout=900)
    a, b, c = np.load(one), np.load(slab), np.load(repl)
    np.testing.assert_allclose(b["l"], a["l"], rtol=2e-6)
    np.testing.assert_allclose(c["l"], a["l"], rtol=2e-6)
    # (two ranks: one order of a + b.  From three on the collectives may add the ranks in another order than the one
    # rank adds its views: rounding noise of 1e-11 in a voxel whose gradient is of the order of Adam's epsilon moves that
    # voxel's update by 1e-6 -- the bound admits that, not a wrong plane)
    tol = 2e-6 if world == 2 else 1e-4
    for other in (b, c):
        assert np.abs(other["var"] - a["var"]).max() <= tol * np.abs(a["var"]).max()
        assert np.abs(other["d_s"] - a["d_s"]).max() <= (1e-6 if world == 2 else 1e-5)
    # the two multi-rank forms apply the same kernels to the same sums: with two ranks (a + b has one order) identical
    # variables; with three the collectives may add the ranks in different orders
    if world == 2:
        assert np.array_equal(b["var"], c["var"])


def test_grid_stylizer_with_lbfgs_decreases_the_loss_and_matches_a_host_replay():
    """config.optimizer = 'lbfgs' (north_star's other outer loop): GridStylizer drives engine.LBFGSState with the
    gradient of the HIP chain; the trajectory equals a replay of the same gradients through torch.optim.LBFGS and the
    loss goes down"""
    layers = ["conv1_1", "conv2_1"]
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(24, 2, layers)
    rot = T.rot_to_device(mats, "cuda")
    gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=2e-4, optimizer="lbfgs")
    assert isinstance(gs.adam, eng.LBFGSState) and not gs.fuse_adam
    gs.var.copy_(torch.tensor(vel0))
    ref = torch.tensor(vel0).cuda().clone().requires_grad_()
    opt = torch.optim.LBFGS([ref], lr=2e-4, max_iter=1, history_size=10, tolerance_grad=0.0, tolerance_change=0.0)
    ls = []
    for _ in range(6):
        x_before = gs.var.clone()
        _, g = gs.gradient(rot)
        g = g.clone()

        def closure():
            ref.grad = g.clone()
            return torch.zeros((), device="cuda")
        assert rel(ref.detach(), x_before) < 1e-6
        opt.step(closure)
        ls.append(float(gs.step(rot)))
        assert rel(gs.var, ref.detach()) < 1e-5
    assert ls[-1] < ls[0]


def test_graphed_loss_replays_equal_eager_calls_with_several_graphs_alive():
    """engine.GraphedLoss (the particle stylers' one-view loss chain as a hipGraph): replays on changing inputs equal
    eager calls; two graphs of different sizes alive at once and used in turn (their scratch buffers are the captures'
    own); a graph dropped and re-captured after set_style_image; the measured choice picks one of the two modes"""
    out = {}
    for G in (20, 32):
        d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, 2, ["conv1_1", "conv2_1", "conv3_1"], seed=G)
        out[G] = (loss, T.rot_to_device(mats, "cuda"), eng)
    eng = out[20][2]
    graphed = {G: eng.GraphedLoss(out[G][0], force=True) for G in out}
    rng = np.random.RandomState(0)
    for it in range(5):
        for G in (20, 32, 20):
            loss, rot, _ = out[G]
            d = torch.tensor(blob_density(G, rng) * (1 + 0.1 * it), device="cuda")
            l_g, g_g = graphed[G](d, rot)
            l_g, g_g = l_g.clone(), g_g.clone()
            g_e = torch.zeros_like(d)
            l_e = loss.loss_and_grad(d, rot, g_e)
            assert rel(l_g, l_e) < 1e-5 and rel(g_g, g_e) < 1e-5, (it, G)
    assert graphed[20].mode == "graph" and graphed[20]._graph is not None
    # new style targets (new tensors: the capture is keyed on their addresses and taken again when they move -- when the
    # allocator hands the new Grams the very addresses of the old ones the graph stays, and reads the new values)
    loss, rot, _ = out[20]
    keep_alive = list(loss.style_grams.values())          # the old Grams stay allocated: the new ones must move
    old = graphed[20]._graph
    loss.set_style_image(style_image(20, 20, rng))
    d = torch.tensor(blob_density(20, rng), device="cuda")
    for _ in range(3):
        l_g, g_g = graphed[20](d, rot)
    g_e = torch.zeros_like(d)
    l_e = loss.loss_and_grad(d, rot, g_e)
    assert graphed[20]._graph is not old and rel(l_g, l_e) < 1e-5 and rel(g_g, g_e) < 1e-5
    del keep_alive
    loss.set_style_image(style_image(20, 20, rng))        # ... and whatever the allocator does here, the values hold
    l_g, g_g = graphed[20](d, rot)
    l_g, g_g = graphed[20](d, rot)
    g_e = torch.zeros_like(d)
    l_e = loss.loss_and_grad(d, rot, g_e)
    assert rel(l_g, l_e) < 1e-5 and rel(g_g, g_e) < 1e-5
    auto = eng.GraphedLoss(loss)
    for _ in range(4):
        l_a, g_a = auto(d, rot)
    assert auto.mode in ("graph", "eager") and auto.trial is not None
    assert rel(l_a, l_e) < 1e-5 and rel(g_a, g_e) < 1e-5


@pytest.mark.parametrize("user", ["grid_stylizer", "graphed_loss"])
def test_replay_takes_the_views_it_is_given_however_they_arrive(user):
    """the two users of engine.Replay -- GridStylizer(graph=True) stepping, GraphedLoss(force=True) called -- against an
    eager twin given the same views: warm-up and capture, a replay with the same unmodified view tensor (no copy), the
    same tensor overwritten in place, another tensor of equal shape, and the first one again.  Loss and gradient (for
    the stylizer: the variable after the step) are bit-equal at every stage, and no stage captures again"""
    layers = ["conv1_1", "conv2_1", "conv3_1"]
    G = 24 if user == "grid_stylizer" else 20
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(G, 2, layers)
    a, b, c = (T.rot_to_device(uniform_views(6)[i:i + 2], "cuda") for i in (0, 2, 4))
    # (the three view sets matter: a stage replayed on stale matrices cannot equal its twin by accident)
    probe = []
    for views in (a, b, c):
        g = torch.zeros(G, G, G, device="cuda")
        loss.loss_and_grad(torch.tensor(d0).cuda(), views, g)
        probe.append(g)
    assert not torch.equal(probe[0], probe[1]) and not torch.equal(probe[1], probe[2]) and not torch.equal(probe[0], probe[2])
    rot = a.clone()
    if user == "grid_stylizer":
        twins = []
        for graph in (True, False):
            gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=1e-3, graph=graph)
            gs.var.copy_(torch.tensor(vel0))
            twins.append(gs)
        replayed = twins[0]

        def both(views, it):
            out = [(gs.step(views).clone(), gs.var.clone()) for gs in twins]
            return out[0], out[1]
    else:
        replayed = eng.GraphedLoss(loss, force=True)
        eager = eng.GraphedLoss(loss, force=False)
        rng = np.random.RandomState(5)
        base = blob_density(G, rng)

        def both(views, it):
            d = torch.tensor(base * (1 + 0.1 * it), device="cuda")              # (the density changes with every call)
            out = []
            for fn in (replayed, eager):
                l, g = fn(d, views)
                out.append((l.clone(), g.clone()))
            return out[0], out[1]
    stages = [("warm-up", rot), ("capture", rot), ("same tensor, unmodified", rot), ("overwritten in place", b),
              ("another tensor", c), ("the first tensor again", rot), ("same tensor, unmodified", rot)]
    graph = None
    for it, (stage, views) in enumerate(stages):
        if stage == "overwritten in place":
            rot.copy_(views)
            views = rot
        got, want = both(views, it)
        for x, y in zip(got, want):
            assert torch.equal(x, y), (user, stage)
        if stage == "warm-up":
            assert replayed._graph is None
        elif stage == "capture":
            graph = replayed._graph
            assert graph is not None
        else:
            assert replayed._graph is graph, (user, stage)
            # the views' stamp is taken anew exactly when they were copied into the static buffer
            assert (replayed._replay.stamps[-1] is stamp) == (stage == "same tensor, unmodified"), (user, stage)
        stamp = None if graph is None else replayed._replay.stamps[-1]
    assert (eager if user == "graphed_loss" else twins[1])._graph is None

"""The 2-D grid stylizer (``grid2d.GridStylizer2D``, ``styler_grid.Styler`` with a 2-D resolution) at 24 x 32 -- non-square, so
a swapped axis shows -- with style layers conv1_1, conv2_1, conv3_1 and synthetic weights, against the float64 reference
loop of tests/grid2d_ref.py and against its own compositions.  Initial variables are small but non-zero, for the reason
given in tests/test_sequence_gpu.py (``v_init_for``): at zero velocity every back-traced point sits on a grid node."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import grid2d_ref as R
from tests import ranks
from tests import resize_ref as RR
from tests.test_sequence_gpu import _config, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 32
LAYERS = ["conv1_1", "conv2_1", "conv3_1"]
TARGETS = ("v", "d", "s", "p", "sp")


def T(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def same(a, b):
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def sequence_case(F=4, h=H, w=W, seed=11, cells=1.5):
    """F frames of a smoke blob drifting through smooth velocity fields (advect2d units), and a style image"""
    from neural_flow_style_amd import synthetic as S
    rng = np.random.RandomState(seed)
    d = [S.blob_density2d(h, w, rng)]
    u = [S.curl_velocity2d(h, w, rng, max_cells=cells) for _ in range(F)]
    for t in range(F - 1):
        d.append(O.advect2d(torch.tensor(d[-1])[None, ..., None], torch.tensor(u[t])[None])[0, ..., 0].numpy())
    return d, u, S.style_image(h, w, rng)


def init_for(kind, F, h=H, w=W, cells=0.3):
    return None if kind == "d" else [R.make_var(kind, h, w, cells, 40 + t) for t in range(F)]


@functools.lru_cache(maxsize=None)
def weights():
    return O.synthetic_vgg19_weights(123, upto="conv3_1")


def ref_cfg(**over):
    cfg = dict(grid_variable="v", num_frames=1, interp=1, frames_per_opt=1, window_sigma=0.0, iter=1, lr=0.01,
               style_layer=LAYERS, w_style_layer=[1.0] * 3, w_style=1.0, upto="conv3_1", resize_scale=1.0, adv_order=1,
               transport_recursive=True)
    cfg.update(over)
    return cfg


def make_loss(simg, resize_scale=1.0):
    from neural_flow_style_amd import engine, vgg
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv3_1"), "cuda:0")
    loss = engine.ImageStyleLoss(net, LAYERS, [1.0] * 3, 1.0, resize_scale=resize_scale)
    loss.set_style_image(simg)
    return loss


def stylizer(loss, d0, kind, init, **kw):
    from neural_flow_style_amd.grid2d import GridStylizer2D
    gs = GridStylizer2D(loss, T(d0), target=kind, **kw)
    if init is not None:
        gs.var.copy_(T(init))
    return gs


# ---- 1. the gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resize_scale", [1.0, 1.5])
@pytest.mark.parametrize("kind", TARGETS)
def test_gradient_matches_float64_autograd(kind, resize_scale):
    d, _, simg = sequence_case()
    init = init_for(kind, 1)
    x0 = d[0][..., None] if kind == "d" else init[0]
    cfg = ref_cfg(grid_variable=kind, resize_scale=resize_scale)
    want_l, want_g = R.loss_and_gradient(kind, d[0], x0, cfg, weights(), R.style_features(simg, cfg, weights()))
    gs = stylizer(make_loss(simg, resize_scale), d[0], kind, None if kind == "d" else init[0], graph=False)
    loss, g = gs.gradient()
    rl, rg = abs(float(loss.sum()) - want_l) / want_l, rel(g.reshape(want_g.shape).cpu().numpy(), want_g)
    print("%-2s resize_scale %.1f: loss rel %.2e, gradient rel L2 %.2e" % (kind, resize_scale, rl, rg))
    assert tuple(g.shape) == tuple(gs.var.shape)
    assert rg <= 1e-3 and rl <= 2e-3, (rg, rl)


# ---- 2. replay -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", TARGETS)
def test_four_steps_with_replay_on_and_off_are_the_same_bits(kind):
    d, _, simg = sequence_case()
    init = init_for(kind, 1)
    loss = make_loss(simg)
    out = []
    for graph in (False, True):
        gs = stylizer(loss, d[0], kind, None if kind == "d" else init[0], lr=0.01, graph=graph)
        ls = [float(gs.step()) for _ in range(4)]
        assert (gs._replay is not None and gs._replay.graph is not None) == graph
        out.append((ls, gs.var.clone(), gs.adam.m.clone(), gs.adam.v.clone()))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-5)      # (the printed loss; the bits asked for are below)
    for a, b in zip(out[0][1:], out[1][1:]):
        assert same(a, b)
    assert not torch.equal(out[0][1], T(d[0] if kind == "d" else init[0]))       # (it moved)


# ---- 3, 4. sequences through Styler.run ------------------------------------------------------------------------------------------------
def _cfg_for(F, simg, **over):
    base = dict(resolution=[H, W], num_frames=F, batch_size=1, frames_per_opt=1, window_sigma=1.0, interp=1, lr=0.02,
                iter=3, octave_n=1, style_layer=LAYERS, w_style_layer=[1, 1, 1], w_style=1.0, w_content=0, rotate=False,
                resize_scale=1.0, style_target=simg, grid_variable="v", adv_order=1)
    base.update(over)
    return _config(**base)


def _styler(F, simg, res=(H, W), **over):
    from neural_flow_style_amd.styler_grid import Styler
    st = Styler(_cfg_for(F, simg, resolution=list(res), **over))
    st.load_img(list(res))
    return st


LR = {"v": 0.02, "d": 0.05, "s": 0.004, "p": 0.004, "sp": 0.004}


@pytest.mark.parametrize("kind,interp,recursive,fpo", [("v", 1, True, 1), ("v", 1, False, 1), ("d", 1, True, 2),
                                                       ("s", 1, True, 1), ("sp", 1, True, 1), ("v", 2, True, 1)])
def test_sequence_matches_the_reference_loop(kind, interp, recursive, fpo):
    F = 5 if interp == 2 else 4
    d, u, simg = sequence_case(F)
    init = init_for(kind, F)
    over = dict(grid_variable=kind, interp=interp, transport_recursive=recursive, frames_per_opt=fpo, lr=LR[kind])
    params = {"d": d, "v": u}
    if init is not None:
        params[kind + "_init"] = init
    res = _styler(F, simg, **over).run(params)
    cfg = ref_cfg(num_frames=F, window_sigma=1.0, iter=3, **over)
    hist, outs, vels, imgs = R.sequence_run(cfg, d, u, weights(), simg, init=init)
    np.testing.assert_allclose(res["l_frames"], hist, rtol=2e-3)
    for t in range(F):
        rd = rel(res["d"][t], imgs[t])
        if kind == "d":
            rv = rel(res["opt"][t], outs[t])
        else:                                   # ('s' / 'sp' are compared through the velocity they stand for)
            rv = rel(res["v"][t], vels[t])
        print("%-2s frame %d: density rel %.2e, variable rel %.2e" % (kind, t, rd, rv))
        assert rd < 1e-3, t
        assert rv < (1e-3 if kind == "d" else 2e-2), t
    assert res["d"].shape == (F, H, W, 1) and res["d"].dtype == np.float32
    assert res["r"].shape == (F, H, W, 3) and res["r"].dtype == np.uint8
    assert all(x.shape == R.var_shape(kind, H, W) if kind != "d" else x.shape == (H, W, 1) for x in res["opt"])
    if kind != "d":
        assert all(x.shape == (H, W, 2) for x in res["v"])
    assert (res["s"] is not None) == (kind in ("s", "sp")) and (res["phi"] is not None) == (kind in ("p", "sp"))
    if kind == "sp":
        assert all(x.shape == (H, W) for x in res["s"]) and all(x.shape == (H, W) for x in res["phi"])
    assert np.asarray(res["l_frames"]).shape == (3, len(range(0, F, interp))) and res["octave_sizes"] == [[H, W]]
    assert res["d_intm"] == [] and len(res["opt_octave"]) == 1 and len(res["l"]) == 1


# ---- 5. the aligned update -----------------------------------------------------------------------------------------------------------------
def test_aligned_update_is_denoise_when_nothing_moves():
    from neural_flow_style_amd.util import denoise, temporal_weights
    F = 7
    _, _, simg = sequence_case()
    for rec in (True, False):
        st = _styler(F, simg, window_sigma=1.3, transport_recursive=rec)
        upd_np = np.random.RandomState(3).randn(F, H, W, 2).astype(np.float32)
        upd = {t: T(upd_np[t]) for t in range(F)}
        u = {t: torch.zeros(H, W, 2).cuda() for t in range(F)}
        Wt = temporal_weights(F, 1.3)
        want = denoise(upd_np, sigma=(1.3, 0, 0, 0))
        for t in range(F):
            got = st.aligned_update(t, upd, u, Wt, list(range(F))).cpu().numpy()
            np.testing.assert_allclose(got, want[t], atol=2e-6)


# ---- 6. MacCormack ---------------------------------------------------------------------------------------------------------------------------
def _smooth_case(seed):
    """a density without plateaus (the limiter compares against the corners' extrema: on a plateau the comparison is
    between equal numbers and an ulp decides it), with exact zeros"""
    from neural_flow_style_amd import synthetic as S
    rng = np.random.RandomState(seed)
    d = S.blob_density2d(H, W, rng, n_blobs=6)
    d = (0.8 * d / d.max()).astype(np.float32)
    return d, S.style_image(H, W, rng), R.make_var("v", H, W, 0.6, seed)


def _limiter64(d, vel):
    """the limiter's decisions of oracle.advect_maccormack in float64"""
    dt = torch.tensor(d, dtype=torch.float64)[None, ..., None]
    g = O.mgrid(H, W, dtype=torch.float64).unsqueeze(0)
    vp = torch.tensor(vel, dtype=torch.float64)[None].permute(0, 3, 1, 2)
    d_fwd = O.batch_warp2d(dt, g - vp, [1, H, W])
    d_adv = d_fwd + (dt - O.batch_warp2d(d_fwd, g + vp, [1, H, W])) * 0.5
    lo, hi = O._stencil_extrema(dt, g - vp)
    return ((d_adv > hi) | (lo > d_adv))[0, ..., 0].numpy()


def _keep_bits(keep):
    words = keep.view(torch.int64).cpu().numpy()
    e = np.arange(H * W)
    return ((words[e >> 6] >> (e & 63)) & 1).astype(bool).reshape(H, W)


# chosen on the CPU: the reference loop in float32 and in float64 takes the same limiter decisions at the start and after
# each of the three steps (54 to 58 pixels fire), and the two final images differ by 1.7e-6 relative (seeds 4 and 5 also
# agree on every decision and differ by 1e-3: an Adam step at the rounding floor, not the limiter)
MC_SEED = 2


def test_adv_order_2_gradient_is_the_hand_composition_and_three_steps_follow_the_reference():
    from neural_flow_style_amd import ops
    d, simg, v0 = _smooth_case(MC_SEED)
    loss = make_loss(simg)
    gs = stylizer(loss, d, "v", v0, lr=0.01, adv_order=2, graph=False)
    l, g = gs.gradient()
    img = ops.colour_clamp_gather(gs.d_adv.reshape(H * W, 1)).view(1, H, W, 1)
    l2, g_img = loss.loss_and_grad(img, img)
    g_adv = ops.clamp01_bwd(g_img.view(H, W), gs.d_adv.contiguous())
    g_hand = ops.advect_maccormack_bwd(T(d)[..., None], gs.var, gs._mc_fwd, gs._mc_keep, g_adv[..., None],
                                       need_d=False, need_vel=True)[1]
    assert same(g, g_hand)          # (the gradient; the loss scalar is summed with float atomics and is not held to bits)
    np.testing.assert_allclose(float(l.sum()), float(l2.sum()), rtol=1e-5)
    for _ in range(3):
        gs.step()
    gs.forward_field()
    cfg = ref_cfg(iter=3, adv_order=2)
    hist, outs, vels, imgs = R.sequence_run(cfg, [d], None, weights(), simg, init=[v0])
    # the limiter's decisions of the two final forwards agree (else the comparison below would measure the limiter)
    k32, k64 = _keep_bits(gs._mc_keep), _limiter64(d, outs[0])
    print("limiter fired at %d pixels (float32) / %d (float64), %d differ" % (k32.sum(), k64.sum(), (k32 != k64).sum()))
    assert np.array_equal(k32, k64) and k32.any()
    assert rel(gs.img[0].cpu().numpy(), imgs[0]) < 1e-3


# ---- 7. octaves --------------------------------------------------------------------------------------------------------------------------------
def _resize_dev(x, size, factor=1.0):
    from neural_flow_style_amd import ops
    x = T(np.asarray(x, np.float32)).unsqueeze(0)
    return ops.resize3d(x, (1,) + tuple(size), "bilinear", True, factor)[0].cpu().numpy()


def test_two_octaves_equal_their_composition():
    F, COARSE, FULL = 3, (H // 2, W // 2), (H, W)
    d, u, simg = sequence_case(F)
    init = init_for("s", F)
    kw = dict(grid_variable="s", iter=2, lr=LR["s"], octave_scale=2)
    both = _styler(F, simg, octave_n=2, **kw).run({"d": d, "v": u, "s_init": init})
    assert both["octave_sizes"] == [list(COARSE), list(FULL)]
    f_in, f = float(RR.potential_factor(FULL, COARSE)), float(RR.potential_factor(COARSE, FULL))
    a = _styler(F, simg, res=COARSE, octave_n=1, **kw).run(
        {"d": [_resize_dev(x, COARSE) for x in d], "v": [_resize_dev(x, COARSE) for x in u],
         "s_init": [_resize_dev(x, COARSE, f_in) for x in init]})
    b = _styler(F, simg, octave_n=1, **kw).run({"d": d, "v": u, "s_init": [_resize_dev(x, FULL, f) for x in a["opt"]]})
    np.testing.assert_allclose(both["l"][0], a["l"][0], rtol=1e-5)
    np.testing.assert_allclose(both["l"][1], b["l"][0], rtol=1e-5)
    for t in range(F):
        assert both["opt_octave"][0][t].shape == COARSE
        assert rel(both["opt_octave"][0][t], a["opt"][t]) < 1e-5, t
        assert rel(both["opt"][t], b["opt"][t]) < 1e-5, t
    assert rel(both["d"], b["d"]) < 1e-5
    assert len(both["d_intm"]) == 1 and both["d_intm"][0].shape == (F,) + COARSE + (3,)


# ---- 8. the invariants after four Adam steps ---------------------------------------------------------------------------------------------------
def test_stream_result_is_divergence_free_and_potential_result_rotation_free():
    d, u, simg = sequence_case(1)
    for kind in ("s", "p"):
        res = _styler(1, simg, grid_variable=kind, iter=4, lr=LR[kind], window_sigma=0.0).run(
            {"d": d[:1], "v": u[:1], kind + "_init": init_for(kind, 1)})
        var, vel = res["opt"][0], res["v"][0]
        assert vel.dtype == np.float32 and np.array_equal(vel, R.velocity(kind, var))
        if kind == "s":
            got, bound = np.abs(R.divergence(vel)).max(), R.divergence_bound(var)
        else:
            got, bound = np.abs(R.rotation(vel)).max(), R.rotation_bound(var)
        print("%s: %.3e (bound %.3e)" % (kind, got, bound))
        assert got <= bound


# ---- 9. two ranks ---------------------------------------------------------------------------------------------------------------------------------
_RANK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from tests.test_grid2d_stylizer_gpu import sequence_case, _styler, init_for
world = int(os.environ.get("WORLD_SIZE", "1"))
torch.cuda.set_device(0)
if world > 1:
    dist.init_process_group("gloo")
d, u, simg = sequence_case(4)
st = _styler(4, simg, window_sigma=1.0, iter=3)
if world > 1:
    st.pg = dist.group.WORLD
res = st.run({"d": d, "v": u, "v_init": init_for("v", 4)})
if int(os.environ.get("RANK", "0")) == 0:
    np.savez(sys.argv[1], l=np.asarray(res["l_frames"]), opt=np.stack(res["opt"]), d=res["d"])
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


def test_frames_sharded_over_two_ranks_reproduce_the_single_rank_run(tmp_path):
    ranks.require_gpus_for(2)
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % {"root": ROOT})
    env = dict(os.environ, PYTHONPATH=ROOT)
    one, two = tmp_path / "one.npz", tmp_path / "two.npz"
    ranks.run_ranks([sys.executable, str(script), str(one)], 1, env, timeout=300)
    ranks.run_ranks([sys.executable, str(script), str(two)], 2, env, timeout=300)
    a, b = np.load(one), np.load(two)
    np.testing.assert_allclose(b["l"], a["l"], rtol=1e-5)
    assert rel(b["opt"], a["opt"]) < 1e-5
    assert rel(b["d"], a["d"]) < 1e-5


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from neural_flow_style_amd.grid2d import GridStylizer2D
    from neural_flow_style_amd.styler_grid import Styler
    d, _, simg = sequence_case()
    with pytest.raises(ValueError, match="no views"):
        Styler(_cfg_for(4, simg, rotate=True))
    with pytest.raises(ValueError, match="lbfgs"):
        GridStylizer2D(make_loss(simg), T(d[0]), target="v", optimizer="lbfgs")
    with pytest.raises(ValueError, match="lbfgs"):
        Styler(_cfg_for(4, simg, optimizer="lbfgs"))

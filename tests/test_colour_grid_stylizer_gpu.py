"""grid_variable 'c' of the grid-sequence stylizer: the gradient of one frame's loss in the colour field against the float64
reference (tests/colour_grid_ref.py), ``Styler(config).run`` against the float64 loop, the result's surface, the other
optimisers, octaves, the default start, two ranks and the refusals.  17 x 12 x 12, synthetic weights, conv1_1 and conv2_1,
three uniform views."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import colour_grid_ref as GR
from tests import colour_runs as RUNS
from tests import ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = [17, 12, 12]
COARSE = [11, 8, 8]                      # RES // 1.5
LAYERS = ["conv1_1", "conv2_1"]
F_MAX = 3
# Two runs of the same launches on the same numbers give the same VARIABLES bit for bit (with the 'tiled' transpose), but not
# the same loss scalars: the loss kernels of the image chain (style_loss_fwd, tv_loss: gram.hip, field.hip) add their
# per-block partial sums into the loss with float atomics, in whatever order the blocks arrive.  The partials are
# non-negative (sums of squares), so two orders differ by at most (P - 1) 2^-24 relative for P partials; two layers of at
# most 64 Gram blocks and the TV blocks stay below P = 160: 1e-5.
LOSS_RTOL = 1e-5


def rel(a, b):
    a = torch.as_tensor(np.asarray(a)).double(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).norm() / (b.norm() + 1e-300))


@functools.lru_cache(maxsize=None)
def scene():
    """three frames of a smoke ball of compact support drifting along z (empty space around it: e == 0 there), smooth
    simulation velocities of about a cell, colours with some entries outside [0,1], a style image, the float64 loss
    network and its style features: computed once and left alone"""
    from scipy.ndimage import gaussian_filter
    from neural_flow_style_amd import synthetic as S
    rng = np.random.RandomState(29)
    D, H, W = RES
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    d, u = [], []
    for t in range(F_MAX):
        r2 = ((z - 7.0 - t) / 4.5) ** 2 + ((y - 5.5) / 3.6) ** 2 + ((x - 5.5) / 3.6) ** 2
        d.append((np.maximum(1 - r2, 0) ** 2 * (0.6 + 0.4 * np.cos(0.9 * x + 0.5 * y + t))).astype(np.float32))
        v = np.stack([gaussian_filter(rng.randn(D, H, W), 2.0) for _ in range(3)], -1)
        v = v / np.abs(v).max() * (2.0 / (np.array(RES) - 1))                # at most one cell along each axis
        u.append(v.astype(np.float32))
    c_init = rng.uniform(-0.15, 1.15, (F_MAX, D, H, W, 3)).astype(np.float32)
    simg = S.style_image(H, W, rng)
    w64 = {k: (np.asarray(a, np.float64), np.asarray(b, np.float64))
           for k, (a, b) in O.synthetic_vgg19_weights(123, upto="conv2_1").items()}
    sfe = O.style_target_features(torch.tensor(np.asarray(simg, np.float64))[None], w64, LAYERS, upto="conv2_1")
    return dict(d=d, u=u, c_init=c_init, simg=simg, w64=w64, sfe=sfe)


def _styler(F=1, res=RES, **over):
    from neural_flow_style_amd.styler_grid import Styler
    cfg = RUNS.base_config(res, "c", F=F, grid_variable="c", style_target=scene()["simg"], **over)
    st = Styler(cfg)
    st.load_img(list(res[1:]))
    return st, cfg


def _params(F, c_init=True):
    sc = scene()
    p = {"d": sc["d"][:F], "v": sc["u"][:F]}
    if c_init:
        p["c_init"] = [sc["c_init"][t] for t in range(F)]
    return p


@pytest.mark.parametrize("v_batch,style_mask,w_tv", [(1, True, 0.0), (1, False, 0.05), (3, True, 0.05), (3, False, 0.0)])
def test_gradient_of_one_frame(v_batch, style_mask, w_tv):
    """d loss / d c against the float64 reference: relative L2 <= 1e-3 (BASELINE's gradient bar), the summed loss within
    1e-3 relative; exactly zero for colours outside [0,1] and where e == 0"""
    from neural_flow_style_amd import engine
    sc = scene()
    st, cfg = _styler(v_batch=v_batch, style_mask=style_mask, w_tv=w_tv)
    st.loss.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    c = sc["c_init"][0]
    gs = engine.ColourGridStylizer(st.loss, st._dev(sc["d"][0]), k=cfg.k, lr=cfg.lr)
    gs.var.copy_(st._dev(c))
    assert len(st.rot_mat_) == 3
    losses, g = gs.gradient(st._rot())
    assert tuple(losses.shape) == (3,) and tuple(g.shape) == tuple(RES) + (3,) and g.device == st.device
    l_ref, g_ref = GR.loss_and_grad(sc["d"][0], c, dict(vars(cfg)), st.rot_mat_, sc["w64"], sc["sfe"])
    rg, rl = rel(g.cpu(), g_ref), abs(float(losses.sum()) - l_ref) / abs(l_ref)
    print("colour grid gradient v_batch %d mask %s tv %g: rel-L2 %.3g  loss rel %.3g" % (v_batch, style_mask, w_tv, rg, rl))
    e = gs.grey().cpu()
    outside = torch.tensor((c < 0) | (c > 1))
    empty = (e == 0).unsqueeze(-1).expand_as(outside)
    assert bool(outside.any()) and bool(empty.any()) and bool((~outside & ~empty).any())
    assert float(g_ref.abs().max()) > 0
    assert rg <= 1e-3, rg
    assert rl <= 1e-3, rl
    assert float(g.cpu()[outside].abs().max()) == 0.0
    assert float(g.cpu()[empty].abs().max()) == 0.0
    assert float(g_ref[outside].abs().max()) == 0.0 and float(g_ref[empty].abs().max()) == 0.0
    assert gs.contexts_formed == 1
    gs.gradient(st._rot())                                       # the same density and view tensor: the context is kept
    assert gs.contexts_formed == 1


@functools.lru_cache(maxsize=None)
def _sequence_run():
    st, cfg = _styler(F=2, iter=3, window_sigma=1.0, lr=0.01, style_mask=True, w_tv=0.01)
    return st, cfg, st.run(_params(2))


def test_run_against_the_float64_loop():
    """2 frames, 3 Adam steps, window_sigma = 1 with simulation velocities: per-step losses within 1e-3 of the float64
    loop, the variables within 1e-3 relative L2"""
    sc = scene()
    st, cfg, res = _sequence_run()
    hist, g_ref = GR.sequence_run(dict(vars(cfg)), sc["d"][:2], np.stack(sc["u"][:2]), sc["w64"], sc["sfe"], st.rot_mat_,
                                  sc["c_init"])
    got = np.asarray(res["l_frames"])
    print("colour grid run losses", got, "reference", np.asarray(hist), "rel", np.abs(got - hist) / np.abs(hist))
    assert got.shape == (3, 2)
    np.testing.assert_allclose(got, hist, rtol=1e-3)
    for t in range(2):
        r_ = rel(res["opt"][t], g_ref[t])
        print("frame %d variable rel-L2 %.3g" % (t, r_))
        assert r_ <= 1e-3, (t, r_)


def test_result_surface():
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import transform as T
    sc = scene()
    st, cfg, res = _sequence_run()
    F = 2
    assert set(res) >= {"l", "l_frames", "d_intm", "opt_octave", "octave_sizes", "d", "r", "v", "s", "phi", "opt", "p", "c",
                        "c_init", "frames"}
    assert res["v"] is None and res["s"] is None and res["phi"] is None and res["p"] is None
    assert res["d_intm"] == [] and res["frames"] == [0, 1] and res["octave_sizes"] == [RES]
    assert res["r"].shape == (F, RES[1], RES[2], 3) and res["r"].dtype == np.uint8
    assert res["d"].shape == (F,) + tuple(RES) + (1,) and res["d"].dtype == np.float32
    assert len(res["c_init"]) == F and all(np.array_equal(res["c_init"][t], sc["c_init"][t]) for t in range(F))
    assert res["r"].max() > 0 and len(np.unique(res["r"])) > 8
    eye = T.rot_to_device([np.identity(3)], st.device)
    for t in range(F):
        opt, c = res["opt"][t], res["c"][t]
        assert opt.shape == tuple(RES) + (3,) and opt.dtype == np.float32 and c.shape == opt.shape and c.dtype == np.float32
        assert not np.array_equal(opt, sc["c_init"][t])
        e = ops.smooth3d_relu_fwd(st._dev(sc["d"][t]), float(cfg.k))
        assert not bool(torch.signbit(torch.as_tensor(res["d"][t])).any())
        assert np.array_equal(res["d"][t][..., 0], torch.abs(e).cpu().numpy())
        e_np = res["d"][t]
        assert c.min() >= 0.0 and c.max() <= 1.0 and (e_np == 0).any()
        assert float(np.abs(c[np.broadcast_to(e_np == 0, c.shape)]).max()) == 0.0
        np.testing.assert_array_equal(c, np.clip(opt, 0, 1) * np.clip(e_np, 0, 1))
        # 'r': the identity view of 'opt', rendered again through ops (no atomics on the way: the very bits)
        w = torch.empty((1,) + tuple(RES), device=st.device)
        grey, _ = ops.rotate_render_fwd(e, eye, cfg.transmit, False, d_rot=w)
        _, gmax = ops.maxnorm_fwd(grey, 1)
        ops.ray_weights(w, cfg.transmit, gmax, out=w)
        img = torch.clamp(ops.colour_project_fwd(ops.emission_fwd(st._dev(opt), e), eye, w), 0, 1)
        r, _ = ops.loss_net_input_fwd(img.contiguous(), RES[1], RES[2], want_x=False)
        assert np.array_equal(res["r"][t], r[0].cpu().numpy().astype(np.uint8))


@pytest.mark.parametrize("optimizer,lr", [("lbfgs", 1.0), ("lapnorm", 0.02)])
def test_other_optimisers_lower_the_loss(optimizer, lr):
    """two steps of L-BFGS / Laplacian-normalised descent on a one-frame problem: the loss before the third step is below
    the loss before the first"""
    st, cfg = _styler(F=1, iter=3, lr=lr, optimizer=optimizer, window_sigma=0)
    res = st.run(_params(1))
    l = np.asarray(res["l_frames"])[:, 0]
    print("%s losses" % optimizer, l)
    assert l.shape == (3,) and np.isfinite(l).all()
    assert l[2] < l[0]
    assert not np.array_equal(res["opt"][0], scene()["c_init"][0])


def _resize_dev(x, size):
    from neural_flow_style_amd import ops
    return ops.resize3d(torch.tensor(np.asarray(x, np.float32)).cuda().contiguous(), tuple(size), "bilinear", True, 1.0).cpu().numpy()


def test_two_octaves_equal_their_composition():
    """octave_n = 2 against run A (one octave at 11 x 8 x 8 on inputs resampled with ops.resize3d) followed by run B (one
    octave at full size from A's result, resampled with factor 1, handed over by c_init): the same launches on the same
    numbers, and with the 'tiled' transpose the same bits"""
    kw = dict(F=2, iter=2, window_sigma=1.0, lr=0.01, w_tv=0.01, octave_scale=1.5, colour_bwd_route="tiled")
    p = _params(2)
    both = _styler(octave_n=2, **kw)[0].run(p)
    assert both["octave_sizes"] == [COARSE, RES]
    a = _styler(res=COARSE, octave_n=1, **kw)[0].run({k: [_resize_dev(x, COARSE) for x in v] for k, v in p.items()})
    b = _styler(octave_n=1, **kw)[0].run({"d": p["d"], "v": p["v"], "c_init": [_resize_dev(x, RES) for x in a["opt"]]})
    np.testing.assert_allclose(both["l"][0], a["l"][0], rtol=LOSS_RTOL)
    np.testing.assert_allclose(both["l"][1], b["l"][0], rtol=LOSS_RTOL)
    for t in range(2):
        assert np.array_equal(both["opt_octave"][0][t], a["opt"][t])
        assert np.array_equal(both["opt"][t], b["opt"][t]) and np.array_equal(both["c"][t], b["c"][t])
    assert np.array_equal(both["r"], b["r"]) and np.array_equal(both["d"], b["d"])
    assert len(both["d_intm"]) == 1 and both["d_intm"][0].shape == (2, COARSE[1], COARSE[2], 3)      # in colour
    assert both["d_intm"][0].dtype == np.uint8 and np.array_equal(both["d_intm"][0], a["r"])


def test_default_start_is_one_field_for_all_frames():
    """without c_init: seeded noise around the VGG mean / 255, ONE field shared by the frames (no flicker is seeded)"""
    st, cfg = _styler(F=2, iter=1, window_sigma=0)
    res = st.run(_params(2, c_init=False))
    ci = res["c_init"]
    assert len(ci) == 2 and ci[0].shape == tuple(RES) + (3,) and ci[0].dtype == np.float32
    assert np.array_equal(ci[0], ci[1])
    mean = np.array(O.VGG_MEAN) / 255
    assert np.all(np.abs(ci[0] - mean) <= 5.0 / 255 + 1e-6) and float(ci[0].std()) > 0.005
    st2, _ = _styler(F=2, iter=1, window_sigma=0)
    assert np.array_equal(st2.run(_params(2, c_init=False))["c_init"][0], ci[0])       # seeded
    # the step moved the colours where the frame's own smoke is, and only there
    for t in range(2):
        moved = np.abs(res["opt"][t] - ci[t]).max(-1) > 0
        assert moved.any() and not moved[res["d"][t][..., 0] == 0].any()


_RANK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from tests.test_colour_grid_stylizer_gpu import _params, _styler
world = int(os.environ.get("WORLD_SIZE", "1"))
torch.cuda.set_device(0)
if world > 1:
    dist.init_process_group("gloo")
st, _ = _styler(F=3, iter=2, window_sigma=1.0, lr=0.01, w_tv=0.01, colour_bwd_route="tiled")
if world > 1:
    st.pg = dist.group.WORLD
res = st.run(_params(3))
if int(os.environ.get("RANK", "0")) == 0:
    np.savez(sys.argv[1], l=np.asarray(res["l_frames"]), opt=np.stack(res["opt"]), c=np.stack(res["c"]), r=res["r"])
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


def test_frames_sharded_over_two_ranks_reproduce_the_single_rank_run(tmp_path):
    """a 3-frame sequence, two ranks sharing the one GPU: with the 'tiled' transpose the very bits of the single-rank run"""
    ranks.require_gpus_for(2)
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % {"root": ROOT})
    env = dict(os.environ, PYTHONPATH=ROOT)
    one, two = tmp_path / "one.npz", tmp_path / "two.npz"
    ranks.run_ranks([sys.executable, str(script), str(one)], 1, env, timeout=300)
    ranks.run_ranks([sys.executable, str(script), str(two)], 2, env, timeout=300)
    a, b = np.load(one), np.load(two)
    assert a["l"].shape == (2, 3)
    np.testing.assert_allclose(b["l"], a["l"], rtol=LOSS_RTOL)
    for k in ("opt", "c", "r"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("flag,over", [("resolution", dict(resolution=[12, 12])), ("render_liquid", dict(render_liquid=True)),
                                       ("ray_mode", dict(ray_mode="max")), ("style_mask_on_ref", dict(style_mask_on_ref=True)),
                                       ("w_density", dict(w_density=1.0))])
def test_constructor_refusals(flag, over):
    with pytest.raises(ValueError, match=flag):
        _styler(**over)


def test_adv_order_is_accepted_and_has_no_effect():
    kw = dict(F=1, iter=2, window_sigma=0, lr=0.01, colour_bwd_route="tiled")
    a = _styler(adv_order=1, **kw)[0].run(_params(1))
    b = _styler(adv_order=2, **kw)[0].run(_params(1))
    np.testing.assert_allclose(a["l"], b["l"], rtol=LOSS_RTOL)
    assert np.array_equal(a["opt"][0], b["opt"][0])

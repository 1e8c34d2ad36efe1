"""``colour_render 'liquid'`` on both colour stylizers (grid_variable 'c' of styler_grid, target_field 'c' of styler_3p): the
gradient of one frame's loss against the float64 reference (tests/colour_liquid_ref.py), ``Styler(config).run`` against the
float64 loops, a uniform colour over a non-white background, the other optimisers, octaves and two ranks on the grid, and
the default-flag runs of both against arrays recorded on the commit before the flag (tests/golden/colour_liquid_unchanged.npz).

The scenes are those of tests/test_colour_grid_stylizer_gpu.py and tests/test_colour_stylizer_gpu.py: 17 x 12 x 12, synthetic
weights, conv1_1 and conv2_1, three uniform views; transmit = 0.2, the chocolate driver's.  At that transmit the grid scene's
smoke ball is nearly transparent as it stands (its grey liquid image stays below 0.47), so the liquid tests take its
densities times 2.5 -- the same geometry, velocities, colours and style -- and every test asserts that the grey liquid
image of each frame it runs, at each size it runs it, has pixels below 0.1 and above 0.5 (``_grid_opaque_enough`` on the
grid: the kernel's own grey of the smoothed densities at the styler's views).  The octave test also runs the frames at
11 x 8 x 8, where a ray has 11 samples of a ball smoothed by the same k and stays below 0.48 at 2.5; it takes the
densities times 5.  The particle scene is taken as it is.  The uniform-colour identity is held on
the grid, where q = c0 e exactly; on particles the absorbing volume is smoothed and the emission is not, so it does not
hold there (engine.ColourRenderLoss's docstring)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import colour_liquid_ref as LR
from tests import colour_liquid_runs as LRUNS
from tests import colour_ref as CR
from tests import colour_runs as RUNS
from tests import ranks
from tests import test_colour_grid_stylizer_gpu as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = G.RES
TRANSMIT = 0.2
BG = [0.2, 0.6, 0.05]                     # not white
DENSER = 2.5                              # (module docstring)
DENSER_OCTAVES = 5.0                      # for the run that also renders at G.COARSE
LIQUID = dict(colour_render="liquid", colour_background=BG, transmit=TRANSMIT)
rel = G.rel


def _opaque_enough(grey):
    lo, hi = float(grey.min()), float(grey.max())
    print("grey liquid image in [%.3f, %.3f]" % (lo, hi))
    assert lo < 0.1 and hi > 0.5, (lo, hi)


def _ref_cfg(cfg):
    return dict(vars(cfg))


# ---- the grid ---------------------------------------------------------------------------------------------------------

def _gdens(t, denser=DENSER):
    return (G.scene()["d"][t] * np.float32(denser)).astype(np.float32)


def _gstyler(F=1, res=RES, **over):
    kw = dict(LIQUID)
    kw.update(over)
    return G._styler(F=F, res=res, **kw)


def _gparams(F, denser=DENSER):
    p = G._params(F)
    p["d"] = [_gdens(t, denser) for t in range(F)]
    return p


def _grid_greys(st, cfg, dens):
    """the grey liquid images [V,H,W] of the density frames ``dens`` as the styler ``st`` renders them: nfs_liquid_weights'
    grey of the smoothed densities at the styler's views"""
    from neural_flow_style_amd import ops
    return [ops.liquid_weights(ops.smooth3d_relu_fwd(st._dev(d), float(cfg.k)), st._rot(), TRANSMIT)[1] for d in dens]


def _grid_opaque_enough(st, cfg, dens):
    greys = _grid_greys(st, cfg, dens)
    assert len(greys) == len(dens) and all(tuple(g.shape) == (len(st.rot_mat_),) + tuple(d.shape[1:]) for g, d in zip(greys, dens))
    for g in greys:
        _opaque_enough(g)


@pytest.mark.parametrize("v_batch,style_mask,w_tv", [(1, True, 0.0), (1, False, 0.05), (3, True, 0.05), (3, False, 0.0)])
def test_grid_gradient_of_one_frame(v_batch, style_mask, w_tv):
    """d loss / d c against the float64 reference: relative L2 <= 1e-3 (BASELINE's gradient bar), the summed loss within
    1e-3 relative; exactly zero for colours outside [0,1] and where e == 0"""
    from neural_flow_style_amd import engine
    sc = G.scene()
    st, cfg = _gstyler(v_batch=v_batch, style_mask=style_mask, w_tv=w_tv)
    assert st.loss.liquid and st.loss.background == tuple(float(x) for x in BG)
    st.loss.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    c = sc["c_init"][0]
    gs = engine.ColourGridStylizer(st.loss, st._dev(_gdens(0)), k=cfg.k, lr=cfg.lr)
    gs.var.copy_(st._dev(c))
    assert len(st.rot_mat_) == 3
    losses, g = gs.gradient(st._rot())
    ctx = gs.context(st._rot())
    assert ctx["gmax"] is None and tuple(ctx["t_total"].shape) == (3,) + tuple(RES[1:])
    assert tuple(ctx["bg_img"].shape) == (3,) + tuple(RES[1:]) + (3,) and tuple(ctx["d_gray"].shape) == (3,) + tuple(RES[1:]) + (1,)
    assert torch.equal(ctx["d_gray"][..., 0], ctx["grey"])
    _opaque_enough(ctx["grey"])
    assert tuple(losses.shape) == (3,) and tuple(g.shape) == tuple(RES) + (3,)
    l_ref, g_ref = LR.grid_loss_and_grad(_gdens(0), c, _ref_cfg(cfg), st.rot_mat_, sc["w64"], sc["sfe"])
    rg, rl = rel(g.cpu(), g_ref), abs(float(losses.sum()) - l_ref) / abs(l_ref)
    print("liquid grid gradient v_batch %d mask %s tv %g: rel-L2 %.3g  loss rel %.3g" % (v_batch, style_mask, w_tv, rg, rl))
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


def test_grid_run_against_the_float64_loop():
    """2 frames, 3 Adam steps, window_sigma = 1 with simulation velocities: per-step losses within 1e-3 of the float64
    loop, the variables within 1e-3 relative L2; 'r' is the identity view of 'opt' over the background, bit for bit"""
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import transform as T
    sc = G.scene()
    st, cfg = _gstyler(F=2, iter=3, window_sigma=1.0, lr=0.01, style_mask=True, w_tv=0.01)
    res = st.run(_gparams(2))
    hist, g_ref = LR.grid_sequence_run(_ref_cfg(cfg), [_gdens(0), _gdens(1)], np.stack(sc["u"][:2]), sc["w64"], sc["sfe"],
                                       st.rot_mat_, sc["c_init"])
    got = np.asarray(res["l_frames"])
    print("liquid grid run losses", got, "reference", np.asarray(hist), "rel", np.abs(got - hist) / np.abs(hist))
    assert got.shape == (3, 2)
    np.testing.assert_allclose(got, hist, rtol=1e-3)
    for t in range(2):
        r_ = rel(res["opt"][t], g_ref[t])
        print("frame %d variable rel-L2 %.3g" % (t, r_))
        assert r_ <= 1e-3, (t, r_)
    eye = T.rot_to_device([np.identity(3)], st.device)
    bg = torch.tensor(BG, dtype=torch.float32, device=st.device)
    for t in range(2):
        e = ops.smooth3d_relu_fwd(st._dev(_gdens(t)), float(cfg.k))
        assert np.array_equal(res["d"][t][..., 0], torch.abs(e).cpu().numpy())
        np.testing.assert_array_equal(res["c"][t], np.clip(res["opt"][t], 0, 1) * np.clip(res["d"][t], 0, 1))
        w, grey, tt = ops.liquid_weights(e, eye, TRANSMIT)
        _opaque_enough(grey)
        J = ops.colour_project_fwd(ops.emission_fwd(st._dev(res["opt"][t]), e), eye, w) + tt.unsqueeze(-1) * bg
        r, _ = ops.loss_net_input_fwd(torch.clamp(J, 0, 1).contiguous(), RES[1], RES[2], want_x=False)
        assert np.array_equal(res["r"][t], r[0].cpu().numpy().astype(np.uint8))
        # a transparent corner pixel shows the background
        assert np.abs(res["r"][t][0, 0].astype(np.float64) - 255 * np.array(BG)).max() <= 1.0


def test_grid_uniform_colour_renders_the_reference_line_153():
    """c = c0 everywhere, q = c0 e: J = c0 (1 - t) + t bg at a non-white background.  Tolerance: a pixel is a sum of 17
    samples; the projection's samples of c0 e and the weights' samples of e come from the same coordinates up to
    view_ref's K_COORD roundings (|de| dc <= 1.7 * 16 EPS * 30 = 5e-5 per sample, times w <= 0.2, times 17: 1.7e-4), the
    roundings of the sums are an order below: 2e-4"""
    from neural_flow_style_amd import engine
    st, cfg = _gstyler()
    c0 = torch.tensor([0.26, 0.5, 0.75], device=st.device)
    gs = engine.ColourGridStylizer(st.loss, st._dev(_gdens(0)), k=cfg.k, lr=cfg.lr)
    gs.var.copy_(c0.expand_as(gs.var))
    ctx = gs.context(st._rot())
    _opaque_enough(ctx["grey"])
    J, img = st.loss.project(gs.emission(), ctx)
    t = ctx["t_total"].unsqueeze(-1)
    want = c0 * (1 - t) + t * torch.tensor(BG, device=st.device)
    err = float((J - want).abs().max())
    print("uniform colour: max |J - (c0 (1 - t) + t bg)| = %.3g" % err)
    assert err <= 2e-4 and torch.equal(img, torch.clamp(J, 0, 1))
    assert float((want - torch.tensor(BG, device=st.device)).abs().max()) > 0.3          # (not the background alone)


@pytest.mark.parametrize("optimizer,lr", [("lbfgs", 1.0), ("lapnorm", 0.02)])
def test_grid_other_optimisers_lower_the_loss(optimizer, lr):
    st, cfg = _gstyler(F=1, iter=3, lr=lr, optimizer=optimizer, window_sigma=0)
    p = _gparams(1)
    _grid_opaque_enough(st, cfg, p["d"])
    res = st.run(p)
    l = np.asarray(res["l_frames"])[:, 0]
    print("liquid %s losses" % optimizer, l)
    assert l.shape == (3,) and np.isfinite(l).all()
    assert l[2] < l[0]
    assert not np.array_equal(res["opt"][0], G.scene()["c_init"][0])


def test_grid_two_octaves_equal_their_composition():
    """octave_n = 2 against one octave at 11 x 8 x 8 followed by one at full size from its result (as the smoke test of
    tests/test_colour_grid_stylizer_gpu.py): with the 'tiled' transpose the same bits; 'd_intm' is over the background.
    Both frames are opaque enough at both sizes (the densities times DENSER_OCTAVES: module docstring)"""
    kw = dict(F=2, iter=2, window_sigma=1.0, lr=0.01, w_tv=0.01, octave_scale=1.5, colour_bwd_route="tiled")
    p = _gparams(2, DENSER_OCTAVES)
    both = _gstyler(octave_n=2, **kw)[0].run(p)
    assert both["octave_sizes"] == [G.COARSE, RES]
    p_coarse = {k: [G._resize_dev(x, G.COARSE) for x in v] for k, v in p.items()}
    st_a, cfg_a = _gstyler(res=G.COARSE, octave_n=1, **kw)
    st_b, cfg_b = _gstyler(octave_n=1, **kw)
    _grid_opaque_enough(st_a, cfg_a, p_coarse["d"])
    _grid_opaque_enough(st_b, cfg_b, p["d"])
    a = st_a.run(p_coarse)
    b = st_b.run({"d": p["d"], "v": p["v"], "c_init": [G._resize_dev(x, RES) for x in a["opt"]]})
    np.testing.assert_allclose(both["l"][0], a["l"][0], rtol=G.LOSS_RTOL)
    np.testing.assert_allclose(both["l"][1], b["l"][0], rtol=G.LOSS_RTOL)
    for t in range(2):
        assert np.array_equal(both["opt_octave"][0][t], a["opt"][t])
        assert np.array_equal(both["opt"][t], b["opt"][t]) and np.array_equal(both["c"][t], b["c"][t])
    assert np.array_equal(both["r"], b["r"]) and np.array_equal(both["d"], b["d"])
    assert len(both["d_intm"]) == 1 and both["d_intm"][0].shape == (2, G.COARSE[1], G.COARSE[2], 3)
    assert np.array_equal(both["d_intm"][0], a["r"])
    assert np.abs(both["d_intm"][0][:, 0, 0].astype(np.float64) - 255 * np.array(BG)).max() <= 1.0


_RANK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from tests.test_colour_liquid_stylizer_gpu import _gparams, _grid_greys, _gstyler
world = int(os.environ.get("WORLD_SIZE", "1"))
torch.cuda.set_device(0)
if world > 1:
    dist.init_process_group("gloo")
st, cfg = _gstyler(F=3, iter=2, window_sigma=1.0, lr=0.01, w_tv=0.01, colour_bwd_route="tiled")
assert st.loss.liquid
if world > 1:
    st.pg = dist.group.WORLD
p = _gparams(3)
res = st.run(p)
if int(os.environ.get("RANK", "0")) == 0:
    grey = torch.stack(_grid_greys(st, cfg, p["d"])).cpu().numpy()
    np.savez(sys.argv[1], l=np.asarray(res["l_frames"]), opt=np.stack(res["opt"]), c=np.stack(res["c"]), r=res["r"], grey=grey)
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


def test_grid_frames_sharded_over_two_ranks_reproduce_the_single_rank_run(tmp_path):
    """a 3-frame sequence, two ranks sharing the one GPU: with the 'tiled' transpose the very bits of the single-rank run;
    each of the three frames is opaque enough, in both runs"""
    ranks.require_gpus_for(2)
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % {"root": ROOT})
    env = dict(os.environ, PYTHONPATH=ROOT)
    one, two = tmp_path / "one.npz", tmp_path / "two.npz"
    ranks.run_ranks([sys.executable, str(script), str(one)], 1, env, timeout=300)
    ranks.run_ranks([sys.executable, str(script), str(two)], 2, env, timeout=300)
    a, b = np.load(one), np.load(two)
    assert a["l"].shape == (2, 3)
    for run in (a, b):
        assert run["grey"].shape == (3, 3) + tuple(RES[1:])
        for t in range(3):
            _opaque_enough(run["grey"][t])
    np.testing.assert_allclose(b["l"], a["l"], rtol=G.LOSS_RTOL)
    for k in ("opt", "c", "r"):
        assert np.array_equal(a[k], b[k]), k


# ---- particles --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    """the particle scene (tests/colour_liquid_runs.py: test_colour_stylizer_gpu's draws) with the float64 loss network"""
    sc = LRUNS.particle_scene()
    w64 = {k: (np.asarray(a, np.float64), np.asarray(b, np.float64))
           for k, (a, b) in O.synthetic_vgg19_weights(123, upto="conv2_1").items()}
    sfe = O.style_target_features(torch.tensor(np.asarray(sc["simg"], np.float64))[None], w64, G.LAYERS, upto="conv2_1")
    return dict(sc, w64=w64, sfe=sfe)


def _pstyler(scene, F=1, **over):
    from neural_flow_style_amd.styler_3p import Styler
    kw = dict(LIQUID)
    kw.update(over)
    cfg = RUNS.base_config(RES, "c", F=F, style_target=scene["simg"], **kw)
    st = Styler(cfg)
    st.load_img(RES[1:])
    return st, cfg


def _pref_loss_grad(scene, cfg, t, c, R):
    c64 = torch.tensor(np.asarray(c, np.float64), requires_grad=True)
    l = LR.particle_frame_loss(torch.tensor(scene["p"][t]).double(), torch.tensor(scene["r"][t]).double(), c64,
                               _ref_cfg(cfg), RES, torch.tensor(np.asarray(R, np.float32)).double(), scene["w64"],
                               scene["sfe"])
    (g,) = torch.autograd.grad(l, c64)
    return float(l.detach()), g


@pytest.mark.parametrize("mode,v_batch,style_mask,w_tv", [("sequential", 1, True, 0.0), ("sum", 1, False, 0.05),
                                                          ("sum", 3, True, 0.05), ("sequential", 1, False, 0.05)])
def test_particle_gradient_of_one_frame(scene, mode, v_batch, style_mask, w_tv):
    """d loss / d c against the float64 reference: relative L2 <= 1e-3, the summed loss within 1e-3, per view batch in the
    sequential mode and for the summed views; colours outside [0,1] get exactly zero"""
    st, cfg = _pstyler(scene, views_mode=mode, v_batch=v_batch, style_mask=style_mask, w_tv=w_tv)
    assert st.colour.liquid
    st.colour.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    p, r = st._dev(scene["p"][0]), st._dev(scene["r"][0])
    c = scene["c_init"][0]
    var = st._dev(c)
    outside = torch.tensor((c < 0) | (c > 1))
    assert bool(outside.any())
    nv = len(st.rot_mat_)
    assert nv == 3
    batches = [(i, i + v_batch) for i in range(0, nv, v_batch)] if mode == "sequential" else [(0, nv)]
    greys = []
    for lo, hi in batches:
        rot = st._rot(lo, hi)
        losses, g = st._value_and_grad(p, r, var, RES, rot, view_shard=False)
        ctx = st._colour_ctx(st._colour_frame(p, r, RES), rot)
        assert ctx["gmax"] is None
        greys.append(ctx["grey"])
        assert tuple(losses.shape) == (hi - lo,) and tuple(g.shape) == (LRUNS.N, 3)
        l_ref, g_ref = 0.0, 0.0
        for b in range(lo, hi, v_batch):
            l_b, g_b = _pref_loss_grad(scene, cfg, 0, c, st.rot_mat_[b:b + v_batch])
            l_ref, g_ref = l_ref + l_b, g_ref + g_b
        rg, rl = rel(g.cpu(), g_ref), abs(float(losses.sum()) - l_ref) / abs(l_ref)
        print("liquid particle gradient %s v_batch %d mask %s tv %g views %d:%d  rel-L2 %.3g  loss rel %.3g"
              % (mode, v_batch, style_mask, w_tv, lo, hi, rg, rl))
        assert float(g_ref.abs().max()) > 0
        assert rg <= 1e-3, rg
        assert rl <= 1e-3, rl
        assert float(g.cpu()[outside].abs().max()) == 0.0
    _opaque_enough(torch.cat(greys))


def test_particle_run_against_the_float64_loop(scene):
    """3 Adam steps, 2 frames, window_sigma > 0, the sequential view loop: per-step losses within 1e-3 of the float64 loop
    on the same c_init, the variables within 1e-3; 'r' is over the background"""
    F = scene["F"]
    st, cfg = _pstyler(scene, F=F, iter=3, window_sigma=1.0, lr=0.01, style_mask=True, w_tv=0.01)
    res = st.run({"p": scene["p"], "r": scene["r"], "c_init": scene["c_init"]})
    g_opt = [torch.tensor(scene["c_init"][t]).double() for t in range(F)]
    opt = [O.TFAdam() for _ in range(F)]
    Wt = O.temporal_filter_matrix(F, cfg.window_sigma)
    hist = []
    for _ in range(3):
        upd = []
        for t in range(F):
            var, acc, ls = g_opt[t].clone(), 0.0, []
            for i in range(len(st.rot_mat_)):
                l, g = _pref_loss_grad(scene, cfg, t, var, st.rot_mat_[i:i + 1])
                var = opt[t].step(var, g, cfg.lr)
                ls.append(l)
                acc = acc + torch.nan_to_num(var)
            hist.append(float(np.mean(ls)))
            upd.append(acc / len(st.rot_mat_) - g_opt[t])
        for t in range(F):
            g_opt[t] = g_opt[t] + sum(float(Wt[t, s]) * upd[s] for s in range(F))
    got = np.asarray(res["l"][0])
    print("liquid particle run losses", got, "reference", np.asarray(hist), "rel", np.abs(got - hist) / np.abs(hist))
    assert got.shape == (3 * F,)
    np.testing.assert_allclose(got, hist, rtol=1e-3)
    for t in range(F):
        assert rel(res["opt"][t], g_opt[t]) <= 1e-3
    assert res["r"].shape == (F, RES[1], RES[2], 3) and res["r"].dtype == np.uint8 and len(np.unique(res["r"])) > 8
    # the float64 image of the result at the identity view, over the background: 'r' is its truncation up to float32
    # rounding of a value in 0..255 (a level either way at a level's edge)
    for t in range(F):
        d = CR.grey_volume(torch.tensor(scene["p"][t]).double(), _ref_cfg(cfg), RES)
        eye = torch.eye(3, dtype=torch.float64)[None]
        w, tt, _ = LR.weights(d, eye, LR.tau_of(_ref_cfg(cfg)))
        _opaque_enough(1 - tt)
        q = CR.colour_volume(torch.tensor(scene["p"][t]).double(), torch.tensor(scene["r"][t]).double(),
                                torch.tensor(res["opt"][t]).double(), _ref_cfg(cfg), RES)
        img = 255 * torch.clamp(LR.image(q, eye, w, tt, BG), 0, 1)[0].numpy()
        assert np.abs(np.floor(img) - res["r"][t].astype(np.float64)).max() <= 1.0


# ---- default flags: what both paths computed before the flag -----------------------------------------------------------

def _gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "colour_liquid_unchanged.npz"))


def test_default_flags_keep_the_grid_path_bit_for_bit():
    """grid_variable 'c' without the new flags, 'tiled' transpose: the variables, the masked colours and the images of the
    commit before --colour_render, bit for bit (tests/golden/make_colour_liquid_fixture.py); the loss scalars to 1e-5, for
    the reason tests/test_colour_grid_stylizer_gpu.py gives at LOSS_RTOL"""
    gold, got = _gold(), LRUNS.unchanged_grid_run()
    np.testing.assert_allclose(got["l"], gold["grid_l"], rtol=G.LOSS_RTOL)
    for k in ("opt", "c", "r"):
        assert np.array_equal(got[k], gold["grid_" + k]), (k, np.abs(got[k].astype(np.float64) - gold["grid_" + k]).max())


def test_default_flags_keep_the_particle_path():
    """target_field 'c' without the new flags against the recorded run, to the tolerances of test_colour_stylizer_gpu's
    _same_run: its splat adds with float atomics, so two runs of one build differ by their order"""
    gold, got = _gold(), LRUNS.unchanged_particle_run()
    np.testing.assert_allclose(got["l"], gold["particle_l"], rtol=1e-5)
    for x, y in zip(got["opt"], gold["particle_opt"]):
        assert rel(x, y) <= 1e-5
    assert np.abs(got["r"].astype(np.int32) - gold["particle_r"].astype(np.int32)).max() <= 1

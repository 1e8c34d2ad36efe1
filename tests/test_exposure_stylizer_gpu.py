"""``colour_render 'exposure'`` on the stylizers: ``target_field 'pc'`` of styler_3p on the scene of tests/joint_runs.py with
the colour render overridden -- the gradient [N,6] of one frame against the float64 joint loss of tests/exposure_ref.py and
a 2-frame, 3-step ``Styler(config).run`` against the float64 loop -- and one ``target_field 'c'`` particle run and one
``grid_variable 'c'`` grid run against their float64 loops.

The 'pc' scene is taken at DENSITY SCALE 1 (the particles as they are, transmit 0.2): tests/test_exposure_cpu.py holds, on
the reference alone, that 1 - t of its rays reaches below 0.1 and above 0.5 and that the absorbing volume carries 0.60 of
|d loss / d v| (the bar is 0.1), so a gradient that left the new adjoint out could not pass 1e-3 here.  The grid run takes
the grid scene's densities times 2.5, as the liquid tests do.  Default-flag runs are held to their fixtures by the existing
tests."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import colour_ref as CR
from tests import exposure_ref as ER
from tests import joint_runs as JR
from tests import test_colour_grid_stylizer_gpu as G
from tests import test_colour_liquid_stylizer_gpu as L

pytestmark = pytest.mark.gpu

RES = JR.RES
N = JR.N
rel = G.rel
KAPPA = 1.5


@pytest.fixture(scope="module")
def scene():
    return JR.scene()


def _styler(F=1, **over):
    from neural_flow_style_amd.styler_3p import Styler
    kw = dict(colour_render="exposure")
    kw.update(over)
    cfg = JR.config(F=F, **kw)
    st = Styler(cfg)
    st.load_img(RES[1:])
    return st, cfg


def _ref(scene, cfg, t, v, c, R):
    return ER.joint_loss_and_grad(torch.tensor(scene["p"][t]).double(), torch.tensor(scene["r"][t]).double(), v, c,
                                  JR.ref_cfg(cfg), RES, R, scene["w64"], scene["sfe"])


def _var(st, v, c, scale=1.0):
    return st._dev(np.concatenate([np.asarray(v, np.float32), np.asarray(c, np.float32) / np.float32(scale)], 1))


@pytest.mark.parametrize("mode,v_batch,w_tv,kappa", [("sequential", 1, 0.0, 1.0), ("sum", 3, 0.05, 1.0),
                                                     ("sum", 1, 0.05, KAPPA)])
def test_pc_gradient_of_one_frame(scene, mode, v_batch, w_tv, kappa):
    """d loss / d (v, c) [N,6] against the float64 joint loss: relative L2 <= 1e-3 on the whole, on the v columns and on
    the c columns, the summed loss within 1e-3; colours outside [0,1] get exactly zero"""
    st, cfg = _styler(views_mode=mode, v_batch=v_batch, w_tv=w_tv, colour_exposure=kappa)
    assert st._joint and st.colour.fixed_exposure and st.colour.exposure == kappa and st.loss is None
    st.colour.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    p, r = st._dev(scene["p"][0]), st._dev(scene["r"][0])
    v, c = scene["v"], scene["c_init"][0]
    var = _var(st, v, c)
    outside = torch.tensor((c < 0) | (c > 1))
    assert bool(outside.any())
    nv = len(st.rot_mat_)
    assert nv == 3
    batches = [(i, i + v_batch) for i in range(0, nv, v_batch)] if mode == "sequential" else [(0, nv)]
    for lo, hi in batches:
        losses, g = st._value_and_grad(p, r, var, RES, st._rot(lo, hi), view_shard=False)
        assert tuple(losses.shape) == (hi - lo,) and tuple(g.shape) == (N, 6)
        l_ref, gv_ref, gc_ref = _ref(scene, cfg, 0, v, c, st.rot_mat_[lo:hi])
        g = g.cpu()
        ra, rv, rc = rel(g, torch.cat([gv_ref, gc_ref], 1)), rel(g[:, :3], gv_ref), rel(g[:, 3:], gc_ref)
        rl = abs(float(losses.sum()) - l_ref) / abs(l_ref)
        print("exposure joint gradient %s v_batch %d tv %g kappa %g views %d:%d  rel-L2 %.3g (v %.3g, c %.3g)  loss rel %.3g"
              % (mode, v_batch, w_tv, kappa, lo, hi, ra, rv, rc, rl))
        assert float(gv_ref.abs().max()) > 0 and float(gc_ref.abs().max()) > 0
        assert ra <= 1e-3, ra
        assert rv <= 1e-3, rv
        assert rc <= 1e-3, rc
        assert rl <= 1e-3, rl
        assert float(g[:, 3:][outside].abs().max()) == 0.0


def test_pc_run_follows_the_float64_loop_and_its_loss_falls(scene):
    """3 Adam steps, 2 frames, window_sigma = 1, the sequential view loop: the per-step losses follow the float64 loop to
    LOSS_RTOL and the loss falls; 'opt' within 1e-3 relative L2 per column block; 'p' is params p + 'v'"""
    F = scene["F"]
    st, cfg = _styler(F=F, iter=3, window_sigma=1.0, lr=0.002, w_tv=0.01)
    res = st.run({"p": scene["p"], "r": scene["r"], "c_init": scene["c_init"]})
    g_opt = [torch.cat([torch.zeros(N, 3, dtype=torch.float64), torch.tensor(scene["c_init"][t]).double()], 1)
             for t in range(F)]
    opt = [O.TFAdam() for _ in range(F)]
    Wt = O.temporal_filter_matrix(F, cfg.window_sigma)
    hist = []
    for _ in range(3):
        upd = []
        for t in range(F):
            var, acc, ls = g_opt[t].clone(), 0.0, []
            for i in range(len(st.rot_mat_)):
                l, g_v, g_c = _ref(scene, cfg, t, var[:, :3], var[:, 3:], st.rot_mat_[i:i + 1])
                var = opt[t].step(var, torch.cat([g_v, g_c], 1), cfg.lr)
                ls.append(l)
                acc = acc + torch.nan_to_num(var)
            hist.append(float(np.mean(ls)))
            upd.append(acc / len(st.rot_mat_) - g_opt[t])
        for t in range(F):
            g_opt[t] = g_opt[t] + sum(float(Wt[t, u]) * upd[u] for u in range(F))
    got = np.asarray(res["l"][0])
    print("exposure joint run losses", got, "reference", np.asarray(hist), "rel", np.abs(got - hist) / np.abs(hist))
    assert got.shape == (3 * F,)
    np.testing.assert_allclose(got, hist, rtol=G.LOSS_RTOL)
    for t in range(F):
        assert got[2 * F + t] < got[t], (t, got)
        assert res["opt"][t].shape == (N, 6)
        rv, rc = rel(res["opt"][t][:, :3], g_opt[t][:, :3]), rel(res["opt"][t][:, 3:], g_opt[t][:, 3:])
        print("frame %d 'opt' rel-L2: v %.3g  c %.3g" % (t, rv, rc))
        assert rv <= 1e-3 and rc <= 1e-3
        assert np.array_equal(res["v"][t], res["opt"][t][:, :3]) and float(np.abs(res["v"][t]).max()) > 0
        np.testing.assert_allclose(res["p"][t], scene["p"][t] + res["v"][t], rtol=0, atol=1e-7)
    assert res["r"].shape == (F, RES[1], RES[2], 3) and res["r"].dtype == np.uint8 and len(np.unique(res["r"])) > 8


def _pref_loss_grad(scene, cfg, t, c, R):
    c64 = torch.tensor(np.asarray(c, np.float64), requires_grad=True)
    l = ER.particle_frame_loss(torch.tensor(scene["p"][t]).double(), torch.tensor(scene["r"][t]).double(), c64,
                               dict(vars(cfg)), RES, torch.tensor(np.asarray(R, np.float32)).double(), scene["w64"],
                               scene["sfe"])
    (g,) = torch.autograd.grad(l, c64)
    return float(l.detach()), g


def test_particle_colour_run_against_the_float64_loop(scene):
    """target_field 'c' under 'exposure' (kappa = 1.5, the mask clip(grey, 0, 1) on): 2 Adam steps, 2 frames, window_sigma
    > 0, the sequential view loop: per-step losses and the variables within 1e-3 of the float64 loop (BASELINE's bar, as
    the liquid run's); the context is formed once per frame and view set"""
    F = scene["F"]
    st, cfg = _styler(F=F, target_field="c", iter=2, window_sigma=1.0, lr=0.01, style_mask=True, w_tv=0.01,
                      colour_exposure=KAPPA)
    assert st._colour and st.colour.fixed_exposure
    res = st.run({"p": scene["p"], "r": scene["r"], "c_init": scene["c_init"]})
    g_opt = [torch.tensor(scene["c_init"][t]).double() for t in range(F)]
    opt = [O.TFAdam() for _ in range(F)]
    Wt = O.temporal_filter_matrix(F, cfg.window_sigma)
    hist = []
    for _ in range(2):
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
    print("exposure particle run losses", got, "reference", np.asarray(hist), "rel", np.abs(got - hist) / np.abs(hist))
    assert got.shape == (2 * F,)
    np.testing.assert_allclose(got, hist, rtol=1e-3)
    for t in range(F):
        assert rel(res["opt"][t], g_opt[t]) <= 1e-3
    assert res["r"].shape == (F, RES[1], RES[2], 3) and res["r"].dtype == np.uint8 and len(np.unique(res["r"])) > 8
    # over black: the float64 image of the result at the identity view ('r' is its truncation up to a level either way)
    rc_ = dict(vars(cfg))
    eye = torch.eye(3, dtype=torch.float64)[None]
    for t in range(F):
        d = CR.grey_volume(torch.tensor(scene["p"][t]).double(), rc_, RES)
        w, _, _ = ER.weights(d, eye, ER.tau_of(rc_), ER.kappa_of(rc_))
        q = CR.colour_volume(torch.tensor(scene["p"][t]).double(), torch.tensor(scene["r"][t]).double(),
                             torch.tensor(res["opt"][t]).double(), rc_, RES)
        img = 255 * torch.clamp(CR.image(q, eye, w), 0, 1)[0].numpy()
        assert np.abs(np.floor(img) - res["r"][t].astype(np.float64)).max() <= 1.0


def test_grid_colour_run_against_the_float64_loop():
    """grid_variable 'c' under 'exposure' (kappa = 1.5, the mask on): 2 frames, 2 Adam steps, window_sigma = 1 with
    simulation velocities: per-step losses and the variables within 1e-3 of the float64 loop; one context per frame"""
    sc = G.scene()
    st, cfg = G._styler(F=2, iter=2, window_sigma=1.0, lr=0.01, style_mask=True, w_tv=0.01, colour_render="exposure",
                        colour_exposure=KAPPA, transmit=L.TRANSMIT, colour_background=[0.2, 0.6, 0.05])
    assert st.loss.fixed_exposure and st.loss.exposure == KAPPA
    res = st.run(L._gparams(2))
    hist, g_ref = ER.grid_sequence_run(dict(vars(cfg)), [L._gdens(0), L._gdens(1)], np.stack(sc["u"][:2]), sc["w64"],
                                       sc["sfe"], st.rot_mat_, sc["c_init"])
    got = np.asarray(res["l_frames"])
    print("exposure grid run losses", got, "reference", np.asarray(hist), "rel", np.abs(got - hist) / np.abs(hist))
    assert got.shape == (2, 2)
    np.testing.assert_allclose(got, hist, rtol=1e-3)
    for t in range(2):
        r_ = rel(res["opt"][t], g_ref[t])
        print("frame %d variable rel-L2 %.3g" % (t, r_))
        assert r_ <= 1e-3, (t, r_)
    # over black whatever colour_background says: a transparent corner pixel is black
    assert int(res["r"][:, 0, 0].max()) <= 1

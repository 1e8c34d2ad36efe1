"""``target_field 'pc'`` of styler_3p: positions and colours of a liquid in one variable [N,6].  The gradient of one frame's
loss against the float64 joint loss of tests/absorb_ref.py (the displacement and the colour columns separately), the
colour columns' scale, ``Styler(config).run`` against the float64 loop, and a two-octave run.

The scene is tests/joint_runs.py's: the particle scene of the colour tests displaced by up to 0.02 of the domain (a third of
a cell), 17 x 12 x 12, three uniform views, transmit 0.2, a non-white background, no mask.  tests/test_absorb_cpu.py holds, on
the reference alone, that its grey liquid image has pixels below 0.1 and above 0.5 and that the absorbing volume carries 0.31
of |d loss / d v|: a gradient that left the new kernel out could not pass the 1e-3 bar here."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import absorb_ref as AR
from tests import colour_liquid_ref as LR
from tests import colour_ref as CR
from tests import joint_runs as JR

pytestmark = pytest.mark.gpu

RES = JR.RES
N = JR.N


def rel(a, b):
    a = torch.as_tensor(np.asarray(a)).double(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.fixture(scope="module")
def scene():
    return JR.scene()


def _styler(F=1, **over):
    from neural_flow_style_amd.styler_3p import Styler
    cfg = JR.config(F=F, **over)
    st = Styler(cfg)
    st.load_img(RES[1:])
    return st, cfg


def _ref(scene, cfg, t, v, c, R):
    return AR.joint_loss_and_grad(torch.tensor(scene["p"][t]).double(), torch.tensor(scene["r"][t]).double(), v, c,
                                  JR.ref_cfg(cfg), RES, R, scene["w64"], scene["sfe"])


def _var(st, v, c, scale=1.0):
    return st._dev(np.concatenate([np.asarray(v, np.float32), np.asarray(c, np.float32) / np.float32(scale)], 1))


@pytest.mark.parametrize("mode,v_batch,w_tv,w_pressure", [("sequential", 1, 0.0, 0.0), ("sequential", 1, 0.05, 0.0),
                                                          ("sum", 1, 0.05, 0.0), ("sum", 3, 0.0, 0.0),
                                                          ("sum", 3, 0.05, 0.0), ("sum", 1, 0.05, 1e7)])
def test_gradient_of_one_frame(scene, mode, v_batch, w_tv, w_pressure):
    """d loss / d (v, c) against the float64 joint loss: relative L2 <= 1e-3 on the v columns and on the c columns
    separately, the summed loss within 1e-3, per view batch in the sequential mode and for the summed views; colours
    outside [0,1] get exactly zero.  w_pressure = 1e7 puts the pressure term beside the style term of the synthetic weights
    (4e6 here): in float64 it is 0.6 of the loss and its gradient a fifth of |d loss / d v|"""
    st, cfg = _styler(views_mode=mode, v_batch=v_batch, w_tv=w_tv, w_pressure=w_pressure)
    assert st._joint and st.colour.liquid and st.loss is None
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
        rv, rc = rel(g[:, :3], gv_ref), rel(g[:, 3:], gc_ref)
        rl = abs(float(losses.sum()) - l_ref) / abs(l_ref)
        print("joint gradient %s v_batch %d tv %g pressure %g views %d:%d  v rel-L2 %.3g  c rel-L2 %.3g  loss rel %.3g"
              % (mode, v_batch, w_tv, w_pressure, lo, hi, rv, rc, rl))
        assert float(gv_ref.abs().max()) > 0 and float(gc_ref.abs().max()) > 0
        assert rv <= 1e-3, rv
        assert rc <= 1e-3, rc
        assert rl <= 1e-3, rl
        assert float(g[:, 3:][outside].abs().max()) == 0.0
    if w_pressure:
        # the term is there: the same evaluation without it differs
        st0, _ = _styler(views_mode=mode, v_batch=v_batch, w_tv=w_tv)
        st0.colour.image_loss.set_style_image(st0._style_feature(st0.style_img, RES[1:]))
        _, g0 = st0._value_and_grad(p, r, var, RES, st0._rot(0, nv), view_shard=False)
        assert rel(g0.cpu()[:, :3], g[:, :3]) > 1e-2


def test_in_a_grid_order_it_is_the_same_gradient(scene):
    """the splats see the particles through a permutation (``_particle_order``); the gradient comes back in the caller's
    order: against the float64 loss as above"""
    from neural_flow_style_amd import transform as T
    st, cfg = _styler(views_mode="sum", v_batch=3, w_tv=0.05)
    st.colour.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    p, r = st._dev(scene["p"][0]), st._dev(scene["r"][0])
    v, c = scene["v"], scene["c_init"][0]
    st._orders = {(p.data_ptr(), p.shape[0]): T.grid_order(p, st.resolution)}
    assert not torch.equal(st._orders[(p.data_ptr(), p.shape[0])].cpu(), torch.arange(N))
    losses, g = st._value_and_grad(p, r, _var(st, v, c), RES, st._rot(0, 3), view_shard=False)
    l_ref, gv_ref, gc_ref = _ref(scene, cfg, 0, v, c, st.rot_mat_)
    g = g.cpu()
    rv, rc = rel(g[:, :3], gv_ref), rel(g[:, 3:], gc_ref)
    print("joint gradient in grid order: v rel-L2 %.3g  c rel-L2 %.3g" % (rv, rc))
    assert rv <= 1e-3 and rc <= 1e-3 and abs(float(losses.sum()) - l_ref) <= 1e-3 * abs(l_ref)


def test_colour_lr_scale_scales_the_colour_columns(scene):
    """the variable stores c / s and its gradient's colour columns are s g_c: at s = 5 five times those at s = 1, the
    displacement columns the same.  Tolerance 1e-4 relative L2: the stored colours are rounded once more (c / 5 * 5, 1e-7)
    and the splats add with float atomics in an order of their own (1e-6); both are orders below it"""
    v, c = scene["v"], scene["c_init"][0]
    out = {}
    for s in (1.0, 5.0):
        st, cfg = _styler(views_mode="sum", v_batch=3, w_tv=0.05, colour_lr_scale=s)
        st.colour.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
        p, r = st._dev(scene["p"][0]), st._dev(scene["r"][0])
        out[s] = st._value_and_grad(p, r, _var(st, v, c, s), RES, st._rot(0, 3), view_shard=False)[1].cpu()
    assert float(out[1.0][:, 3:].abs().max()) > 0
    assert rel(out[5.0][:, 3:], 5.0 * out[1.0][:, 3:]) <= 1e-4
    assert rel(out[5.0][:, :3], out[1.0][:, :3]) <= 1e-4


def test_run_against_the_float64_loop(scene):
    """3 Adam steps, 2 frames, window_sigma = 1, the sequential view loop, colour_lr_scale = 5: per-step losses within 1e-3
    of the float64 loop written out as in test_particle_run_against_the_float64_loop, 'opt' within 1e-3 relative L2 per
    column block; 'p' is params p + 'v'; 'r' is over the background; the loss falls"""
    F, s = scene["F"], 5.0
    st, cfg = _styler(F=F, iter=3, window_sigma=1.0, lr=0.002, w_tv=0.01, colour_lr_scale=s)
    res = st.run({"p": scene["p"], "r": scene["r"], "c_init": scene["c_init"]})
    g_opt = [torch.cat([torch.zeros(N, 3, dtype=torch.float64), torch.tensor(scene["c_init"][t]).double() / s], 1)
             for t in range(F)]
    opt = [O.TFAdam() for _ in range(F)]
    Wt = O.temporal_filter_matrix(F, cfg.window_sigma)
    hist = []
    for _ in range(3):
        upd = []
        for t in range(F):
            var, acc, ls = g_opt[t].clone(), 0.0, []
            for i in range(len(st.rot_mat_)):
                l, g_v, g_c = _ref(scene, cfg, t, var[:, :3], var[:, 3:] * s, st.rot_mat_[i:i + 1])
                var = opt[t].step(var, torch.cat([g_v, s * g_c], 1), cfg.lr)
                ls.append(l)
                acc = acc + torch.nan_to_num(var)
            hist.append(float(np.mean(ls)))
            upd.append(acc / len(st.rot_mat_) - g_opt[t])
        for t in range(F):
            g_opt[t] = g_opt[t] + sum(float(Wt[t, u]) * upd[u] for u in range(F))
    got = np.asarray(res["l"][0])
    print("joint run losses", got, "reference", np.asarray(hist), "rel", np.abs(got - hist) / np.abs(hist))
    assert got.shape == (3 * F,)
    np.testing.assert_allclose(got, hist, rtol=1e-3)
    for t in range(F):
        assert got[2 * F + t] < got[t], (t, got)
        assert res["opt"][t].shape == (N, 6)
        rv, rc = rel(res["opt"][t][:, :3], g_opt[t][:, :3]), rel(res["opt"][t][:, 3:], g_opt[t][:, 3:] * s)
        print("frame %d 'opt' rel-L2: v %.3g  c %.3g" % (t, rv, rc))
        assert rv <= 1e-3 and rc <= 1e-3
        assert np.array_equal(res["v"][t], res["opt"][t][:, :3])
        np.testing.assert_allclose(res["p"][t], scene["p"][t] + res["v"][t], rtol=0, atol=1e-7)
        want_c = np.clip(res["opt"][t][:, 3:], 0, 1) * np.clip(scene["r"][t] / np.float32(cfg.rest_density), 0, 1)
        np.testing.assert_allclose(res["c"][t], want_c, rtol=0, atol=1e-6)
    assert np.array_equal(res["c_init"], scene["c_init"])
    assert res["d"].shape == (F,) + tuple(RES) + (1,)
    assert res["r"].shape == (F, RES[1], RES[2], 3) and res["r"].dtype == np.uint8 and len(np.unique(res["r"])) > 8
    # the float64 image of the result at the identity view, over the background: 'r' is its truncation up to float32
    # rounding of a value in 0..255 (a level either way at a level's edge)
    rc_ = JR.ref_cfg(cfg)
    eye = torch.eye(3, dtype=torch.float64)[None]
    for t in range(F):
        x = torch.tensor(scene["p"][t]).double() + torch.tensor(res["v"][t]).double()
        e = O.smooth3d_relu(AR.raw_volume(x, rc_, RES), cfg.k)[0, ..., 0]
        w, tt, _ = LR.weights(e, eye, LR.tau_of(rc_))
        q = CR.colour_volume(x, torch.tensor(scene["r"][t]).double(), torch.tensor(res["opt"][t][:, 3:]).double(), rc_, RES)
        img = 255 * torch.clamp(LR.image(q, eye, w, tt, JR.BG), 0, 1)[0].numpy()
        assert np.abs(np.floor(img) - res["r"][t].astype(np.float64)).max() <= 1.0


def test_two_octaves_complete_with_colour_intermediates(scene):
    F = scene["F"]
    st, cfg = _styler(F=F, iter=2, window_sigma=1.0, lr=0.002, w_tv=0.01, octave_n=2, octave_scale=1.5, views_mode="sum",
                      v_batch=3)
    res = st.run({"p": scene["p"], "r": scene["r"], "c_init": scene["c_init"]})
    assert len(res["l"]) == 2 and all(len(l) == 2 * F and np.isfinite(l).all() for l in res["l"])
    assert len(res["d_intm"]) == 1 and res["d_intm"][0].shape == (F, 8, 8, 3) and res["d_intm"][0].dtype == np.uint8
    assert len(np.unique(res["d_intm"][0])) > 8
    assert not np.array_equal(res["d_intm"][0][..., 0], res["d_intm"][0][..., 1])         # (in colour, not grey)
    assert res["opt"][0].shape == (N, 6) and res["r"].shape == (F, RES[1], RES[2], 3)
    assert float(np.abs(res["v"][0]).max()) > 0

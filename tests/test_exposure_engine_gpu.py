"""``engine.ColourRenderLoss(render='exposure')`` and its ``loss_and_grad(absorb=True)``: the gradient in the absorbing volume
against float64 autograd of the fixed-exposure model (tests/exposure_ref.py) at a constant emission, as
tests/test_absorb_engine_gpu.py holds the liquid's: the same scene (the colour grid tests', 17 x 12 x 12, the densities times
2.5 as there, transmit 0.2), three views, v_batch 1 and 3, w_tv 0 and 0.05, no mask; the emission's gradient is that of
absorb=False bit for bit on the 'tiled' route and the losses are to the order of their float atomics; the context is spent;
the style_mask refusal.  kappa = 1.5."""
import numpy as np
import pytest
import torch

from tests import colour_grid_ref as GR
from tests import colour_liquid_ref as LR
from tests import colour_ref as CR
from tests import exposure_ref as ER
from tests import test_colour_grid_stylizer_gpu as G
from tests import test_colour_liquid_stylizer_gpu as L

pytestmark = pytest.mark.gpu

RES = G.RES
rel = G.rel
KAPPA = 1.5
EXPOSURE = dict(colour_render="exposure", colour_exposure=KAPPA, transmit=L.TRANSMIT)


def _setup(**over):
    """the exposure grid styler's loss, the smoothed volume e, the emission q of the scene's first colours"""
    from neural_flow_style_amd import ops
    kw = dict(EXPOSURE)
    kw.update(over)
    st, cfg = G._styler(**kw)
    st.loss.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    e = ops.smooth3d_relu_fwd(st._dev(L._gdens(0)), float(cfg.k))
    q = ops.emission_fwd(st._dev(G.scene()["c_init"][0]), e)
    return st, cfg, e, q


@pytest.mark.parametrize("v_batch,w_tv", [(1, 0.0), (1, 0.05), (3, 0.0), (3, 0.05)])
def test_gradient_in_the_absorbing_volume(v_batch, w_tv):
    """g_d against float64 autograd: relative L2 <= 1e-3 and the summed loss within 1e-3 (BASELINE's gradient bar); g_q
    equals that of absorb=False with the 'tiled' route bit for bit, the losses to LOSS_RTOL"""
    sc = G.scene()
    st, cfg, e, q = _setup(v_batch=v_batch, w_tv=w_tv, style_mask=False)
    loss, rot = st.loss, st._rot()
    assert loss.fixed_exposure and not loss.liquid and loss.exposure == KAPPA and len(st.rot_mat_) == 3
    ctx0 = loss.prepare(e, rot)
    assert ctx0["gmax"] is None and set(ctx0) == {"rot", "w", "grey", "d_gray", "gmax"}
    assert tuple(ctx0["w"].shape) == (3,) + tuple(RES) and tuple(ctx0["d_gray"].shape) == (3,) + tuple(RES[1:]) + (1,)
    assert torch.equal(ctx0["d_gray"][..., 0], torch.clamp(ctx0["grey"], 0, 1))
    print("grey image in [%.3f, %.3f]" % (float(ctx0["grey"].min()), float(ctx0["grey"].max())))
    losses0, g_q0 = loss.loss_and_grad(q, ctx0, route="tiled")
    assert not ctx0.get("spent")
    ctx = loss.prepare(e, rot)
    losses, g_q, g_d = loss.loss_and_grad(q, ctx, route="tiled", absorb=True)
    # g_q bit for bit; the loss scalars of two runs of the SAME launches differ by the order of their float atomics (the
    # reason and the bound at tests/test_colour_grid_stylizer_gpu.py's LOSS_RTOL)
    assert torch.equal(g_q, g_q0)
    np.testing.assert_allclose(losses.cpu().numpy(), losses0.cpu().numpy(), rtol=G.LOSS_RTOL)
    assert tuple(g_d.shape) == tuple(RES) and ctx["spent"]
    with pytest.raises(ValueError, match="spent"):
        loss.loss_and_grad(q, ctx, route="tiled")
    # float64: the emission held constant, the volume the variable, the views v_batch at a time
    rc = dict(vars(cfg))
    e64 = GR.grey(L._gdens(0), cfg.k).clone().requires_grad_()
    q64 = GR.emission(torch.tensor(np.asarray(sc["c_init"][0], np.float64)), e64.detach())
    R = torch.as_tensor(np.asarray(st.rot_mat_, np.float32)).double()
    assert ER.kappa_of(rc) == KAPPA
    # the volume is opaque enough for the absorption to matter: 1 - t of the float64 samples, as the liquid tests hold it
    _, _, S64 = ER.weights(e64.detach(), R, ER.tau_of(rc), KAPPA)
    L._opaque_enough(1 - torch.exp(-ER.tau_of(rc) * S64.sum(1)))
    l_ref = 0.0
    for Rb in LR._view_batches(rc, R):
        w, _, _ = ER.weights(e64, Rb, ER.tau_of(rc), ER.kappa_of(rc))
        l_ref = l_ref + CR.image_loss(torch.clamp(CR.image(q64, Rb, w), 0, 1), None, rc, sc["w64"], sc["sfe"])
    (g_ref,) = torch.autograd.grad(l_ref, e64)
    rg, rl = rel(g_d.cpu(), g_ref), abs(float(losses.sum()) - float(l_ref.detach())) / abs(float(l_ref.detach()))
    print("exposure absorb gradient v_batch %d tv %g: rel-L2 %.3g  loss rel %.3g  |g_d| %.3g"
          % (v_batch, w_tv, rg, rl, float(g_ref.norm())))
    assert float(g_ref.abs().max()) > 0
    assert rg <= 1e-3, rg
    assert rl <= 1e-3, rl


def test_absorb_is_refused_with_the_mask_and_the_background_has_no_effect():
    st, cfg, e, q = _setup(style_mask=True)
    ctx = st.loss.prepare(e, st._rot())
    with pytest.raises(ValueError, match="style_mask.*clip\\(grey"):
        st.loss.loss_and_grad(q, ctx, absorb=True)
    assert not ctx.get("spent")
    losses, g_q = st.loss.loss_and_grad(q, ctx, route="tiled")                    # (the masked path without absorb goes on)
    assert bool(torch.isfinite(losses).all())
    st2, _, _, _ = _setup(style_mask=True, colour_background=[0.2, 0.6, 0.05])
    ctx2 = st2.loss.prepare(e, st2._rot())
    assert torch.equal(ctx2["w"], ctx["w"]) and torch.equal(ctx2["grey"], ctx["grey"])
    J, img = st.loss.project(q, ctx)
    J2, _ = st2.loss.project(q, ctx2)
    assert torch.equal(J, J2) and torch.equal(img, torch.clamp(J, 0, 1))
    losses2, g_q2 = st2.loss.loss_and_grad(q, ctx2, route="tiled")
    assert torch.equal(g_q2, g_q)
    np.testing.assert_allclose(losses2.cpu().numpy(), losses.cpu().numpy(), rtol=G.LOSS_RTOL)

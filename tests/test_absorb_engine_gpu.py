"""``engine.ColourRenderLoss.loss_and_grad(absorb=True)``: the gradient in the absorbing volume against float64 autograd of
the liquid model (tests/colour_liquid_ref.py) at a constant emission, on the scene of the colour grid tests (17 x 12 x 12, the
densities times 2.5 so that the liquid is opaque enough at transmit 0.2: tests/test_colour_liquid_stylizer_gpu.py), three
views, no mask; the emission's gradient is that of absorb=False bit for bit and the losses are to the order of their float
atomics; the context is spent; the two refusals."""
import numpy as np
import pytest
import torch

from tests import colour_grid_ref as GR
from tests import colour_liquid_ref as LR
from tests import colour_ref as CR
from tests import test_colour_grid_stylizer_gpu as G
from tests import test_colour_liquid_stylizer_gpu as L

pytestmark = pytest.mark.gpu

RES = G.RES
rel = G.rel


def _setup(**over):
    """the liquid grid styler's loss, the smoothed volume e, the emission q of the scene's first colours and the views"""
    from neural_flow_style_amd import ops
    st, cfg = L._gstyler(style_mask=False, **over)
    st.loss.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    e = ops.smooth3d_relu_fwd(st._dev(L._gdens(0)), float(cfg.k))
    q = ops.emission_fwd(st._dev(G.scene()["c_init"][0]), e)
    return st, cfg, e, q


@pytest.mark.parametrize("v_batch,w_tv", [(1, 0.0), (1, 0.05), (3, 0.0), (3, 0.05)])
def test_gradient_in_the_absorbing_volume(v_batch, w_tv):
    """g_d against float64 autograd: relative L2 <= 1e-3 and the summed loss within 1e-3 (BASELINE's gradient bar); g_q
    equals that of absorb=False with the 'tiled' route bit for bit, the losses to LOSS_RTOL"""
    sc = G.scene()
    st, cfg, e, q = _setup(v_batch=v_batch, w_tv=w_tv)
    loss, rot = st.loss, st._rot()
    assert loss.liquid and len(st.rot_mat_) == 3
    ctx0 = loss.prepare(e, rot)
    L._opaque_enough(ctx0["grey"])
    losses0, g_q0 = loss.loss_and_grad(q, ctx0, route="tiled")
    assert not ctx0.get("spent")
    ctx = loss.prepare(e, rot)
    assert ctx["d3"] is e
    losses, g_q, g_d = loss.loss_and_grad(q, ctx, route="tiled", absorb=True)
    # g_q bit for bit.  The loss scalars of two runs of the SAME launches differ by the order of their float atomics (the
    # reason and the bound at tests/test_colour_grid_stylizer_gpu.py's LOSS_RTOL), so they are held to that bound: the two
    # calls issue the same launches up to this point
    assert torch.equal(g_q, g_q0)
    np.testing.assert_allclose(losses.cpu().numpy(), losses0.cpu().numpy(), rtol=G.LOSS_RTOL)
    assert tuple(g_d.shape) == tuple(RES) and ctx["spent"]
    with pytest.raises(ValueError, match="spent"):
        loss.loss_and_grad(q, ctx, route="tiled")
    # float64: the emission held constant, the volume the variable, the views v_batch at a time
    rc = L._ref_cfg(cfg)
    e64 = GR.grey(L._gdens(0), cfg.k).clone().requires_grad_()
    q64 = GR.emission(torch.tensor(np.asarray(sc["c_init"][0], np.float64)), e64.detach())
    R = torch.as_tensor(np.asarray(st.rot_mat_, np.float32)).double()
    l_ref = 0.0
    for Rb in LR._view_batches(rc, R):
        w, t, _ = LR.weights(e64, Rb, LR.tau_of(rc))
        img = torch.clamp(LR.image(q64, Rb, w, t, LR.background_of(rc)), 0, 1)
        l_ref = l_ref + CR.image_loss(img, None, rc, sc["w64"], sc["sfe"])
    (g_ref,) = torch.autograd.grad(l_ref, e64)
    rg, rl = rel(g_d.cpu(), g_ref), abs(float(losses.sum()) - float(l_ref.detach())) / abs(float(l_ref.detach()))
    print("absorb gradient v_batch %d tv %g: rel-L2 %.3g  loss rel %.3g  |g_d| %.3g" % (v_batch, w_tv, rg, rl, float(g_ref.norm())))
    assert float(g_ref.abs().max()) > 0
    assert rg <= 1e-3, rg
    assert rl <= 1e-3, rl


def test_absorb_is_refused_on_the_smoke_render_and_with_the_mask():
    from neural_flow_style_amd import ops
    st, cfg = G._styler(transmit=L.TRANSMIT, style_mask=False)                    # the smoke colour render
    st.loss.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    e = ops.smooth3d_relu_fwd(st._dev(L._gdens(0)), float(cfg.k))
    q = ops.emission_fwd(st._dev(G.scene()["c_init"][0]), e)
    assert not st.loss.liquid
    with pytest.raises(ValueError, match="smoke colour render.*maximum"):
        st.loss.loss_and_grad(q, st.loss.prepare(e, st._rot()), absorb=True)
    st, cfg = L._gstyler(style_mask=True)
    st.loss.image_loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    ctx = st.loss.prepare(e, st._rot())
    with pytest.raises(ValueError, match="style_mask.*mask 1 - t"):
        st.loss.loss_and_grad(q, ctx, absorb=True)
    assert not ctx.get("spent")
    losses, g_q = st.loss.loss_and_grad(q, ctx)                                   # (today's path goes on)
    assert bool(torch.isfinite(losses).all())

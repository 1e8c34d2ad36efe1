"""The colour view path's float64 restatement (tests/colour_ref.py) against itself: the two identities that pin the model
-- the grey limit and the transpose -- linearity of the projection, and the hand-written adjoint chain against
torch.autograd through the oracle's own rotate and splat."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import colour_ref as CR
from tests import view_ref as VR

TAU = 0.3


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.fixture(scope="module", params=CR.SHAPES, ids=str)
def scene(request):
    res = list(request.param)
    cfg = CR.splat_cfg(res, k=0)
    p, r, c = CR.particles(300, 3)
    R = CR.views()[:3].double()
    d = CR.grey_volume(p, cfg, res)
    w, I, M = CR.weights(d, R, TAU, v_batch=1)
    return dict(res=res, cfg=cfg, p=p, r=r, c=c, R=R, d=d, w=w, I=I, M=M)


def test_grey_limit(scene):
    """c = 1, pd = rest_density, k = 0: every channel of J is the grey path's normalised render I / M"""
    s = scene
    ones = torch.ones_like(s["c"])
    rho = torch.full_like(s["r"], s["cfg"]["rest_density"])
    q = CR.colour_volume(s["p"], rho, ones, s["cfg"], s["res"])
    J = CR.image(q, s["R"], s["w"])
    grey = s["I"] / s["M"].reshape(-1, 1, 1)
    for ch in range(3):
        assert _rel(J[..., ch], grey) <= 1e-12
    Js, _ = CR.project_all(s["R"], q, s["w"])                     # ... and so is the stencil restatement's
    assert _rel(Js, grey.unsqueeze(-1).expand_as(Js)) <= 1e-12


def test_transpose(scene):
    """<A q, g> = <q, A^T g>"""
    s = scene
    gen = torch.Generator().manual_seed(4)
    q = CR.colour_volume(s["p"], s["r"], s["c"], s["cfg"], s["res"])
    g = torch.randn(s["w"].shape[:1] + s["w"].shape[2:] + (3,), generator=gen, dtype=torch.float64)
    J, _ = CR.project_all(s["R"], q, s["w"])
    lhs = float((J * g).sum())
    rhs = float((q * CR.transpose_ref(s["R"], g, s["w"])).sum())
    scale = float((J.abs() * g.abs()).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


def test_stencil_and_oracle_projections_agree(scene):
    s = scene
    q = CR.colour_volume(s["p"], s["r"], s["c"], s["cfg"], s["res"])
    J, _ = CR.project_all(s["R"], q, s["w"])
    assert _rel(J, CR.image(q, s["R"], s["w"])) <= 1e-10


def test_linearity(scene):
    s = scene
    gen = torch.Generator().manual_seed(5)
    q1 = torch.rand(tuple(s["res"]) + (3,), generator=gen, dtype=torch.float64)
    q2 = torch.randn(tuple(s["res"]) + (3,), generator=gen, dtype=torch.float64)
    A = lambda q: CR.project_all(s["R"], q, s["w"])[0]
    lhs = A(2.5 * q1 - 0.75 * q2)
    rhs = 2.5 * A(q1) - 0.75 * A(q2)
    assert _rel(lhs, rhs) <= 1e-12
    assert float(A(torch.zeros_like(q1)).abs().max()) == 0.0


def test_ray_weight_and_projection_bounds_are_positive_and_small(scene):
    """the float32 bounds of an exact input: a few ulps of the value, never zero where the value is not"""
    s = scene
    S = CR.rotate(s["d"].unsqueeze(-1), s["R"])[..., 0]
    for v in range(S.shape[0]):
        w, ew = CR.ray_weights(S[v], torch.zeros_like(S[v]), TAU, s["M"][v])
        assert _rel(w, s["w"][v]) <= 1e-12
        assert bool((ew > 0).all()) and float((ew / w).max()) < 1e-4


@pytest.mark.parametrize("style_mask,w_tv", [(True, 0.0), (False, 0.05)])
def test_reference_gradient_against_autograd(style_mask, w_tv):
    """d loss / d c by the chain the engine runs -- A^T(clamp01_bwd(g_img)), the splat's adjoint, the colour clamp's --
    against torch.autograd through the oracle's rotate and splat, float64"""
    res = [17, 12, 12]
    layers = ["conv1_1", "conv2_1"]
    cfg = dict(CR.splat_cfg(res, k=3), style_layer=layers, w_style_layer=[1.0, 1.0], w_style=1.0, style_mask=style_mask,
               w_tv=w_tv, transmit=TAU, v_batch=1, resize_scale=1.0)
    p, r, c = CR.particles(400, 7)
    c = (c * 1.3 - 0.15).requires_grad_()                            # some colours outside [0,1]
    R = CR.views()[:3].double()
    rng = np.random.RandomState(1)
    w64 = {k: (np.asarray(a, np.float64), np.asarray(b, np.float64))
           for k, (a, b) in O.synthetic_vgg19_weights(123, upto="conv2_1").items()}
    simg = torch.tensor(rng.rand(1, 12, 12, 3) * 255)
    sfe = O.style_target_features(simg, w64, layers, upto="conv2_1")
    d = CR.grey_volume(p, cfg, res)
    loss = CR.frame_loss(p, r, c, cfg, res, R, w64, sfe, d=d)
    (g_auto,) = torch.autograd.grad(loss, c)

    # the explicit chain
    w, I, M = CR.weights(d, R, TAU, 1)
    d_gray = torch.clamp(I / M.reshape(-1, 1, 1), 0, 1).unsqueeze(-1)
    cc = torch.clamp(c.detach(), 0, 1).requires_grad_()
    q = O.p2g(p.unsqueeze(0), cfg["domain"], res, cfg["radius"], cfg["rest_density"], cfg["nsize"], pc=cc.unsqueeze(0),
              pd=r.unsqueeze(0), is_2d=False, clip=cfg["clip"], support=cfg["support"])[0]
    J, _ = CR.project_all(R, q.detach(), w)
    img = torch.clamp(J, 0, 1).requires_grad_()
    (g_img,) = torch.autograd.grad(CR.image_loss(img, d_gray, cfg, w64, sfe), img)
    g_J = torch.where((J >= 0) & (J <= 1), g_img, torch.zeros_like(g_img))
    g_q = CR.transpose_ref(R, g_J, w)
    (g_cc,) = torch.autograd.grad(q, cc, g_q)
    cd = c.detach()
    g_c = torch.where((cd >= 0) & (cd <= 1), g_cc, torch.zeros_like(g_cc))
    assert float(g_auto.abs().max()) > 0
    assert float((g_c - g_auto).norm() / g_auto.norm()) <= 1e-10
    outside = (cd < 0) | (cd > 1)
    assert bool(outside.any()) and float(g_auto[outside].abs().max()) == 0.0

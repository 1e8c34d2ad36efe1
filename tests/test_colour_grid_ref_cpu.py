"""tests/colour_grid_ref.py held to itself, without a GPU: its gradient against central differences, its exact zeros, the
float32 restatement of the two emission formulas, and planted defects that the checks must reject."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import colour_grid_ref as GR

RES = (6, 8, 8)
LAYERS = ["conv1_1", "conv2_1"]


@pytest.fixture(scope="module")
def problem():
    rng = np.random.RandomState(11)
    D, H, W = RES
    z, y, x = np.meshgrid(np.linspace(-1, 1, D), np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    d = (np.exp(-4 * (z ** 2 + y ** 2 + x ** 2)) * rng.uniform(0.5, 1.0, RES)).astype(np.float32)
    d[:, :, :2] = 0.0                                    # two planes of empty space: e == 0 on the outer one
    c = rng.uniform(0.1, 0.9, RES + (3,)).astype(np.float32)
    c[0, 3, 4, 0], c[1, 3, 4, 1], c[2, 4, 4, 2], c[3, 4, 5, 0] = -0.2, 1.3, -1.0, 2.0      # outside [0,1], e > 0 there
    simg = (rng.rand(H, W, 3) * 255).astype(np.float32)
    w64 = {k: (np.asarray(a, np.float64), np.asarray(b, np.float64))
           for k, (a, b) in O.synthetic_vgg19_weights(123, upto="conv2_1").items()}
    sfe = O.style_target_features(torch.tensor(np.asarray(simg, np.float64))[None], w64, LAYERS, upto="conv2_1")
    th = np.radians(10.0)
    rot = np.array([np.eye(3), [[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]], np.float32)
    cfg = dict(k=3, transmit=0.3, v_batch=1, style_layer=LAYERS, w_style_layer=[1, 1], w_style=1.0, style_mask=True,
               w_tv=0.05, resize_scale=1.0, upto="conv2_1", network="vgg_19.ckpt")
    return dict(d=d, c=c, cfg=cfg, rot=rot, w64=w64, sfe=sfe)


def test_gradient_against_central_differences(problem):
    """autograd's d loss / d c at voxels inside (0,1) against (L(c + h) - L(c - h)) / 2h in float64, h = 1e-5.
    The bar: truncation h^2 L''' / 6 and rounding 2^-53 L / h are both below 1e-9 of the gradient's scale; a ReLU or
    clip kink crossed within +-h leaves an error of the order of h times a slope jump, 1e-5 of that scale.  So 1e-4 of
    max |g| holds whichever happens, and a wrong chain is off by the order of the gradient itself."""
    p = problem
    l0, g = GR.loss_and_grad(p["d"], p["c"], p["cfg"], p["rot"], p["w64"], p["sfe"])
    assert np.isfinite(l0) and float(g.abs().max()) > 0
    e = GR.grey(p["d"], p["cfg"]["k"])
    live = [(2, 4, 4, 0), (3, 3, 5, 1), (1, 5, 3, 2), (4, 4, 4, 1)]
    assert all(float(e[i[:3]]) > 0 for i in live)
    h, scale = 1e-5, float(g.abs().max())
    c64 = torch.tensor(p["c"].astype(np.float64))
    for idx in live:
        vals = []
        for s in (+1, -1):
            cc = c64.clone()
            cc[idx] += s * h
            vals.append(float(GR.frame_loss(e, cc, p["cfg"], p["rot"], p["w64"], p["sfe"])))
        fd = (vals[0] - vals[1]) / (2 * h)
        print("central difference at %s: %.9g  autograd %.9g" % (idx, fd, float(g[idx])))
        assert abs(fd - float(g[idx])) <= 1e-4 * scale, (idx, fd, float(g[idx]))


def test_exact_zeros(problem):
    p = problem
    _, g = GR.loss_and_grad(p["d"], p["c"], p["cfg"], p["rot"], p["w64"], p["sfe"])
    e = GR.grey(p["d"], p["cfg"]["k"])
    outside = torch.tensor((p["c"] < 0) | (p["c"] > 1))
    empty = (e == 0).unsqueeze(-1).expand_as(g)
    assert int(outside.sum()) == 4 and int(empty.sum()) > 0
    assert float(g[outside].abs().max()) == 0.0 and float(g[empty].abs().max()) == 0.0
    inside_live = ~outside & ~empty
    assert float(g[inside_live].abs().max()) > 0


def test_boundary_colours_pass_their_gradient():
    """a colour exactly 0 or exactly 1 is inside (nfs_clamp01_bwd's convention), in the float64 reference and in the
    float32 restatement alike"""
    c, e, g = GR.check_inputs()
    got = GR.emission_bwd_np(g, c, e)
    assert got[0, 0] == g[0, 0] * e[0] and got[1, 1] == g[1, 1] * e[1] and got[2, 2] == g[2, 2] * e[2]      # 0, 1, -0.0
    assert got[3, 0] == 0 and got[4, 1] == 0 and got[5, 2] == 0                                             # outside, NaN
    assert not np.signbit(got[3, 0]) and not np.signbit(got[5, 2])


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_float32_restatement_is_the_float64_model_rounded_once(C):
    c, e, g = GR.check_inputs(C=C, seed=C)
    assert np.isnan(c).sum() == 1 and (c == 0).any() and (c == 1).any() and (c < 0).any() and (c > 1).any()
    assert np.signbit(e[e == 0]).tolist() == [False, True]
    assert GR.fwd_agrees(GR.emission_fwd_np, c, e)
    assert GR.bwd_agrees(GR.emission_bwd_np, g, c, e)
    q = GR.emission_fwd_np(c, e)
    assert not np.isnan(q).any()


def _drop_boundary(g, c, e):
    with np.errstate(invalid="ignore"):
        return np.where((c > 0) & (c < 1), g * e[:, None], np.float32(0))


def _e_of_wrong_voxel_fwd(c, e):
    n, C = c.shape
    return (GR.emission_fwd_np(c, np.ones(n, np.float32)).reshape(-1) * e[np.arange(n * C) % n]).reshape(n, C)


def _e_of_wrong_voxel_bwd(g, c, e):
    n, C = c.shape
    return (GR.emission_bwd_np(g, c, np.ones(n, np.float32)).reshape(-1) * e[np.arange(n * C) % n]).reshape(n, C)


def _mask_from_q(g, c, e):
    q = GR.emission_fwd_np(c, e)
    return np.where((q >= 0) & (q <= 1), g * e[:, None], np.float32(0))


def test_planted_defects_are_rejected():
    c, e, g = GR.check_inputs()
    assert GR.fwd_agrees(GR.emission_fwd_np, c, e) and GR.bwd_agrees(GR.emission_bwd_np, g, c, e)
    assert not GR.bwd_agrees(_drop_boundary, g, c, e)                                   # a clamp that drops the boundary
    assert not GR.fwd_agrees(_e_of_wrong_voxel_fwd, c, e)                               # e at flat % n
    assert not GR.bwd_agrees(_e_of_wrong_voxel_bwd, g, c, e)
    assert not GR.fwd_agrees(lambda c_, e_: GR.emission_fwd_np(c_, e_)[:, ::-1], c, e)  # the channels swapped
    assert not GR.bwd_agrees(lambda g_, c_, e_: GR.emission_bwd_np(g_, c_, e_)[:, ::-1], g, c, e)
    assert not GR.bwd_agrees(_mask_from_q, g, c, e)                                     # the mask taken from q, not c

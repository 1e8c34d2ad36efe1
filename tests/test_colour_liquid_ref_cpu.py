"""tests/colour_liquid_ref.py pinned without a GPU, in float64: the partition of unity sum_z w S + t = 1, the reference's
commented line (styler_3p.py:153) for a uniform colour over an arbitrary background, phi's limit at 0 and -0.0, the
transpose with w as autograd's dJ/dq; and the surface of the feature: the two flags, the key set of a bare get_config([]),
the new refusals and the standing one of render_liquid with a colour variable."""
import json
import os

import numpy as np
import pytest
import torch

from tests import colour_liquid_ref as LR
from tests import colour_ref as CR
from tests import view_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = float(np.float32(0.2))


def _volume(shape, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(shape, generator=g, dtype=torch.float64) * scale
    d[:, 0, 0] = 0.0                                # an empty ray at the identity
    d[:, 0, 1] = -0.0
    return d


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_partition_of_unity(shape):
    R = CR.views().double()
    w, t, S = LR.weights(_volume(shape, 1), R, TAU)
    one = (w * S).sum(1) + t
    assert float((one - 1).abs().max()) <= 1e-13
    assert float(w.min()) >= 0.0 and float(w.max()) <= TAU * (1 + 1e-15)
    assert float(t.max()) == 1.0 and float(t.min()) < 0.5            # the empty ray, and rays that are not transparent


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_uniform_colour_is_the_reference_line_153(shape):
    """q = c0 d: J = c0 (1 - t) + t bg, the line the reference left commented out, at its colour and at another, over white
    and over an arbitrary background"""
    R = CR.views().double()
    d = _volume(shape, 2)
    w, t, _ = LR.weights(d, R, TAU)
    for c0, bg in (([0.26, 0.5, 0.75], [1.0, 1.0, 1.0]), ([0.9, 0.1, 0.4], [0.2, 0.6, 0.05])):
        q = d.unsqueeze(-1) * torch.tensor(c0, dtype=torch.float64)
        J = LR.image(q, R, w, t, bg)
        want = (1 - t).unsqueeze(-1) * torch.tensor(c0, dtype=torch.float64) + t.unsqueeze(-1) * torch.tensor(bg, dtype=torch.float64)
        assert float((J - want).abs().max()) <= 1e-13


def test_grey_image_is_the_liquid_render():
    """C = 1, q = d, bg = 0: J = 1 - t, view_ref's liquid image"""
    R = CR.views().double()
    d = _volume((17, 6, 9), 3)
    w, t, S = LR.weights(d, R, TAU)
    J = LR.image(d.unsqueeze(-1), R, w, t, [0.0])
    for v in range(R.shape[0]):
        ref = VR.ray(S[v], torch.zeros_like(S[v]), TAU)["liquid"]
        assert float((J[v, ..., 0] - ref).abs().max()) <= 1e-13


def test_phi_limits_and_the_ray_of_zeros():
    x = torch.tensor([0.0, -0.0, 1e-300, 1e-9, 9.9e-6, 1.01e-5, 2.0 ** -5, 1.0, 50.0, 800.0], dtype=torch.float64)
    ph = LR.phi(x)
    assert float(ph[0]) == 1.0 and float(ph[1]) == 1.0 and float(ph[2]) == 1.0
    exact = [1.0, 1.0, 1.0, 1 - 5e-10, None, None, None, 1 - np.exp(-1.0), (1 - np.exp(-50.0)) / 50.0, 1 / 800.0]
    for got, want in zip(ph.tolist(), exact):
        assert want is None or abs(got - want) <= 4e-16 * want
    # continuous across the switch of forms, and decreasing
    assert all(a > b for a, b in zip(ph[2:].tolist(), ph[3:].tolist()))
    assert abs(float(ph[4]) - float(ph[5])) < 2e-7
    # a ray of zeros and a ray of -0.0: w = tau everywhere, t = 1; bounds are finite and positive
    for z in (0.0, -0.0):
        r = LR.ray(torch.full((5, 2), z, dtype=torch.float64), torch.zeros(5, 2, dtype=torch.float64), TAU)
        assert bool((r["w"] == TAU).all()) and bool((r["t"] == 1).all()) and bool((r["grey"] == 0).all())
        assert bool((r["e_w"] > 0).all()) and bool(torch.isfinite(r["e_w"]).all())
    # ray() and weights() are the same numbers
    d = _volume((5, 3, 4), 4)
    w, t, S = LR.weights(d, CR.views().double()[:1], TAU)
    r = LR.ray(S[0], torch.zeros_like(S[0]), TAU)
    assert float((r["w"] - w[0]).abs().max()) <= 1e-15 and float((r["t"] - t[0]).abs().max()) <= 1e-15


def test_bounds_are_above_float32_rounding_of_the_inputs():
    """the bounds are not too tight: the reference evaluated on samples perturbed by half an ulp stays within them"""
    g = torch.Generator().manual_seed(5)
    s = torch.rand((17, 40), generator=g, dtype=torch.float64) * 6
    es = s * VR.EPS
    r = LR.ray(s, es, TAU)
    sign = torch.where(torch.rand(s.shape, generator=g) < 0.5, -1.0, 1.0).double()
    r2 = LR.ray(s + sign * es, torch.zeros_like(s), TAU)
    assert VR.err_ratio((r2["w"] - r["w"]).abs(), r["e_w"]) <= 1.0
    assert VR.err_ratio((r2["t"] - r["t"]).abs(), r["e_t"]) <= 1.0


def test_autograd_of_the_image_is_the_transpose_with_w():
    shape = (5, 4, 6)
    R = CR.views().double()
    d = _volume(shape, 6)
    w, t, _ = LR.weights(d, R, TAU)
    g = torch.randn((R.shape[0],) + shape[1:] + (3,), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    q = torch.rand(shape + (3,), generator=torch.Generator().manual_seed(8), dtype=torch.float64).requires_grad_()
    (gq,) = torch.autograd.grad((LR.image(q, R, w, t, [0.3, 0.2, 0.9]) * g).sum(), q)
    ref = CR.transpose_ref(R, g, w)
    assert float((gq - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# ---- the surface -----------------------------------------------------------------------------------------------------

def test_flags_parse_and_have_their_defaults():
    from neural_flow_style_amd import config
    cfg, rest = config.get_config([])
    assert not rest and not hasattr(cfg, "colour_render") and not hasattr(cfg, "colour_background")
    config.complete(cfg)
    assert cfg.colour_render == "" and list(cfg.colour_background) == [1.0, 1.0, 1.0]
    cfg, rest = config.get_config(["--colour_render", "liquid", "--colour_background", "0.26", "0.5", "0.75"])
    assert not rest and cfg.colour_render == "liquid" and cfg.colour_background == [0.26, 0.5, 0.75]
    config.complete(cfg)
    assert cfg.colour_render == "liquid" and cfg.colour_background == [0.26, 0.5, 0.75]
    assert config.get_config(["--colour_render", "smoke"])[0].colour_render == "smoke"
    bare = type("Cfg", (), {"seed": 1})()
    config.complete(bare)
    assert bare.colour_render == "" and list(bare.colour_background) == [1.0, 1.0, 1.0]
    assert config.check_colour_render(cfg, colour=True) == ("liquid", (0.26, 0.5, 0.75))
    assert config.check_colour_render(bare, colour=False) == ("", (1.0, 1.0, 1.0))


def test_a_bare_get_config_keeps_its_key_set():
    from neural_flow_style_amd import config
    cfg, _ = config.get_config([])
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "config_defaults.json")))
    extras = {"views_mode", "grid_variable", "synthetic_weights", "transport_recursive", "ray_mode"}
    assert set(vars(cfg)) - extras == set(pinned) - extras
    assert set(vars(cfg)) >= extras and not ({"colour_render", "colour_background", "lap_n", "lr_decay"} & set(vars(cfg)))


def _cfg(**over):
    from neural_flow_style_amd import config
    cfg, _ = config.get_config([])
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


COLOUR = {"styler_3p": dict(target_field="c"), "styler_grid": dict(grid_variable="c", resolution=[8, 8, 8])}


def _styler(module):
    import importlib
    return importlib.import_module("neural_flow_style_amd." + module).Styler


@pytest.mark.parametrize("module", ["styler_3p", "styler_grid"])
def test_the_new_refusals_come_before_a_network_is_loaded(module):
    """each a ValueError naming the flag, raised in the constructor's first lines (no device, no network: this test has
    neither)"""
    Styler = _styler(module)
    for bad in ("max", "Liquid", "mean"):
        with pytest.raises(ValueError, match="colour_render"):
            Styler(_cfg(colour_render=bad, **COLOUR[module]))
    with pytest.raises(ValueError, match="colour_render") as e:
        Styler(_cfg(colour_render="liquid", **{k: v for k, v in COLOUR[module].items() if k == "resolution"}))
    assert "colour variable" in str(e.value)
    for bad in ([1.0, 1.0], [0.5, 0.5, 1.5], [-0.1, 0, 0], [0.1, float("nan"), 0.2], "white", 1.0, [0, 0, 0, 0]):
        with pytest.raises(ValueError, match="colour_background"):
            Styler(_cfg(colour_render="liquid", colour_background=bad, **COLOUR[module]))
        with pytest.raises(ValueError, match="colour_background"):       # (checked whatever the render is)
            Styler(_cfg(colour_background=bad, **COLOUR[module]))


def test_the_2d_particle_stylizer_refuses_the_liquid_colour_render():
    with pytest.raises(ValueError, match="colour_render"):
        _styler("styler_2p")(_cfg(colour_render="liquid", target_field="c"))


@pytest.mark.parametrize("module", ["styler_3p", "styler_grid"])
@pytest.mark.parametrize("render", ["", "liquid"])
def test_render_liquid_with_a_colour_variable_still_raises(module, render):
    """the grey flag keeps its meaning and stays refused on the colour paths; the message points at the colour flag"""
    with pytest.raises(ValueError, match="render_liquid") as e:
        _styler(module)(_cfg(render_liquid=True, colour_render=render, **COLOUR[module]))
    assert "--colour_render liquid" in str(e.value)


def test_the_engine_refuses_the_same_values():
    from neural_flow_style_amd import engine
    with pytest.raises(ValueError, match="colour_render"):
        engine.ColourRenderLoss(None, 0.2, render="max")
    with pytest.raises(ValueError, match="colour_background"):
        engine.ColourRenderLoss(None, 0.2, render="liquid", background=(0, 0, 2))
    plain = engine.ColourRenderLoss(None, 0.2)
    assert not plain.liquid and plain.background == (1.0, 1.0, 1.0)
    assert not engine.ColourRenderLoss(None, 0.2, render="smoke").liquid
    liquid = engine.ColourRenderLoss(None, 0.2, 3, "liquid", (0.26, 0.5, 0.75))
    assert liquid.liquid and liquid.v_batch == 3 and liquid.background == (0.26, 0.5, 0.75)

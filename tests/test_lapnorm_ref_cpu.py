"""Laplacian-normalised descent without a GPU: the cosine schedule, the float64 reference step of tests/lapnorm_ref.py and the
public surface (flags, refusals).  Odd sizes: TF's 'SAME' padding of the strided smoothing is asymmetric there."""
import numpy as np
import pytest

from tests import lapnorm_ref as R

SHAPES = [((7, 9, 6, 3), True), ((9, 8, 2), False)]


# ---- the schedule --------------------------------------------------------------------------------------------------------
def test_cosine_decay_runs_from_factor_times_lr_down_to_lr():
    from neural_flow_style_amd.util import cosine_decay
    lr, n, f = 0.0125, 7, 2.5
    assert cosine_decay(0, n, lr, f) == pytest.approx(f * lr, rel=1e-15)
    assert cosine_decay(n, n, lr, f) == pytest.approx(lr, rel=1e-15)
    assert cosine_decay(n + 3, n, lr, f) == cosine_decay(n, n, lr, f)                 # (held at lr past the end)
    seq = [cosine_decay(i, n, lr, f) for i in range(n + 1)]
    assert all(a > b for a, b in zip(seq, seq[1:]))                                   # monotone for a factor > 1


@pytest.mark.parametrize("lr", [0.0007, 0.02, 1.0 / 3.0, 3e-5])
def test_cosine_decay_at_factor_one_is_the_learning_rate_bit_for_bit(lr):
    """runs that do not set --lr_decay keep their bits: the function returns lr * 1.0"""
    from neural_flow_style_amd.util import cosine_decay
    for n in (1, 3, 20, 97):
        for i in range(n + 2):
            got = float(cosine_decay(i, n, lr, 1.0))
            assert got == lr and np.float64(got).tobytes() == np.float64(lr).tobytes(), (i, n)
            assert float(cosine_decay(i, n, lr, 1)) == lr                             # (the flag's default is the int 1)


# ---- the reference step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,is_3d", SHAPES)
@pytest.mark.parametrize("lap_n", [0, 1, 3])
def test_update_does_not_depend_on_the_scale_of_the_gradient(shape, is_3d, lap_n):
    """the point of the normalisation: g and a * g (a > 0) give the same update"""
    rng = np.random.RandomState(5)
    g, x = rng.randn(*shape), rng.randn(*shape)
    _, upd = R.step(x, g, 0.03, lap_n, is_3d)
    for a in (1e-3, 7.0, 4096.0):
        _, upd_a = R.step(x, a * g, 0.03, lap_n, is_3d)
        assert R.rel(upd_a, upd) < 1e-12, (a, R.rel(upd_a, upd))
    assert np.abs(upd).max() > 0


@pytest.mark.parametrize("shape,is_3d", SHAPES)
@pytest.mark.parametrize("lap_n", [0, 1, 3])
def test_zero_gradient_gives_a_zero_update_and_no_nan(shape, is_3d, lap_n):
    x = np.random.RandomState(6).randn(*shape)
    x1, upd = R.step(x, np.zeros(shape), 0.5, lap_n, is_3d)
    assert np.isfinite(upd).all() and not upd.any() and np.array_equal(x1, x)


@pytest.mark.parametrize("shape,is_3d", SHAPES)
def test_without_a_pyramid_the_mean_absolute_update_is_the_learning_rate(shape, is_3d):
    g = np.random.RandomState(7).randn(*shape) * 37.0
    _, upd = R.step(np.zeros(shape), g, 0.0125, 0, is_3d)
    assert abs(np.abs(upd).mean() - 0.0125) < 1e-12 * 0.0125


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_flags_parse_and_have_their_defaults():
    from neural_flow_style_amd import config
    cfg, rest = config.get_config([])
    config.complete(cfg)                       # (the defaults of the build flags that are not in the bare Namespace)
    assert cfg.lr_decay == 1 and isinstance(cfg.lr_decay, (int, float)) and cfg.lap_n == 3 and not rest
    cfg, rest = config.get_config(["--optimizer", "lapnorm", "--lap_n", "2", "--lr_decay", "2.5"])
    assert (cfg.optimizer, cfg.lap_n, cfg.lr_decay) == ("lapnorm", 2, 2.5) and not rest
    assert isinstance(cfg.lap_n, int) and isinstance(cfg.lr_decay, float)
    config.complete(cfg)
    assert (cfg.lap_n, cfg.lr_decay) == (2, 2.5)
    bare = type("Cfg", (), {"seed": 1})()
    config.complete(bare)
    assert bare.lr_decay == 1 and bare.lap_n == 3


def test_optimizers_are_made_by_name_and_the_error_names_all_three():
    from neural_flow_style_amd import engine
    opt = engine.make_optimizer("lapnorm", lap_n=2)
    assert isinstance(opt, engine.LapDescentState) and opt.lap_n == 2
    assert engine.make_optimizer("lapnorm").lap_n == 3 and engine.LapDescentState().lap_n == 3
    assert engine.optimizer_slot("lapnorm", 7, 3) == engine.optimizer_slot("adam", 7, 3) == 2
    with pytest.raises(ValueError) as e:
        engine.make_optimizer("sgd")
    assert all(name in str(e.value) for name in ("'adam'", "'lbfgs'", "'lapnorm'"))
    with pytest.raises(ValueError, match="lap_n"):
        engine.LapDescentState(lap_n=-1)


def _cfg(**over):
    from neural_flow_style_amd import config
    cfg, _ = config.get_config([])
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("module", ["styler_grid", "styler_3p", "styler_2p"])
def test_stylers_refuse_bad_flags_by_name_before_anything_else(module):
    """the checks come first in every Styler's constructor (before the device and the loss network are touched)"""
    import importlib
    Styler = importlib.import_module("neural_flow_style_amd." + module).Styler
    with pytest.raises(ValueError, match="lap_n"):
        Styler(_cfg(lap_n=-1))
    for bad in (0.0, -2.0):
        with pytest.raises(ValueError, match="lr_decay"):
            Styler(_cfg(lr_decay=bad))


@pytest.mark.parametrize("module", ["styler_3p", "styler_2p"])
def test_particle_stylers_refuse_lapnorm(module):
    import importlib
    Styler = importlib.import_module("neural_flow_style_amd." + module).Styler
    with pytest.raises(ValueError, match="optimizer lapnorm") as e:
        Styler(_cfg(optimizer="lapnorm"))
    assert "grid" in str(e.value)

"""Flag surface of the reference's ``config.py`` (config.py:15-114): same flag names, types and
defaults, so a reference driver's ``config`` Namespace drops in.  ``get_config()`` returns
``(Namespace, unparsed)``.  Drivers add non-flag attributes afterwards (``rng``, ``num_kernels``,
``kernel_scale``; test_smokegun.py:22,117-120) -- ``complete()`` fills their defaults.

Build-specific additions (not in the reference): ``--views_mode`` (``sequential`` = the reference's
one-Adam-step-per-view loop, ``sum`` = gradient of the summed view losses, shardable over GPUs),
``--grid_variable`` / ``--transport_recursive`` for the grid (TNST-style) path, ``--synthetic_weights`` (explicit
opt-in to seeded synthetic VGG filters when no converted checkpoint exists), ``--ray_mode`` (``max`` / ``mean``: the
per-ray reductions north_star names beside the reference's transmittance / liquid integrals; '' follows
``render_liquid``).  The reference's own ``--optimizer`` flag (config.py:78, default 'adam', the only value its code
honours) additionally takes ``lbfgs`` here: limited-memory BFGS, north_star's other outer loop (engine.LBFGSState),
and -- on the grid path -- ``lapnorm``: Laplacian-normalised descent (engine.LapDescentState) with ``--lap_n`` pyramid
levels (0: mean-|g| normalisation).  ``--lr_decay``: the factor of the reference's ``cosine_decay`` (util.py:49-53) on the
grid path's learning rate, from ``lr_decay * lr`` at the first iteration of an octave down to ``lr``; 1 = constant.
``--lr_decay`` (float, default 1) and ``--lap_n`` (int, default 3) are parsed when given and otherwise defaulted by
``complete()``, like the attributes the drivers inject.  So are ``--colour_render`` ('' / 'smoke': the colour paths'
emission-absorption render over black, max-normalised; 'liquid': front-to-back alpha compositing over a background,
include/nfs_liquid.h; 'exposure': the smoke model at a fixed exposure ``--colour_exposure`` (positive float, default 1) with
no maximum, include/nfs_exposure.h; default '') and ``--colour_background`` (three floats in [0,1], the liquid render's background;
default 1 1 1), read by the two colour stylizers (styler_3p ``target_field 'c'``, styler_grid ``grid_variable 'c'``).
``--target_field pc`` (styler_3p): positions and colours in one variable, of a liquid through ``--colour_render liquid`` or
of smoke through ``--colour_render exposure``; ``--colour_lr_scale`` (positive float, default 1, defaulted by
``complete()`` too): one optimiser step of ``lr`` moves a colour of that variable by ``colour_lr_scale * lr``.
``--target_field g`` (styler_3p): the variable is a displacement field on a coarse carrier grid, sampled at the particles
(include/nfs_carrier.h); ``--carrier_resolution`` (three ints >= 1; ``complete()`` defaults it to ``max(n // 8, 2)`` per axis
of ``resolution``) is that grid and ``--carrier_interp`` (``cubic`` / ``linear``, default ``cubic``) the sampling kernel.
``--carrier_steps`` (int >= 1, default 1): the field is a velocity over one unit of pseudo-time and the particles are carried
through it in that many explicit Euler steps (include/nfs_flow.h); 1 is the one-sample displacement p + g2p(u, p).  A field
stylised at K steps must be applied at the same K.
"""
from __future__ import annotations

import argparse

import numpy as np


def str2bool(v):
    return str(v).lower() in ("true", "1", "yes", "y", "t")


# (group, flag, kwargs) -- one row per reference flag
_FLAGS = [
    ("Path", "data_dir", dict(type=str, default="data")),
    ("Path", "log_dir", dict(type=str, default="log")),
    ("Path", "model_dir", dict(type=str, default="model")),
    ("Path", "d_path", dict(type=str, default="d/%03d.npz")),
    ("Path", "v_path", dict(type=str, default="v/%03d.npz")),
    ("Path", "tag", dict(type=str, default="test")),
    ("Data", "dataset", dict(type=str, default="smokegun")),
    ("Data", "target_frame", dict(type=int, default=70)),
    ("Data", "num_frames", dict(type=int, default=1)),
    ("Data", "scale", dict(type=float, default=2.0)),
    ("Network", "network", dict(type=str, default="tensorflow_inception_graph.pb",
                                choices=["tensorflow_inception_graph.pb", "vgg_19.ckpt"])),
    ("Network", "pool1", dict(type=str2bool, default=False)),
    ("Network", "batch_size", dict(type=int, default=1)),
    ("Grid", "resolution", dict(nargs="+", type=int, default=[384, 288])),
    ("Grid", "adv_order", dict(type=int, default=1, choices=[1, 2])),
    ("Particle", "domain", dict(nargs="+", type=int, default=[12.8, 12.8, 12.8])),
    ("Particle", "radius", dict(type=float, default=0.025)),
    ("Particle", "disc", dict(type=int, default=2)),
    ("Particle", "nsize", dict(type=int, default=1)),
    ("Particle", "rest_density", dict(type=float, default=1000)),
    ("Particle", "w_pressure", dict(type=float, default=0)),
    ("Particle", "w_density", dict(type=float, default=0)),
    ("Particle", "window_sigma", dict(type=float, default=2)),
    ("Particle", "interp", dict(type=int, default=1)),
    ("Particle", "support", dict(type=float, default=4)),
    ("Particle", "k", dict(type=int, default=3)),
    ("Particle", "clip", dict(type=str2bool, default=False)),
    ("Render", "resize_scale", dict(type=float, default=1.0)),
    ("Render", "transmit", dict(type=float, default=0.01)),
    ("Render", "rotate", dict(type=str2bool, default=False)),
    ("Render", "phi0", dict(type=int, default=-5)),
    ("Render", "phi1", dict(type=int, default=5)),
    ("Render", "phi_unit", dict(type=int, default=5)),
    ("Render", "theta0", dict(type=int, default=-10)),
    ("Render", "theta1", dict(type=int, default=10)),
    ("Render", "theta_unit", dict(type=int, default=10)),
    ("Render", "v_batch", dict(type=int, default=1)),
    ("Render", "n_views", dict(type=int, default=9)),
    ("Render", "sample_type", dict(type=str, default="poisson", choices=["uniform", "poisson", "both"])),
    ("Render", "render_liquid", dict(type=str2bool, default=False)),
    ("Optimizer", "target_field", dict(type=str, default="p", choices=["d", "p", "c", "pc", "g"])),
    ("Optimizer", "optimizer", dict(type=str, default="adam")),
    ("Optimizer", "iter", dict(type=int, default=20)),
    ("Optimizer", "lr", dict(type=float, default=0.0007)),
    ("Optimizer", "lr_scale", dict(type=float, default=1)),
    ("Optimizer", "octave_n", dict(type=int, default=2)),
    ("Optimizer", "octave_scale", dict(type=float, default=1.8)),
    ("Optimizer", "frames_per_opt", dict(type=int, default=10)),
    ("Style", "content_layer", dict(type=str, default="mixed4d_3x3_bottleneck_pre_relu")),
    ("Style", "content_channel", dict(type=int, default=139)),
    ("Style", "w_content", dict(type=float, default=1)),
    ("Style", "w_content_amp", dict(type=float, default=100)),
    ("Style", "content_target", dict(type=str, default="")),
    ("Style", "top_k", dict(type=int, default=5)),
    ("Style", "style_layer", dict(nargs="+", type=str, default=["conv3_1"])),
    ("Style", "w_style", dict(type=float, default=0)),
    ("Style", "w_style_layer", dict(nargs="+", type=float, default=[1])),
    ("Style", "hist_layer", dict(nargs="+", type=str, default=["input"])),
    ("Style", "w_hist", dict(type=float, default=0)),
    ("Style", "w_hist_layer", dict(nargs="+", type=float, default=[1])),
    ("Style", "w_tv", dict(type=float, default=0)),
    ("Style", "style_target", dict(type=str, default="")),
    ("Style", "style_mask", dict(type=str2bool, default=False)),
    ("Style", "style_mask_on_ref", dict(type=str2bool, default=False)),
    ("Style", "style_tiling", dict(type=int, default=1)),
    ("Style", "style_init", dict(type=str, default="noise", choices=["noise", "style"])),
    ("Misc", "seed", dict(type=int, default=123)),
    ("Misc", "gpu_id", dict(type=str, default="0")),
    # ---- build-specific -------------------------------------------------------------------
    ("MI355X", "views_mode", dict(type=str, default="sequential", choices=["sequential", "sum"])),
    ("MI355X", "grid_variable", dict(type=str, default="", choices=["", "v", "d", "s", "p", "sp", "c"])),
    ("MI355X", "synthetic_weights", dict(type=str2bool, default=False)),
    ("MI355X", "transport_recursive", dict(type=str2bool, default=True)),
    ("MI355X", "ray_mode", dict(type=str, default="", choices=["", "transmit", "liquid", "max", "mean"])),
    # (argparse.SUPPRESS: parsed when given; their defaults -- 1 and 3 -- come from complete(), which every Styler calls,
    # so that the Namespace of a bare get_config([]) stays the reference's flags plus the five extras above)
    ("MI355X", "lr_decay", dict(type=float, default=argparse.SUPPRESS)),
    ("MI355X", "lap_n", dict(type=int, default=argparse.SUPPRESS)),
    ("MI355X", "colour_render", dict(type=str, default=argparse.SUPPRESS)),
    ("MI355X", "colour_background", dict(nargs=3, type=float, default=argparse.SUPPRESS)),
    ("MI355X", "colour_lr_scale", dict(type=float, default=argparse.SUPPRESS)),
    ("MI355X", "colour_exposure", dict(type=float, default=argparse.SUPPRESS)),
    ("MI355X", "carrier_resolution", dict(nargs=3, type=int, default=argparse.SUPPRESS)),
    ("MI355X", "carrier_interp", dict(type=str, default=argparse.SUPPRESS)),
    ("MI355X", "carrier_steps", dict(type=int, default=argparse.SUPPRESS)),
]

COLOUR_RENDERS = ("", "smoke", "liquid", "exposure")
CARRIER_INTERPS = ("cubic", "linear")


def make_parser():
    parser = argparse.ArgumentParser()
    groups = {}
    for grp, flag, kw in _FLAGS:
        g = groups.get(grp)
        if g is None:
            g = groups[grp] = parser.add_argument_group(grp)
        g.add_argument("--" + flag, **kw)
    return parser


parser = make_parser()


def get_config(argv=None):
    config, unparsed = parser.parse_known_args(argv)
    return config, unparsed


def check_optimizer(config, grid):
    """the build-specific optimiser flags, checked where a stylizer is constructed (``grid``: the grid path, styler_grid):
    ValueError naming the flag for ``lap_n`` < 0, ``lr_decay`` <= 0, and ``optimizer='lapnorm'`` on the particle stylizers --
    a Laplacian pyramid needs a grid, and particle attributes have none"""
    lap_n, lr_decay = getattr(config, "lap_n", 3), getattr(config, "lr_decay", 1)
    if int(lap_n) < 0:
        raise ValueError("--lap_n %d: the number of pyramid levels of optimizer 'lapnorm' is 0 (mean-|g| normalisation) "
                         "or more" % int(lap_n))
    if not float(lr_decay) > 0:
        raise ValueError("--lr_decay %g: the cosine schedule's factor must be positive (1 = constant learning rate)"
                         % float(lr_decay))
    if getattr(config, "optimizer", "adam") == "lapnorm" and not grid:
        raise ValueError("--optimizer lapnorm on a particle stylizer (styler_3p / styler_2p): the Laplacian pyramid needs a "
                         "grid and particle attributes have none -- it is an optimiser of the grid path (styler_grid, "
                         "--grid_variable); use 'adam' or 'lbfgs' here")


def colour_background(background):
    """``colour_background`` as a tuple of three floats in [0,1], or a ValueError naming the flag (a NaN is not in [0,1])"""
    try:
        bg = tuple(float(x) for x in background)
    except (TypeError, ValueError):
        bg = None
    if bg is None or len(bg) != 3 or not all(0.0 <= x <= 1.0 for x in bg):
        raise ValueError("--colour_background %r: the background of the liquid colour render is three numbers in [0,1]"
                         % (background,))
    return bg


def colour_exposure(exposure):
    """``colour_exposure`` as a finite positive float, or a ValueError naming the flag (None: the default 1)"""
    try:
        k = float(1.0 if exposure is None else exposure)
    except (TypeError, ValueError):
        k = float("nan")
    if not (0.0 < k < float("inf")):
        raise ValueError("--colour_exposure %r: the exposure of colour_render 'exposure' must be finite and positive"
                         % (exposure,))
    return k


def check_colour_render(config, colour):
    """the colour render's flags, checked where a stylizer is constructed, before a network is loaded (``colour``: the
    stylizer's variable is, or holds, a colour rendered through views -- styler_3p target_field 'c' and 'pc', styler_grid
    grid_variable 'c').
    ValueError naming the flag for a ``colour_render`` outside '' / 'smoke' / 'liquid' / 'exposure', for 'liquid' or
    'exposure' without a colour variable, for a ``colour_background`` that is not three numbers in [0,1] and for a
    ``colour_exposure`` that is not finite and positive (both whatever the render is).  -> (render, background); the
    exposure is ``colour_exposure(config.colour_exposure)``"""
    render = getattr(config, "colour_render", "")
    render = "" if render is None else render
    if render not in COLOUR_RENDERS:
        raise ValueError("--colour_render %r is none of %s" % (render, COLOUR_RENDERS))
    bg = colour_background(getattr(config, "colour_background", (1.0, 1.0, 1.0)))
    colour_exposure(getattr(config, "colour_exposure", 1.0))
    if render == "exposure" and not colour:
        raise ValueError("--colour_render exposure (--colour_exposure) without a colour variable: the fixed-exposure colour "
                         "render belongs to --target_field c / pc of the 3-D particle stylizer and --grid_variable c of the "
                         "grid stylizer")
    if render == "liquid" and not colour:
        raise ValueError("--colour_render liquid without a colour variable: the liquid colour render belongs to "
                         "--target_field c of the 3-D particle stylizer and --grid_variable c of the grid stylizer (the "
                         "grey liquid render is --render_liquid)")
    return render, bg


def default_carrier_resolution(resolution):
    """``max(n // 8, 2)`` per axis of ``resolution``"""
    return [max(int(n) // 8, 2) for n in resolution]


def check_carrier(config):
    """the carrier grid's flags (target_field 'g'), checked where the stylizer is constructed, before a network is loaded:
    ValueError naming the flag for a ``carrier_resolution`` that is not three ints >= 1 and a ``carrier_interp`` outside
    'cubic' / 'linear'.  -> (resolution as a tuple of three ints, cubic as a bool)"""
    res = getattr(config, "carrier_resolution", None)
    if res is None:
        res = default_carrier_resolution(getattr(config, "resolution", ()))
    try:
        ok = len(res) == 3 and all(float(v) == int(v) and not isinstance(v, bool) and int(v) >= 1 for v in res)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("--carrier_resolution %r: the carrier grid of target_field 'g' is three ints >= 1" % (res,))
    interp = getattr(config, "carrier_interp", None)
    interp = "cubic" if interp is None else interp
    if interp not in CARRIER_INTERPS:
        raise ValueError("--carrier_interp %r is none of %s" % (interp, CARRIER_INTERPS))
    return tuple(int(v) for v in res), interp == "cubic"


def check_carrier_steps(config):
    """``carrier_steps`` (target_field 'g') as an int >= 1, or a ValueError naming the flag (absent or None: 1)"""
    steps = getattr(config, "carrier_steps", None)
    steps = 1 if steps is None else steps
    try:
        ok = not isinstance(steps, bool) and float(steps) == int(steps) and int(steps) >= 1
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("--carrier_steps %r: the number of Euler steps of the carrier flow is an int >= 1 (1 = the "
                         "one-sample displacement)" % (steps,))
    return int(steps)


def complete(config):
    """defaults for the attributes the reference drivers inject after parsing"""
    if not hasattr(config, "rng") or config.rng is None:
        config.rng = np.random.RandomState(config.seed)
    if not hasattr(config, "num_kernels"):
        config.num_kernels = 1
    if not hasattr(config, "kernel_scale"):
        config.kernel_scale = 2
    if not hasattr(config, "views_mode"):
        config.views_mode = "sequential"
    if not hasattr(config, "grid_variable"):
        config.grid_variable = ""
    if not hasattr(config, "synthetic_weights"):
        config.synthetic_weights = False
    if not hasattr(config, "transport_recursive"):
        config.transport_recursive = True
    if not hasattr(config, "ray_mode"):
        config.ray_mode = ""
    if not hasattr(config, "lr_decay"):
        config.lr_decay = 1
    if not hasattr(config, "lap_n"):
        config.lap_n = 3
    if not hasattr(config, "colour_render"):
        config.colour_render = ""
    if not hasattr(config, "colour_background"):
        config.colour_background = [1.0, 1.0, 1.0]
    if not hasattr(config, "colour_lr_scale"):
        config.colour_lr_scale = 1.0
    if not hasattr(config, "colour_exposure"):
        config.colour_exposure = 1.0
    if not hasattr(config, "carrier_resolution"):
        config.carrier_resolution = default_carrier_resolution(getattr(config, "resolution", ()))
    if not hasattr(config, "carrier_interp"):
        config.carrier_interp = "cubic"
    if not hasattr(config, "carrier_steps"):
        config.carrier_steps = 1

    return config

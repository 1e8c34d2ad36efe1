"""The smoke colour render at a fixed exposure (colour_render 'exposure', include/nfs_exposure.h) without a GPU: the closed
form of tests/exposure_ref.py against autograd of the float64 model, grey <= kappa (1 - t), a float32 emulation inside every
bound and planted defects outside one, the flags, the constructor refusals, the binding of libnfs_exposure.so (the open table
_lib.SIDE_OPEN), the entry points' refusals, and the condition on the inputs of the GPU tests
(tests/test_exposure_stylizer_gpu.py), checked on the reference alone."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from neural_flow_style_amd import _lib
from tests import colour_ref as CR
from tests import exposure_ref as ER
from tests import test_side_libraries_cpu as SL
from tests import view_ref as VR

TAU = float(np.float32(0.2))
KAPPA = 1.5                                                          # (exact in float32, and not 1: a dropped kappa shows)


def _built():
    SL._built()
    if not all(os.path.exists(r.path) for r in _lib.SIDE_OPEN.values()):
        _lib.build()
    return _lib


# ---- the arithmetic ---------------------------------------------------------------------------------------------------

def _case(seed=3, shape=(9, 4, 5), C=3, scale=6.0):
    g = torch.Generator().manual_seed(seed)
    S = torch.rand(shape, generator=g, dtype=torch.float64) * scale
    S[:, 0, 0] = 0.0                                                  # an empty ray
    S[2, 1, 1] = 0.0                                                  # a zero sample inside a ray
    Q = torch.rand(shape + (C,), generator=g, dtype=torch.float64)
    gJ = torch.randn(shape[1:] + (C,), generator=g, dtype=torch.float64)
    return S, Q, gJ


@pytest.mark.parametrize("C", [1, 3])
def test_closed_form_equals_autograd_of_the_model(C):
    S, Q, gJ = _case(C=C)
    Sv = S.clone().requires_grad_()
    (want,) = torch.autograd.grad((ER.model_image(Sv, Q, TAU, KAPPA) * gJ).sum(), Sv)
    got = ER.closed_form(S, Q, gJ, TAU, KAPPA)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print("closed form against autograd: %.3g relative (scale %.3g)" % (err, float(want.abs().max())))
    assert err <= 1e-12


def test_closed_form_equals_autograd_through_the_rotation():
    """the same through ER.weights / CR.image on a volume and three views: g_S scattered by the rotation's transpose is
    autograd's gradient in d"""
    shape = (7, 5, 6)
    g = torch.Generator().manual_seed(8)
    d = torch.rand(shape, generator=g, dtype=torch.float64) * 4.0
    q = torch.rand(shape + (3,), generator=g, dtype=torch.float64)
    R = CR.views().double()[:3]
    gJ = torch.randn((3,) + shape[1:] + (3,), generator=g, dtype=torch.float64)
    dv = d.clone().requires_grad_()
    w, _, _ = ER.weights(dv, R, TAU, KAPPA)
    (want,) = torch.autograd.grad((CR.image(q, R, w) * gJ).sum(), dv)
    Sd = CR.rotate(d.unsqueeze(-1), R)[..., 0]
    Qr = CR.rotate(q, R)
    g_S = torch.stack([ER.closed_form(Sd[v], Qr[v], gJ[v], TAU, KAPPA) for v in range(3)])
    dv2 = d.clone().requires_grad_()
    (got,) = torch.autograd.grad((CR.rotate(dv2.unsqueeze(-1), R)[..., 0] * g_S).sum(), dv2)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print("through the rotation: %.3g relative" % err)
    assert err <= 1e-12


@pytest.mark.parametrize("kappa", [1.0, KAPPA, 0.25])
def test_grey_is_at_most_kappa_times_one_minus_t(kappa):
    """S e^(-tau S) <= (1 - e^(-tau S)) / tau sample by sample: grey <= kappa (1 - t); so at kappa = 1 a uniform colour
    c0 (q = c0 S) renders at most c0 (1 - t) <= 1 and is never clipped"""
    for scale in (0.01, 1.0, 6.0, 60.0):
        S, _, _ = _case(seed=5, scale=scale)
        grey = ER.grey_of(S, TAU, kappa)
        t = torch.exp(-TAU * S.sum(0))
        assert float((grey - kappa * (1 - t)).max()) <= 1e-15
        assert float(grey.min()) >= 0.0 and float(grey[0, 0]) == 0.0             # (the empty ray)
        c0 = torch.tensor([0.26, 0.5, 1.0], dtype=torch.float64)
        J = ER.model_image(S, S.unsqueeze(-1) * c0, TAU, kappa)
        assert float((J - kappa * c0 * (1 - t).unsqueeze(-1)).max()) <= 1e-15
        if kappa == 1.0:
            assert float(J.max()) <= 1.0
    # ray() and weights() are the same numbers
    d = _case(seed=4, shape=(5, 3, 4))[0]
    w, grey, Sr = ER.weights(d, CR.views().double()[:1], TAU, KAPPA)
    r = ER.ray(Sr[0], torch.zeros_like(Sr[0]), TAU, KAPPA)
    assert float((r["w"] - w[0]).abs().max()) <= 1e-15 and float((r["grey"] - grey[0]).abs().max()) <= 1e-15
    assert float((r["w"] - ER.weights_of(Sr[0], TAU, KAPPA)).abs().max()) <= 1e-15


# ---- a float32 emulation and planted defects ---------------------------------------------------------------------------

F32 = np.float32


def emulate(s, Q, g, tau, kappa, defect=None):
    """the two kernels in sequential float32 numpy, one rounding per operation: s [D,n], Q [D,n,C], g [n,C] (float32) ->
    (w [D,n], grey [n], g_s [D,n]).  ``defect``: one planted mistake"""
    D, n = s.shape
    C = Q.shape[-1]
    tau, kappa = F32(tau), F32(kappa)
    ntau = F32(-tau * F32(1.44269504088896341))
    kt = tau if defect == "dropped kappa" else F32(kappa * tau)
    w = np.zeros((D, n), F32)
    acc, grey = np.zeros(n, F32), np.zeros(n, F32)
    for z in range(D - 1, -1, -1):
        s0 = s[z] + F32(0.0)
        before = acc
        acc = (acc + s0).astype(F32)
        arg = ((before if defect == "exclusive running sum" else acc) * ntau).astype(F32)
        w[z] = (kt * np.exp2(arg.astype(np.float64)).astype(F32)).astype(F32)
        grey = (grey + (w[z] * s0).astype(F32)).astype(F32)
    g_s = np.zeros((D, n), F32)
    P = np.zeros(n, F32)
    order = range(D - 1, -1, -1) if defect == "prefix from the far end" else range(D)
    for z in order:
        a = np.zeros(n, F32)
        for c in range(C):
            a = (a + (g[:, c] * Q[z, :, c]).astype(F32)).astype(F32)
        aw = (a * w[z]).astype(F32)
        before = P
        P = (P + aw).astype(F32)
        p = before if defect == "exclusive prefix" else P
        g_s[z] = -p if defect == "missing tau" else (-tau * p).astype(F32)
    return w, grey, g_s


DEFECTS = {"exclusive prefix": "g_s", "prefix from the far end": "g_s", "missing tau": "g_s", "dropped kappa": "w",
           "exclusive running sum": "w"}


def _emulation_case(C, scale):
    S, Q, gJ = _case(seed=21 + C, shape=(13, 6, 7), C=C, scale=scale)
    s32 = S.reshape(13, -1).numpy().astype(F32)
    Q32 = Q.reshape(13, -1, C).numpy().astype(F32)
    g32 = gJ.reshape(-1, C).numpy().astype(F32)
    g32[5] = 0.0                                                      # a ray of zero gradient
    s64, Q64, g64 = (torch.tensor(x.astype(np.float64)) for x in (s32, Q32, g32))
    zero = torch.zeros_like(s64)
    r = ER.ray(s64, zero, TAU, KAPPA)                                 # (the samples are exact here: es = eQ = 0)
    ab = ER.absorb(r["w"], r["e_w"], Q64, torch.zeros_like(Q64), g64, TAU)
    return s32, Q32, g32, r, ab


def _ratios(out, r, ab):
    w, grey, g_s = (torch.tensor(x.astype(np.float64)) for x in out)
    return {"w": VR.err_ratio((w - r["w"]).abs(), r["e_w"]), "grey": VR.err_ratio((grey - r["grey"]).abs(), r["e_grey"]),
            "g_s": VR.err_ratio((g_s - ab["g_s"]).abs(), ab["e_g_s"])}


@pytest.mark.parametrize("scale", [0.5, 6.0])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_float32_emulation_is_inside_every_bound_and_each_defect_leaves_one(C, scale):
    s32, Q32, g32, r, ab = _emulation_case(C, scale)
    good = _ratios(emulate(s32, Q32, g32, TAU, KAPPA), r, ab)
    print("float32 emulation C%d scale %g, err/bound: w %.3g  grey %.3g  g_s %.3g"
          % (C, scale, good["w"], good["grey"], good["g_s"]))
    assert max(good.values()) <= 1.0, good
    assert float(ab["g_s"].abs().max()) > 1e-3 and bool((ab["e_g_s"][:, 5] == 0).all())
    assert bool((emulate(s32, Q32, g32, TAU, KAPPA)[2][:, 5] == 0).all())
    for defect, where in DEFECTS.items():
        bad = _ratios(emulate(s32, Q32, g32, TAU, KAPPA, defect), r, ab)
        print("  %-24s err/bound: w %.3g  grey %.3g  g_s %.3g" % (defect, bad["w"], bad["grey"], bad["g_s"]))
        assert bad[where] > 1.0, (defect, bad)


def test_bounds_are_above_float32_rounding_of_the_inputs():
    """the bounds are not too tight: the reference evaluated on samples perturbed by half an ulp stays within them"""
    g = torch.Generator().manual_seed(5)
    s = torch.rand((17, 40), generator=g, dtype=torch.float64) * 6
    es = s * VR.EPS
    r = ER.ray(s, es, TAU, KAPPA)
    sign = torch.where(torch.rand(s.shape, generator=g) < 0.5, -1.0, 1.0).double()
    r2 = ER.ray(s + sign * es, torch.zeros_like(s), TAU, KAPPA)
    assert VR.err_ratio((r2["w"] - r["w"]).abs(), r["e_w"]) <= 1.0
    assert VR.err_ratio((r2["grey"] - r["grey"]).abs(), r["e_grey"]) <= 1.0


# ---- the flags --------------------------------------------------------------------------------------------------------

def test_exposure_is_a_colour_render_and_colour_exposure_a_flag():
    from neural_flow_style_amd import config
    assert "exposure" in config.COLOUR_RENDERS
    cfg, rest = config.get_config(["--colour_render", "exposure", "--colour_exposure", "2.5"])
    assert not rest and cfg.colour_render == "exposure" and cfg.colour_exposure == 2.5
    bare, _ = config.get_config([])
    assert not hasattr(bare, "colour_exposure") and config.complete(bare).colour_exposure == 1.0
    assert config.check_colour_render(cfg, colour=True) == ("exposure", (1.0, 1.0, 1.0))
    assert config.colour_exposure(cfg.colour_exposure) == 2.5 and config.colour_exposure(None) == 1.0
    other = type("Cfg", (), {"seed": 1})()
    assert config.complete(other).colour_exposure == 1.0
    for bad in (0.0, -1.0, float("nan"), float("inf"), "bright"):
        with pytest.raises(ValueError, match="colour_exposure"):
            config.colour_exposure(bad)


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


@pytest.fixture
def no_network(monkeypatch):
    from neural_flow_style_amd import styler_base

    def refuse(self, cfg):
        raise AssertionError("the base class was reached: the refusal came too late")
    monkeypatch.setattr(styler_base.StylerBase, "__init__", refuse)


@pytest.mark.parametrize("module", ["styler_3p", "styler_grid"])
def test_constructor_refusals_come_before_a_network_is_loaded(module, no_network):
    Styler = _styler(module)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="colour_exposure"):
            Styler(_cfg(colour_render="exposure", colour_exposure=bad, **COLOUR[module]))
        with pytest.raises(ValueError, match="colour_exposure"):        # (checked whatever the render is)
            Styler(_cfg(colour_exposure=bad, **COLOUR[module]))
        with pytest.raises(ValueError, match="colour_exposure"):
            Styler(_cfg(colour_render="liquid", colour_exposure=bad, **COLOUR[module]))
    with pytest.raises(ValueError, match="colour_exposure") as e:    # 'exposure' without a colour variable
        Styler(_cfg(colour_render="exposure", **{k: v for k, v in COLOUR[module].items() if k == "resolution"}))
    assert "colour variable" in str(e.value) and "colour_render" in str(e.value)
    with pytest.raises(ValueError, match="render_liquid"):           # the standing refusal, whatever the colour render
        Styler(_cfg(colour_render="exposure", render_liquid=True, **COLOUR[module]))


def test_the_2d_particle_stylizer_refuses_it(no_network):
    with pytest.raises(ValueError, match="colour_exposure") as e:
        _styler("styler_2p")(_cfg(colour_render="exposure", target_field="c"))
    assert "colour variable" in str(e.value)
    with pytest.raises(ValueError, match="colour_exposure"):
        _styler("styler_2p")(_cfg(colour_exposure=0.0, target_field="c"))


def _pc_config(**over):
    from tests import colour_runs as RUNS
    kw = dict(colour_render="exposure", transmit=0.2)
    kw.update(over)
    return RUNS.base_config([17, 12, 12], "pc", **kw)


@pytest.mark.parametrize("over,flag", [
    (dict(colour_exposure=0.0), "colour_exposure"), (dict(colour_exposure=float("nan")), "colour_exposure"),
    (dict(style_mask=True), "style_mask"), (dict(render_liquid=True), "render_liquid"), (dict(ray_mode="max"), "ray_mode"),
    (dict(w_density=1.0), "w_density"), (dict(style_mask_on_ref=True), "style_mask_on_ref"), (dict(pg=object()), "pg"),
    (dict(colour_lr_scale=0.0), "colour_lr_scale"), (dict(colour_background=[0.1, 0.2]), "colour_background"),
])
def test_constructor_refusals_of_pc_under_exposure(over, flag, no_network):
    from neural_flow_style_amd.styler_3p import Styler
    with pytest.raises(ValueError, match=flag):
        Styler(_pc_config(**over))


@pytest.mark.parametrize("over", [dict(), dict(colour_exposure=2.0), dict(w_pressure=10.0)])
def test_pc_accepts_exposure(over, monkeypatch):
    """the constructor gets as far as the base class (on the parent commit 'exposure' is no colour render)"""
    from neural_flow_style_amd import styler_base
    from neural_flow_style_amd.styler_3p import Styler

    class Reached(Exception):
        pass

    def reached(self, cfg):
        raise Reached()
    monkeypatch.setattr(styler_base.StylerBase, "__init__", reached)
    with pytest.raises(Reached):
        Styler(_pc_config(**over))
    for module in ("styler_3p", "styler_grid"):
        with pytest.raises(Reached):
            _styler(module)(_cfg(colour_render="exposure", **COLOUR[module]))
    # the smoke render's refusal still names the flag
    with pytest.raises(ValueError, match="colour_render"):
        Styler(_pc_config(colour_render="smoke"))


def test_engine_constructor_and_absorb_refusals():
    from neural_flow_style_amd import engine
    masked = types.SimpleNamespace(style_mask=True)
    plain = types.SimpleNamespace(style_mask=False)
    loss = engine.ColourRenderLoss(plain, 0.2, 3, "exposure", exposure=2.0)
    assert loss.fixed_exposure and not loss.liquid and loss.exposure == 2.0 and loss.v_batch == 3
    assert engine.ColourRenderLoss(plain, 0.2, render="exposure").exposure == 1.0
    assert not engine.ColourRenderLoss(plain, 0.2, render="liquid").fixed_exposure
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="colour_exposure"):
            engine.ColourRenderLoss(plain, 0.2, render="exposure", exposure=bad)
    with pytest.raises(ValueError, match="style_mask.*clip\\(grey"):
        engine.ColourRenderLoss(masked, 0.2, render="exposure").loss_and_grad(None, {}, absorb=True)
    with pytest.raises(ValueError, match="spent"):
        engine.ColourRenderLoss(plain, 0.2, render="exposure").loss_and_grad(None, {"spent": True}, absorb=True)
    with pytest.raises(ValueError, match="smoke colour render.*maximum"):     # the standing refusal and its message
        engine.ColourRenderLoss(plain, 0.2, render="smoke").loss_and_grad(None, {}, absorb=True)


# ---- the binding --------------------------------------------------------------------------------------------------------

NAMES = {"nfs_exposure_version", "nfs_exposure_weights", "nfs_exposure_absorb_bwd"}
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def test_the_open_table_holds_exposure():
    assert "exposure" in _lib.SIDE_OPEN
    r = _lib.SIDE_OPEN["exposure"]
    assert r.key == "exposure" and r.version_fn == "nfs_exposure_version"
    assert os.path.basename(r.path) == "libnfs_exposure.so" and os.path.dirname(r.path) == os.path.dirname(_lib.LIB_PATH)
    assert r.header_path == os.path.join(os.path.dirname(_lib.HEADER_PATH), "nfs_exposure.h")
    assert not (set(_lib.SIDE_OPEN) & (set(_lib.SIDE) | set(_lib.SIDE_LATER)))


def test_header_binding_and_exported_symbols_are_one_set():
    r = _built().SIDE_OPEN["exposure"]
    declared = SL._declared(r.header_path)
    assert declared == NAMES == set(r.signatures) == set(r.restypes)
    assert SL._defined(r.path) == declared
    assert getattr(_lib.side("exposure"), r.version_fn)() == r.abi == 100
    assert _lib.side("exposure") is r.handle
    assert r.signatures["nfs_exposure_weights"] == [_P, _P, _F, _F, _P, _P] + [_I] * 4 + [_P]
    assert r.signatures["nfs_exposure_absorb_bwd"] == [_P] * 4 + [_F, _P] + [_I] * 5 + [_P]
    assert r.signatures["nfs_exposure_version"] == [] and all(t is ctypes.c_int for t in r.restypes.values())


def test_no_name_is_shared_with_any_other_library():
    _built()
    r = _lib.SIDE_OPEN["exposure"]
    closed = list(_lib.SIDE.values()) + list(_lib.SIDE_LATER.values())
    others = [(_lib.HEADER_PATH, _lib.LIB_PATH)] + [(o.header_path, o.path) for o in closed]
    others += [(o.header_path, o.path) for o in _lib.SIDE_OPEN.values() if o is not r]
    assert len(others) >= 7
    for header, path in others:
        assert not (SL._declared(header) & SL._declared(r.header_path)), header
        assert not (SL._defined(path) & SL._defined(r.path)), path
    assert all(_lib._OWNER_OPEN[n] is r for n in NAMES) and not (NAMES & set(_lib._OWNER)) and not (NAMES & set(_lib.SIGNATURES))


def test_call_routes_to_it_and_side_finds_the_open_table():
    _built()
    assert _lib.side("exposure") is _lib.SIDE_OPEN["exposure"].handle
    with pytest.raises(KeyError):
        _lib.side("nothing")
    for name, args in (("nfs_exposure_weights", (None, None, 0.2, 1.0, None, None, 1, 1, 1, 1, None)),
                       ("nfs_exposure_absorb_bwd", (None, None, None, None, 0.2, None, 1, 1, 1, 1, 3, None))):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args)
        assert e.value.code == _lib.NFS_EINVAL and e.value.name == name
        assert _lib.lib().nfs_last_error().decode().startswith(name + ": null pointer")


def test_a_name_shared_with_any_other_table_is_refused():
    r = _lib.SIDE_OPEN["exposure"]
    for taken in ("nfs_liquid_weights", "nfs_liquid_absorb_bwd", "nfs_ray_weights"):      # SIDE, SIDE_LATER, SIDE
        twin = types.SimpleNamespace(signatures={taken: []}, header_path="include/nfs_twin.h")
        with pytest.raises(_lib.NfsLibraryError, match=taken):
            _lib._owners_open([r, twin], _lib._OWNER)
    twin = types.SimpleNamespace(signatures={"nfs_rotate_fwd": []}, header_path="include/nfs_twin.h")    # nfs_hip.h
    assert "nfs_rotate_fwd" in _lib.SIGNATURES
    with pytest.raises(_lib.NfsLibraryError, match="nfs_rotate_fwd"):
        _lib._owners_open([r, twin], _lib._OWNER)
    twin = types.SimpleNamespace(signatures={"nfs_exposure_weights": []}, header_path="include/nfs_twin.h")   # the open table
    with pytest.raises(_lib.NfsLibraryError, match="nfs_exposure_weights"):
        _lib._owners_open([r, twin], _lib._OWNER)
    fine = types.SimpleNamespace(signatures={"nfs_twin_version": []}, header_path="include/nfs_twin.h")
    assert _lib._owners_open([r, fine], _lib._OWNER)["nfs_twin_version"] is fine


def test_a_stale_version_is_refused_either_way():
    r = _built().SIDE_OPEN["exposure"]
    for abi, text in ((r.abi + 1, "the library is stale"), (r.abi - 1, "the header is stale")):
        with pytest.raises(_lib.NfsLibraryError, match=text):
            _lib._open(os.path.basename(r.path), r.path, r.header_path, r.signatures, r.restypes, r.version_fn, abi)


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch; tests/test_exposure_kernels_gpu.py repeats the refusals on device buffers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
def test_every_argument_refusal():
    _built()
    V, D, H, W, C = 2, 3, 4, 5, 3
    block = ctypes.create_string_buffer(8192)
    base = ctypes.addressof(block)
    # g_img 480 B, q 720, d 240, rot 72, w 480, grey 160, g_s 480: 1 KiB apart
    g_img, q, d, rot, w, grey, g_s = [base + 1024 * i for i in range(7)]
    nan, inf = float("nan"), float("inf")

    def refused(name, args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg

    name, ok = "nfs_exposure_weights", [d, rot, 0.2, 1.0, w, grey, V, D, H, W]
    for i in (0, 1, 4):                                              # d, rot and w are required; grey may be null
        args = list(ok)
        args[i] = None
        refused(name, args, "null pointer")
    for i in range(6, 10):
        for bad in (0, -1):
            args = list(ok)
            args[i] = bad
            refused(name, args, "at least 1")
    refused(name, ok[:6] + [1, 1024, 1024, 1024], "below 2^30")
    refused(name, ok[:6] + [4, 1024, 512, 512], "below 2^30")
    for bad in (0.0, -0.2, nan, inf, -inf):
        refused(name, ok[:2] + [bad] + ok[3:], "tau must be finite and positive")
        refused(name, ok[:3] + [bad] + ok[4:], "gain must be finite and positive")
    for i in (0, 1):
        for off in (0, 8):
            args = list(ok)
            args[4] = ok[i] + off
            refused(name, args, "w must not alias")
    for i in (0, 1, 4):
        for off in (0, 8):
            args = list(ok)
            args[5] = ok[i] + off
            refused(name, args, "grey must not alias")

    name, ok = "nfs_exposure_absorb_bwd", [g_img, q, rot, w, 0.2, g_s, V, D, H, W, C]
    for i in (0, 1, 2, 3, 5):
        args = list(ok)
        args[i] = None
        refused(name, args, "null pointer")
    for i in range(6, 10):
        for bad in (0, -1):
            args = list(ok)
            args[i] = bad
            refused(name, args, "at least 1")
    for bad in (0, 5, -1):
        refused(name, ok[:10] + [bad], "C must be 1..4")
    refused(name, ok[:6] + [1, 1024, 1024, 1024, C], "below 2^30")
    for bad in (0.0, -0.2, nan, inf):
        refused(name, ok[:4] + [bad] + ok[5:], "tau must be finite and positive")
    for i in (0, 1, 2):
        for off in (0, 8):
            args = list(ok)
            args[5] = ok[i] + off
            refused(name, args, "g_s must not alias")
    for off in (16, -16):                                            # w itself is allowed, a shifted w is not
        args = list(ok)
        args[5] = w + off
        refused(name, args, "g_s may be w itself")


# ---- the inputs of the GPU stylizer tests, on the reference alone -----------------------------------------------------

def test_the_absorbing_path_carries_its_share_of_the_joint_gradient():
    """the scene of tests/joint_runs.py under colour_render 'exposure' at kappa = 1, DENSITY SCALE 1 (the particle scene as
    it is, transmit 0.2, the three uniform views): the grey image has pixels below 0.1 and above 0.5 of its ceiling, and the
    part of d loss / d v that goes through the absorbing volume is at least 0.1 of the whole in L2 (so a gradient without
    the new adjoint cannot pass 1e-3)"""
    from tests import absorb_ref as AR
    from tests import joint_runs as JR
    sc = JR.scene()
    cfg = JR.ref_cfg(colour_render="exposure", w_tv=0.05)
    p, r = torch.tensor(sc["p"][0]).double(), torch.tensor(sc["r"][0]).double()
    v, c = torch.tensor(sc["v"]).double(), torch.tensor(sc["c_init"][0]).double()
    R = torch.tensor(np.asarray(JR.uniform_views(), np.float32)).double()
    e = AR.O.smooth3d_relu(AR.raw_volume(p + v, cfg, JR.RES), cfg["k"])[0, ..., 0]
    _, grey, S = ER.weights(e, R, ER.tau_of(cfg), ER.kappa_of(cfg))
    t = torch.exp(-ER.tau_of(cfg) * S.sum(1))
    print("grey image in [%.3f, %.3f], 1 - t in [%.3f, %.3f]" % (float(grey.min()), float(grey.max()), float((1 - t).min()),
                                                                 float((1 - t).max())))
    assert float((grey - (1 - t)).max()) <= 1e-15
    assert float((1 - t).min()) < 0.1 and float((1 - t).max()) > 0.5
    full = dict(cfg, v_batch=3)
    _, g_all, _ = ER.joint_loss_and_grad(p, r, v, c, full, JR.RES, R, sc["w64"], sc["sfe"])
    _, g_emit, _ = ER.joint_loss_and_grad(p, r, v, c, full, JR.RES, R, sc["w64"], sc["sfe"], absorbing=False)
    share = float((g_all - g_emit).norm() / g_all.norm())
    print("the absorbing path carries %.3g of |d loss / d v|" % share)
    assert share >= 0.1

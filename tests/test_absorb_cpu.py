"""The liquid colour render's derivative in the density, without a GPU: the closed form of tests/absorb_ref.py against
autograd of the float64 model, the telescoping identity, psi's two forms, the binding of libnfs_absorb.so (the second table
_lib.SIDE_LATER), the entry point's refusals, the constructor refusals of target_field 'pc', and the conditions on the inputs
of the GPU tests (tests/test_joint_stylizer_gpu.py), checked on the reference alone."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from neural_flow_style_amd import _lib
from tests import absorb_ref as AR
from tests import colour_liquid_ref as LR
from tests import colour_ref as CR
from tests import test_side_libraries_cpu as SL

TAU = 0.2


def _built():
    SL._built()
    if not all(os.path.exists(r.path) for r in _lib.SIDE_LATER.values()):
        _lib.build()
    return _lib


# ---- the arithmetic ---------------------------------------------------------------------------------------------------

def _case(seed=3, shape=(9, 4, 5), C=3):
    g = torch.Generator().manual_seed(seed)
    S = torch.rand(shape, generator=g, dtype=torch.float64) * 6.0
    S[:, 0, 0] = 0.0                                                  # an empty ray
    S[2, 1, 1] = 0.0                                                  # a zero sample inside a ray
    Q = torch.rand(shape + (C,), generator=g, dtype=torch.float64)
    gJ = torch.randn(shape[1:] + (C,), generator=g, dtype=torch.float64)
    bg = torch.tensor([0.2, 0.6, 0.05, 0.4], dtype=torch.float64)[:C]
    return S, Q, gJ, bg


@pytest.mark.parametrize("C", [1, 3])
def test_closed_form_equals_autograd_of_the_model(C):
    S, Q, gJ, bg = _case(C=C)
    Sv = S.clone().requires_grad_()
    J = AR.model_image(Sv, Q, bg, TAU)
    (want,) = torch.autograd.grad((J * gJ).sum(), Sv)
    got = AR.closed_form(S, Q, gJ, bg, TAU)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print("closed form against autograd: %.3g relative (scale %.3g)" % (err, float(want.abs().max())))
    assert err <= 1e-12


def test_closed_form_equals_autograd_through_the_rotation():
    """the same through LR.weights / LR.image on a volume and three views: g_S scattered by the rotation's transpose is
    autograd's gradient in d"""
    shape = (7, 5, 6)
    g = torch.Generator().manual_seed(8)
    d = torch.rand(shape, generator=g, dtype=torch.float64) * 4.0
    q = torch.rand(shape + (3,), generator=g, dtype=torch.float64)
    R = CR.views().double()[:3]
    gJ = torch.randn((3,) + shape[1:] + (3,), generator=g, dtype=torch.float64)
    bg = [0.2, 0.6, 0.05]
    dv = d.clone().requires_grad_()
    w, t, S = LR.weights(dv, R, TAU)
    (want,) = torch.autograd.grad((LR.image(q, R, w, t, bg) * gJ).sum(), dv)
    Sd = CR.rotate(d.unsqueeze(-1), R)[..., 0].clone().requires_grad_()
    Qr = CR.rotate(q, R)
    g_S = torch.stack([AR.closed_form(Sd[v].detach(), Qr[v], gJ[v], torch.tensor(bg, dtype=torch.float64), TAU)
                       for v in range(3)])
    dv2 = d.clone().requires_grad_()
    (got,) = torch.autograd.grad((CR.rotate(dv2.unsqueeze(-1), R)[..., 0] * g_S).sum(), dv2)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print("through the rotation: %.3g relative" % err)
    assert err <= 1e-12


def test_the_total_derivative_is_constant_along_a_ray():
    """Q = kappa_c S: g_S[z] + w[z] sum_c g kappa = -tau t sum_c g (bg - kappa) for every z"""
    S, _, gJ, bg = _case()
    kappa = torch.tensor([0.3, 0.7, 0.55], dtype=torch.float64)
    Q = S.unsqueeze(-1) * kappa
    g_S = AR.closed_form(S, Q, gJ, bg, TAU)
    B = torch.flip(torch.cumsum(torch.flip(S, [0]), 0), [0]) - S
    w = TAU * torch.exp(-TAU * B) * LR.phi(TAU * S)
    t = torch.exp(-TAU * S.sum(0))
    lhs = g_S + w * (gJ * kappa).sum(-1)
    rhs = -TAU * t * (gJ * (bg - kappa)).sum(-1)
    err = float((lhs - rhs.unsqueeze(0)).abs().max())
    print("telescoping identity: %.3g" % err)
    assert float(rhs.abs().max()) > 1e-3 and err <= 1e-12


def test_psi_series_and_quotient_agree_where_both_are_accurate():
    """between 0.05 and 0.3 the five-term series truncates below x^9 / 47900160 < 5e-13 and the quotient cancels 2 ulp / x
    < 1e-14; the limit, the tail and the kernel's change of form"""
    x = torch.linspace(0.05, 0.3, 101, dtype=torch.float64)
    assert float((AR.psi_series(x) - AR.psi_quotient(x)).abs().max()) <= 1e-12
    assert float(AR.psi(torch.zeros(1, dtype=torch.float64))) == -0.5
    assert float(AR.psi(torch.tensor([-0.0], dtype=torch.float64))) == -0.5
    big = torch.tensor([50.0, 200.0, 1e4], dtype=torch.float64)
    assert bool(torch.isfinite(AR.psi(big)).all()) and float((AR.psi(big) * big + 1).abs().max()) < 1e-12
    # at the kernel's threshold the series' truncation is what the bound's docstring says
    one = torch.tensor([AR.PSI_SERIES_BELOW], dtype=torch.float64)
    assert float((AR.psi_series(one) - AR.psi_quotient(one)).abs()) < 2.1e-8
    # psi = phi' / phi
    xs = torch.linspace(0.1, 5, 50, dtype=torch.float64).requires_grad_()
    (dphi,) = torch.autograd.grad(LR.phi(xs).sum(), xs)
    assert float((dphi / LR.phi(xs.detach()) - AR.psi(xs.detach())).abs().max()) <= 1e-12


# ---- the binding --------------------------------------------------------------------------------------------------------

NAMES = {"nfs_absorb_version", "nfs_liquid_absorb_bwd"}
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def test_the_second_table_holds_absorb_and_the_first_its_five_keys():
    assert list(_lib.SIDE) == SL.KEYS and list(_lib.SIDE_LATER) == ["absorb"]
    r = _lib.SIDE_LATER["absorb"]
    assert r.key == "absorb" and r.version_fn == "nfs_absorb_version"
    assert os.path.basename(r.path) == "libnfs_absorb.so" and os.path.dirname(r.path) == os.path.dirname(_lib.LIB_PATH)
    assert r.header_path == os.path.join(os.path.dirname(_lib.HEADER_PATH), "nfs_absorb.h")


def test_header_binding_and_exported_symbols_are_one_set():
    r = _built().SIDE_LATER["absorb"]
    declared = SL._declared(r.header_path)
    assert declared == NAMES == set(r.signatures) == set(r.restypes)
    assert SL._defined(r.path) == declared
    assert getattr(_lib.side("absorb"), r.version_fn)() == r.abi == 100
    assert _lib.side("absorb") is r.handle
    assert r.signatures["nfs_liquid_absorb_bwd"] == [_P] * 7 + [_F, _P] + [_I] * 5 + [_P]
    assert r.signatures["nfs_absorb_version"] == [] and all(t is ctypes.c_int for t in r.restypes.values())


def test_no_name_is_shared_with_the_other_six_libraries():
    _built()
    r = _lib.SIDE_LATER["absorb"]
    others = [(_lib.HEADER_PATH, _lib.LIB_PATH)] + [(o.header_path, o.path) for o in _lib.SIDE.values()]
    assert len(others) == 6
    for header, path in others:
        assert not (SL._declared(header) & SL._declared(r.header_path)), header
        assert not (SL._defined(path) & SL._defined(r.path)), path
    assert all(_lib._OWNER[n] is r for n in NAMES)
    assert set(_lib._OWNER) == set().union(*[set(o.signatures) for o in list(_lib.SIDE.values()) + [r]])


def test_call_routes_to_it_and_side_finds_either_table():
    _built()
    for key in list(_lib.SIDE) + ["absorb"]:
        assert _lib.side(key) is (_lib.SIDE.get(key) or _lib.SIDE_LATER[key]).handle
    with pytest.raises(KeyError):
        _lib.side("nothing")
    with pytest.raises(_lib.NfsError) as e:
        _lib.call("nfs_liquid_absorb_bwd", *([None] * 7), 0.2, None, 1, 1, 1, 1, 3, None)
    assert e.value.code == _lib.NFS_EINVAL and e.value.name == "nfs_liquid_absorb_bwd"
    assert _lib.lib().nfs_last_error().decode().startswith("nfs_liquid_absorb_bwd: null pointer")


def test_a_name_declared_twice_across_the_tables_is_refused():
    r = _lib.SIDE_LATER["absorb"]
    twin = types.SimpleNamespace(signatures={"nfs_liquid_weights": []}, header_path="include/nfs_twin.h")
    with pytest.raises(_lib.NfsLibraryError, match="nfs_liquid_weights"):
        _lib._owners(list(_lib.SIDE.values()) + [r, twin])
    twin = types.SimpleNamespace(signatures={"nfs_liquid_absorb_bwd": []}, header_path="include/nfs_twin.h")
    with pytest.raises(_lib.NfsLibraryError, match="nfs_liquid_absorb_bwd"):
        _lib._owners(list(_lib.SIDE.values()) + [r, twin])


def test_a_stale_version_is_refused_either_way():
    r = _built().SIDE_LATER["absorb"]
    for abi, text in ((r.abi + 1, "the library is stale"), (r.abi - 1, "the header is stale")):
        with pytest.raises(_lib.NfsLibraryError, match=text):
            _lib._open(os.path.basename(r.path), r.path, r.header_path, r.signatures, r.restypes, r.version_fn, abi)


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch; tests/test_absorb_kernels_gpu.py repeats the refusals on device buffers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
def test_every_argument_refusal():
    _built()
    V, D, H, W, C = 2, 3, 4, 5, 3
    block = ctypes.create_string_buffer(16384)
    base = ctypes.addressof(block)
    # g_img 480 B, q 720, d 240, rot 72, w 480, t_total 160, bg 12, g_s 480: 1 KiB apart
    g_img, q, d, rot, w, t, bg, g_s = [base + 1024 * i for i in range(8)]
    ok = [g_img, q, d, rot, w, t, bg, 0.2, g_s, V, D, H, W, C]

    def refused(args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call("nfs_liquid_absorb_bwd", *args, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith("nfs_liquid_absorb_bwd:") and text in msg, msg

    for i in (0, 1, 2, 3, 4, 5, 6, 8):                               # every pointer is required
        args = list(ok)
        args[i] = None
        refused(args, "null pointer")
    for i in range(9, 13):                                           # every size below 1
        for bad in (0, -1):
            args = list(ok)
            args[i] = bad
            refused(args, "at least 1")
    for bad in (0, 5, -1):
        refused(ok[:13] + [bad], "C must be 1..4")
    refused(ok[:9] + [1, 1024, 1024, 1024, C], "below 2^30")
    refused(ok[:9] + [4, 1024, 512, 512, C], "below 2^30")
    for i in (0, 1, 2, 3, 5, 6):                                     # g_s on an input, or overlapping one
        for off in (0, 8):
            args = list(ok)
            args[8] = ok[i] + off
            if i == 6 and off:
                args[8] = ok[i] - 8                                  # (bg is 12 bytes: a range that reaches it from below)
            refused(args, "g_s must not alias")
    for off in (16, -16):                                            # w itself is allowed, a shifted w is not
        args = list(ok)
        args[8] = w + off
        refused(args, "g_s may be w itself")


# ---- target_field 'pc': flags and refusals, before a network is loaded -----------------------------------------------

def test_pc_is_a_target_field_and_colour_lr_scale_a_flag():
    from neural_flow_style_amd.config import check_colour_render, complete, get_config
    cfg, rest = get_config(["--target_field", "pc", "--colour_render", "liquid", "--colour_lr_scale", "5"])
    assert not rest and cfg.target_field == "pc" and cfg.colour_lr_scale == 5.0
    bare, _ = get_config([])
    assert not hasattr(bare, "colour_lr_scale") and complete(bare).colour_lr_scale == 1.0
    assert check_colour_render(cfg, colour=True)[0] == "liquid"


def _pc_config(**over):
    from tests import colour_runs as RUNS
    kw = dict(colour_render="liquid", transmit=0.2)
    kw.update(over)
    return RUNS.base_config([17, 12, 12], "pc", **kw)


@pytest.mark.parametrize("over,flag", [
    (dict(colour_render=""), "colour_render"), (dict(colour_render="smoke"), "colour_render"),
    (dict(style_mask=True), "style_mask"), (dict(render_liquid=True), "render_liquid"), (dict(ray_mode="max"), "ray_mode"),
    (dict(w_density=1.0), "w_density"), (dict(style_mask_on_ref=True), "style_mask_on_ref"), (dict(pg=object()), "pg"),
    (dict(colour_lr_scale=0.0), "colour_lr_scale"), (dict(colour_lr_scale=-2.0), "colour_lr_scale"),
    (dict(colour_lr_scale=float("nan")), "colour_lr_scale"), (dict(colour_background=[0.1, 0.2]), "colour_background"),
])
def test_constructor_refusals_of_pc(over, flag, monkeypatch):
    from neural_flow_style_amd import styler_base
    from neural_flow_style_amd.styler_3p import Styler

    def no_network(self, cfg):
        raise AssertionError("the base class was reached: the refusal came too late")
    monkeypatch.setattr(styler_base.StylerBase, "__init__", no_network)
    with pytest.raises(ValueError, match=flag):
        Styler(_pc_config(**over))


def test_pc_allows_w_pressure(monkeypatch):
    """the positions move, so the pressure term is allowed: the constructor gets as far as the base class"""
    from neural_flow_style_amd import styler_base
    from neural_flow_style_amd.styler_3p import Styler

    class Reached(Exception):
        pass

    def reached(self, cfg):
        raise Reached()
    monkeypatch.setattr(styler_base.StylerBase, "__init__", reached)
    with pytest.raises(Reached):
        Styler(_pc_config(w_pressure=10.0))


def test_engine_refuses_absorb_where_it_is_not_built():
    from neural_flow_style_amd import engine
    masked = types.SimpleNamespace(style_mask=True)
    plain = types.SimpleNamespace(style_mask=False)
    with pytest.raises(ValueError, match="smoke colour render.*maximum"):
        engine.ColourRenderLoss(plain, 0.2, render="").loss_and_grad(None, {}, absorb=True)
    with pytest.raises(ValueError, match="style_mask.*mask 1 - t"):
        engine.ColourRenderLoss(masked, 0.2, render="liquid").loss_and_grad(None, {}, absorb=True)
    with pytest.raises(ValueError, match="spent"):
        engine.ColourRenderLoss(plain, 0.2, render="liquid").loss_and_grad(None, {"spent": True}, absorb=True)


# ---- the inputs of the GPU stylizer tests, on the reference alone -----------------------------------------------------

def test_the_joint_scene_is_opaque_enough_and_the_absorbing_path_carries_its_share():
    """the particle scene of tests/colour_liquid_runs.py displaced by RandomState(77).uniform(-0.02, 0.02): at transmit 0.2
    and the three uniform views the grey liquid image has pixels below 0.1 and above 0.5, and the part of d loss / d v that
    goes through the absorbing volume is at least 0.1 of the whole in L2 (so a gradient without it cannot pass 1e-3)"""
    from tests import joint_runs as JR
    sc = JR.scene()
    cfg = JR.ref_cfg(w_tv=0.05)
    p, r = torch.tensor(sc["p"][0]).double(), torch.tensor(sc["r"][0]).double()
    v, c = torch.tensor(sc["v"]).double(), torch.tensor(sc["c_init"][0]).double()
    R = torch.tensor(np.asarray(JR.uniform_views(), np.float32)).double()
    e = AR.O.smooth3d_relu(AR.raw_volume(p + v, cfg, JR.RES), cfg["k"])[0, ..., 0]
    _, t, _ = LR.weights(e, R, LR.tau_of(cfg))
    grey = 1 - t
    print("grey liquid image in [%.3f, %.3f]" % (float(grey.min()), float(grey.max())))
    assert float(grey.min()) < 0.1 and float(grey.max()) > 0.5
    full = dict(cfg, v_batch=3)
    _, g_all, _ = AR.joint_loss_and_grad(p, r, v, c, full, JR.RES, R, sc["w64"], sc["sfe"])
    _, g_emit, _ = AR.joint_loss_and_grad(p, r, v, c, full, JR.RES, R, sc["w64"], sc["sfe"], absorbing=False)
    share = float((g_all - g_emit).norm() / g_all.norm())
    print("the absorbing path carries %.3g of |d loss / d v|" % share)
    assert share >= 0.1

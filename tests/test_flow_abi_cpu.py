"""libnfs_flow.so and --carrier_steps without a GPU: include/nfs_flow.h parses and states its constant, 'flow' is a bound key
of the open table _lib.SIDE_OPEN with both entry points and the version, the library exports exactly what the header
declares, the flag parses and defaults, the constructor refusals come before a network is loaded, and the entry points
refuse what the header says they refuse."""
import ctypes
import os

import pytest
import torch

from neural_flow_style_amd import _lib
from tests import test_side_libraries_cpu as SL

NAMES = {"nfs_flow_version", "nfs_flow_fwd", "nfs_flow_bwd"}
_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _built():
    SL._built()
    if not all(os.path.exists(r.path) for r in _lib.SIDE_OPEN.values()):
        _lib.build()
    return _lib


# ---- the header and the binding --------------------------------------------------------------------------------------

def test_the_header_parses_and_states_its_constant():
    r = _lib.SIDE_OPEN["flow"]
    sigs, restypes, structs, consts = _lib._read(r.header_path)
    assert set(sigs) == NAMES == SL._declared(r.header_path) and not structs
    assert consts["NFS_FLOW_ABI_VERSION"] == 100 == r.abi
    assert sigs["nfs_flow_version"] == []
    assert sigs["nfs_flow_fwd"] == [_P] * 3 + [_I] * 4 + [_L, _I, _I, _P]
    assert sigs["nfs_flow_bwd"] == [_P] * 4 + [_I] * 4 + [_L, _I, _I, _P]
    assert all(t is ctypes.c_int for t in restypes.values())


def test_the_open_table_holds_flow_and_the_closed_tables_do_not():
    assert "flow" in _lib.SIDE_OPEN and "flow" not in _lib.SIDE and "flow" not in _lib.SIDE_LATER
    r = _lib.SIDE_OPEN["flow"]
    assert r.key == "flow" and r.version_fn == "nfs_flow_version"
    assert os.path.basename(r.path) == "libnfs_flow.so" and os.path.dirname(r.path) == os.path.dirname(_lib.LIB_PATH)
    assert r.header_path == os.path.join(os.path.dirname(_lib.HEADER_PATH), "nfs_flow.h")
    assert all(_lib._OWNER_OPEN[n] is r for n in NAMES) and not (NAMES & set(_lib._OWNER)) and not (NAMES & set(_lib.SIGNATURES))


def test_the_library_exports_what_the_header_declares():
    r = _built().SIDE_OPEN["flow"]
    assert SL._defined(r.path) == NAMES == set(r.signatures) == set(r.restypes)
    assert getattr(_lib.side("flow"), r.version_fn)() == r.abi == 100
    assert _lib.side("flow") is r.handle
    others = [_lib.LIB_PATH] + [o.path for o in list(_lib.SIDE.values()) + list(_lib.SIDE_LATER.values())]
    others += [o.path for o in _lib.SIDE_OPEN.values() if o is not r]
    for path in others:
        assert not (SL._defined(path) & NAMES), path


def test_the_makefile_builds_it_as_a_side_library_on_the_shared_axis_rule():
    text = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    side = [line for line in text.splitlines() if line.startswith("SIDE ")][0].split(":=")[1].split()
    assert "flow" in side and os.path.exists(os.path.join(_lib.CSRC_DIR, "flow.hip"))
    body = open(os.path.join(_lib.CSRC_DIR, "flow.hip")).read()
    # it includes the axis rule and the derivative weights, and defines neither
    assert '#include "g2p_axis.h"' in body and "void g2p_axis(" not in body and "void g2p_axis_d(" not in body
    assert "g2p_axis_d(" in body and "__fadd_rn(" in body and "__fmul_rn(" in body
    axis = open(os.path.join(_lib.CSRC_DIR, "g2p_axis.h")).read()
    assert "void g2p_axis(" in axis and "void g2p_axis_d(" in axis


# ---- the flag ----------------------------------------------------------------------------------------------------------

def test_the_flag_parses_and_defaults():
    from neural_flow_style_amd import config
    cfg, rest = config.get_config(["--target_field", "g", "--carrier_steps", "4", "--resolution", "16", "24", "40"])
    assert not rest and cfg.carrier_steps == 4 and config.check_carrier_steps(cfg) == 4
    assert config.check_carrier(cfg) == ((2, 3, 5), True)                   # (its two-tuple stays)
    bare, _ = config.get_config(["--resolution", "16", "24", "40"])
    assert not hasattr(bare, "carrier_steps") and config.check_carrier_steps(bare) == 1
    assert config.complete(bare).carrier_steps == 1
    assert config.complete(cfg).carrier_steps == 4
    group = [g for g in config.parser._action_groups if g.title == "MI355X"][0]
    assert "carrier_steps" in [a.dest for a in group._group_actions]
    for bad in (0, -1, 2.5, "many", True, [2], float("nan"), float("inf")):
        cfg.carrier_steps = bad
        with pytest.raises(ValueError, match="carrier_steps"):
            config.check_carrier_steps(cfg)
    for good, want in ((1, 1), (7, 7), (3.0, 3), (None, 1)):
        cfg.carrier_steps = good
        assert config.check_carrier_steps(cfg) == want


def _cfg(target="g", **over):
    from tests import colour_runs as RUNS
    kw = dict(carrier_resolution=[4, 5, 3]) if target == "g" else {}
    kw.update(over)
    return RUNS.base_config([16, 16, 16], target, **kw)


@pytest.fixture
def no_network(monkeypatch):
    from neural_flow_style_amd import styler_base

    def refuse(self, cfg):
        raise AssertionError("the base class was reached: the refusal came too late")
    monkeypatch.setattr(styler_base.StylerBase, "__init__", refuse)


@pytest.mark.parametrize("target,over", [
    ("g", dict(carrier_steps=0)), ("g", dict(carrier_steps=-3)), ("g", dict(carrier_steps=2.5)),
    ("g", dict(carrier_steps="four")), ("g", dict(carrier_steps=True)),
    ("p", dict(carrier_steps=4)), ("d", dict(carrier_steps=2)), ("pd", dict(carrier_steps=3)), ("p", dict(carrier_steps=0)),
])
def test_constructor_refusals_come_before_a_network_is_loaded(target, over, no_network):
    from neural_flow_style_amd.styler_3p import Styler
    with pytest.raises(ValueError, match="carrier_steps"):
        Styler(_cfg(target, **over))


def test_the_2d_particle_stylizer_still_refuses_the_carrier(no_network):
    from neural_flow_style_amd.styler_2p import Styler
    with pytest.raises(ValueError, match="3-D only"):
        Styler(_cfg("g", carrier_steps=4))


def test_the_constructor_accepts_it(monkeypatch):
    from neural_flow_style_amd import styler_base
    from neural_flow_style_amd.styler_3p import Styler

    class Reached(Exception):
        pass

    def reached(self, cfg):
        raise Reached()
    monkeypatch.setattr(styler_base.StylerBase, "__init__", reached)
    for target, over in (("g", dict(carrier_steps=4)), ("g", dict(carrier_steps=1)), ("g", dict()),
                         ("g", dict(carrier_steps=8, carrier_interp="linear", w_pressure=10.0)),
                         ("p", dict(carrier_steps=1)), ("p", dict())):
        with pytest.raises(Reached):
            Styler(_cfg(target, **over))


# ---- the entry points' refusals ---------------------------------------------------------------------------------------

def test_call_routes_to_it():
    _built()
    for name, args in (("nfs_flow_fwd", (None, None, None, 3, 1, 1, 1, 1, 1, 1, None)),
                       ("nfs_flow_bwd", (None, None, None, None, 3, 1, 1, 1, 1, 1, 1, None))):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args)
        assert e.value.code == _lib.NFS_EINVAL and e.value.name == name
        assert _lib.lib().nfs_last_error().decode().startswith(name + ": null pointer")


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch; tests/test_flow_kernels_gpu.py repeats the refusals on device buffers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
def test_every_argument_refusal():
    _built()
    block = ctypes.create_string_buffer(8192)
    base = ctypes.addressof(block)
    # N 8, nd 3, K 4, grid 2 x 3 x 4: u 288 B, p 96, path 480, g_out 96, lam 480: 1 KiB apart
    u, p, path, g_out, lam = [base + 1024 * i for i in range(5)]

    def refused(name, args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg

    for name, ok, n_ptr, outputs in (("nfs_flow_fwd", [u, p, path, 3, 2, 3, 4, 8, 4, 1], 3, (2,)),
                                     ("nfs_flow_bwd", [u, path, g_out, lam, 3, 2, 3, 4, 8, 4, 1], 4, (3,))):
        for i in range(n_ptr):
            refused(name, ok[:i] + [None] + ok[i + 1:], "null pointer")
        for bad in (1, 4, 0, -3):
            refused(name, ok[:n_ptr] + [bad] + ok[n_ptr + 1:], "nd must be 2 or 3")
        for i in (n_ptr + 1, n_ptr + 2, n_ptr + 3):
            for bad in (0, -1):
                refused(name, ok[:i] + [bad] + ok[i + 1:], "at least 1")
        refused(name, ok[:n_ptr + 4] + [-1] + ok[n_ptr + 5:], "at least 0")
        for bad in (0, -1, -7):
            refused(name, ok[:n_ptr + 5] + [bad] + ok[n_ptr + 6:], "K, the number of steps, must be at least 1")
        refused(name, ok[:n_ptr + 4] + [2 ** 60, 4] + ok[n_ptr + 6:], "below 2^62")
        refused(name, ok[:n_ptr + 4] + [2 ** 40, 2 ** 31 - 1] + ok[n_ptr + 6:], "below 2^62")
        out = outputs[0]
        for i in range(n_ptr):
            if i == out:
                continue
            for off in (0, 8):
                args = list(ok)
                args[out] = ok[i] + off
                refused(name, args, "must not alias")
            args = list(ok)                                                  # (the output ends inside the input)
            args[out] = ok[i] - 476
            refused(name, args, "must not alias")
    # nd 2: Z is not read
    _lib.call("nfs_flow_fwd", u, p, path, 2, 2, 3, 0, 0, 4, 1, None)
    _lib.call("nfs_flow_bwd", u, path, g_out, lam, 2, 2, 3, -5, 0, 4, 0, None)
    # N == 0 succeeds with nothing launched (there is no device here to launch on)
    _lib.call("nfs_flow_fwd", u, p, path, 3, 2, 3, 4, 0, 1, 1, None)
    _lib.call("nfs_flow_bwd", u, path, g_out, lam, 3, 2, 3, 4, 0, 1, 1, None)

"""libnfs_carrier.so and target_field 'g' without a GPU: include/nfs_carrier.h parses and states its constants, 'carrier' is
a bound key of the open table _lib.SIDE_OPEN with both entry points and the version, the library exports exactly what the
header declares, the flags parse and default, every constructor refusal comes before a network is loaded, and the entry
points refuse what the header says they refuse."""
import ctypes
import os

import pytest
import torch

from neural_flow_style_amd import _lib
from tests import test_side_libraries_cpu as SL

NAMES = {"nfs_carrier_version", "nfs_carrier_displace", "nfs_carrier_bwd"}
_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _built():
    SL._built()
    if not all(os.path.exists(r.path) for r in _lib.SIDE_OPEN.values()):
        _lib.build()
    return _lib


# ---- the header and the binding --------------------------------------------------------------------------------------

def test_the_header_parses_and_states_its_constants():
    r = _lib.SIDE_OPEN["carrier"]
    sigs, restypes, structs, consts = _lib._read(r.header_path)
    assert set(sigs) == NAMES == SL._declared(r.header_path) and not structs
    assert consts["NFS_CARRIER_ABI_VERSION"] == 100 == r.abi
    assert consts["NFS_CARRIER_BLOCK"] == 256 and consts["NFS_CARRIER_QUANTUM_LOG2"] == -52
    assert sigs["nfs_carrier_version"] == []
    assert sigs["nfs_carrier_displace"] == [_P] * 4 + [_I] * 4 + [_L, _I, _P]
    assert sigs["nfs_carrier_bwd"] == [_P] * 4 + [_I] * 5 + [_L, _I, _I, _P]
    assert all(t is ctypes.c_int for t in restypes.values())


def test_the_open_table_holds_carrier_and_the_closed_tables_do_not():
    assert "carrier" in _lib.SIDE_OPEN and "carrier" not in _lib.SIDE and "carrier" not in _lib.SIDE_LATER
    r = _lib.SIDE_OPEN["carrier"]
    assert r.key == "carrier" and r.version_fn == "nfs_carrier_version"
    assert os.path.basename(r.path) == "libnfs_carrier.so" and os.path.dirname(r.path) == os.path.dirname(_lib.LIB_PATH)
    assert r.header_path == os.path.join(os.path.dirname(_lib.HEADER_PATH), "nfs_carrier.h")
    assert all(_lib._OWNER_OPEN[n] is r for n in NAMES) and not (NAMES & set(_lib._OWNER)) and not (NAMES & set(_lib.SIGNATURES))


def test_the_library_exports_what_the_header_declares():
    r = _built().SIDE_OPEN["carrier"]
    assert SL._defined(r.path) == NAMES == set(r.signatures) == set(r.restypes)
    assert getattr(_lib.side("carrier"), r.version_fn)() == r.abi == 100
    assert _lib.side("carrier") is r.handle
    others = [_lib.LIB_PATH] + [o.path for o in list(_lib.SIDE.values()) + list(_lib.SIDE_LATER.values())]
    others += [o.path for o in _lib.SIDE_OPEN.values() if o is not r]
    for path in others:
        assert not (SL._defined(path) & NAMES), path


def test_the_makefile_builds_it_as_a_side_library():
    text = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    side = [line for line in text.splitlines() if line.startswith("SIDE ")][0].split(":=")[1].split()
    assert "carrier" in side and os.path.exists(os.path.join(_lib.CSRC_DIR, "carrier.hip"))
    # the axis rule is one text for both libraries
    for src in ("splat.hip", "carrier.hip"):
        body = open(os.path.join(_lib.CSRC_DIR, src)).read()
        assert '#include "g2p_axis.h"' in body and "void g2p_axis(" not in body, src
    assert "void g2p_axis(" in open(os.path.join(_lib.CSRC_DIR, "g2p_axis.h")).read()


# ---- the flags ---------------------------------------------------------------------------------------------------------

def test_the_flags_parse_and_default():
    from neural_flow_style_amd import config
    cfg, rest = config.get_config(["--target_field", "g", "--carrier_resolution", "4", "5", "3", "--carrier_interp", "linear",
                                   "--resolution", "16", "24", "40"])
    assert not rest and cfg.target_field == "g" and cfg.carrier_resolution == [4, 5, 3] and cfg.carrier_interp == "linear"
    assert config.check_carrier(cfg) == ((4, 5, 3), False)
    bare, _ = config.get_config(["--resolution", "16", "24", "40"])
    assert not hasattr(bare, "carrier_resolution") and not hasattr(bare, "carrier_interp")
    assert config.check_carrier(bare) == ((2, 3, 5), True)              # (defaults without complete(), as the constructor sees them)
    done = config.complete(bare)
    assert done.carrier_resolution == [2, 3, 5] and done.carrier_interp == "cubic"
    assert config.complete(config.get_config(["--resolution", "200", "300", "200"])[0]).carrier_resolution == [25, 37, 25]
    assert config.default_carrier_resolution([8, 15, 100]) == [2, 2, 12]
    assert "g" in [a for a in config.parser._actions if a.dest == "target_field"][0].choices


def _cfg(**over):
    from tests import colour_runs as RUNS
    kw = dict(carrier_resolution=[4, 5, 3])
    kw.update(over)
    return RUNS.base_config([16, 16, 16], "g", **kw)


@pytest.fixture
def no_network(monkeypatch):
    from neural_flow_style_amd import styler_base

    def refuse(self, cfg):
        raise AssertionError("the base class was reached: the refusal came too late")
    monkeypatch.setattr(styler_base.StylerBase, "__init__", refuse)


@pytest.mark.parametrize("over,flag", [
    (dict(carrier_resolution=[4, 5]), "carrier_resolution"), (dict(carrier_resolution=[4, 5, 0]), "carrier_resolution"),
    (dict(carrier_resolution=[4, 5, -2]), "carrier_resolution"), (dict(carrier_resolution=[4, 5, 2.5]), "carrier_resolution"),
    (dict(carrier_resolution="coarse"), "carrier_resolution"), (dict(carrier_resolution=[4, 5, 3, 2]), "carrier_resolution"),
    (dict(carrier_resolution=7), "carrier_resolution"),
    (dict(carrier_interp="quintic"), "carrier_interp"), (dict(carrier_interp=""), "carrier_interp"),
    (dict(w_density=1.0), "w_density"), (dict(pg=object()), "pg"),
])
def test_constructor_refusals_come_before_a_network_is_loaded(over, flag, no_network):
    from neural_flow_style_amd.styler_3p import Styler
    with pytest.raises(ValueError, match=flag):
        Styler(_cfg(**over))


def test_the_2d_particle_stylizer_refuses_it(no_network):
    from neural_flow_style_amd.styler_2p import Styler
    with pytest.raises(ValueError, match="3-D only") as e:
        Styler(_cfg())
    assert "target_field 'g'" in str(e.value)


def test_the_constructor_accepts_it_and_run_refuses_a_process_group(monkeypatch):
    from neural_flow_style_amd import styler_base
    from neural_flow_style_amd.styler_3p import Styler

    class Reached(Exception):
        pass

    def reached(self, cfg):
        raise Reached()
    monkeypatch.setattr(styler_base.StylerBase, "__init__", reached)
    for over in (dict(), dict(carrier_interp="linear"), dict(w_pressure=10.0), dict(carrier_resolution=[1, 1, 1])):
        with pytest.raises(Reached):
            Styler(_cfg(**over))
    st = Styler.__new__(Styler)                                   # (run() refuses before it touches anything else)
    st._colour, st._joint, st._carrier, st.pg = False, False, True, object()
    with pytest.raises(ValueError, match="process group"):
        st.run({})


# ---- the entry points' refusals ---------------------------------------------------------------------------------------

def test_call_routes_to_it():
    _built()
    for name, args in (("nfs_carrier_displace", (None, None, None, None, 3, 1, 1, 1, 1, 1, None)),
                       ("nfs_carrier_bwd", (None, None, None, None, 3, 1, 1, 1, 1, 1, 1, 0, None))):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args)
        assert e.value.code == _lib.NFS_EINVAL and e.value.name == name
        assert _lib.lib().nfs_last_error().decode().startswith(name + ": null pointer")


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch; tests/test_carrier_kernels_gpu.py repeats the refusals on device buffers)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
def test_every_argument_refusal():
    _built()
    block = ctypes.create_string_buffer(8192)
    base = ctypes.addressof(block)
    # N 8, nd 3, C 3, grid 2 x 3 x 4: g_v 96 B, p 96, g_u 288, u 288, p_out 96, v_out 96, the counter 4: 1 KiB apart
    g_v, p, g_u, u, p_out, v_out, nbox = [base + 1024 * i for i in range(7)]

    def refused(name, args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg

    name, ok = "nfs_carrier_bwd", [g_v, p, g_u, nbox, 3, 2, 3, 4, 3, 8, 1, 0]
    for i in (0, 1, 2):                                              # the counter may be null
        args = list(ok)
        args[i] = None
        refused(name, args, "null pointer")
    for bad in (1, 4, 0, -3):
        refused(name, ok[:4] + [bad] + ok[5:], "nd must be 2 or 3")
    for i in (5, 6, 7, 8):
        for bad in (0, -1):
            args = list(ok)
            args[i] = bad
            refused(name, args, "at least 1")
    refused(name, ok[:9] + [-1] + ok[10:], "at least 0")
    for bad in (2, -1, 7):
        refused(name, ok[:11] + [bad], "route must be 0")
    refused(name, ok[:5] + [2048, 1024, 1024, 1] + ok[9:], "below 2^31")
    refused(name, ok[:5] + [1024, 1024, 512, 4] + ok[9:], "below 2^31")
    refused(name, ok[:4] + [2, 65536, 32768, 0, 1] + ok[9:], "below 2^31")      # (nd 2: Z is not read)
    for i in (0, 1):
        for off in (0, 8):
            args = list(ok)
            args[2] = ok[i] + off
            refused(name, args, "must not alias")
            args = list(ok)
            args[3] = ok[i] + off
            refused(name, args, "must not alias")
    refused(name, ok[:3] + [g_u + 16] + ok[4:], "must not alias")

    name, ok = "nfs_carrier_displace", [u, p, p_out, v_out, 3, 2, 3, 4, 8, 1]
    for i in (0, 1, 2):                                              # v_out may be null
        args = list(ok)
        args[i] = None
        refused(name, args, "null pointer")
    for bad in (1, 4, 0):
        refused(name, ok[:4] + [bad] + ok[5:], "nd must be 2 or 3")
    for i in (5, 6, 7):
        args = list(ok)
        args[i] = 0
        refused(name, args, "at least 1")
    refused(name, ok[:8] + [-1, 1], "at least 0")
    for out in (2, 3):
        for i in (0, 1):
            args = list(ok)
            args[out] = ok[i] + 8
            refused(name, args, "must not alias")
    refused(name, ok[:3] + [p_out + 4] + ok[4:], "must not alias")

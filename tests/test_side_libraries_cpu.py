"""The side libraries (one libnfs_<key>.so per key of _lib.SIDE) without a GPU: each exports exactly what its header
include/nfs_<key>.h declares and the binding binds, under the version the header states; no name lives in two of the six
libraries; _lib.call finds the library that owns a name; and the loader refuses a stale side, a missing header and a name
declared twice."""
import ctypes as C
import functools
import importlib.util
import os
import re
import shutil
import subprocess
import types

import pytest

from neural_flow_style_amd import _lib

KEYS = ["grid2d", "descent", "colour", "emission", "liquid"]
_P, _I, _F, _L = C.c_void_p, C.c_int, C.c_float, C.c_int64

NAMES = {
    "grid2d": {"nfs_grid2d_version", "nfs_source2d_velocity_fwd", "nfs_source2d_velocity_bwd", "nfs_advect2d_source_fwd",
               "nfs_advect2d_source_bwd", "nfs_advect2d_bwd_adam_fwd", "nfs_transport_step2d"},
    "descent": {"nfs_descent_version", "nfs_descent_step", "nfs_advect_descent_fwd", "nfs_advect2d_descent_fwd"},
    "colour": {"nfs_colour_version", "nfs_ray_weights", "nfs_colour_project_fwd", "nfs_colour_project_bwd"},
    "emission": {"nfs_emission_version", "nfs_emission_fwd", "nfs_emission_bwd", "nfs_emission_bwd_adam"},
    "liquid": {"nfs_liquid_version", "nfs_liquid_weights"},
}

# rows typed by hand from the two headers whose every entry point takes a different list
ROWS = {
    "grid2d": {
        "nfs_grid2d_version": [],
        "nfs_source2d_velocity_fwd": [_P, _I, _P, _I, _I, _P],
        "nfs_source2d_velocity_bwd": [_P, _I, _P, _I, _I, _P],
        "nfs_advect2d_source_fwd": [_P, _P, _I, _P, _I, _I, _P],
        "nfs_advect2d_source_bwd": [_P, _P, _I, _P, _P, _I, _I, _P],
        "nfs_advect2d_bwd_adam_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _F, _F, _F, _F, _P],
        "nfs_transport_step2d": [_P, _P, _F, _F, _P, _F, _P, _I, _I, _I, _P],
    },
    "descent": {
        "nfs_descent_version": [],
        "nfs_descent_step": [_P, _P, _L, _F, _P],
        "nfs_advect_descent_fwd": [_P, _P, _P, _F, _P, _P, _I, _I, _I, _P],
        "nfs_advect2d_descent_fwd": [_P, _P, _P, _F, _P, _I, _I, _P],
    },
}

# one entry point per library and arguments it refuses for a null pointer
REFUSED = {
    "grid2d": ("nfs_advect2d_source_fwd", (None, None, 0, None, 4, 4, None)),
    "descent": ("nfs_descent_step", (None, None, 4, 0.1, None)),
    "colour": ("nfs_ray_weights", (None, 0.1, None, 1, None, 1, 1, 1, 1, None)),
    "emission": ("nfs_emission_fwd", (None, None, None, 1, 3, None)),
    "liquid": ("nfs_liquid_weights", (None, None, 0.2, None, None, None, 1, 1, 1, 1, None)),
}


def _built():
    if not all(os.path.exists(p) for p in [_lib.LIB_PATH] + [r.path for r in _lib.SIDE.values()]):
        _lib.build()
    return _lib


@functools.lru_cache(maxsize=None)
def _defined(path):
    """the nfs_* symbols a shared object defines"""
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-nm")
    nm = nm if os.path.exists(nm) else shutil.which("nm")
    assert nm, "neither llvm-nm of the ROCm toolchain that built the library nor nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.split()}
    return frozenset(n for n in names if re.fullmatch(r"nfs_\w+", n))


def _declared(header_path):
    """the nfs_* names a header declares, read without the binding's reader"""
    hdr = re.sub(r"/\*.*?\*/", " ", open(header_path).read(), flags=re.S)
    return set(re.findall(r"\b(nfs_[a-z0-9_]+)\s*\(", hdr))


def test_the_table_holds_the_five_keys_in_order():
    assert list(_lib.SIDE) == KEYS
    for key, r in _lib.SIDE.items():
        assert r.key == key and r.version_fn == "nfs_%s_version" % key
        assert os.path.basename(r.path) == "libnfs_%s.so" % key and os.path.dirname(r.path) == os.path.dirname(_lib.LIB_PATH)
        assert r.header_path == os.path.join(os.path.dirname(_lib.HEADER_PATH), "nfs_%s.h" % key)


@pytest.mark.parametrize("key", list(_lib.SIDE))
def test_header_binding_and_exported_symbols_are_one_set(key):
    r = _built().SIDE[key]
    declared = _declared(r.header_path)
    assert declared == NAMES[key]
    assert declared == set(r.signatures) == set(r.restypes)
    assert _defined(r.path) == declared
    assert getattr(_lib.side(key), r.version_fn)() == r.abi == 100
    assert _lib.side(key) is r.handle


@pytest.mark.parametrize("key", sorted(ROWS))
def test_derived_binding_equals_the_rows_typed_by_hand(key):
    assert _lib.SIDE[key].signatures == ROWS[key]
    assert all(t is C.c_int for t in _lib.SIDE[key].restypes.values())


def test_no_name_lives_in_two_of_the_six_libraries():
    """libnfs_hip.so keeps its 134 entry points and its version; by declared names and by defined symbols the six are
    pairwise disjoint: nothing moved between them"""
    _built()
    hip = _defined(_lib.LIB_PATH)
    assert hip == set(_lib.SIGNATURES) and len(hip) == 134
    assert _lib.lib().nfs_version() == _lib.ABI_VERSION
    six = [(_lib.HEADER_PATH, _lib.LIB_PATH)] + [(r.header_path, r.path) for r in _lib.SIDE.values()]
    assert len(six) == 6
    for i in range(6):
        for j in range(i + 1, 6):
            for sets in ([_declared(six[i][0]), _declared(six[j][0])], [_defined(six[i][1]), _defined(six[j][1])]):
                assert sets[0] and sets[1] and not (sets[0] & sets[1]), (six[i][1], six[j][1], sets[0] & sets[1])


@pytest.mark.parametrize("key", list(_lib.SIDE))
def test_call_routes_a_name_to_the_library_that_declares_it(key):
    _built()
    name, args = REFUSED[key]
    assert _lib._OWNER[name] is _lib.SIDE[key]
    with pytest.raises(_lib.NfsError, match="%s: null pointer" % name) as e:
        _lib.call(name, *args)
    assert e.value.code == _lib.NFS_EINVAL


@pytest.mark.parametrize("key", list(_lib.SIDE))
def test_a_side_library_of_another_abi_version_is_refused_either_way(key, monkeypatch):
    """as for libnfs_hip.so: the message says which side is stale, and nothing is cached"""
    r = _built().SIDE[key]
    built = getattr(_lib.side(key), r.version_fn)()
    monkeypatch.setattr(r, "handle", None)
    for header, text in ((built + 1, "the library is stale"), (built - 1, "the header is stale")):
        monkeypatch.setattr(r, "abi", header)
        with pytest.raises(_lib.NfsLibraryError, match=text) as e:
            _lib.side(key)
        assert r.path in str(e.value) and "ABI %d" % built in str(e.value) and "declares %d" % header in str(e.value)
        assert r.handle is None


def test_a_missing_side_header_is_named(tmp_path):
    (tmp_path / "pkg").mkdir()
    (tmp_path / "include").mkdir()
    shutil.copy(_lib.__file__, tmp_path / "pkg" / "_lib.py")
    shutil.copy(_lib.HEADER_PATH, tmp_path / "include" / "nfs_hip.h")
    spec = importlib.util.spec_from_file_location("_lib_without_side_headers", tmp_path / "pkg" / "_lib.py")
    with pytest.raises(Exception) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "NfsLibraryError"
    assert os.path.join(str(tmp_path), "include", "nfs_grid2d.h") in str(e.value)


def test_a_name_declared_twice_is_refused_when_the_lookup_is_built():
    a = types.SimpleNamespace(header_path="nfs_a.h", signatures={"nfs_a_version": [], "nfs_both": [_P]})
    b = types.SimpleNamespace(header_path="nfs_b.h", signatures={"nfs_b_version": [], "nfs_both": [_P]})
    with pytest.raises(_lib.NfsLibraryError, match="nfs_both") as e:
        _lib._owners([a, b])
    assert "nfs_a.h" in str(e.value) and "nfs_b.h" in str(e.value)
    del b.signatures["nfs_both"]
    assert _lib._owners([a, b]) == {"nfs_a_version": a, "nfs_both": a, "nfs_b_version": b}
    # a name of nfs_hip.h is the main library's: a side header that declares it would take its calls
    b.signatures["nfs_fill"] = [_P]
    with pytest.raises(_lib.NfsLibraryError, match="nfs_fill") as e:
        _lib._owners([a, b])
    assert "nfs_b.h" in str(e.value) and _lib.HEADER_PATH in str(e.value)

"""CPU-side checks of the boundary: the C-ABI library loads, exports every symbol the
header declares, and the product path refuses to run without the HIP extension / a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ensure_built():
    from neural_flow_style_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_library_exports_every_declared_symbol():
    _lib = _ensure_built()
    hdr = open(os.path.join(ROOT, "include", "nfs_hip.h")).read()
    declared = set(re.findall(r"\b(nfs_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert L.nfs_version() >= 100


def test_library_defines_no_undeclared_symbol():
    """the reverse direction: every nfs_* symbol the product library defines is declared in the header"""
    _lib = _ensure_built()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-nm")
    nm = nm if os.path.exists(nm) else shutil.which("nm")
    assert nm, "neither llvm-nm of the ROCm toolchain that built the library nor nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.split()}
    defined = {n for n in defined if re.fullmatch(r"nfs_\w+", n)}
    assert len(defined) > 100, len(defined)
    assert defined == set(_lib.SIGNATURES), (defined ^ set(_lib.SIGNATURES))


_P, _I, _F, _L = C.c_void_p, C.c_int, C.c_float, C.c_int64


def test_derived_binding_equals_the_rows_typed_by_hand():
    """rows of the table _lib.py spelled by hand before it read the header (copied from it, not from the reader): every
    type spelling of the header, the long and the irregular rows"""
    from neural_flow_style_amd import _lib
    SplatCfg, ConvDesc = _lib.SplatCfg, _lib.ConvDesc
    rows = {
        "nfs_version": ([], C.c_int),
        "nfs_last_error": ([], C.c_char_p),
        "nfs_gemm_last": ([_P], C.c_int),
        "nfs_gemm_timer_read_kind": ([_I, _P, _P, _P, _P], C.c_int),
        "nfs_conv3x3_executed_flops": ([_I, _I, _I, _I, _I, _I], C.c_double),
        "nfs_conv3x3_plan": ([_I, _I, _I, _I, _I, _I, _P], C.c_int),
        "nfs_conv3x3_workspace_floats": ([_I, _I, _I, _I, _I], C.c_int64),
        "nfs_lap_up_rms": ([_P, _P, _F, _P, _P, _I, _L, _F, _P, _P, _I, _I, _I, _I, _I, _P], C.c_int),
        "nfs_maxpool3_fwd": ([_P, _P, _P, _I, _I, _I, _I, _I, _P], C.c_int),
        "nfs_advect_bwd_adam_fwd_live_ever": ([_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P], C.c_int),
        "nfs_adam_tf_step": ([_P, _P, _P, _P, _L, _F, _F, _F, _F, _P], C.c_int),
        "nfs_resize3d": ([_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P], C.c_int),
        "nfs_conv2d_fwd": ([_P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P], C.c_int),
        "nfs_p2g_wavg_bwd": ([_P, _P, _P, _P, _P, _P, _P, _I, _I, _F, C.POINTER(SplatCfg), _P], C.c_int),
        # (the descriptor array was a _P in that table: the header says what it points to)
        "nfs_conv2d_group": ([C.POINTER(ConvDesc), _I, _I, _P, _L, _P], C.c_int),
        "nfs_render_coef_layout": ([_I, _I, _I, _I, _P, _P], C.c_int),
        "nfs_conv2d_plan": ([_I, _I, _I, _I, _I, _I, _I, _I, _P], C.c_int),
        "nfs_conv2d_group_plan": ([C.POINTER(ConvDesc), _I, _I, _P], C.c_int),
    }
    assert len(rows["nfs_conv2d_fwd"][0]) == 23 and len(rows["nfs_resize3d"][0]) == 13
    for name, (argtypes, restype) in rows.items():
        assert _lib.SIGNATURES[name] == argtypes, name
        assert _lib.RESTYPES[name] is restype, name
    assert set(_lib.RESTYPES) == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 134
    assert (_lib.NFS_EINVAL, _lib.NFS_ELAUNCH) == (-1, -2)


_GOOD_HEADER = """
/* a header in the shape of nfs_hip.h: int nfs_in_a_comment(short x);
 */
#ifndef NFS_T_H
#define NFS_T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define NFS_OK 0
#define NFS_EBAD (-3)  /* why */
#define NFS_ABI_VERSION 12
typedef void* nfs_stream_t;
typedef struct {
  int nd;            /* 2 or 3 */
  int res[3];
  float radius, support;   // two at once
  const float* F;
  float* G;
  int B, Bs, C[2];
} nfs_cfg_t;
int nfs_a(const float* x, float* y, int n, float s, double d, int64_t k, const nfs_cfg_t* cfg,
          nfs_stream_t stream);
const char* nfs_b(void);
int64_t nfs_c(unsigned long long* m, const unsigned long long* k, const uint8_t* b, uint32_t* w);
double nfs_d(const long long* o, long long* p, double* t, int* i, const int* j);
#ifdef __cplusplus
}
#endif
#endif /* NFS_T_H */
"""


def test_reader_returns_exactly_what_a_small_header_declares():
    from neural_flow_style_amd import _lib
    signatures, restypes, structs, constants = _lib.read_header(_GOOD_HEADER)
    assert list(structs) == ["nfs_cfg_t"]
    cfg = structs["nfs_cfg_t"]
    assert issubclass(cfg, C.Structure) and cfg.__name__ == "nfs_cfg_t"
    assert cfg._fields_ == [("nd", _I), ("res", _I * 3), ("radius", _F), ("support", _F), ("F", _P), ("G", _P),
                            ("B", _I), ("Bs", _I), ("C", _I * 2)]
    assert signatures == {"nfs_a": [_P, _P, _I, _F, C.c_double, _L, C.POINTER(cfg), _P], "nfs_b": [],
                          "nfs_c": [_P, _P, _P, _P], "nfs_d": [_P, _P, _P, _P, _P]}
    assert restypes == {"nfs_a": C.c_int, "nfs_b": C.c_char_p, "nfs_c": C.c_int64, "nfs_d": C.c_double}
    assert constants == {"NFS_OK": 0, "NFS_EBAD": -3, "NFS_ABI_VERSION": 12}


@pytest.mark.parametrize("statement, quoted", [
    ("int nfs_f(const float* x, short n);", "short"),
    ("int nfs_f(unsigned n);", "unsigned"),
    ("int nfs_f(size_t n);", "size_t"),
    ("int nfs_f(const float* x, void (*done)(int));", "void (*done)(int)"),
    ("int nfs_f(int n, ...);", "..."),
    ("int nfs_f(int res[3]);", "int res[3]"),
    ("int nfs_f(const char* name);", "const char *"),
    ("void nfs_f(int n);", "void"),
    ("int other_f(int n);", "int other_f(int n)"),
    ("typedef struct { int n; size_t bytes; } nfs_s;", "size_t"),
    ("typedef struct { int n; float x } nfs_s;", "float x"),
    ("int nfs_f(const nfs_never_t* cfg);", "nfs_never_t"),
    ("int x;", "int x"),
    ("int nfs_f(int n)", "int nfs_f(int n)"),
])
def test_reader_refuses_what_is_outside_its_vocabulary(statement, quoted):
    """nothing is skipped or guessed: a declaration the reader cannot bind exactly raises and quotes it"""
    from neural_flow_style_amd import _lib
    text = "typedef void* nfs_stream_t;\nint nfs_ok(int n);\n%s\nint nfs_after(int n);\n" % statement
    with pytest.raises(_lib.NfsLibraryError) as e:
        _lib.read_header(text)
    assert quoted in str(e.value), str(e.value)


def test_a_missing_header_is_named(tmp_path):
    import importlib.util
    from neural_flow_style_amd import _lib
    (tmp_path / "pkg").mkdir()
    shutil.copy(_lib.__file__, tmp_path / "pkg" / "_lib.py")
    spec = importlib.util.spec_from_file_location("_lib_without_header", tmp_path / "pkg" / "_lib.py")
    with pytest.raises(Exception) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "NfsLibraryError"
    assert os.path.join(str(tmp_path), "include", "nfs_hip.h") in str(e.value)


def test_a_library_of_another_abi_version_is_refused_either_way(monkeypatch):
    """the binding is the header at hand: a library that reports another nfs_version(), older or newer, does not load,
    and the message says which side is stale"""
    _lib = _ensure_built()
    built = _lib.lib().nfs_version()
    monkeypatch.setattr(_lib, "_lib", None)
    for header, text in ((built + 1, "the library is stale"), (built - 1, "the header is stale")):
        monkeypatch.setattr(_lib, "ABI_VERSION", header)
        with pytest.raises(_lib.NfsLibraryError, match=text) as e:
            _lib.lib()
        assert "ABI %d" % built in str(e.value) and "declares %d" % header in str(e.value)
        assert _lib._lib is None


def test_struct_layouts_equal_the_compiler_s(tmp_path):
    """sizeof and every offsetof of the three structs as the host C compiler lays out nfs_hip.h, against the classes the
    reader generated (the field names are the reader's: a field it dropped or renamed does not compile or leaves a gap)"""
    from neural_flow_style_amd import _lib
    structs = {"nfs_splat_cfg": _lib.SplatCfg, "nfs_gram_layer_t": _lib.GramLayer, "nfs_conv2d_desc_t": _lib.ConvDesc}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "nfs_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (name, field, name, field, name, field))
    lines += ['  return 0;', '}', '']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"),
                    str(tmp_path / "layout.c")], check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {w[0]: tuple(int(v) for v in w[1:]) for w in (line.split() for line in out.splitlines())}
    want = {}
    for name, cls in structs.items():
        want[name] = (C.sizeof(cls),)
        for field, _ in cls._fields_:
            want["%s.%s" % (name, field)] = (getattr(cls, field).offset, getattr(cls, field).size)
    assert got == want
    assert [got[n] for n in structs] == [(52,), (72,), (104,)]
    assert sum(len(cls._fields_) for cls in structs.values()) == 9 + 12 + 19


def test_a_descriptor_array_casts_as_the_benchmark_reads_it():
    """the grouped entry points take the ctypes array itself; bench.py reads the recorded argument back through a cast
    to a pointer to the whole array"""
    from neural_flow_style_amd import _lib
    arr = (_lib.GramLayer * 2)()
    arr[0].HW, arr[0].C, arr[1].HW, arr[1].C, arr[1].scale = 81, 512, 129, 256, 0.5
    back = C.cast(arr, C.POINTER(_lib.GramLayer * 2)).contents
    assert [(y.HW, y.C) for y in back] == [(81, 512), (129, 256)] and back[1].scale == 0.5
    assert C.addressof(back) == C.addressof(arr)
    assert _lib.SIGNATURES["nfs_gram_group_bwd"][0].from_param(arr) is not None        # accepted as the argument
    with pytest.raises(TypeError):                                                     # (what the old cast produced)
        _lib.SIGNATURES["nfs_gram_group_bwd"][0].from_param(C.c_void_p(C.addressof(arr)))


def test_argument_errors_do_not_need_a_gpu():
    _lib = _ensure_built()
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("nfs_render_fwd", None, None, None, 1, 1, 1, 1, 0.1, 0, None)
    assert _lib.lib().nfs_version() >= _lib.ABI_VERSION                              # the binding's header and the library
    assert _lib.ABI_VERSION == _lib.lib().nfs_version()
    assert _lib.lib().nfs_maxnorm_workspace_floats(3) == 2 * 32 * 3                  # (sum, ties) x 32 blocks x groups
    assert _lib.lib().nfs_conv3x3_packed_floats(3, 64, 0) == 9 * 3 * 64              # conv1_1: direct only
    # + Winograd F(4x4,3x3) filters (36 floats per (ci, co))
    # + the same filters in MFMA fragment order, for the 32x32x2 and the 16x16x4 instruction (36 + 36)
    # + the 16x16x4 pack as three bf16 limb planes for the split-limb GEMM (6 bytes per value: 54)
    # + where both channel counts are >= 128: the F(5x5,3x3) filters, their fragment order (49 + 49) and its limb planes (73.5)
    assert _lib.lib().nfs_conv3x3_packed_floats(256, 512, 0) == (9 + 36 + 36 + 36 + 54 + 98) * 256 * 512 + 147 * 256 * 512 // 2
    # narrow layers (64 / 128 channels both sides): + the filters in the fragment order of the single-kernel path
    assert _lib.lib().nfs_conv3x3_packed_floats(64, 128, 0) == (9 + 36 + 36 + 36 + 54 + 36) * 64 * 128


# the eight entry points that run only on the four-voxel advect kernel: name -> (number of pointer arguments before D, H, W
# (d is the first, g_out the third); of them the index of adv_next, or None; takes a slab (z0, nz) after D, H, W)
_ADVECT_X4 = {
    "nfs_advect_fwd_live": (4, None, False),
    "nfs_advect_bwd_adam": (5, None, False),
    "nfs_advect_bwd_adam_fwd": (6, 5, False),
    "nfs_advect_bwd_adam_fwd_live": (7, 5, False),
    "nfs_advect_bwd_adam_fwd_live_ever": (8, 5, False),
    "nfs_advect_fwd_slab": (3, None, True),
    "nfs_advect_bwd_adam_slab": (5, None, True),
    "nfs_advect_bwd_adam_fwd_slab": (6, 5, True),
}


# (the pointers below are host memory that must never reach a kernel: with a device present a bug in the code under test
# would turn a failed assertion into a launch)
@pytest.mark.skipif(torch.cuda.is_available(), reason="passes dummy host pointers: only where nothing can be launched")
@pytest.mark.parametrize("name", sorted(_ADVECT_X4))
def test_four_voxel_advect_entry_points_refuse_before_any_launch(name):
    """shapes the four-voxel kernel does not take, a slab outside the volume and an adv_next that aliases d come back as
    NFS_EINVAL with a text that names the entry point and the requirement"""
    import ctypes
    _lib = _ensure_built()
    nptr, adv, slab = _ADVECT_X4[name]
    bufs = [ctypes.create_string_buffer(64) for _ in range(nptr)]           # distinct, non-null, never dereferenced
    ptrs = [ctypes.addressof(b) for b in bufs]
    adam = () if "adam" not in name else (1e-3, 0.9, 0.999, 1e-8)

    def refused(ptrs, D, H, W, z0, nz, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *ptrs, D, H, W, *((z0, nz) if slab else ()), *adam, None)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg

    refused(ptrs, 3, 3, 3, 0, 3, "needs D, H, W >= 2")                        # 27 voxels: no multiple of 4
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        refused(ptrs, *shape, 0, shape[0], "needs D, H, W >= 2")
    if slab:
        refused(ptrs, 4, 4, 4, 2, 3, "slab outside the volume")
        refused(ptrs, 4, 4, 4, -1, 2, "slab outside the volume")
        refused(ptrs, 4, 4, 4, 0, 0, "slab outside the volume")
        refused(ptrs, 4, 3, 3, 1, 1, "needs D, H, W >= 2")                     # 36 voxels, but a slab of 9
    if adv is not None:
        refused(ptrs[:adv] + [ptrs[0]] + ptrs[adv + 1:], 4, 4, 4, 0, 4, "adv_next must not alias d or g_out")
        refused(ptrs[:adv] + [ptrs[2]] + ptrs[adv + 1:], 4, 4, 4, 0, 4, "adv_next must not alias d or g_out")
        # the alias check comes before the shape check
        refused(ptrs[:adv] + [ptrs[0]] + ptrs[adv + 1:], 3, 3, 3, 0, 3, "adv_next must not alias d or g_out")
    for i in range(nptr):
        refused(ptrs[:i] + [None] + ptrs[i + 1:], 4, 4, 4, 0, 4, "null pointer")


def test_no_cpu_fallback():
    import neural_flow_style_amd.ops as ops
    with pytest.raises(ValueError):
        ops.render_fwd(torch.zeros(1, 2, 2, 2), 0.1)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "neural-flow-style_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("no oracle", ""), os.path.join(dirpath, f)


def test_view_sampling_shapes_and_determinism():
    import neural_flow_style_amd.transform as T
    mats, views = T.rot_mat(-5, 5, 5, -10, 10, 10, sample_type="uniform")
    assert len(mats) == 9 and views[0] == {"phi": -5.0, "theta": -10.0}
    # R = Ry(theta) @ Rz(phi), orthonormal
    for m in mats:
        np.testing.assert_allclose(m @ m.T, np.eye(3), atol=1e-12)
    np.testing.assert_allclose(mats[4], np.eye(3), atol=1e-12)
    a, va = T.rot_mat(-5, 5, 5, -10, 10, 10, "poisson", np.random.RandomState(123), nv=8)
    b, vb = T.rot_mat(-5, 5, 5, -10, 10, 10, "poisson", np.random.RandomState(123), nv=8)
    assert len(a) == 8 and va == vb
    for v in va[:-1]:
        assert -5 <= v["phi"] <= 5 and -10 <= v["theta"] <= 10
    # Poisson-disc property: pairwise distance >= r = max(units)/2
    pts = np.array([[v["theta"], v["phi"]] for v in T.rot_mat_poisson(-5, 5, 5, -10, 10, 10, np.random.RandomState(1))])
    dist = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(len(pts)) * 1e9
    assert dist.min() >= 5.0 - 1e-9


def test_config_surface_matches_the_reference_defaults():
    """every flag of the reference's config.get_config() (fixture generated from the reference itself by
    tests/golden/make_config_fixture.py) exists with the same default; the build adds only documented extras"""
    import json
    import os
    from neural_flow_style_amd.config import get_config
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_defaults.json")))
    mine = vars(get_config([])[0])
    assert len(ref) >= 60
    for k, v in ref.items():
        assert k in mine, k
        got = mine[k]
        assert (list(got) if isinstance(got, (list, tuple)) else got) == v, (k, got, v)
    assert set(mine) - set(ref) == {"views_mode", "grid_variable", "synthetic_weights", "transport_recursive", "ray_mode"}


def test_product_library_has_no_wrong_result_ablation_switches():
    """the timing-only ablation branches (NFS_GEMM_DBG / NFS_CONV_DBG: skip loads, stores or MFMAs, wrong results by
    construction) exist only in ``make ABLATE=1`` builds: the product library must not even contain the variable names"""
    import os
    from neural_flow_style_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"NFS_GEMM_DBG", b"NFS_CONV_DBG"):
        assert name not in blob, name

"""CPU-side checks of the boundary: the C-ABI library loads, exports every symbol the
header declares, and the product path refuses to run without the HIP extension / a GPU."""
import os
import re

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


def test_argument_errors_do_not_need_a_gpu():
    _lib = _ensure_built()
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("nfs_render_fwd", None, None, None, 1, 1, 1, 1, 0.1, 0, None)
    assert _lib.lib().nfs_version() >= _lib.ABI_VERSION                              # the binding's table and the library
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

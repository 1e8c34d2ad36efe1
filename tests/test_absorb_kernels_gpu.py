"""libnfs_absorb.so element by element: nfs_liquid_absorb_bwd's g_s against the float64 closed form of tests/absorb_ref.py,
each element within its own float32 error bound, on every shape of tests/colour_ref.py and its four views, with three
channels and with one; the ray of zero gradient; the underflowing ray; the telescoping identity; g_s written over w; volumes
one cell wide (the kernel's scalar stencil); a NaN sample; the refusals on device buffers.  Every check prints the largest
err / bound it saw (pytest -s).

The volume is tests/test_liquid_kernels_gpu.py's (an empty ray, a ray of -0.0, tau S = 1e-7, both sides of phi's change of
form, a ray whose t is below the smallest normal float32) with, besides, a ray whose samples lie on both sides of psi's own
change of form at tau S = 1 and one sample with tau S = 34, past the start of psi's tail.  w and t_total are what
ops.liquid_weights wrote for it: the kernel reads those, the reference its own float64 values, and the bounds of both
(LR.ray) enter the bound.  tau = 0.2."""
import math

import numpy as np
import pytest
import torch

from tests import absorb_ref as AR
from tests import colour_ref as CR
from tests import view_ref as VR
from tests.test_liquid_kernels_gpu import TAU, TAU32, volume as liquid_volume

pytestmark = pytest.mark.gpu

DEV = "cuda"
BG = [0.2, 0.6, 0.05, 0.4]                                        # not white (the first C entries)


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


@pytest.fixture(scope="module")
def views():
    return CR.views(DEV)


def check(name, got, ref, bound):
    r = VR.err_ratio((got.double() - ref.double()).abs(), bound)
    print("%-60s max err/bound %.3g" % (name, r))
    assert r <= 1.0, (name, r)
    return r


def volume(shape):
    d = liquid_volume(shape)
    step = AR.PSI_SERIES_BELOW / TAU
    d[0::2, 2, 1] = step * (1 - 2.0 ** -10)                          # both sides of psi's change of form
    d[1::2, 2, 1] = step * (1 + 2.0 ** -10)
    d[0, 3, 0] = 34.0 / TAU                                          # psi's tail (and an opaque sample at the near end)
    return d


def inputs(shape, V, C, seed=11):
    gen = torch.Generator(device="cpu").manual_seed(seed + C)
    q = torch.rand(shape + (C,), generator=gen, dtype=torch.float64).float().to(DEV)
    g = torch.randn((V,) + shape[1:] + (C,), generator=gen, dtype=torch.float64).float()
    g[1, 0, 0, :] = 0.0                                              # a ray of exact zeros
    return q, g.to(DEV), torch.tensor(BG[:C], dtype=torch.float32, device=DEV)


_cache = {}


def case(ops, views, shape, C):
    """inputs, the kernel's weights and g_s, and per view the reference (AR.view): computed once and left alone"""
    key = (shape, C)
    if key not in _cache:
        d = volume(shape)
        V = views.shape[0]
        q, g, bg = inputs(shape, V, C)
        w, _, t = ops.liquid_weights(d, views, TAU)
        g_s = ops.liquid_absorb_bwd(g, q, d, views, w, t, bg, TAU)
        refs = [AR.view(VR.Stencil(views[v], shape), d.double(), q.double(), g[v].double(), bg.double(), TAU32)
                for v in range(V)]
        _cache[key] = dict(d=d, q=q, g=g, bg=bg, w=w, t=t, g_s=g_s, refs=refs)
    return _cache[key]


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_liquid_absorb_bwd(ops, views, shape, C):
    k = case(ops, views, shape, C)
    V = views.shape[0]
    assert tuple(k["g_s"].shape) == (V,) + shape
    for v, (r, s, es) in enumerate(k["refs"]):
        check("absorb g_s %s C%d v%d" % (shape, C, v), k["g_s"][v], r["g_s"], r["e_g_s"])
        # what the kernel read is within its own bounds of what the reference used
        check("  its w %s v%d" % (shape, v), k["w"][v], r["w"], r["e_w"])
        check("  its t %s v%d" % (shape, v), k["t"][v], r["t"], r["e_t"])
    g_s = k["g_s"]
    assert bool(torch.isfinite(g_s).all())
    assert bool((g_s[1, :, 0, 0] == 0).all())                        # the ray of zero gradient: exact zeros
    assert 0.0 <= float(k["t"][0, 2, 0]) < 2.0 ** -126 and bool(torch.isfinite(g_s[0, :, 2, 0]).all())
    assert float(g_s.abs().max()) > 1e-3
    # the identity view's rays really take every branch of psi
    x = TAU32 * k["refs"][0][1]
    assert bool((x[:, 2, 1] < AR.PSI_SERIES_BELOW).any()) and bool((x[:, 2, 1] > AR.PSI_SERIES_BELOW).any())
    assert float(x[0, 3, 0]) > 32


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_the_total_derivative_is_constant_along_a_ray(ops, views, shape):
    """q = kappa_c d: g_s[z] + w[z] sum_c g kappa = -tau t sum_c g (bg - kappa) for every z, the kernel's g_s and w against
    the reference's t, within the summed bounds (g_s's own and |sum_c g kappa| e_w)"""
    k = case(ops, views, shape, 3)
    kappa = torch.tensor([0.3, 0.7, 0.55], dtype=torch.float32, device=DEV)
    q = (k["d"].unsqueeze(-1) * kappa).contiguous()
    g_s = ops.liquid_absorb_bwd(k["g"], q, k["d"], views, k["w"], k["t"], k["bg"], TAU)
    for v in range(views.shape[0]):
        st = VR.Stencil(views[v], shape)
        g64 = k["g"][v].double()
        r, _, _ = AR.view(st, k["d"].double(), q.double(), g64, k["bg"].double(), TAU32)
        gk = (g64 * kappa.double()).sum(-1)
        lhs = g_s[v].double() + k["w"][v].double() * gk
        rhs = (-TAU32 * r["t"] * (g64 * (k["bg"].double() - kappa.double())).sum(-1)).unsqueeze(0).expand_as(lhs)
        ref_lhs = r["g_s"] + r["w"] * gk
        # (in float64 the identity holds to the rounding of q = kappa d in float32, which the reference samples too)
        assert float((ref_lhs - rhs).abs().max()) <= 1e-5 * (1 + float(rhs.abs().max()))
        check("telescoping %s v%d" % (shape, v), lhs, ref_lhs, r["e_g_s"] + gk.abs() * r["e_w"])


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_written_over_the_weights_it_is_the_same_bits(ops, views, shape, C):
    k = case(ops, views, shape, C)
    w2 = k["w"].clone()
    out = ops.liquid_absorb_bwd(k["g"], k["q"], k["d"], views, w2, k["t"], k["bg"], TAU, out=w2)
    assert out.data_ptr() == w2.data_ptr()
    assert torch.equal(w2, k["g_s"]) and not torch.equal(w2, k["w"])


@pytest.mark.parametrize("shape", [(5, 4, 1), (6, 1, 1), (1, 3, 1)], ids=str)
def test_a_volume_one_cell_wide(ops, views, shape):
    """W == 1: there is no x-pair to load, so the kernel takes the scalar stencil (tri_setup); the same bounds, all views"""
    gen = torch.Generator(device="cpu").manual_seed(5)
    d = (torch.rand(shape, generator=gen, dtype=torch.float64) * 6.0).float()
    if shape[1] > 1:
        d[:, 0, 0] = 0.0                                             # an empty ray beside the others
    d = d.to(DEV)
    V = views.shape[0]
    for C in (3, 1):
        q, g, bg = inputs(shape, V, C)
        w, _, t = ops.liquid_weights(d, views, TAU)
        g_s = ops.liquid_absorb_bwd(g, q, d, views, w, t, bg, TAU)
        assert tuple(g_s.shape) == (V,) + shape and bool(torch.isfinite(g_s).all())
        for v in range(V):
            r, _, _ = AR.view(VR.Stencil(views[v], shape), d.double(), q.double(), g[v].double(), bg.double(), TAU32)
            check("absorb g_s %s C%d v%d" % (shape, C, v), g_s[v], r["g_s"], r["e_g_s"])
        assert bool((g_s[1, :, 0, 0] == 0).all())
        w2 = w.clone()
        ops.liquid_absorb_bwd(g, q, d, views, w2, t, bg, TAU, out=w2)
        assert torch.equal(w2, g_s)


def test_a_nan_sample_poisons_its_own_ray_only(ops, views):
    """a NaN voxel of d reaches the rays whose stencil holds it (at the identity: its own column, and neighbours only
    through a corner of weight zero); every other ray is what it was, bit for bit"""
    shape = (17, 6, 9)
    k = case(ops, views, shape, 3)
    eye = views[:1].contiguous()
    g = k["g"][:1].contiguous()
    w, _, t = ops.liquid_weights(k["d"], eye, TAU)
    good = ops.liquid_absorb_bwd(g, k["q"], k["d"], eye, w, t, k["bg"], TAU)
    bad = k["d"].clone()
    z0, y0, x0 = 9, 3, 4
    bad[z0, y0, x0] = float("nan")
    w2, _, t2 = ops.liquid_weights(bad, eye, TAU)
    got = ops.liquid_absorb_bwd(g, k["q"], bad, eye, w2, t2, k["bg"], TAU)
    far = torch.ones(shape[1:], dtype=torch.bool, device=DEV)
    far[y0 - 1:y0 + 2, x0 - 1:x0 + 2] = False
    assert torch.equal(got[0][:, far], good[0][:, far])
    assert bool(torch.isnan(got[0, :, y0, x0]).all())               # t is NaN on its own ray: every sample of it
    assert int(torch.isnan(got[0]).any(0).sum()) <= 9


def test_refusals_on_device_buffers(ops, views):
    from neural_flow_style_amd import _lib
    shape = (3, 4, 5)
    V, C = views.shape[0], 3
    k = case(ops, views, shape, C)
    g_s = torch.empty((V,) + shape, device=DEV)
    P = lambda x: x.data_ptr()
    ok = [P(k["g"]), P(k["q"]), P(k["d"]), P(views), P(k["w"]), P(k["t"]), P(k["bg"]), TAU, P(g_s), V, *shape, C]

    def refused(changes, text):
        args = list(ok)
        for i, a in changes.items():
            args[i] = a
        with pytest.raises(_lib.NfsError, match=text) as e:
            _lib.call("nfs_liquid_absorb_bwd", *args, None)
        assert e.value.code == _lib.NFS_EINVAL

    refused({0: None}, "null pointer")
    refused({8: None}, "null pointer")
    refused({9: 0}, "at least 1")
    refused({12: 0}, "at least 1")
    refused({13: 5}, "C must be 1..4")
    refused({9: 1, 10: 1024, 11: 1024, 12: 1024}, "below 2\\^30")
    for i in (0, 1, 2, 3, 5, 6):
        refused({8: ok[i]}, "g_s must not alias")
    refused({8: P(k["d"]) + 4}, "g_s must not alias")
    refused({8: P(k["w"]) + 16}, "g_s may be w itself")
    refused({8: P(k["w"]) - 16}, "g_s may be w itself|g_s must not alias")
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.liquid_absorb_bwd(k["g"], k["q"], k["d"].double(), views, k["w"], k["t"], k["bg"], TAU)
    with pytest.raises(ValueError, match="do not fit"):
        ops.liquid_absorb_bwd(k["g"][:1], k["q"], k["d"], views, k["w"], k["t"], k["bg"], TAU)

"""libnfs_exposure.so element by element: nfs_exposure_weights' w and grey and nfs_exposure_absorb_bwd's g_s against the float64
closed forms of tests/exposure_ref.py, each element within its own counted float32 bound.  Output buffers start as NaN.  Every
case takes three kinds of view matrix -- the identity, rotations by 10 degrees, and a non-orthogonal matrix (a shear scaled
by 1.4) that pushes samples past every border -- and the shapes (V, D, H, W) are the smallest that reach each path of the
kernels:
    (2, 7, 5, 1)    W == 1: the scalar corners (tri_setup); D no multiple of the unroll of 4
    (1, 3, 1, 2)    D below the unroll; W == 2, the narrowest pair load; one row
    (3, 9, 6, 11)   odd sizes, two unrolled groups and a tail
    (2, 4, 19, 23)  874 rays: more than one block of 256, the last one partial; D exactly one unrolled group
with C = 1..4 channels.  Besides: g_s written over w is the same bits; a volume with -0.0 samples; a NaN sample leaves every
other ray bit-identical; every refusal on device buffers.  Every check prints the largest err / bound it saw (pytest -s).
tau = 0.2, kappa = 1.5 (exact in float32)."""
import math

import numpy as np
import pytest
import torch

from tests import exposure_ref as ER
from tests import view_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAU = 0.2
TAU32 = float(np.float32(TAU))
KAPPA = 1.5
SHAPES = [(2, 7, 5, 1), (1, 3, 1, 2), (3, 9, 6, 11), (2, 4, 19, 23)]
KINDS = ["identity", "rot10", "sheared"]


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


def _ry(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rz(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def matrices(kind, V):
    """V views of one kind, each view its own matrix where the kind allows one"""
    if kind == "identity":
        m = [np.eye(3)] * V
    elif kind == "rot10":
        m = [(_ry(10), _rz(10), _ry(10) @ _rz(-10))[v % 3] for v in range(V)]
    else:
        shear = np.array([[1.0, 0.3, -0.2], [-0.25, 1.0, 0.35], [0.3, -0.2, 1.0]])
        m = [1.4 * (shear, shear.T, shear @ shear)[v % 3] for v in range(V)]
    return torch.tensor(np.asarray(m, np.float32), device=DEV)


def check(name, got, ref, bound):
    r = VR.err_ratio((got.double() - ref.double()).abs(), bound)
    print("%-64s max err/bound %.3g" % (name, r))
    assert r <= 1.0, (name, r)
    return r


def volume(shape3, seed=7):
    """densities up to 6 (tau S up to 1.2 per sample), an empty ray and a ray of -0.0 at the identity"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    d = (torch.rand(shape3, generator=gen, dtype=torch.float64) * 6.0).float()
    d[:, 0, 0] = 0.0
    if shape3[1] > 1:
        d[:, 1, 0] = -0.0
    return d.to(DEV)


def inputs(shape, C, seed=11):
    V, shape3 = shape[0], tuple(shape[1:])
    gen = torch.Generator(device="cpu").manual_seed(seed + C)
    q = torch.rand(shape3 + (C,), generator=gen, dtype=torch.float64).float().to(DEV)
    g = torch.randn((V,) + shape3[1:] + (C,), generator=gen, dtype=torch.float64).float()
    g[V - 1, 0, 0, :] = 0.0                                          # a ray of exact zeros
    return q, g.to(DEV)


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


_cache = {}


def weights_case(ops, shape, kind):
    """the volume, the views, the kernel's w and grey (into NaN buffers) and the reference's per-view samples: once"""
    key = (shape, kind)
    if key not in _cache:
        V, shape3 = shape[0], tuple(shape[1:])
        d, rot = volume(shape3), matrices(kind, V)
        w, grey = ops.exposure_weights(d, rot, TAU, KAPPA, w=nans(*shape), grey=nans(V, *shape3[1:]))
        sts = [VR.Stencil(rot[v], shape3) for v in range(V)]
        samples = [st.sample(d.double()) for st in sts]
        rays = [ER.ray(s, es, TAU32, KAPPA) for s, es in samples]
        _cache[key] = dict(d=d, rot=rot, w=w, grey=grey, sts=sts, samples=samples, rays=rays)
    return _cache[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exposure_weights(ops, shape, kind):
    k = weights_case(ops, shape, kind)
    V, shape3 = shape[0], tuple(shape[1:])
    assert tuple(k["w"].shape) == shape and tuple(k["grey"].shape) == (V,) + shape3[1:]
    assert bool(torch.isfinite(k["w"]).all()) and bool(torch.isfinite(k["grey"]).all())
    for v, r in enumerate(k["rays"]):
        check("exposure w %s %s v%d" % (shape, kind, v), k["w"][v], r["w"], r["e_w"])
        check("exposure grey %s %s v%d" % (shape, kind, v), k["grey"][v], r["grey"], r["e_grey"])
        # grey <= kappa (1 - t), up to the bound
        assert bool((k["grey"][v].double() <= KAPPA * (1 - r["t"]) + r["e_grey"]).all())
    ceil = np.float32(np.float32(KAPPA) * np.float32(TAU))
    assert float(k["w"].max()) <= float(ceil) and float(k["w"].min()) > 0.0
    if kind == "identity":
        # the empty ray and the ray of -0.0: w = kappa tau exactly, grey = +0
        assert bool((k["w"][:, :, 0, 0] == float(ceil)).all()) and bool((k["grey"][:, 0, 0] == 0).all())
        if shape3[1] > 1:
            assert bool((k["w"][:, :, 1, 0] == float(ceil)).all())
            assert not bool(torch.signbit(k["grey"][:, 1, 0]).any())
    if kind == "sheared":
        # the matrix really pushes samples past every border of every axis it can
        x, _ = VR.coords(k["rot"][0], shape3)
        for ax, n in enumerate(shape3):
            if n > 1:
                assert float(x[..., ax].min()) < 0 and float(x[..., ax].max()) > n - 1, (ax, n)
    # grey may be null
    w2, _ = ops.exposure_weights(k["d"], k["rot"], TAU, KAPPA)
    from neural_flow_style_amd import _lib
    w3 = nans(*shape)
    _lib.call("nfs_exposure_weights", k["d"].data_ptr(), k["rot"].data_ptr(), TAU, KAPPA, w3.data_ptr(), None, *shape, None)
    torch.cuda.synchronize()
    assert torch.equal(w2, k["w"]) and torch.equal(w3, k["w"])


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exposure_absorb_bwd(ops, shape, kind, C):
    k = weights_case(ops, shape, kind)
    V, shape3 = shape[0], tuple(shape[1:])
    q, g = inputs(shape, C)
    g_s = ops.exposure_absorb_bwd(g, q, k["rot"], k["w"], TAU, out=nans(*shape))
    assert tuple(g_s.shape) == shape and bool(torch.isfinite(g_s).all())
    for v in range(V):
        QS = [k["sts"][v].sample(q[..., c].double()) for c in range(C)]
        r = k["rays"][v]
        ab = ER.absorb(r["w"], r["e_w"], torch.stack([x[0] for x in QS], -1), torch.stack([x[1] for x in QS], -1),
                       g[v].double(), TAU32)
        check("exposure g_s %s %s C%d v%d" % (shape, kind, C, v), g_s[v], ab["g_s"], ab["e_g_s"])
    assert bool((g_s[V - 1, :, 0, 0] == 0).all())                    # the ray of zero gradient: exact zeros
    assert float(g_s.abs().max()) > 1e-3
    # written over the weights it is the same bits
    w2 = k["w"].clone()
    out = ops.exposure_absorb_bwd(g, q, k["rot"], w2, TAU, out=w2)
    assert out.data_ptr() == w2.data_ptr()
    assert torch.equal(w2, g_s) and not torch.equal(w2, k["w"])


def test_a_volume_with_negative_zero_samples(ops):
    """every second voxel -0.0: the results are those of the volume with +0.0 in their place, bit for bit, and finite"""
    shape = (3, 9, 6, 11)
    shape3 = shape[1:]
    d = volume(shape3)
    mask = (torch.arange(d.numel(), device=DEV).reshape(shape3) % 2) == 0
    plus = torch.where(mask, torch.zeros_like(d), d)
    minus = torch.where(mask, -torch.zeros_like(d), d)
    assert bool(torch.signbit(minus[mask]).all()) and not bool(torch.signbit(plus[mask]).any())
    q, g = inputs(shape, 3)
    for kind in KINDS:
        rot = matrices(kind, shape[0])
        wp, gp = ops.exposure_weights(plus, rot, TAU, KAPPA)
        wm, gm = ops.exposure_weights(minus, rot, TAU, KAPPA)
        assert torch.equal(wp, wm) and torch.equal(gp, gm) and bool(torch.isfinite(wm).all())
        assert not bool(torch.signbit(gm).any())
        assert torch.equal(ops.exposure_absorb_bwd(g, q, rot, wp, TAU), ops.exposure_absorb_bwd(g, q, rot, wm, TAU))
    # a volume of -0.0 alone: w = kappa tau, grey = +0
    w0, g0 = ops.exposure_weights(-torch.zeros(shape3, device=DEV), matrices("rot10", shape[0]), TAU, KAPPA)
    assert bool((w0 == float(np.float32(np.float32(KAPPA) * np.float32(TAU)))).all())
    assert bool((g0 == 0).all()) and not bool(torch.signbit(g0).any())


def test_a_nan_sample_poisons_its_own_ray_only(ops):
    """a NaN voxel of d (then of q) reaches the rays whose stencil holds it (at the identity: its own column, and
    neighbours only through a corner of weight zero); every other ray is what it was, bit for bit"""
    shape = (1, 9, 6, 11)
    shape3 = shape[1:]
    d, eye = volume(shape3), matrices("identity", 1)
    q, g = inputs(shape, 3)
    w, grey = ops.exposure_weights(d, eye, TAU, KAPPA)
    good = ops.exposure_absorb_bwd(g, q, eye, w, TAU)
    z0, y0, x0 = 5, 3, 4
    far = torch.ones(shape3[1:], dtype=torch.bool, device=DEV)
    far[y0 - 1:y0 + 2, x0 - 1:x0 + 2] = False
    bad = d.clone()
    bad[z0, y0, x0] = float("nan")
    w2, grey2 = ops.exposure_weights(bad, eye, TAU, KAPPA)
    assert torch.equal(w2[0][:, far], w[0][:, far]) and torch.equal(grey2[0][far], grey[0][far])
    assert bool(torch.isnan(w2[0, :z0 + 1, y0, x0]).all()) and bool(torch.isnan(grey2[0, y0, x0]))
    # behind the sample the ray is what it was (sample z0 + 1 may hold the voxel through a corner of weight zero)
    assert torch.equal(w2[0, z0 + 2:, y0, x0], w[0, z0 + 2:, y0, x0])
    assert int(torch.isnan(w2[0]).any(0).sum()) <= 9
    got = ops.exposure_absorb_bwd(g, q, eye, w2, TAU)
    assert torch.equal(got[0][:, far], good[0][:, far]) and bool(torch.isnan(got[0, :, y0, x0]).all())
    qbad = q.clone()
    qbad[z0, y0, x0, 1] = float("nan")
    got = ops.exposure_absorb_bwd(g, qbad, eye, w, TAU)
    assert torch.equal(got[0][:, far], good[0][:, far])
    assert bool(torch.isnan(got[0, z0:, y0, x0]).all()) and torch.equal(got[0, :z0 - 1, y0, x0], good[0, :z0 - 1, y0, x0])
    assert int(torch.isnan(got[0]).any(0).sum()) <= 9


def test_refusals_on_device_buffers(ops):
    from neural_flow_style_amd import _lib
    shape, C = (3, 9, 6, 11), 3
    k = weights_case(ops, shape, "rot10")
    V = shape[0]
    q, g = inputs(shape, C)
    w, grey, g_s = nans(*shape), nans(V, *shape[2:]), nans(*shape)
    P = lambda x: x.data_ptr()
    nan, inf = float("nan"), float("inf")

    def refused(name, ok, changes, text):
        args = list(ok)
        for i, a in changes.items():
            args[i] = a
        with pytest.raises(_lib.NfsError, match=text) as e:
            _lib.call(name, *args, None)
        assert e.value.code == _lib.NFS_EINVAL
        assert _lib.lib().nfs_last_error().decode().startswith(name + ":")

    name, ok = "nfs_exposure_weights", [P(k["d"]), P(k["rot"]), TAU, KAPPA, P(w), P(grey), *shape]
    for i in (0, 1, 4):
        refused(name, ok, {i: None}, "null pointer")
    for i in (6, 7, 8, 9):
        refused(name, ok, {i: 0}, "at least 1")
    refused(name, ok, {6: 1, 7: 1024, 8: 1024, 9: 1024}, "below 2\\^30")
    for bad in (0.0, -TAU, nan, inf):
        refused(name, ok, {2: bad}, "tau must be finite and positive")
        refused(name, ok, {3: bad}, "gain must be finite and positive")
    refused(name, ok, {4: P(k["d"])}, "w must not alias")
    refused(name, ok, {4: P(k["rot"])}, "w must not alias")
    refused(name, ok, {5: P(k["d"]) + 4}, "grey must not alias")
    refused(name, ok, {5: P(w) + 16}, "grey must not alias")
    torch.cuda.synchronize()
    assert bool(torch.isnan(w).all()) and bool(torch.isnan(grey).all())      # nothing was launched

    name, ok = "nfs_exposure_absorb_bwd", [P(g), P(q), P(k["rot"]), P(k["w"]), TAU, P(g_s), *shape, C]
    for i in (0, 1, 2, 3, 5):
        refused(name, ok, {i: None}, "null pointer")
    for i in (6, 7, 8, 9):
        refused(name, ok, {i: 0}, "at least 1")
    for bad in (0, 5):
        refused(name, ok, {10: bad}, "C must be 1..4")
    refused(name, ok, {6: 1, 7: 1024, 8: 1024, 9: 1024}, "below 2\\^30")
    for bad in (0.0, -TAU, nan, inf):
        refused(name, ok, {4: bad}, "tau must be finite and positive")
    for i in (0, 1, 2):
        refused(name, ok, {5: ok[i]}, "g_s must not alias")
    refused(name, ok, {5: P(q) + 4}, "g_s must not alias")
    refused(name, ok, {5: P(k["w"]) + 16}, "g_s may be w itself")
    refused(name, ok, {5: P(k["w"]) - 16}, "g_s may be w itself|g_s must not alias")
    torch.cuda.synchronize()
    assert bool(torch.isnan(g_s).all())
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.exposure_weights(k["d"].double(), k["rot"], TAU, KAPPA)
    with pytest.raises(ValueError, match="do not fit"):
        ops.exposure_absorb_bwd(g[:1], q, k["rot"], k["w"], TAU)

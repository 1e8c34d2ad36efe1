"""libnfs_liquid.so element by element: nfs_liquid_weights' w, t_total and grey against the float64 restatement of
tests/colour_liquid_ref.py, each element within its own float32 error bound, on every shape of tests/colour_ref.py and its
four views; the partition of unity; the projection with these weights against the grey liquid render; every route of the
projection's transpose with these weights; 0 <= w <= tau; volumes one cell wide (the kernel's scalar stencil); buffers that
touch end to end (no false refusal); a NaN sample; the refusals on device buffers.  Every check prints
the largest err / bound it saw (pytest -s).

The volumes carry, as columns along D (the rays of the identity view): an empty ray, a ray of -0.0, samples with
tau S = 1e-7, samples on both sides of phi's change of form at tau S = 2^-5, and a ray whose sum takes t below the smallest
normal float32.  tau = 0.2, the chocolate driver's."""
import math

import numpy as np
import pytest
import torch

from tests import colour_liquid_ref as LR
from tests import colour_ref as CR
from tests import view_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAU = 0.2
TAU32 = float(np.float32(TAU))                       # the value the kernels receive


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


def volume(shape, seed=1):
    D = shape[0]
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = (torch.rand(shape, generator=g, dtype=torch.float64) * 6.0).float()
    d[:, 0, 0] = 0.0                                              # an empty ray: w = tau all the way, t = 1
    d[:, 0, 1] = -0.0                                             # the mark of smooth3d_relu's cut voxels: counts as 0
    d[:, 1, 0] = 1e-7 / TAU                                       # tau S = 1e-7: phi must not lose its relative accuracy
    step = 2.0 ** -5 / TAU
    d[0::2, 1, 1] = step * (1 - 2.0 ** -10)                       # ... and both sides of phi's change of form
    d[1::2, 1, 1] = step * (1 + 2.0 ** -10)
    d[:, 2, 0] = 94.5 / (TAU * D)                                 # t = exp(-94.5) = 9e-42, below the smallest normal
    return d.to(DEV)


_refs = {}


def reference(views, shape):
    """per view: (stencil, samples, their bound, LR.ray of them), computed once per shape and left alone"""
    if shape not in _refs:
        d = volume(shape)
        out = []
        for v in range(views.shape[0]):
            st = VR.Stencil(views[v], shape)
            s, es = st.sample(d.double())
            out.append((st, s, es, LR.ray(s, es, TAU32)))
        _refs[shape] = (d, out)
    return _refs[shape]


_got = {}


def kernel(ops, views, shape):
    if shape not in _got:
        d, _ = reference(views, shape)
        _got[shape] = ops.liquid_weights(d, views, TAU)
    return _got[shape]


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_liquid_weights(ops, views, shape):
    d, refs = reference(views, shape)
    w, grey, t = kernel(ops, views, shape)
    V = views.shape[0]
    assert tuple(w.shape) == (V,) + shape and tuple(grey.shape) == tuple(t.shape) == (V,) + shape[1:]
    for v, (st, s, es, r) in enumerate(refs):
        check("liquid w %s v%d" % (shape, v), w[v], r["w"], r["e_w"])
        check("liquid t_total %s v%d" % (shape, v), t[v], r["t"], r["e_t"])
        check("liquid grey %s v%d" % (shape, v), grey[v], r["grey"], r["e_grey"])
        # the partition of unity, the kernel's weights on the reference's samples, within the summed bounds
        one = (w[v].double() * s).sum(0) + t[v].double()
        check("partition of unity %s v%d" % (shape, v), one, torch.ones_like(one), (r["e_w"] * s.abs()).sum(0) + r["e_t"])
    assert bool((w >= 0).all()) and float(w.max()) <= TAU32
    # the special rays, at the identity
    assert bool((w[0, :, 0, 0] == TAU32).all()) and float(t[0, 0, 0]) == 1.0 and float(grey[0, 0, 0]) == 0.0
    assert float(t[0, 0, 1]) >= 1.0 - 1e-5            # (the ray of -0.0; its neighbours may enter with a rounding's weight)
    assert 0.0 <= float(t[0, 2, 0]) < 2.0 ** -126 and float(grey[0, 2, 0]) == 1.0
    assert float(grey.min()) < 0.1 and float(grey.max()) > 0.5


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_a_volume_of_negative_zeros_is_empty(ops, views, shape):
    """-0.0 everywhere (a frame that nfs_smooth3d_relu_fwd cut entirely): every weight is tau, every ray transparent"""
    d = torch.full(shape, -0.0, device=DEV)
    assert bool(torch.signbit(d).all())
    w, grey, t = ops.liquid_weights(d, views, TAU)
    assert bool((w == TAU32).all()) and bool((t == 1).all()) and bool((grey == 0).all())


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_null_images_and_given_buffers(ops, views, shape):
    """grey and t_total are each nullable, and the weights do not depend on it; buffers passed in are the ones written"""
    from neural_flow_style_amd import _lib
    d, _ = reference(views, shape)
    w, grey, t = kernel(ops, views, shape)
    V = views.shape[0]
    for want_grey, want_t in ((False, False), (True, False), (False, True)):
        w2 = torch.full_like(w, -1.0)
        g2, t2 = torch.full_like(grey, -1.0), torch.full_like(t, -1.0)
        _lib.call("nfs_liquid_weights", d.data_ptr(), views.data_ptr(), TAU, w2.data_ptr(),
                  g2.data_ptr() if want_grey else None, t2.data_ptr() if want_t else None, V, *shape, None)
        torch.cuda.synchronize()
        assert torch.equal(w2, w)
        assert torch.equal(g2, grey) if want_grey else bool((g2 == -1).all())
        assert torch.equal(t2, t) if want_t else bool((t2 == -1).all())
    bw, bg, bt = torch.empty_like(w), torch.empty_like(grey), torch.empty_like(t)
    out = ops.liquid_weights(d, views, TAU, w=bw, grey=bg, t_total=bt)
    assert [o.data_ptr() for o in out] == [bw.data_ptr(), bg.data_ptr(), bt.data_ptr()]
    assert torch.equal(bw, w) and torch.equal(bg, grey) and torch.equal(bt, t)


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_projection_of_the_grey_volume_is_the_liquid_render(ops, views, shape):
    """C = 1, q = d, no background: colour_project_fwd with the liquid weights and rotate_render_fwd(liquid=True) render
    the same image 1 - t, each within its own bound of the same reference"""
    d, refs = reference(views, shape)
    w, grey, t = kernel(ops, views, shape)
    img = ops.colour_project_fwd(d.unsqueeze(-1).contiguous(), views, w)
    rr, _ = ops.rotate_render_fwd(d, views, TAU, True)
    for v, (st, s, es, r) in enumerate(refs):
        J, eJ = CR.project(st, d.double().unsqueeze(-1), r["w"], r["e_w"])
        assert float((J[..., 0] - r["grey"]).abs().max()) <= 1e-12              # the identity, in float64
        check("project(q = d, liquid w) %s v%d" % (shape, v), img[v], J, eJ)
        vr = VR.ray(s, es, TAU32)
        check("rotate_render_fwd(liquid) %s v%d" % (shape, v), rr[v], vr["liquid"], vr["e_liquid"])
        check("liquid grey against it %s v%d" % (shape, v), grey[v], rr[v], r["e_grey"] + vr["e_liquid"])


def _routes(ops, V, shape):
    r = ["atomic", "tiled"]
    if ops.render_coef_layout(V, *shape) is not None:
        r.append("coef")
    return r


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_every_transpose_route_with_liquid_weights(ops, views, shape):
    """ops.colour_project_bwd on the kernel's own weights (non-negative, at most tau: the 'coef' route's bound
    max |g| max w holds) against CR.transpose of the same numbers"""
    V, C = views.shape[0], 3
    w, _, _ = kernel(ops, views, shape)
    gen = torch.Generator(device="cpu").manual_seed(6)
    g = torch.randn((V,) + shape[1:] + (C,), generator=gen, dtype=torch.float64).float().to(DEV)
    g[1, 0, 0, :] = 0.0
    scs = CR.transpose(views, g.double(), w.double())
    routes = _routes(ops, V, shape)
    assert ("coef" in routes) == (shape[0] >= 16)
    for route in routes + [None]:
        got = ops.colour_project_bwd(g, views, w, route=route)
        kind = route or ops.colour_bwd_route(V, *shape)
        for c in range(C):
            if kind == "atomic":
                bound = VR.adjoint_bound(scs[c], True)
            else:
                gmax = float((w * g[..., c].unsqueeze(1)).abs().max()) if kind == "tiled" \
                    else float(g[..., c].abs().max() * w.max())
                assert kind != "coef" or gmax >= float((w * g[..., c].unsqueeze(1)).abs().max())
                bound = VR.adjoint_bound(scs[c], False, VR.fixed_point_quantum(gmax, views, shape))
            check("transpose, liquid w %s c%d %s" % (shape, c, route or "default"), got[..., c], scs[c]["ref"], bound)


@pytest.mark.parametrize("shape", [(5, 4, 1), (6, 1, 1), (1, 3, 1)], ids=str)
def test_a_volume_one_cell_wide(ops, views, shape):
    """W == 1: there is no x-pair to load, so the kernel takes the scalar stencil (tri_setup); the same bounds, all views"""
    g = torch.Generator(device="cpu").manual_seed(5)
    d = (torch.rand(shape, generator=g, dtype=torch.float64) * 6.0).float()
    empty = shape[1] > 1
    if empty:
        d[:, 0, 0] = 0.0                                          # an empty ray beside the others
    d = d.to(DEV)
    w, grey, t = ops.liquid_weights(d, views, TAU)
    V = views.shape[0]
    assert tuple(w.shape) == (V,) + shape and tuple(grey.shape) == tuple(t.shape) == (V,) + shape[1:]
    for v in range(V):
        s, es = VR.Stencil(views[v], shape).sample(d.double())
        r = LR.ray(s, es, TAU32)
        check("liquid w %s v%d" % (shape, v), w[v], r["w"], r["e_w"])
        check("liquid t_total %s v%d" % (shape, v), t[v], r["t"], r["e_t"])
        check("liquid grey %s v%d" % (shape, v), grey[v], r["grey"], r["e_grey"])
        one = (w[v].double() * s).sum(0) + t[v].double()
        check("partition of unity %s v%d" % (shape, v), one, torch.ones_like(one), (r["e_w"] * s.abs()).sum(0) + r["e_t"])
    assert bool((w >= 0).all()) and float(w.max()) <= TAU32
    assert float(grey.max()) > 0.3
    if empty:
        assert bool((w[0, :, 0, 0] == TAU32).all()) and float(t[0, 0, 0]) == 1.0


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_buffers_that_touch_end_to_end_are_no_overlap(ops, views, shape):
    """d, rot, w, grey and t_total carved end to end out of ONE allocation, each beginning at the float after the last of
    the one before: none overlaps another, so the call goes through (no false refusal) and writes what it writes into
    separate allocations, bit for bit, leaving d and rot as they were"""
    from neural_flow_style_amd import _lib
    d, _ = reference(views, shape)
    w, grey, t = kernel(ops, views, shape)
    V = views.shape[0]
    sizes = [d.numel(), views.numel(), w.numel(), grey.numel(), t.numel()]
    block = torch.full((sum(sizes),), -1.0, device=DEV)
    pd, pr, pw, pg, pt = torch.split(block, sizes)
    pd.copy_(d.reshape(-1)); pr.copy_(views.reshape(-1))
    assert pr.data_ptr() == pd.data_ptr() + 4 * sizes[0] and pg.data_ptr() == pw.data_ptr() + 4 * sizes[2]
    _lib.call("nfs_liquid_weights", pd.data_ptr(), pr.data_ptr(), TAU, pw.data_ptr(), pg.data_ptr(), pt.data_ptr(), V, *shape,
              None)
    torch.cuda.synchronize()
    assert torch.equal(pd, d.reshape(-1)) and torch.equal(pr, views.reshape(-1))
    assert torch.equal(pw, w.reshape(-1)) and torch.equal(pg, grey.reshape(-1)) and torch.equal(pt, t.reshape(-1))


def test_a_nan_sample_poisons_its_own_ray_only(ops, views):
    """a NaN voxel reaches the rays whose stencil holds it (at the identity: its own column, and neighbours only through a
    corner of weight zero); every other ray is what it was, bit for bit; on its own ray the weights behind it stay finite"""
    shape = (17, 6, 9)
    d, _ = reference(views, shape)
    w, grey, t = kernel(ops, views, shape)
    bad = d.clone()
    z0, y0, x0 = 9, 3, 4
    bad[z0, y0, x0] = float("nan")
    eye = views[:1].contiguous()
    w2, g2, t2 = ops.liquid_weights(bad, eye, TAU)
    far = torch.ones(shape[1:], dtype=torch.bool, device=DEV)
    far[y0 - 1:y0 + 2, x0 - 1:x0 + 2] = False
    assert torch.equal(w2[0][:, far], w[0][:, far]) and torch.equal(t2[0][far], t[0][far]) and torch.equal(g2[0][far], grey[0][far])
    assert bool(torch.isnan(w2[0, :z0, y0, x0]).all()) and math.isnan(float(t2[0, y0, x0])) and math.isnan(float(g2[0, y0, x0]))
    assert bool(torch.isfinite(w2[0, z0 + 2:, y0, x0]).all()) and torch.equal(w2[0, z0 + 2:, y0, x0], w[0, z0 + 2:, y0, x0])
    assert int(torch.isnan(t2).sum()) <= 9


def test_refusals_on_device_buffers(ops, views):
    from neural_flow_style_amd import _lib
    shape = (3, 4, 5)
    V = views.shape[0]
    d, _ = reference(views, shape)
    w = torch.empty((V,) + shape, device=DEV)
    grey, t = torch.empty((V,) + shape[1:], device=DEV), torch.empty((V,) + shape[1:], device=DEV)
    P = lambda x: x.data_ptr()

    def refused(args, text):
        with pytest.raises(_lib.NfsError, match=text) as e:
            _lib.call("nfs_liquid_weights", *args, None)
        assert e.value.code == _lib.NFS_EINVAL

    refused([None, P(views), TAU, P(w), P(grey), P(t), V, *shape], "null pointer")
    refused([P(d), P(views), TAU, None, P(grey), P(t), V, *shape], "null pointer")
    refused([P(d), P(views), TAU, P(w), P(grey), P(t), 0, *shape], "at least 1")
    refused([P(d), P(views), TAU, P(w), P(grey), P(t), V, 3, 4, 0], "at least 1")
    refused([P(d), P(views), TAU, P(w), P(grey), P(t), 1, 1024, 1024, 1024], "below 2\\^30")
    refused([P(d), P(views), TAU, P(d), P(grey), P(t), V, *shape], "w must not alias d or rot")
    refused([P(d), P(views), TAU, P(w), P(views), P(t), V, *shape], "grey must not alias d or rot")
    refused([P(d), P(views), TAU, P(w), P(grey), P(d) + 4, V, *shape], "t_total must not alias d or rot")
    refused([P(d), P(views), TAU, P(w), P(grey), P(grey), V, *shape], "must not alias one another")
    refused([P(d), P(views), TAU, P(w), P(w) + 16, P(t), V, *shape], "must not alias one another")
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.liquid_weights(d.double(), views, TAU)

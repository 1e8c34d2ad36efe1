"""libnfs_colour.so element by element: the ray weights, the colour projection and its transpose (every route
ops.colour_project_bwd can take) against the float64 restatement of tests/colour_ref.py, each element within its own
float32 error bound.  Every check prints the largest err / bound it saw (pytest -s), as tests/test_view_path_gpu.py does.

Volumes: (3,4,5) lies below the coefficient layout's D >= 16, (17,6,9) enters it, a W row of (16,5,70) spans two waves.
Views: identity, two rotations and 1.4 I, whose border samples are all clamped."""
import pytest
import torch

from tests import colour_ref as CR
from tests import view_ref as VR

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAU = 0.3


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


def check(name, got, ref, bound):
    r = VR.err_ratio((got.double() - ref.double()).abs(), bound)
    print("%-56s max err/bound %.3g" % (name, r))
    assert r <= 1.0, (name, r)


def rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float().to(DEV)


def randn(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).float().to(DEV)


@pytest.fixture(scope="module")
def views():
    return CR.views(DEV)


_stencils = {}


def stencils(R, shape):
    if shape not in _stencils:
        _stencils[shape] = [VR.Stencil(R[v], shape) for v in range(R.shape[0])]
    return _stencils[shape]


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
@pytest.mark.parametrize("groups", ["G=1", "G=V"])
def test_ray_weights(ops, views, shape, groups):
    V = views.shape[0]
    G = 1 if groups == "G=1" else V
    d_rot = rand((V,) + shape, 1, 0.0, 1.0)
    d_rot[0, :, 0, 0] = 0.0                                         # an empty ray: w = 1 / M all the way
    gmax = rand((G,), 2, 0.5, 3.0)
    w = ops.ray_weights(d_rot, TAU, gmax)
    for v in range(V):
        ref, e = CR.ray_weights(d_rot[v].double(), torch.zeros_like(d_rot[v], dtype=torch.float64), TAU,
                                float(gmax[v // (V // G)]))
        check("ray_weights %s %s v%d" % (shape, groups, v), w[v], ref, e)
    # in place: the weights over the samples they came from, the same bits
    buf = d_rot.clone()
    out = ops.ray_weights(buf, TAU, gmax, out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf, w)


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_colour_project_fwd(ops, views, shape, C):
    V = views.shape[0]
    q = rand(shape + (C,), 3, -1.0, 1.0)
    w = rand((V,) + shape, 4, 0.0, 2.0)
    img = ops.colour_project_fwd(q, views, w)
    assert tuple(img.shape) == (V,) + shape[1:] + (C,)
    for v, st in enumerate(stencils(views, shape)):
        ref, e = CR.project(st, q.double(), w[v].double(), torch.zeros_like(w[v], dtype=torch.float64))
        check("colour_project_fwd %s C=%d v%d" % (shape, C, v), img[v], ref, e)


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
def test_forward_agrees_with_rotate_fwd_summed(ops, views, shape):
    """C = 1, w = 1: the projection is rotate_fwd summed along the ray, each within its own bound of the same reference"""
    V = views.shape[0]
    q = rand(shape + (1,), 5, -1.0, 1.0)
    ones = torch.ones((V,) + shape, dtype=torch.float32, device=DEV)
    img = ops.colour_project_fwd(q, views, ones)
    summed = ops.rotate_fwd(q, views).double().sum(1)
    for v, st in enumerate(stencils(views, shape)):
        ref, e = CR.project(st, q.double(), ones[v].double(), torch.zeros_like(ones[v], dtype=torch.float64))
        check("project vs reference %s v%d" % (shape, v), img[v], ref, e)
        check("rotate_fwd summed vs reference %s v%d" % (shape, v), summed[v], ref, e)
        check("project vs rotate_fwd summed %s v%d" % (shape, v), img[v], summed[v], 2 * e)


def _routes(ops, V, shape):
    r = ["atomic", "tiled"]
    if ops.render_coef_layout(V, *shape) is not None:
        r.append("coef")
    return r


@pytest.mark.parametrize("shape", CR.SHAPES, ids=str)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_colour_project_bwd(ops, views, shape, C):
    """the transpose, overwriting and accumulating into a non-zero g_q, on every route (and the default one)"""
    V = views.shape[0]
    g = randn((V,) + shape[1:] + (C,), 6)
    g[1, 0, 0, :] = 0.0                                            # a ray without a gradient
    w = rand((V,) + shape, 7, 0.0, 2.0)
    init = rand(shape + (C,), 8, -2.0, 2.0)
    scs = CR.transpose(views, g.double(), w.double())
    routes = _routes(ops, V, shape)
    assert ("coef" in routes) == (shape[0] >= 16)
    assert ops.colour_bwd_route(V, *shape) in routes
    for route in routes + [None]:
        got = ops.colour_project_bwd(g, views, w, route=route)
        acc = init.clone()
        ret = ops.colour_project_bwd(g, views, w, g_q=acc, route=route)
        assert ret.data_ptr() == acc.data_ptr() and tuple(got.shape) == shape + (C,)
        kind = route or ops.colour_bwd_route(V, *shape)
        for c in range(C):
            if kind == "atomic":
                b0 = VR.adjoint_bound(scs[c], True)
                b1 = VR.adjoint_bound(scs[c], True, init=init[..., c].double())
            else:
                # the fixed-point scale: the largest materialised product ('tiled': the pre-pass over it), or the
                # bound the coefficient form is handed, max |g| max w in float32
                if kind == "tiled":
                    gmax = float((w * g[..., c].unsqueeze(1)).abs().max())
                else:
                    gmax = float(g[..., c].abs().max() * w.max())
                quantum = VR.fixed_point_quantum(gmax, views, shape)
                b0 = VR.adjoint_bound(scs[c], False, quantum)
                # (the sum lands in a fresh buffer and is added to g_q: one more rounding of the total)
                b1 = VR.adjoint_bound(scs[c], False, quantum, init=init[..., c].double()) \
                    + VR.EPS * (scs[c]["ref"] + init[..., c].double()).abs()
            tag = "%s C=%d c%d %s" % (shape, C, c, route or "default")
            check("colour_project_bwd " + tag, got[..., c], scs[c]["ref"], b0)
            check("colour_project_bwd += " + tag, acc[..., c], scs[c]["ref"] + init[..., c].double(), b1)


def test_transpose_identity_on_the_kernels(ops, views):
    """<A q, g> = <q, A^T g> with both sides from the kernels, to the float32 accumulation of the two inner products"""
    shape = (17, 6, 9)
    V = views.shape[0]
    q = rand(shape + (3,), 9, 0.0, 1.0)
    w = rand((V,) + shape, 10, 0.0, 1.0)
    g = randn((V,) + shape[1:] + (3,), 11)
    lhs = float((ops.colour_project_fwd(q, views, w).double() * g.double()).sum())
    rhs = float((q.double() * ops.colour_project_bwd(g, views, w).double()).sum())
    scale = float((ops.colour_project_fwd(q, views, w).double().abs() * g.double().abs()).sum())
    print("transpose identity: lhs %.9g rhs %.9g rel %.3g" % (lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 64 * VR.EPS * scale


def test_refusals_on_device_buffers(ops, views):
    from neural_flow_style_amd import _lib
    shape = (3, 4, 5)
    V = views.shape[0]
    w = rand((V,) + shape, 12)
    q = rand(shape + (3,), 13)
    gmax = rand((1,), 14, 0.5, 1.0)
    img = torch.empty((V,) + shape[1:] + (3,), device=DEV)
    P = lambda t: t.data_ptr()

    def refused(name, args, text):
        with pytest.raises(_lib.NfsError, match=text) as e:
            _lib.call(name, *args, None)
        assert e.value.code == _lib.NFS_EINVAL

    refused("nfs_ray_weights", [P(w), TAU, P(gmax), 3, P(w), V, *shape], "G must divide V")
    refused("nfs_ray_weights", [P(w), TAU, P(gmax), 1, P(gmax), V, *shape], "must not alias")
    refused("nfs_ray_weights", [P(w), TAU, P(gmax), 1, P(w), 1, 1024, 1024, 1024], "below 2\\^30")
    refused("nfs_colour_project_fwd", [P(q), P(views), P(w), P(img), V, *shape, 5], "C must be 1..4")
    refused("nfs_colour_project_fwd", [P(q), P(views), P(w), P(q), V, *shape, 3], "must not alias")
    refused("nfs_colour_project_fwd", [P(q), P(views), P(w), P(img), 0, *shape, 3], "at least 1")
    refused("nfs_colour_project_bwd", [P(img), P(views), P(w), P(img), 1, V, *shape, 3], "must not alias")
    refused("nfs_colour_project_bwd", [P(img), P(views), P(w), None, 1, V, *shape, 3], "null pointer")
    with pytest.raises(ValueError, match="coef"):
        ops.colour_project_bwd(img, views, w, route="coef")               # D = 3: no coefficient layout
    with pytest.raises(ValueError, match="route"):
        ops.colour_project_bwd(img, views, w, route="nope")


def test_default_route_by_size(ops):
    assert ops.colour_bwd_route(3, 17, 12, 12) == "atomic"                  # launch-bound
    assert ops.colour_bwd_route(8, 16, 64, 64) == "atomic"                  # 2^19 samples: the last size it won at
    assert ops.colour_bwd_route(8, 16, 64, 65) == "tiled"
    assert ops.colour_bwd_route(8, 32, 100, 100) == "tiled"
    assert ops.colour_bwd_route(8, 200, 200, 200) == "coef" and ops.colour_bwd_route(9, 200, 300, 200) == "coef"
    assert ops.colour_bwd_route(8, 12, 512, 512) == "tiled"                 # 2.5e7 samples, no coefficient layout (D < 16)
    assert ops.colour_bwd_route(8, 16, 64, 96) == "tiled" and ops.colour_bwd_route(8, 64, 128, 128) == "coef"
    assert ops.colour_bwd_route(1, 16, 512, 1023) == "tiled" and ops.colour_bwd_route(1, 16, 512, 1024) == "coef"


@pytest.mark.parametrize("shape,kind", [((16, 64, 130), "tiled"), ((12, 80, 140), "tiled"), ((16, 64, 130), "coef")], ids=str)
def test_default_route_above_the_threshold(ops, views, monkeypatch, shape, kind):
    """the default route just past the size at which it leaves the scatter kernel, with and without a coefficient layout;
    and into the coefficient form (its own threshold, 2^23 samples, lowered for the test: the route itself is held to the
    reference at every shape above)"""
    V, C = views.shape[0], 3
    if kind == "coef":
        monkeypatch.setattr(ops, "COLOUR_COEF_FROM", 0)
    assert V * shape[0] * shape[1] * shape[2] > ops.COLOUR_ATOMIC_UPTO and ops.colour_bwd_route(V, *shape) == kind
    g = randn((V,) + shape[1:] + (C,), 15)
    w = rand((V,) + shape, 16, 0.0, 2.0)
    got = ops.colour_project_bwd(g, views, w)
    scs = CR.transpose(views, g.double(), w.double())
    for c in range(C):
        gmax = float((w * g[..., c].unsqueeze(1)).abs().max()) if kind == "tiled" else float(g[..., c].abs().max() * w.max())
        bound = VR.adjoint_bound(scs[c], False, VR.fixed_point_quantum(gmax, views, shape))
        check("colour_project_bwd default (%s) %s c%d" % (kind, shape, c), got[..., c], scs[c]["ref"], bound)

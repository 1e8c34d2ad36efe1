"""libnfs_carrier.so on the GPU (include/nfs_carrier.h): nfs_carrier_displace bit for bit against nfs_g2p_fwd, and
nfs_carrier_bwd -- both routes of every case -- cell by cell against the float64 transpose of tests/carrier_ref.py, each
(cell, channel) within its own bound.  Every test prints the largest err / bound it saw (pytest -s)."""
import itertools

import numpy as np
import pytest
import torch

from tests import carrier_ref as CREF
from tests import splat_ref as SR
from tests.test_splat_gpu import DEV, G2P_DIMS, Report

pytestmark = pytest.mark.gpu

LARGE = {2: (48, 56), 3: (40, 40, 40)}
NS = [1, 255, 256, 257, 1500]


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


@pytest.fixture(scope="module")
def fixed_point():
    return CREF.header_constants()


def _dims(nd):
    return list(G2P_DIMS[nd]) + [LARGE[nd]]


def _uniform(rng, N, dims):
    """uniform(-0.3, 1.3) without the particles whose floor is a rounding decision (at most 1 % of them)"""
    p = torch.tensor(rng.uniform(-0.3, 1.3, (N, len(dims))).astype(np.float32), device=DEV)
    tie = SR.g2p_near_tie(p, dims)
    assert float(tie.double().mean()) <= 0.01 or N < 100, float(tie.double().mean())
    return p[~tie].contiguous() if N >= 100 else _redraw(rng, p, tie, dims)


def _redraw(rng, p, tie, dims):
    """the sets whose COUNT is the point (N = 1): a tie is drawn again instead of dropped"""
    for _ in range(50):
        if not bool(tie.any()):
            return p
        p[tie] = torch.tensor(rng.uniform(-0.3, 1.3, (int(tie.sum()), len(dims))).astype(np.float32), device=DEV)
        tie = SR.g2p_near_tie(p, dims)
    raise AssertionError("no tie-free set")


def _exact_points(rng, dims):
    """the points of test_splat_gpu.test_g2p: float32 roundings of cell centres and faces (those that became rounding
    decisions dropped, those exact in float32 kept) and five exact ones"""
    nd = len(dims)
    n = np.asarray(dims, np.float64)
    centres = (rng.randint(0, 64, (200, nd)) % n + 0.5) / n
    faces = (rng.randint(0, 64, (200, nd)) % (n + 1)) / n
    p = torch.tensor(np.concatenate([centres, faces]).astype(np.float32), device=DEV)
    tie = SR.g2p_near_tie(p, dims)
    n64 = torch.tensor(n, device=DEV)
    exact_x = ((p.double() * n64).float().double() == p.double() * n64).all(-1)
    p = p[~tie | exact_x]
    exact = torch.tensor([[0.0] * nd, [1.0] * nd, [0.5] * nd, [-0.25] * nd, [1.25] * nd], device=DEV)
    return torch.cat([p, exact]).contiguous()


def _both_routes(ops, rep, fixed_point, case, g, p, dims, cubic, ref_on_cpu=False):
    """route 0 and route 1 against the reference; -> (g_u of route 0, boxes of route 0, reference, bound).
    ``ref_on_cpu``: the reference on the host (its index_add_ of float64 onto ONE index is slow on the device)"""
    ref, plain, quanta = CREF.g2p_transpose_parts(g.cpu() if ref_on_cpu else g, p.cpu() if ref_on_cpu else p, dims, cubic,
                                                  fixed_point=fixed_point)
    ref, plain, quanta = ref.to(DEV), plain.to(DEV), quanta.to(DEV)
    bound = plain + quanta
    out0, n0 = ops.carrier_bwd(g, p, dims, cubic=cubic, route=0, count=True)
    out1, n1 = ops.carrier_bwd(g, p, dims, cubic=cubic, route=1, count=True)
    assert tuple(out0.shape) == tuple(dims) + (g.shape[1],)
    rep.check("route 0", case, out0, ref, bound)
    rep.check("route 1", case, out1, ref, plain)                    # (no fixed point on the per-tap route)
    assert int(n1) == 0 and 0 <= int(n0) <= (p.shape[0] + 255) // 256
    return out0, int(n0), ref, bound


# ---- displace ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_displace_is_g2p_bit_for_bit_and_the_sum_is_exact(ops, nd, cubic):
    rng = np.random.RandomState(4100 + 10 * nd + cubic)
    for dims in _dims(nd):
        u = torch.tensor(rng.randn(*dims, nd).astype(np.float32), device=DEV)
        p = torch.cat([torch.tensor(rng.uniform(-0.3, 1.3, (1500, nd)).astype(np.float32), device=DEV),
                       _exact_points(rng, dims)]).contiguous()
        want = ops.g2p_fwd(u, p, cubic=cubic)
        p_out, v = ops.carrier_displace(u, p, cubic=cubic)
        assert torch.equal(v, want), (dims, float((v - want).abs().max()))
        assert torch.equal(p_out, p + want), dims
        alone, none = ops.carrier_displace(u, p, cubic=cubic, want_v=False)
        assert none is None and torch.equal(alone, p_out)
    for N in (1, 257):
        p = torch.tensor(rng.uniform(0, 1, (N, nd)).astype(np.float32), device=DEV)
        p_out, v = ops.carrier_displace(u, p, cubic=cubic)
        assert torch.equal(v, ops.g2p_fwd(u, p, cubic=cubic)) and torch.equal(p_out, p + v)


def test_displace_through_autograd_is_the_transpose(ops):
    """transform.carrier_displace: differentiable in u only, and its gradient is ops.carrier_bwd of the incoming one"""
    from neural_flow_style_amd import transform as T
    rng = np.random.RandomState(4200)
    dims = (4, 5, 3)
    u = torch.tensor(rng.randn(*dims, 3).astype(np.float32), device=DEV, requires_grad=True)
    p = torch.tensor(rng.uniform(0, 1, (300, 3)).astype(np.float32), device=DEV, requires_grad=True)
    g = torch.tensor(rng.randn(300, 3).astype(np.float32), device=DEV)
    out = T.carrier_displace(u, p, cubic=True)
    assert torch.equal(out, ops.carrier_displace(u.detach(), p.detach())[0])
    out.backward(g)
    assert p.grad is None
    ref, bound = CREF.g2p_transpose(g, p.detach(), dims, True, fixed_point=CREF.header_constants())
    assert SR.err_ratio((u.grad.double() - ref).abs(), bound) <= 1.0 and float(u.grad.abs().max()) > 0


# ---- the transpose -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_bwd_uniform_and_exact_points(ops, fixed_point, nd, cubic, C):
    """uniform(-0.3, 1.3) (particles outside the domain: clipped taps that coincide, weights far above 1) and the exact
    points of test_g2p, on every dims and every N"""
    rep = Report("carrier_bwd nd=%d %s C=%d" % (nd, "cubic" if cubic else "linear", C))
    rng = np.random.RandomState(4300 + 10 * nd + cubic + 100 * C)
    for dims in _dims(nd):
        for N in NS:
            p = _uniform(rng, N, dims)
            g = torch.tensor(rng.randn(p.shape[0], C).astype(np.float32), device=DEV)
            _both_routes(ops, rep, fixed_point, "%s N=%d" % (dims, N), g, p, dims, cubic)
        p = _exact_points(rng, dims)
        g = torch.tensor(rng.randn(p.shape[0], C).astype(np.float32), device=DEV)
        _both_routes(ops, rep, fixed_point, "%s exact" % (dims,), g, p, dims, cubic)
    rep.done()


def _cloud(rng, N, nd):
    """four fifths of the particles in a cloud 0.15 of the domain wide, the rest uniform(-0.3, 1.3)"""
    k = (4 * N) // 5
    return np.concatenate([rng.uniform(0.3, 0.45, (k, nd)), rng.uniform(-0.3, 1.3, (N - k, nd))]).astype(np.float32)


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_bwd_in_grid_order_and_shuffled(ops, fixed_point, nd, cubic, C):
    """the large grids, once in transform.grid_order and once shuffled: the uniform set, and a cloud whose ordered blocks
    fit the LDS box -- those must take the box route (n_box_blocks > 0), route 1 must not (0).  Ordered and shuffled are
    the same sums: each within the bound of its own order"""
    from neural_flow_style_amd import transform as T
    rep = Report("carrier_bwd ordered nd=%d %s C=%d" % (nd, "cubic" if cubic else "linear", C))
    rng = np.random.RandomState(4400 + 10 * nd + cubic + 100 * C)
    dims = LARGE[nd]
    for name, raw in (("uniform", rng.uniform(-0.3, 1.3, (1500, nd)).astype(np.float32)), ("cloud", _cloud(rng, 1500, nd))):
        p = torch.tensor(raw, device=DEV)
        tie = SR.g2p_near_tie(p, dims)
        assert float(tie.double().mean()) <= 0.01
        p = p[~tie].contiguous()
        g = torch.tensor(rng.randn(p.shape[0], C).astype(np.float32), device=DEV)
        order = T.grid_order(p, dims)
        shuffle = torch.tensor(rng.permutation(p.shape[0]), device=DEV)
        boxes = {}
        for how, perm in (("ordered", order), ("shuffled", shuffle)):
            pp, gg = p[perm].contiguous(), g[perm].contiguous()
            _, boxes[how], _, _ = _both_routes(ops, rep, fixed_point, "%s %s %s" % (dims, name, how), gg, pp, dims, cubic)
        print("%s %s: box-route blocks ordered %d, shuffled %d of %d" % (dims, name, boxes["ordered"], boxes["shuffled"],
                                                                        (p.shape[0] + 255) // 256))
        if name == "cloud":
            assert boxes["ordered"] > 0
    rep.done()


@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_bwd_every_contribution_on_the_same_cells(ops, fixed_point, nd, cubic):
    """1024 particles at one position: four blocks, every contribution on the same 2^nd or 4^nd cells"""
    rep = Report("carrier_bwd one position nd=%d %s" % (nd, "cubic" if cubic else "linear"))
    rng = np.random.RandomState(4500 + 10 * nd + cubic)
    for dims in (LARGE[nd], G2P_DIMS[nd][0]):
        for C in (1, 3, 5):
            p = torch.tensor(np.tile(rng.uniform(0.2, 0.8, (1, nd)).astype(np.float32), (1024, 1)), device=DEV)
            assert not bool(SR.g2p_near_tie(p, dims).any())           # (seeded: drawn once, and it is none)
            g = torch.tensor(rng.randn(1024, C).astype(np.float32), device=DEV)
            out, boxes, ref, _ = _both_routes(ops, rep, fixed_point, "%s C=%d" % (dims, C), g, p, dims, cubic, ref_on_cpu=True)
            assert boxes == 4
            assert int((ref.abs().sum(-1) > 0).sum()) <= (4 if cubic else 2) ** nd
            assert bool(((ref == 0) == (out == 0)).all())             # nothing outside the stencil is touched
    rep.done()


@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_inner_product_identity_from_the_kernels(ops, fixed_point, nd, cubic):
    """<g2p(u, p), g> = <u, g2p^T(g)> from the kernels' own outputs, within the summed bounds of both sides"""
    rng = np.random.RandomState(4600 + 10 * nd + cubic)
    for dims in _dims(nd):
        p = _uniform(rng, 1500, dims)
        u = torch.tensor(rng.randn(*dims, nd).astype(np.float32), device=DEV)
        g = torch.tensor(rng.randn(p.shape[0], nd).astype(np.float32), device=DEV)
        _, v = ops.carrier_displace(u, p, cubic=cubic)
        _, bv = SR.g2p(u, p, cubic)
        _, bu = CREF.g2p_transpose(g, p, dims, cubic, fixed_point=fixed_point)
        for route in (0, 1):
            g_u = ops.carrier_bwd(g, p, dims, cubic=cubic, route=route)
            lhs, rhs = float((v.double() * g.double()).sum()), float((u.double() * g_u.double()).sum())
            slack = float((bv * g.double().abs()).sum()) + float((bu * u.double().abs()).sum())
            print("identity nd %d %s %s route %d: |lhs - rhs| %.3g of %.3g allowed" % (nd, cubic, dims, route,
                                                                                    abs(lhs - rhs), slack))
            assert abs(lhs - rhs) <= slack


def test_g_u_is_overwritten_and_n_zero_only_zeroes(ops):
    from neural_flow_style_amd import _lib
    dims, C = (4, 5, 3), 3
    g_u = torch.full(dims + (C,), 7.0, device=DEV)
    count = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    empty = torch.zeros(1, 3, device=DEV)                                # (a valid address; N = 0 reads none of it)
    stream = ops._stream()
    _lib.call("nfs_carrier_bwd", empty.data_ptr(), empty.data_ptr(), g_u.data_ptr(), count.data_ptr(), 3, 4, 5, 3, C, 0, 1,
              0, stream)
    assert float(g_u.abs().max()) == 0.0 and int(count) == 0
    p_out = torch.full((1, 3), 5.0, device=DEV)
    u = torch.zeros(dims + (3,), device=DEV)
    _lib.call("nfs_carrier_displace", u.data_ptr(), empty.data_ptr(), p_out.data_ptr(), None, 3, 4, 5, 3, 0, 1, stream)
    assert float(p_out.min()) == 5.0
    # a second call on the same buffer replaces the first
    rng = np.random.RandomState(4700)
    p = torch.tensor(rng.uniform(0, 1, (300, 3)).astype(np.float32), device=DEV)
    g = torch.tensor(rng.randn(300, C).astype(np.float32), device=DEV)
    for route in (0, 1):
        g_u.fill_(7.0)
        _lib.call("nfs_carrier_bwd", g.data_ptr(), p.data_ptr(), g_u.data_ptr(), None, 3, 4, 5, 3, C, 300, 1, route, stream)
        ref, bound = CREF.g2p_transpose(g, p, dims, True, fixed_point=CREF.header_constants())
        assert SR.err_ratio((g_u.double() - ref).abs(), bound) <= 1.0


def test_refusals_on_device_buffers(ops):
    from neural_flow_style_amd import _lib
    N, C, dims = 8, 3, (2, 3, 4)
    g = torch.zeros(N, C, device=DEV)
    p = torch.full((N, 3), 0.5, device=DEV)
    g_u = torch.full(dims + (C,), 3.0, device=DEV)
    u = torch.zeros(dims + (3,), device=DEV)
    p_out = torch.full((N, 3), 3.0, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = ops._stream()

    def refused(name, args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args, stream)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg

    ok = [g.data_ptr(), p.data_ptr(), g_u.data_ptr(), count.data_ptr(), 3, 2, 3, 4, C, N, 1, 0]
    for i in (0, 1, 2):
        refused("nfs_carrier_bwd", ok[:i] + [None] + ok[i + 1:], "null pointer")
    refused("nfs_carrier_bwd", ok[:4] + [4] + ok[5:], "nd must be 2 or 3")
    for i in (5, 6, 7, 8):
        refused("nfs_carrier_bwd", ok[:i] + [0] + ok[i + 1:], "at least 1")
    refused("nfs_carrier_bwd", ok[:9] + [-1] + ok[10:], "at least 0")
    for bad in (2, -1):
        refused("nfs_carrier_bwd", ok[:11] + [bad], "route must be 0")
    refused("nfs_carrier_bwd", ok[:5] + [2048, 1024, 1024, 1] + ok[9:], "below 2^31")
    refused("nfs_carrier_bwd", ok[:2] + [g.data_ptr()] + ok[3:], "must not alias")
    refused("nfs_carrier_bwd", ok[:2] + [p.data_ptr() + 8] + ok[3:], "must not alias")
    refused("nfs_carrier_bwd", ok[:3] + [g_u.data_ptr() + 4] + ok[4:], "must not alias")
    okd = [u.data_ptr(), p.data_ptr(), p_out.data_ptr(), None, 3, 2, 3, 4, N, 1]
    for i in (0, 1, 2):
        refused("nfs_carrier_displace", okd[:i] + [None] + okd[i + 1:], "null pointer")
    refused("nfs_carrier_displace", okd[:4] + [1] + okd[5:], "nd must be 2 or 3")
    refused("nfs_carrier_displace", okd[:5] + [0] + okd[6:], "at least 1")
    refused("nfs_carrier_displace", okd[:2] + [p.data_ptr()] + okd[3:], "must not alias")
    refused("nfs_carrier_displace", okd[:3] + [u.data_ptr()] + okd[4:], "must not alias")
    torch.cuda.synchronize()
    assert float(g_u.min()) == 3.0 and float(p_out.min()) == 3.0      # nothing was launched
    with pytest.raises(ValueError):
        ops.carrier_displace(torch.zeros(2, 3, 4, 2, device=DEV), p)
    with pytest.raises(ValueError):
        ops.carrier_bwd(g, p, (2, 3))

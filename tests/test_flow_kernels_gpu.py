"""libnfs_flow.so on the GPU (include/nfs_flow.h): nfs_flow_fwd step by step bit for bit against nfs_g2p_fwd and, at K = 1,
nfs_carrier_displace; nfs_flow_bwd step by step against the float64 ``tests/flow_ref.pull`` evaluated at the kernel's own
path[k] and lam[k+1], every element within its own bound; ``ops.flow_grad`` (both routes of the transpose) and
``transform.carrier_flow`` against the float64 adjoint on a float64 path of its own; and the scene the feature exists for:
the one-step map folds, eight steps do not.  The sweep tests print the largest err / bound they saw (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import flow_ref as FREF
from tests import splat_ref as SR
from tests.test_carrier_kernels_gpu import NS, _dims, _exact_points, _uniform
from tests.test_splat_gpu import DEV, Report

pytestmark = pytest.mark.gpu

KS = [1, 2, 5]


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


def h32(K):
    """1.0f / K as the entry points form it"""
    return float(np.float32(1.0) / np.float32(K))


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def _sets(rng, dims):
    """(name, p) of one grid: uniform(-0.3, 1.3) at every N of tests/test_carrier_kernels_gpu.py, and that file's exact
    cell centres and faces"""
    for N in NS:
        yield "N=%d" % N, _uniform(rng, N, dims)
    yield "exact", _exact_points(rng, dims)


AMP = 0.3


def _runs_away(dims, cubic):
    """whether float32 rounding alone can carry a particle of uniform(-0.3, 1.3) away on this grid.  t cells outside the
    domain the Catmull-Rom weights of an axis sum in magnitude to about 4 t^3, every tap is clipped onto the border cells
    and the sample is a sum of cancelling products: its float32 error is up to EPS AMP prod_a 4 t_a^3 in units of p, that
    is n times as many cells per unit of pseudo-time.  Where that exceeds t itself at the farthest start, t_a = 0.3 n_a +
    0.5, the next sample is taken farther out still, with an error that grew as t^(3 nd): the position reaches infinity
    within a few steps, and no reference can follow it.  (Linear weights grow as t: never.)"""
    if not cubic:
        return False
    t = [0.3 * n + 0.5 for n in dims]
    return max(dims) * SR.EPS * AMP * float(np.prod([4 * v ** 3 for v in t])) > max(t)


def _field(rng, dims, cubic):
    """a velocity of up to 0.3 of the domain per unit of pseudo-time: particles cross several cells of the small grids.
    On a grid where rounding can run away (``_runs_away``: the two large grids under the cubic kernel, none of
    G2P_DIMS) the field is that of a CLOSED domain -- zero on the outermost layer of cells, so every sample whose taps are
    all clipped onto the border is an exact zero and a particle out there stays where it is -- and moves freely inside."""
    u = rng.uniform(-AMP, AMP, tuple(dims) + (len(dims),)).astype(np.float32)
    if _runs_away(dims, cubic):
        for a in range(len(dims)):
            u[(slice(None),) * a + ([0, -1],)] = 0.0
    return torch.tensor(u, device=DEV)


def test_the_closed_fields_are_the_large_cubic_ones():
    for nd in (2, 3):
        assert [_runs_away(d, True) for d in _dims(nd)] == [False] * 5 + [True]
        assert not any(_runs_away(d, False) for d in _dims(nd))
        u = _field(np.random.RandomState(0), _dims(nd)[-1], True)
        assert float(u[0].abs().max()) == 0 and float(u[:, -1].abs().max()) == 0 and float(u[1:-1, 1:-1].abs().max()) > 0.2


# ---- forward -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_fwd_every_step_is_g2p_bit_for_bit(ops, nd, cubic, K):
    rng = np.random.RandomState(5100 + 10 * nd + cubic + 100 * K)
    h = h32(K)
    for dims in _dims(nd):
        u = _field(rng, dims, cubic)
        for name, p in _sets(rng, dims):
            path = ops.flow_fwd(u, p, K, cubic=cubic)
            assert tuple(path.shape) == (K + 1, p.shape[0], nd) and torch.equal(path[0], p), (dims, name)
            for k in range(K):
                want = path[k] + h * ops.g2p_fwd(u, path[k].contiguous(), cubic=cubic)
                assert torch.equal(path[k + 1], want), (dims, name, k, float((path[k + 1] - want).abs().max()))
            if K == 1:
                assert torch.equal(path[1], ops.carrier_displace(u, p, cubic=cubic)[0]), (dims, name)
            assert p.shape[0] < 100 or float((path[K] - p).abs().max()) > 0


# ---- the sweep ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_bwd_every_step_within_the_bound_of_the_float64_pull(ops, nd, cubic, K):
    rep = Report("flow_bwd nd=%d %s K=%d" % (nd, "cubic" if cubic else "linear", K))
    rng = np.random.RandomState(5200 + 10 * nd + cubic + 100 * K)
    h = h32(K)
    for dims in _dims(nd):
        u = _field(rng, dims, cubic)
        for name, p in _sets(rng, dims):
            N = p.shape[0]
            g = torch.tensor(rng.randn(N, nd).astype(np.float32), device=DEV)
            path = ops.flow_fwd(u, p, K, cubic=cubic)
            lam = ops.flow_bwd(u, path, g, cubic=cubic)
            assert tuple(lam.shape) == (K + 1, N, nd) and torch.equal(lam[K], g), (dims, name)
            # particles whose floor is a rounding decision at some path[k] are left out (the sets came without any at
            # k = 0: the exact points are exact in float32 there, and stay in)
            tie = torch.zeros(N, dtype=torch.bool, device=DEV)
            for k in range(1, K):
                tie |= SR.g2p_near_tie(path[k], dims)
            share = float(tie.double().mean())
            assert share <= 0.01 if N >= 100 else share == 0.0, (dims, name, share)
            keep = (~tie).repeat(K)
            # all K steps as one evaluation over the K N (position, incoming gradient) pairs the kernel saw
            ref, bound = FREF.pull(u, path[:K].reshape(K * N, nd), lam[1:].reshape(K * N, nd), h, cubic)
            rep.check("pull", "%s %s" % (dims, name), lam[:K].reshape(K * N, nd)[keep], ref[keep], bound[keep])
            assert N < 100 or float((lam[0] - g).abs().max()) > 0 or max(dims) == 1
    rep.done()


# ---- the whole gradient ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_flow_grad_against_the_float64_adjoint(ops, nd, cubic):
    """relative L2 <= 1e-3 (the project's bar for gradient parity) of g_u, by both routes of the transpose, and of g_p,
    against ``flow_ref.adjoint`` on the float64 path ``flow_ref.flow`` makes for itself; ``transform.carrier_flow`` returns
    the same two gradients through autograd.  A statement about the interior: positions in (0.05, 0.95) and a velocity of
    at most two cells (0.2 of the domain on the small grids), so no particle leaves the domain by more than a cell --
    outside it the cubic weights grow as t^3 and cancel, and a float32 path and a float64 path of its own part ways by
    far more than 1e-3 (the sweep test above holds the kernel to its bound out there, at its own path)"""
    from neural_flow_style_amd import transform as T
    rng = np.random.RandomState(5300 + 10 * nd + cubic)
    for dims, K in ((_dims(nd)[2], 5), (_dims(nd)[-1], 5), (_dims(nd)[0], 2)):
        amp = min(0.2, 2.0 / max(dims))
        u = torch.tensor(rng.uniform(-amp, amp, tuple(dims) + (nd,)).astype(np.float32), device=DEV)
        p = torch.tensor(rng.uniform(0.05, 0.95, (1500, nd)).astype(np.float32), device=DEV)
        p = p[T.grid_order(p, dims)].contiguous()
        g = torch.tensor(rng.randn(1500, nd).astype(np.float32), device=DEV)
        path64 = FREF.flow(u, p, K, cubic, discrete=torch.float64)
        want_u, want_p = FREF.adjoint(u, path64, g, cubic, discrete=torch.float64)
        path = ops.flow_fwd(u, p, K, cubic=cubic)
        print("flow nd %d %s %s K %d: float32 path[K] against the float64 one, rel-L2 %.3g"
              % (nd, "cubic" if cubic else "linear", dims, K, rel(path[K], path64[K])))
        for route in (0, 1):
            g_u, g_p = ops.flow_grad(u, path, g, cubic=cubic, route=route)
            ru, rp = rel(g_u, want_u), rel(g_p, want_p)
            print("flow_grad nd %d %s %s K %d route %d: rel-L2 g_u %.3g g_p %.3g"
                  % (nd, "cubic" if cubic else "linear", dims, K, route, ru, rp))
            assert tuple(g_u.shape) == tuple(u.shape) and tuple(g_p.shape) == tuple(p.shape)
            assert ru <= 1e-3 and rp <= 1e-3
        uv, pv = u.clone().requires_grad_(), p.clone().requires_grad_()
        out = T.carrier_flow(uv, pv, K, cubic=cubic)
        assert torch.equal(out, path[K])
        out.backward(g)
        assert torch.equal(pv.grad, g_p)                                   # (the sweep is a gather: the same bits)
        assert rel(uv.grad, want_u) <= 1e-3
        # in p alone, and in u alone
        pv2 = p.clone().requires_grad_()
        T.carrier_flow(u, pv2, K, cubic=cubic).backward(g)
        assert torch.equal(pv2.grad, g_p)
        uv2 = u.clone().requires_grad_()
        T.carrier_flow(uv2, p, K, cubic=cubic).backward(g)
        assert rel(uv2.grad, want_u) <= 1e-3


# ---- what the steps are for ----------------------------------------------------------------------------------------------

def _dets(ops, u, p, K):
    """det(d p' / d p) per particle: row a of the Jacobian is lam[0] of the sweep with g_out = e_a"""
    path = ops.flow_fwd(u, p, K, cubic=True)
    rows = []
    for a in range(3):
        e = torch.zeros_like(p)
        e[:, a] = 1.0
        rows.append(ops.flow_bwd(u, path, e, cubic=True)[0])
    return torch.linalg.det(torch.stack(rows, 1).double())


def test_one_step_folds_and_eight_do_not(ops):
    """a 4 x 5 x 3 carrier, displacements of up to 0.2 of the domain (float64 on the host: 16.0 % of the particles folded
    at K = 1, none at K = 8 with the smallest determinant 0.045; the thresholds are half of each)"""
    rng = np.random.RandomState(29)
    u = torch.tensor(rng.uniform(-0.2, 0.2, (4, 5, 3, 3)).astype(np.float32), device=DEV)
    p = torch.tensor(rng.uniform(0.05, 0.95, (300, 3)).astype(np.float32), device=DEV)
    d1, d8 = _dets(ops, u, p, 1), _dets(ops, u, p, 8)
    print("det(dp'/dp): K = 1 folded %.1f %% min %.3g; K = 8 folded %.1f %% min %.3g"
          % (100 * float((d1 <= 0).double().mean()), float(d1.min()), 100 * float((d8 <= 0).double().mean()), float(d8.min())))
    assert float((d1 <= 0).double().mean()) >= 0.08
    assert not bool((d8 <= 0).any()) and float(d8.min()) >= 0.02


# ---- the entry points ----------------------------------------------------------------------------------------------------

def test_n_zero_launches_nothing_and_refusals_on_device_buffers(ops):
    from neural_flow_style_amd import _lib
    N, K, dims = 8, 4, (2, 3, 4)
    u = torch.zeros(dims + (3,), device=DEV)
    p = torch.full((N, 3), 0.5, device=DEV)
    g = torch.zeros(N, 3, device=DEV)
    path = torch.full((K + 1, N, 3), 3.0, device=DEV)
    lam = torch.full((K + 1, N, 3), 3.0, device=DEV)
    stream = ops._stream()

    def refused(name, args, text):
        with pytest.raises(_lib.NfsError) as e:
            _lib.call(name, *args, stream)
        assert e.value.code == _lib.NFS_EINVAL
        msg = _lib.lib().nfs_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg

    okf = [u.data_ptr(), p.data_ptr(), path.data_ptr(), 3, 2, 3, 4, N, K, 1]
    okb = [u.data_ptr(), path.data_ptr(), g.data_ptr(), lam.data_ptr(), 3, 2, 3, 4, N, K, 1]
    for name, ok, n_ptr in (("nfs_flow_fwd", okf, 3), ("nfs_flow_bwd", okb, 4)):
        for i in range(n_ptr):
            refused(name, ok[:i] + [None] + ok[i + 1:], "null pointer")
        refused(name, ok[:n_ptr] + [4] + ok[n_ptr + 1:], "nd must be 2 or 3")
        for i in (n_ptr + 1, n_ptr + 2, n_ptr + 3):
            refused(name, ok[:i] + [0] + ok[i + 1:], "at least 1")
        refused(name, ok[:n_ptr + 4] + [-1] + ok[n_ptr + 5:], "at least 0")
        refused(name, ok[:n_ptr + 5] + [0] + ok[n_ptr + 6:], "K, the number of steps, must be at least 1")
        for i in range(n_ptr - 1):
            refused(name, ok[:n_ptr - 1] + [ok[i] + 8] + ok[n_ptr:], "must not alias")
        # N == 0: success, nothing written
        _lib.call(name, *(ok[:n_ptr + 4] + [0] + ok[n_ptr + 5:]), stream)
    torch.cuda.synchronize()
    assert float(path.min()) == 3.0 and float(lam.min()) == 3.0        # nothing was launched
    with pytest.raises(ValueError):
        ops.flow_fwd(torch.zeros(2, 3, 4, 2, device=DEV), p, 2)
    with pytest.raises(ValueError):
        ops.flow_bwd(u, path, g[:4])
    with pytest.raises(_lib.NfsError):
        ops.flow_fwd(u, p, 0)

"""tests/flow_ref.py without a GPU: the float64 adjoint of the K-step carrier flow against torch.autograd through K steps of
oracle.g2p run in float64 -- nd 2 and 3, cubic and linear, K in {1, 3, 8}, on the dims of tests/test_splat_gpu.G2P_DIMS (axes
of length 1 among them), positions in (-0.1, 1.1) -- and, at K = 1, g_u against tests/carrier_ref.g2p_transpose."""
import itertools

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import carrier_ref as CREF
from tests import flow_ref as FREF
from tests.test_splat_gpu import G2P_DIMS

CASES = list(itertools.product([2, 3], [False, True], [1, 3, 8]))


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def _case(nd, dims, seed, N=200, amp=0.2):
    rng = np.random.RandomState(seed)
    u = torch.tensor(rng.uniform(-amp, amp, tuple(dims) + (nd,)))
    p = torch.tensor(rng.uniform(-0.1, 1.1, (N, nd)).astype(np.float32))
    g = torch.tensor(rng.randn(N, nd))
    return u, p, g


def _oracle_flow(u, p, K, nd, cubic):
    x = p
    for _ in range(K):
        x = x + O.g2p(u[None], x[None], is_2d=nd == 2, is_linear=not cubic)[0] / K
    return x


@pytest.mark.parametrize("nd,cubic,K", CASES)
def test_adjoint_is_autograd_through_k_steps_of_the_oracle(nd, cubic, K):
    for j, dims in enumerate(G2P_DIMS[nd]):
        u, p, g = _case(nd, dims, 2900 + 100 * j + 10 * nd + cubic + 1000 * K)
        uv, pv = u.clone().requires_grad_(), p.double().requires_grad_()
        end = _oracle_flow(uv, pv, K, nd, cubic)
        want_u, want_p = torch.autograd.grad((end * g).sum(), (uv, pv))
        path = FREF.flow(u, p, K, cubic, discrete=torch.float64)
        assert tuple(path.shape) == (K + 1, p.shape[0], nd) and torch.equal(path[0], p.double())
        assert rel(path[K], end.detach()) <= 1e-12
        g_u, g_p = FREF.adjoint(u, path, g, cubic, discrete=torch.float64)
        ru, rp = rel(g_u, want_u), rel(g_p, want_p)
        print("nd %d %s K %d %s: adjoint against autograd, rel-L2 g_u %.3g g_p %.3g"
              % (nd, "cubic" if cubic else "linear", K, dims, ru, rp))
        assert tuple(g_u.shape) == tuple(dims) + (nd,) and tuple(g_p.shape) == tuple(p.shape)
        assert ru <= 1e-12 and rp <= 1e-12
        assert float((g_p - g).abs().max()) > 1e-3 or max(dims) == 1      # (the Jacobian is no identity in disguise)


@pytest.mark.parametrize("nd,cubic", list(itertools.product([2, 3], [False, True])))
def test_one_step_is_the_transpose_and_the_bound_is_a_bound(nd, cubic):
    for j, dims in enumerate(G2P_DIMS[nd]):
        u, p, g = _case(nd, dims, 3900 + 100 * j + 10 * nd + cubic)
        path = FREF.flow(u, p, 1, cubic)
        g_u, g_p = FREF.adjoint(u, path, g, cubic)
        want, _ = CREF.g2p_transpose(g, p, dims, cubic)
        assert torch.equal(g_u, want)
        value, bound = FREF.pull(u, p, g, 1.0, cubic)
        assert torch.equal(value, g_p) and bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
        # linear in the unit roundoff: a bound of some 1e-7 of the value's scale, never a loose one
        assert float((bound / (value.abs() + g.abs().max())).median()) < 1e-4


def test_the_derivative_weights_are_the_derivatives_of_the_weights():
    """central differences of ``splat_ref._g2p_axis``'s weights in x, away from the floor's jumps; their sum is zero (the
    weights sum to one), and on an axis of length 1 every tap is cell 0: the sample is constant and J vanishes"""
    from tests import splat_ref as SR
    n, d = 7, 1e-6
    p = torch.tensor(np.random.RandomState(5).uniform(-0.1, 1.1, 400))
    x = p * n
    p = p[((x - 0.5) - torch.round(x - 0.5)).abs() > 1e-3]
    for cubic in (False, True):
        _, _, _, dw, dwe = FREF._axis_d(p, n, cubic, torch.float64)
        _, hi, _ = SR._g2p_axis(p + d / n, n, cubic, torch.float64)
        _, lo, _ = SR._g2p_axis(p - d / n, n, cubic, torch.float64)
        for j in range(len(dw)):
            assert float(((hi[j] - lo[j]) / (2 * d) - dw[j]).abs().max()) <= 1e-7
            assert bool((dwe[j] >= 0).all())
        assert float(sum(dw).abs().max()) <= 1e-12
        u = torch.tensor(np.random.RandomState(6).randn(1, 1, 2))
        g = torch.tensor(np.random.RandomState(7).randn(30, 2))
        q = torch.tensor(np.random.RandomState(8).uniform(-0.1, 1.1, (30, 2)).astype(np.float32))
        value, _ = FREF.pull(u, q, g, 0.25, cubic)
        assert float((value - g).abs().max()) <= 1e-12

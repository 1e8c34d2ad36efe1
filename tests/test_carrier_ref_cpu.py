"""tests/carrier_ref.py without a GPU: the float64 transpose of g2p against torch.autograd of oracle.g2p run in float64, and
the inner-product identity <g2p(u, p), g> = <u, g2p^T(g)>, for nd 2 and 3, linear and cubic, on the dims of
tests/test_splat_gpu.G2P_DIMS (axes of length 1, 2 and 3 among them) with particles inside, on and outside the domain."""
import itertools

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import carrier_ref as CREF
from tests import splat_ref as SR
from tests.test_splat_gpu import G2P_DIMS

CASES = list(itertools.product([2, 3], [False, True]))


def _case(nd, dims, C, seed, N=300):
    rng = np.random.RandomState(seed)
    u = torch.tensor(rng.randn(*dims, C))
    rand = rng.uniform(-0.3, 1.3, (N, nd))
    n = np.asarray(dims, np.float64)
    centres = (rng.randint(0, 64, (40, nd)) % n + 0.5) / n
    exact = np.asarray([[0.0] * nd, [1.0] * nd, [0.5] * nd, [-0.25] * nd, [1.25] * nd])
    p = torch.tensor(np.concatenate([rand, centres, exact]).astype(np.float32))
    g = torch.tensor(rng.randn(p.shape[0], C))
    return u, p, g


@pytest.mark.parametrize("nd,cubic", CASES)
def test_transpose_is_autograd_of_the_oracle(nd, cubic):
    for k, dims in enumerate(G2P_DIMS[nd]):
        u, p, g = _case(nd, dims, 3, 700 + 10 * nd + cubic + 100 * k)
        uv = u.clone().requires_grad_()
        out = O.g2p(uv[None], p.double()[None], is_2d=nd == 2, is_linear=not cubic)[0]
        (want,) = torch.autograd.grad((out * g).sum(), uv)
        got, bound = CREF.g2p_transpose(g, p, dims, cubic, discrete=torch.float64)
        # both sides are float64 sums of the same terms in another order and with the weights written another way: the
        # bound is linear in the unit roundoff, so a float64 evaluation is held to 2^-29 of it (2^-53 against 2^-24),
        # times 8 for the oracle's own rounding of weights that reach |t|^3 ~ 1e2 per axis outside the domain
        err = SR.err_ratio((got - want).abs(), bound * 2.0 ** -26)
        print("nd %d %s %s: transpose against autograd, err / (2^-26 bound) %.3g" % (nd, "cubic" if cubic else "linear",
                                                                                   dims, err))
        assert tuple(got.shape) == tuple(dims) + (3,) and err <= 1.0
        assert bool((bound >= 0).all()) and bool((bound[got != 0] > 0).all())


@pytest.mark.parametrize("nd,cubic", CASES)
def test_inner_product_identity(nd, cubic):
    for k, dims in enumerate(G2P_DIMS[nd]):
        for C in (1, 3, 5):
            u, p, g = _case(nd, dims, C, 900 + 10 * nd + cubic + 100 * k + C)
            v, _ = SR.g2p(u, p, cubic)
            g_u, _ = CREF.g2p_transpose(g, p, dims, cubic)
            lhs, rhs = float((v * g).sum()), float((u * g_u).sum())
            scale = float((v.abs() * g.abs()).sum())
            assert abs(lhs - rhs) <= 1e-12 * scale, (dims, C, lhs, rhs)


def test_coinciding_taps_add_and_the_quantum_term_is_per_block():
    """an axis of length 1 takes every tap on cell 0: the transpose there is the sum of all weights (1 for both kernels)
    times g; and the fixed-point term charges each contribution its own block's quantum"""
    p = torch.tensor([[0.3, 0.2], [0.9, 0.7], [0.5, 0.5]], dtype=torch.float32)
    g = torch.tensor([[2.0], [-3.0], [0.5]], dtype=torch.float64)
    for cubic in (False, True):
        got, _ = CREF.g2p_transpose(g, p, (1, 1), cubic)
        assert abs(float(got[0, 0, 0]) - (-0.5)) <= 1e-12
    plain, b0 = CREF.g2p_transpose(g, p, (1, 1), True)
    same, b1 = CREF.g2p_transpose(g, p, (1, 1), True, fixed_point=(2, -10))
    assert torch.equal(plain, same)
    # blocks {0,1} and {2}: m = sum|w| per axis squared times |g|; 16 contributions per particle
    ax = [SR._g2p_axis(p[:, a], 1, True, torch.float32) for a in range(2)]
    m = g.abs()[:, 0] * sum(w.abs() for w in ax[0][1]) * sum(w.abs() for w in ax[1][1])
    want = 2.0 ** -10 * 16 * (2 * float(torch.max(m[0], m[1])) + float(m[2]))
    assert abs(float((b1 - b0)[0, 0, 0]) - want) <= 1e-12 * want

"""Float64 restatement of the carrier flow and of its adjoint (csrc/flow.hip, include/nfs_flow.h), built on
``tests/splat_ref._g2p_axis`` and ``tests/carrier_ref``:

    path[0] = p,  path[k+1] = path[k] + h g2p(u, path[k]),  h = 1 / K                    ``flow``
    lam[K] = g_out,  lam[k] = lam[k+1] + h J(path[k])^T lam[k+1]                          ``pull`` (one step), ``adjoint``
    (J^T lam)[a] = n_a sum_taps W_a,tap s_tap,   W_a,tap = w'_a prod_{b != a} w_b,   s_tap = u[cell(tap)] . lam
    g_u = h sum_k g2p^T(lam[k+1]; path[k]),  g_p = lam[0]                                 ``adjoint``

w' is the derivative of an axis weight in t (cubic) or dx (linear), t and dx taken from the clipped index as the sampling
takes them: -1.5 t^2 + 2 t - 0.5, 4.5 t^2 - 5 t, -4.5 t^2 + 4 t + 0.5, 1.5 t^2 - t, and -1, +1.  As in the two files this one
is built on, the floor decisions are float32 from the float32 inputs, as the kernel takes them (``discrete=torch.float64``
takes them in float64: that is autograd through K steps of oracle.g2p run in float64, which the CPU test pins this file
against); everything continuous is float64.

The bound of ``pull``, per particle and component a, is the first-order sum of the float32 roundings nfs_flow_bwd makes,
EPS = 2^-24 per correctly rounded operation, every term named (there is no fitted constant).  A fused multiply-add makes
fewer roundings than the product and the sum it replaces, so the bound holds whichever the compiler chose.

    h n_a [ sum_taps ( (We + nd EPS |W|) |s|  +  nd EPS |W| S )  +  taps^nd EPS sum_taps |W| |s| ]  +  EPS (2 h n_a |J| + |value|)

* We: the error of W_a,tap from its factors' errors, propagated through the product over the axes as ``splat_ref.g2p``
  propagates it (we |f| + fe |w| + we fe per further factor).  A factor's error is
    - a weight w_b: ``splat_ref._g2p_axis``'s own (the rounding of x = p n and of the subtraction through the slope of the
      weight, and K_CR EPS max(1, |t|)^3 for its evaluation; linear: EPS (|x| + 2 |dx| + 1));
    - a derivative weight w'_a, cubic: slope_j dt + K_DW EPS A_j with dt = EPS (|x| + |t|) (the rounding of x and of the
      subtraction), slope_j >= |d w'_j / dt| = 3|t| + 2, 9|t| + 5, 9|t| + 4, 3|t| + 1, A_j the sum of the absolute values of
      the terms of w'_j (1.5 t^2 + 2|t| + 0.5, 4.5 t^2 + 5|t|, 4.5 t^2 + 4|t| + 0.5, 1.5 t^2 + |t|) and K_DW = 5 the roundings
      of its evaluation: t t, two products by a constant, two sums, each relative to a quantity of at most A_j;
    - a derivative weight, linear: the constants -1 and +1, no error.
* nd EPS |W| |s|: the nd - 1 roundings of the products that form W from its nd factors, and the one of the product W s.
* nd EPS |W| S, S = sum_c |u[cell, c]| |lam_c|: s is nd products (EPS S together) and nd - 1 sums (EPS S each at most).
* taps^nd EPS sum |W| |s|: the taps^nd additions into J_a, partial sums below sum |W| |s|.
* EPS (2 h n_a |J| + |value|): the product n_a J_a, the product by h, and the final sum lam_a + (.).
h is taken as given (the caller passes the float32 value the kernel forms, 1.0f / K); n_a is exact in float32."""
import itertools

import torch

from tests import carrier_ref as CREF
from tests import splat_ref as SR

EPS = SR.EPS
K_DW = 5


def _sample(u, x, cubic, discrete):
    """g2p(u, x) in float64 (``splat_ref.g2p`` without its bound; x may be float64)"""
    return SR.g2p(u, x, cubic, discrete)[0]


def flow(u, p, K, cubic=True, discrete=torch.float32):
    """u [X,Y,(Z),nd], p [N,nd] -> path [K+1,N,nd] float64, every step in float64 from the float64 position before it"""
    h = 1.0 / K
    path = [p.double()]
    for _ in range(K):
        path.append(path[-1] + h * _sample(u, path[-1], cubic, discrete))
    return torch.stack(path)


def _axis_d(pk, n, cubic, discrete):
    """``splat_ref._g2p_axis`` and beside it the derivative weights and their errors: (idx, w, we, dw, dwe)"""
    idx, w, we = SR._g2p_axis(pk, n, cubic, discrete)
    x64 = pk.double() * n
    if not cubic:
        one, zero = torch.ones_like(x64), torch.zeros_like(x64)
        return idx, w, we, [-one, one], [zero, zero]
    t = x64 - (idx[1].double() + 0.5)
    a, t2 = t.abs(), t * t
    dt = EPS * (x64.abs() + a)
    dw = [-1.5 * t2 + 2 * t - 0.5, 4.5 * t2 - 5 * t, -4.5 * t2 + 4 * t + 0.5, 1.5 * t2 - t]
    slope = [3 * a + 2, 9 * a + 5, 9 * a + 4, 3 * a + 1]
    mag = [1.5 * t2 + 2 * a + 0.5, 4.5 * t2 + 5 * a, 4.5 * t2 + 4 * a + 0.5, 1.5 * t2 + a]
    return idx, w, we, dw, [s * dt + K_DW * EPS * m for s, m in zip(slope, mag)]


def pull(u, pk, lam_next, h, cubic=True, discrete=torch.float32):
    """one step of the sweep: u [X,Y,(Z),nd], pk [N,nd] = path[k], lam_next [N,nd] = lam[k+1], h
    -> (lam[k] [N,nd] float64, its bound [N,nd]); the bound is the module docstring's"""
    nd = pk.shape[1]
    dims = [int(v) for v in u.shape[:nd]]
    uf = u.double().reshape(-1, nd)
    lam = lam_next.double()
    ax = [_axis_d(pk[:, a], dims[a], cubic, discrete) for a in range(nd)]
    taps = 4 if cubic else 2
    J = torch.zeros_like(lam)
    E, S = torch.zeros_like(lam), torch.zeros_like(lam)
    for combo in itertools.product(range(taps), repeat=nd):
        flat = 0
        for a in range(nd):
            flat = flat * dims[a] + ax[a][0][combo[a]]
        uc = uf[flat]
        s, sa = (uc * lam).sum(-1), (uc.abs() * lam.abs()).sum(-1)
        for a in range(nd):
            W, We = None, None
            for b in range(nd):
                f, fe = (ax[b][3], ax[b][4]) if b == a else (ax[b][1], ax[b][2])
                f, fe = f[combo[b]], fe[combo[b]]
                if W is None:
                    W, We = f, fe
                else:
                    W, We = W * f, We * f.abs() + fe * W.abs() + We * fe
            J[:, a] += W * s
            E[:, a] += (We + nd * EPS * W.abs()) * s.abs() + nd * EPS * W.abs() * sa
            S[:, a] += W.abs() * s.abs()
    hn = h * torch.tensor([float(v) for v in dims], dtype=torch.float64, device=pk.device)
    value = lam + hn * J
    bound = hn * (E + (taps ** nd) * EPS * S) + EPS * (2 * (hn * J).abs() + value.abs())
    return value, bound


def adjoint(u, path, g_out, cubic=True, discrete=torch.float32):
    """u, path [K+1,N,nd] (of ``flow``, or a kernel's), g_out [N,nd] -> (g_u [like u], g_p [N,nd]) in float64: the sweep by
    ``pull`` with h = 1 / K, and g_u = h sum_k ``carrier_ref.g2p_transpose``(lam[k+1]; path[k])"""
    K, nd = path.shape[0] - 1, path.shape[2]
    h = 1.0 / K
    dims = [int(v) for v in u.shape[:nd]]
    lam = g_out.double()
    g_u = torch.zeros(*dims, nd, dtype=torch.float64, device=u.device)
    for k in range(K - 1, -1, -1):
        g_u += h * CREF.g2p_transpose(lam, path[k], dims, cubic, discrete)[0]
        lam = pull(u, path[k], lam, h, cubic, discrete)[0]
    return g_u, lam

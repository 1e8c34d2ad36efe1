"""Float64 restatement of the transpose of g2p in the grid (csrc/carrier.hip, include/nfs_carrier.h):
g_u[cell, c] = sum_i sum_{taps of i that land on the cell} w g_v[i, c], with a per-cell bound on what a float32 kernel may
differ from it by, in ANY order of summation.

Built on ``tests/splat_ref._g2p_axis``: the floor decisions are float32 from the float32 inputs, as the kernel takes them
(``discrete=torch.float64`` takes them in float64: that is autograd of oracle.g2p run in float64, which the CPU test pins
this file against); weights and sums are float64.  Clipping makes several taps of one particle land on the same border
cell: their weights add, because every tap is its own contribution here too.

The bound, per cell and channel, with w the weight of a contribution, we its error (``_g2p_axis``'s, propagated through the
product over the axes as ``splat_ref.g2p`` does) and n_cell the number of contributions landing on the cell:

    sum_contrib (we |g| + nd EPS |w| |g|)  +  (n_cell + 1) EPS sum_contrib |w| |g|  [+ sum_contrib quantum(block of i)]

the rounding of the weight and of the product w g; n_cell float additions in any order (partial sums are below
sum |w||g|) and one conversion of an exact partial sum to float32; and, for the kernel's fixed-point route, one quantum per
contribution: include/nfs_carrier.h states that a block of NFS_CARRIER_BLOCK consecutive particles truncates each
contribution by less than 2^NFS_CARRIER_QUANTUM_LOG2 times the block's largest m_i = (prod_a sum_taps |w_a,tap|)
max_c |g_v[i,c]|.  Both constants are read from that header."""
import itertools
import os

import torch

from tests import splat_ref as SR

EPS = SR.EPS


def header_constants():
    """NFS_CARRIER_BLOCK and NFS_CARRIER_QUANTUM_LOG2 as include/nfs_carrier.h states them"""
    from neural_flow_style_amd import _lib
    consts = _lib._read(os.path.join(os.path.dirname(_lib.HEADER_PATH), "nfs_carrier.h"))[3]
    return consts["NFS_CARRIER_BLOCK"], consts["NFS_CARRIER_QUANTUM_LOG2"]


def g2p_transpose_parts(g_v, p, dims, cubic=True, discrete=torch.float32, fixed_point=None):
    """-> (g_u, the bound without the fixed-point term, the fixed-point term): see ``g2p_transpose``"""
    nd = p.shape[1]
    dims = [int(v) for v in dims]
    assert len(dims) == nd
    N, C = g_v.shape
    cells = 1
    for v in dims:
        cells *= v
    g = g_v.double()
    ag = g.abs()
    ax = [SR._g2p_axis(p[:, a], dims[a], cubic, discrete) for a in range(nd)]
    taps = 4 if cubic else 2
    quantum = None
    if fixed_point is not None and N > 0:
        block, qlog2 = fixed_point
        m = ag.max(-1).values
        for a in range(nd):
            m = m * sum(w.abs() for w in ax[a][1])
        nb = (N + block - 1) // block
        mb = torch.zeros(nb * block, dtype=torch.float64, device=p.device)
        mb[:N] = m
        mb = mb.reshape(nb, block).max(-1).values
        quantum = (2.0 ** qlog2) * mb.repeat_interleave(block)[:N]
    out = torch.zeros(cells, C, dtype=torch.float64, device=p.device)
    A, S, Q = torch.zeros_like(out), torch.zeros_like(out), torch.zeros_like(out)
    n_cell = torch.zeros(cells, dtype=torch.float64, device=p.device)
    for combo in itertools.product(range(taps), repeat=nd):
        flat, w, we = 0, None, None
        for a in range(nd):
            wa, ea = ax[a][1][combo[a]], ax[a][2][combo[a]]
            flat = flat * dims[a] + ax[a][0][combo[a]]
            if w is None:
                w, we = wa, ea
            else:
                w, we = w * wa, we * wa.abs() + ea * w.abs() + we * ea
        out.index_add_(0, flat, w[:, None] * g)
        A.index_add_(0, flat, (we + nd * EPS * w.abs())[:, None] * ag)
        S.index_add_(0, flat, w.abs()[:, None] * ag)
        n_cell.index_add_(0, flat, torch.ones_like(w))
        if quantum is not None:
            Q.index_add_(0, flat, quantum[:, None].expand(N, C).contiguous())
    bound = A + (n_cell + 1)[:, None] * EPS * S
    return out.reshape(*dims, C), bound.reshape(*dims, C), Q.reshape(*dims, C)


def g2p_transpose(g_v, p, dims, cubic=True, discrete=torch.float32, fixed_point=None):
    """g_v [N,C], p [N,nd], dims -> (g_u [*dims,C] float64, bound [*dims,C]).
    ``fixed_point``: None, or (block, quantum_log2) of the kernel's LDS route (``header_constants()``)"""
    out, bound, Q = g2p_transpose_parts(g_v, p, dims, cubic, discrete, fixed_point)
    return out, bound + Q

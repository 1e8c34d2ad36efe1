"""The adjoint of MacCormack advection (include/nfs_hip.h: nfs_advect_maccormack_bwd) restated in float64 on the
float32 inputs, element by element, with a derived error bound for every element of both gradients.

Scheme (oracle.nfs_oracle.advect_maccormack; SL = border-replicating multilinear sample, x = voxel index):
    F = SL(d, x - v)    B = SL(F, x + v)    A = F + (d - B)/2    out = keep ? F : A
``keep`` is the limiter's comparison: piecewise constant, no gradient through it.  Given g = dL/d out:
    gA = keep ? 0 : g      gB = -gA/2      gF = g + SL^T(gB; x + v)
    g_d = gA/2 + SL^T(gF; x - v)
    g_vel = +(n-1)/2 gB grad F(x + v)  -  (n-1)/2 gF grad d(x - v)
The function takes the forward's own ``d_fwd`` and ``keep``: it decides and samples nothing again, so a kernel is held
to it on the kernel's own decisions with nothing left out.

A trace outside the volume samples one clamped cell on that axis (both clipped corners coincide): the sample is
(1 - w) f + w f = f, so the scatter puts weight 1 on that cell and the derivative along that axis is 0.

Bounds (EPS = 2^-24, float32's unit round-off), all derived, none fitted to a kernel's output:
  * a traced coordinate in cells carries float32 rounding dx_k <= 6 EPS (2 + |v_k|) (n_k - 1)/2: six roundings (the
    grid step, step * i, -1 + ., +- v, + 1, * (n-1)) of quantities no larger than 2 + |v_k| in normalised units; the
    one-FMA form of the scalar 3-D stencil has one rounding of at most EPS (n + |v| (n-1)/2), which is smaller.
  * a scatter weight moves by at most dx_k times the product of the other axes' weights; when the coordinate is within
    ``face_margin`` of a face the neighbouring cell's corners may receive that much too.
  * gF: ``count`` fixed-point additions of at most one quantum each, the float32 weights (1 - w: one rounding per
    axis, the products in double), and one rounding of the float32 result.
  * g_d: float atomics in any order -- (count + K) EPS times the sum of |contributions| per destination -- plus the
    error of gF carried through the weights.
  * g_vel: the float32 evaluation of a gradient component costs K_GRAD EPS times the larger of the spread and the
    magnitude of the sampled corners -- the lean stencil forms d/dz and d/dy as differences of *interpolated* values
    (three chained FMAs each, rounding in proportion to the values, not to their differences), the generic one as
    weighted corner differences (in proportion to the spread); then the rounding of the *other* axes' coordinates times
    twice the spread (a mixed second difference), the error of gF times the component, and the last float32 products
    and sum.
Second-order terms in dx (below 1e-9 of the first-order ones on these grids) are not carried.

``unsure`` marks the voxels where either trace lies within ``face_margin`` cells of a cell face inside the domain:
component k of a multilinear gradient jumps across a face of axis k, and a float32 coordinate may sit on the other
side of it.  ``vel_excess`` therefore accepts, per component and per half, either of the two cells that share the
face (the clamped cell beyond the border, with derivative 0, included); away from faces both candidates are the same
cell, so no element is exempt."""
import itertools
import math

import numpy as np

EPS = 2.0 ** -24
K_GRAD = 8.0          # roundings of one gradient component: two weight products, a difference, a product, the sums
K_ATOMIC = 3.0        # beyond the additions themselves: the weight product (2) and its product with the gradient (1)


def unpack_mask(words, shape):
    """the keep mask as the kernels write it (int64 words, bit e = element e) -> bool array of ``shape``"""
    w = np.asarray(words).astype(np.int64).view(np.uint64)
    n = int(np.prod(shape))
    e = np.arange(n, dtype=np.uint64)
    return (((w[(e >> np.uint64(6)).astype(np.int64)] >> (e & np.uint64(63))) & np.uint64(1)) != 0).reshape(shape)


def fixed_point_quantum(gmax, nelem):
    """the adjoint's quantum 2^-k: float32 m = (max|g| * 0.5) * nelem < 2^e (frexp), k = 62 - e"""
    m = np.float32(np.float32(np.float32(gmax) * np.float32(0.5)) * np.float32(float(nelem)))
    m = min(float(m), 3.0e38)
    if not m > 0.0:
        return 1.0
    _, e = math.frexp(m)
    return 2.0 ** (e - 62)


def _trace(dims, v64, sign, face_margin):
    """per axis: coordinate in cells, its float32 rounding bound, and the stencil (i0, i1, w0, w1 merged where clamped;
    near, alt0, alt1: the cell on the other side of a face within face_margin)"""
    axes = []
    nax = len(dims)
    for k, n in enumerate(dims):
        shape = [1] * nax
        shape[k] = n
        i = np.arange(n, dtype=np.float64).reshape(shape)
        c = (-1.0 + i * (2.0 / (n - 1) if n > 1 else 0.0)) + sign * v64[..., k]
        x = (c + 1.0) * (n - 1) * 0.5
        dx = 6 * EPS * (2.0 + np.abs(v64[..., k])) * (n - 1) * 0.5
        fl = np.clip(np.floor(x), -1, n).astype(np.int64)
        i0, i1 = np.clip(fl, 0, n - 1), np.clip(fl + 1, 0, n - 1)
        two = i0 != i1
        w1 = np.where(two, x - i0, 0.0)
        r = np.rint(x)
        near = (np.abs(x - r) < face_margin) & (r >= 0) & (r <= n - 1) & (n > 1)
        ri = r.astype(np.int64)
        a0 = np.where(x >= r, ri - 1, ri)
        alt0 = np.where(near, np.clip(a0, 0, n - 1), i0)
        alt1 = np.where(near, np.clip(a0 + 1, 0, n - 1), i1)
        axes.append(dict(n=n, x=x, dx=dx, i=(i0, i1), w=(1.0 - w1, w1), near=near, alt=(alt0, alt1)))
    return axes


def _corners(axes, skip=None):
    """index tuples and weight products over the corners of every axis but ``skip`` (there: None)"""
    ks = [k for k in range(len(axes)) if k != skip]
    for corner in itertools.product((0, 1), repeat=len(ks)):
        idx = [None] * len(axes)
        w = 1.0
        for k, b in zip(ks, corner):
            idx[k] = axes[k]["i"][b]
            w = w * axes[k]["w"][b]
        yield idx, w


def _scatter(shape, axes, vals):
    """SL^T: sum of contributions, of their magnitudes, and their number, per destination element"""
    out, m1, cnt = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for idx, w in _corners(axes):
        contrib = w[..., None] * vals
        np.add.at(out, tuple(idx), contrib)
        np.add.at(m1, tuple(idx), np.abs(contrib))
        np.add.at(cnt, tuple(idx), (contrib != 0).astype(np.float64))
    return out, m1, cnt


def _scatter_coord_error(shape, axes, mag):
    """bound on what the float32 rounding of the traced coordinates moves between destinations: per axis k, dx_k times
    the other axes' weights onto both corners of k (and onto the neighbours beyond them next to a face)"""
    out = np.zeros(shape)
    for k, ax in enumerate(axes):
        n = ax["n"]
        i0, i1 = ax["i"]
        pts = [(i0, 1.0), (i1, 1.0), (np.clip(i0 - 1, 0, n - 1), ax["near"] * 1.0), (np.clip(i1 + 1, 0, n - 1), ax["near"] * 1.0)]
        for idx, w in _corners(axes, skip=k):
            for p, on in pts:
                idx[k] = p
                np.add.at(out, tuple(idx), (w * on * ax["dx"])[..., None] * mag)
    return out


def _gradient(field, axes):
    """per axis k: the sample's derivative along k in cells for the cell the trace lies in and for the alternative
    across a nearby face [2, *dims, C]; the spread and the largest magnitude of the corners the stencil (or its
    alternatives) reads [*dims, C]"""
    comps = []
    lo = hi = None
    for k, ax in enumerate(axes):
        both = []
        for pair in (ax["i"], ax["alt"]):
            g = 0.0
            for idx, w in _corners(axes, skip=k):
                idx[k] = pair[1]
                f1 = field[tuple(idx)]
                idx[k] = pair[0]
                f0 = field[tuple(idx)]
                g = g + np.asarray(w)[..., None] * (f1 - f0)
                for f in (f0, f1):
                    lo = f if lo is None else np.minimum(lo, f)
                    hi = f if hi is None else np.maximum(hi, f)
            both.append(g)
        comps.append(np.stack(both))
    return comps, hi - lo, np.maximum(np.abs(lo), np.abs(hi))


def adjoint(d, vel, d_fwd, keep, g, init_d=None, face_margin=1e-4):
    """d, d_fwd, g [*dims, C], vel [*dims, nd] (nd == len(dims)), keep bool [*dims, C]; init_d: what g_d's buffer held.
    Returns a dict: g_d, g_vel (float64), bound_d, bound_vel, unsure [*dims], gF, e_gF, half_B and
    half_d (the two terms of g_vel = half_B - half_d), and vel_cand [2, 2, *dims, nd]
    (candidate of the B half x candidate of the d half)."""
    dims = d.shape[:-1]
    nd = vel.shape[-1]
    assert nd == len(dims)
    d64, v64, F, g64 = (np.asarray(a, dtype=np.float64) for a in (d, vel, d_fwd, g))
    shape = d64.shape
    gA = np.where(keep, 0.0, g64)
    gB = -0.5 * gA
    fw = _trace(dims, v64, +1.0, face_margin)          # x + v: where B sampled F
    bk = _trace(dims, v64, -1.0, face_margin)          # x - v: where F sampled d
    quantum = fixed_point_quantum(np.abs(np.asarray(g, dtype=np.float32)).max() if g64.size else 0.0, g64.size)
    sB, m1B, cntB = _scatter(shape, fw, gB)
    gF = g64 + sB
    e_gF = cntB * quantum + 4 * EPS * m1B + _scatter_coord_error(shape, fw, np.abs(gB)) + EPS * np.abs(gF)
    sF, m1F, cntF = _scatter(shape, bk, gF)
    init = np.zeros(shape) if init_d is None else np.asarray(init_d, dtype=np.float64)
    g_d = init + 0.5 * gA + sF
    mag = m1F + np.abs(init) + np.abs(0.5 * gA)
    e_carried, _, _ = _scatter(shape, bk, e_gF)
    bound_d = ((cntF + 1 + K_ATOMIC) * EPS * mag + 4 * EPS * m1F + _scatter_coord_error(shape, bk, np.abs(gF) + e_gF)
               + e_carried + EPS * np.abs(g_d))
    GB, spreadB, magB = _gradient(F, fw)
    Gd, spreadD, magD = _gradient(d64, bk)
    rndB, rndD = K_GRAD * EPS * np.maximum(spreadB, magB), K_GRAD * EPS * np.maximum(spreadD, magD)
    dx_fw, dx_bk = sum(a["dx"] for a in fw), sum(a["dx"] for a in bk)
    g_vel = np.zeros(dims + (nd,))
    bound_vel = np.zeros(dims + (nd,))
    cand = np.zeros((2, 2) + dims + (nd,))
    half_B, half_d = np.zeros(dims + (nd,)), np.zeros(dims + (nd,))
    for k, n in enumerate(dims):
        h = 0.5 * (n - 1)
        tB = h * (gB[None] * GB[k]).sum(-1)                     # [2, *dims]: channels summed
        tD = h * (gF[None] * Gd[k]).sum(-1)
        g_vel[..., k] = tB[0] - tD[0]
        half_B[..., k], half_d[..., k] = tB[0], tD[0]
        cand[..., k] = tB[:, None] - tD[None, :]
        eB = (np.abs(gB) * (rndB + 2 * (dx_fw - fw[k]["dx"])[..., None] * spreadB)).sum(-1)
        eD = ((np.abs(gF) + e_gF) * (rndD + 2 * (dx_bk - bk[k]["dx"])[..., None] * spreadD)
              + e_gF * np.abs(Gd[k]).max(0)).sum(-1)
        C = shape[-1]
        bound_vel[..., k] = h * (eB + eD) + (4 + C) * EPS * (np.abs(tB).max(0) + np.abs(tD).max(0))
    unsure = np.zeros(dims, bool)
    for a in fw + bk:
        unsure |= a["near"]
    return dict(g_d=g_d, g_vel=g_vel, bound_d=bound_d, bound_vel=bound_vel, unsure=unsure, gF=gF, e_gF=e_gF,
                vel_cand=cand, quantum=quantum, half_B=half_B, half_d=half_d)


def vel_excess(ref, got):
    """how far each component of ``got`` [*dims, nd] lies outside the bound around its nearest candidate (<= 0: inside)"""
    err = np.abs(np.asarray(got, dtype=np.float64)[None, None] - ref["vel_cand"])
    return err.min(axis=(0, 1)) - ref["bound_vel"]


# ---- the cases both test files run: those of test_grid_ops_gpu's per-voxel MacCormack test -----------------------------
CASES = [
    # (id, dims, C, velocity: 'random' up to 3 cells / 'integer' whole cells / 'tiny' 1e-3 cells)
    ("3d-C1", (17, 12, 20), 1, "random"), ("3d-C3-side2", (9, 2, 14), 3, "random"), ("3d-C1-side1", (1, 11, 13), 1, "random"),
    ("3d-C3", (10, 13, 7), 3, "random"), ("2d-C1", (31, 17), 1, "random"), ("2d-C3-side2", (2, 40), 3, "random"),
    ("2d-C1-side1", (1, 29), 1, "random"), ("2d-C3", (19, 24), 3, "random"),
    ("3d-C1-integer", (10, 9, 8), 1, "integer"), ("2d-C3-integer", (12, 15), 3, "integer"),
    ("3d-C3-tiny", (8, 9, 10), 3, "tiny"), ("2d-C1-tiny", (20, 14), 1, "tiny"),
]


def make_case(case):
    """(d [*dims,C], vel [*dims,nd], rng) float32, built as that test builds them (same seeds)"""
    name, dims, C, kind = case
    rng = np.random.RandomState(sum(map(ord, name)))
    nd = len(dims)
    cell = [2.0 / (n - 1) if n > 1 else 0.0 for n in dims]
    d = (rng.randn(*dims, C) * 2.0 - 0.5).astype(np.float32)
    if kind == "integer":
        k = rng.randint(-2, 3, tuple(dims) + (nd,))
        v = np.stack([k[..., a] * cell[a] for a in range(nd)], -1).astype(np.float32)
    elif kind == "tiny":
        d = (np.round(d * 2.0) / 2.0).astype(np.float32)
        v = (rng.uniform(-1e-3, 1e-3, tuple(dims) + (nd,)) * np.asarray(cell)).astype(np.float32)
    else:
        v = (rng.uniform(-3.0, 3.0, tuple(dims) + (nd,)) * np.asarray(cell)).astype(np.float32)
    return d, v, rng

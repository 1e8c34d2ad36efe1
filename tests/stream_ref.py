"""Float64 NumPy reference of the stream-function variable (grid variable 's'): the stream velocity of a stream function
psi [D,H,W,3], its transpose, the transpose with every sign made positive (the scale rounding errors are measured
against), and the discrete divergence.  Written with slices over the array axes, independent of oracle/ and of the other
references under tests/.

Definition (include/nfs_hip.h): with D_A the forward difference along array axis A, the last slice replicated (and zero
along an axis of length 1),

    vel0 = D_W psi1 - D_H psi0,   vel1 = D_D psi0 - D_W psi2,   vel2 = D_H psi2 - D_D psi1

-- the curl of transform.py:517-555 with its channels reversed, so that component k moves along array axis k.  Forward
differences commute, hence D_D vel0 + D_H vel1 + D_W vel2 = 0 wherever no replicated slice is involved."""
import numpy as np

AXIS_D, AXIS_H, AXIS_W = 0, 1, 2


def fwd_diff(a, axis):
    """forward difference along ``axis``, last slice replicated; zeros along an axis of length 1 (dtype of ``a``)"""
    n = a.shape[axis]
    out = np.zeros_like(a)
    if n < 2:
        return out
    lo = [slice(None)] * a.ndim
    hi = list(lo)
    for o in range(n):
        l = min(o, n - 2)
        dst = list(lo)
        dst[axis], lo[axis], hi[axis] = o, l, l + 1
        out[tuple(dst)] = a[tuple(hi)] - a[tuple(lo)]
    return out


def fwd_diff_T(g, axis, absolute=False):
    """transpose of ``fwd_diff``: output o = a[l + 1] - a[l], l = min(o, n - 2), sends +g[o] to l + 1 and -g[o] to l
    (``absolute``: +|g[o]| to both)"""
    n = g.shape[axis]
    out = np.zeros_like(g)
    if n < 2:
        return out
    src = [slice(None)] * g.ndim
    for o in range(n):
        l = min(o, n - 2)
        src[axis] = o
        go = np.abs(g[tuple(src)]) if absolute else g[tuple(src)]
        up, dn = list(src), list(src)
        up[axis], dn[axis] = l + 1, l
        out[tuple(up)] += go
        out[tuple(dn)] += go if absolute else -go
    return out


def velocity(s, reverse=True):
    """stream velocity [D,H,W,3] of s [D,H,W,3], in the dtype of ``s`` (float32 in: every difference and every component
    rounded once, as the kernels do).  ``reverse=False``: the curl in its own (x,y,z) channel order."""
    s0, s1, s2 = s[..., 0], s[..., 1], s[..., 2]
    v0 = fwd_diff(s1, AXIS_W) - fwd_diff(s0, AXIS_H)
    v1 = fwd_diff(s0, AXIS_D) - fwd_diff(s2, AXIS_W)
    v2 = fwd_diff(s2, AXIS_H) - fwd_diff(s1, AXIS_D)
    return np.stack([v0, v1, v2] if reverse else [v2, v1, v0], axis=-1)


def velocity_T(g, absolute=False):
    """transpose of ``velocity`` applied to g [D,H,W,3]; ``absolute``: every coefficient +1 and |g| in place of g -- the
    sum of the magnitudes of the terms, A in the tests' bounds"""
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
    sg = 1.0 if absolute else -1.0
    t = lambda x, ax: fwd_diff_T(x, ax, absolute)
    gs0 = sg * t(g0, AXIS_H) + t(g1, AXIS_D)
    gs1 = t(g0, AXIS_W) + sg * t(g2, AXIS_D)
    gs2 = sg * t(g1, AXIS_W) + t(g2, AXIS_H)
    return np.stack([gs0, gs1, gs2], axis=-1)


def divergence(vel):
    """D_D vel0 + D_H vel1 + D_W vel2 in float64, on the voxels with index <= n - 3 on every axis (no replicated slice
    within reach); empty when an axis is shorter than 3"""
    v = np.asarray(vel, np.float64)
    D, H, W = v.shape[:3]
    if min(D, H, W) < 3:
        return np.zeros((0,), np.float64)
    c = (slice(0, D - 2), slice(0, H - 2), slice(0, W - 2))
    d0 = v[1:D - 1, :H - 2, :W - 2, 0] - v[c + (0,)]
    d1 = v[:D - 2, 1:H - 1, :W - 2, 1] - v[c + (1,)]
    d2 = v[:D - 2, :H - 2, 1:W - 1, 2] - v[c + (2,)]
    return d0 + d1 + d2


def max_forward_difference(s):
    """M of the divergence bound: the largest |forward difference of s| over the three axes and channels"""
    s = np.asarray(s, np.float64)
    return max(float(np.abs(fwd_diff(s, ax)).max()) for ax in (AXIS_D, AXIS_H, AXIS_W))


def divergence_bound(s):
    """max |div| <= 12 * 2^-23 * M for a float32 stream velocity: each difference is rounded once (<= 2^-24 M relative
    to a value <= M, i.e. within 2^-23 M with room to spare) and each component, a difference of two of them, once more:
    2 * 2^-23 * M per component; the divergence sums six components"""
    return 12.0 * 2.0 ** -23 * max_forward_difference(s)


def _gauss1d(a, sigma, axis):
    r = max(int(4.0 * sigma + 0.5), 1)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="symmetric")
    out = np.zeros_like(a)
    idx = [slice(None)] * a.ndim
    for j, kj in enumerate(k):
        idx[axis] = slice(j, j + a.shape[axis])
        out += kj * p[tuple(idx)]
    return out


def make_psi(shape, cells, seed):
    """the tests' stream function: three channels of Gaussian-filtered white noise (sigma = n / 8 per axis), scaled so that
    the largest stream-velocity component is ``cells`` cells (one cell along an axis of n voxels = 2 / (n - 1)); float32.
    Never zero: at a zero velocity every back-traced point sits on a grid node, where the stencil has a kink."""
    rng = np.random.RandomState(seed)
    s = rng.randn(*shape, 3)
    for ax, n in enumerate(shape):
        s = _gauss1d(s, max(n / 8.0, 0.5), ax)
    cell = np.asarray([2.0 / max(n - 1, 1) for n in shape])
    peak = float(np.abs(velocity(s) / cell).max())
    assert peak > 0
    return (s * (cells / peak)).astype(np.float32)

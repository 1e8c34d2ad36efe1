"""Float64 NumPy reference of the potential variable (grid variable 'p') and of the Helmholtz pair (grid variable 'sp'):
the velocity each stands for, its transpose, the transpose with every sign made positive (the scale rounding errors are
measured against), and the discrete rotation and divergence.  Written with slices over the array axes, independent of
oracle/ and of the velocity code of the other references under tests/.

Definitions (include/nfs_hip.h): with D_A the forward difference along array axis A, the last slice replicated (and zero
along an axis of length 1),

    potential velocity of phi [D,H,W]:    vel0 = D_D phi,   vel1 = D_H phi,   vel2 = D_W phi
    transpose:                            g_phi = D_D^T g0 + D_H^T g1 + D_W^T g2
    Helmholtz variable a [D,H,W,4] = (psi0, psi1, psi2, phi):
        vel0 = (D_W psi1 - D_H psi0) + D_D phi,  vel1 = (D_D psi0 - D_W psi2) + D_H phi,  vel2 = (D_H psi2 - D_D psi1) + D_W phi
        (each bracket and each difference rounded once, then one addition)

-- the potential velocity is grad of transform.py:508-515 with its channels reversed, so that component k moves along array
axis k.  Forward differences commute, hence D_A vel_B = D_B vel_A for the potential part wherever no replicated slice is
involved: the flow is irrotational, as the stream part is divergence-free."""
import numpy as np


def _sl(ndim, axis, s):
    idx = [slice(None)] * ndim
    idx[axis] = s
    return tuple(idx)


def diff(a, axis):
    """D_axis a: a[i + 1] - a[i], the last slice a copy of the one before; zeros along an axis of length 1 (dtype of a)"""
    n = a.shape[axis]
    out = np.zeros_like(a)
    if n < 2:
        return out
    out[_sl(a.ndim, axis, slice(0, n - 1))] = a[_sl(a.ndim, axis, slice(1, n))] - a[_sl(a.ndim, axis, slice(0, n - 1))]
    out[_sl(a.ndim, axis, slice(n - 1, n))] = out[_sl(a.ndim, axis, slice(n - 2, n - 1))]
    return out


def diff_T(g, axis, absolute=False):
    """transpose of ``diff``: the replicated last output is the difference n - 2 once more, so its g joins that one's;
    difference i then sends +g to i + 1 and -g to i (``absolute``: +|g| to both)"""
    n = g.shape[axis]
    out = np.zeros_like(g)
    if n < 2:
        return out
    e = (np.abs(g) if absolute else g)[_sl(g.ndim, axis, slice(0, n - 1))].copy()
    e[_sl(g.ndim, axis, slice(n - 2, n - 1))] += (np.abs(g) if absolute else g)[_sl(g.ndim, axis, slice(n - 1, n))]
    out[_sl(g.ndim, axis, slice(1, n))] += e
    out[_sl(g.ndim, axis, slice(0, n - 1))] += e if absolute else -e
    return out


def velocity(phi):
    """potential velocity [D,H,W,3] of phi [D,H,W], in the dtype of ``phi`` (float32 in: every difference rounded once, as
    the kernels do)"""
    return np.stack([diff(phi, 0), diff(phi, 1), diff(phi, 2)], axis=-1)


def velocity_T(g, absolute=False):
    """transpose of ``velocity`` applied to g [D,H,W,3] -> [D,H,W]; ``absolute``: every coefficient +1 and |g| in place of
    g -- the sum of the magnitudes of the terms, A in the tests' bounds"""
    return diff_T(g[..., 0], 0, absolute) + diff_T(g[..., 1], 1, absolute) + diff_T(g[..., 2], 2, absolute)


def stream_part(a):
    """the divergence-free part of the Helmholtz velocity: from channels 0-2 of a [D,H,W,4] (or of a stream function)"""
    p0, p1, p2 = a[..., 0], a[..., 1], a[..., 2]
    return np.stack([diff(p1, 2) - diff(p0, 1), diff(p0, 0) - diff(p2, 2), diff(p2, 1) - diff(p1, 0)], axis=-1)


def helmholtz_velocity(a):
    """velocity [D,H,W,3] of a [D,H,W,4] = (psi, phi): the two parts, each formed on its own, added once"""
    return stream_part(a) + velocity(a[..., 3])


def helmholtz_velocity_T(g, absolute=False):
    """transpose of ``helmholtz_velocity`` applied to g [D,H,W,3] -> [D,H,W,4]"""
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
    sg = 1.0 if absolute else -1.0
    t = lambda x, ax: diff_T(x, ax, absolute)
    return np.stack([sg * t(g0, 1) + t(g1, 0), t(g0, 2) + sg * t(g2, 0), sg * t(g1, 2) + t(g2, 1),
                     velocity_T(g, absolute)], axis=-1)


def _inner(v):
    """the voxels with index <= n - 3 on every axis (no replicated slice within reach of one further difference)"""
    D, H, W = v.shape[:3]
    return (slice(0, D - 2), slice(0, H - 2), slice(0, W - 2))


def rotation(vel):
    """(D_H vel2 - D_W vel1, D_W vel0 - D_D vel2, D_D vel1 - D_H vel0) in float64 on the voxels with index <= n - 3 on
    every axis, [.,.,.,3]; empty when an axis is shorter than 3"""
    v = np.asarray(vel, np.float64)
    if min(v.shape[:3]) < 3:
        return np.zeros((0, 3), np.float64)
    c = _inner(v)
    d = lambda k, ax: diff(v[..., k], ax)[c]
    return np.stack([d(2, 1) - d(1, 2), d(0, 2) - d(2, 0), d(1, 0) - d(0, 1)], axis=-1)


def divergence(vel):
    """D_D vel0 + D_H vel1 + D_W vel2 in float64 on the same voxels"""
    v = np.asarray(vel, np.float64)
    if min(v.shape[:3]) < 3:
        return np.zeros((0,), np.float64)
    c = _inner(v)
    return diff(v[..., 0], 0)[c] + diff(v[..., 1], 1)[c] + diff(v[..., 2], 2)[c]


def max_forward_difference(phi):
    """M of the rotation bound: the largest |forward difference of phi| over the three axes"""
    return float(np.abs(velocity(np.asarray(phi, np.float64))).max())


def rotation_bound(phi):
    """max |rot| <= 2^-22 * M for a float32 potential velocity: a rotation component is D_A vel_B - D_B vel_A, four stored
    differences of phi that cancel exactly in exact arithmetic; each was rounded once, to within 2^-24 * M"""
    return 2.0 ** -22 * max_forward_difference(phi)


def _smooth(a, sigma, axis):
    """Gaussian filter along one axis, mirrored at the ends"""
    r = max(int(np.ceil(3.0 * sigma)), 1)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    n = a.shape[axis]
    src = np.arange(-r, n + r)
    src = np.where(src < 0, -src - 1, src)
    src = np.where(src >= n, 2 * n - 1 - src, src) % max(n, 1)
    p = np.take(a, src, axis=axis)
    out = np.zeros_like(a)
    for j, kj in enumerate(k):
        out += kj * np.take(p, np.arange(j, j + n), axis=axis)
    return out


def _noise(shape, seed, channels=None):
    rng = np.random.RandomState(seed)
    x = rng.randn(*(tuple(shape) + ((channels,) if channels else ())))
    for ax, n in enumerate(shape):
        x = _smooth(x, max(n / 8.0, 0.5), ax)
    return x


def _cells(vel, shape):
    return float(np.abs(vel / np.asarray([2.0 / max(n - 1, 1) for n in shape])).max())


def make_phi(shape, cells, seed):
    """the tests' potential: Gaussian-filtered white noise (sigma = n / 8 per axis), scaled so that the largest velocity
    component is ``cells`` cells (one cell along an axis of n voxels = 2 / (n - 1)); float32.  Never flat: no voxel where all
    three differences vanish -- at a zero velocity the back-traced point sits on a grid node, where the stencil has a kink."""
    x = _noise(shape, seed)
    peak = _cells(velocity(x), shape)
    assert peak > 0
    phi = (x * (cells / peak)).astype(np.float32)
    if min(shape) >= 2:
        assert np.abs(velocity(phi)).max(axis=-1).min() > 0
    return phi


def make_a(shape, cells, seed):
    """the tests' Helmholtz variable [D,H,W,4]: a smooth stream function and a smooth potential whose velocities have the
    same largest component, together scaled so that the largest component of the Helmholtz velocity is ``cells`` cells;
    float32"""
    x = _noise(shape, seed, channels=4)
    ps, pp = _cells(stream_part(x), shape), _cells(velocity(x[..., 3]), shape)
    assert ps > 0 and pp > 0
    x[..., :3] /= ps
    x[..., 3] /= pp
    return (x * (cells / _cells(helmholtz_velocity(x), shape))).astype(np.float32)

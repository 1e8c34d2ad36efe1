"""Float64 restatement of the view path -- rotate, the ray integral and their adjoints -- with a per-element bound on
what a float32 kernel may differ from it by.

torch float64 throughout, on the device of the inputs: the CPU tests run it on small shapes, the GPU tests on the GPU
(one view at a time at the headline size).  Conventions are the kernels' (include/nfs_hip.h):

* sample coordinates.  The kernel reads a float32 matrix R; x_a = (sum_b R_ab g_b + 1) (n_a - 1) / 2 with
  g_b = -1 + 2 o_b / (n_b - 1), and g_b = -1 when n_b = 1 (tf.linspace(-1, 1, 1) = [-1]).  Clamping x to [0, n - 1]
  and interpolating trilinearly is the reference's border replication (transform.py:395-417) restated: the two
  clipped corners coincide and their weights add up.
* rays run along axis D; the transmittance of plane z is exp(-tau sum_{z' >= z} s), far end (z = D - 1) first.
  The coefficient form splits a ray into depth segments, plane z in segment (D - 1 - z) // seg_len.

Error bounds are first-order sums of the float32 roundings a kernel can make; their constants:

* K_COORD = 16: a coordinate is formed in about ten roundings in any kernel's form (lin_coord's step and product,
  three products and sums with R, + 1, the half extent; or the adjoint's float copies of its double affine map and
  its fma per step), each at most EPS times the largest term, |c| + sum_b |A_ab o_b| <= MAG below.
* K_SAMPLE = 12: three levels of lerps a + w (b - a), three roundings each, against the largest corner |d|.
* K_ADJ = 8: the adjoint's weight products (gs wz, gs - wz1, two by wy, 1 - wx, two by ax), one rounding each.
* exp: the hardware exp2 (v_exp_f32) is within 2 ulp, the product by -tau log2(e) adds two roundings: 8 EPS with
  slack per exponential, and up to three exponentials multiply into one transmittance (segment, combination).
"""
import math

import numpy as np
import torch

EPS = 2.0 ** -24
K_COORD = 16
K_SAMPLE = 12
K_ADJ = 8
K_EXP = 8


def lattice(n, device):
    if n == 1:
        return torch.full((1,), -1.0, dtype=torch.float64, device=device)
    return -1.0 + 2.0 * torch.arange(n, dtype=torch.float64, device=device) / (n - 1)


def coords(R, shape):
    """R [3,3] (any dtype; the float32 values are used), shape (D,H,W) -> (x [D,H,W,3] unclamped voxel coordinates,
    dc [D,H,W,3] bound on a kernel's coordinate error)"""
    dev = R.device
    R = R.float().double()
    ha = torch.tensor([(n - 1) / 2.0 for n in shape], dtype=torch.float64, device=dev)
    G = torch.stack(torch.meshgrid(*[lattice(n, dev) for n in shape], indexing="ij"), -1)
    x = (G @ R.T + 1.0) * ha
    # |c| + sum_b |A_ab o_b| with c = (1 - sum_b R_ab) ha, A_ab o_b = R_ab (g_b + 1) ha: a bound on every partial sum
    mag = ha * (1.0 + (2.0 + G.abs()) @ R.abs().T)
    return x, K_COORD * EPS * mag


class Stencil:
    """the trilinear stencil of every sample of one view (output lattice [D,H,W] over a volume of the same shape)"""

    def __init__(self, R, shape):
        self.shape = tuple(shape)
        x, dc = coords(R, shape)
        dev = x.device
        nm1 = torch.tensor([n - 1 for n in shape], dtype=torch.float64, device=dev)
        xc = torch.minimum(x.clamp(min=0.0), nm1)
        base = torch.minimum(torch.floor(xc), (nm1 - 1).clamp(min=0))
        self.w = xc - base                                         # [D,H,W,3] weight of the upper corner
        self.i0 = base.long()
        self.i1 = torch.minimum(self.i0 + 1, nm1.long())
        self.dc = dc
        # the corners a coordinate within dc of xc can touch: floor(xc - dc) .. floor(xc + dc) + 1 (2 or 3 per axis)
        lo = torch.floor((xc - dc).clamp(min=0.0)).long()
        hi = torch.minimum(torch.floor(torch.minimum(xc + dc, nm1)).long() + 1, nm1.long())
        ext, emask = [], []
        for k in range(3):
            i = torch.minimum(lo + k, nm1.long())
            m = (lo + k <= hi)
            if k:
                m = m & (i != torch.minimum(lo + k - 1, nm1.long()))
            ext.append(i)
            emask.append(m)
        self.ext, self.emask = ext, emask

    def _lin(self, iz, iy, ix):
        _, H, W = self.shape
        return (iz * H + iy) * W + ix

    def corners(self):
        """(linear index, weight) of the 8 corners, k = 4 a + 2 b + c over (z, y, x)"""
        out = []
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    ii = [(self.i0, self.i1)[t][..., ax] for t, ax in ((a, 0), (b, 1), (c, 2))]
                    ww = [(1 - self.w[..., ax]) if t == 0 else self.w[..., ax] for t, ax in ((a, 0), (b, 1), (c, 2))]
                    out.append((self._lin(*ii), ww[0] * ww[1] * ww[2]))
        return out

    def ext_corners(self):
        """linear indices and 0/1 masks of the extended stencil (up to 27 distinct voxels per sample)"""
        for a in range(3):
            for b in range(3):
                for c in range(3):
                    m = self.emask[a][..., 0] & self.emask[b][..., 1] & self.emask[c][..., 2]
                    yield self._lin(self.ext[a][..., 0], self.ext[b][..., 1], self.ext[c][..., 2]), m

    def sample(self, vol):
        """vol [D,H,W] (float64) -> (samples, error bound of a float32 kernel's samples)"""
        flat = vol.reshape(-1)
        s = sum(w * flat[i] for i, w in self.corners())
        vmin = vmax = None
        amax = torch.zeros_like(s)
        for i, m in self.ext_corners():
            v = flat[i]
            vmin = v if vmin is None else torch.where(m, torch.minimum(vmin, v), vmin)
            vmax = v if vmax is None else torch.where(m, torch.maximum(vmax, v), vmax)
            amax = torch.where(m, torch.maximum(amax, v.abs()), amax)
        err = (vmax - vmin) * self.dc.sum(-1) + K_SAMPLE * EPS * amax
        return s, err

    def scatter(self, g, g_err=None):
        """adjoint of sample() at the sample gradient g [D,H,W] (float64), whose own error is g_err (or 0) ->
        dict ref (the adjoint), m1 = sum |g| w, dw = sum over the extended stencil of |g| |dc|_1 + g_err, count =
        the number of samples with g != 0 whose extended stencil holds the voxel (the contributions a kernel can
        make to it)"""
        n = g.numel()
        ref = torch.zeros(n, dtype=torch.float64, device=g.device)
        m1 = torch.zeros_like(ref)
        cnt = torch.zeros_like(ref)
        ga = g.abs().reshape(-1)
        for i, w in self.corners():
            w = w.reshape(-1)
            i = i.reshape(-1)
            ref.index_add_(0, i, g.reshape(-1) * w)
            m1.index_add_(0, i, ga * w)
        e = ga * self.dc.sum(-1).reshape(-1)
        if g_err is not None:
            e = e + g_err.reshape(-1)
        dw = torch.zeros_like(ref)
        nz = (ga != 0).double()
        for i, m in self.ext_corners():
            m = m.reshape(-1)
            dw.index_add_(0, i.reshape(-1), torch.where(m, e, torch.zeros_like(e)))
            cnt.index_add_(0, i.reshape(-1), torch.where(m, nz, torch.zeros_like(nz)))
        shp = self.shape
        return dict(ref=ref.reshape(shp), m1=m1.reshape(shp), dw=dw.reshape(shp), count=cnt.reshape(shp))


def adjoint_bound(sc, atomic, quantum=0.0, init=None):
    """bound on |kernel - sc['ref']| for one view's scatter (sum the dicts of several views first).  atomic: float
    atomics in any order (each of `count` additions rounds against the running sum); else the tiled 64-bit
    fixed point: exact sums of contributions truncated to `quantum` each, one final rounding."""
    ref, m1, dw, cnt = sc["ref"], sc["m1"], sc["dw"], sc["count"]
    b = dw + K_ADJ * EPS * m1
    if init is not None:
        ref = ref + init
        m1 = m1 + init.abs()
    if atomic:
        return b + (cnt + 1) * EPS * m1 + EPS * ref.abs()
    return b + cnt * quantum + EPS * ref.abs() + EPS * (init.abs() if init is not None else 0.0)


def add_scatters(a, b):
    return {k: a[k] + b[k] for k in a} if a is not None else dict(b)


def is_rigid(R):
    """the tiled adjoint's test for a rotation: R^T R = I to 1e-4, formed from the float32 matrix"""
    R = R.float().double()
    return bool(((R.T @ R - torch.eye(3, dtype=torch.float64, device=R.device)).abs() <= 1e-4).all())


def fixed_point_quantum(gmax, R, shape):
    """the tiled adjoint's fixed-point quantum 2^-k for max |g| = gmax over the views R [V,3,3] of a volume `shape`:
    gmax * bound < 2^e (float32 product, frexp), k = 62 - e; bound = 4 max(D,H,W) V + 8, and D H W more for every
    view that is no rotation (a launch of 32 views counts only its own: this is the coarsest quantum any launch uses)"""
    D, H, W = shape
    V = R.shape[0]
    bf = np.float32(4.0 * max(shape) * V + 8.0)
    for v in range(V):
        if not is_rigid(R[v]):
            bf = np.float32(bf + np.float32(float(D * H * W)))
    _, e = math.frexp(float(np.float32(gmax) * bf))
    return 2.0 ** (e - 62)


# ---- the ray integral ------------------------------------------------------------------------------------------------

def _suffix(x):
    return torch.flip(torch.cumsum(torch.flip(x, [0]), 0), [0])


def ray(s, es, tau, g=None):
    """s [D,...] samples along axis 0 (float64), es their error bound, g [...] the image gradient (optional) ->
    dict of the ray quantities of every mode and their bounds"""
    D = s.shape[0]
    sa = s.abs()
    acc = _suffix(s)
    T = torch.exp(-tau * acc)
    sT = s * T
    S = s.sum(0)
    Sabs = sa.sum(0)
    I = sT.sum(0)
    Iabs = (sa * T).sum(0)
    eS = es.sum(0) + D * EPS * Sabs
    # every transmittance factor sees at most the whole ray's sum error; up to three exponentials multiply into it
    eT = T * (tau * (eS + 4 * EPS * Sabs) + 3 * K_EXP * EPS)
    eI = (T * es + sa * eT).sum(0) + 2 * D * EPS * Iabs
    Tl = torch.exp(-tau * S)
    eTl = Tl * (tau * (eS + 4 * EPS * Sabs) + K_EXP * EPS)
    out = dict(raysum=S, e_raysum=eS, T=T, e_T=eT, img=I, e_img=eI, Iabs=Iabs,
               liquid=1.0 - Tl, e_liquid=eTl + EPS,
               mean=S / D, e_mean=(eS + EPS * Sabs) / D + EPS * (S / D).abs(),
               max=s.amax(0), e_max=es.amax(0))
    if g is not None:
        Q = torch.cumsum(sT, 0)                                    # sum_{z' <= z} s T
        Qabs = torch.cumsum(sa * T, 0)
        ga = g.abs()
        out["grad"] = g * (T - tau * Q)
        out["grad_mag"] = ga * (T + tau * Qabs)
        out["e_grad"] = ga * (eT + 3 * tau * eI) + 8 * EPS * ga * (T + 2 * tau * Iabs)
        out["grad_liquid"] = (g * tau * Tl).expand_as(s)
        out["e_grad_liquid"] = (ga * tau * eTl + 2 * EPS * ga * tau * Tl).expand_as(s)
        out["grad_mean"] = (g / D).expand_as(s)
        out["e_grad_mean"] = (EPS * ga / D).expand_as(s)
        m = s.amax(0)
        ties = (s == m).sum(0).double()
        out["grad_max"] = torch.where(s == m, g / ties, torch.zeros_like(s))
        out["e_grad_max"] = EPS * out["grad_max"].abs()
    return out


def segments(D, seg_len):
    """the planes of each depth segment, far segment first: [(zlo, zhi)] with plane z in segment (D - 1 - z) // seg_len"""
    out = []
    for k in range((D + seg_len - 1) // seg_len):
        zhi = D - 1 - k * seg_len
        out.append((max(zhi - seg_len + 1, 0), zhi))
    return out


def coef(s, es, tau, nseg, seg_len, g=None):
    """the coefficient form of one view: s [D,H,W].  -> dict u [D,H,W], seg [3,nseg,H,W] (segment ray sum, segment
    image sum, max |u|), their bounds, and with g the coefficients ab [nseg,H,W,2] = (g E_s, g tau (I - F_s)) and
    the sample gradient A u - B"""
    D = s.shape[0]
    segs = segments(D, seg_len)
    assert len(segs) <= nseg
    u = torch.zeros_like(s)
    eu = torch.zeros_like(s)
    seg = torch.zeros((3, nseg) + tuple(s.shape[1:]), dtype=torch.float64, device=s.device)
    eseg = torch.zeros_like(seg)
    whole = ray(s, es, tau)
    for k, (zlo, zhi) in enumerate(segs):
        r = ray(s[zlo:zhi + 1], es[zlo:zhi + 1], tau)
        sl = s[zlo:zhi + 1]
        t = r["T"]
        i = r["img"] - torch.cumsum(sl * t, 0)                     # the segment's image sum over z' > z
        u[zlo:zhi + 1] = t + tau * i
        eu[zlo:zhi + 1] = r["e_T"] + 2 * tau * r["e_img"] + 2 * EPS * (t + tau * r["Iabs"])
        seg[0, k], seg[1, k] = r["raysum"], r["img"]
        seg[2, k] = u[zlo:zhi + 1].abs().amax(0)
        eseg[0, k], eseg[1, k] = r["e_raysum"], r["e_img"]
        eseg[2, k] = eu[zlo:zhi + 1].amax(0)
    out = dict(u=u, e_u=eu, seg=seg, e_seg=eseg, img=whole["img"], e_img=whole["e_img"], raysum=whole["raysum"],
               e_raysum=whole["e_raysum"])
    if g is not None:
        ab, eab = ray_coef(g, seg, tau)
        out["ab"] = ab
        G = torch.zeros_like(s)
        for k, (zlo, zhi) in enumerate(segs):
            G[zlo:zhi + 1] = ab[k, ..., 0] * u[zlo:zhi + 1] - ab[k, ..., 1]
        out["grad"] = G
    return out


def ray_coef(g, seg, tau):
    """(A, B) per (segment, ray) from a seg triple [3,nseg,...] and the image gradient g [...] (float64), and a bound
    on a float32 kernel's (A, B) computed from the same seg: E_s = exp(-tau P_s), P_s = the ray sums of the farther
    segments, F_s = sum_{s' < s} E_s' I_s', I = F_nseg; A = g E_s, B = g tau (I - F_s)"""
    nseg = seg.shape[1]
    S, Is = seg[0], seg[1]
    P = torch.cumsum(S, 0) - S
    Pabs = torch.cumsum(S.abs(), 0) - S.abs()
    E = torch.exp(-tau * P)
    EI = E * Is
    F = torch.cumsum(EI, 0) - EI
    Itot = EI.sum(0)
    J = (E * Is.abs()).sum(0)
    A = g * E
    B = g * tau * (Itot - F)
    ga = g.abs()
    Ptot = S.abs().sum(0)
    eE = E * (tau * nseg * EPS * Pabs + K_EXP * EPS)
    eF = (K_EXP + 2 * nseg) * EPS * (1 + tau * Ptot) * J
    eA = ga * eE + EPS * A.abs()
    eB = ga * tau * (2 * eF + 4 * EPS * J) + EPS * B.abs()
    return torch.stack([A, B], -1), torch.stack([eA, eB], -1)


def coef_grad(u, ab, seg_len):
    """the sample gradient A u - B from a kernel's own u [D,H,W] and ab [nseg,H,W,2] (float64) and the bound of its
    fma, relative to |A| |u| + |B|"""
    D = u.shape[0]
    G = torch.zeros_like(u)
    e = torch.zeros_like(u)
    for k, (zlo, zhi) in enumerate(segments(D, seg_len)):
        A, B = ab[k, ..., 0], ab[k, ..., 1]
        G[zlo:zhi + 1] = A * u[zlo:zhi + 1] - B
        e[zlo:zhi + 1] = 2 * EPS * (A.abs() * u[zlo:zhi + 1].abs() + B.abs())
    return G, e


# ---- how much weight one voxel collects ----------------------------------------------------------------------------

def weight_per_voxel(R, shape):
    """the adjoint of one view at g = 1: the summed trilinear weight every voxel collects (float64)"""
    st = Stencil(R, shape)
    return st.scatter(torch.ones(shape, dtype=torch.float64, device=R.device))["ref"]


def bound_factor(V, shape):
    """the tiled adjoint's launcher bound on the summed weight of a voxel over V rotation views"""
    return 4.0 * max(shape) * V + 8.0


def err_ratio(err, bound):
    """largest err / bound (elements with bound 0 must have err 0)"""
    err = err.double()
    bound = bound.double()
    bad = (bound == 0) & (err != 0)
    if bool(bad.any()):
        return math.inf
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0

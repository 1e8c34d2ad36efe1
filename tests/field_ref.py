"""The first-order field path restated in float64 on the float32 inputs, element by element, with a derived error bound
for every element: the border-replicating trilinear sample (nfs_advect_fwd, nfs_transport_step, nfs_warp3d_fwd), its
adjoint (nfs_advect_bwd, nfs_warp3d_bwd), the [1,k,1]/(k+2) smoothing with its sign-bit mask (nfs_smooth3d_relu_fwd /
_bwd) and TF ApplyAdam (nfs_adam_tf_step, the fused update of nfs_advect_bwd_adam).  The stencil pieces (trace, corners,
scatter, gradient, candidates at faces) are those of tests/maccormack_ref.py; the order-1 adjoint is that module's with
``keep`` all true (gA = gB = 0, gF = g), written here without the error its second-order half carries.

Two stencils compute the same sample (csrc/warp.hip):
  * lean (advect1_kernel, transport_step_kernel: scalar or 3-channel fields with every side >= 2): the coordinate in
    cells by one FMA, CLAMPED to [0, n-1], base cell min(floor, n-2), weights in [0, 1]; the sample by chained FMAs
    (x within each row, then y, then z).
  * generic (warp_*_kernel, transport_step_generic_kernel, the oracle): x = (c + 1)(n - 1)/2, both corners clipped, the
    weight w1 = x - clipped i0 NOT clamped: outside the volume the two corners coincide and carry 1 - w1 and w1, which
    sum to one but are as large as the distance to the border.  Every rounding of the weighted sum then scales with
        A = prod_k (|1 - w1_k| + |w1_k|)      (1 inside the volume),
    the amplification the bounds of the generic stencil carry.  It is the reference's own arithmetic, not a defect.

Bounds (EPS = 2^-24, float32's unit round-off); every constant is counted from the arithmetic, none is fitted to a
kernel's output:
  * spread and magnitude are taken over every corner a float32 coordinate can make the stencil read (_near_range: the
    own cell and, within face_margin of a face, the cell across it, on every axis).
  * coordinate: dx_k of maccormack_ref._trace per axis (six roundings of quantities <= 2 + |v_k|; the lean FMA has one);
    with a scale one more rounding of scale * v_k.  An explicit coordinate c is traced as the velocity lin - c (its own
    two roundings are among the six).  The sample moves by at most dx_k times the spread of the corners (those of the
    cell across a face within face_margin included): it is continuous across faces, so it needs no candidates.
  * sample, lean: each of the three levels takes a difference (EPS spread) and an FMA (EPS magnitude) and passes the
    error of the level below through a convex combination: K_LEAN = 3 times EPS (spread + magnitude), both taken over
    the cell the lean stencil loads (_lean_range: on a clamped axis that includes a neighbour of weight zero).
  * sample, generic: per term 1 - w1 (1), the weight product (2), the product with the corner (1), w1 itself (1), and
    the 7 additions of the 8-term sum: K_GENERIC = 12 times EPS A magnitude.
  * scatter (always the generic stencil, float atomics): per contribution K_SCATTER = 4 roundings (1 - w1, two products,
    the product with g), per destination one rounding for each contribution that can arrive (all eight corners of a
    voxel, the coinciding ones too) and one for what the buffer held, each of at most EPS times the summed magnitudes
    (amplified by A); plus the coordinate rounding moving weight between destinations (_scatter_coord_error).
  * gradient component, generic: four terms of two 1 - w roundings, a weight product, a difference and a product (5) and
    3 additions: K_GRAD = 8 times EPS A_other max(spread, magnitude) (A over the other two axes; on a clamped axis the
    two corners are one and the difference is an exact zero; the magnitude, as in maccormack_ref, because autograd through
    the oracle forms the component as a signed sum of the eight weighted corners, not of their differences).
  * gradient component, lean (lean_grad): d/dz = b1 - b0 of twice-interpolated values, each off by 2 EPS (spread +
    magnitude), plus the difference's own rounding: 4 * 2 + 1 = K_GRAD_LEAN = 9 times EPS max(spread, magnitude), over
    the cell the lean stencil loads; d/dy and d/dx have fewer.  Then, for both stencils as in maccormack_ref: the other axes' coordinate rounding
    times twice the spread, and 4 + C roundings of the products with g, the channel sum and the (n-1)/2 factor.
  * smoothing: three passes of fma(wa, c, fma(wb, b, wa a)) -- 3 roundings each -- and per pass weights off by at most
    3 EPS (k + 2, its reciprocal, k times it): K_SMOOTH = 18 times EPS times the same filter applied to |d|.
  * Adam: see ``adam``.
Second-order terms in EPS are not carried."""
import itertools

import numpy as np

from tests import maccormack_ref as MR
from tests.maccormack_ref import EPS, vel_excess  # noqa: F401  (vel_excess: re-exported for the tests)

K_LEAN = 3.0
K_GENERIC = 12.0
K_SCATTER = 4.0
K_GRAD = MR.K_GRAD
K_GRAD_LEAN = 9.0
K_SMOOTH = 18.0
K_ADAM_M = 3.0        # b1 m, (1 - b1) g, their sum
K_ADAM_V = 4.0        # b2 v, (1 - b2) g, times g, the sum
K_ADAM_X = 4.0        # lr_t m', sqrt, + eps, the division (the subtraction is EPS |x'|)
FACE_MARGIN = 1e-4


# ---- the stencil ---------------------------------------------------------------------------------------------------
def _lin(dims, k):
    n = dims[k]
    shape = [1] * len(dims)
    shape[k] = n
    return -1.0 + np.arange(n, dtype=np.float64).reshape(shape) * (2.0 / (n - 1) if n > 1 else 0.0)


def trace(dims, cv, scale=1.0, explicit=False, face_margin=FACE_MARGIN):
    """maccormack_ref._trace for x - scale * vel (cv = vel [*dims, nd]) or for explicit coordinates (cv [nd, *dims])"""
    dims = tuple(dims)
    cv = np.asarray(cv, dtype=np.float64)
    if explicit:
        v = np.stack([_lin(dims, k) - cv[k] for k in range(len(dims))], -1)
    else:
        v = cv * float(scale)
    axes = MR._trace(dims, v, -1.0, face_margin)
    if not explicit and scale != 1.0:
        for k, ax in enumerate(axes):
            ax["dx"] = ax["dx"] + EPS * np.abs(v[..., k]) * (ax["n"] - 1) * 0.5
    return axes


def amplification(axes):
    """per axis |1 - w1| + |w1| of the generic stencil's un-clamped weight w1 = x - clipped i0 (1 inside the volume)"""
    out = []
    for ax in axes:
        w1 = ax["x"] - ax["i"][0]
        out.append(np.abs(1.0 - w1) + np.abs(w1))
    return out


def _prod(arrs, skip=None):
    p = 1.0
    for k, a in enumerate(arrs):
        if k != skip:
            p = p * a
    return p


def _interp(f, axes):
    s = 0.0
    for idx, w in MR._corners(axes):
        s = s + np.asarray(w)[..., None] * f[tuple(idx)]
    return s


def _near_range(f, axes):
    """spread and largest magnitude over every corner a float32 coordinate can make the stencil read: per axis the own
    pair and the pair across a face within face_margin, in every combination (maccormack_ref._gradient crosses one axis
    at a time; a trace on a lattice node is near a face of all three)"""
    lo = hi = None
    for idx in itertools.product(*[(ax["i"][0], ax["i"][1], ax["alt"][0], ax["alt"][1]) for ax in axes]):
        v = f[tuple(idx)]
        lo = v if lo is None else np.minimum(lo, v)
        hi = v if hi is None else np.maximum(hi, v)
    return hi - lo, np.maximum(np.abs(lo), np.abs(hi))


def _lean_range(f, axes, spread, mag):
    """spread and magnitude over what the LEAN stencil reads as well: its cell is base = min(floor of the clamped
    coordinate, n - 2) on every axis, so on a clamped axis it loads (and rounds in proportion to) a neighbour of weight
    zero that the merged stencil of maccormack_ref never sees"""
    dims = f.shape[:-1]
    base = []
    for ax in axes:
        n = ax["n"]
        b = np.minimum(np.floor(np.clip(ax["x"], 0, n - 1)), max(n - 2, 0)).astype(np.int64)
        base.append(np.broadcast_to(b, dims))
    lo = hi = None
    for c in np.ndindex(*[min(n, 2) for n in dims]):
        v = f[tuple(b + k for b, k in zip(base, c))]
        lo = v if lo is None else np.minimum(lo, v)
        hi = v if hi is None else np.maximum(hi, v)
    return np.maximum(spread, hi - lo), np.maximum(mag, np.maximum(np.abs(lo), np.abs(hi)))


def sample(field, cv, scale=1.0, explicit=False, stencil="generic", face_margin=FACE_MARGIN):
    """field [*dims, C] sampled at x - scale * vel (cv [*dims, nd]) or at explicit normalised coordinates (cv [nd, *dims]);
    any C, axes of length 1, 2-D as D == 1.  Returns (sample, bound) [*dims, C] for the ``stencil`` ('lean' / 'generic')"""
    f = np.asarray(field, dtype=np.float64)
    axes = trace(f.shape[:-1], cv, scale, explicit, face_margin)
    s = _interp(f, axes)
    spread, mag = _near_range(f, axes)
    coord = sum(a["dx"] for a in axes)[..., None] * spread
    if stencil == "lean":
        spread, mag = _lean_range(f, axes, spread, mag)
        rnd = K_LEAN * EPS * (spread + mag)
    else:
        rnd = K_GENERIC * EPS * _prod(amplification(axes))[..., None] * mag
    return s, coord + rnd


def transport(g, u, scale=1.0, w_g=1.0, addend=None, w_addend=0.0, stencil="generic"):
    """w_g * sample(g, x - scale u) + w_addend * addend: |w_g| times the sample's bound plus the roundings of the two
    products and the sum (an FMA has fewer)"""
    s, b = sample(g, u, scale=scale, stencil=stencil)
    a = 0.0 if addend is None else float(w_addend) * np.asarray(addend, dtype=np.float64)
    out = float(w_g) * s + a
    return out, abs(float(w_g)) * b + EPS * (np.abs(float(w_g) * s) + np.abs(a) + np.abs(out))


def _adjoint(f, axes, g, init, stencil):
    """SL^T g (+ init) and the gradient of the sample along every axis in normalised units, summed over the channels.
    Returns g_src, bound_src, cand [2, *dims, nd] (own cell / the cell across a near face), bound_coord, unsure"""
    shape, dims = f.shape, f.shape[:-1]
    nd, C = len(dims), f.shape[-1]
    amp = amplification(axes)
    A = _prod(amp)
    sF, _, _ = MR._scatter(shape, axes, g)
    m1A, _, _ = MR._scatter(shape, axes, A[..., None] * np.abs(g))
    cnt = np.zeros(shape)
    for idx, _w in MR._corners(axes):
        np.add.at(cnt, tuple(idx), (g != 0).astype(np.float64))
    g_src = init + sF
    bound_src = ((cnt + 1) * EPS * (m1A + np.abs(init)) + K_SCATTER * EPS * m1A
                 + MR._scatter_coord_error(shape, axes, np.abs(g)))
    G, _, _ = MR._gradient(f, axes)
    spread, mag = _near_range(f, axes)
    if stencil == "lean":
        spread, mag = _lean_range(f, axes, spread, mag)
    dx_tot = sum(a["dx"] for a in axes)
    cand = np.zeros((2,) + dims + (nd,))
    bound = np.zeros(dims + (nd,))
    for k, n in enumerate(dims):
        h = 0.5 * (n - 1)
        cand[..., k] = h * (g[None] * G[k]).sum(-1)
        if stencil == "lean":
            rnd = K_GRAD_LEAN * EPS * np.maximum(spread, mag)
        else:
            rnd = K_GRAD * EPS * _prod(amp, skip=k)[..., None] * np.maximum(spread, mag)
        e = (np.abs(g) * (rnd + 2 * (dx_tot - axes[k]["dx"])[..., None] * spread)).sum(-1)
        bound[..., k] = h * e + (4 + C) * EPS * h * (np.abs(g)[None] * np.abs(G[k])).sum(-1).max(0)
    unsure = np.zeros(dims, bool)
    for a in axes:
        unsure |= a["near"]
    return g_src, bound_src, cand, bound, unsure


def advect_adjoint(d, vel, g, init_d=None, stencil="generic", face_margin=FACE_MARGIN):
    """adjoint of out = SL(d, x - vel): d, g [*dims, C], vel [*dims, nd]; init_d: what g_d's buffer held.  Returns a dict
    in maccormack_ref.adjoint's layout: g_d, bound_d (the scatter is always the generic stencil's), g_vel, bound_vel,
    vel_cand [2, 2, *dims, nd] (vel_excess accepts either cell sharing a face within face_margin of the trace: the
    two-candidate latitude) and unsure [*dims], the voxels where the two candidates can differ"""
    f, v, g64 = (np.asarray(a, dtype=np.float64) for a in (d, vel, g))
    init = np.zeros(f.shape) if init_d is None else np.asarray(init_d, dtype=np.float64)
    axes = trace(f.shape[:-1], v, face_margin=face_margin)
    g_d, bound_d, cand, bound, unsure = _adjoint(f, axes, g64, init, stencil)
    return dict(g_d=g_d, bound_d=bound_d, g_vel=-cand[0], bound_vel=bound, vel_cand=np.stack([-cand, -cand]),
                unsure=unsure)


def warp_fwd(imgs, coords, stencil="generic"):
    """nfs_warp3d_fwd: imgs [B,X,Y,Z,C], coords [B,3,X,Y,Z] -> (out, bound) [B,X,Y,Z,C]; nfs_warp2d_fwd on two axes:
    imgs [B,X,Y,C], coords [B,2,X,Y] (nothing below assumes three: the 2-D stencil has fewer roundings than K_GENERIC
    counts)"""
    res = [sample(imgs[b], coords[b], explicit=True, stencil=stencil) for b in range(imgs.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def warp_adjoint(imgs, coords, g):
    """nfs_warp3d_bwd: g_imgs [B,X,Y,Z,C] and g_coords [B,3,X,Y,Z] with their bounds; vel_cand / bound_vel hold the
    coordinate gradient per batch entry in [X,Y,Z,3] layout for vel_excess.  nfs_warp2d_bwd on two axes: g_imgs
    [B,X,Y,C], g_coords [B,2,X,Y], the candidates in [X,Y,2] layout"""
    out = []
    for b in range(imgs.shape[0]):
        f = np.asarray(imgs[b], dtype=np.float64)
        axes = trace(f.shape[:-1], coords[b], explicit=True)
        g_src, bound_src, cand, bound, unsure = _adjoint(f, axes, np.asarray(g[b], dtype=np.float64), np.zeros(f.shape),
                                                         "generic")
        out.append(dict(g_d=g_src, bound_d=bound_src, g_vel=cand[0], bound_vel=bound, vel_cand=np.stack([cand, cand]),
                        unsure=unsure))
    return out


def lean_live(d, vel, face_margin=FACE_MARGIN):
    """the live bit of advect1_kernel in float64: 'the eight corners of the lean stencil's cell (base min(floor of the
    clamped coordinate), n - 2)) are not all equal'.  d [D,H,W], vel [D,H,W,3] -> bool [8, D, H, W]: the decision for
    every choice of own cell / cell across a face within face_margin per axis (all eight agree away from faces)"""
    d = np.asarray(d)
    dims = d.shape
    axes = trace(dims, vel, face_margin=face_margin)
    bases = []
    for ax in axes:
        n = ax["n"]
        own = np.minimum(np.floor(np.clip(ax["x"], 0, n - 1)), n - 2).astype(np.int64)
        r = np.rint(ax["x"])
        other = np.where(ax["x"] >= r, r - 1, r).astype(np.int64)
        bases.append((own, np.where(ax["near"], np.clip(other, 0, n - 2), own)))
    out = []
    for pick in np.ndindex(2, 2, 2):
        b = [np.broadcast_to(bases[k][pick[k]], dims) for k in range(3)]
        first = d[b[0], b[1], b[2]]
        differ = np.zeros(dims, bool)
        for c in np.ndindex(2, 2, 2):
            differ |= d[b[0] + c[0], b[1] + c[1], b[2] + c[2]] != first
        out.append(differ)
    return np.stack(out)


# ---- smoothing -----------------------------------------------------------------------------------------------------
def smooth_linear(a, k):
    """separable [1,k,1]/(k+2) along z, y, x with SAME zero padding; k <= 0: the identity.  Symmetric taps and zero
    padding make it its own transpose (``smooth_T``)"""
    a = np.asarray(a, dtype=np.float64)
    if k <= 0:
        return a.copy()
    wa, wb = 1.0 / (k + 2.0), k / (k + 2.0)
    for axis in (2, 1, 0):
        pad = [(0, 0)] * 3
        pad[axis] = (1, 1)
        p = np.pad(a, pad)
        sl = [slice(None)] * 3
        lo, hi = list(sl), list(sl)
        lo[axis], hi[axis] = slice(0, -2), slice(2, None)
        a = wa * (p[tuple(lo)] + p[tuple(hi)]) + wb * a
    return a


def smooth_T(g, k):
    """the transpose of smooth_linear: g_d[i] = sum_j W[j, i] g[j] with W[j, i] = W[i, j]"""
    return smooth_linear(g, k)


def smooth_bound(a, k):
    return K_SMOOTH * EPS * smooth_linear(np.abs(np.asarray(a, dtype=np.float64)), k) if k > 0 else np.zeros(np.shape(a))


def smooth(d, k):
    """(max(pre, 0), pre, bound) of nfs_smooth3d_relu_fwd for d [D,H,W]"""
    pre = smooth_linear(d, k)
    return np.maximum(pre, 0.0), pre, smooth_bound(d, k)


def smooth_adjoint(g, mask, k):
    """(smooth^T(g * mask), bound): mask = the kernel's own decisions (sign bit clear)"""
    gm = np.asarray(g, dtype=np.float64) * np.asarray(mask, dtype=np.float64)
    return smooth_T(gm, k), smooth_bound(gm, k)


# ---- TF ApplyAdam --------------------------------------------------------------------------------------------------
def adam(x, m, v, g, lr_t, b1=0.9, b2=0.999, eps=1e-8):
    """one TF ApplyAdam step in float64 from float32 state and the float32 gradient as given.  The scalars are used as
    given: pass the float32 values the kernel receives (then 1 - b, one float32 subtraction of neighbours of 1, is exact):
        m' = b1 m + (1 - b1) g,  v' = b2 v + (1 - b2) g g,  x' = x - lr_t m' / (sqrt(v') + eps).
    Bounds: m' three roundings (two products, the sum; an FMA has two) of at most EPS (|b1 m| + |(1 - b1) g|) each; v'
    four (b2 v, (1 - b2) g, times g, the sum) likewise; x': the product lr_t m', the square root, the addition of eps and
    the division -- K_ADAM_X = 4 times EPS times the step lr_t |m'| / (sqrt(v') + eps) -- the error of the float32 m' and
    v' the kernel divides carried through (v' has no cancellation: its square root is off by bound_v / (2 sqrt v')),
    and EPS |x'| for the subtraction.  Returns x', m', v', bound_x, bound_m, bound_v"""
    x, m, v, g = (np.asarray(a, dtype=np.float64) for a in (x, m, v, g))
    lr, c1, c2, ep = float(lr_t), float(b1), float(b2), float(eps)
    o1, o2 = 1.0 - c1, 1.0 - c2
    m1 = c1 * m + o1 * g
    bm = K_ADAM_M * EPS * (np.abs(c1 * m) + np.abs(o1 * g))
    v1 = c2 * v + o2 * g * g
    bv = K_ADAM_V * EPS * (np.abs(c2 * v) + o2 * g * g)
    s = np.sqrt(v1)
    step = lr * m1 / (s + ep)
    ds = np.where(s > 0, bv / (2.0 * np.where(s > 0, s, 1.0)), 0.0)
    x1 = x - step
    bx = (K_ADAM_X * EPS * np.abs(step) + abs(lr) * bm / (s + ep) + np.abs(step) * ds / (s + ep) + EPS * np.abs(x1))
    return x1, m1, v1, bx, bm, bv


B1, B2, ADAM_EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))


def err_ratio(err, bound):
    """largest err / bound over the elements: 0 where the error is zero, inf where an error meets a zero bound or where
    the error is not a number (a NaN or an infinity in what is checked never passes)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(np.where(np.isfinite(r), r, np.inf)))


def vel_ratio(ref, got):
    """err_ratio for a velocity (coordinate) gradient: the distance of every component of ``got`` to its nearest
    candidate (vel_excess) over bound_vel"""
    err = np.abs(np.asarray(got, dtype=np.float64)[None, None] - ref["vel_cand"]).min(axis=(0, 1))
    return err_ratio(np.where(np.isfinite(np.asarray(got, dtype=np.float64)), err, np.nan), ref["bound_vel"])


# ---- the cases both test files run -----------------------------------------------------------------------------------
# taken by the lean kernel (all three sides >= 2, n % 4 == 0): a partial wave; W < 64 (walk64 wraps rows and planes); W at
# and past a wave; n = 1024; 9 of 16 blocks with work (the XCD permutation leaves empty blocks inside the grid); 16
# blocks with a partial last wave
LEAN_SHAPES = [(2, 2, 2), (8, 6, 2), (5, 3, 4), (3, 4, 64), (3, 5, 68), (4, 8, 32), (9, 10, 92), (12, 20, 68)]
# refused by it: n % 4 != 0, a side of 1
GENERIC_SHAPES = [(11, 9, 13), (3, 3, 3), (1, 11, 13), (9, 1, 14), (9, 14, 1)]
MULTI_SHAPES = [(6, 8, 5), (12, 10, 16)]          # C = 2 and C = 3
KINDS = ["random", "integer", "tiny", "far", "zero"]
CAPPED_KINDS = ("random", "far")                   # the kinds the 1 % latitude cap holds for


def takes_lean(shape, C=1):
    return C == 1 and min(shape) >= 2 and int(np.prod(shape)) % 4 == 0


def smoke_density(shape):
    """exact-zero regions, a plateau clipped at 1 and smooth flanks (test_dead_skip_gpu's field)"""
    D, H, W = shape
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    r2 = ((zz - D / 2) / (D / 3.0)) ** 2 + ((yy - H / 2) / (H / 3.0)) ** 2 + ((xx - W / 2) / (W / 3.0)) ** 2
    d = np.clip(2.5 * np.exp(-3.0 * r2), 0, 1).astype(np.float32)
    d[d < 0.05] = 0.0
    return d


def make_case(shape, C, kind, density="randn"):
    """(d [*shape, C], vel [*shape, 3], rng) float32; cell = 2/(n-1): 'random' up to 3 cells, 'integer' whole cells (traces
    on faces and on the border), 'tiny' 1e-3 cells on a density rounded to halves, 'far' 1.5 .. 4 normalised units (most
    traces leave the volume), 'zero'"""
    rng = np.random.RandomState((sum(shape) * 131 + int(np.prod(shape)) * 7 + C * 17 + KINDS.index(kind)) % (2 ** 31))
    cell = np.asarray([2.0 / (n - 1) if n > 1 else 0.0 for n in shape])
    if density == "smoke":
        assert C == 1
        d = smoke_density(shape)[..., None]
    else:
        d = (rng.randn(*shape, C) * 2.0 - 0.5).astype(np.float32)
    vs = tuple(shape) + (3,)
    if kind == "integer":
        v = (rng.randint(-2, 3, vs) * cell).astype(np.float32)
    elif kind == "tiny":
        if density != "smoke":
            d = (np.round(d * 2.0) / 2.0).astype(np.float32)
        v = (rng.uniform(-1e-3, 1e-3, vs) * cell).astype(np.float32)
    elif kind == "far":
        v = (rng.uniform(1.5, 4.0, vs) * rng.choice([-1.0, 1.0], vs)).astype(np.float32)
    elif kind == "zero":
        v = np.zeros(vs, np.float32)
    else:
        v = (rng.uniform(-3.0, 3.0, vs) * cell).astype(np.float32)
    return d, v, rng


def field_cases():
    """(shape, C) of every advect case of the GPU test"""
    return ([(s, 1) for s in LEAN_SHAPES + GENERIC_SHAPES] + [(s, C) for s in MULTI_SHAPES for C in (2, 3)])


# transport_step.  Lean (C = 1, 3 with every side >= 2: two voxels per lane, 512 per block): a partial wave, n odd,
# n = 512 * 8 - 1, n just past 512 * 8, 9 of 16 blocks with work; generic: C = 2, a side of 1
TRANSPORT_CASES = [((2, 2, 2), 1), ((5, 3, 3), 3), ((7, 9, 65), 1), ((7, 9, 65), 3), ((2, 3, 683), 1), ((2, 3, 683), 3),
                   ((9, 10, 92), 1), ((6, 8, 5), 2), ((12, 10, 16), 2), ((1, 11, 13), 1), ((9, 1, 14), 3), ((9, 14, 1), 1)]
TRANSPORT_KINDS = ("random", "far", "integer")
TRANSPORT_SCALES = (1.0, -1.0, 2.0)
TRANSPORT_W_G, TRANSPORT_W_ADD = float(np.float32(0.7)), 0.25


def transport_takes_lean(shape, C):
    return C in (1, 3) and min(shape) >= 2


WARP_SHAPES = [(7, 6, 9), (5, 8, 1)]              # [X,Y,Z]; Z == 1 takes the gather without 8-byte pairs


def warp_case(shape, C):
    """imgs [2,X,Y,Z,C], explicit coordinates [2,3,X,Y,Z] in [-1.3, 1.3], g like imgs"""
    rng = np.random.RandomState(sum(shape) + C)
    imgs = (rng.randn(2, *shape, C) * 2.0 - 0.5).astype(np.float32)
    coords = rng.uniform(-1.3, 1.3, (2, 3) + tuple(shape)).astype(np.float32)
    g = rng.randn(2, *shape, C).astype(np.float32)
    return imgs, coords, g


SMOOTH_KS = [3.0, 0.5, 0.0]
# at and either side of the 8-row / 64-column / 25-plane tile
SMOOTH_SHAPES = [(1, 1, 1), (2, 9, 65), (25, 8, 64), (26, 17, 66), (51, 7, 129), (7, 9, 1), (7, 1, 13)]
SMOOTH_SHAPES_16 = [(26, 17, 55), (3, 33, 28)]     # run with the 16-row instance forced


def smooth_input(shape, seed=0):
    """randn with leading planes (two; fewer where D <= 2, so that a plane of data is left) and one interior
    3x3x3-padded block (5^3 where it fits) of exact zeros"""
    rng = np.random.RandomState(1000 + seed + sum(shape))
    d = rng.randn(*shape).astype(np.float32)
    d[:min(2, shape[0] - 1)] = 0.0
    if int(np.prod(shape)) > 1:
        c = [n // 2 for n in shape]
        d[max(c[0] - 2, 0):c[0] + 3, max(c[1] - 2, 0):c[1] + 3, max(c[2] - 2, 0):c[2] + 3] = 0.0
    return d


ADAM_NS = [1, 3, 4, 7, 1003, 4096]


def adam_case(n):
    """x, m, v (non-zero state), and three gradients mixing 1.0, 1e-7 and exact zeros"""
    rng = np.random.RandomState(77 + n)
    x = rng.randn(n).astype(np.float32)
    m = (rng.randn(n) * 0.1).astype(np.float32)
    v = (rng.rand(n) * 0.01).astype(np.float32)
    gs = []
    for _ in range(3):
        g = rng.randn(n).astype(np.float32)
        pick = rng.randint(0, 4, n)
        g[pick == 0] = 1.0
        g[pick == 1] = 1e-7
        g[pick == 2] = 0.0
        gs.append(g)
    return x, m, v, gs

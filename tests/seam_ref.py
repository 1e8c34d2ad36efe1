"""The seam between a rendered image and the loss network, and the small kernels beside it, restated in numpy with a
derived bound for every element: max-normalisation (nfs_maxnorm_fwd / _bwd, K5), its fusion with the loss-net input
(nfs_maxnorm_input_fwd / _bwd, K5f), the loss-net input (nfs_loss_net_input_fwd / _bwd, A5), the legacy bicubic resize
(nfs_resize_bicubic_tf1, K24) and the elementwise links of the 2-D colour stylizer (nfs_colour_clamp_gather,
nfs_clamp01_bwd, nfs_colour_clamp_scatter_bwd, nfs_iterate_update, nfs_fill, nfs_axpy).  The explicit 2-D warp
(nfs_warp2d_fwd / _bwd) is tests/field_ref.py's warp_fwd / warp_adjoint on two axes; only its cases live here.

What is exact (restated in numpy float32, compared bit for bit).  IEEE division, a single product and a single sum are
correctly rounded and a maximum does not depend on its order, so
  * K5 forward: gmax = max(x), out = x / gmax;
  * K5f forward: StoreInput rounds every operation (contract(off)): x[., c] = fl(fl(fl(x / m) 255) - mean_c);
  * K5f's incoming gradient: GradInput likewise: g = fl(fl(fl(255 g0) + fl(255 g1)) + fl(255 g2));
  * A5 at the image's own size: d_img = fl(255 img), g_img = fl(255 g_x), for a grey image GradInput's sum of the three;
  * the 2-D links: none has a product that could be contracted (clamps, selects, one subtraction and one addition).
A group whose maximum is zero (0 / 0) or that holds a NaN (fmaxf drops it, the comparisons x == m do not) is out of
scope of the max-normalisation's adjoint; the forward of a group with maximum +0.0 over negative values is held to its
gmax bit for bit and to the IEEE quotients (-inf, and a NaN of either sign for 0 / 0).

Bounds (U = 2^-24, one float32 rounding; every constant is counted from the kernel's arithmetic, none is fitted to an
output, second-order terms are not carried).

K5 / K5f adjoint, g_x[i] = g[i] / m - [x[i] == m] corr, corr = s / (m m) / ties, s = sum_j g[j] x[j]:
  * every element: the division, U |g / m|;
  * the elements that hold the maximum, besides: the sum's error over m^2 ties, three roundings of corr (m m, the two
    divisions: K_CORR = 3) and the subtraction's own, U |g_x|.  The tie count is a sum of ones: exact.
  * the sum: a term passes through one product (none under an FMA), the chain of the thread that owns it, the six
    steps of the wave's butterfly, the serial sum over the block's waves and, in the two-phase form, the serial sum of
    the MN_NB = 32 partials.  sum_depth counts them:
        one block of 1024 threads:   ceil(n / 1024) + 6 + 16
        32 blocks of 256 threads:    ceil(n / 8192) + 6 + 4 + 32
    (the chain of L terms has L - 1 additions; the product takes the L-th place).  The error of s is at most
    depth U sum |g x| -- 40 U for n = 16387 in one block, 45 U in 32, where n U would be 16387 U: one dropped element
    moves s by its own |g x|, some 1 / n of sum |g x|, and that is 2^24 / (45 n) = 23 bounds at the largest case.
  nfs_maxnorm_bwd takes the two-phase form for n >= 16384 with a workspace, one block otherwise; nfs_maxnorm_input_bwd
  always takes the two-phase form.
  Exact cases: m a power of two, x multiples of 1/4 with |x| <= |m|, g small integers, ties in {1, 2, 4}: s, g / m and
  corr are float32 numbers in any summation order (``units`` below 2^24 is the precondition) and the kernel must EQUAL
  the float64 value.

A5, the contract (legacy TF): scale = f32(in) / f32(out), s = f32(dst) scale in float32, i0 = floor(s),
i1 = min(i0 + 1, in - 1), w = s - i0; everything after that in float64 on the float32 image:
    top = tl + (tr - tl) wx, bot likewise, r = top + (bot - top) wy, d_img = 255 r, x = d_img - mean.
  * per lerp level the difference, the weight (rounded where the build forms it from the unrounded product dst scale)
    and the product are off by at most U spread each (K_LERP_SPREAD = 3, spread over the four corners) and the sum by
    U magnitude (K_LERP_MAG = 1, the largest |corner|); two levels, the first passing through the convex second;
  * the coordinate: where the build contracts s - i0 with the product, w moves by U |s|: U |s_x| times the larger of
    |tr - tl|, |br - bl|, and U |s_y| times the larger of |bl - tl|, |br - tr|;
  * times 255, plus U |d_img| for that product; x carries U |x| more for the subtraction.
  x against d_img: x is fl(d_img - mean) (off by U |x|) or, contracted, fl(255 r - mean) with d_img = fl(255 r) (off
  by U |d_img| more): |x - (d_img - mean)| <= U (|d_img| + |x|).  (U |d_img| alone is broken by honest float32: mean has
  an ulp of 2^-17 and a small d_img a finer one, so the plain rounded difference is already off by up to U |x|.)
  Adjoint: every input pixel is the float64 sum of its contributions c = g wy wx, g = 255 g_x (Cin = 1: the sum of the
  three).  Built as field_ref's scatter bound: per contribution K_A5_SCATTER = 4 roundings (1 - wy, 1 - wx, two
  products) and those of g (one product; Cin = 1: three products and two sums, each at most U sum_c |255 g_c|), one
  rounding per arriving addend (all four corners of an output pixel, the coinciding and the zero-weight ones too), each
  of at most U times the summed magnitudes; and the coordinate: U (|s| + 1) |g| times the other axis' weight, onto
  both corners of the axis.
  Exact cases: scales of 2 and 1/2 per axis give weights in {0, 1/2}; images in multiples of 1/4 and integer gradients
  make every product and partial sum a float32 (``units``): d_img and g_img must EQUAL the float64 value, x its rounding.

K24: coordinate and table index as the kernel and TF form them in float32, src = f32(o) (f32(in) / f32(out)),
t = rint((src - floor(src)) 1024) / 1024; Keys weights (A = -0.75) in float64 at that t; taps floor - 1 .. floor + 2
clamped; rows first, then columns.  t, t + 1, 1 - t and 2 - t are exact (multiples of 1/1024 below 2), the constants
A + 2, A + 3, 5A, 8A, 4A too.  The weights' error is carried through the float32 Horner forms step by step
(_keys_weights: per step one product and one sum, each U times its own magnitude, the error so far times the factor),
the two 4-term sums take one product and three additions each, at most U times the summed magnitudes each:
    bound = (K_BICUBIC = 8) U sum |wy| |wx| |x|  +  sum (e_wy |wx| + |wy| e_wx) |x|.
  At the image's own size t = 0 and the weights are exactly [0, 1, 0, 0]: the output equals the input bit for bit.
  A condition on the inputs, not a tolerance: where the subtraction src - floor is contracted with the product, the
  table index could flip if (src - floor) 1024 lay within 1024 2U src of a half-integer; bicubic_tie_margin measures
  that distance and the CPU test asserts that no coordinate of any case is that near a tie.

axpy: y + a x in float64, within U (|a x| + |y + a x|): the product's rounding and the sum's (an FMA has only the
second).  (U (|y| + |a x|) is the FMA's worst case alone; the two separate roundings break it where y and a x have the
same sign.)"""
import math

import numpy as np

from tests.field_ref import err_ratio  # noqa: F401  (re-exported for the two test files)
from tests.loss_ref import LIMIT, U, is_f32, units  # noqa: F401

F32 = np.float32
MEAN = np.asarray([F32(0.485) * F32(255.0), F32(0.456) * F32(255.0), F32(0.406) * F32(255.0)], dtype=np.float32)
FLT_MAX = np.finfo(np.float32).max

K_CORR = 3.0
K_LERP_SPREAD, K_LERP_MAG = 3.0, 1.0
K_A5_SCATTER = 4.0
K_BICUBIC = 8.0
MN_NB = 32
MN_MULTI = 16384                 # the first n per group that takes 32 blocks


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


# ---- K5 / K5f ----------------------------------------------------------------------------------------------------------
def sum_depth(n, two_phase):
    """the roundings a term of s = sum g x passes through (module docstring)"""
    if two_phase:
        return math.ceil(n / (256.0 * MN_NB)) + 6 + 4 + MN_NB
    return math.ceil(n / 1024.0) + 6 + 16


def maxnorm_fwd(x):
    """x float32 [G, n] -> (out, gmax) in numpy float32: exact"""
    x = np.asarray(x, dtype=np.float32)
    m = x.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return x / m[:, None], m


def maxnorm_input_fwd(x):
    """x float32 [G, n] -> (x_net [G, n, 3], gmax): StoreInput in numpy float32, exact"""
    y, m = maxnorm_fwd(x)
    v = y * F32(255.0)
    return np.stack([v - MEAN[0], v - MEAN[1], v - MEAN[2]], -1), m


def grad_input(g_x):
    """GradInput in numpy float32: [..., 3] -> [...]"""
    g = np.asarray(g_x, dtype=np.float32) * F32(255.0)
    return (g[..., 0] + g[..., 1]) + g[..., 2]


def maxnorm_adjoint(x, g, two_phase):
    """x, g float32 [G, n] -> (g_x float64, bound)"""
    x64, g64 = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n = x64.shape[1]
    m = x64.max(axis=1, keepdims=True)
    tie = x64 == m
    ties = tie.sum(axis=1, keepdims=True).astype(np.float64)
    s = (g64 * x64).sum(axis=1, keepdims=True)
    s_abs = np.abs(g64 * x64).sum(axis=1, keepdims=True)
    corr = s / (m * m * ties)
    gx = g64 / m - tie * corr
    bound = U * np.abs(g64 / m) + tie * (sum_depth(n, two_phase) * U * s_abs / (m * m * ties) + K_CORR * U * np.abs(corr)
                                         + U * np.abs(gx))
    return gx, bound


def maxnorm_exact_units(x, g):
    """the precondition of the exact cases: the largest number of units any partial sum of s, g / m and the result can
    take.  x multiples of 1/4, g integers, m a power of two, ties a power of two: s counts in 1/4, the result in
    1 / (4 m^2 ties)"""
    x64, g64 = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    m = x64.max(axis=1, keepdims=True)
    ties = (x64 == m).sum(axis=1, keepdims=True).astype(np.float64)
    worst = units(np.abs(g64 * x64).sum(axis=1), 0.25)
    for j in range(x64.shape[0]):
        unit = 0.25 / float(m[j, 0] ** 2 * ties[j, 0])
        s_abs = np.abs(g64[j] * x64[j]).sum()
        worst = max(worst, units(np.abs(g64[j] / m[j]) + s_abs / (m[j] ** 2 * ties[j]), unit))
    return worst


MAXNORM_NS = [1, 5, 1023, 1025, 16383, 16384, 16387]
MAXNORM_GS = [1, 3]
MAXNORM_CASES = [(G, n) for n in MAXNORM_NS for G in MAXNORM_GS]
SIGNS = ("pos", "neg", "mixed")


def maxnorm_plants(n):
    """where the single maximum is planted in turn: 0, 3, the last element of the float4 walk, the first tail element,
    the last element (those that exist, each once)"""
    out = []
    for p in (0, 3, 4 * (n // 4) - 1, 4 * (n // 4), n - 1):
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def maxnorm_tie_sets(n):
    """ties of 2 and of 4: from 16384 elements on in four different blocks of the 32-block walk (block = i / 256 mod 32:
    0, 21, 10, 30), below that in different waves where the group has them"""
    out = []
    if n >= 2:
        out.append([min(3, n - 2), n - 1])
    if n >= 4:
        out.append([1, n // 3, 2 * n // 3 + 1, n - (300 if n >= 1024 else 2)] if n >= 8 else [0, 1, n - 2, n - 1])
    return out


def maxnorm_variants(n):
    """every (plant positions) of one (G, n): the single plants, then the tie sets"""
    return [[p] for p in maxnorm_plants(n)] + maxnorm_tie_sets(n)


def _negative_mask(n, rng):
    """mixed-sign groups: from 1024 elements on, whole 256-element chunks are negative (chunk mod 3 != 0 -- in the
    32-block walk block b owns the chunks b, b + 32, ...: at n <= 16387 the blocks 1, 2, 4, 5, ... see only negative
    values, the blocks 0, 3, 6, ... positive ones); smaller groups mix element by element"""
    i = np.arange(n)
    if n >= 1024:
        return ((i // 256) % MN_NB) % 3 != 0
    return rng.rand(n) < 0.6


def maxnorm_case(G, n, variant, exact=False, zero_group=False):
    """x [G, n] float32 with the maximum of every group at the positions ``plants``; group j of variant v takes the sign
    SIGNS[(v + j) % 3]: all-positive, all-negative, or mixed (random cases: negative values down to -3 under a maximum
    of 1.37, so a maximum over magnitudes is a different number).  exact: multiples of 1/4 under a power of two.  zero_group: group 0
    becomes negative values under a maximum of +0.0 (forward only).  Returns x, signs"""
    plants = maxnorm_variants(n)[variant]
    rng = np.random.RandomState(1000 * n + 10 * G + variant + (500 if exact else 0))
    x = np.empty((G, n), np.float32)
    signs = []
    for j in range(G):
        sign = SIGNS[(variant + j) % 3]
        signs.append(sign)
        if exact:
            mag = rng.randint(3, 8, n) * 0.25                  # 0.75 .. 1.75
            top = {"pos": 2.0, "neg": -0.5, "mixed": 2.0}[sign]
            low = rng.randint(3, 9, n) * -0.25                 # -0.75 .. -2 (|x| <= |m|)
        else:
            mag = rng.uniform(0.1, 1.0, n)
            top = {"pos": 1.37, "neg": -0.05, "mixed": 1.37}[sign]
            low = -rng.uniform(0.1, 3.0, n)
        if sign == "pos":
            v = mag
        elif sign == "neg":
            v = -mag
        else:
            v = np.where(_negative_mask(n, rng), low, mag)
        v = np.asarray(v, np.float64)
        v[plants] = top
        x[j] = v.astype(np.float32)
    if zero_group:
        x[0] = -np.abs(x[0]) - F32(0.125)
        x[0, plants] = 0.0
        signs[0] = "zero"
    return x, signs


def maxnorm_grad(G, n, variant, exact=False, channels=1):
    """the incoming gradient [G, n] (channels = 3: K5f's g_x [G, n, 3]); exact: small integers, thinned for K5f so that
    255 (g0 + g1 + g2) x stays below 2^24 units"""
    rng = np.random.RandomState(7000 + 1000 * n + 10 * G + variant + channels)
    shape = (G, n) if channels == 1 else (G, n, channels)
    if not exact:
        return rng.randn(*shape).astype(np.float32)
    if channels == 1:
        return rng.randint(-3, 4, shape).astype(np.float32)
    return (rng.randint(-1, 2, shape) * (rng.rand(*shape) < 0.125)).astype(np.float32)


# ---- A5 ----------------------------------------------------------------------------------------------------------------
def tf1_axis(n_in, n_out):
    """(i0, i1, w float64, s float64) of the legacy bilinear resize with the float32 coordinate of the contract"""
    scale = F32(n_in) / F32(n_out)
    s = np.arange(n_out, dtype=np.float32) * scale
    assert s.dtype == np.float32
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    s64 = s.astype(np.float64)
    return i0, i1, s64 - i0, s64


def tf1_floor_agrees(n_in, n_out):
    """the float32 floor(s) is the floor of the exact rational dst in / out"""
    i0 = tf1_axis(n_in, n_out)[0]
    return bool(np.array_equal(i0, (np.arange(n_out, dtype=np.int64) * n_in) // n_out))


def _corners4(img64, H2, W2):
    B, H, W, C = img64.shape
    y0, y1, wy, sy = tf1_axis(H, H2)
    x0, x1, wx, sx = tf1_axis(W, W2)
    tl, tr = img64[:, y0][:, :, x0], img64[:, y0][:, :, x1]
    bl, br = img64[:, y1][:, :, x0], img64[:, y1][:, :, x1]
    return (tl, tr, bl, br), wy.reshape(1, H2, 1, 1), wx.reshape(1, 1, W2, 1), sy.reshape(1, H2, 1, 1), sx.reshape(1, 1, W2, 1)


def loss_net_input(img, H2, W2):
    """img float32 [B, H, W, Cin] -> d_img, x (float64 [B, H2, W2, 3]), their bounds, and the coordinate term that
    bound_d holds (what one rounding of each coordinate can move d_img by)"""
    img64 = np.asarray(img, dtype=np.float64)
    B, H, W, Cin = img64.shape
    if (H2, W2) == (H, W):
        r, br_, co = img64, np.zeros(img64.shape), np.zeros(img64.shape)
    else:
        (tl, tr, bl, br), wy, wx, sy, sx = _corners4(img64, H2, W2)
        top = tl + (tr - tl) * wx
        bot = bl + (br - bl) * wx
        r = top + (bot - top) * wy
        st = np.stack([tl, tr, bl, br])
        spread, mag = st.max(0) - st.min(0), np.abs(st).max(0)
        co = U * sx * np.maximum(np.abs(tr - tl), np.abs(br - bl)) + U * sy * np.maximum(np.abs(bl - tl), np.abs(br - tr))
        br_ = 2 * U * (K_LERP_SPREAD * spread + K_LERP_MAG * mag) + co
    d = 255.0 * r
    bd = 255.0 * br_ + U * np.abs(d)
    co = 255.0 * co
    if Cin == 1:
        d, bd, co = np.repeat(d, 3, -1), np.repeat(bd, 3, -1), np.repeat(co, 3, -1)
    x = d - MEAN.astype(np.float64)
    return d, x, bd, bd + U * np.abs(x), co


def loss_net_input_adjoint(g_x, H, W, Cin):
    """g_x float32 [B, H2, W2, 3] -> (g_img float64 [B, H, W, Cin], bound, the coordinate term the bound holds)"""
    g3 = 255.0 * np.asarray(g_x, dtype=np.float64)
    B, H2, W2, _ = g3.shape
    if Cin == 1:
        g = g3.sum(-1, keepdims=True)
        gabs = np.abs(g3).sum(-1, keepdims=True)
        kg = 3.0
    else:
        g, gabs, kg = g3, np.abs(g3), 1.0
    if (H2, W2) == (H, W):
        return g, kg * U * gabs, np.zeros(g.shape)
    y0, y1, wy, sy = tf1_axis(H, H2)
    x0, x1, wx, sx = tf1_axis(W, W2)
    out, m1, coord, cnt = (np.zeros((B, H, W, Cin)) for _ in range(4))
    bb = np.arange(B).reshape(B, 1, 1)
    dy, dx = (U * (sy + 1.0)).reshape(1, H2, 1, 1), (U * (sx + 1.0)).reshape(1, 1, W2, 1)
    for iy, qy in ((y0, 1.0 - wy), (y1, wy)):
        for ix, qx in ((x0, 1.0 - wx), (x1, wx)):
            w = qy.reshape(1, H2, 1, 1) * qx.reshape(1, 1, W2, 1)
            idx = (bb, iy.reshape(1, H2, 1), ix.reshape(1, 1, W2))
            np.add.at(out, idx, w * g)
            np.add.at(m1, idx, w * gabs)
            np.add.at(cnt, idx, np.ones(g.shape))
            np.add.at(coord, idx, (dy * qx.reshape(1, 1, W2, 1) + dx * qy.reshape(1, H2, 1, 1)) * gabs)
    return out, (cnt + K_A5_SCATTER + kg) * U * m1 + coord, coord


A5_CASES = [((10, 12), (10, 12)), ((10, 12), (15, 18)), ((13, 11), (9, 8)), ((20, 16), (5, 4)), ((10, 12), (15, 12)),
            ((10, 12), (10, 18)), ((1, 7), (3, 14)), ((7, 1), (14, 2)), ((33, 70), (49, 105))]
A5_EXACT_CASES = [((10, 12), (20, 24)), ((10, 12), (5, 6)), ((10, 12), (20, 6)), ((10, 12), (5, 24))]
A5_CINS = [1, 3]
A5_B = 2


def a5_case(hw, hw2, Cin, exact=False):
    """img [2, H, W, Cin] in [0, 1] and g_x [2, H2, W2, 3]; exact: multiples of 1/4 and integers"""
    rng = np.random.RandomState(hw[0] * 131 + hw[1] * 17 + hw2[0] * 7 + hw2[1] + Cin + (900 if exact else 0))
    if exact:
        img = (rng.randint(0, 5, (A5_B,) + hw + (Cin,)) * 0.25).astype(np.float32)
        g = rng.randint(-3, 4, (A5_B,) + hw2 + (3,)).astype(np.float32)
    else:
        img = rng.rand(A5_B, *hw, Cin).astype(np.float32)
        g = rng.randn(A5_B, *hw2, 3).astype(np.float32)
    return img, g


# ---- K24 ---------------------------------------------------------------------------------------------------------------
def _keys_weights(t):
    """Keys weights (A = -0.75) at t in float64 [n, 4] and the error bound of the kernel's float32 Horner forms"""
    a = -0.75

    def outer(v):                      # ((a v - 5a) v + 8a) v - 4a
        p0 = a * v
        p1 = p0 - 5 * a
        e = U * (np.abs(p0) + np.abs(p1))
        p2 = p1 * v
        p3 = p2 + 8 * a
        e = e * v + U * (np.abs(p2) + np.abs(p3))
        p4 = p3 * v
        p5 = p4 - 4 * a
        return p5, e * v + U * (np.abs(p4) + np.abs(p5))

    def inner(v):                      # ((a + 2) v - (a + 3)) v v + 1
        q0 = (a + 2) * v
        q1 = q0 - (a + 3)
        e = U * (np.abs(q0) + np.abs(q1))
        q2 = q1 * v
        e = e * v + U * np.abs(q2)
        q3 = q2 * v
        e = e * v + U * np.abs(q3)
        q4 = q3 + 1.0
        return q4, e + U * np.abs(q4)

    u = 1.0 - t
    w0, e0 = outer(t + 1.0)
    w1, e1 = inner(t)
    w2, e2 = inner(u)
    w3, e3 = outer(u + 1.0)
    return np.stack([w0, w1, w2, w3], 1), np.stack([e0, e1, e2, e3], 1)


def bicubic_axis(n_in, n_out, raw_fraction=False):
    """taps [n_out, 4] (clamped), weights float64 [n_out, 4], their error bound, and the float32 coordinate"""
    src = np.arange(n_out, dtype=np.float32) * (F32(n_in) / F32(n_out))
    fl = np.floor(src)
    frac = (src - fl) * F32(1024.0)
    assert frac.dtype == np.float32
    t = frac.astype(np.float64) / 1024.0 if raw_fraction else np.rint(frac).astype(np.float64) / 1024.0
    loc = fl.astype(np.int64)
    idx = np.clip(np.stack([loc - 1, loc, loc + 1, loc + 2], 1), 0, n_in - 1)
    w, e = _keys_weights(t)
    return idx, w, e, src


def bicubic_tie_margin(n_in, n_out):
    """(distance of (src - floor) 1024 to the nearest half-integer, the margin 1024 2U src a contracted subtraction
    could move it by), both [n_out], from the exact rational coordinate"""
    o = np.arange(n_out, dtype=np.int64)
    num = o * n_in                                            # src = num / n_out
    frac1024 = ((num % n_out) * 1024.0) / n_out
    dist = np.abs(frac1024 - np.floor(frac1024) - 0.5)
    return dist, 1024.0 * 2.0 * U * (num / float(n_out))


def resize_bicubic(x, oh, ow):
    """x float32 [B, H, W, C] -> (out float64 [B, oh, ow, C], bound, the weights' share of the bound)"""
    x64 = np.asarray(x, dtype=np.float64)
    B, H, W, C = x64.shape
    iy, wy, ey, _ = bicubic_axis(H, oh)
    ix, wx, ex, _ = bicubic_axis(W, ow)
    out, mag, werr = np.zeros((B, oh, ow, C)), np.zeros((B, oh, ow, C)), np.zeros((B, oh, ow, C))
    for k in range(4):
        rows = x64[:, iy[:, k]]                               # [B, oh, W, C]
        for q in range(4):
            v = rows[:, :, ix[:, q]]                          # [B, oh, ow, C]
            a, b = wy[:, k].reshape(1, oh, 1, 1), wx[:, q].reshape(1, 1, ow, 1)
            ea, eb = ey[:, k].reshape(1, oh, 1, 1), ex[:, q].reshape(1, 1, ow, 1)
            out += a * b * v
            mag += np.abs(a * b * v)
            werr += (ea * np.abs(b) + np.abs(a) * eb) * np.abs(v)
    return out, K_BICUBIC * U * mag + werr, werr


BICUBIC_CASES = [((17, 12), (8, 6)), ((17, 12), (17, 12)), ((17, 12), (25, 30)), ((17, 12), (4, 3)), ((1, 5), (5, 16)),
                 ((33, 70), (49, 105))]
BICUBIC_CS = [1, 3, 16]


def bicubic_case(hw, C):
    rng = np.random.RandomState(hw[0] * 31 + hw[1] + C)
    return (rng.randn(2, *hw, C) * 2.0 - 0.5).astype(np.float32)


# ---- the 2-D links -----------------------------------------------------------------------------------------------------
LINK_NCS = [1, 255, 771]                                      # N C
LINK_CS = [1, 3]
SPECIALS = np.asarray([0.0, -0.0, 1.0, np.nextafter(F32(0), F32(1)), -np.nextafter(F32(0), F32(1)),
                       np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), 1e-40, -1e-40, np.inf, -np.inf,
                       FLT_MAX, -FLT_MAX, np.nan, 0.5, -0.25, 1.25], dtype=np.float32)


def link_cases():
    return [(nc // C, C) for nc in LINK_NCS for C in LINK_CS if nc % C == 0]


def link_values(N, C, seed=0):
    """[N, C] float32: the special values first (as many as fit), then uniform in [-0.5, 1.5]"""
    rng = np.random.RandomState(N * 7 + C + seed)
    v = rng.uniform(-0.5, 1.5, N * C).astype(np.float32)
    k = min(v.size, SPECIALS.size)
    v[:k] = SPECIALS[:k] if seed == 0 else np.roll(SPECIALS, seed)[:k]
    if v.size > SPECIALS.size:
        v = v[rng.permutation(v.size)]
    return v.reshape(N, C)


def link_order(N, seed=0):
    return np.random.RandomState(N + 31 + seed).permutation(N).astype(np.int64)


def inside01(v):
    """0 <= v <= 1 (ends and -0.0 included; a NaN is outside)"""
    with np.errstate(invalid="ignore"):
        return (v >= 0) & (v <= 1)


def colour_clamp_gather(var, order=None):
    """fminf(fmaxf(v, 0), 1) through the permutation; a NaN clamps to 0.  The sign of a zero result is defined only
    where it is not the outcome of fmaxf(-0.0, +0.0), which may return either: ``zero_defined`` marks the rest"""
    v = np.asarray(var, dtype=np.float32)
    v = v if order is None else v[order]
    with np.errstate(invalid="ignore"):
        out = np.where(np.isnan(v), F32(0), np.minimum(np.maximum(v, F32(0)), F32(1))).astype(np.float32)
    zero_defined = ~((v == 0) & np.signbit(v))
    return out, zero_defined


def clamp01_bwd(g, x):
    return np.where(inside01(np.asarray(x, np.float32)), np.asarray(g, np.float32), F32(0)).astype(np.float32)


def colour_clamp_scatter_bwd(g_cc, var, order=None):
    var = np.asarray(var, dtype=np.float32)
    out = np.full(var.shape, np.nan, np.float32)
    rows = np.arange(var.shape[0]) if order is None else order
    out[rows] = np.where(inside01(var[rows]), np.asarray(g_cc, np.float32), F32(0))
    return out


def iterate_update(x, g_opt):
    """r = g + (nan_to_num(x) - g) in numpy float32, one rounding per operation"""
    x, g = np.asarray(x, np.float32), np.asarray(g_opt, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.nan_to_num(x, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX).astype(np.float32)
        d = v - g
        return g + d


def iterate_case(n):
    """x with NaN, +-inf, +-FLT_MAX against g_opt of both signs and magnitudes up to FLT_MAX (the difference overflows)"""
    rng = np.random.RandomState(n + 5)
    x = rng.randn(n).astype(np.float32)
    g = rng.randn(n).astype(np.float32)
    sx = np.asarray([np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX, FLT_MAX, np.inf, 0.0, -0.0, 1e-40], np.float32)
    sg = np.asarray([1.0, 2.0, -2.0, -FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -0.0, 0.0, -1e-40], np.float32)
    k = min(n, sx.size)
    x[:k], g[:k] = sx[:k], sg[:k]
    return x, g


def axpy(y, x, a):
    """(y + a x in float64, bound); a as the float32 the kernel receives"""
    y64, x64, a = np.asarray(y, np.float64), np.asarray(x, np.float64), float(np.float32(a))
    return y64 + a * x64, U * (np.abs(a * x64) + np.abs(y64 + a * x64))


# ---- the explicit 2-D warp -----------------------------------------------------------------------------------------------
WARP2D_SHAPES = [(2, 2), (1, 7), (7, 1), (5, 7), (33, 70)]
WARP2D_CS = [1, 3]


def warp2d_case(shape, C):
    """imgs [2, X, Y, C], explicit coordinates [2, 2, X, Y] uniform in [-1.3, 1.3], g like imgs"""
    rng = np.random.RandomState(sum(shape) * 3 + C)
    imgs = (rng.randn(2, *shape, C) * 2.0 - 0.5).astype(np.float32)
    coords = rng.uniform(-1.3, 1.3, (2, 2) + tuple(shape)).astype(np.float32)
    g = rng.randn(2, *shape, C).astype(np.float32)
    return imgs, coords, g

"""The node operations of the Inception-v1 loss network (csrc/inception.hip) restated in float64 numpy -- no torch, no
tiles, no K chunks; layout NHWC, filters HWIO [kh,kw,Ci,Co], TF SAME padding -- the inputs on which float32 arithmetic is
exact, and a worst-case float32 bound for every output element.

Exact inputs.  With integer x, w, gy, bias and y_old (|.| <= 3) every product and every partial sum is a whole number;
``exact_units(S)`` asserts that the sum of |terms| stays below 2^24, so float32 holds each partial sum in whatever order
K chunks, K splits and summed problems add them: the convolution, the small data gradient, the pool adjoint and
relu_mask_add must EQUAL the float64 value.

Bounds (u = 2^-24, one float32 rounding):

  implicit GEMM     1.01 (n + Z + 4) u S + u |y|,  S = sum |x'| |w| (+ |bias| + |y_old|), n = kh kw Cin accumulated
                    products (v_mfma_f32_32x32x2_f32 rounds at most once per accumulated product), Z the partial sums the
                    reduction adds (the K splits of a call, the ztotal of a summed run, 1 without a reduction), 4 = the
                    bias, the accumulate, the store and one to spare.  A summed run: n of its longest problem and the S
                    of all of them (sum_i n_i u S_i <= max n_i u sum_i S_i).
  small data grad   the same with n = (taps that reach the pixel's parity class) x Co fma steps and Z = 1.
  max pool          forward and arg: equal.  Adjoint: at most 9 window terms + the old value are added (9 roundings) and
                    one is to spare: 10 u sum |gy over the <= 9 windows| (+ u |gx_old|).
  avg pool          (k^2 + 2) u sum |x| / k^2: k^2 - 1 adds, the factor 1/k^2 as a float32, the product, one to spare;
                    the adjoint alike over |gy|; accumulated: + u |gx| for that add.
  relu_mask_add     equality with the float32 expression: one IEEE add has one answer.
  LRN forward       1.01 (beta (2 r + 3) + P + 2) u |y|: the window sum has only positive terms, so its absolute sum is
                    the sum itself and 2 r + 1 terms (one product, at most 2 r adds: 2 r + 1 roundings each at most) + the
                    product by alpha + the add of bias make a relative error (2 r + 3) u of scale, which the power
                    carries to y times beta; P ulps for powf, one for the product with x, one to spare.
  LRN adjoint       on the GIVEN y and scale (the kernel's own forward outputs, so that the forward error is not counted
                    twice):  1.01 u ((P + 2) |gy s^-beta| + (2 r + 7) 2 alpha beta |x| sum |gy y / s| + |gx|):
                    first term powf and its product; second: a window term has a product and a quotient and goes through
                    at most 2 r adds (2 r + 2; + 1 to spare), then the products by beta, by x and by the sum and the
                    subtraction (4); |gx| the stored value.  Accumulated: + u |gx + gx_old|, one more add.

P, the allowance of the device powf in ulps: no accuracy table of the HIP math library is installed beside the
compiler this suite is built with, so P = 4 (the HIP documentation lists fewer).  It is not fitted to any output.

The LRN bounds against rounding alone: a plain float32 numpy restatement (``lrn32``, ``lrn_bwd32``: numpy's float32
power in place of the device's) sits at 0.17 - 0.31 (forward) and 0.26 - 0.40 (adjoint) of them on the five parameter
sets of the GPU test (tests/test_inception_ref_cpu.py asserts < 0.5), and a dropped window term exceeds them by more
than 10^3.
"""
import numpy as np

from tests.conv_ref import exact_units, int_tensor  # noqa: F401  (re-exported)
from tests.loss_ref import LIMIT, U, err_ratio, f64, is_f32, units  # noqa: F401  (re-exported)

P_POWF = 4
_f = np.float32


# ---- the operations ------------------------------------------------------------------------------------------------------
def same(n, k, stride):
    """TF SAME: (output size, padding before)"""
    out = -(-n // stride)
    return out, max((out - 1) * stride + k - n, 0) // 2


def _geometry(H, W, kh, kw, stride):
    Ho, pt = same(H, kh, stride)
    Wo, pl = same(W, kw, stride)
    # the padded extent that holds every tap of every output
    Hp, Wp = max((Ho - 1) * stride + kh, pt + H), max((Wo - 1) * stride + kw, pl + W)
    return Ho, Wo, pt, pl, Hp, Wp


def _padded(x, pt, pl, Hp, Wp, value=0.0):
    B, H, W, C = x.shape
    xp = np.full((B, Hp, Wp, C), value, np.float64)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp


def conv2d(x, w, bias=None, stride=1, mask=None, relu=False, y_old=None):
    """(pre, y, S): pre = sum x'[oy s + dy - pt, ox s + dx - pl, ci] w[dy, dx, ci, co] + bias with x' = x (mask > 0),
    y = relu?(pre) + y_old, S = sum |x'| |w| + |bias| + |y_old|"""
    x, w = f64(x), f64(w)
    if mask is not None:
        x = x * (f64(mask) > 0)
    kh, kw = w.shape[:2]
    B, H, W, _ = x.shape
    Ho, Wo, pt, pl, Hp, Wp = _geometry(H, W, kh, kw, stride)
    xp, ap, aw = _padded(x, pt, pl, Hp, Wp), _padded(np.abs(x), pt, pl, Hp, Wp), np.abs(w)
    pre = np.zeros((B, Ho, Wo, w.shape[3]))
    S = np.zeros_like(pre)
    for dy in range(kh):
        for dx in range(kw):
            ys, xs = slice(dy, dy + (Ho - 1) * stride + 1, stride), slice(dx, dx + (Wo - 1) * stride + 1, stride)
            pre += xp[:, ys, xs] @ w[dy, dx]
            S += ap[:, ys, xs] @ aw[dy, dx]
    if bias is not None:
        pre = pre + f64(bias)
        S = S + np.abs(f64(bias))
    y = np.maximum(pre, 0.0) if relu else pre
    if y_old is not None:
        y = y + f64(y_old)
        S = S + np.abs(f64(y_old))
    return pre, y, S


def conv2d_dgrad(gy, w, in_hw, stride=1, act=None):
    """(gx [B,H,W,Ci], S): the adjoint of conv2d wrt x as a sum over OUTPUT pixels -- output (oy, ox) hands
    sum_co g'[oy, ox, co] w[dy, dx, ci, co] to input (oy s + dy - pt, ox s + dx - pl) -- with g' = gy (act > 0);
    S the same sum over |terms|"""
    gy, w = f64(gy), f64(w)
    if act is not None:
        gy = gy * (f64(act) > 0)
    kh, kw = w.shape[:2]
    H, W = in_hw
    B, Ho, Wo, _ = gy.shape
    Ho_, Wo_, pt, pl, Hp, Wp = _geometry(H, W, kh, kw, stride)
    assert (Ho, Wo) == (Ho_, Wo_)
    gp, sp = np.zeros((B, Hp, Wp, w.shape[2])), np.zeros((B, Hp, Wp, w.shape[2]))
    ag, aw = np.abs(gy), np.abs(w)
    for dy in range(kh):
        for dx in range(kw):
            ys, xs = slice(dy, dy + (Ho - 1) * stride + 1, stride), slice(dx, dx + (Wo - 1) * stride + 1, stride)
            gp[:, ys, xs] += gy @ w[dy, dx].T
            sp[:, ys, xs] += ag @ aw[dy, dx].T
    return gp[:, pt:pt + H, pl:pl + W].copy(), sp[:, pt:pt + H, pl:pl + W].copy()


def dgrad_taps(in_hw, kh, kw, stride):
    """[H,W]: the taps (dy, dx) that reach a pixel's parity class -- dy = (iy + pt) mod s, + s, ... < kh"""
    H, W = in_hw
    pt, pl = same(H, kh, stride)[1], same(W, kw, stride)[1]
    ny = np.array([len(range((iy + pt) % stride, kh, stride)) for iy in range(H)])
    nx = np.array([len(range((ix + pl) % stride, kw, stride)) for ix in range(W)])
    return ny[:, None] * nx[None, :]


def maxpool3(x, stride):
    """(y, arg uint8): 3x3 SAME max pool; arg = the row-major window position 0..8 of the FIRST maximum among the
    in-range taps (padding taps do not take part)"""
    x = f64(x)
    B, H, W, C = x.shape
    Ho, Wo, pt, pl, Hp, Wp = _geometry(H, W, 3, 3, stride)
    xp = _padded(x, pt, pl, Hp, Wp, -np.inf)
    y = np.full((B, Ho, Wo, C), -np.inf)
    arg = np.zeros((B, Ho, Wo, C), np.uint8)
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        v = xp[:, dy:dy + (Ho - 1) * stride + 1:stride, dx:dx + (Wo - 1) * stride + 1:stride]
        better = v > y
        y = np.where(better, v, y)
        arg[better] = tap
    return y, arg


def maxpool3_bwd(gy, arg, in_hw, stride, gx_old=None, relu_of=None):
    """(gx, S): every output hands gy to the input its arg names; gx = (gx_old + that) (relu_of > 0);
    S = sum |gy| over the windows that contain the pixel, whatever their arg"""
    gy = f64(gy)
    H, W = in_hw
    B, Ho, Wo, C = gy.shape
    _, _, pt, pl, Hp, Wp = _geometry(H, W, 3, 3, stride)
    gp, sp = np.zeros((B, Hp, Wp, C)), np.zeros((B, Hp, Wp, C))
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        ys, xs = slice(dy, dy + (Ho - 1) * stride + 1, stride), slice(dx, dx + (Wo - 1) * stride + 1, stride)
        gp[:, ys, xs] += gy * (arg == tap)
        sp[:, ys, xs] += np.abs(gy)
    gx, S = gp[:, pt:pt + H, pl:pl + W].copy(), sp[:, pt:pt + H, pl:pl + W].copy()
    if gx_old is not None:
        gx = gx + f64(gx_old)
    if relu_of is not None:
        gx = gx * (f64(relu_of) > 0)
    return gx, S


def lrn_params(bias, alpha, beta):
    """as the kernel receives them: float32"""
    return float(_f(bias)), float(_f(alpha)), float(_f(beta))


def _window(v, r):
    """sum_{|j - c| <= r, 0 <= j < C} v_j along the last axis"""
    C = v.shape[-1]
    out = np.zeros_like(v)
    for c in range(C):
        out[..., c] = v[..., max(c - r, 0):min(c + r, C - 1) + 1].sum(axis=-1)
    return out


def lrn(x, r, bias, alpha, beta):
    """(y, scale): scale = bias + alpha sum_{|j-c| <= r} x_j^2, y = x scale^-beta"""
    x = f64(x)
    bias, alpha, beta = lrn_params(bias, alpha, beta)
    scale = bias + alpha * _window(x * x, r)
    return x * scale ** -beta, scale


def lrn_bwd(x, y, scale, gy, r, alpha, beta, gx_old=None):
    """(gx, bound) from the GIVEN y and scale: gx_c = gy_c s_c^-beta - 2 alpha beta x_c sum_{|j-c| <= r} gy_j y_j / s_j
    (+ gx_old)"""
    x, y, scale, gy = f64(x), f64(y), f64(scale), f64(gy)
    _, alpha, beta = lrn_params(0.0, alpha, beta)
    first = gy * scale ** -beta
    gx = first - 2.0 * alpha * beta * x * _window(gy * y / scale, r)
    mag = 2.0 * alpha * beta * np.abs(x) * _window(np.abs(gy * y / scale), r)
    bound = 1.01 * U * ((P_POWF + 2) * np.abs(first) + (2 * r + 7) * mag + np.abs(gx))
    if gx_old is not None:
        gx = gx + f64(gx_old)
        bound = bound + U * np.abs(gx)
    return gx, bound


def lrn_bound(y, r, beta):
    return 1.01 * (float(_f(beta)) * (2 * r + 3) + P_POWF + 2) * U * np.abs(f64(y))


def avgpool_valid(x, k):
    """(y, S = sum |x| over the window): k x k, stride 1, VALID"""
    x = f64(x)
    B, H, W, C = x.shape
    Ho, Wo = H - k + 1, W - k + 1
    y, S = np.zeros((B, Ho, Wo, C)), np.zeros((B, Ho, Wo, C))
    for dy in range(k):
        for dx in range(k):
            y += x[:, dy:dy + Ho, dx:dx + Wo]
            S += np.abs(x[:, dy:dy + Ho, dx:dx + Wo])
    return y / (k * k), S


def avgpool_valid_bwd(gy, in_hw, k, gx_old=None):
    """(gx, S = sum |gy| over the windows that contain the pixel): the adjoint, as a sum over outputs"""
    gy = f64(gy)
    H, W = in_hw
    B, Ho, Wo, C = gy.shape
    gx, S = np.zeros((B, H, W, C)), np.zeros((B, H, W, C))
    for dy in range(k):
        for dx in range(k):
            gx[:, dy:dy + Ho, dx:dx + Wo] += gy
            S[:, dy:dy + Ho, dx:dx + Wo] += np.abs(gy)
    gx = gx / (k * k)
    if gx_old is not None:
        gx = gx + f64(gx_old)
    return gx, S


def relu_mask_add(g, act, addend):
    """out = g (act > 0) + addend in float32 (each operand may be None); float32 out"""
    if g is None:
        return np.asarray(addend, _f).copy()
    v = np.asarray(g, _f)
    if act is not None:
        v = np.where(np.asarray(act, _f) > 0, v, _f(0.0)).astype(_f)
    return v + np.asarray(addend, _f) if addend is not None else v.copy()


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def gemm_bound(S, n, Z, y):
    """n accumulated products (a number, or an array per pixel [.., H, W, 1]), Z partial sums"""
    return 1.01 * (f64(n) + Z + 4) * U * f64(S) + U * np.abs(f64(y))


def ratio(got, ref, bound):
    """largest |got - ref| / bound over the elements (loss_ref.err_ratio: inf where an error meets a zero bound or is
    not a number)"""
    return err_ratio(np.abs(f64(got) - f64(ref)), bound)


def maxpool_bwd_bound(S, gx_old=None):
    return 10.0 * U * f64(S) + (0.0 if gx_old is None else U * np.abs(f64(gx_old)))


def avgpool_bound(S, k, gx_acc=None):
    return (k * k + 2) * U * f64(S) / (k * k) + (0.0 if gx_acc is None else U * np.abs(f64(gx_acc)))


# ---- the float32 restatement of LRN (what rounding alone does) ---------------------------------------------------------------
def lrn32(x, r, bias, alpha, beta):
    x = np.asarray(x, _f)
    C = x.shape[-1]
    s = np.zeros_like(x)
    for c in range(C):
        for j in range(max(c - r, 0), min(c + r, C - 1) + 1):
            s[..., c] += x[..., j] * x[..., j]
    s = _f(bias) + _f(alpha) * s
    return x * np.power(s, -_f(beta)), s


def lrn_bwd32(x, y, scale, gy, r, alpha, beta):
    x, y, scale, gy = (np.asarray(a, _f) for a in (x, y, scale, gy))
    C = x.shape[-1]
    s = np.zeros_like(x)
    for c in range(C):
        for j in range(max(c - r, 0), min(c + r, C - 1) + 1):
            s[..., c] += gy[..., j] * y[..., j] / scale[..., j]
    return gy * np.power(scale, -_f(beta)) - _f(2.0) * _f(alpha) * _f(beta) * x * s


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def realistic(B, H, W, Ci, Co, kh, kw, seed, bias_std=10.0):
    """post-ReLU-like activations max(randn, 0) * 30, He-scaled filters, a bias of standard deviation 10, float32"""
    rng = np.random.RandomState(seed)
    x = np.maximum(rng.randn(B, H, W, Ci), 0.0).astype(_f) * _f(30.0)
    w = (rng.randn(kh, kw, Ci, Co) * np.sqrt(2.0 / (kh * kw * Ci))).astype(_f)
    bias = (rng.randn(Co) * bias_std).astype(_f)
    return x, w, bias


def mask_tensor(shape, seed):
    """a ReLU mask operand: exact zeros (+0 and -0), negative and positive values, a third each"""
    rng = np.random.RandomState(seed)
    m = rng.randn(*shape).astype(_f)
    z = rng.rand(*shape)
    m[z < 0.33] = 0.0
    m[z < 0.16] = -0.0
    return m


def conv_inputs(case, exact, seed_shift=0):
    """the inputs of a convolution case (kh, kw, stride, Ci, Co, B, H, W): x, w, bias, y_old [B,Ho,Wo,Co]"""
    kh, kw, stride, Ci, Co, B, H, W = case
    seed = (kh * 7919 + kw * 104729 + stride * 31 + Ci * 1009 + Co * 17 + B * 5 + H * 131 + W + seed_shift) % (2 ** 31)
    Ho, Wo = same(H, kh, stride)[0], same(W, kw, stride)[0]
    if exact:
        return dict(x=int_tensor((B, H, W, Ci), seed), w=int_tensor((kh, kw, Ci, Co), seed + 1),
                    bias=int_tensor((Co,), seed + 2), y_old=int_tensor((B, Ho, Wo, Co), seed + 3))
    x, w, bias = realistic(B, H, W, Ci, Co, kh, kw, seed)
    y_old = (np.random.RandomState(seed + 3).randn(B, Ho, Wo, Co) * 20).astype(_f)
    return dict(x=x, w=w, bias=bias, y_old=y_old)


# ---- reading a mismatch --------------------------------------------------------------------------------------------------
def decode(flat, shape, bm=64):
    """flat index into [B,Ho,Wo,C] -> 'image b at (oy, ox) channel c -- row r of m-tile t, column tile n' for tiles of
    bm rows x 64 columns"""
    b, oy, ox, c = np.unravel_index(int(flat), shape)
    m = (b * shape[1] + oy) * shape[2] + ox
    return "image %d at (%d, %d) channel %d -- row %d of m-tile %d, column tile %d" % (b, oy, ox, c, m % bm, m // bm,
                                                                                        c // 64)


def first_mismatches(got, ref, bound, bm=64, n=5):
    """a report of the first n entries where |got - ref| > bound (or got is not a number), decoded; '' when none.
    bound 0: equality"""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = ~(np.abs(got - ref) <= f64(bound))
    idx = np.flatnonzero(bad)
    if idx.size == 0:
        return ""
    bb = np.broadcast_to(f64(bound), ref.shape).reshape(-1)
    lines = ["%d of %d entries outside the bound; the first:" % (idx.size, bad.size)]
    for i in idx[:n]:
        lines.append("  %s: got %r, reference %r, bound %.3g" % (decode(i, ref.shape, bm), got.reshape(-1)[i],
                                                                 ref.reshape(-1)[i], bb[i]))
    return "\n".join(lines)


# ---- the cases of tests/test_inception_nodes_gpu.py (tests/test_inception_ref_cpu.py holds them to their conditions) ---------
# (kh, kw, stride, Cin, Cout, B, H, W) -> what ops.conv2d_plan must report: bm, cmode, ksplit, cps and ``last``, the chunks of
# the last split
CONV_CASES = [
    # 128-row tile, CMODE 0: M = 8385 = 65 tiles + 65 rows (the last tile's second row-half holds one row); one chunk
    ((1, 1, 1, 8, 512, 1, 129, 65), dict(bm=128, cmode=0, ksplit=1, cps=1, last=1)),
    # 128-row tile, CMODE 1: 3 chunks of 4 taps, the last one partial
    ((3, 3, 1, 3, 512, 1, 129, 65), dict(bm=128, cmode=1, ksplit=1, cps=3, last=3)),
    # 128-row tile, CMODE 1, 13 chunks
    ((7, 7, 1, 3, 1024, 1, 64, 65), dict(bm=128, cmode=1, ksplit=1, cps=13, last=13)),
    # 16 splits of 10 chunks, cchunks 17: every split after the first starts in the middle of a tap; the last has 3
    ((3, 3, 1, 272, 64, 1, 9, 8), dict(bm=64, cmode=0, ksplit=16, cps=10, last=3, cchunks=17)),
    # partial chunk (36 = 2 x 16 + 4), Cout < 64, 9 splits of 9 (odd), the last of 3
    ((5, 5, 1, 36, 8, 1, 5, 4), dict(bm=64, cmode=0, ksplit=9, cps=9, last=3, cchunks=3)),
    # 6 splits of 9, the last of 7; a single pixel
    ((1, 1, 1, 832, 384, 1, 1, 1), dict(bm=64, cmode=0, ksplit=6, cps=9, last=7)),
    # the classifier: 8 splits of 8 (even cps), Cout no multiple of 64
    ((1, 1, 1, 1024, 1008, 1, 2, 2), dict(bm=64, cmode=0, ksplit=8, cps=8, last=8)),
    # 2 splits; also run without a workspace (one block per tile)
    ((3, 3, 1, 32, 64, 1, 6, 6), dict(bm=64, cmode=0, ksplit=2, cps=9, last=9)),
    # partial chunk with 4 live channels, Cout = 64 + 4, images wrap inside one tile
    ((3, 3, 1, 20, 68, 2, 6, 7), dict(bm=64, cmode=0, ksplit=2, cps=9, last=9, cchunks=2)),
    # kh != kw, Cout = 4
    ((1, 3, 1, 24, 4, 1, 7, 9), dict(bm=64, cmode=0, ksplit=1, cps=6, last=6)),
    ((3, 1, 1, 24, 4, 1, 7, 9), dict(bm=64, cmode=0, ksplit=1, cps=6, last=6)),
    # stride 2, odd and even sides
    ((3, 3, 2, 16, 64, 2, 5, 6), dict(bm=64, cmode=0, ksplit=1, cps=9, last=9)),
    ((3, 3, 2, 16, 64, 2, 6, 5), dict(bm=64, cmode=0, ksplit=1, cps=9, last=9)),
    # the first layer; an image smaller than the filter
    ((7, 7, 2, 3, 64, 2, 21, 30), dict(bm=64, cmode=1, ksplit=1, cps=13, last=13)),
    ((7, 7, 2, 3, 64, 1, 1, 1), dict(bm=64, cmode=1, ksplit=1, cps=13, last=13)),
]
NO_WORKSPACE_CASE = (3, 3, 1, 32, 64, 1, 6, 6)


def case_id(case):
    return "k%dx%d-s%d-%dto%d-b%d-%dx%d" % tuple(case)


def has_dgrad_form(case):
    """the data-gradient form (x_mask, filters packed transposed) is run for stride-1 cases with Cin > 4"""
    return case[2] == 1 and case[3] > 4


def dgrad_case(case):
    """the data-gradient form of a case as the kernel sees it: Cin and Cout swapped (both multiples of 4)"""
    kh, kw, stride, Ci, Co, B, H, W = case
    return (kh, kw, 1, Co, Ci, B, H, W)


# grouped launches: B, [(k, Cin, Cout, H, W, sum_with_prev)]; GROUP_PLANS: what nfs_conv2d_group_plan must report per problem
# as (ksplit, cps, partial, zbase, ztotal, position in the launch order)
GROUPS = {
    # a module's forward pair at B = 2, 7 x 9: the three 1x1 convolutions on the module input ...
    "fwd_1x1": (2, [(1, 192, 64, 7, 9, 0), (1, 192, 96, 7, 9, 0), (1, 192, 16, 7, 9, 0)]),
    # ... then 5x5, the pool projection and 3x3, listed shortest blocks first so that the launch reorders them
    "fwd_5x5_pool_3x3": (2, [(5, 16, 32, 7, 9, 0), (1, 192, 32, 7, 9, 0), (3, 96, 128, 7, 9, 0)]),
    # a summed run with unequal splits: the 1x1 data gradients of a module into one y.  The run's first problem is not its
    # longest: the launch puts the 208-channel problem first, the reduction keeps the listed order (zbase)
    "summed": (2, [(1, 96, 192, 7, 9, 0), (1, 208, 192, 7, 9, 1), (1, 16, 192, 7, 9, 1)]),
    # the full table: six problems at 3 x 3 pixels, k = 1, 3, 5, up to 16 splits
    "six": (1, [(1, 528, 256, 3, 3, 0), (3, 160, 320, 3, 3, 0), (5, 32, 128, 3, 3, 0), (1, 528, 128, 3, 3, 0),
                (3, 320, 16, 3, 3, 0), (5, 128, 32, 3, 3, 0)]),
    # different H x W; the second problem is not split: its tiles write y themselves
    "two_sizes": (2, [(3, 32, 64, 5, 6, 0), (1, 64, 32, 9, 4, 0)]),
    # many m tiles (263 x 2 blocks), no split
    "one_large": (4, [(3, 16, 128, 70, 60, 0)]),
}
GROUP_PLANS = {
    "fwd_1x1": [(2, 6, 1, 0, 2, 0), (2, 6, 1, 0, 2, 1), (2, 6, 1, 0, 2, 2)],
    "fwd_5x5_pool_3x3": [(4, 7, 1, 0, 4, 1), (2, 6, 1, 0, 2, 2), (7, 8, 1, 0, 7, 0)],
    "summed": [(1, 6, 1, 0, 4, 1), (2, 7, 1, 1, 4, 0), (1, 1, 1, 3, 4, 2)],
    "six": [(5, 7, 1, 0, 5, 4), (12, 8, 1, 0, 12, 2), (7, 8, 1, 0, 7, 3), (5, 7, 1, 0, 5, 5), (15, 12, 1, 0, 15, 1),
            (16, 13, 1, 0, 16, 0)],
    "two_sizes": [(3, 6, 1, 0, 3, 0), (1, 4, 0, 0, 1, 1)],
    "one_large": [(1, 9, 0, 0, 1, 0)],
}

# nfs_conv2d_dgrad_small: (kh, kw, stride, Ci, Co, B, H, W, masked) per family, and the kernel the family must reach
# ("lds": stride 2 and Co <= 64; "generic" otherwise)
def _small(filters, stride, cis, cos, images):
    return [(kh, kw, stride, ci, co, 2, H, W, masked) for (kh, kw) in filters for ci in cis for co in cos
            for (H, W) in images for masked in (True, False)]


SMALL_DGRAD = {
    # one tile exactly, tiles of one pixel row, ragged tiles, images smaller than a filter
    "lds": _small([(7, 7), (5, 5), (3, 3), (7, 3)], 2, (1, 2, 3, 4), (4, 36, 64),
                  [(16, 16), (17, 33), (15, 31), (2, 3), (1, 1)]),
    # Co > 64 at stride 2: the four parity classes of the generic kernel
    "generic_s2": _small([(7, 7)], 2, (3, 4), (68, 128), [(21, 30), (16, 17), (2, 2), (1, 1)]),
    "generic_s1": _small([(7, 7), (3, 3)], 1, (1, 2, 3, 4), (36,), [(13, 8), (1, 1)]),
}


def small_dgrad_kernel(case):
    """which kernel nfs_conv2d_dgrad_small takes (its own rule: stride 2 and Co <= 64 -> the LDS kernel)"""
    return "lds" if case[2] == 2 and case[4] <= 64 else "generic"


def small_dgrad_inputs(case, exact):
    kh, kw, stride, Ci, Co, B, H, W, masked = case
    seed = (kh * 7 + kw * 13 + stride * 3 + Ci * 101 + Co * 11 + H * 1009 + W * 37 + B) % (2 ** 31)
    Ho, Wo = same(H, kh, stride)[0], same(W, kw, stride)[0]
    if exact:
        gy, w = int_tensor((B, Ho, Wo, Co), seed), int_tensor((kh, kw, Ci, Co), seed + 1)
    else:
        rng = np.random.RandomState(seed)
        gy = rng.randn(B, Ho, Wo, Co).astype(_f)
        w = (rng.randn(kh, kw, Ci, Co) * np.sqrt(2.0 / (kh * kw * Ci))).astype(_f)
    act = mask_tensor((B, Ho, Wo, Co), seed + 2) if masked else None
    return gy, w, act


POOL_SHAPES = [(9, 12), (10, 11), (1, 7), (7, 1), (2, 3), (1, 1)]
POOL_CHANNELS = [4, 8, 64]
AVGPOOL_CASES = [(7, 7, 7), (7, 7, 8), (3, 10, 15), (1, 4, 5)]          # (k, H, W)
# (C, ld, r, bias, alpha, beta): the three sets of tests/test_inception_gpu.py, a window wider than the row, no window
LRN_CASES = [(64, 64, 5, 2.0, 1e-4, 0.5), (192, 192, 5, 2.0, 1e-4, 0.5), (24, 64, 2, 1.0, 2e-2, 0.75),
             (4, 8, 5, 2.0, 1e-4, 0.5), (16, 20, 0, 1.0, 2e-2, 0.75)]


def lrn_inputs(C, seed=None):
    rng = np.random.RandomState(C if seed is None else seed)
    return (rng.randn(2, 5, 6, C) * 30).astype(_f), rng.randn(2, 5, 6, C).astype(_f)


def tie_tensor(shape, seed):
    """integers in {0, 1, 2} after a ReLU-like clip: most windows hold their maximum more than once"""
    return np.clip(np.random.RandomState(seed).randint(-2, 3, size=shape), 0, 2).astype(_f)


def placeholder_descs(ConvDesc, problems, masks=False):
    """a descriptor array for nfs_conv2d_group_plan, which reads shapes and checks pointers for null and alignment but
    follows none: the addresses are placeholders (a summed problem shares the y of the one before it)"""
    arr = (ConvDesc * len(problems))()
    for j, (q, (k, ci, co, H, W, summed)) in enumerate(zip(arr, problems)):
        q.x, q.packed, q.y = 4096 * (3 * j + 1), 4096 * (3 * j + 2), arr[j - 1].y if summed else 4096 * (3 * j + 3)
        q.ldx, q.ldy, q.H, q.W, q.Cin, q.Cout, q.kh, q.kw = ci, co, H, W, ci, co, k, k
        q.sum_with_prev = summed
    return arr


# what each problem of a group carries: b bias, r ReLU, p y_pre, a accumulate onto a non-zero y, m x_mask, d the
# data-gradient form (filters packed transposed: the reference is conv2d_dgrad).  A follower of a summed run carries
# neither b, r nor p (the planner refuses them) and its a is ignored.
GROUP_FLAGS = {
    "fwd_1x1": ["brp", "br", "br"],
    "fwd_5x5_pool_3x3": ["br", "brp", "br"],
    "summed": ["dm", "dm", "dm"],
    "six": ["brp", "br", "a", "dm", "bra", "p"],
    "two_sizes": ["br", "dma"],
    "one_large": ["brp"],
}


def group_problems(name, exact, accumulate_first=False):
    """the problems of a group with their inputs: dicts k, Ci, Co (of the kernel's GEMM), H, W, summed, flags, x, w (HWIO
    as packed: [k,k,Ci,Co], or [k,k,Co,Ci] packed transposed for the d form), bias, mask, y_old"""
    B, shapes = GROUPS[name]
    out = []
    for j, ((k, ci, co, H, W, summed), flags) in enumerate(zip(shapes, GROUP_FLAGS[name])):
        if accumulate_first and j == 0:
            flags = flags + "a"
        seed = (sum(ord(c) for c in name) * 131 + j * 7 + (1 if exact else 0)) % (2 ** 31)
        wshape = (k, k, co, ci) if "d" in flags else (k, k, ci, co)
        if exact:
            x, w, bias = int_tensor((B, H, W, ci), seed), int_tensor(wshape, seed + 1), int_tensor((co,), seed + 2)
            y_old = int_tensor((B, H, W, co), seed + 3)
        else:
            x, _, bias = realistic(B, H, W, ci, co, k, k, seed)
            w = (np.random.RandomState(seed + 1).randn(*wshape) * np.sqrt(2.0 / (k * k * ci))).astype(_f)
            y_old = (np.random.RandomState(seed + 3).randn(B, H, W, co) * 20).astype(_f)
        out.append(dict(k=k, Ci=ci, Co=co, H=H, W=W, summed=bool(summed), flags=flags, x=x, w=w,
                        bias=bias if "b" in flags else None,
                        mask=mask_tensor((B, H, W, ci), seed + 4) if "m" in flags else None,
                        y_old=y_old if "a" in flags else None))
    return out


def group_runs(problems):
    """[[indices of a run]]: a problem and the summed problems behind it"""
    runs = []
    for j, pr in enumerate(problems):
        if pr["summed"]:
            runs[-1].append(j)
        else:
            runs.append([j])
    return runs


def run_reference(problems, run):
    """(pre, y, S, n) of a run: the sum of its problems' convolutions finished by the epilogue of the FIRST"""
    lin, S = 0.0, 0.0
    for j in run:
        pr = problems[j]
        if "d" in pr["flags"]:
            v, s = conv2d_dgrad(pr["x"], pr["w"], (pr["H"], pr["W"]), 1, act=pr["mask"])
        else:
            v, _, s = conv2d(pr["x"], pr["w"], None, 1, mask=pr["mask"])
        lin, S = lin + v, S + s
    first = problems[run[0]]
    pre = lin
    if first["bias"] is not None:
        pre, S = pre + f64(first["bias"]), S + np.abs(f64(first["bias"]))
    y = np.maximum(pre, 0.0) if "r" in first["flags"] else pre
    if first["y_old"] is not None:
        y, S = y + f64(first["y_old"]), S + np.abs(f64(first["y_old"]))
    return pre, y, S, max(problems[j]["k"] ** 2 * problems[j]["Ci"] for j in run)


WAYS = ("bias_relu_pre", "accumulate", "dgrad")


def conv_reference(case, exact, way):
    """inputs and float64 reference of one way to run a convolution case:
         bias_relu_pre  y = relu(conv(x) + bias), y_pre = the value before the ReLU
         accumulate     y = y_old + conv(x): no bias, no ReLU
         dgrad          the data gradient of the case's convolution, gx = sum gy (act > 0) w, which the kernel runs as a
                        convolution of gy [B,H,W,Co] with the filters packed transposed (K = kh kw Co); the mask needs
                        more than 4 channels
       -> dict x | gy, w, bias, y_old, mask, pre, y, S, n (accumulated products), kernel (the case as the kernel sees it)"""
    kh, kw, stride, Ci, Co, B, H, W = case
    d = conv_inputs(case, exact)
    if way == "dgrad":
        assert has_dgrad_form(case)
        seed = Ci * 31 + Co * 7 + H + (1 if exact else 0)
        gy = int_tensor((B, H, W, Co), seed) if exact else np.random.RandomState(seed).randn(B, H, W, Co).astype(_f)
        mask = mask_tensor((B, H, W, Co), seed + 1) if Co > 4 else None
        gx, S = conv2d_dgrad(gy, d["w"], (H, W), 1, act=mask)
        return dict(gy=gy, w=d["w"], mask=mask, pre=gx, y=gx, S=S, n=kh * kw * Co, kernel=dgrad_case(case))
    if way == "bias_relu_pre":
        pre, y, S = conv2d(d["x"], d["w"], d["bias"], stride, relu=True)
        d["y_old"] = None
    else:
        pre, y, S = conv2d(d["x"], d["w"], None, stride, y_old=d["y_old"])
        d["bias"] = None
    d.update(pre=pre, y=y, S=S, n=kh * kw * Ci, kernel=case, mask=None)
    return d

"""tests/seam_ref.py pinned without a GPU: (1) every restatement against the float64 oracle (autograd for the adjoints):
to 1e-12 per element where the float32 coordinates of the contract are the exact rationals, elsewhere within the
coordinate term the bound states; (2) the bounds are not too tight: a straight numpy float32 emulation of every kernel,
one rounding per operation and no FMA, in the kernel's own summation order, stays at err / bound <= 1 on every case the
GPU test runs (and EQUALS the reference on the exact cases); (3) not too loose: planted defects in that emulation each
leave a bound (or break bit equality) on at least one listed case; (4) the preconditions: the ``units`` of the exact
cases, the floor agreement of the bilinear coordinate, the tie margin of the bicubic table index, the cap on the share
of pixels with the two-candidate latitude of the 2-D warp's coordinate gradient.

Largest err / bound of the honest float32 emulation per operator (each test prints its own):
    K5 / K5f adjoint 1.00 (the half-ulp of g / m on every element: tight by nature), 0.08 / 0.04 on the maxima
    A5 resized d_img 0.41  x 0.51  g_img 0.13; at the image's own size 0.95  0.90  0.98 (one or two roundings: tight)
    K24 0.25   axpy 0.94   warp2d (float32 oracle) fwd 0.14  g_imgs 0.15  g_coords 0.15"""
import math

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import field_ref as FR
from tests import seam_ref as S

U, F32 = S.U, np.float32


def _id(c):
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)


# ---- K5 / K5f ----------------------------------------------------------------------------------------------------------
def _sum32(p, two_phase, drop=None):
    """sum of p (float32 [n]) in the kernel's order: the strided chain of every thread, the xor butterfly of every wave,
    the serial sum over a block's waves and (two-phase) over the 32 partials"""
    p = np.asarray(p, np.float32).copy()
    if drop is not None:
        p[drop] = 0
    T, nw = (256 * S.MN_NB, 4) if two_phase else (1024, 16)
    L = math.ceil(p.size / T)
    a = np.zeros(L * T, np.float32)
    a[:p.size] = p
    a = a.reshape(L, T)
    acc = np.zeros(T, np.float32)
    for l in range(L):
        acc = acc + a[l]
    w = acc.reshape(-1, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lanes ^ o]
    blocks = w[:, 0].reshape(-1, nw)
    r = np.zeros(blocks.shape[0], np.float32)
    for i in range(nw):
        r = r + blocks[:, i]
    s = F32(0)
    for k in range(r.size):
        s = s + r[k]
    assert isinstance(s, np.float32) or s.dtype == np.float32
    return F32(s)


def emu_maxnorm_max(x, defect=None):
    x = np.asarray(x, np.float32)
    n = x.shape[1]
    if defect == "tail":                                    # the first tail element of the float4 walk left out
        keep = np.ones(n, bool)
        keep[min(4 * (n // 4), n - 1)] = n == 1
        return x[:, keep].max(axis=1)
    if defect == "magnitude":
        return np.abs(x).max(axis=1)
    return x.max(axis=1)


def emu_maxnorm_bwd(x, g, two_phase, defect=None):
    x, g = np.asarray(x, np.float32), np.asarray(g, np.float32)
    out = np.empty_like(x)
    for j in range(x.shape[0]):
        m = x[j].max()
        tie = x[j] == m
        ties = F32(tie.sum() + (1 if defect == "ties" else 0))
        s = _sum32(x[j] * g[j], two_phase, drop=(x.shape[1] // 2 if defect == "drop" else None))
        corr = s / (m * m) / ties
        gi = g[j] / m
        out[j] = np.where(tie | (defect == "all"), gi - corr, gi)
    assert out.dtype == np.float32
    return out


def _forms(n, fused):
    """(two_phase) of every launch form the GPU test takes for this n"""
    if fused:
        return [True]
    return [True, False] if n >= S.MN_MULTI else [False]


def _maxnorm_sweep(fused, defect=None, exact=False):
    """largest err / bound of the emulated adjoint over all cases and variants, (over every element, over the elements
    that hold a maximum); exact: the number of unequal elements"""
    worst, worst_tie = 0.0, 0.0
    for G, n in S.MAXNORM_CASES:
        for v in range(len(S.maxnorm_variants(n))):
            x, _ = S.maxnorm_case(G, n, v, exact=exact)
            if fused:
                g = S.grad_input(S.maxnorm_grad(G, n, v, exact=exact, channels=3))
            else:
                g = S.maxnorm_grad(G, n, v, exact=exact)
            for two in _forms(n, fused):
                ref, bound = S.maxnorm_adjoint(x, g, two)
                got = emu_maxnorm_bwd(x, g, two, defect).astype(np.float64)
                if exact:
                    worst = max(worst, float((got != ref).sum()))
                else:
                    tie = x == x.max(1, keepdims=True)
                    worst = max(worst, S.err_ratio(np.abs(got - ref), bound))
                    worst_tie = max(worst_tie, S.err_ratio(np.abs(got - ref)[tie], bound[tie]))
    return worst if exact else (worst, worst_tie)


def test_maxnorm_cases_are_what_they_claim():
    """the planted maximum is the group's only maximum (or its 2 / 4 ties), sits where it was planted, mixed groups have
    blocks of the 32-block walk that see only negative values and others that see the maximum, and no group has a zero
    maximum or a NaN"""
    for G, n in S.MAXNORM_CASES:
        seen = set()
        for v, plants in enumerate(S.maxnorm_variants(n)):
            x, signs = S.maxnorm_case(G, n, v)
            seen.update(signs)
            assert np.isfinite(x).all() and (x.max(1) != 0).all()
            for j in range(G):
                assert sorted(np.flatnonzero(x[j] == x[j].max())) == sorted(plants)
                if signs[j] == "mixed" and n >= S.MN_MULTI:
                    blk = (np.arange(n) // 256) % S.MN_NB
                    bmax = np.asarray([x[j][blk == b].max() for b in range(S.MN_NB)])
                    assert (bmax < 0).sum() >= 8 and (bmax > 0).sum() >= 8
                if signs[j] == "mixed" and n > 5:
                    assert np.abs(x[j]).max() > x[j].max() > 0
            if len(plants) == 4 and n >= S.MN_MULTI:
                assert len({(p // 256) % S.MN_NB for p in plants}) == 4
        if n >= 5:
            assert seen == set(S.SIGNS)
    x, signs = S.maxnorm_case(3, 1025, 1, zero_group=True)
    assert signs[0] == "zero" and S.bits(x[0].max())[()] == 0 and (np.delete(x[0], 3) < 0).all()


def test_maxnorm_reference_is_autograd_of_x_over_amax():
    for G, n in [(3, 5), (3, 1025), (1, 16387)]:
        for v in range(len(S.maxnorm_variants(n))):
            x, _ = S.maxnorm_case(G, n, v)
            g = S.maxnorm_grad(G, n, v)
            xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            y = xt / xt.amax(dim=1, keepdim=True)
            (y * torch.tensor(g, dtype=torch.float64)).sum().backward()
            ref, _ = S.maxnorm_adjoint(x, g, False)
            assert np.abs(ref - xt.grad.numpy()).max() <= 1e-12 * np.abs(ref).max()
            out, m = S.maxnorm_fwd(x)
            assert np.abs(out - y.detach().numpy()).max() <= U * np.abs(out).max() and out.dtype == np.float32


@pytest.mark.parametrize("fused", [False, True], ids=["K5", "K5f"])
def test_maxnorm_bound_holds_for_float32_and_sees_the_planted_defects(fused):
    r, rt = _maxnorm_sweep(fused)
    print("%s adjoint, honest float32: max err/bound %.3g (the half-ulp of g / m: tight by nature), on the maxima %.3g"
          % ("K5f" if fused else "K5", r, rt))
    assert r <= 1.0
    for defect in ("ties", "all", "drop"):
        rd = _maxnorm_sweep(fused, defect)[0]
        print("   defect %-6s max err/bound %.3g" % (defect, rd))
        assert rd > 1.0, defect


@pytest.mark.parametrize("fused", [False, True], ids=["K5", "K5f"])
def test_maxnorm_exact_cases(fused):
    """the precondition (every partial sum below 2^24 units), and: the float32 emulation EQUALS the float64 value, a
    defect does not"""
    for G, n in S.MAXNORM_CASES:
        for v, plants in enumerate(S.maxnorm_variants(n)):
            x, _ = S.maxnorm_case(G, n, v, exact=True)
            gx = S.maxnorm_grad(G, n, v, exact=True, channels=3 if fused else 1)
            g = S.grad_input(gx) if fused else gx
            assert len(plants) in (1, 2, 4) and S.is_f32(np.asarray(g, np.float64))
            m = x.max(1).astype(np.float64)
            assert (np.frexp(np.abs(m))[0] == 0.5).all() and (x * 4 == np.round(x * 4)).all()
            assert (np.abs(x) <= np.abs(m)[:, None])[m > 0].all()         # (a negative maximum is the smallest magnitude)
            assert S.maxnorm_exact_units(x, g) < S.LIMIT
    assert _maxnorm_sweep(fused, exact=True) == 0
    for defect in ("ties", "all", "drop"):
        assert _maxnorm_sweep(fused, defect, exact=True) > 0, defect


def test_maxnorm_forward_defects_break_bit_equality():
    """one tail element left out of the maximum; the maximum of a mixed-sign group taken over magnitudes"""
    hit = {"tail": 0, "magnitude": 0}
    for G, n in S.MAXNORM_CASES:
        for v in range(len(S.maxnorm_variants(n))):
            x, _ = S.maxnorm_case(G, n, v)
            out, m = S.maxnorm_fwd(x)
            assert S.same_bits(m, emu_maxnorm_max(x))
            for d in hit:
                md = emu_maxnorm_max(x, d)
                with np.errstate(divide="ignore", invalid="ignore"):
                    hit[d] += not (S.same_bits(md, m) and S.same_bits(x / md[:, None], out))
    assert hit["tail"] > 0 and hit["magnitude"] > 0, hit


def test_store_input_and_grad_input_are_float32():
    x, _ = S.maxnorm_case(3, 1025, 0)
    xn, m = S.maxnorm_input_fwd(x)
    assert xn.dtype == np.float32 and xn.shape == (3, 1025, 3)
    want = (x.astype(np.float64) / m[:, None].astype(np.float64)) * 255.0
    assert (np.abs(xn - (want[..., None] - S.MEAN.astype(np.float64))) <= 3 * U * (np.abs(want)[..., None] + 124.0)).all()
    g = S.maxnorm_grad(3, 1025, 0, channels=3)
    assert S.grad_input(g).dtype == np.float32
    assert np.abs(S.grad_input(g) - 255.0 * g.astype(np.float64).sum(-1)).max() <= 5 * U * 255.0 * np.abs(g).sum(-1).max()


# ---- A5 ----------------------------------------------------------------------------------------------------------------
A5 = [(hw, hw2, Cin) for (hw, hw2) in S.A5_CASES for Cin in S.A5_CINS]
A5X = [(hw, hw2, Cin) for (hw, hw2) in S.A5_EXACT_CASES for Cin in S.A5_CINS]


def _exact_coords(n_in, n_out):
    s = S.tf1_axis(n_in, n_out)[3]
    return bool(np.array_equal(s * n_out, np.arange(n_out, dtype=np.float64) * n_in))


def _axis32(n_in, n_out, defect):
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    s = (dst + F32(0.5)) * scale - F32(0.5) if defect == "half" else dst * scale
    s = np.maximum(s, F32(0))
    i0 = np.floor(s).astype(np.int64)
    i1 = i0 + 1 if defect == "unclamped" else np.minimum(i0 + 1, n_in - 1)
    w = s - i0.astype(np.float32)
    assert w.dtype == np.float32
    return i0, i1, w


def emu_a5_fwd(img, H2, W2, defect=None):
    img = np.asarray(img, np.float32)
    B, H, W, Cin = img.shape
    if (H2, W2) == (H, W):
        r = img
    else:
        pad = np.zeros((B, H + 1, W + 1, Cin), np.float32)    # (what an unclamped i1 reads past the image: zeros)
        pad[:, :H, :W] = img
        y0, y1, wy = _axis32(H, H2, defect)
        x0, x1, wx = _axis32(W, W2, defect)
        wy, wx = wy.reshape(1, H2, 1, 1), wx.reshape(1, 1, W2, 1)
        if defect == "swap":
            wy, wx = F32(1) - wy, F32(1) - wx
        tl, tr = pad[:, y0][:, :, x0], pad[:, y0][:, :, x1]
        bl, br = pad[:, y1][:, :, x0], pad[:, y1][:, :, x1]
        top = tl + (tr - tl) * wx
        bot = bl + (br - bl) * wx
        r = top + (bot - top) * wy
    d = r * F32(255)
    if Cin == 1:
        d = np.repeat(d, 3, -1)
    x = d - S.MEAN
    assert d.dtype == np.float32 and x.dtype == np.float32
    return d, x


def emu_a5_bwd(g_x, H, W, Cin, defect=None):
    g3 = np.asarray(g_x, np.float32) * F32(255)
    B, H2, W2, _ = g3.shape
    if Cin == 1:
        g = g3[..., :1] if defect == "one_channel" else ((g3[..., 0] + g3[..., 1]) + g3[..., 2])[..., None]
    else:
        g = g3
    if (H2, W2) == (H, W):
        return g
    y0, y1, wy = _axis32(H, H2, defect)
    x0, x1, wx = _axis32(W, W2, defect)
    out = np.full((B, H + 1, W + 1, Cin), F32(0.5 if defect == "no_fill" else 0), np.float32)
    wy, wx = wy.reshape(1, H2, 1, 1), wx.reshape(1, 1, W2, 1)
    if defect == "swap":
        wy, wx = F32(1) - wy, F32(1) - wx
    for iy, qy in ((y0, F32(1) - wy), (y1, wy)):
        for ix, qx in ((x0, F32(1) - wx), (x1, wx)):
            c = g * qy * qx
            assert c.dtype == np.float32
            for b in range(B):                                # float32 accumulation, one addend at a time
                for yy in range(H2):
                    for xx in range(W2):
                        out[b, iy[yy], ix[xx]] += c[b, yy, xx]
    return out[:, :H, :W]


@pytest.mark.parametrize("case", A5, ids=_id)
def test_a5_reference_is_the_float64_oracle(case):
    hw, hw2, Cin = case
    img, g = S.a5_case(hw, hw2, Cin)
    d, x, bd, bx, co = S.loss_net_input(img, *hw2)
    it = torch.tensor(img, dtype=torch.float64, requires_grad=True)
    o = O.tf1_resize_bilinear(it, *hw2) * 255 if hw != hw2 else it * 255
    o = torch.cat([o] * 3, -1) if Cin == 1 else o
    (o * torch.tensor(g, dtype=torch.float64)).sum().backward()
    if hw == hw2 or (hw, hw2) == ((10, 12), (15, 18)):        # the sizes O.plugin_to_loss_net's one scale can reach
        p = O.plugin_to_loss_net(it, resize_scale=hw2[0] / hw[0], is_color=Cin == 3)
        assert torch.equal(p, o)
    gi, bg, cg = S.loss_net_input_adjoint(g, hw[0], hw[1], Cin)
    exact = _exact_coords(hw[0], hw2[0]) and _exact_coords(hw[1], hw2[1])
    # the float32 coordinate of the contract is within two roundings (the scale, the product) of the exact rational
    tol_d = 1e-12 * 255 + (0 if exact else 2 * co)
    tol_g = 1e-12 * np.abs(gi).max() + (0 if exact else 2 * cg)
    assert (np.abs(d - o.detach().numpy()) <= tol_d).all()
    assert (np.abs(gi - it.grad.numpy()) <= tol_g).all()
    assert np.array_equal(x, d - S.MEAN.astype(np.float64))
    assert S.tf1_floor_agrees(hw[0], hw2[0]) and S.tf1_floor_agrees(hw[1], hw2[1])
    if hw == (20, 16):
        assert (gi == 0).mean() > 0.5                         # most input pixels receive nothing


def _a5_ratios(case, defect=None, exact=False):
    hw, hw2, Cin = case
    img, g = S.a5_case(hw, hw2, Cin, exact=exact)
    d, x, bd, bx, _ = S.loss_net_input(img, *hw2)
    gi, bg, _ = S.loss_net_input_adjoint(g, hw[0], hw[1], Cin)
    d32, x32 = emu_a5_fwd(img, *hw2, defect=defect)
    g32 = emu_a5_bwd(g, hw[0], hw[1], Cin, defect=defect)
    if exact:
        return (float((d32 != d).sum()), float((x32 != x.astype(np.float32)).sum()), float((g32 != gi).sum()))
    link = S.err_ratio(np.abs(x32.astype(np.float64) - (d32.astype(np.float64) - S.MEAN)), U * (np.abs(d32) + np.abs(x32)))
    assert defect is not None or link <= 1.0
    return (S.err_ratio(np.abs(d32 - d), bd), S.err_ratio(np.abs(x32 - x), bx), S.err_ratio(np.abs(g32 - gi), bg))


def test_a5_bound_holds_for_float32_and_sees_the_planted_defects():
    r = np.max([_a5_ratios(c) for c in A5 if c[0] != c[1]], axis=0)
    ri = np.max([_a5_ratios(c) for c in A5 if c[0] == c[1]], axis=0)
    print("A5 honest float32: max err/bound d_img %.3g x %.3g g_img %.3g; at the image's own size (one or two roundings: "
          "tight by nature) %.3g %.3g %.3g" % (tuple(r) + tuple(ri)))
    assert max(r.max(), ri.max()) <= 1.0
    for defect, which in (("half", 0), ("unclamped", 0), ("swap", 0), ("half", 2), ("swap", 2), ("no_fill", 2),
                          ("one_channel", 2)):
        rd = max(_a5_ratios(c, defect)[which] for c in A5)
        print("   defect %-12s %s max err/bound %.3g" % (defect, ("d_img", "x", "g_img")[which], rd))
        assert rd > 1.0, (defect, which)


def test_a5_identity_is_one_product():
    for Cin in S.A5_CINS:
        img, g = S.a5_case((10, 12), (10, 12), Cin)
        d32, _ = emu_a5_fwd(img, 10, 12)
        assert S.same_bits(d32, np.repeat(img * F32(255), 3 // Cin, -1))
    assert S.same_bits(emu_a5_bwd(g, 10, 12, 3), g * F32(255))


def test_a5_the_plain_difference_already_leaves_u_d_img():
    """why x is held to U (|d_img| + |x|) against d_img: fl(d_img - mean) alone is further than U |d_img| from
    d_img - mean for small d_img (mean's ulp is 2^-17)"""
    d = np.float32(3.1415927)
    x = d - S.MEAN[0]
    err = abs(float(x) - (float(d) - float(S.MEAN[0])))
    assert U * abs(float(d)) < err <= U * abs(float(x))


@pytest.mark.parametrize("case", A5X, ids=_id)
def test_a5_exact_cases(case):
    hw, hw2, Cin = case
    img, g = S.a5_case(hw, hw2, Cin, exact=True)
    for n_in, n_out in zip(hw, hw2):
        w = S.tf1_axis(n_in, n_out)[2]
        assert set(np.unique(w)) <= {0.0, 0.5} and _exact_coords(n_in, n_out)
    d, x, _, _, _ = S.loss_net_input(img, *hw2)
    gi, _, _ = S.loss_net_input_adjoint(g, hw[0], hw[1], Cin)
    # corners in 1/4, weights in 1/2 twice, times 255: units of 255/16 = the unit 1/16; gradients: 255 g w w in 1/4
    assert S.units(255.0 * 4 * np.ones(1), 1.0 / 16) < S.LIMIT and S.is_f32(d)
    gabs, _, _ = S.loss_net_input_adjoint(np.abs(g), hw[0], hw[1], Cin)
    assert S.units(gabs, 0.25) < S.LIMIT and S.is_f32(gi)
    assert _a5_ratios(case, exact=True) == (0.0, 0.0, 0.0)
    assert max(_a5_ratios(case, "swap", exact=True)) > 0


# ---- K24 ---------------------------------------------------------------------------------------------------------------
K24 = [(hw, hw2, C) for (hw, hw2) in S.BICUBIC_CASES for C in S.BICUBIC_CS]


def _taps32(n_in, n_out, defect):
    a = F32(-0.75)
    src = np.arange(n_out, dtype=np.float32) * (F32(n_in) / F32(n_out))
    fl = np.floor(src)
    t = src - fl if defect == "raw" else np.rint((src - fl) * F32(1024)) / F32(1024)
    t1, u = t + F32(1), F32(1) - t
    u1 = u + F32(1)
    w = np.stack([((a * t1 - F32(5) * a) * t1 + F32(8) * a) * t1 - F32(4) * a,
                  ((a + F32(2)) * t - (a + F32(3))) * t * t + F32(1),
                  ((a + F32(2)) * u - (a + F32(3))) * u * u + F32(1),
                  ((a * u1 - F32(5) * a) * u1 + F32(8) * a) * u1 - F32(4) * a], 1)
    assert w.dtype == np.float32
    loc = fl.astype(np.int64)
    return np.clip(np.stack([loc - 1, loc, loc + 1, loc + 2], 1), 0, n_in - 1), w


def emu_bicubic(x, oh, ow, defect=None):
    x = np.asarray(x, np.float32)
    B, H, W, C = x.shape
    iy, wy = _taps32(H, oh, defect)
    ix, wx = _taps32(W, ow, defect)
    flat = x.reshape(B, -1)
    c = np.arange(C).reshape(1, 1, C)

    def at(k, q):                                             # x[b, iy[k], ix[q], c] for every output element
        pix = iy[:, k].reshape(oh, 1, 1) * W + ix[:, q].reshape(1, ow, 1)
        if defect == "stride":                                # the pixel index not multiplied by C
            return flat[:, pix + c]
        return flat[:, pix * C + c]

    if defect == "stride":                                    # ... in a kernel that also sums the columns first
        rows = []
        for k in range(4):
            r = np.zeros((B, oh, ow, C), np.float32)
            for q in range(4):
                r = r + wx[:, q].reshape(1, 1, ow, 1) * at(k, q)
            rows.append(r)
        return ((wy[:, 0].reshape(1, oh, 1, 1) * rows[0] + wy[:, 1].reshape(1, oh, 1, 1) * rows[1])
                + wy[:, 2].reshape(1, oh, 1, 1) * rows[2]) + wy[:, 3].reshape(1, oh, 1, 1) * rows[3]
    col = []
    for q in range(4):
        r = np.zeros((B, oh, ow, C), np.float32)
        for k in range(4):
            r = r + wy[:, k].reshape(1, oh, 1, 1) * at(k, q)
        col.append(r)
    out = ((wx[:, 0].reshape(1, 1, ow, 1) * col[0] + wx[:, 1].reshape(1, 1, ow, 1) * col[1])
           + wx[:, 2].reshape(1, 1, ow, 1) * col[2]) + wx[:, 3].reshape(1, 1, ow, 1) * col[3]
    assert out.dtype == np.float32
    return out


def test_bicubic_reference_is_the_oracle_and_the_bound_holds_for_float32():
    """the oracle takes its weights from a float32 table: it is held to the share of the bound that covers the weights;
    the honest float32 emulation to the whole bound"""
    worst = 0.0
    for hw, hw2, C in K24:
        x = S.bicubic_case(hw, C)
        ref, bound, werr = S.resize_bicubic(x, *hw2)
        o = O.tf1_resize_bicubic(torch.tensor(x, dtype=torch.float64), *hw2).numpy()
        assert (np.abs(ref - o) <= werr + 1e-12 * np.abs(x).max()).all(), (hw, hw2, C)
        got = emu_bicubic(x, *hw2)
        worst = max(worst, S.err_ratio(np.abs(got - ref), bound))
        if hw == hw2:
            assert S.same_bits(got, x) and np.array_equal(ref, x.astype(np.float64))
        if hw == (1, 5):
            assert (S.bicubic_axis(1, 5)[0] == 0).all()       # every row tap clamps to 0
    print("K24 honest float32: max err/bound %.3g" % worst)
    assert worst <= 1.0


def test_bicubic_sees_the_planted_defects():
    for defect, Cs in (("raw", S.BICUBIC_CS), ("stride", [3])):
        rd = 0.0
        for hw, hw2, C in K24:
            if C in Cs:
                x = S.bicubic_case(hw, C)
                ref, bound, _ = S.resize_bicubic(x, *hw2)
                rd = max(rd, S.err_ratio(np.abs(emu_bicubic(x, *hw2, defect=defect) - ref), bound))
        print("   defect %-6s max err/bound %.3g" % (defect, rd))
        assert rd > 1.0, defect


def test_bicubic_table_index_is_far_from_a_tie():
    """a condition on the inputs: no coordinate of any case is within 1024 2U src of a half-integer table index"""
    nearest = {}
    for hw, hw2 in S.BICUBIC_CASES:
        for n_in, n_out in zip(hw, hw2):
            dist, margin = S.bicubic_tie_margin(n_in, n_out)
            assert (dist > margin).all(), (n_in, n_out)
            nearest[(n_in, n_out)] = (float(dist.min()), float(margin.max()))
            # and the float32 index of the reference is the index of the exact rational
            src = S.bicubic_axis(n_in, n_out)[3].astype(np.float64)
            exact = (np.arange(n_out) * n_in % n_out) * 1024.0 / n_out
            assert np.array_equal(np.rint((src - np.floor(src)) * 1024.0), np.rint(exact))
    print("nearest table-index tie per axis (distance, margin):", nearest)


# ---- the 2-D links -----------------------------------------------------------------------------------------------------
def test_link_references_are_the_documented_conventions():
    """a NaN clamps to 0 and passes no gradient, the ends pass theirs (tests/colour_grid_ref.py); torch.clamp's adjoint"""
    for N, C in S.link_cases():
        v = S.link_values(N, C)
        order = S.link_order(N)
        assert sorted(order) == list(range(N))
        out, defined = S.colour_clamp_gather(v, order)
        want = torch.clamp(torch.tensor(np.nan_to_num(v[order].astype(np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf)), 0, 1)
        assert np.array_equal(out.astype(np.float64), want.numpy()) and out.dtype == np.float32
        g = np.random.RandomState(N).randn(N, C).astype(np.float32)
        vt = torch.tensor(np.nan_to_num(v.astype(np.float64), nan=-1.0, posinf=np.inf, neginf=-np.inf), requires_grad=True)
        (torch.clamp(vt, 0, 1) * torch.tensor(g, dtype=torch.float64)).sum().backward()
        assert np.array_equal(S.clamp01_bwd(g, v).astype(np.float64), vt.grad.numpy())
        gv = S.colour_clamp_scatter_bwd(g, v, order)
        assert not np.isnan(gv).any()
        assert np.array_equal(gv[order], np.where(S.inside01(v[order]), g, 0))
    v = S.link_values(257, 3)
    assert np.isnan(v).any() and np.isinf(v).any() and (v == 1).any() and (np.nanmin(np.abs(v[v != 0])) < 1e-44)


def test_iterate_update_reference():
    x, g = S.iterate_case(257)
    r = S.iterate_update(x, g)
    assert r.dtype == np.float32 and not np.isnan(r).any()
    fin = np.isfinite(x) & (np.abs(g) < 1e30) & (np.abs(x) < 1e30)
    assert np.abs(r[fin] - x[fin].astype(np.float64)).max() <= 2 * U * (np.abs(x[fin]) + 2 * np.abs(g[fin])).max()
    assert r[0] == g[0] + (F32(0) - g[0])                     # NaN -> 0
    assert np.isinf(r[3]) and np.isinf(r[4])                  # FLT_MAX - -FLT_MAX overflows


def test_axpy_bound_holds_for_float32():
    rng = np.random.RandomState(3)
    y, x, a = rng.randn(771).astype(np.float32), rng.randn(771).astype(np.float32), 0.3
    ref, bound = S.axpy(y, x, a)
    r = S.err_ratio(np.abs((y + F32(a) * x).astype(np.float64) - ref), bound)
    print("axpy honest float32: max err/bound %.3g" % r)
    assert r <= 1.0
    assert S.err_ratio(np.abs((y + F32(a) * x * F32(1 + 2 ** -20)).astype(np.float64) - ref), bound) > 1.0


# ---- the explicit 2-D warp -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.WARP2D_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", S.WARP2D_CS)
def test_warp2d_reference(shape, C):
    """field_ref's warp_fwd / warp_adjoint on two axes against O.batch_warp2d and autograd: float64 to 1e-12 (times the
    amplification outside the image), the float32 oracle inside every bound; the share of pixels with the two-candidate
    latitude is capped at 1 %"""
    imgs, coords, g = S.warp2d_case(shape, C)
    s, bs = FR.warp_fwd(imgs, coords)
    refs = FR.warp_adjoint(imgs, coords, g)
    res = {}
    for dtype in (torch.float64, torch.float32):
        it = torch.tensor(imgs, dtype=dtype).requires_grad_()
        ct = torch.tensor(coords, dtype=dtype).requires_grad_()
        out = O.batch_warp2d(it, ct, [2, *shape])
        (out * torch.tensor(g, dtype=dtype)).sum().backward()
        res[dtype] = (out.detach().numpy(), it.grad.numpy(), np.moveaxis(ct.grad.numpy(), 1, -1))
    o, gi, gc = res[torch.float64]
    o32, gi32, gc32 = res[torch.float32]
    r = [FR.err_ratio(np.abs(o32 - s), bs), 0.0, 0.0]
    for b, ref in enumerate(refs):
        axes = FR.trace(shape, coords[b], explicit=True)
        A = FR._prod(FR.amplification(axes))
        A_dest = np.ones(shape)
        for idx, _w in FR.MR._corners(axes):
            np.maximum.at(A_dest, tuple(idx), A)
        assert (np.abs(s[b] - o[b]) <= 1e-12 * np.abs(imgs).max() * A[..., None]).all()
        assert (np.abs(ref["g_d"] - gi[b]) <= 1e-12 * np.abs(gi).max() * A_dest[..., None]).all()
        near = np.abs(ref["vel_cand"] - gc[b][None, None]).min(axis=(0, 1))
        assert (near <= 1e-12 * max(np.abs(gc).max(), 1.0) * A[..., None]).all()
        r[1] = max(r[1], FR.err_ratio(np.abs(gi32[b] - ref["g_d"]), ref["bound_d"]))
        r[2] = max(r[2], FR.vel_ratio(ref, gc32[b]))
        share = float(ref["unsure"].mean())
        assert share <= 0.01, (shape, C, b, share)
    print("warp2d %s C%d float32 oracle err/bound: fwd %.3f g_imgs %.3f g_coords %.3f" % ((shape, C) + tuple(r)))
    assert max(r) <= 1.0

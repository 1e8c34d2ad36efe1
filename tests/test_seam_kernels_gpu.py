"""The seam between a rendered image and the loss network, and the small kernels beside it, element by element against
tests/seam_ref.py: max-normalisation and its fusion with the loss-net input (K5, K5f), the loss-net input (A5), the
legacy bicubic resize (K24), the elementwise links of the 2-D colour stylizer and the explicit 2-D warp (through
tests/field_ref.py on two axes).  What numpy float32 can restate exactly is compared bit for bit; everything else lies
within its own derived bound of the float64 restatement.  Every output buffer is pre-filled with NaN, so an unwritten
element shows; every check prints the largest err / bound it saw (pytest -s).  The references, their bounds and the cases
are pinned without a GPU by tests/test_seam_ref_cpu.py."""
import numpy as np
import pytest
import torch

from tests import field_ref as FR
from tests import seam_ref as S

pytestmark = pytest.mark.gpu
U, F32 = S.U, np.float32


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


def T(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _id(c):
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)


def ratio(name, got, ref, bound, quiet=False):
    r = S.err_ratio(np.abs(np.asarray(got, dtype=np.float64) - ref), bound)
    if not quiet:
        print("%-72s max err/bound %.3g" % (name, r))
    assert r <= 1.0, (name, r)
    return r


def equal_or_both_nan(a, b):
    """bit equality, a NaN of either sign standing for a NaN (0 / 0 has no defined sign)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(S.bits(a)[~nan], S.bits(b)[~nan]))


# ---- K5 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.MAXNORM_CASES, ids=_id)
def test_maxnorm_fwd_is_exact(ops, case):
    """gmax = max(x) and out = x / gmax bit for bit: every plant position, ties, all-positive, all-negative and
    mixed-sign groups (the atomic maximum of the 32-block form switches between a signed max and an unsigned min), a
    group with maximum +0.0 over negative values; a second call gives the same bits"""
    G, n = case
    for v in range(len(S.maxnorm_variants(n))):
        for zero in ([False, True] if v == 1 and n > 1 else [False]):
            x, signs = S.maxnorm_case(G, n, v, zero_group=zero)
            out_ref, m_ref = S.maxnorm_fwd(x)
            xt = T(x)
            out, gmax = ops.maxnorm_fwd(xt, G, out=nans(G, n), gmax=nans(G))
            assert S.same_bits(N(gmax), m_ref), (case, v, signs, N(gmax), m_ref)
            assert equal_or_both_nan(N(out), out_ref), (case, v, signs)
            assert not zero or (N(gmax)[0] == 0 and not np.signbit(N(gmax)[0]) and np.isinf(N(out)[0]).sum() == n - 1)
            out2, gmax2 = ops.maxnorm_fwd(xt, G, out=nans(G, n), gmax=nans(G))
            assert equal_or_both_nan(N(out2), N(out)) and S.same_bits(N(gmax2), N(gmax))
    print("maxnorm_fwd %s: %d variants bit for bit" % (_id(case), len(S.maxnorm_variants(n))))


def _maxnorm_bwd_forms(ops, xt, gmax, gt, G, n):
    """(two_phase, g_img) of every form nfs_maxnorm_bwd has for this n: through the wrapper (32 blocks from 16384 on),
    and from 16384 on also without a workspace (one block on a large group)"""
    from neural_flow_style_amd import _lib
    out = [(n >= S.MN_MULTI, ops.maxnorm_bwd(xt, gmax, gt, g_img=nans(G, n)))]
    if n >= S.MN_MULTI:
        g_img = nans(G, n)
        _lib.call("nfs_maxnorm_bwd", xt.data_ptr(), gmax.data_ptr(), gt.data_ptr(), g_img.data_ptr(), G, n, None,
                  ops._stream())
        out.append((False, g_img))
    return out


@pytest.mark.parametrize("case", S.MAXNORM_CASES, ids=_id)
def test_maxnorm_bwd(ops, case):
    G, n = case
    worst = worst_tie = 0.0
    for v in range(len(S.maxnorm_variants(n))):
        x, signs = S.maxnorm_case(G, n, v)
        g = S.maxnorm_grad(G, n, v)
        xt, gt = T(x), T(g)
        gmax = T(x.max(1))
        tie = x == x.max(1, keepdims=True)
        for two, g_img in _maxnorm_bwd_forms(ops, xt, gmax, gt, G, n):
            ref, bound = S.maxnorm_adjoint(x, g, two)
            name = "maxnorm_bwd %s v%d %s" % (_id(case), v, "32 blocks" if two else "one block")
            worst = max(worst, ratio(name, N(g_img), ref, bound, quiet=True))
            worst_tie = max(worst_tie, ratio(name, N(g_img)[tie], ref[tie], bound[tie], quiet=True))
        assert S.same_bits(N(ops.maxnorm_bwd(xt, gmax, gt, g_img=nans(G, n))), N(ops.maxnorm_bwd(xt, gmax, gt)))
    print("%-72s max err/bound %.3g (on the maxima %.3g)" % ("maxnorm_bwd %s" % _id(case), worst, worst_tie))


@pytest.mark.parametrize("case", S.MAXNORM_CASES, ids=_id)
def test_maxnorm_bwd_exact_cases(ops, case):
    """m a power of two, x in quarters, integer g, 1 / 2 / 4 ties: the kernel EQUALS the float64 value"""
    G, n = case
    for v in range(len(S.maxnorm_variants(n))):
        x, _ = S.maxnorm_case(G, n, v, exact=True)
        g = S.maxnorm_grad(G, n, v, exact=True)
        assert S.maxnorm_exact_units(x, g) < S.LIMIT
        xt, gt = T(x), T(g)
        for two, g_img in _maxnorm_bwd_forms(ops, xt, T(x.max(1)), gt, G, n):
            ref, _ = S.maxnorm_adjoint(x, g, two)
            assert np.array_equal(N(g_img).astype(np.float64), ref), (case, v, two)
    print("maxnorm_bwd exact %s: %d variants equal" % (_id(case), len(S.maxnorm_variants(n))))


# ---- K5f ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.MAXNORM_CASES, ids=_id)
def test_maxnorm_input_fwd_is_exact(ops, case):
    """x[., c] = fl(fl(fl(x / m) 255) - mean_c) bit for bit: the one-block form below 16384 elements per group, the
    one-launch form (every block takes the whole group's maximum, by float4 where the group is 16-byte aligned) from
    there on"""
    G, n = case
    for v in range(len(S.maxnorm_variants(n))):
        x, signs = S.maxnorm_case(G, n, v)
        ref, m_ref = S.maxnorm_input_fwd(x)
        xt = T(x.reshape(G, 1, n))
        xn, gmax = ops.maxnorm_input_fwd(xt, G, out=nans(G, 1, n, 3), gmax=nans(G))
        assert S.same_bits(N(gmax), m_ref), (case, v, signs)
        assert S.same_bits(N(xn).reshape(G, n, 3), ref), (case, v, signs)
        xn2, gmax2 = ops.maxnorm_input_fwd(xt, G, out=nans(G, 1, n, 3), gmax=nans(G))
        assert S.same_bits(N(xn2), N(xn)) and S.same_bits(N(gmax2), N(gmax))
    print("maxnorm_input_fwd %s: %d variants bit for bit" % (_id(case), len(S.maxnorm_variants(n))))


@pytest.mark.parametrize("case", S.MAXNORM_CASES, ids=_id)
def test_maxnorm_input_bwd(ops, case):
    """the incoming gradient 255 (g0 + g1 + g2) restated exactly in float32, then K5's reference and bound (always the
    two-phase form); and the exact cases"""
    G, n = case
    worst = worst_tie = 0.0
    for v in range(len(S.maxnorm_variants(n))):
        for exact in (False, True):
            x, _ = S.maxnorm_case(G, n, v, exact=exact)
            g_x = S.maxnorm_grad(G, n, v, exact=exact, channels=3)
            g = S.grad_input(g_x)
            xt, gt, gmax = T(x.reshape(G, 1, n)), T(g_x.reshape(G, 1, n, 3)), T(x.max(1))
            g_img = N(ops.maxnorm_input_bwd(xt, gmax, gt, out=nans(G, 1, n))).reshape(G, n)
            ref, bound = S.maxnorm_adjoint(x, g, True)
            if exact:
                assert S.maxnorm_exact_units(x, g) < S.LIMIT
                assert np.array_equal(g_img.astype(np.float64), ref), (case, v)
                continue
            tie = x == x.max(1, keepdims=True)
            name = "maxnorm_input_bwd %s v%d" % (_id(case), v)
            worst = max(worst, ratio(name, g_img, ref, bound, quiet=True))
            worst_tie = max(worst_tie, ratio(name, g_img[tie], ref[tie], bound[tie], quiet=True))
            again = N(ops.maxnorm_input_bwd(xt, gmax, gt, out=nans(G, 1, n))).reshape(G, n)
            assert S.same_bits(again, g_img)
    print("%-72s max err/bound %.3g (on the maxima %.3g)" % ("maxnorm_input_bwd %s" % _id(case), worst, worst_tie))


# ---- A5 ----------------------------------------------------------------------------------------------------------------
A5 = [(hw, hw2, Cin) for (hw, hw2) in S.A5_CASES for Cin in S.A5_CINS]
A5X = [(hw, hw2, Cin) for (hw, hw2) in S.A5_EXACT_CASES for Cin in S.A5_CINS]


def _a5_run(ops, img, g, hw, hw2, Cin):
    shape = (S.A5_B,) + hw2 + (3,)
    it = T(img)
    d, x = ops.loss_net_input_fwd(it, *hw2, out_d_img=nans(*shape), out_x=nans(*shape))
    d1, _ = ops.loss_net_input_fwd(it, *hw2, want_x=False, out_d_img=nans(*shape))
    _, x1 = ops.loss_net_input_fwd(it, *hw2, want_d_img=False, out_x=nans(*shape))
    assert S.same_bits(N(d1), N(d)) and S.same_bits(N(x1), N(x))
    gi = ops.loss_net_input_bwd(T(g), hw[0], hw[1], Cin, out=nans(S.A5_B, *hw, Cin))
    return N(d), N(x), N(gi)


@pytest.mark.parametrize("case", A5, ids=_id)
def test_loss_net_input(ops, case):
    hw, hw2, Cin = case
    img, g = S.a5_case(hw, hw2, Cin)
    d, x, gi = _a5_run(ops, img, g, hw, hw2, Cin)
    d_ref, x_ref, bd, bx, _ = S.loss_net_input(img, *hw2)
    gi_ref, bg, _ = S.loss_net_input_adjoint(g, hw[0], hw[1], Cin)
    name = "loss_net_input %s" % _id(case)
    ratio(name + " d_img", d, d_ref, bd)
    ratio(name + " x", x, x_ref, bx)
    ratio(name + " x against d_img", x.astype(np.float64), d.astype(np.float64) - S.MEAN, U * (np.abs(d) + np.abs(x)))
    ratio(name + " g_img", gi, gi_ref, bg)
    if hw == hw2:                                             # one product each way: bit for bit
        assert S.same_bits(d, np.repeat(img * F32(255), 3 // Cin, -1))
        g3 = g * F32(255)
        assert S.same_bits(gi, g3 if Cin == 3 else ((g3[..., 0] + g3[..., 1]) + g3[..., 2])[..., None])
    if hw == (20, 16):
        assert ((gi == 0) == (gi_ref == 0)).all() and (gi == 0).mean() > 0.5


@pytest.mark.parametrize("case", A5X, ids=_id)
def test_loss_net_input_exact_cases(ops, case):
    """scales of 2 and 1/2 per axis, images in quarters, integer gradients: d_img and g_img EQUAL the float64 value, x
    its rounding (the preconditions are asserted by tests/test_seam_ref_cpu.py)"""
    hw, hw2, Cin = case
    img, g = S.a5_case(hw, hw2, Cin, exact=True)
    d, x, gi = _a5_run(ops, img, g, hw, hw2, Cin)
    d_ref, x_ref, _, _, _ = S.loss_net_input(img, *hw2)
    gi_ref, _, _ = S.loss_net_input_adjoint(g, hw[0], hw[1], Cin)
    assert np.array_equal(d.astype(np.float64), d_ref)
    assert np.array_equal(x, x_ref.astype(np.float32))
    assert np.array_equal(gi.astype(np.float64), gi_ref)
    print("loss_net_input exact %s: equal" % _id(case))


# ---- K24 ---------------------------------------------------------------------------------------------------------------
K24 = [(hw, hw2, C) for (hw, hw2) in S.BICUBIC_CASES for C in S.BICUBIC_CS]


@pytest.mark.parametrize("case", K24, ids=_id)
def test_resize_bicubic_tf1(ops, case):
    hw, hw2, C = case
    x = S.bicubic_case(hw, C)
    out = N(ops.resize_bicubic_tf1(T(x), *hw2, out=nans(2, *hw2, C)))
    ref, bound, _ = S.resize_bicubic(x, *hw2)
    ratio("resize_bicubic_tf1 %s" % _id(case), out, ref, bound)
    if hw == hw2:                                             # weights exactly [0, 1, 0, 0]
        assert S.same_bits(out, x)


# ---- the 2-D links -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.link_cases(), ids=_id)
@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
def test_colour_clamp_links_are_exact(ops, case, permuted):
    N_, C = case
    v = S.link_values(N_, C)
    g = S.link_values(N_, C, seed=3)
    g[np.isnan(g)] = -0.0                                     # (a NaN has no bits to compare; -0.0 must pass as it is)
    order = S.link_order(N_) if permuted else None
    assert order is None or sorted(order.tolist()) == list(range(N_))
    ot = None if order is None else torch.tensor(order).cuda()
    out = N(ops.colour_clamp_gather(T(v), ot, out=nans(N_, C)))
    ref, defined = S.colour_clamp_gather(v, order)
    assert np.array_equal(out, ref) and np.array_equal(S.bits(out)[defined], S.bits(ref)[defined])
    back = N(ops.clamp01_bwd(T(g), T(v), out=nans(N_, C)))
    assert S.same_bits(back, S.clamp01_bwd(g, v))
    gv = N(ops.colour_clamp_scatter_bwd(T(g), T(v), ot, out=nans(N_, C)))
    assert not np.isnan(gv).any()                             # every row written
    assert S.same_bits(gv, S.colour_clamp_scatter_bwd(g, v, order))
    print("colour_clamp_gather / clamp01_bwd / colour_clamp_scatter_bwd N%d C%d %s: bit for bit"
          % (N_, C, "permuted" if permuted else "identity"))


@pytest.mark.parametrize("n", S.LINK_NCS)
def test_iterate_update_is_exact(ops, n):
    x, g = S.iterate_case(n)
    r = S.iterate_update(x, g)
    xt, gt = T(x), T(g)
    ops.iterate_update(xt, gt)
    assert S.same_bits(N(xt), r) and S.same_bits(N(gt), r)
    print("iterate_update n%d: x and g_opt bit for bit" % n)


@pytest.mark.parametrize("n", [1, 257])
def test_fill_writes_n_elements(ops, n):
    buf = nans(2 * n)
    ops.fill(buf[:n], 0.75)
    got = N(buf)
    assert (got[:n] == F32(0.75)).all() and np.isnan(got[n:]).all()
    ops.fill(buf[:n], -0.0)
    assert S.same_bits(N(buf)[:n], np.full(n, -0.0, np.float32))


@pytest.mark.parametrize("n", S.LINK_NCS)
def test_axpy(ops, n):
    rng = np.random.RandomState(n)
    y, x, a = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32), 0.3
    yt = T(y)
    ops.axpy(yt, T(x), a)
    ref, bound = S.axpy(y, x, a)
    ratio("axpy n%d" % n, N(yt), ref, bound)
    yi, xi = rng.randint(-9, 10, n).astype(np.float32), rng.randint(-9, 10, n).astype(np.float32)
    yt = T(yi)
    ops.axpy(yt, T(xi), -4.0)
    assert np.array_equal(N(yt), yi - 4 * xi)


# ---- the explicit 2-D warp -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.WARP2D_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", S.WARP2D_CS)
def test_warp2d(ops, shape, C):
    """nfs_warp2d_fwd / _bwd through field_ref on two axes; g_coords with the two-candidate latitude of warp3d (its share
    is capped by tests/test_seam_ref_cpu.py); the null-pointer branches: without g_imgs the bits of g_coords stay, without
    g_coords g_imgs stays inside its bound"""
    imgs, coords, g = S.warp2d_case(shape, C)
    it, ct, gt = T(imgs), T(coords), T(g)
    name = "%s C%d" % ("x".join(map(str, shape)), C)
    out = ops.warp2d_fwd(it, ct, out=nans(*imgs.shape))
    s, b = FR.warp_fwd(imgs, coords)
    ratio("warp2d_fwd " + name, N(out), s, b)
    gi, gc = ops.warp2d_bwd(it, ct, gt, out_coords=nans(*coords.shape))
    _, gc_only = ops.warp2d_bwd(it, ct, gt, need_imgs=False, out_coords=nans(*coords.shape))
    gi_only, none = ops.warp2d_bwd(it, ct, gt, need_coords=False)
    assert none is None and _ is None and S.same_bits(N(gc_only), N(gc))
    for bi, ref in enumerate(FR.warp_adjoint(imgs, coords, g)):
        ratio("warp2d_bwd g_imgs %s b%d" % (name, bi), N(gi)[bi], ref["g_d"], ref["bound_d"])
        ratio("warp2d_bwd g_imgs alone %s b%d" % (name, bi), N(gi_only)[bi], ref["g_d"], ref["bound_d"])
        r = FR.vel_ratio(ref, np.moveaxis(N(gc)[bi], 0, -1))
        print("%-72s max err/bound %.3g (%d pixels with two candidates)"
              % ("warp2d_bwd g_coords %s b%d" % (name, bi), r, int(ref["unsure"].sum())))
        assert r <= 1.0

"""tests/inception_ref.py held to account without a GPU: its float64 restatements against the oracle's TF-semantics
functions and their autograd, planted defects against the equality and the bounds the GPU module uses, the conditions on
every GPU case (exact units, float32 inputs, the path each case is there for, through the plan queries), and the rule of
a summed run."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import inception_ref as R


def t64(a):
    return torch.tensor(np.asarray(a, np.float64))


def nchw(a):
    return t64(a).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).detach().numpy()


def close(a, b, tol=1e-12):
    a, b = R.f64(a), R.f64(b)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= tol * max(float(np.abs(b).max()), 1e-300)


# ---- the references against the oracle ------------------------------------------------------------------------------------
# (kh, kw, stride, Ci, Co, B, H, W): stride 2 with odd and even sides, kh != kw, a 1x1 image, an image below the filter
XCHECK = [(3, 3, 1, 5, 7, 2, 6, 5), (3, 3, 2, 4, 6, 2, 7, 9), (3, 3, 2, 4, 6, 1, 8, 6), (7, 7, 2, 3, 8, 1, 10, 13),
          (1, 3, 1, 6, 4, 1, 5, 4), (5, 2, 2, 3, 5, 2, 6, 7), (7, 7, 2, 3, 4, 1, 1, 1), (5, 5, 1, 2, 3, 1, 2, 3)]


@pytest.mark.parametrize("case", XCHECK, ids=R.case_id)
def test_conv2d_and_its_adjoint_equal_the_oracle_and_autograd(case):
    kh, kw, stride, Ci, Co, B, H, W = case
    rng = np.random.RandomState(kh + H)
    x, w, b = rng.randn(B, H, W, Ci), rng.randn(kh, kw, Ci, Co), rng.randn(Co)
    assert R.same(H, kh, stride) == (-(-H // stride), O._tf_same(H, kh, stride)[0])
    xt = nchw(x).requires_grad_()
    want = O.tf_conv2d_same(xt, t64(w), t64(b), stride)
    pre, y, S = R.conv2d(x, w, b, stride, relu=True)
    assert close(pre, nhwc(want)) and close(y, np.maximum(nhwc(want), 0))
    gy, act = rng.randn(*pre.shape), rng.randn(*pre.shape)
    (want * nchw(gy * (act > 0))).sum().backward()
    gx, Sg = R.conv2d_dgrad(gy, w, (H, W), stride, act=act)
    assert close(gx, nhwc(xt.grad))
    # S is the same sum over absolute values
    assert close(S, R.conv2d(np.abs(x), np.abs(w), np.abs(b), stride)[0])
    assert close(Sg, R.conv2d_dgrad(np.abs(gy) * (act > 0), np.abs(w), (H, W), stride)[0])
    # the mask and the accumulate
    m = R.mask_tensor(x.shape, 3)
    old = rng.randn(*pre.shape)
    _, y2, _ = R.conv2d(x, w, None, stride, mask=m, y_old=old)
    assert close(y2, nhwc(O.tf_conv2d_same(nchw(x * (m > 0)), t64(w), None, stride)) + old)


@pytest.mark.parametrize("stride,B,H,W,C", [(1, 2, 6, 5, 3), (2, 2, 7, 9, 4), (2, 1, 8, 6, 2), (1, 1, 1, 1, 4), (2, 1, 1, 1, 4),
                                            (2, 1, 2, 3, 4), (1, 1, 1, 7, 2)])
def test_maxpool3_and_its_adjoint_equal_the_oracle_on_tie_free_input(stride, B, H, W, C):
    rng = np.random.RandomState(H * 10 + W)
    x = rng.randn(B, H, W, C)
    xt = nchw(x).requires_grad_()
    want = O.tf_maxpool3_same(xt, stride)
    y, arg = R.maxpool3(x, stride)
    assert np.array_equal(y, nhwc(want))
    gy = rng.randn(*y.shape)
    (want * nchw(gy)).sum().backward()
    gx, S = R.maxpool3_bwd(gy, arg, (H, W), stride)
    assert close(gx, nhwc(xt.grad))
    old, act = rng.randn(B, H, W, C), rng.randn(B, H, W, C)
    assert close(R.maxpool3_bwd(gy, arg, (H, W), stride, gx_old=old, relu_of=act)[0], (nhwc(xt.grad) + old) * (act > 0))
    assert np.all(S >= np.abs(gx) - 1e-12)


def _nine_taps(x, stride):
    """the tie rule spelled out: the first maximum in row-major window order among the taps inside the image"""
    B, H, W, C = x.shape
    (Ho, pt), (Wo, pl) = R.same(H, 3, stride), R.same(W, 3, stride)
    y, arg = np.zeros((B, Ho, Wo, C)), np.zeros((B, Ho, Wo, C), np.uint8)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for c in range(C):
                    best, at = None, 0
                    for tap in range(9):
                        iy, ix = oy * stride - pt + tap // 3, ox * stride - pl + tap % 3
                        if 0 <= iy < H and 0 <= ix < W and (best is None or x[b, iy, ix, c] > best):
                            best, at = x[b, iy, ix, c], tap
                    y[b, oy, ox, c], arg[b, oy, ox, c] = best, at
    return y, arg


@pytest.mark.parametrize("stride", [1, 2])
def test_maxpool3_tie_rule_is_the_literal_nine_tap_loop(stride):
    for (H, W) in R.POOL_SHAPES:
        x = R.tie_tensor((2, H, W, 4), H * 31 + W)
        y, arg = R.maxpool3(x, stride)
        y9, arg9 = _nine_taps(x, stride)
        assert np.array_equal(y, y9) and np.array_equal(arg, arg9), (H, W)
    assert len(np.unique(R.maxpool3(R.tie_tensor((2, 9, 12, 4), 1), stride)[1])) > 4     # (ties do move the position)


@pytest.mark.parametrize("C,ld,r,bias,alpha,beta", R.LRN_CASES)
def test_lrn_and_its_adjoint_equal_the_oracle_and_autograd(C, ld, r, bias, alpha, beta):
    x, gy = R.lrn_inputs(C)
    b32, a32, be32 = R.lrn_params(bias, alpha, beta)
    xt = nchw(x).requires_grad_()
    want = O.tf_lrn(xt, r, b32, a32, be32)
    y, scale = R.lrn(x, r, bias, alpha, beta)
    assert close(y, nhwc(want))
    (want * nchw(gy)).sum().backward()
    gx, bound = R.lrn_bwd(x, y, scale, gy, r, alpha, beta)
    assert close(gx, nhwc(xt.grad))
    old = np.ones_like(gx)
    assert close(R.lrn_bwd(x, y, scale, gy, r, alpha, beta, gx_old=old)[0], gx + old)


@pytest.mark.parametrize("k,H,W", R.AVGPOOL_CASES)
def test_avgpool_valid_and_its_adjoint_equal_torch(k, H, W):
    rng = np.random.RandomState(k + W)
    x = rng.randn(2, H, W, 4)
    xt = nchw(x).requires_grad_()
    want = torch.nn.functional.avg_pool2d(xt, k, 1)
    y, S = R.avgpool_valid(x, k)
    assert close(y, nhwc(want))
    gy = rng.randn(*y.shape)
    (want * nchw(gy)).sum().backward()
    assert close(R.avgpool_valid_bwd(gy, (H, W), k)[0], nhwc(xt.grad))


def test_relu_mask_add_is_the_float32_expression():
    rng = np.random.RandomState(0)
    g, add = rng.randn(2, 3, 4, 8).astype(np.float32), rng.randn(2, 3, 4, 8).astype(np.float32)
    act = R.mask_tensor(g.shape, 1)
    assert np.signbit(act[act == 0]).any() and (~np.signbit(act[act == 0])).any() and (act < 0).any()
    out = R.relu_mask_add(g, act, add)
    assert out.dtype == np.float32 and np.array_equal(out, (g * (act > 0) + add).astype(np.float32))
    assert np.array_equal(R.relu_mask_add(g, None, None), g) and np.array_equal(R.relu_mask_add(None, act, add), add)
    assert np.array_equal(R.relu_mask_add(g, act, None), g * (act > 0))


# ---- planted defects ------------------------------------------------------------------------------------------------------
def _chunked(x, w, bias, stride, mask=None, ksplit=1, defect=None, pad_shift=0):
    """the implicit GEMM as the kernel cuts it, in float64: K = taps x 16-channel chunks dealt to ``ksplit`` splits whose
    partial sums are added and finished by one epilogue -- with one defect planted"""
    x, w = R.f64(x), R.f64(w)
    keep = (R.f64(mask) >= 0 if defect == "mask_ge" else R.f64(mask) > 0) if mask is not None else 1.0
    x = x * keep
    kh, kw, Ci, Co = w.shape
    B, H, W, _ = x.shape
    (Ho, pt), (Wo, pl) = R.same(H, kh, stride), R.same(W, kw, stride)
    pt, pl = pt + pad_shift, pl + pad_shift
    cch = -(-Ci // 16)
    chunks = [(tap, cc) for tap in range(kh * kw) for cc in range(cch)]
    cps = -(-len(chunks) // ksplit)
    parts = np.zeros((ksplit, B, Ho, Wo, Co))
    for it, (tap, cc) in enumerate(chunks):
        if defect == "tap" and tap == kh * kw - 2:
            continue
        dy, dx = divmod(tap, kw)
        c0, c1 = cc * 16, min(cc * 16 + 16, Ci)
        if defect == "chunk_tail" and c1 == Ci and Ci % 16:
            c1 -= 4
        for oy in range(Ho):
            iy = oy * stride - pt + dy
            if not 0 <= iy < H:
                continue
            for ox in range(Wo):
                ix = ox * stride - pl + dx
                if 0 <= ix < W:
                    parts[it // cps, :, oy, ox] += x[:, iy, ix, c0:c1] @ w[dy, dx, c0:c1]
    if defect == "split":
        parts[ksplit // 2] = 0.0
    y = parts.sum(axis=0)
    if defect == "row_wrap":                              # the rows beyond M of the last tile land on row 0
        y[0, 0, 0] += y[0, 0, 0]
    return y + R.f64(bias) * (ksplit if defect == "bias_z" else 1)


PLANT = (3, 3, 1, 36, 8, 2, 5, 6)


@pytest.mark.parametrize("defect", ["tap", "chunk_tail", "split", "bias_z", "mask_ge", "row_wrap"])
def test_a_planted_gemm_defect_breaks_equality_and_exceeds_the_bound(defect):
    kh, kw, stride, Ci, Co, B, H, W = PLANT
    for exact in (True, False):
        d = R.conv_inputs(PLANT, exact)
        mask = R.mask_tensor(d["x"].shape, 9)
        if not exact:       # (the mask's zeros must hide something: the realistic x holds zeros of its own)
            d["x"] = d["x"] + np.float32(1.0)
        pre, _, S = R.conv2d(d["x"], d["w"], d["bias"], stride, mask=mask)
        bound = R.gemm_bound(S, kh * kw * Ci, 4, pre)
        sound = _chunked(d["x"], d["w"], d["bias"], stride, mask, ksplit=4)
        assert close(sound, pre, 1e-13)
        assert not R.first_mismatches(sound, pre, 0.0 if exact else bound)
        bad = _chunked(d["x"], d["w"], d["bias"], stride, mask, ksplit=4, defect=defect)
        if exact:
            R.exact_units(S)
            assert np.any(bad != pre), defect
        else:
            assert R.ratio(bad, pre, bound) > 1.0, defect
            assert "outside the bound" in R.first_mismatches(bad, pre, bound)


def test_a_pad_before_off_by_one_at_an_even_size_with_stride_2_is_caught():
    case = (3, 3, 2, 16, 8, 1, 6, 8)
    assert R.same(6, 3, 2) == (3, 0) and R.same(5, 3, 2) == (3, 1)
    for exact in (True, False):
        d = R.conv_inputs(case, exact)
        pre, _, S = R.conv2d(d["x"], d["w"], d["bias"], 2)
        bound = R.gemm_bound(S, 9 * 16, 1, pre)
        assert close(_chunked(d["x"], d["w"], d["bias"], 2), pre, 1e-13)
        bad = _chunked(d["x"], d["w"], d["bias"], 2, pad_shift=1)
        assert np.any(bad != pre) if exact else R.ratio(bad, pre, bound) > 1.0
        # ... and in the small data gradient
        gy = R.int_tensor(pre.shape, 4) if exact else np.random.RandomState(4).randn(*pre.shape)
        gx, Sg = R.conv2d_dgrad(gy, d["w"], (6, 8), 2)
        shifted = R.conv2d_dgrad(np.pad(gy, ((0, 0), (1, 0), (1, 0), (0, 0)))[:, :3, :4], d["w"], (6, 8), 2)[0]
        assert np.any(shifted != gx) if exact else R.ratio(shifted, gx, R.gemm_bound(Sg, 4 * 8, 1, gx)) > 1.0


def test_a_follower_written_instead_of_added_is_caught():
    for exact in (True, False):
        probs = R.group_problems("summed", exact)
        pre, y, S, n = R.run_reference(probs, [0, 1, 2])
        last = R.run_reference(probs, [2])[1]
        bound = R.gemm_bound(S, n, 4, y)
        assert n == 208
        assert np.any(last != y) if exact else R.ratio(last, y, bound) > 1.0
        # the order of a sum does not matter, the epilogue's owner does
        assert close(R.run_reference(probs, [2, 1, 0])[1], y, 1e-13)


@pytest.mark.parametrize("stride", [1, 2])
def test_a_pool_tie_given_to_the_last_maximum_is_caught(stride):
    x = R.tie_tensor((2, 9, 12, 4), 5)
    y, arg = R.maxpool3(x, stride)
    # the same loop with >= for >: the LAST maximum among the taps inside the image
    (Ho, pt), (Wo, pl) = R.same(9, 3, stride), R.same(12, 3, stride)
    xp = np.full((2, (Ho - 1) * stride + 3 + pt, (Wo - 1) * stride + 3 + pl, 4), -np.inf)
    xp[:, pt:pt + 9, pl:pl + 12] = x
    best, argl = np.full(y.shape, -np.inf), np.zeros(y.shape, np.uint8)
    for tap in range(9):
        v = xp[:, tap // 3:tap // 3 + (Ho - 1) * stride + 1:stride, tap % 3:tap % 3 + (Wo - 1) * stride + 1:stride]
        later = (v >= best) & np.isfinite(v)
        best, argl = np.where(later, v, best), np.where(later, tap, argl).astype(np.uint8)
    assert np.array_equal(best, y) and float((argl != arg).mean()) > 0.3
    for exact in (True, False):
        gy = R.int_tensor(y.shape, 2) if exact else np.random.RandomState(2).randn(*y.shape).astype(np.float32)
        gx, S = R.maxpool3_bwd(gy, arg, (9, 12), stride)
        bad = R.maxpool3_bwd(gy, argl, (9, 12), stride)[0]
        assert np.any(bad != gx) if exact else R.ratio(bad, gx, R.maxpool_bwd_bound(S)) > 1.0


def _lrn_wrong(x_row, C, r, bias, alpha, beta, clamp, dr):
    """tf.nn.lrn on rows of ld floats with the window clamped at ``clamp`` and the radius off by ``dr``"""
    x = R.f64(x_row)
    b, a, be = R.lrn_params(bias, alpha, beta)
    y = np.zeros(x.shape[:-1] + (C,))
    for c in range(C):
        lo, hi = max(c - r - dr, 0), min(c + r + dr, clamp)
        y[..., c] = x[..., c] * (b + a * (x[..., lo:hi + 1] ** 2).sum(axis=-1)) ** -be
    return y


@pytest.mark.parametrize("C,ld,r,bias,alpha,beta", [c for c in R.LRN_CASES if c[1] > c[0]])
def test_planted_lrn_defects_exceed_the_bound(C, ld, r, bias, alpha, beta):
    x, _ = R.lrn_inputs(C)
    row = np.full(x.shape[:3] + (ld,), 7.0, np.float32)             # non-zero pad channels
    row[..., :C] = x
    y, _ = R.lrn(x, r, bias, alpha, beta)
    bound = R.lrn_bound(y, r, beta)
    assert R.ratio(_lrn_wrong(row, C, r, bias, alpha, beta, C - 1, 0), y, bound) < 1e-3
    if r > 0:
        assert R.ratio(_lrn_wrong(row, C, r, bias, alpha, beta, C, 0), y, bound) > 1e3       # clamped at C
    if r < C:
        assert R.ratio(_lrn_wrong(row, C, r, bias, alpha, beta, C - 1, 1), y, bound) > 1e3   # radius + 1
    if 0 < r < C:
        assert R.ratio(_lrn_wrong(row, C, r, bias, alpha, beta, C - 1, -1), y, bound) > 1e3  # radius - 1


@pytest.mark.parametrize("C,ld,r,bias,alpha,beta", R.LRN_CASES)
def test_float32_restatement_of_lrn_is_inside_the_bounds(C, ld, r, bias, alpha, beta):
    """what float32 rounding alone does, with numpy's float32 power for the device's: 0.17 - 0.40 of the bounds"""
    x, gy = R.lrn_inputs(C)
    y, scale = R.lrn(x, r, bias, alpha, beta)
    y32, s32 = R.lrn32(x, r, bias, alpha, beta)
    fwd = R.ratio(y32, y, R.lrn_bound(y, r, beta))
    gx, bound = R.lrn_bwd(x, y32, s32, gy, r, alpha, beta)
    bwd = R.ratio(R.lrn_bwd32(x, y32, s32, gy, r, alpha, beta), gx, bound)
    print("LRN C=%d r=%d: float32 restatement at %.3f (forward), %.3f (adjoint) of the bound" % (C, r, fwd, bwd))
    assert 0.0 < fwd < 0.5 and 0.0 < bwd < 0.5
    # a window term dropped from the adjoint
    if r > 0:
        g2 = gy.copy()
        g2[..., 1] = 0
        dropped = R.lrn_bwd(x, y32, s32, g2, r, alpha, beta)[0]
        dropped[..., 1] = gx[..., 1]
        assert R.ratio(dropped, gx, bound) > 1e3


# ---- every GPU case against its conditions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,want", R.CONV_CASES, ids=[R.case_id(c) for c, _ in R.CONV_CASES])
def test_convolution_cases_take_the_path_they_are_there_for(case, want):
    from neural_flow_style_amd import _lib, ops
    kh, kw, stride, Ci, Co, B, H, W = case
    p = ops.conv2d_plan(B, H, W, Ci, Co, kh, kw, stride)
    last = p["nchunks"] - (p["ksplit"] - 1) * p["cps"]
    assert {k: p[k] for k in want if k != "last"} == {k: v for k, v in want.items() if k != "last"}, p
    assert last == want["last"] and 0 < last <= p["cps"], p
    assert p["nchunks"] == (-(-kh * kw // 4) if Ci <= 4 else kh * kw * -(-Ci // 16))
    M = B * R.same(H, kh, stride)[0] * R.same(W, kw, stride)[0]
    assert p["mtiles"] == -(-M // p["bm"]) and p["ntiles"] == -(-Co // 64)
    nws = _lib.lib().nfs_conv2d_workspace_floats(B, H, W, Ci, Co, kh, kw, stride)
    assert nws == (p["ksplit"] * M * p["ntiles"] * 64 if p["ksplit"] > 1 else 0)


def test_the_singled_out_paths_are_what_the_table_says():
    from neural_flow_style_amd import ops
    plans = {R.case_id(c): ops.conv2d_plan(c[5], c[6], c[7], c[3], c[4], c[0], c[1], c[2]) for c, _ in R.CONV_CASES}
    # 128-row tile in both chunk modes; M = 65 tiles + 65 rows: one row in the second half of the last tile
    big = [p for p in plans.values() if p["bm"] == 128]
    assert sorted(p["cmode"] for p in big) == [0, 1, 1] and 129 * 65 == 65 * 128 + 65
    assert all((p["mtiles"] * 128 // 128) * p["ntiles"] >= 512 for p in big)
    # every split after the first begins in the middle of a tap
    p = plans["k3x3-s1-272to64-b1-9x8"]
    assert p["ksplit"] == 16 and all((z * p["cps"]) % p["cchunks"] != 0 for z in range(1, p["ksplit"]))
    # odd cps, cps = 1, even cps, a shorter last split: the breaks of the two-chunk-unrolled pipeline
    cps = {p["cps"] for p in plans.values()}
    assert 1 in cps and any(c % 2 for c in cps if c > 1) and any(c % 2 == 0 for c in cps)
    assert any((p["nchunks"] - (p["ksplit"] - 1) * p["cps"]) % 2 != p["cps"] % 2 for p in plans.values() if p["ksplit"] > 1)
    # the data-gradient forms are split too, and Cout = 4 swaps into the 4-channel chunk mode
    d = [ops.conv2d_plan(c[5], c[6], c[7], c[3], c[4], c[0], c[1], 1) for c in map(R.dgrad_case, [c for c, _ in R.CONV_CASES
                                                                                                 if R.has_dgrad_form(c)])]
    assert sum(p["ksplit"] > 1 for p in d) >= 6 and sum(p["cmode"] for p in d) == 2


@pytest.mark.parametrize("name", sorted(R.GROUPS))
def test_groups_are_laid_out_as_the_table_says(name):
    from neural_flow_style_amd import _lib, ops
    B, shapes = R.GROUPS[name]
    plan = ops.conv2d_group_plan(R.placeholder_descs(_lib.ConvDesc, shapes), B)
    assert [tuple(p[k] for k in ("ksplit", "cps", "partial", "zbase", "ztotal", "position")) for p in plan] == R.GROUP_PLANS[name]
    assert sorted(p["position"] for p in plan) == list(range(len(shapes)))
    order = sorted(range(len(plan)), key=lambda j: plan[j]["position"])
    assert all(plan[a]["cps"] >= plan[b]["cps"] for a, b in zip(order, order[1:]))          # longest blocks first
    for run in R.group_runs([dict(summed=s[5]) for s in shapes]):
        assert [plan[j]["zbase"] for j in run] == list(np.cumsum([0] + [plan[j]["ksplit"] for j in run[:-1]]))
        assert {plan[j]["ztotal"] for j in run} == {sum(plan[j]["ksplit"] for j in run)}
        assert all(plan[j]["partial"] == int(len(run) > 1 or plan[j]["ksplit"] > 1) for j in run)
    flags = R.GROUP_FLAGS[name]
    assert len(flags) == len(shapes) and all(not (s[5] and set(f) & set("brp")) for s, f in zip(shapes, flags))


def test_the_group_table_reaches_what_it_is_there_for():
    P = R.GROUP_PLANS
    assert [p[5] for p in P["six"]] != sorted(p[5] for p in P["six"]) and max(p[0] for p in P["six"]) == 16
    assert [p[5] for p in P["fwd_5x5_pool_3x3"]] == [1, 2, 0]                              # reordered
    assert P["summed"][0][4] == 4 and P["summed"][1][5] == 0 and len({p[0] for p in P["summed"]}) > 1
    assert P["two_sizes"][1][2] == 0 and P["one_large"] == [(1, 9, 0, 0, 1, 0)]
    B, ((k, ci, co, H, W, _),) = R.GROUPS["one_large"]
    assert -(-B * H * W // 64) == 263


def test_a_follower_of_a_summed_run_that_carries_an_epilogue_is_refused():
    """the reduction takes bias, relu, y_pre and accumulate from the FIRST problem of a run: a follower's would be
    dropped without a word, so the planner refuses them -- except accumulate, which it ignores"""
    from neural_flow_style_amd import _lib, ops
    B, shapes = R.GROUPS["summed"]

    def descs():
        return R.placeholder_descs(_lib.ConvDesc, shapes)
    arr = descs()
    arr[0].bias, arr[0].relu, arr[0].y_pre, arr[0].ldp, arr[0].accumulate = 64, 1, 128, 192, 1     # the first may
    arr[1].accumulate = arr[2].accumulate = 1                                                   # ignored on a follower
    assert [p["ztotal"] for p in ops.conv2d_group_plan(arr, B)] == [4, 4, 4]
    assert _lib.lib().nfs_conv2d_group_workspace_floats(arr, 3, B) == 4 * B * 7 * 9 * 192
    for field, value in (("bias", 64), ("relu", 1), ("y_pre", 128)):
        arr = descs()
        setattr(arr[2], field, value)
        arr[2].ldp = 192
        with pytest.raises(_lib.NfsError, match="from its first problem"):
            ops.conv2d_group_plan(arr, B)
        assert _lib.lib().nfs_conv2d_group_workspace_floats(arr, 3, B) == -1
        # the launch refuses in the planner too, before anything is enqueued (no pointer is followed)
        with pytest.raises(_lib.NfsError, match="nfs_conv2d_group: a summed run"):
            _lib.call("nfs_conv2d_group", arr, 3, B, None, 0, None)
    with pytest.raises(_lib.NfsError, match="filter up to 7x7"):
        ops.conv2d_plan(1, 4, 4, 8, 8, 9, 9, 1)


@pytest.mark.parametrize("case", [c for c, _ in R.CONV_CASES], ids=R.case_id)
def test_convolution_inputs_are_exact_and_float32(case):
    for way in R.WAYS:
        if way == "dgrad" and not R.has_dgrad_form(case):
            continue
        d = R.conv_reference(case, True, way)
        assert R.exact_units(d["S"]) > 0
        r = R.conv_reference(case, False, way)
        for k in ("x", "gy", "w", "bias", "y_old", "mask"):
            if r.get(k) is not None:
                assert r[k].dtype == np.float32 and d[k].dtype == np.float32, k
        if way != "dgrad":
            assert float((r["x"] == 0).mean()) > 0.3 and float(r["x"].min()) == 0.0       # post-ReLU-like
        elif d["mask"] is not None:
            assert (d["mask"] == 0).any() and (d["mask"] < 0).any()


@pytest.mark.parametrize("name", sorted(R.GROUPS))
def test_group_inputs_are_exact_and_float32(name):
    for acc in (False, True):
        probs = R.group_problems(name, True, accumulate_first=acc)
        for run in R.group_runs(probs):
            assert R.exact_units(R.run_reference(probs, run)[2]) > 0
    for pr in R.group_problems(name, False):
        assert all(pr[k] is None or pr[k].dtype == np.float32 for k in ("x", "w", "bias", "mask", "y_old"))


@pytest.mark.parametrize("family", sorted(R.SMALL_DGRAD))
def test_small_data_gradient_cases_are_exact_and_reach_their_kernel(family):
    cases = R.SMALL_DGRAD[family]
    assert len(set(cases)) == len(cases)
    for case in cases:
        kh, kw, stride, Ci, Co, B, H, W, masked = case
        assert R.small_dgrad_kernel(case) == ("lds" if family == "lds" else "generic")
        assert 1 <= Ci <= 4 and Co % 4 == 0
        gy, w, act = R.small_dgrad_inputs(case, True)
        gx, S = R.conv2d_dgrad(gy, w, (H, W), stride, act=act)
        R.exact_units(S)
        assert R.dgrad_taps((H, W), kh, kw, stride).max() <= -(-kh // stride) * -(-kw // stride)
    if family != "generic_s1":
        # every parity class holds pixels somewhere, and the classes do differ in their taps
        assert len(np.unique(R.dgrad_taps((21, 30), 7, 7, 2))) == 3


def test_pool_adjoint_inputs_are_exact():
    for stride in (1, 2):
        for (H, W) in R.POOL_SHAPES:
            x = R.tie_tensor((2, H, W, 8), H + W)
            assert set(np.unique(x)) <= {0.0, 1.0, 2.0}
            y, arg = R.maxpool3(x, stride)
            gy = R.int_tensor(y.shape, 3)
            R.exact_units(R.maxpool3_bwd(gy, arg, (H, W), stride)[1], extra=3.0)


def test_decode_names_image_pixel_channel_and_tile():
    shape = (2, 5, 7, 130)
    flat = np.ravel_multi_index((1, 4, 6, 129), shape)
    assert R.decode(flat, shape, 64) == "image 1 at (4, 6) channel 129 -- row 5 of m-tile 1, column tile 2"
    got = np.zeros(shape)
    ref = got.copy()
    ref.reshape(-1)[flat] = 1.0
    assert "image 1 at (4, 6) channel 129" in R.first_mismatches(got, ref, 0.5, 64)
    assert R.first_mismatches(got, got, 0.0) == ""

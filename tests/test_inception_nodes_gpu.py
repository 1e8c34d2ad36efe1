"""The node kernels of the Inception-v1 loss network (csrc/inception.hip) element by element against the float64
restatements of tests/inception_ref.py: equality on integer inputs, the derived per-element bound on realistic ones,
operands as channel ranges of wider rows whose other floats must come back bit-identical.  The cases, the paths they are
there for and the bounds are tests/inception_ref.py's; tests/test_inception_ref_cpu.py holds them to their conditions.
Every check prints its largest error / bound ("ratio <family> ...") before it asserts."""
import itertools

import numpy as np
import pytest
import torch

from tests import inception_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = pytest.mark.parametrize("exact", [True, False], ids=["int", "real"])


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def rows(a, ld, c0, fill):
    """[B,H,W,C] as the channel range c0.. of rows of ld floats; the other floats differ from channel to channel"""
    a = np.asarray(a, np.float32)
    buf = np.empty(a.shape[:3] + (ld,), np.float32)
    buf[...] = fill + 0.25 * np.arange(ld, dtype=np.float32)
    buf[..., c0:c0 + a.shape[3]] = a
    return dev(buf)


def bits(t):
    return t.contiguous().view(torch.int32)


def untouched(after, before, ranges=()):
    """every float outside the channel ranges [(c0, C)] is bit-identical"""
    keep = torch.ones(after.shape[-1], dtype=torch.bool, device=after.device)
    for c0, C in ranges:
        keep[c0:c0 + C] = False
    return torch.equal(bits(after[..., keep]), bits(before[..., keep]))


def check(got, ref, bound, exact, family, what, bm=64):
    got = host(got)
    print("ratio %s %s %s: %.4f" % (family, what, "int" if exact else "real", R.ratio(got, ref, bound)))
    report = R.first_mismatches(got, ref, 0.0 if exact else bound, bm)
    assert not report, "%s (%s)\n%s" % (what, "equality" if exact else "bound", report)


class Scratch:
    """a workspace of n floats between two guard pads"""
    PAD = 32

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * self.PAD,), 11.0, device=DEV) if n > 0 else None

    @property
    def ptr(self):
        return None if self.buf is None else self.buf.data_ptr() + 4 * self.PAD

    def pads_untouched(self):
        if self.buf is None:
            return True
        want = torch.full((self.PAD,), 11.0, device=DEV)
        return torch.equal(bits(self.buf[:self.PAD]), bits(want)) and torch.equal(bits(self.buf[self.PAD + self.n:]), bits(want))


def conv_raw(x, cx, Cin, packed, bias, y, cy, Cout, kh, kw, stride, relu, accumulate, scratch, mask=None, cm=0):
    """nfs_conv2d_fwd with a workspace of the test's own (None: without one)"""
    from neural_flow_style_amd import _lib, ops
    B, H, W, ldx = x.shape
    _lib.call("nfs_conv2d_fwd", x.data_ptr() + 4 * cx, ldx, None if mask is None else mask.data_ptr() + 4 * cm,
              0 if mask is None else mask.shape[3], packed.data_ptr(), None if bias is None else bias.data_ptr(),
              y.data_ptr() + 4 * cy, y.shape[3], None, 0, B, H, W, Cin, Cout, kh, kw, stride, int(relu), int(accumulate),
              None if scratch is None else scratch.ptr, 0 if scratch is None else scratch.n, ops._stream())


# ---- the implicit GEMM -----------------------------------------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("case", [c for c, _ in R.CONV_CASES], ids=R.case_id)
def test_conv2d_bias_relu_and_the_value_before_it(case, exact):
    from neural_flow_style_amd import ops
    kh, kw, stride, Ci, Co, B, H, W = case
    p = ops.conv2d_plan(B, H, W, Ci, Co, kh, kw, stride)
    d = R.conv_reference(case, exact, "bias_relu_pre")
    if exact:
        R.exact_units(d["S"])
    xb = rows(d["x"], Ci + 8, 4, 7.0)
    yb, pb = rows(np.zeros_like(d["y"]), Co + 12, 8, -3.0), rows(np.zeros_like(d["y"]), Co + 8, 4, 5.0)
    x0, y0, p0 = xb.clone(), yb.clone(), pb.clone()
    packed = ops.conv2d_pack(dev(d["w"]))
    ops.conv2d_fwd(xb, 4, Ci, packed, dev(d["bias"]), yb, 8, Co, kh, kw, stride, relu=True, y_pre=pb, cp=4)
    what = R.case_id(case)
    check(pb[..., 4:4 + Co], d["pre"], R.gemm_bound(d["S"], d["n"], p["ksplit"], d["pre"]), exact, "conv2d", what + " y_pre",
          p["bm"])
    check(yb[..., 8:8 + Co], d["y"], R.gemm_bound(d["S"], d["n"], p["ksplit"], d["y"]), exact, "conv2d", what + " y", p["bm"])
    assert untouched(yb, y0, [(8, Co)]) and untouched(pb, p0, [(4, Co)]) and untouched(xb, x0)


@KINDS
@pytest.mark.parametrize("case", [c for c, _ in R.CONV_CASES], ids=R.case_id)
def test_conv2d_accumulates_onto_a_non_zero_output(case, exact):
    """no bias, no ReLU, through the raw call with a workspace between guard pads; the two-split case also without one"""
    from neural_flow_style_amd import _lib, ops
    kh, kw, stride, Ci, Co, B, H, W = case
    p = ops.conv2d_plan(B, H, W, Ci, Co, kh, kw, stride)
    d = R.conv_reference(case, exact, "accumulate")
    if exact:
        R.exact_units(d["S"])
    xb = rows(d["x"], Ci + 12, 8, 7.0)
    packed = ops.conv2d_pack(dev(d["w"]))
    nws = _lib.lib().nfs_conv2d_workspace_floats(B, H, W, Ci, Co, kh, kw, stride)
    assert (nws > 0) == (p["ksplit"] > 1)
    for scratch, Z in [(Scratch(nws), p["ksplit"])] + ([(None, 1)] if case == R.NO_WORKSPACE_CASE else []):
        yb = rows(d["y_old"], Co + 8, 4, -3.0)
        y0 = yb.clone()
        conv_raw(xb, 8, Ci, packed, None, yb, 4, Co, kh, kw, stride, False, True, scratch)
        what = "%s accumulate%s" % (R.case_id(case), "" if scratch is not None else " without a workspace")
        check(yb[..., 4:4 + Co], d["y"], R.gemm_bound(d["S"], d["n"], Z, d["y"]), exact, "conv2d", what, p["bm"])
        assert untouched(yb, y0, [(4, Co)]) and (scratch is None or scratch.pads_untouched())


@KINDS
@pytest.mark.parametrize("case", [c for c, _ in R.CONV_CASES if R.has_dgrad_form(c)], ids=R.case_id)
def test_conv2d_data_gradient_form_masks_while_it_loads(case, exact):
    """filters packed transposed, Cin and Cout swapped, the ReLU mask (exact zeros of both signs, negatives) applied to
    the gradient as it is read; against the adjoint written as a sum over output pixels"""
    from neural_flow_style_amd import ops
    kh, kw, stride, Ci, Co, B, H, W = case
    p = ops.conv2d_plan(B, H, W, Co, Ci, kh, kw, 1)
    d = R.conv_reference(case, exact, "dgrad")
    if exact:
        R.exact_units(d["S"])
    gb = rows(d["gy"], Co + 8, 4, 7.0)
    mb = None if d["mask"] is None else rows(d["mask"], Co + 12, 8, 1.0)
    xb = rows(np.zeros_like(d["y"]), Ci + 12, 8, -3.0)
    x0, g0 = xb.clone(), gb.clone()
    packed = ops.conv2d_pack(dev(d["w"]), transpose=True)
    ops.conv2d_fwd(gb, 4, Co, packed, None, xb, 8, Ci, kh, kw, 1, relu=False, x_mask=mb, cm=8)
    check(xb[..., 8:8 + Ci], d["y"], R.gemm_bound(d["S"], d["n"], p["ksplit"], d["y"]), exact, "conv2d_dgrad_form",
          R.case_id(case), p["bm"])
    assert untouched(xb, x0, [(8, Ci)]) and untouched(gb, g0)


# ---- grouped launches ------------------------------------------------------------------------------------------------------
# where a problem writes when it is not a buffer of its own: (buffer, floats per pixel, first channel) -- the branches of a
# module write into channel ranges of its concatenated output
GROUP_LAYOUT = {
    "fwd_1x1": {0: ("out", 264, 0)},
    "fwd_5x5_pool_3x3": {0: ("out", 264, 192), 1: ("out", 264, 224), 2: ("out", 264, 64)},
}


def _group_buffers(name, probs):
    """device operands of a group: per problem the dict ops.conv2d_group takes; the output buffers by name with the
    channel ranges that are written"""
    from neural_flow_style_amd import ops
    layout, outs, written, dicts = GROUP_LAYOUT.get(name, {}), {}, {}, []
    B = R.GROUPS[name][0]
    for j, pr in enumerate(probs):
        if pr["summed"]:
            key, ld, cy = dicts[-1]["_key"], dicts[-1]["y"].shape[3], dicts[-1]["cy"]
        else:
            key, ld, cy = layout.get(j, ("y%d" % j, pr["Co"] + 12, 8))
            if key not in outs:
                outs[key] = rows(np.zeros((B, pr["H"], pr["W"], 0)), ld, 0, -3.0)
                written[key] = []
            if pr["y_old"] is not None:
                outs[key][..., cy:cy + pr["Co"]] = dev(pr["y_old"])
            written[key].append((cy, pr["Co"]))
        q = dict(x=rows(pr["x"], pr["Ci"] + 8, 4, 7.0), cx=4, Cin=pr["Ci"], k=pr["k"], y=outs[key], cy=cy, Cout=pr["Co"],
                 packed=ops.conv2d_pack(dev(pr["w"]), transpose="d" in pr["flags"]),
                 bias=None if pr["bias"] is None else dev(pr["bias"]), relu="r" in pr["flags"],
                 accumulate="a" in pr["flags"], sum_with_prev=pr["summed"], _key=key)
        if pr["mask"] is not None:
            q.update(x_mask=rows(pr["mask"], pr["Ci"] + 12, 8, 1.0), cm=8)
        if "p" in pr["flags"]:
            q.update(y_pre=rows(np.zeros((B, pr["H"], pr["W"], pr["Co"])), pr["Co"] + 8, 4, 5.0), cp=4)
        dicts.append(q)
    return dicts, outs, written


@KINDS
@pytest.mark.parametrize("name,acc", [(n, False) for n in sorted(R.GROUPS)] + [("summed", True)])
def test_grouped_launch_every_output_of_every_problem(name, acc, exact):
    from neural_flow_style_amd import _lib, ops
    probs = R.group_problems(name, exact, accumulate_first=acc)
    B = R.GROUPS[name][0]
    dicts, outs, written = _group_buffers(name, probs)
    before = {k: v.clone() for k, v in outs.items()}
    pre0 = {j: q["y_pre"].clone() for j, q in enumerate(dicts) if "y_pre" in q}
    arr, n, _ = ops.conv2d_group_descs(dicts)
    plan = ops.conv2d_group_plan(arr, B)
    assert [tuple(p[k] for k in ("ksplit", "cps", "partial", "zbase", "ztotal", "position")) for p in plan] == R.GROUP_PLANS[name]
    nws = _lib.lib().nfs_conv2d_group_workspace_floats(arr, n, B)
    scratch = Scratch(nws)
    _lib.call("nfs_conv2d_group", arr, n, B, scratch.ptr, scratch.n, ops._stream())
    # the same problems one by one: a follower of a run accumulates
    singles, souts, _ = _group_buffers(name, probs)
    for q, pr in zip(singles, probs):
        ops.conv2d_fwd(q["x"], 4, q["Cin"], q["packed"], q["bias"], q["y"], q["cy"], q["Cout"], q["k"], q["k"], 1,
                       relu=q["relu"], y_pre=q.get("y_pre"), cp=4, x_mask=q.get("x_mask"), cm=8,
                       accumulate=q["accumulate"] or pr["summed"])
    for run in R.group_runs(probs):
        j0 = run[0]
        pre, y, S, nprod = R.run_reference(probs, run)
        if exact:
            R.exact_units(S)
        Z = plan[j0]["ztotal"] if plan[j0]["partial"] else 1
        q, Co = dicts[j0], probs[j0]["Co"]
        what = "%s%s run %s" % (name, " accumulated" if acc else "", run)
        got = q["y"][..., q["cy"]:q["cy"] + Co]
        bound = R.gemm_bound(S, nprod, Z, y)
        check(got, y, bound, exact, "conv2d_group", what + " y")
        if "y_pre" in q:
            check(q["y_pre"][..., 4:4 + Co], pre, R.gemm_bound(S, nprod, Z, pre), exact, "conv2d_group", what + " y_pre")
            assert untouched(q["y_pre"], pre0[j0], [(4, Co)])
        Zs = sum(ops.conv2d_plan(B, probs[j]["H"], probs[j]["W"], probs[j]["Ci"], Co, probs[j]["k"], probs[j]["k"], 1)["ksplit"]
                 for j in run) + len(run)
        single = singles[j0]["y"][..., q["cy"]:q["cy"] + Co]
        check(got, R.f64(host(single)), bound + R.gemm_bound(S, nprod, Zs, y), exact, "conv2d_group_vs_single", what)
    for key in outs:
        assert untouched(outs[key], before[key], written[key]), key
    assert scratch.pads_untouched()


# ---- the data gradient down to the image -------------------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("family,ci", [("lds", 1), ("lds", 2), ("lds", 3), ("lds", 4), ("generic_s2", None),
                                       ("generic_s1", None)])
def test_conv2d_dgrad_small(family, ci, exact):
    from neural_flow_style_amd import ops
    worst = 0.0
    for case in R.SMALL_DGRAD[family]:
        kh, kw, stride, Ci, Co, B, H, W, masked = case
        if ci is not None and Ci != ci:
            continue
        gy, w, act = R.small_dgrad_inputs(case, exact)
        gx, S = R.conv2d_dgrad(gy, w, (H, W), stride, act=act)
        gb = rows(gy, Co + 8, 4, 7.0)
        ab = None if act is None else rows(act, Co + 12, 8, 1.0)
        g0 = gb.clone()
        got = host(ops.conv2d_dgrad_small(gb, 4, Co, dev(w), (H, W), stride, y_act=ab, ca=8))
        bound = R.gemm_bound(S, R.dgrad_taps((H, W), kh, kw, stride)[None, :, :, None] * Co, 1, gx)
        worst = max(worst, R.ratio(got, gx, bound))
        report = R.first_mismatches(got, gx, 0.0 if exact else bound)
        assert not report, "%r\n%s" % (case, report)
        assert untouched(gb, g0)
    print("ratio conv2d_dgrad_small %s%s %s: %.4f" % (family, "" if ci is None else " Ci=%d" % ci, "int" if exact else "real",
                                                       worst))


# ---- pools, LRN, mask-add ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
def test_maxpool3_ties_go_to_the_first_maximum_byte_for_byte(stride):
    from neural_flow_style_amd import ops
    worst = 0.0
    for (H, W), C in itertools.product(R.POOL_SHAPES, R.POOL_CHANNELS):
        x = R.tie_tensor((2, H, W, C), H * 131 + W * 7 + C)
        y, arg = R.maxpool3(x, stride)
        xb = dev(x)
        yo, ao = ops.maxpool3_fwd(xb, stride)
        what = "stride %d, %d x %d x %d" % (stride, H, W, C)
        assert not R.first_mismatches(host(yo), y, 0.0), what
        assert ao.dtype == torch.uint8 and not R.first_mismatches(host(ao), arg, 0.0), what + " arg"
        for exact in (True, False):
            gy = R.int_tensor(y.shape, C + H) if exact else np.random.RandomState(C + H).randn(*y.shape).astype(np.float32)
            old = R.int_tensor(x.shape, C + W + 1) if exact else np.random.RandomState(W).randn(*x.shape).astype(np.float32)
            for gx_old, relu_of in itertools.product((None, old), (None, x)):
                gx, S = R.maxpool3_bwd(gy, arg, (H, W), stride, gx_old=gx_old, relu_of=relu_of)
                if exact:
                    R.exact_units(S, extra=3.0)
                got = host(ops.maxpool3_bwd(dev(gy), ao, (H, W), stride, gx=None if gx_old is None else dev(gx_old),
                                            relu_of=None if relu_of is None else xb))
                bound = R.maxpool_bwd_bound(S, gx_old)
                worst = max(worst, 0.0 if exact else R.ratio(got, gx, bound))
                report = R.first_mismatches(got, gx, 0.0 if exact else bound)
                assert not report, "%s adjoint%s%s\n%s" % (what, "" if gx_old is None else " accumulated",
                                                           "" if relu_of is None else " relu_of", report)
    print("ratio maxpool3_bwd stride %d real: %.4f" % (stride, worst))


@pytest.mark.parametrize("k,H,W", R.AVGPOOL_CASES)
def test_avgpool_valid_and_its_adjoint(k, H, W):
    from neural_flow_style_amd import ops
    rng = np.random.RandomState(k * 10 + W)
    x = np.maximum(rng.randn(2, H, W, 8), 0).astype(np.float32) * np.float32(30)
    y, S = R.avgpool_valid(x, k)
    check(ops.avgpool_valid_fwd(dev(x), k), y, R.avgpool_bound(S, k), False, "avgpool_valid", "k %d forward" % k)
    gy = rng.randn(*y.shape).astype(np.float32)
    gx, Sg = R.avgpool_valid_bwd(gy, (H, W), k)
    check(ops.avgpool_valid_bwd(dev(gy), (H, W), k), gx, R.avgpool_bound(Sg, k), False, "avgpool_valid", "k %d adjoint" % k)
    old = rng.randn(*x.shape).astype(np.float32)
    gxa, _ = R.avgpool_valid_bwd(gy, (H, W), k, gx_old=old)
    check(ops.avgpool_valid_bwd(dev(gy), (H, W), k, gx=dev(old)), gxa, R.avgpool_bound(Sg, k, gxa), False, "avgpool_valid",
          "k %d adjoint accumulated" % k)


@pytest.mark.parametrize("C,ld,r,bias,alpha,beta", R.LRN_CASES)
def test_lrn_and_its_adjoint_on_the_kernel_s_own_forward(C, ld, r, bias, alpha, beta):
    from neural_flow_style_amd import ops
    x, gy = R.lrn_inputs(C)
    xb, gb = rows(x, ld, 0, 9.0), rows(gy, ld, 0, -4.0)              # non-zero pad channels
    y, scale = R.lrn(x, r, bias, alpha, beta)
    yo, so = ops.lrn_fwd(xb, C, r, bias, alpha, beta)
    what = "C %d ld %d r %d" % (C, ld, r)
    check(yo[..., :C], y, R.lrn_bound(y, r, beta), False, "lrn", what + " forward")
    check(so[..., :C], scale, 1.01 * (2 * r + 3) * R.U * scale, False, "lrn", what + " scale")
    assert float(yo[..., C:].abs().sum()) == 0                      # the pad of y as ops.lrn_fwd defines it
    so[..., C:] = float("nan")                                      # the pad of scale is not read
    y_own, s_own = host(yo)[..., :C], host(so)[..., :C]
    gx, bound = R.lrn_bwd(x, y_own, s_own, gy, r, alpha, beta)
    got = ops.lrn_bwd(xb, yo, so, gb, C, r, alpha, beta)
    check(got[..., :C], gx, bound, False, "lrn", what + " adjoint")
    assert float(got[..., C:].abs().sum()) == 0
    old = np.random.RandomState(r).randn(*x.shape).astype(np.float32)
    ob = rows(old, ld, 0, 6.0)
    o0 = ob.clone()
    gxa, bounda = R.lrn_bwd(x, y_own, s_own, gy, r, alpha, beta, gx_old=old)
    assert ops.lrn_bwd(xb, yo, so, gb, C, r, alpha, beta, gx=ob) is ob
    check(ob[..., :C], gxa, bounda, False, "lrn", what + " adjoint accumulated")
    assert untouched(ob, o0, [(0, C)])


@KINDS
def test_relu_mask_add_every_combination_the_call_accepts(exact):
    """g, g + act, g + addend, g + act + addend, addend, act + addend (act alone and nothing at all are refused: there
    would be nothing to write); each operand and out with a row stride and an offset of its own"""
    from neural_flow_style_amd import _lib, ops
    B, H, W, C = 2, 9, 11, 24
    if exact:
        g, add = R.int_tensor((B, H, W, C), 1), R.int_tensor((B, H, W, C), 2)
    else:
        rng = np.random.RandomState(3)
        g, add = rng.randn(B, H, W, C).astype(np.float32), (rng.randn(B, H, W, C) * 1e-3).astype(np.float32)
    act = R.mask_tensor((B, H, W, C), 4)
    assert np.signbit(act[act == 0]).any() and (~np.signbit(act[act == 0])).any() and (act < 0).any()
    gb, ab, db = rows(g, C + 8, 4, 7.0), rows(act, C + 12, 8, 1.0), rows(add, C + 4, 0, 2.0)
    for use in [(1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1), (0, 0, 1), (0, 1, 1)]:
        ob = rows(np.zeros((B, H, W, 0)), C + 16, 12, -3.0)
        o0 = ob.clone()
        ops.relu_mask_add(gb if use[0] else None, 4, ab if use[1] else None, 8, db if use[2] else None, 0, C, out=ob, co=12)
        want = R.relu_mask_add(g if use[0] else None, act if use[1] else None, add if use[2] else None)
        assert np.array_equal(host(ob[..., 12:12 + C]), want), use
        assert untouched(ob, o0, [(12, C)]), use
    ob = rows(np.zeros((B, H, W, 0)), C + 16, 12, -3.0)
    o0 = ob.clone()
    for pa, la in ((ab.data_ptr() + 32, C + 12), (None, 0)):
        with pytest.raises(_lib.NfsError, match="null pointer"):
            _lib.call("nfs_relu_mask_add", None, 0, pa, la, None, 0, ob.data_ptr() + 48, C + 16, B * H * W, C, ops._stream())
    assert untouched(ob, o0)

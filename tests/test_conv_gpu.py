"""The VGG 3x3 convolution chain (vgg.hip, winograd.hip, winograd_fused.hip, winograd5.hip) element by element against the
float64 restatement of tests/conv_ref.py.

Every case
  1. asserts through nfs_conv3x3_plan that it runs the path it is named for,
  2. hands in outputs pre-filled with NaN (an element the kernel does not write cannot pass),
  3. fills the shared conv workspace with NaN first (a result must not depend on stale V / M),
  4. names the first entries outside their bound as (image, tile, position in tile, channel).

Exact inputs (integers; the direct kernels, and every Winograd path with zero filters) must EQUAL float64.  Realistic
inputs must stay inside the derived worst-case bound of conv_ref's header at every element, in both arithmetics of the
batched GEMM; on the cases of at most 300 tiles the kernel's max err / bound may be at most 8 x that of the float32 numpy
restatement of the same algorithm on the same input.  ``pytest -s`` prints the ratios (docs/kernels/convolution.md).
The last test asserts that the cases together ran every path the launch code can reach.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

PRECISION_FACTOR = 8.0
_SEEN = set()       # (family, direction, form, whole | ragged, schedules, K parts, extra) recorded after a case passed
_BATCHED = ("wg4_three", "wg5")


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def poison_workspace(ops, B, H, W, Ci, Co):
    from neural_flow_style_amd import _lib
    want = _lib.lib().nfs_conv3x3_workspace_floats(B, H, W, Ci, Co)
    if want > 0:
        ops.conv_workspace(torch.device("cuda", torch.cuda.current_device()), want).fill_(float("nan"))


def gemm_last():
    from neural_flow_style_amd import _lib
    buf = (ctypes.c_longlong * 11)()
    _lib.call("nfs_gemm_last", buf)
    return dict(zip(("variant", "bm", "bn", "nbuf", "pre", "ksplit", "T", "K", "N", "Z", "trialled"), (int(v) for v in buf)))


def expect(ops, B, H, W, K, N, pooled, key):
    p = ops.conv3x3_plan(B, H, W, K, N, pooled)
    assert R.plan_key(p) == key, "the case is named for %s, the launch code runs %s" % (key, R.plan_key(p))
    return p


def seen(key, direction, form, extra=None):
    family, ragged, sched, k = key.split("/")
    _SEEN.add((family, direction, form, ragged, sched, k, extra))


def inside(what, got, ref, bound, m):
    """every element of ``got`` within ``bound`` of ``ref`` (no NaN left); prints and returns max err / bound"""
    got = host(got)
    report = R.first_mismatches(got, ref, bound, m)
    assert not report, "%s\n%s" % (what, report)
    r = R.err_ratio(np.abs(got - ref), bound)
    print("  %-58s max err / bound %.5f" % (what, r))
    return r


def equal(what, got, ref, m):
    got = host(got)
    report = R.first_mismatches(got, ref, 0.0, m)
    assert not report, "%s\n%s" % (what, report)


def modes_of(*keys):
    """both arithmetics of the batched GEMM where one runs, else the current one alone"""
    return (0, 1) if any(k.split("/")[0] in _BATCHED for k in keys) else (None,)


class gemm_mode:
    def __init__(self, ops, mode):
        self.ops, self.mode = ops, mode

    def __enter__(self):
        self.prev = self.ops.gemm_mode(self.mode) if self.mode is not None else None

    def __exit__(self, *exc):
        if self.prev is not None:
            self.ops.gemm_mode(self.prev)


def single_extra(key, K, N):
    return (K, N) if key.startswith("wg4_single") else None


def _ids(cases):
    return ["x".join(str(v) for v in c[0]) for c in cases]


# ---- realistic inputs: plain layers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,key_f,key_g", R.PLAIN_LAYERS, ids=_ids(R.PLAIN_LAYERS))
def test_plain_layer_inside_its_bound(ops, shape, key_f, key_g):
    B, H, W, Ci, Co = shape
    pf = expect(ops, B, H, W, Ci, Co, 0, key_f)
    pg = expect(ops, B, H, W, Co, Ci, 0, key_g)
    mf, mg = R.tile_of(key_f), R.tile_of(key_g)
    d = R.layer_inputs(shape)
    x, w, bias, gy, add = d["x"], d["w"], d["bias"], d["gy"], d["addend"]
    # float64, once
    pre, _ = R.conv(x, w, bias)
    y = np.maximum(pre, 0.0)
    by = R.wino_bound(x, w, mf, y)
    wd = R.dgrad_filters(w)
    g, _ = R.conv(gy, wd)
    mask = x > 0
    g_m, g_u = R.layer_dgrad(g, mask=mask, addend=add), R.layer_dgrad(g, mask=mask, addend=add, addend_unmasked=True)
    bg = R.wino_bound(gy, wd, mg, 0.0)                                     # (+ u |gx| per form below)
    u = R.U
    X, Wt, Bias, GY, ADD = dev(x), dev(w), dev(bias), dev(gy), dev(add)
    wf, wdp = ops.conv3x3_pack(Wt, 0), ops.conv3x3_pack(Wt, 1)
    ratios = {}
    print("\n%s  fwd %s  dgrad %s" % (shape, key_f, key_g))
    for mode in modes_of(key_f, key_g):
        with gemm_mode(ops, mode):
            tag = "" if mode is None else "[gemm_mode %d] " % mode
            poison_workspace(ops, B, H, W, Ci, Co)
            out = ops.conv3x3_fwd(X, wf, Bias, Co, relu=True, out=nan(B, H, W, Co))
            if pf["family"] in _BATCHED:
                last = gemm_last()
                assert (last["Z"], last["T"], last["K"], last["N"], last["ksplit"]) == \
                    (pf["Z"], pf["tiles"], Ci, Co, pf["kparts"]), (last, pf)
            ratios["fwd", mode] = inside(tag + "y = relu(conv + bias)", out, y, by, mf)
            rb = ops.conv3x3_relu_bits(B, H, W, Ci, Co, False, X.device)
            assert rb is not None
            rb.fill_(float("nan"))
            poison_workspace(ops, B, H, W, Ci, Co)
            out_b = ops.conv3x3_fwd(X, wf, Bias, Co, relu=True, out=nan(B, H, W, Co), relu_bits=rb)
            assert torch.equal(out, out_b), "recording the ReLU bit cache changed y"
            # data gradient: plain, masked + addend from the float mask and from the bit cache, addend_unmasked
            poison_workspace(ops, B, H, W, Ci, Co)
            gx = ops.conv3x3_dgrad(GY, wdp, Ci, out=nan(B, H, W, Ci))
            if pg["family"] in _BATCHED:
                last = gemm_last()
                assert (last["Z"], last["T"], last["K"], last["N"], last["ksplit"]) == \
                    (pg["Z"], pg["tiles"], Co, Ci, pg["kparts"]), (last, pg)
            ratios["dgrad", mode] = inside(tag + "gx = dgrad(gy)", gx, g, bg + u * np.abs(g), mg)
            poison_workspace(ops, B, H, W, Ci, Co)
            gx_m = ops.conv3x3_dgrad(GY, wdp, Ci, x_in=X, addend=ADD, out=nan(B, H, W, Ci))
            inside(tag + "gx = dgrad(gy) (x_in > 0) + addend", gx_m, g_m, (bg + u * np.abs(g_m)) * mask, mg)
            poison_workspace(ops, B, H, W, Ci, Co)
            gx_b = ops.conv3x3_dgrad(GY, wdp, Ci, x_in=X, addend=ADD, out=nan(B, H, W, Ci), relu_bits=rb)
            assert torch.equal(gx_m, gx_b), "the bit-cache data gradient differs from the float-mask one"
            poison_workspace(ops, B, H, W, Ci, Co)
            gx_u = ops.conv3x3_dgrad(GY, wdp, Ci, x_in=X, addend=ADD, out=nan(B, H, W, Ci), addend_unmasked=True)
            inside(tag + "gx = (dgrad(gy) + addend) (x_in > 0)", gx_u, g_u, (bg + u * np.abs(g_u)) * mask, mg)
    # precision: the float32 restatement of the same algorithm on the same input sets the threshold
    ch = slice(0, R.RESTATED_CHANNELS)
    if R.tiles(shape, mf) <= R.PRECISION_TILES:
        y32 = np.maximum(R.winograd32(x, w, mf, ch) + bias[ch], np.float32(0))
        r32 = R.err_ratio(np.abs(R.f64(y32) - y[..., ch]), by[..., ch])
        print("  %-58s max err / bound %.5f" % ("float32 restatement, forward", r32))
        for mode in modes_of(key_f, key_g):
            assert ratios["fwd", mode] <= PRECISION_FACTOR * r32, (mode, ratios["fwd", mode], r32)
    if R.tiles(shape, mg) <= R.PRECISION_TILES:
        g32 = R.winograd32(gy, wd.astype(np.float32), mg, ch)
        r32 = R.err_ratio(np.abs(R.f64(g32) - g[..., ch]), (bg + u * np.abs(g))[..., ch])
        print("  %-58s max err / bound %.5f" % ("float32 restatement, data gradient", r32))
        for mode in modes_of(key_f, key_g):
            assert ratios["dgrad", mode] <= PRECISION_FACTOR * r32, (mode, ratios["dgrad", mode], r32)
    seen(key_f, "fwd", "plain", single_extra(key_f, Ci, Co))
    seen(key_g, "dgrad", "plain", single_extra(key_g, Co, Ci))


# ---- realistic inputs: pooled layers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,key_f,key_g,key_gf", R.POOLED_LAYERS, ids=_ids(R.POOLED_LAYERS))
def test_pooled_layer_inside_its_bound(ops, shape, key_f, key_g, key_gf):
    B, H, W, Ci, Co = shape
    expect(ops, B, H, W, Ci, Co, 1, key_f)
    expect(ops, B, H, W, Co, Ci, 1, key_g)
    expect(ops, B, H, W, Co, Ci, 2, key_gf)
    d = R.layer_inputs(shape, pooled=True)
    x, w, bias, gyp, add = d["x"], d["w"], d["bias"], d["gy"], d["addend"]
    pre, _ = R.conv(x, w, bias)
    y = np.maximum(pre, 0.0)
    by = R.wino_bound(x, w, 4, y)
    yp = R.avgpool2(y)
    bp = R.pool_bound(by, yp)
    und = R.undecided(pre, by)
    assert und.mean() <= R.UNDECIDED_CAP
    wd = R.dgrad_filters(w)
    mask = x > 0
    u = R.U
    X, Wt, Bias, GYP, ADD = dev(x), dev(w), dev(bias), dev(gyp), dev(add)
    wf, wdp = ops.conv3x3_pack(Wt, 0), ops.conv3x3_pack(Wt, 1)
    print("\n%s pooled  fwd %s  dgrad %s (bits) %s (float)  undecided %.4f" % (shape, key_f, key_g, key_gf, und.mean()))
    ratios = {}
    for mode in modes_of(key_f, key_g):
        with gemm_mode(ops, mode):
            tag = "" if mode is None else "[gemm_mode %d] " % mode
            poison_workspace(ops, B, H, W, Ci, Co)
            y_k, p_k = ops.conv3x3_fwd_pool(X, wf, Bias, Co, relu=True, out=nan(B, H, W, Co), out_pool=nan(B, H // 2, W // 2, Co))
            ratios[mode] = inside(tag + "y = relu(conv + bias)", y_k, y, by, 4)
            inside(tag + "y_pool = avgpool2(y)", p_k, yp, bp, 2)
            # the mask rule: where the float64 pre-activation is clear of zero by its bound, the kernel's mask is the reference's
            mk = host(y_k) > 0
            wrong = (mk != (pre > 0)) & ~und
            assert not wrong.any(), "a decided ReLU mask differs: first at %s" % R.decode(np.flatnonzero(wrong)[0], pre.shape, 4)
            # the bit cache: the same y and pool, with the full-resolution output and without it
            rb = ops.conv3x3_relu_bits(B, H, W, Ci, Co, True, X.device)
            assert rb is not None
            rb.fill_(float("nan"))
            poison_workspace(ops, B, H, W, Ci, Co)
            y_b, p_b = ops.conv3x3_fwd_pool(X, wf, Bias, Co, relu=True, relu_bits=rb, out=nan(B, H, W, Co),
                                            out_pool=nan(B, H // 2, W // 2, Co))
            assert torch.equal(y_b, y_k) and torch.equal(p_b, p_k), "recording the ReLU bit cache changed y or y_pool"
            rb2 = torch.full_like(rb, float("nan"))
            poison_workspace(ops, B, H, W, Ci, Co)
            y_n, p_n = ops.conv3x3_fwd_pool(X, wf, Bias, Co, relu=True, relu_bits=rb2, want_y=False,
                                            out_pool=nan(B, H // 2, W // 2, Co))
            assert y_n is None and torch.equal(p_n, p_k), "y_pool without y differs"
            assert torch.equal(rb2.view(torch.int32), rb.view(torch.int32)), "the bit cache without y differs"
            # the pooled gradient: only on undecided entries does the reference take the kernel's own mask
            g_y = R.pooled_gy(gyp, np.where(und, mk, pre > 0))
            g, _ = R.conv(g_y, wd)
            bg = R.wino_bound(g_y, wd, 4, 0.0)
            forms = [("gx = dgrad(g_y)", {}, g, bg + u * np.abs(g))]
            g_m = R.layer_dgrad(g, mask=mask, addend=add)
            forms.append(("gx = dgrad(g_y) (x_in > 0) + addend", dict(x_in=X, addend=ADD), g_m, (bg + u * np.abs(g_m)) * mask))
            g_u = R.layer_dgrad(g, mask=mask, addend=add, addend_unmasked=True)
            forms.append(("gx = (dgrad(g_y) + addend) (x_in > 0)", dict(x_in=X, addend=ADD, addend_unmasked=True), g_u,
                          (bg + u * np.abs(g_u)) * mask))
            for what, kw, ref, bound in forms:
                poison_workspace(ops, B, H, W, Ci, Co)
                q_f = ops.conv3x3_dgrad_pool(GYP, y_k, wdp, Ci, out=nan(B, H, W, Ci), **kw)
                inside(tag + what + ", float output", q_f, ref, bound, 4)
                if not kw:
                    q0 = q_f
                poison_workspace(ops, B, H, W, Ci, Co)
                q_b = ops.conv3x3_dgrad_pool(GYP, None, wdp, Ci, relu_bits=rb, hw=(H, W), out=nan(B, H, W, Ci), **kw)
                assert torch.equal(q_b, q_f), "%s: the bit-cache form differs from the float-mask form" % what
            if R.tiles(shape, 4) <= R.PRECISION_TILES:
                ch = slice(0, R.RESTATED_CHANNELS)
                g32 = R.winograd32(g_y, wd.astype(np.float32), 4, ch)
                r32 = R.err_ratio(np.abs(R.f64(g32) - g[..., ch]), forms[0][3][..., ch])
                rk = R.err_ratio(np.abs(host(q0) - g), forms[0][3])
                print("  %-58s max err / bound %.5f" % (tag + "float32 restatement, pooled gradient", r32))
                assert rk <= PRECISION_FACTOR * r32, (mode, rk, r32)
    if R.tiles(shape, 4) <= R.PRECISION_TILES:
        ch = slice(0, R.RESTATED_CHANNELS)
        y32 = np.maximum(R.winograd32(x, w, 4, ch) + bias[ch], np.float32(0))
        r32 = R.err_ratio(np.abs(R.f64(y32) - y[..., ch]), by[..., ch])
        print("  %-58s max err / bound %.5f" % ("float32 restatement, forward", r32))
        for mode, r in ratios.items():
            assert r <= PRECISION_FACTOR * r32, (mode, r, r32)
    for form in ("pool_float", "pool_bits"):
        seen(key_f, "fwd", form, single_extra(key_f, Ci, Co))
    seen(key_g, "dgrad", "pool_bits", single_extra(key_g, Co, Ci))
    seen(key_gf, "dgrad", "pool_float", single_extra(key_gf, Co, Ci))


# ---- exact: every Winograd path with zero filters ----------------------------------------------------------------------------
ZERO_LAYERS = [(c[0], False) for c in R.PLAIN_LAYERS] + [(c[0], True) for c in R.POOLED_LAYERS]


@pytest.mark.parametrize("shape,pooled", ZERO_LAYERS, ids=["%s%s" % ("x".join(map(str, s)), "-pooled" if p else "")
                                                           for s, p in ZERO_LAYERS])
def test_zero_filters_leave_bias_mask_pool_and_addend_exact(ops, shape, pooled):
    """U = G 0 G^T = 0 exactly, so y == relu(bias), y_pool == its average, gx == addend where the addend follows the mask
    (the rule of nfs_hip.h: dgrad (x_in > 0) + addend) and gx == addend (x_in > 0) in the addend_unmasked form, at every
    pixel, ragged edges and floored pool rows included"""
    B, H, W, Ci, Co = shape
    assert ops.conv3x3_plan(B, H, W, Ci, Co, int(pooled))["family"].startswith("wg")
    x = R.int_tensor((B, H, W, Ci), 1)
    bias = R.int_tensor((Co,), 2)
    add = R.int_tensor((B, H, W, Ci), 3)
    gy = R.int_tensor((B, H // 2, W // 2, Co) if pooled else (B, H, W, Co), 4)
    mask = x > 0
    y = np.broadcast_to(np.maximum(R.f64(bias), 0.0), (B, H, W, Co))
    X, Bias, ADD, GY = dev(x), dev(bias), dev(add), dev(gy)
    Wz = torch.zeros(3, 3, Ci, Co, device="cuda")
    wf, wdp = ops.conv3x3_pack(Wz, 0), ops.conv3x3_pack(Wz, 1)
    for mode in modes_of("wg4_three"):
        with gemm_mode(ops, mode):
            poison_workspace(ops, B, H, W, Ci, Co)
            if not pooled:
                equal("y == relu(bias)", ops.conv3x3_fwd(X, wf, Bias, Co, relu=True, out=nan(B, H, W, Co)), y, 4)
                grads = [lambda **kw: ops.conv3x3_dgrad(GY, wdp, Ci, out=nan(B, H, W, Ci), **kw)]
            else:
                y_k, p_k = ops.conv3x3_fwd_pool(X, wf, Bias, Co, relu=True, out=nan(B, H, W, Co),
                                                out_pool=nan(B, H // 2, W // 2, Co))
                equal("y == relu(bias)", y_k, y, 4)
                equal("y_pool == its average", p_k, R.avgpool2(y), 2)
                rb = ops.conv3x3_relu_bits(B, H, W, Ci, Co, True, X.device)
                rb.fill_(float("nan"))
                ops.conv3x3_fwd_pool(X, wf, Bias, Co, relu=True, relu_bits=rb, want_y=False)
                grads = [lambda **kw: ops.conv3x3_dgrad_pool(GY, y_k, wdp, Ci, out=nan(B, H, W, Ci), **kw),
                         lambda **kw: ops.conv3x3_dgrad_pool(GY, None, wdp, Ci, relu_bits=rb, hw=(H, W),
                                                             out=nan(B, H, W, Ci), **kw)]
            for grad in grads:
                poison_workspace(ops, B, H, W, Ci, Co)
                equal("gx == 0", grad(), np.zeros((B, H, W, Ci)), 4)
                poison_workspace(ops, B, H, W, Ci, Co)
                equal("gx == 0 (x_in > 0) + addend", grad(x_in=X, addend=ADD), R.f64(add), 4)
                poison_workspace(ops, B, H, W, Ci, Co)
                equal("gx == (0 + addend) (x_in > 0) [addend_unmasked]", grad(x_in=X, addend=ADD, addend_unmasked=True),
                      R.f64(add) * mask, 4)


# ---- exact: the direct kernels on integers -------------------------------------------------------------------------------------
def _exact_layer(ops, shape, splitk, m_f, m_g, masked):
    """forward and data gradient of a layer on integer inputs against float64, no tolerance"""
    B, H, W, Ci, Co = shape
    x, w = R.int_tensor((B, H, W, Ci), 11), R.int_tensor((3, 3, Ci, Co), 12)
    bias, gy = R.int_tensor((Co,), 13), R.int_tensor((B, H, W, Co), 14)
    y, S = R.conv(x, w, bias, relu=True)
    R.exact_units(S, 3.0)
    g, Sg = R.dgrad(gy, w)
    R.exact_units(Sg, 3.0)
    X, Wt, Bias, GY = dev(x), dev(w), dev(bias), dev(gy)
    wf, wdp = ops.conv3x3_pack(Wt, 0), ops.conv3x3_pack(Wt, 1)
    if splitk:
        poison_workspace(ops, B, H, W, Ci, Co)
    equal("y == relu(conv + bias)", ops.conv3x3_fwd(X, wf, Bias, Co, relu=True, out=nan(B, H, W, Co), splitk=splitk), y, m_f)
    if splitk:
        poison_workspace(ops, B, H, W, Ci, Co)
    equal("gx == dgrad(gy)", ops.conv3x3_dgrad(GY, wdp, Ci, out=nan(B, H, W, Ci), splitk=splitk), g, m_g)
    if masked:
        x_in, add = R.int_tensor((B, H, W, Ci), 15), R.int_tensor((B, H, W, Ci), 16)
        if splitk:
            poison_workspace(ops, B, H, W, Ci, Co)
        got = ops.conv3x3_dgrad(GY, wdp, Ci, x_in=dev(x_in), addend=dev(add), out=nan(B, H, W, Ci), splitk=splitk)
        equal("gx == dgrad(gy) (x_in > 0) + addend", got, R.layer_dgrad(g, x_in, add), m_g)


C3_SHAPES = [((1, 8, 16), (False, 1, 1), (True, 2, 2)),            # one 8 x 16 forward tile
             ((1, 14, 14), (True, 2, 2), (False, 1, 1)),           # one 14 x 14 gradient tile
             ((2, 13, 37), (True, 12, 12), (True, 6, 6)),          # several tiles, both edges ragged both ways
             ((8, 120, 130), (True, 1080, 1024), (True, 720, 512))]    # more tiles than blocks: the tile walk wraps


@pytest.mark.parametrize("bhw,fwd,grad", C3_SHAPES, ids=["x".join(map(str, c[0])) for c in C3_SHAPES])
def test_conv1_1_exact(ops, bhw, fwd, grad):
    B, H, W = bhw
    for direction, K, N, (ragged, ntiles, blocks) in (("fwd", 3, 64, fwd), ("dgrad", 64, 3, grad)):
        p = ops.conv3x3_plan(B, H, W, K, N)
        assert (p["family"], p["ragged"], p["tiles"], p["blocks"]) == ("c3_mfma", ragged, ntiles, blocks), p
    _exact_layer(ops, (B, H, W, 3, 64), True, (8, 16), (14, 14), masked=False)
    for direction, (ragged, ntiles, blocks) in (("fwd", fwd), ("dgrad", grad)):
        _SEEN.add(("c3_mfma", direction, "plain", "ragged" if ragged else "whole", "wraps" if ntiles > blocks else "--", "k1",
                   None))


def test_generic_three_channel_kernels_exact(ops):
    B, H, W = 2, 9, 7
    assert ops.conv3x3_plan(B, H, W, 3, 128)["family"] == "c3_generic"
    assert ops.conv3x3_plan(B, H, W, 128, 3)["family"] == "c3_generic"
    _exact_layer(ops, (B, H, W, 3, 128), True, 4, 4, masked=False)
    _SEEN.add(("c3_generic", "fwd", "plain", "whole", "--", "k1", None))
    _SEEN.add(("c3_generic", "dgrad", "plain", "whole", "--", "k1", None))


# (shape, (column tile, ragged pixel tile) of the forward pass and of the gradient without a workspace)
DIRECT_LAYERS = [((2, 13, 11, 64, 64), (64, True), (64, True)), ((2, 13, 11, 64, 128), (64, True), (64, True)),
                 ((2, 13, 11, 512, 64), (64, True), (64, True)), ((2, 13, 11, 512, 128), (64, True), (64, True)),
                 ((2, 16, 16, 64, 64), (64, False), (64, False)),
                 ((4, 100, 127, 64, 128), (128, True), (64, True)), ((4, 100, 128, 128, 64), (64, False), (128, False)),
                 ((4, 100, 128, 64, 128), (128, False), (64, False)), ((4, 100, 127, 128, 64), (64, True), (128, True))]


@pytest.mark.parametrize("shape,fwd,grad", DIRECT_LAYERS, ids=_ids(DIRECT_LAYERS))
def test_direct_implicit_gemm_without_workspace_exact(ops, shape, fwd, grad):
    B, H, W, Ci, Co = shape
    for K, N, want in ((Ci, Co, fwd), (Co, Ci, grad)):
        p = ops.conv3x3_plan(B, H, W, K, N)["no_ws"]
        assert (p["bn"], p["ragged"], p["kparts"]) == (want[0], want[1], 1), p
    _exact_layer(ops, shape, False, 4, 4, masked=True)
    for direction, want in (("fwd", fwd), ("dgrad", grad)):
        _SEEN.add(("direct", direction, "plain", "ragged" if want[1] else "whole", "bn%d" % want[0], "k1", None))


def test_direct_implicit_gemm_split_k_exact(ops):
    """Winograd refuses H < 2, so a one-row image is the only way to the direct kernel's split-K planner"""
    shape = (4, 1, 40, 512, 512)
    B, H, W, Ci, Co = shape
    p = ops.conv3x3_plan(B, H, W, Ci, Co)
    assert p["family"] == "direct" and p["kparts"] > 1, p
    ops._conv_ws.clear()                     # a fresh workspace of exactly the size the plan is stated for
    _exact_layer(ops, shape, True, 4, 4, masked=True)
    _SEEN.add(("direct", "fwd", "plain", "whole", "bn%d" % p["bn"], "split", None))
    _SEEN.add(("direct", "dgrad", "plain", "whole", "bn%d" % p["bn"], "split", None))


# ---- the ledger ----------------------------------------------------------------------------------------------------------------
def reachable():
    """every combination the launch code reaches without an environment toggle, from its rules:
    family x forward / gradient x plain / pooled-float / pooled-bits x whole / ragged x schedule x K parts.
      three kernels   both schedules (same-channel layers: input and output transform alike) x 1 | 2 K parts; the pooled
                      gradient masked from the float output has no six-wave input transform ("tw" where the bit-cache
                      form runs "ww");
      single kernel   its <K, N> instances, K and N in {64, 128}; every pooled form;
      F(5x5)          plain only (no pooling fused there); seven waves x 1 | 2 K parts, threads x 1 K part.  Threads with
                      two K parts would need T <= 64 and T K > 65536, so K > 1024 channels, twice the widest VGG layer:
                      left out (its filters alone pack to several GB);
      conv1_1         whole and ragged tiles, one block per tile and the wrapping tile walk (ragged there: a shape of
                      more than 512 whole tiles is a million pixels);
      generic Ci = 3, direct implicit GEMM: both column tiles x whole / ragged pixel tiles, and split-K."""
    req = set()
    fwd_forms, grad_forms = ("plain", "pool_float", "pool_bits"), ("plain", "pool_bits", "pool_float")
    for ragged in ("whole", "ragged"):
        for k in ("k1", "k2"):
            for sched in ("ww", "tt"):
                for form in fwd_forms:
                    req.add(("wg4_three", "fwd", form, ragged, sched, k, None))
                for form in grad_forms:
                    s = "tw" if (form == "pool_float" and sched == "ww") else sched
                    req.add(("wg4_three", "dgrad", form, ragged, s, k, None))
        for K in (64, 128):
            for N in (64, 128):
                for form in fwd_forms:
                    req.add(("wg4_single", "fwd", form, ragged, "--", "k1", (K, N)))
                    req.add(("wg4_single", "dgrad", form, ragged, "--", "k1", (K, N)))
        for sched, k in (("ww", "k1"), ("ww", "k2"), ("tt", "k1")):
            for direction in ("fwd", "dgrad"):
                req.add(("wg5", direction, "plain", ragged, sched, k, None))
        for direction in ("fwd", "dgrad"):
            req.add(("c3_mfma", direction, "plain", ragged, "--", "k1", None))
            for bn in ("bn64", "bn128"):
                req.add(("direct", direction, "plain", ragged, bn, "k1", None))
    for direction in ("fwd", "dgrad"):
        req.add(("c3_mfma", direction, "plain", "ragged", "wraps", "k1", None))
        req.add(("c3_generic", direction, "plain", "whole", "--", "k1", None))
        req.add(("direct", direction, "plain", "whole", "bn64", "split", None))
    return req


def test_every_reachable_path_was_run():
    """the cases above, together, ran every combination of ``reachable`` (run the whole module)"""
    missing = sorted(reachable() - _SEEN, key=str)
    assert not missing, "never run: %s" % missing

"""The Gram chain and the scalar losses entry by entry against the float64 restatement of tests/loss_ref.py.

Exact inputs (integer features, powers of two for every scale and weight, integer perturbations of the style Gram):
float32 arithmetic is exact on them in any order, so the kernel's output must EQUAL the float64 value -- a dropped or
doubled pixel, a wrong tile, a wrong mirror, a lost factor 2 or a stale workspace word fails at 1 ulp.  Each exact
input asserts its precondition on the CPU (loss_ref.units) before the GPU is touched.  "Equal" compares float32
values: the sign of a zero is not compared, a NaN equals nothing.

Realistic magnitudes (post-ReLU randn * 30, general scales): each element inside its derived worst-case float32 bound;
every such check prints the largest err / bound it saw (pytest -s).

The plan a shape takes depends on the chip's CU count; it is read back from nfs_gram_workspace_floats (B * npair *
nslab * 4096 + 16384), and a case whose shape is planned onto another path than the one it is named for skips."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import loss_ref as LR

pytestmark = pytest.mark.gpu
NAN = float("nan")
U = LR.U


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


def T(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def f32(x):
    """a Python float that is a float32: what a kernel receives for a float argument"""
    return float(np.float32(x))


def check(name, got, ref, bound):
    r = LR.err_ratio(np.abs(np.asarray(got, dtype=np.float64) - ref), bound)
    print("%-72s max err/bound %.3g" % (name, r))
    assert r <= 1.0, (name, r)


def equal(name, got, ref, decode=None):
    """got (float32) == ref (float64) on every entry; the message names the first entries that differ"""
    got, ref = np.asarray(got), LR.f64(ref)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    assert LR.is_f32(ref), "%s: the reference is not a float32 -- the input is not exact" % name
    bad = ~(got.astype(np.float64) == ref)
    if bad.any():
        idx = np.argwhere(bad)
        show = decode or (lambda v, i: repr(float(v)))
        lines = ["%s: got %s, want %s" % (tuple(int(v) for v in i), show(got[tuple(i)], i), show(ref[tuple(i)], i))
                 for i in idx[:6]]
        raise AssertionError("%s: %d of %d entries differ\n  %s" % (name, len(idx), got.size, "\n  ".join(lines)))


def nslab_of(B, HW, C):
    from neural_flow_style_amd import _lib
    npair = (C // 64) * (C // 64 + 1) // 2
    q, r = divmod(int(_lib.lib().nfs_gram_workspace_floats(B, HW, C)) - 16384, B * npair * 4096)
    assert r == 0 and q >= 1, (B, HW, C, q, r)
    return q


def require_path(shape, path):
    n = nslab_of(*shape)
    if not LR.on_path(path, n, shape[1]):
        pytest.skip("this chip plans %d slabs for %s, which is not the '%s' path" % (n, shape, path))
    return n


def _gid(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def gcase(shape, with_dev):
    return LR.gram_case(shape, with_dev=with_dev)


@functools.lru_cache(maxsize=None)
def real_features(B, HW, C, seed):
    return (np.maximum(np.random.RandomState(seed).randn(B, HW, C), 0) * 30).astype(np.float32)


def real_style_gram(Bs, HW, C, scale, seed):
    """an exactly symmetric float32 style Gram of other features of the same kind"""
    Gs, _ = LR.gram(real_features(Bs, HW, C, seed), scale)
    return ((Gs + Gs.transpose(0, 2, 1)) / 2).astype(np.float32)


# ---- 1. nfs_gram_fwd on exact inputs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["two_pass", "atomic", "scale_dev"])
@pytest.mark.parametrize("shape,path", LR.GRAM_SHAPES, ids=_gid)
def test_gram_fwd_equals_float64_on_exact_inputs(ops, shape, path, variant):
    """integer features, scale 2^-3 (scale_dev: times 2^-(b+1) per image): G == the float64 Gram on every entry.  G is
    passed in full of NaN where the kernels write it (two-pass, one slab) and zeroed by ops.gram_fwd on the float-atomic
    path; G == G^T and a second call gives the same bits"""
    B, HW, C = shape
    n = require_path(shape, path)
    c = gcase(shape, variant == "scale_dev")
    F = T(c["F"])
    dev = None if c["dev"] is None else T(c["dev"])
    out = []
    for _ in range(2):
        if variant == "atomic":
            out.append(ops.gram_fwd(F, c["s"], two_pass=False))
        else:
            out.append(ops.gram_fwd(F, c["s"], scale_dev=dev, G=nans(B, C, C)))
    G = out[0]
    assert bool(torch.isfinite(G).all()), "%s (%d slabs): entries never written" % (shape, n)
    equal("G %s %s (%s, %d slabs)" % (shape, variant, path, n), N(G), c["G"])
    assert torch.equal(G, G.transpose(1, 2)) and torch.equal(G, out[1])


@pytest.mark.parametrize("B,HW,C,two_pass", [(1, 1000, 128, True), (1, 1000, 128, False), (2, 37, 256, True),
                                             (2, 300, 128, True), (3, 1025, 128, True)])
def test_gram_fwd_marker_pixels_and_channels(ops, B, HW, C, two_pass):
    """F is zero but for pixels {0, 31, 32, HW-1} x channels {0, 63, 64, C-1}, each a distinct power of two (loss_ref.
    marker_features): the exponent of an entry of G names its channel pair and its mantissa the pixels that reached it,
    so a failure says which pixel or tile went missing; every other entry must be 0"""
    F = LR.marker_features(B, HW, C)
    ref, mag = LR.gram(F, 1.0)
    assert LR.is_f32(ref)
    G = ops.gram_fwd(T(F), 1.0, G=nans(B, C, C)) if two_pass else ops.gram_fwd(T(F), 1.0, two_pass=False)
    equal("marker G (%d, %d, %d) %s, %d slabs" % (B, HW, C, "two-pass" if two_pass else "atomic", nslab_of(B, HW, C)),
          N(G), ref, decode=lambda v, i: LR.marker_decode(v, int(i[0])))


# ---- 5 (path of 1). realistic magnitudes -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["two_pass", "atomic", "scale_dev"])
@pytest.mark.parametrize("shape,path", LR.GRAM_SHAPES, ids=_gid)
def test_gram_fwd_is_float32_accurate(ops, shape, path, variant):
    """relu(randn) * 30, scale = 1 / (2 HW C) (scale_dev: times a general per-image factor).  Rounding count of an entry:
    HW fma steps of the MFMA chain (one rounding each), at most nslab additions of slab partials (the reduce, or the
    float atomics), the product scale * scale_dev and the scaling itself: (HW + nslab + 4) u of scale sum |F_pi F_pj|"""
    B, HW, C = shape
    n = require_path(shape, path)
    F = real_features(B, HW, C, 9)
    scale = f32(1.0 / (2.0 * HW * C))
    dev = (np.random.RandomState(3).rand(B) + 0.5).astype(np.float32) if variant == "scale_dev" else None
    ref, mag = LR.gram(F, scale, dev)
    if variant == "atomic":
        G = ops.gram_fwd(T(F), scale, two_pass=False)
    else:
        G = ops.gram_fwd(T(F), scale, scale_dev=None if dev is None else T(dev), G=nans(B, C, C))
    check("G %s %s (%s, %d slabs)" % (shape, variant, path, n), N(G), ref, LR.gram_bound(mag, HW, n))


# ---- 2. nfs_style_loss_fwd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["diag", "off", "last"])
@pytest.mark.parametrize("B,Bs,C", [(3, 1, 64), (3, 3, 128), (4, 2, 128), (2, 1, 512), (2, 2, 512)])
def test_style_loss_fwd_equals_float64_on_exact_inputs(ops, B, Bs, C, where):
    """G from nfs_gram_fwd on integer features (itself equal to float64, asserted), Gs = G[:Bs] - 2^-3 E with a symmetric
    integer E confined to one tile (and its mirror), weight 2^-2: Dmat == 2 w (G_b - Gs_{b % Bs}) (== 2 w s E where
    Bs == B) and loss[b] == the float64 loss of image b, PER IMAGE, on top of the power of two loss_acc held before
    (the accumulate contract).  C >= 128 takes the grid-stride loop"""
    c = LR.style_case(B, Bs, C, where, 11)
    G = ops.gram_fwd(T(c["F"]), c["s"], G=nans(B, C, C))
    equal("G", N(G), c["G"])
    lacc = torch.full((B,), c["pre"], dtype=torch.float32, device="cuda")
    Dm = ops.style_loss_fwd(G, T(c["Gs"]), c["w"], lacc, Dmat=nans(B, C, C))
    name = "B %d Bs %d C %d E in the %s tile" % (B, Bs, C, where)
    equal("Dmat " + name, N(Dm), c["D"])
    if Bs == B:
        equal("Dmat == 2 w s E " + name, N(Dm), 2 * c["w"] * c["s"] * c["E"])
    equal("loss per image " + name, N(lacc), c["loss"] + c["pre"])


@pytest.mark.parametrize("B,Bs,HW,C", [(3, 1, 5003, 64), (2, 2, 1000, 128), (4, 2, 144, 512)])
def test_style_loss_fwd_is_float32_accurate(ops, B, Bs, HW, C):
    """realistic G (nfs_gram_fwd of relu(randn) * 30) against the float64 chain from F.  D = 2w (G - Gs): the bound of G
    times 2w, plus the subtraction and the product (2u |D|).  loss[b]: the first-order propagation of G's bound
    (dL/dG = D), plus (C^2 + P) u loss for the squares and the summation, P = 32 block partials added atomically"""
    n = nslab_of(B, HW, C)
    F = real_features(B, HW, C, 21)
    scale, w = f32(1.0 / (2.0 * HW * C)), f32(0.7)
    G64, mag = LR.gram(F, scale)
    Gs = real_style_gram(Bs, HW, C, scale, 22)
    G = ops.gram_fwd(T(F), scale, G=nans(B, C, C))
    lacc = torch.zeros(B, device="cuda")
    Dm = ops.style_loss_fwd(G, T(Gs), w, lacc, Dmat=nans(B, C, C))
    loss, D = LR.style_loss(G64, Gs, w)
    bD, bL = LR.style_bounds(G64, Gs, w, LR.gram_bound(mag, HW, n), 32)
    name = "(%d, %d, %d) Bs %d" % (B, HW, C, Bs)
    check("style_loss_fwd Dmat " + name, N(Dm), D, bD)
    check("style_loss_fwd loss per image " + name, N(lacc), loss, bL)


# ---- 3. the grouped chain ----------------------------------------------------------------------------------------------
def run_group(layers, B, Bs):
    """nfs_gram_style_group_fwd + nfs_gram_group_bwd on ``layers`` (dicts with F, Gs, s, w), GramLayer filled directly;
    every output buffer and the workspace start as NaN.  Returns (parts [P,B], per layer (G, Dmat, dF, relu_mask))"""
    from neural_flow_style_amd import _lib, ops
    n = len(layers)
    arr = (_lib.GramLayer * n)()
    keep = []
    for l, y in enumerate(layers):
        HW, C = y["HW"], y["C"]
        F, Gs = T(y["F"]), T(y["Gs"])
        G, Dm, dF = nans(B, C, C), nans(B, C, C), nans(B, HW, C)
        keep.append((F, Gs, G, Dm, dF, l % 2))
        a = arr[l]
        a.F, a.Gs, a.G, a.Dmat, a.dF = F.data_ptr(), Gs.data_ptr(), G.data_ptr(), Dm.data_ptr(), dF.data_ptr()
        a.B, a.Bs, a.HW, a.C = B, Bs, HW, C
        a.scale, a.weight, a.relu_mask = y["s"], y["w"], l % 2
    L = _lib.lib()
    P, nws = int(L.nfs_gram_style_group_parts(arr, n)), int(L.nfs_gram_style_group_workspace_floats(arr, n))
    # slab layers and one-slab layers in one call, as planned (the grouped plan does not depend on the chip)
    assert (nws, P) == LR.group_plan([(y["HW"], y["C"]) for y in layers], B), (nws, P)
    ws = nans(max(nws, 1))
    parts = nans(P, B)
    _lib.call("nfs_gram_style_group_fwd", arr, n, ops._ptr(parts), ops._ptr(ws), ws.numel(), ops._stream())
    _lib.call("nfs_gram_group_bwd", arr, n, ops._stream())
    torch.cuda.synchronize()
    return N(parts), [(N(k[2]), N(k[3]), N(k[4]), k[5]) for k in keep]


def check_group_exact(tag, layers, parts, outs, B):
    """G and Dmat equal to float64 on every layer; dF within the Gram gradient's bound; the per-image loss -- the sum
    of the partials of ALL layers -- equal to float64 when every layer is exact, else within the bounded layers' bounds"""
    assert np.isfinite(parts).all(), "%s: loss partials never written" % tag
    P = parts.shape[0]
    slack = np.zeros(B)
    for y, (G, Dm, dF, rm) in zip(layers, outs):
        name = "%s layer (%d, %d)" % (tag, y["HW"], y["C"])
        equal("G " + name, G, y["G"])
        equal("Dmat " + name, Dm, y["D"])
        assert np.array_equal(Dm, Dm.transpose(0, 2, 1)), name
        ref, bound = LR.gram_bwd(y["F"], y["D"], y["s"], relu_mask=bool(rm))
        check("dF " + name, dF, ref, bound)
        if not y["exact"]:
            slack += LR.style_bounds(y["G"], y["Gs"], y["w"], 0.0, P)[1]
    got = np.array([math.fsum(parts[:, b].astype(np.float64)) for b in range(B)])
    want = np.array([math.fsum(y["loss"][b] for y in layers) for b in range(B)])
    if all(y["exact"] for y in layers):
        assert np.array_equal(got, want), "%s: per-image loss %r, want %r" % (tag, got.tolist(), want.tolist())
    else:
        check("loss per image " + tag, got, want, slack)


@pytest.mark.parametrize("Bs", [1, 3])
def test_grouped_chain_equals_float64_on_exact_inputs(Bs):
    """nfs_gram_style_group_fwd against float64 (not against the per-layer chain, with which it shares its blocks): seven
    layers in one call -- 16-chunk slabs (1600, 1295 and 1025 pixels, the last slab of 1025 holding one pixel), one slab
    (1024 pixels = 32 chunks, 600, 30, 9), C = 64 / 128 / 512 --, B = 3, Bs = 1 and Bs = B.  Every G and every Dmat (tile
    and mirror) equals float64.  Four layers take a tile-confined E, so their loss is exact: run alone, parts[:, b]
    summed in float64 EQUALS the per-image loss.  Three take a full random integer Gs: D is exact on every tile; their
    loss rounds (d^2 passes 2^24) and is held to (C^2 + P) u loss, one rounding per square and per addition, in the
    seven-layer call.  dF closes the chain against 2 scale F D (F > 0) within the Gram gradient's bound"""
    B = 3
    layers = LR.group_case(B, Bs, LR.GROUP_LAYERS)
    parts, outs = run_group(layers, B, Bs)
    check_group_exact("7 layers Bs %d" % Bs, layers, parts, outs, B)
    ex = [y for y in layers if y["exact"]]
    assert {y["HW"] > 1024 for y in ex} == {True, False}           # slab layers and one-slab layers among them
    parts, outs = run_group(ex, B, Bs)
    check_group_exact("4 exact layers Bs %d" % Bs, ex, parts, outs, B)


def test_grouped_chain_nine_layers_and_padded_channels(ops):
    """ops.gram_style_group with nine layers (two launches of 8 + 1; the rows of parts concatenate) and channels= smaller
    than C on zero-padded layers: scale = 1 / (2 HW channels) counts the logical channels (a power of two here), every
    G equals float64, parts[:, b] still sums to the exact per-image loss, dF within its bound"""
    B, Bs = 3, 1
    layers = LR.group_case(B, Bs, LR.SPLIT_LAYERS)
    assert len(layers) == 9 and any(y["ch"] < y["C"] for y in layers) and all(y["exact"] for y in layers)
    masks = [bool(l % 2) for l in range(9)]
    parts, dFs, Gs_out = ops.gram_style_group([T(y["F"]) for y in layers], [T(y["Gs"]) for y in layers],
                                              [y["w"] for y in layers], masks, want_G=True,
                                              channels=[y["ch"] for y in layers])
    torch.cuda.synchronize()
    parts = N(parts)
    hc = [(y["HW"], y["C"]) for y in layers]
    assert parts.shape == (LR.group_plan(hc[:8], B)[1] + LR.group_plan(hc[8:], B)[1], B) and np.isfinite(parts).all()
    for y, G, dF, rm in zip(layers, Gs_out, dFs, masks):
        name = "9 layers, layer (%d, %d) of %d channels" % (y["HW"], y["C"], y["ch"])
        equal("G " + name, N(G), y["G"])
        ref, bound = LR.gram_bwd(y["F"], y["D"], y["s"], relu_mask=rm)
        check("dF " + name, N(dF), ref, bound)
    got = [math.fsum(parts[:, b].astype(np.float64)) for b in range(B)]
    want = [math.fsum(y["loss"][b] for y in layers) for b in range(B)]
    assert got == want, (got, want)


# ---- 5 (path of 3). the grouped chain at realistic magnitudes ----------------------------------------------------------
@pytest.mark.parametrize("Bs", [1, 3])
def test_grouped_chain_is_float32_accurate(Bs):
    """the seven layers with relu(randn) * 30 features, scale = 1 / (2 HW C), general weights.  G: (HW + nslab + 4) u of
    scale sum |F F| (nslab = 16-chunk slabs above 32 chunks, else 1); Dmat: that times 2w plus 2u |D|; the per-image
    loss over all layers: per layer sum |D| (G's bound) + (C^2 + P) u loss, P the number of partials of the call"""
    B = 3
    layers = []
    for l, (HW, C, _) in enumerate(LR.GROUP_LAYERS):
        F = real_features(B, HW, C, 40 + l)
        s, w = f32(1.0 / (2.0 * HW * C)), f32(0.5 + 0.25 * l)
        G, mag = LR.gram(F, s)
        Gs = real_style_gram(Bs, HW, C, s, 60 + l)
        loss, D = LR.style_loss(G, Gs, w)
        chunks = (HW + 31) // 32
        layers.append(dict(HW=HW, C=C, F=F, s=s, w=w, G=G, Gs=Gs, D=D, loss=loss, mag=mag,
                           nslab=(chunks + 15) // 16 if chunks > 32 else 1))
    parts, outs = run_group(layers, B, Bs)
    assert np.isfinite(parts).all()
    slack = np.zeros(B)
    for y, (G, Dm, dF, rm) in zip(layers, outs):
        name = "layer (%d, %d) Bs %d" % (y["HW"], y["C"], Bs)
        bG = LR.gram_bound(y["mag"], y["HW"], y["nslab"])
        bD, bL = LR.style_bounds(y["G"], y["Gs"], y["w"], bG, parts.shape[0])
        check("group G " + name, G, y["G"], bG)
        check("group Dmat " + name, Dm, y["D"], bD)
        assert np.array_equal(G, G.transpose(0, 2, 1)), name
        # dF from the kernel's own D (float32): the Gram gradient's bound alone
        ref, bound = LR.gram_bwd(y["F"], Dm, y["s"], relu_mask=bool(rm))
        check("group dF " + name, dF, ref, bound)
        slack += bL
    got = np.array([math.fsum(parts[:, b].astype(np.float64)) for b in range(B)])
    want = np.array([math.fsum(y["loss"][b] for y in layers) for b in range(B)])
    check("group loss per image Bs %d" % Bs, got, want, slack)


# ---- 4. the masked chain -----------------------------------------------------------------------------------------------
def test_masked_chain_equals_float64_on_exact_inputs(ops):
    """style_mask_apply -> gram_fwd(scale_dev) -> style_loss_fwd -> gram_bwd(scale_dev, relu_mask=False) ->
    style_mask_bwd as the style-mask branch of the image stylizer runs it.  A 0/1 mask on 40 x 37 pixels (1480: more
    than the 256 threads that sum it) of area 128 / 256, C = 64: 1 / (2 area C) = 2^-14 / 2^-15.  Fm, scale, G, Dmat and
    the per-image loss equal float64; dF is zero where the mask or F is zero and within the Gram gradient's bound"""
    B, h, w, C = 2, 40, 37, 64
    m = LR.mask01(B, h, w, (128, 256), 3)
    F = np.maximum(LR.int_features(B, h * w, C, 4), 0).reshape(B, h, w, C)
    Fm64, s64 = LR.style_mask_apply(F, m)
    G64, mag = LR.gram(Fm64, 1.0, s64)
    assert s64.tolist() == [2.0 ** -14, 2.0 ** -15] and all(LR.units(mag[b], s64[b]) < LR.LIMIT for b in range(B))
    Fm, scale = ops.style_mask_apply(T(F), T(m))
    equal("Fm", N(Fm), Fm64)
    equal("scale", N(scale), s64)
    G = ops.gram_fwd(Fm, 1.0, scale_dev=scale, G=nans(B, C, C))
    equal("masked G (%d slabs)" % nslab_of(B, h * w, C), N(G), G64)
    E, wgt = LR.tile_E(B, C, "diag", 5), 2.0 ** -2
    Gs = G64 - s64[:, None, None] * E
    loss64, D64 = LR.style_loss(G64, Gs, wgt)
    assert LR.is_f32(Gs) and all(LR.units(loss64[b], wgt * s64[b] ** 2) < LR.LIMIT for b in range(B))
    lacc = torch.zeros(B, device="cuda")
    Dm = ops.style_loss_fwd(G, T(Gs), wgt, lacc, Dmat=nans(B, C, C))
    equal("masked Dmat", N(Dm), D64)
    equal("masked loss per image", N(lacc), loss64)
    dFm = ops.gram_bwd(Fm, Dm, 1.0, scale_dev=scale, relu_mask=False)
    ref, bound = LR.gram_bwd(Fm64, D64, 1.0, s64)
    check("masked dFm", N(dFm), ref, bound)
    dF = N(ops.style_mask_bwd(dFm, T(m), T(F)))
    equal("masked dF == dFm m (F > 0)", dF, LR.style_mask_bwd(N(dFm), m, F))
    dead = np.broadcast_to(m == 0, F.shape) | (F == 0)
    assert dead.any() and not dF[dead].any() and dF[~dead].any()


def test_masked_chain_is_float32_accurate(ops):
    """the same chain with a fractional mask (exact zeros in it) and relu(randn) * 30 features, each stage against float64
    on the float32 values the stage before it produced: Fm one rounding; the area a sum of HW floats and scale two more
    operations, (HW + 3) u; G (HW + nslab + 4) u of scale sum |Fm Fm|; Dmat 2u |D| and the loss (C^2 + 32) u loss (G is
    the stage's input); dFm the Gram gradient's bound; dF one rounding"""
    B, h, w, C = 2, 40, 37, 64
    HW = h * w
    rng = np.random.RandomState(6)
    m = (rng.rand(B, h, w, 1) * (rng.rand(B, h, w, 1) < 0.7)).astype(np.float32)
    F = real_features(B, HW, C, 7).reshape(B, h, w, C)
    Fm, scale = ops.style_mask_apply(T(F), T(m))
    Fm64, s64 = LR.style_mask_apply(F, m)
    check("style_mask_apply Fm", N(Fm), Fm64, U * np.abs(Fm64))
    check("style_mask_apply scale", N(scale), s64, 1.01 * (HW + 3) * U * s64)
    n = nslab_of(B, HW, C)
    G = ops.gram_fwd(Fm, 1.0, scale_dev=scale, G=nans(B, C, C))
    G64, mag = LR.gram(N(Fm), 1.0, N(scale))
    check("masked G (%d slabs)" % n, N(G), G64, LR.gram_bound(mag, HW, n))
    wgt = f32(0.7)
    Gs = real_style_gram(1, HW, C, f32(1.0 / (2.0 * HW * C)), 8)
    lacc = torch.zeros(B, device="cuda")
    Dm = ops.style_loss_fwd(G, T(Gs), wgt, lacc, Dmat=nans(B, C, C))
    loss64, D64 = LR.style_loss(N(G), Gs, wgt)
    bD, bL = LR.style_bounds(N(G), Gs, wgt, 0.0, 32)
    check("masked Dmat", N(Dm), D64, bD)
    check("masked loss per image", N(lacc), loss64, bL)
    dFm = ops.gram_bwd(Fm, Dm, 1.0, scale_dev=scale, relu_mask=False)
    ref, bound = LR.gram_bwd(N(Fm), N(Dm), 1.0, N(scale))
    check("masked dFm", N(dFm), ref, bound)
    dF = N(ops.style_mask_bwd(dFm, T(m), T(F)))
    ref = LR.style_mask_bwd(N(dFm), m, F)
    check("masked dF", dF, ref, U * np.abs(ref))
    assert not dF[np.broadcast_to(m == 0, F.shape) | (F == 0)].any()


# ---- 6. content loss ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [False, True], ids=["relu", "signed"])
@pytest.mark.parametrize("mode", ["channel", "last_channel", "all", "target"])
@pytest.mark.parametrize("shape", [(3, 5, 7, 64), (2, 20, 17, 64)], ids=_gid)
def test_content_loss_element_by_element(ops, shape, mode, signed):
    """nfs_content_loss on a post-ReLU tensor and nfs_content_loss_signed on one that is no ReLU output, both with exact
    zeros; (2, 20, 17, 64) has 21760 elements per image, more than the launch's 64 x 256 threads, so the grid-stride loop
    runs.  Gradient per element: the coefficients are two or three float32 operations (4u |g|); with a target the
    rounding of amp * t and of the difference adds (2w/n) 2u (|f| + |amp t|); accumulating onto g0 adds the rounding of
    the sum, u |g0 + g|.  Unsigned: nothing is added where f <= 0 (the bits of g0 stay).  Signed: sign(f) with 0 at 0,
    every element receives its term.  Loss PER IMAGE within (n_b + 80) u sum |terms|: one rounding per addition of the
    image's n_b terms and at most 64 atomics, the few of a term itself"""
    B, h, w, C = shape
    assert (h * w * C > 64 * 256) == (shape == (2, 20, 17, 64))
    rng = np.random.RandomState(17)
    pre = rng.randn(B, h, w, C).astype(np.float32)
    pre[rng.rand(B, h, w, C) < 0.2] = 0.0
    F = pre if signed else np.maximum(pre, 0)
    ch = {"channel": 11, "last_channel": C - 1, "all": 0, "target": 5}[mode]
    tgt = rng.rand(2 if B == 3 else 1, h, w, C).astype(np.float32) if mode == "target" else None
    wgt, amp = f32(2.5), f32(1.7)
    for g0 in (None, (rng.randn(B, h, w, C) * 1e-4).astype(np.float32)):
        loss = torch.zeros(B, device="cuda")
        g = torch.zeros(B, h, w, C, device="cuda") if g0 is None else T(g0)
        ops.content_loss(T(F), wgt, loss, g, channel=ch, target=None if tgt is None else T(tgt), amp=amp, signed=signed)
        r = LR.content_loss(F, wgt, ch, tgt, amp, signed, g0=g0)
        name = "%s %s %s%s" % (_gid(shape), mode, "signed" if signed else "relu", "" if g0 is None else " onto g0")
        check("content grad " + name, N(g), r["grad"], r["grad_bound"])
        check("content loss per image " + name, N(loss), r["loss"], r["loss_bound"])
        if not signed:
            keep = F <= 0
            assert keep.any() and np.array_equal(N(g)[keep], (np.zeros_like(F) if g0 is None else g0)[keep])
        elif g0 is None and mode in ("channel", "last_channel"):
            off = np.broadcast_to(np.arange(C) != ch, F.shape)
            gn = N(g)
            assert not gn[off & (F == 0)].any() and (gn[off & (F < 0)] < 0).all() and (gn[off & (F > 0)] > 0).all()
            assert (gn[~off] < 0).all()                                   # the maximised channel: -w / n_pix everywhere


# ---- 7. TV loss --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 9, 11, 3), (2, 1, 50, 3), (2, 50, 1, 1), (2, 37, 23, 3)], ids=_gid)
def test_tv_loss_equals_float64_with_ties(ops, shape):
    """an integer image 0 .. 255 with a zero background and constant patches (at least a third of the neighbour
    differences are exact ties: sign(0) = 0 is the contract there), weight 2^-6, B = 2: the loss (on top of the 8 that
    loss_acc held) equals float64, the gradient equals scale * k with k an integer in -4 .. 4 when g starts at 0 and is
    within one rounding of g0 + scale * k otherwise; g_acc = None gives the same loss; an all-constant image leaves the
    loss untouched and the gradient zero.  (2, 37, 23, 3) is no multiple of 256 elements"""
    x = LR.tv_image(shape, 5)
    wgt = 2.0 ** -6
    r = LR.tv(x, wgt)
    assert r["ties"] >= 1.0 / 3.0, r["ties"]
    assert r["total"] < 2 ** 24 and LR.units(r["loss"] + 8.0, r["scale"]) < LR.LIMIT
    lacc = torch.full((1,), 8.0, device="cuda")
    g = torch.zeros(shape, device="cuda")
    ops.tv_loss(T(x), wgt, lacc, g)
    equal("tv loss %s" % _gid(shape), N(lacc), np.array([r["loss"] + 8.0]))
    equal("tv gradient %s" % _gid(shape), N(g), r["grad"])
    assert np.abs(N(g) / r["scale"]).max() <= 4
    g0 = np.random.RandomState(2).randn(*shape).astype(np.float32)
    g = T(g0)
    ops.tv_loss(T(x), wgt, torch.zeros(1, device="cuda"), g)
    ref = g0.astype(np.float64) + r["grad"]
    check("tv gradient onto g0 %s" % _gid(shape), N(g), ref, U * np.abs(ref))
    lacc = torch.zeros(1, device="cuda")
    ops.tv_loss(T(x), wgt, lacc, None)
    equal("tv loss without g_acc %s" % _gid(shape), N(lacc), np.array([r["loss"]]))
    lacc = torch.full((1,), 3.25, device="cuda")
    g = torch.zeros(shape, device="cuda")
    ops.tv_loss(T(np.full(shape, 7.0)), 0.3, lacc, g)
    assert float(lacc) == 3.25 and not N(g).any()


# ---- 8. average pool ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 7, 9, 4), (1, 2, 2, 12), (3, 8, 6, 64)], ids=_gid)
def test_avgpool2_equals_float64_on_integers(ops, shape):
    """integer inputs: a window's sum and its quarter are exact.  Forward and adjoint equal float64; odd sides floor; the
    gradient beyond 2 (H // 2), 2 (W // 2) is exactly the addend (0 without one); the mask is x > 0 on an x with exact
    zeros; every output starts as NaN"""
    B, H, W, C = shape
    rng = np.random.RandomState(8)
    x = rng.randint(-4, 5, size=shape).astype(np.float32)
    assert (x == 0).any() and (x < 0).any()
    y = ops.avgpool2_fwd(T(x), out=nans(B, H // 2, W // 2, C))
    equal("avgpool2_fwd %s" % _gid(shape), N(y), LR.avgpool2(x))
    gy = rng.randint(-8, 9, size=(B, H // 2, W // 2, C)).astype(np.float32)
    add = rng.randint(-8, 9, size=shape).astype(np.float32)
    g = N(ops.avgpool2_bwd(T(gy), shape, out=nans(*shape)))
    equal("avgpool2_bwd %s" % _gid(shape), g, LR.avgpool2_bwd(gy, shape))
    assert not g[:, 2 * (H // 2):].any() and not g[:, :, 2 * (W // 2):].any()
    gm = N(ops.avgpool2_bwd(T(gy), shape, x=T(x), addend=T(add), out=nans(*shape)))
    equal("avgpool2_bwd masked + addend %s" % _gid(shape), gm, LR.avgpool2_bwd(gy, shape, x=x, addend=add))
    assert np.array_equal(gm[:, 2 * (H // 2):], add[:, 2 * (H // 2):])
    assert np.array_equal(gm[:, :, 2 * (W // 2):], add[:, :, 2 * (W // 2):])
    assert np.array_equal(gm[x <= 0], add[x <= 0])

"""tests/loss_ref.py pinned without a GPU: (1) against the oracle (gram_matrix, style_loss, content_loss, tv_loss) in
float64, (2) against torch float64 autograd of the same expressions -- at the ties of the TV loss and at f == 0 of the
content loss both give 0 --, and (3) every exact input tests/test_loss_gpu.py uses is built here and meets its
precondition (below 2^24 units of its power of two), so that a float32 sum of its terms is exact in any order."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import loss_ref as LR

TOL = 1e-12


def close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= tol * (np.abs(b).max() + 1e-300)), float(np.abs(a - b).max())


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


# ---- (1), (2): the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bs", [1, 2, 4])
def test_gram_and_style_loss_against_the_oracle_and_autograd(Bs):
    rng = np.random.RandomState(3)
    B, h, w, C, wl = 4, 5, 7, 64, 0.7
    F = np.maximum(rng.randn(B, h, w, C), 0) * 30
    S = np.maximum(rng.randn(Bs, h, w, C), 0) * 30
    scale = 1.0 / (2.0 * h * w * C)
    G, mag = LR.gram(F, scale)
    Gs, _ = LR.gram(S, scale)
    close(G, O.gram_matrix(t64(F)).numpy() * scale)
    assert np.all(mag >= np.abs(G)) and np.array_equal(mag, G)            # post-ReLU: every term is its own magnitude
    dev = rng.rand(B) + 0.5
    close(LR.gram(F, 0.5, dev)[0], O.gram_matrix(t64(F)).numpy() * (0.5 * dev)[:, None, None])
    loss, D = LR.style_loss(G, Gs, wl)
    Ft = t64(F, True)
    St = t64(S)[torch.arange(B) % Bs]
    total, _ = O.style_loss({"x": Ft}, {"x": St}, ["x"], [wl])
    close(loss.sum(), float(total.detach()))
    (gF,) = torch.autograd.grad(total, Ft)
    dF, bound = LR.gram_bwd(F, D, scale)
    close(dF, gF.numpy())
    assert np.all(bound >= 0)
    Gt = t64(G, True)
    lt = wl * ((Gt - t64(Gs)[torch.arange(B) % Bs]) ** 2).sum(dim=(1, 2))
    close(loss, lt.detach().numpy())
    (gG,) = torch.autograd.grad(lt.sum(), Gt)
    close(D, gG.numpy())
    bD, bL = LR.style_bounds(G, Gs, wl, LR.gram_bound(mag, h * w, 3), 32)
    assert np.all(bD > 0) and np.all(bL > 0) and np.all(bL < 1e-3 * loss)


@pytest.mark.parametrize("mode", ["channel", "last_channel", "first_rest", "all", "target"])
@pytest.mark.parametrize("signed", [False, True])
def test_content_loss_against_the_oracle_and_autograd(mode, signed):
    rng = np.random.RandomState(17)
    B, h, w, C, wgt, amp = 3, 5, 7, 64, 2.5, 1.7
    pre = rng.randn(B, h, w, C)
    pre[rng.rand(B, h, w, C) < 0.2] = 0.0                               # f == 0: both gradients must be 0 there
    ch = {"channel": 11, "last_channel": C - 1, "first_rest": 1, "all": 0, "target": 5}[mode]
    tgt = rng.rand(2, h, w, C) if mode == "target" else None
    pt = t64(pre, True)
    f = pt if signed else torch.relu(pt)
    ref = wgt * O.content_loss(f, ch, None if tgt is None else t64(tgt)[torch.arange(B) % 2], amp)
    (g_ref,) = torch.autograd.grad(ref, pt)
    F = pre if signed else np.maximum(pre, 0)
    r = LR.content_loss(F, wgt, ch, tgt, amp, signed)
    close(r["loss"].sum(), float(ref.detach()))
    close(r["grad"], g_ref.numpy())
    if mode in ("channel", "last_channel", "first_rest"):
        zero = (pre == 0) & (np.arange(C) != ch)
        assert zero.any() and np.all(r["grad"][zero] == 0) and np.all(g_ref.numpy()[zero] == 0)
    if not signed:
        assert np.all(r["grad"][F <= 0] == 0) and np.all(r["grad_bound"][F <= 0] == 0)
    assert np.all(r["mag"] >= np.abs(r["loss"])) and np.all(r["loss_bound"] > 0)
    g0 = rng.randn(B, h, w, C) * 1e-4
    r0 = LR.content_loss(F, wgt, ch, tgt, amp, signed, g0=g0)
    close(r0["grad"], g0 + r["grad"])
    assert np.all(r0["grad_bound"] >= r["grad_bound"])


@pytest.mark.parametrize("shape", [(2, 9, 11, 3), (2, 1, 50, 3), (2, 50, 1, 1), (2, 37, 23, 3)])
def test_tv_against_the_oracle_and_autograd_with_ties(shape):
    x = LR.tv_image(shape, 5)
    r = LR.tv(x, 2.0 ** -6)
    xt = t64(x, True)
    ref = O.tv_loss(xt) * 2.0 ** -6
    assert r["loss"] == float(ref.detach())
    (g,) = torch.autograd.grad(ref, xt)
    assert np.array_equal(r["grad"], g.numpy())                          # ties included: sign(0) = 0 on both sides
    assert r["ties"] >= 1.0 / 3.0 and np.abs(r["k"]).max() <= 4 and np.array_equal(r["k"], np.round(r["k"]))
    assert LR.units(r["total"], 1.0) < LR.LIMIT and LR.units(np.abs(r["grad"]), r["scale"]) <= 4
    flat = LR.tv(np.full(shape, 7.0), 0.3)
    assert flat["loss"] == 0.0 and not flat["grad"].any() and flat["ties"] == 1.0


@pytest.mark.parametrize("shape", [(2, 7, 9, 4), (1, 2, 2, 12), (3, 8, 6, 64)])
def test_avgpool2_against_autograd(shape):
    rng = np.random.RandomState(8)
    x = rng.randint(-4, 5, size=shape).astype(np.float64)
    assert (x == 0).any()
    xt = t64(x, True)
    ref = torch.nn.functional.avg_pool2d(xt.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    y = LR.avgpool2(x)
    assert np.array_equal(y, ref.detach().numpy()) and y.shape == (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
    gy = rng.randint(-8, 9, size=y.shape).astype(np.float64)
    (gx,) = torch.autograd.grad(ref, xt, t64(gy))
    assert np.array_equal(LR.avgpool2_bwd(gy, shape), gx.numpy())
    add = rng.randint(-8, 9, size=shape).astype(np.float64)
    g = LR.avgpool2_bwd(gy, shape, x=x, addend=add)
    assert np.array_equal(g, gx.numpy() * (x > 0) + add)
    assert np.array_equal(g[:, 2 * (shape[1] // 2):], add[:, 2 * (shape[1] // 2):])
    assert LR.is_f32(y) and LR.is_f32(g)


def test_style_mask_against_the_oracle_and_autograd():
    rng = np.random.RandomState(41)
    B, h, w, C = 2, 8, 6, 16
    F = np.maximum(rng.randn(B, h, w, C), 0)
    m = rng.rand(B, h, w, 1)
    Fm, scale = LR.style_mask_apply(F, m)
    close(Fm, F * m)
    close(scale, 1.0 / (2.0 * m[..., 0].sum(axis=(1, 2)) * C))
    # the oracle's masked style loss of one layer, with the mask in place of its bicubic resize (same size: identity)
    assert np.abs(O.tf1_resize_bicubic(t64(m), h, w).numpy() - m).max() < 1e-12
    S = np.maximum(rng.randn(B, h, w, C), 0)
    pre = t64(rng.randn(B, h, w, C), True)
    total, _ = O.style_loss({"x": torch.relu(pre)}, {"x": t64(S)}, ["x"], [0.7], d_gray=t64(m))
    (g_ref,) = torch.autograd.grad(total, pre)
    Fp = np.maximum(pre.detach().numpy(), 0)
    Fm, scale = LR.style_mask_apply(Fp, m)
    G, _ = LR.gram(Fm, 1.0, scale)
    Gs, _ = LR.gram(S, 1.0 / (2.0 * h * w * C))
    loss, D = LR.style_loss(G, Gs, 0.7)
    close(loss.sum(), float(total.detach()))
    dFm, _ = LR.gram_bwd(Fm, D, 1.0, scale)
    close(LR.style_mask_bwd(dFm, m, Fp), g_ref.numpy())
    with np.errstate(invalid="ignore"):
        assert np.isinf(LR.style_mask_apply(F, np.zeros_like(m))[1]).all()       # an all-zero mask: 1 / 0


# ---- (3): the exact inputs meet their preconditions --------------------------------------------------------------------
@pytest.mark.parametrize("shape,path", LR.GRAM_SHAPES)
@pytest.mark.parametrize("with_dev", [False, True])
def test_exact_gram_inputs(shape, path, with_dev):
    c = LR.gram_case(shape, with_dev=with_dev)
    F = c["F"]
    assert np.array_equal(F, np.round(F)) and np.abs(F).max() <= 3 and (F == 0).mean() > 0.3
    assert (F > 0).any() and (F < 0).any() and F.nbytes <= 8.4e6
    # the plan this shape takes on a chip of 256 compute units is the path it is named for
    B, HW, C = shape
    chunks, pairs, cps = (HW + 31) // 32, B * (C // 64) * (C // 64 + 1) // 2, 16
    while cps > 4 and pairs * ((chunks + cps - 1) // cps) < 512:
        cps >>= 1
    cps = min(cps, chunks)
    if (chunks + cps - 1) // cps > 256:
        cps = (chunks + 255) // 256
    if pairs >= 256 and chunks <= 32:
        cps = chunks
    assert LR.on_path(path, (chunks + cps - 1) // cps, HW), (shape, path, cps)


def test_marker_features_name_pixels_and_pairs():
    B, HW, C = 2, 300, 128
    F = LR.marker_features(B, HW, C)
    assert (F != 0).sum() == B * 16
    G, mag = LR.gram(F, 1.0)
    assert LR.is_f32(G) and np.array_equal(G, mag)
    cs = [c % C for c in LR.MARK_CHANNELS]
    seen = set()
    for b in range(B):
        for j, cj in enumerate(cs):
            for k, ck in enumerate(cs):
                d = LR.marker_decode(G[b, cj, ck], b)
                assert d == "pair a_j+a_k = %d, pixels [0, 31, 32, -1]" % (LR.MARK_A[j] + LR.MARK_A[k]), d
                seen.add(LR.MARK_A[j] + LR.MARK_A[k])
    assert len(seen) == 10 and (G != 0).sum() == B * 16
    F[0, 32] = 0                                                          # a dropped pixel is named
    assert LR.marker_decode(LR.gram(F, 1.0)[0][0, 63, 64]) == "pair a_j+a_k = 4, pixels [0, 31, -1]"


@pytest.mark.parametrize("B,Bs,C", [(3, 1, 64), (3, 3, 128), (4, 2, 128), (2, 1, 512), (2, 2, 512)])
@pytest.mark.parametrize("where", ["diag", "off", "last"])
def test_exact_style_inputs(B, Bs, C, where):
    c = LR.style_case(B, Bs, C, where, 11)
    E = c["E"]
    assert np.array_equal(E, E.transpose(0, 2, 1)) and np.abs(E).max() == 3
    n = C // 64
    tiles = {(i, j) for i in range(n) for j in range(n) if E[:, 64 * i:64 * i + 64, 64 * j:64 * j + 64].any()}
    t = 1 if n > 2 else 0
    assert tiles == {"diag": {(t, t)}, "off": {(0, n - 1), (n - 1, 0)}, "last": {(n - 1, n - 1)}}[where]
    assert np.all(c["loss"] > 0)


@pytest.mark.parametrize("Bs", [1, 3])
def test_exact_group_inputs(Bs):
    B = 3
    layers = LR.group_case(B, Bs, LR.GROUP_LAYERS)
    assert sum(y["exact"] for y in layers) == 4 and len(layers) == 7
    for y in layers:
        assert np.array_equal(y["Gs"], y["Gs"].transpose(0, 2, 1))
        if Bs == 1:
            assert not np.array_equal(y["F"][1], y["F"][0]) and np.array_equal(y["G"][1], y["G"][0])
    ws, parts = LR.group_plan([(y["HW"], y["C"]) for y in layers], B)
    # 1600 px: 4 slabs, 1295 px (3 pairs): 3 slabs, 1025 px: 3 slabs; the others one slab
    assert ws == B * 4096 * (4 + 3 * 3 + 3) and parts == 16 + 48 + 16 + 1 + 36 + 36 + 1


def test_exact_mask_chain_inputs():
    m = LR.mask01(2, 40, 37, (128, 256), 3)
    assert m.reshape(2, -1).sum(axis=1).tolist() == [128.0, 256.0] and set(np.unique(m)) == {0.0, 1.0}
    F = np.maximum(LR.int_features(2, 40 * 37, 64, 4), 0).reshape(2, 40, 37, 64)
    Fm, scale = LR.style_mask_apply(F, m)
    assert scale.tolist() == [2.0 ** -14, 2.0 ** -15]
    G, mag = LR.gram(Fm, 1.0, scale)
    assert LR.is_f32(G) and all(LR.units(mag[b], scale[b]) < LR.LIMIT for b in range(2))


def test_the_precondition_refuses_what_is_not_exact():
    with pytest.raises(AssertionError):
        LR.units(3.0, 0.3)
    with pytest.raises(AssertionError):
        LR.units(0.75, 0.5)
    assert LR.units(2.0 ** 24, 1.0) == LR.LIMIT and not LR.is_f32(2.0 ** 24 + 1) and LR.is_f32(2.0 ** 24)
    assert LR.err_ratio([0.0, 1.0], [0.0, 2.0]) == 0.5 and LR.err_ratio([1.0], [0.0]) == np.inf
    assert LR.err_ratio([np.nan], [1.0]) == np.inf

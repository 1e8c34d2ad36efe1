"""tests/conv_ref.py pinned without a GPU: the float64 restatement against torch's conv2d and autograd in float64, the
Winograd matrices against the direct sum, the float32 restatement inside the worst-case bound on every realistic input the
GPU module uses, planted defects outside it, and the conditions on the inputs (exact units, undecided share)."""
import numpy as np
import pytest
import torch

from tests import conv_ref as R
from tests import switch_runs as SR

TOL = 1e-12


def _torch_conv(x, w, bias=None):
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), bias, padding=1)
    return y.permute(0, 2, 3, 1)


def _small(seed=3, shape=(2, 7, 9, 5, 6)):
    B, H, W, Ci, Co = shape
    rng = np.random.RandomState(seed)
    return (rng.randn(B, H, W, Ci), rng.randn(3, 3, Ci, Co), rng.randn(Co), rng.randn(B, H, W, Co), rng.randn(B, H, W, Ci),
            rng.randn(B, H, W, Ci))


def test_conv_and_dgrad_equal_torch_float64():
    x, w, b, gy, x_in, add = _small()
    xt = torch.tensor(x, requires_grad=True)
    pre = _torch_conv(xt, torch.tensor(w), torch.tensor(b))
    y, S = R.conv(x, w, b, relu=True)
    scale = S.max()
    assert np.abs(y - torch.relu(pre).detach().numpy()).max() <= TOL * scale
    assert np.abs(R.conv(x, w, b)[0] - pre.detach().numpy()).max() <= TOL * scale
    assert np.all(S >= np.abs(R.conv(x, w)[0]) - TOL * scale)
    (gx,) = torch.autograd.grad(pre, xt, torch.tensor(gy))
    g, Sg = R.dgrad(gy, w)
    assert np.abs(g - gx.numpy()).max() <= TOL * Sg.max()
    # the layer rules
    m = x_in > 0
    assert np.array_equal(R.layer_dgrad(g, x_in, add), g * m + add)
    assert np.array_equal(R.layer_dgrad(g, x_in, add, addend_unmasked=True), (g + add) * m)
    assert np.array_equal(R.layer_dgrad(g), g)


@pytest.mark.parametrize("H,W", [(7, 9), (8, 6), (2, 3)])
def test_pooled_rules_equal_autograd(H, W):
    """y_pool = avg_pool2d(relu(conv)) and the pooled gradient 0.25 gy_pool[h/2, w/2] (x_out > 0), zero beyond the floor"""
    x, w, b, _, x_in, add = _small(5, (2, H, W, 4, 3))
    xt = torch.tensor(x, requires_grad=True)
    yt = torch.relu(_torch_conv(xt, torch.tensor(w), torch.tensor(b)))
    pt = torch.nn.functional.avg_pool2d(yt.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    y, S = R.conv(x, w, b, relu=True)
    assert np.abs(R.avgpool2(y) - pt.detach().numpy()).max() <= TOL * S.max()
    gp = np.random.RandomState(1).randn(*pt.shape)
    (gx,) = torch.autograd.grad(pt, xt, torch.tensor(gp))
    g_y = R.pooled_gy(gp, y > 0)
    assert not g_y[:, 2 * (H // 2):].any() and not g_y[:, :, 2 * (W // 2):].any()
    g, Sg = R.dgrad(g_y, w)
    assert np.abs(g - gx.numpy()).max() <= TOL * max(Sg.max(), 1.0)


@pytest.mark.parametrize("m", [2, 4, 5])
@pytest.mark.parametrize("shape", [(2, 11, 13, 6, 5), (1, 5, 5, 3, 4), (1, 2, 3, 2, 2), (2, 20, 20, 4, 4)])
def test_winograd_float64_equals_the_direct_sum(m, shape):
    """proves G, B^T and A^T of the three families (and the tiling: ragged edges, a single tile)"""
    x, w = _small(11, shape)[:2]
    y, _ = R.conv(x, w)
    aw = R.winograd64(x, w, m, absolute=True)
    assert np.abs(R.winograd64(x, w, m) - y).max() <= TOL * aw.max()
    yd, _ = R.dgrad(_small(11, shape)[3], w)
    assert np.abs(R.winograd64(_small(11, shape)[3], R.dgrad_filters(w), m) - yd).max() <= TOL * aw.max() * 10
    assert np.all(aw >= np.abs(y))


def _directions(shape, key_f, key_g, pooled):
    """(name, input of the GEMM, filters, tile) of the forward pass and of the data gradient of a layer case"""
    d = R.layer_inputs(shape, pooled)
    out = [("fwd", d["x"], d["w"], R.tile_of(key_f))]
    if not pooled:
        out.append(("dgrad", d["gy"], R.dgrad_filters(d["w"]).astype(np.float32), R.tile_of(key_g)))
    return out


ALL_LAYERS = [(c[0], c[1], c[2], False) for c in R.PLAIN_LAYERS] + [(c[0], c[1], c[2], True) for c in R.POOLED_LAYERS]


@pytest.mark.parametrize("shape,key_f,key_g,pooled", ALL_LAYERS)
def test_float32_restatement_is_inside_the_bound(shape, key_f, key_g, pooled):
    """float32 rounding alone stays far inside the bound on every realistic input the GPU module restates (the cases of at
    most PRECISION_TILES tiles): at most 1 % of it.  The kernels are then held to 8 x the restatement's own ratio"""
    for name, a, f, m in _directions(shape, key_f, key_g, pooled):
        if R.tiles(shape, m) > R.PRECISION_TILES:
            continue
        ch = slice(0, R.RESTATED_CHANNELS)
        y, _ = R.conv(a, f)
        got = R.winograd32(a, f, m, ch)
        r = R.err_ratio(np.abs(got - y[..., ch]), R.wino_bound(a, f[..., ch], m, y[..., ch]))
        assert 0 < r < 0.01, (name, r)


def _f2x2_directions(shape):
    d = R.layer_inputs(shape)
    return [("fwd", d["x"], d["w"]), ("dgrad", d["gy"], R.dgrad_filters(d["w"]).astype(np.float32))]


@pytest.mark.parametrize("shape", SR.CONV_PLAIN, ids=["x".join(map(str, s)) for s in SR.CONV_PLAIN])
def test_f2x2_float32_restatement_is_inside_its_own_bound(shape):
    """F(2x2) as NFS_WINOGRAD_TILE=2 runs it, restated in float32 on every layer of the switch battery (forward and data
    gradient, the first 32 output channels): float32 rounding alone stays below 2 % of the c2 = 12 bound, and that bound
    is several times tighter than F(4x4)'s on the same input (printed), which is why F(2x2) is not held to the latter"""
    ch = slice(0, R.RESTATED_CHANNELS)
    for name, a, f in _f2x2_directions(shape):
        y, _ = R.conv(a, f[..., ch])
        b2, b4 = R.wino_bound(a, f[..., ch], 2, y), R.wino_bound(a, f[..., ch], 4, y)
        r = R.err_ratio(np.abs(R.winograd32(a, f, 2, ch) - y), b2)
        print("F(2x2) %s %s: float32 restatement err / bound %.5f, F(4x4) bound / F(2x2) bound %.1f (median)"
              % (shape, name, r, np.median(b4 / b2)))
        assert 0 < r < 0.02, (name, r)
        assert np.median(b4 / b2) > 3.0, (name, np.median(b4 / b2))


def test_f2x2_dropped_output_term_exceeds_the_bound():
    """a term of an F(2x2) output row dropped (A^T row 1 without its last entry): every second output row and, after the
    second pass, every second column is wrong by a whole transform component -- far outside the bound wherever the
    component is not tiny; the intact algorithm stays inside everywhere"""
    x, w, _ = R.realistic(1, 9, 11, 64, 32, 2)
    y, _ = R.conv(x, w)
    bound = R.wino_bound(x, w, 2, y)
    assert not (np.abs(R.winograd64(x, w, 2) - y) > bound).any()
    keep = R.MATS[2]
    try:
        broken = keep[2].copy()
        broken[1, 3] = 0.0
        R.MATS[2] = (keep[0], keep[1], broken)
        z = R.winograd64(x, w, 2)
    finally:
        R.MATS[2] = keep
    bad = np.abs(z - y) > bound
    assert bad[:, 1::2].mean() > 0.9 and bad[:, :, 1::2].mean() > 0.9 and not bad[:, 0::2, 0::2].any()


def _planted(shape=(1, 9, 11, 64, 32), seed=2):
    B, H, W, K, N = shape
    x, w, bias = R.realistic(B, H, W, K, N, seed)
    pre, _ = R.conv(x, w, bias)
    y = np.maximum(pre, 0)
    return x, w, bias, pre, y, R.wino_bound(x, w, 4, y)


def _only(bad, region):
    return bad[region].all() and not (bad & ~region).any()


def test_planted_defects_exceed_the_bound_where_they_touch_and_nowhere_else():
    x, w, bias, pre, y, bound = _planted()
    B, H, W, K = x.shape
    live = pre > bound                                   # (a defect under a closed ReLU changes nothing)

    def outside(z):
        return np.abs(z - y) > bound

    # one tap dropped at one pixel
    h, v, r, s = 4, 5, 0, 2
    z = np.maximum(pre.copy(), 0)
    z[0, h, v] = np.maximum(pre[0, h, v] - x[0, h + r - 1, v + s - 1].astype(np.float64) @ w[r, s].astype(np.float64), 0)
    region = np.zeros(y.shape, bool)
    region[0, h, v] = (y[0, h, v] > bound[0, h, v]) | (z[0, h, v] > bound[0, h, v])     # (not both under a closed ReLU)
    assert region.sum() > 8 and _only(outside(z), region)
    # the last ragged row (H = 9: row 8 is the only row of the third tile row) taken from the next tile (the next image
    # row of tiles does not exist: zeros before bias)
    z = y.copy()
    z[:, 8] = np.maximum(bias.astype(np.float64), 0)
    bad = outside(z)
    assert (bad[:, 8].mean() > 0.5) and not bad[:, :8].any()
    # one 16-channel K slice dropped at K = 64
    x2 = x.copy()
    x2[..., 16:32] = 0
    z = np.maximum(R.conv(x2, w, bias)[0], 0)
    bad = outside(z)
    assert bad[live].mean() > 0.99, bad[live].mean()
    # a pool window read past the floor: H = 9 floors to 4 pooled rows; a fifth window would average row 8 with nothing
    yp = R.avgpool2(y)
    pb = R.pool_bound(bound, yp)
    zp = yp.copy()
    zp[:, 3] = 0.25 * (y[:, 7, 0:10:2] + y[:, 7, 1:10:2] + y[:, 8, 0:10:2] + y[:, 8, 1:10:2])     # rows 7, 8 instead of 6, 7
    bad = np.abs(zp - yp) > pb
    assert bad[:, 3].mean() > 0.9 and not bad[:, :3].any()
    # one mask bit flipped in the data gradient
    gy = np.random.RandomState(4).randn(*y.shape).astype(np.float32)
    g, _ = R.dgrad(gy, w)
    mask = x > 0
    gx = R.layer_dgrad(g, mask=mask)
    gb = R.wino_bound(gy, R.dgrad_filters(w), 4, gx) * mask
    idx = np.unravel_index(np.argmax(np.abs(g) * ~mask), g.shape)      # a closed entry whose gradient is live
    m2 = mask.copy()
    m2[idx] = True
    bad = np.abs(R.layer_dgrad(g, mask=m2) - gx) > gb
    assert bad[idx] and bad.sum() == 1


def test_exact_inputs_stay_below_2_24_units():
    for K, N in [(3, 64), (3, 128), (64, 64), (64, 128), (512, 64), (512, 128)]:
        x = R.int_tensor((2, 13, 11, K), 1)
        w = R.int_tensor((3, 3, K, N), 2)
        y, S = R.conv(x, w)
        assert R.exact_units(S, 3.0) <= 9 * K * 9 + 3
        g, Sg = R.dgrad(R.int_tensor((2, 13, 11, N), 3), w)
        assert R.exact_units(Sg, 3.0) <= 9 * N * 9 + 3
    with pytest.raises(AssertionError):
        R.exact_units(np.array([2.0 ** 24]))
    with pytest.raises(AssertionError):
        R.exact_units(np.array([0.5]))


@pytest.mark.parametrize("case", R.POOLED_LAYERS)
def test_undecided_share_of_the_pooled_cases(case):
    """a ReLU mask is undecided where |pre| <= bound; a condition on the inputs, from the reference alone"""
    shape, key_f = case[0], case[1]
    d = R.layer_inputs(shape, True)
    pre, _ = R.conv(d["x"], d["w"], d["bias"])
    share = R.undecided(pre, R.wino_bound(d["x"], d["w"], R.tile_of(key_f), np.maximum(pre, 0))).mean()
    print("undecided share %s: %.4f" % (shape, share))
    assert share <= R.UNDECIDED_CAP


def test_decode_names_image_tile_position_channel():
    shape = (2, 9, 11, 8)
    flat = np.ravel_multi_index((1, 6, 9, 5), shape)
    assert R.decode(flat, shape, 4) == "image 1 tile (1, 2) at (2, 1) channel 5"
    got = np.zeros(shape)
    ref = np.zeros(shape)
    got.reshape(-1)[flat] = np.nan
    assert "image 1 tile (1, 2) at (2, 1) channel 5" in R.first_mismatches(got, ref, 1.0, 4)
    assert R.first_mismatches(ref, ref, 0.0, 4) == ""

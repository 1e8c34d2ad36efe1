"""The histogram loss kernels (csrc/hist.hip) element by element against the exact restatement of tests/hist_ref.py.

Inputs are drawn at random and then settled (hist_ref.settle): no bin coordinate lies within 8 float32 ulps of a bin
edge, so every discrete decision -- both histograms, the interpolated template bin with its rightmost-equal-quantile
rule and round-half-to-even, the apply bin -- is the restatement's, and every gradient element can be held to a few
ulps with no fraction of the output exempt.  Each case names the entry point it runs: the pixel-parallel
``nfs_hist_loss_wide`` (what ops.hist_loss takes for C <= 4 and C % 4 == 0 up to 128), the per-channel
``nfs_hist_loss`` and ``nfs_hist_loss_masked``."""
import numpy as np
import pytest
import torch

from tests import hist_ref as H

pytestmark = pytest.mark.gpu

F32 = np.float32


def draw(rng, kind, shape):
    if kind == "relu":                               # post-ReLU layer: many exact zeros
        x = rng.gamma(2.0, 15.0, shape)
        x[rng.rand(*shape) < 0.3] = 0.0
    elif kind == "pre_relu":                         # a *_pre_relu layer: both signs
        x = rng.randn(*shape) * 40.0 - 5.0
    else:                                            # image-like: the loss-net input layer
        x = rng.rand(*shape) * 255.0
    return x.astype(F32)


def run(via, f, t, m, w, relu, loss0, g0):
    """one call of the named entry point on copies of the prefilled accumulators; returns (loss, g) as NumPy"""
    from neural_flow_style_amd import _lib, ops
    B, C, Bt = f.shape[0], f.shape[-1], t.shape[0]
    HW, HWt = f.size // (B * C), t.size // (Bt * C)
    F, T = torch.tensor(f).cuda(), torch.tensor(t).cuda()
    M = None if m is None else torch.tensor(m).reshape(B, -1).cuda().contiguous()
    loss, g = torch.tensor(loss0).cuda(), torch.tensor(g0).cuda()
    if via == "ops":
        ops.hist_loss(F, T, w, loss, g, relu_mask=relu, mask=M)
    elif via == "nfs_hist_loss_wide":
        nws = _lib.lib().nfs_hist_loss_wide_workspace_floats(B, C, HW, HWt)
        ws = torch.full((nws,), float("nan"), device="cuda")            # the pipeline must not read stale state
        _lib.call(via, ops._ptr(F), ops._ptr(T), ops._ptr(M), ops._ptr(loss), ops._ptr(g), ops._ptr(ws), nws, B, Bt, HW,
                  HWt, C, float(w), int(relu), ops._stream())
    elif via == "nfs_hist_loss":
        assert M is None
        _lib.call(via, ops._ptr(F), ops._ptr(T), ops._ptr(loss), ops._ptr(g), B, Bt, HW, HWt, C, float(w), int(relu),
                  ops._stream())
    else:
        _lib.call(via, ops._ptr(F), ops._ptr(T), ops._ptr(M), ops._ptr(loss), ops._ptr(g), B, Bt, HW, HWt, C, float(w),
                  int(relu), ops._stream())
    torch.cuda.synchronize()
    return loss.cpu().numpy(), g.cpu().numpy()


def check(name, via, f, t, m=None, w=1.0, relu=False, prefill=False, seed=0):
    """run and hold every element to the restatement; returns the largest gradient error in ulps"""
    rng = np.random.RandomState(seed + 1000)
    B, C = f.shape[0], f.shape[-1]
    f, t = H.settle(f, t, mask=m)
    r = H.reference(f, t, weight=w, mask=m, relu_mask=relu)
    assert np.all(r["margin"] >= 8) and np.all(r["margin_t"] >= 8)
    loss0 = (rng.rand(B) * 50).astype(F32) if prefill else np.zeros(B, F32)
    g0 = (rng.randn(*f.shape) * 10).astype(F32) if prefill else np.zeros(f.shape, F32)
    loss, g = run(via, f, t, m, w, relu, loss0, g0)
    g = g.reshape(B, -1, C)
    g0 = g0.reshape(B, -1, C)
    want = g0.astype(np.float64) + r["grad"].astype(np.float64)            # r["grad"]: 2w (v - matched) alone
    # elements that take no gradient keep the accumulator's bits: masked out, flat / empty channels, ReLU zeros
    fv = f.reshape(B, -1, C)
    live = np.ones(fv.shape[:2], bool) if m is None else np.asarray(m).reshape(B, -1) != 0
    takes = live[..., None] & ~r["skip"][:, None, :] & ((fv > 0) if relu else True)
    assert np.array_equal(g[~takes], g0[~takes])
    assert np.all(r["grad"][~takes] == 0)
    # the rest: 4 ulps of the channel's largest magnitude (a contracted multiply-add in the table may move the matched
    # value by a rounding), times 2w, plus the rounding of the accumulation
    mag = np.maximum(np.abs(r["vmin"]), np.abs(r["vmax"]))[:, None, :]
    unit = np.spacing(mag.astype(F32)).astype(np.float64) * 2 * abs(w)
    err = np.abs(g.astype(np.float64) - want)
    tol = 4 * unit + np.spacing(np.abs(want).astype(F32))
    bad = err > tol
    assert not bad.any(), "%s: %d elements off, worst %.3g ulp at %s" % (
        name, bad.sum(), (err / unit)[bad].max(), np.argwhere(bad)[:5].tolist())
    worst = float(np.where(takes, err / np.where(unit > 0, unit, 1), 0).max())
    # per-image loss: the float64 sum of the float32 differences within a float32 summation bound, added to loss0
    tot = loss0.astype(np.float64) + r["loss"]
    assert np.all(np.abs(loss - tot) <= 1e-5 * r["loss"] + 2 * np.spacing(tot.astype(F32))), (name, loss, tot)
    assert np.all((r["loss"] == 0) == r["skip"].all(1))
    print("hist %-34s %-22s max grad err %.2f ulp" % (name, via, worst))
    return worst


def random_case(seed, B, hw, C, Bt, thw, kind, mask=None):
    """feat [B,h,w,C] / templ [Bt,ht,wt,C] of ``kind``, with image 0's first element the exact joint maximum of every
    channel; mask: None, 'frac' (bicubic-like fractional values incl. small negatives, 30 % exact zeros), 'frac_empty'
    (and the last image fully masked out), 'single' (the last image keeps one live pixel)"""
    rng = np.random.RandomState(seed)
    f = draw(rng, kind, (B,) + hw + (C,))
    t = draw(rng, kind, (Bt,) + thw + (C,))
    f[0, 0, 0] = np.maximum(f.max((0, 1, 2)), t.max((0, 1, 2))) + F32(1.5)
    m = None
    if mask is not None:
        m = (rng.rand(B, *hw) * 1.2 - 0.05).astype(F32)
        m[rng.rand(B, *hw) < 0.3] = 0.0
        m[:, 0, 0] = 0.75
        if mask == "frac_empty":
            m[-1] = 0.0
        elif mask == "single":
            m[-1] = 0.0
            m[-1, hw[0] // 2, hw[1] - 1] = 0.01
    return f, t, m


# (id, entry point, seed, B, (h, w), C, Bt, (ht, wt), kind, mask, weight, relu, prefill)
CASES = [
    ("hw1-Bt=B", "ops", 1, 2, (1, 1), 1, 2, (6, 7), "pre_relu", None, 0.7, False, True),
    ("150x225-tpl120x200-mask", "ops", 2, 2, (150, 225), 3, 1, (120, 200), "image", "frac", 0.3, False, False),
    ("hw256-1<Bt<B-flat-relu", "ops", 3, 3, (16, 16), 4, 2, (7, 9), "relu", None, 1.5, True, True),
    ("hw257-emptyimage", "ops", 4, 2, (1, 257), 8, 2, (5, 5), "pre_relu", "frac_empty", 0.7, False, False),
    ("1<Bt<B-singlepixel-relu", "ops", 5, 3, (12, 17), 64, 2, (9, 9), "relu", "single", 2.0, True, False),
    ("hw37-prefill", "ops", 6, 2, (1, 37), 128, 1, (9, 11), "pre_relu", None, 0.25, False, True),
    ("C5-flat-relu", "ops", 7, 2, (13, 11), 5, 1, (9, 14), "relu", None, 0.7, True, False),
    ("C12-1<Bt<B-prefill", "nfs_hist_loss", 8, 3, (16, 16), 12, 2, (8, 8), "pre_relu", None, 1.3, False, True),
    ("C256-hw37-Bt=B-relu", "ops", 9, 2, (1, 37), 256, 2, (6, 7), "relu", None, 0.7, True, False),
    ("C4-hw257-emptyimage-prefill", "nfs_hist_loss_masked", 10, 3, (1, 257), 4, 2, (6, 6), "pre_relu", "frac_empty",
     0.7, False, True),
    ("C64-singlepixel-relu", "nfs_hist_loss_masked", 11, 2, (20, 19), 64, 1, (8, 9), "relu", "single", 1.1, True, False),
    ("C256-hw256-Bt=B-mask", "nfs_hist_loss_masked", 12, 2, (16, 16), 256, 2, (5, 6), "pre_relu", "frac", 0.5, False,
     True),
]


def _path(via, C, masked):
    if via != "ops":
        return via
    return "wide" if C <= 4 or (C % 4 == 0 and C <= 128) else ("masked" if masked else "channel")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-C%d-%s" % (_path(c[1], c[5], c[9] is not None), c[5], c[0]))
def test_hist_loss_every_element_matches_the_restatement(case):
    name, via, seed, B, hw, C, Bt, thw, kind, mask, w, relu, prefill = case
    f, t, m = random_case(seed, B, hw, C, Bt, thw, kind, mask)
    if "flat" in name:                                # one channel constant over image 0 and its template
        f[0, ..., 1] = 7.5
        t[0, ..., 1] = 7.5
        f[0, 0, 0, 1] = 7.5
    worst = check(name, via, f, t, m, w, relu, prefill, seed)
    assert worst <= 4


@pytest.mark.parametrize("via", ["nfs_hist_loss_wide", "nfs_hist_loss", "nfs_hist_loss_masked"])
def test_hist_loss_exact_ties_and_template_plateaus(via):
    """the constructed tables of hist_ref: source quantiles exactly half-way between two template quantiles (power-of-two
    totals -- round half to even picks the even bin) and source quantiles equal to a template quantile repeated over a
    run of empty template bins (the rightmost equal one is taken); two images, each against its own template (Bt = B)"""
    f0, t0 = H.half_tie_case(-3.7, 11.3)
    f1, t1 = H.half_tie_case(2.0, 300.0)
    f = np.concatenate([f0, f1]).reshape(2, -1, 1)
    t = np.concatenate([t0, t1]).reshape(2, -1, 1)
    m = None if via != "nfs_hist_loss_masked" else np.ones(f.shape[:2], F32)
    check("half-even ties", via, f, t, m, w=0.9, prefill=True)
    p0, q0 = H.plateau_case(-20.0, 7.0)
    p1, q1 = H.plateau_case(0.5, 90.0)
    f, t = np.concatenate([p0, p1]), np.concatenate([q0, q1])
    m = None if via != "nfs_hist_loss_masked" else np.ones(f.shape[:2], F32)
    check("rightmost-equal plateaus", via, f, t, m, w=1.0)


def test_hist_loss_default_layer_at_the_dambreak2d_size():
    """the default hist layer (the 3-channel loss-net input) at 512 x 1024 on the pixel-parallel path: hundreds of
    blocks per (image, channel) flush their histograms into the same workspace state"""
    f, t, _ = random_case(13, 1, (512, 1024), 3, 1, (256, 384), "image")
    check("512x1024x3", "ops", f, t, w=0.5, prefill=True, seed=13)

"""The element-exact histogram-loss restatement of tests/hist_ref.py against the oracle (util.histogram_match_tf restated
with SciPy's interp1d), and its input generator: the restatement must be the oracle value for value wherever the oracle
is defined, and ``settle`` must leave every bin decision unambiguous without moving the range."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import hist_ref as H


def oracle_matched(f, t, mask=None):
    """oracle.histogram_match per (image, channel) of the live source pixels -> [B, HW, C] (source where masked out)"""
    B, C, Bt = f.shape[0], f.shape[-1], t.shape[0]
    fv, tv = f.reshape(B, -1, C), t.reshape(Bt, -1, C)
    live = np.ones(fv.shape[:2], bool) if mask is None else np.asarray(mask).reshape(B, -1) != 0
    out = fv.copy()
    for b in range(B):
        for c in range(C):
            if live[b].any():
                out[b, live[b], c] = O.histogram_match(fv[b, live[b], c], tv[min(b, Bt - 1), :, c])
    return out


def check_against_oracle(f, t, mask=None, w=0.7):
    r = H.reference(f, t, weight=w, mask=mask)
    want = oracle_matched(f, t, mask)
    assert np.array_equal(r["matched"], want)
    lo = float(O.hist_loss(torch.tensor(f, dtype=torch.float64), torch.tensor(t),
                           mask=None if mask is None else torch.tensor(mask)))
    assert abs(float(r["loss"].sum()) - w * lo) <= 1e-6 * max(w * lo, 1e-30)     # d rounded to float32 here
    return r


def draw(rng, kind, shape):
    if kind == "gamma_relu":                         # post-ReLU layer: many exact zeros
        x = rng.gamma(2.0, 15.0, shape)
        x[rng.rand(*shape) < 0.3] = 0.0
    elif kind == "pre_relu":                         # a *_pre_relu layer: both signs
        x = rng.randn(*shape) * 40.0 - 5.0
    elif kind == "offset":                           # a narrow range far from 0
        x = 1000.0 + rng.rand(*shape) * 3.0
    else:                                            # image-like input layer
        x = rng.rand(*shape) * 255.0
    return x.astype(np.float32)


CASES = [  # (B, h, w, C, Bt, ht, wt, kind, masked)
    (2, 13, 11, 5, 1, 9, 14, "gamma_relu", False),
    (1, 20, 20, 3, 1, 20, 20, "image", False),
    (3, 16, 16, 4, 2, 8, 33, "pre_relu", True),
    (2, 1, 1, 3, 2, 7, 5, "pre_relu", False),
    (2, 1, 257, 2, 1, 16, 16, "offset", True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:4])) + "-Bt%d-%s%s" % (c[4], c[7], "-mask" * c[8]))
def test_restatement_equals_the_oracle_on_settled_inputs(case):
    B, h, w, C, Bt, ht, wt, kind, masked = case
    rng = np.random.RandomState(sum(map(ord, kind)) + B * h * w * C)
    f = draw(rng, kind, (B, h, w, C))
    t = draw(rng, kind, (Bt, ht, wt, C))
    m = None
    if masked:
        m = (rng.rand(B, h, w) * (rng.rand(B, h, w) < 0.7)).astype(np.float32)
        m[:, 0, 0] = 0.5                                    # at least one live pixel per image
    fs, ts = H.settle(f, t, mask=m)
    r = check_against_oracle(fs, ts, m)
    assert np.all(r["margin"] >= 8) and np.all(r["margin_t"] >= 8)
    assert not r["skip"].all()


def test_restatement_on_the_oracle_known_answer_cases():
    """the cases of test_oracle_kat.py::test_histogram_match_known_answers_and_the_skipped_cases, through the
    restatement: element for element the oracle's matched values, and the skipped flat / empty cases"""
    src = np.arange(255, dtype=np.float32)
    tpl = np.repeat(src, 2)
    r = check_against_oracle(src.reshape(1, 255, 1), tpl.reshape(1, 510, 1))
    # identical CDFs: every quantile is a template quantile, so the table is the identity
    assert np.array_equal(r["table"][0, :, 0], np.arange(255))
    src = np.linspace(0, 1, 101, dtype=np.float32)
    tpl = np.linspace(3, 4, 50, dtype=np.float32)
    check_against_oracle(src.reshape(1, 101, 1), tpl.reshape(1, 50, 1))
    f = np.full((1, 4, 3, 1), 2.5, np.float32)
    r = check_against_oracle(f, np.full((1, 5, 1), 2.5, np.float32))
    assert r["skip"].all() and r["loss"][0] == 0.0 and np.array_equal(r["matched"].reshape(f.shape), f)
    rng = np.random.RandomState(0)
    feat = rng.rand(1, 6, 5, 2).astype(np.float32) * 10
    templ = rng.rand(1, 4, 4, 2).astype(np.float32) * 10
    mask = (rng.rand(1, 6, 5, 1) < 0.5).astype(np.float32)
    r = check_against_oracle(feat, templ, mask)
    assert np.all(r["grad"][0][mask.reshape(-1) == 0] == 0)
    r = check_against_oracle(feat, templ, np.zeros((1, 6, 5, 1), np.float32))
    assert r["skip"].all() and r["loss"][0] == 0.0 and not r["grad"].any()


def test_constructed_tables_rightmost_rule_and_half_even():
    """the two constructions the GPU tests rely on, against the oracle and against their closed forms"""
    f, t = H.half_tie_case(-3.7, 11.3)
    r = check_against_oracle(f, t)
    n = r["table"][0, :, 0]
    # source bin k sits exactly half-way between template quantiles k and k+1: rint takes the even one
    k = np.arange(253)
    assert np.array_equal(n[:253], np.where(k % 2 == 0, k, k + 1)) and n[253] == 253 and n[254] == 254
    assert np.all(r["margin"] >= 8) and np.all(r["margin_t"] >= 8)
    f, t = H.plateau_case(-20.0, 7.0)
    r = check_against_oracle(f, t)
    n = r["table"][0, :, 0]
    hs = np.bincount(np.clip(np.floor(255 * (f.ravel() + 20.0) / 27.0), 0, 254).astype(int), minlength=255)
    # identical CDFs with runs of empty bins: a source bin before a run maps past it (the rightmost equal quantile)
    live = np.flatnonzero(hs)
    assert np.array_equal(n[live[:-1]], live[1:] - 1)
    assert np.any(live[1:] - live[:-1] > 1)
    assert np.all(r["margin"] >= 8) and np.all(r["margin_t"] >= 8)


def test_settle_gives_the_margin_and_keeps_the_range():
    rng = np.random.RandomState(3)
    # a lattice: every value on a bin edge of 0 ... 255 (the worst case), and arbitrary ranges
    for lo, hi, shape in ((0.0, 255.0, (2, 16, 16, 3)), (-7.25, 3.5, (1, 40, 30, 4)), (100.0, 100.5, (1, 64, 1, 2))):
        f = (lo + (hi - lo) * rng.randint(0, 256, shape) / 255.0).astype(np.float32)
        t = (lo + (hi - lo) * rng.randint(0, 256, (1, 20, 20, shape[-1])) / 255.0).astype(np.float32)
        f[0, 0, 0], t[0, 0, 0] = lo, hi                     # both ends present
        r0 = H.reference(f, t)
        assert (r0["margin"] < 8).any()                      # the lattice is ambiguous to begin with
        fs, ts = H.settle(f, t)
        r = H.reference(fs, ts)
        assert np.all(r["margin"] >= 8) and np.all(r["margin_t"] >= 8)
        assert np.array_equal(r["vmin"], r0["vmin"]) and np.array_equal(r["vmax"], r0["vmax"])
        moved = (fs != f).reshape(r0["margin"].shape)
        assert np.array_equal(moved, r0["margin"] < 8)       # exactly the ambiguous source elements moved

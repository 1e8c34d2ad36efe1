"""tests/splat_ref.py pinned without a GPU: against the oracle run in float64 (values and autograd gradients: a second
derivation of the closed-form adjoints), against the pure-Python loops, on hand-made particles whose cell and clamp
are exact in float32, and against a float32 NumPy replay of the kernel's own order of operations, which must stay
inside the bounds before a GPU sees them."""
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import splat_ref as SR

f32 = np.float32


def _particles(rng, N, nd, lo=-0.06, hi=1.06):
    return torch.tensor(rng.uniform(lo, hi, (N, nd)).astype(np.float32))


def _close(a, b, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# (nd, res, domain, radius): domains representable in float32, cell != 1 in both dimensions
GEOM = {2: ([9, 13], [2.25, 3.25], 0.125), 3: ([5, 7, 6], [2.5, 3.5, 3.0], 0.25)}


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("nsize", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_restatement_matches_oracle_in_float64(nd, nsize, clip, mode):
    rng = np.random.RandomState(100 * nd + 10 * nsize + mode)
    res, dom, radius = GEOM[nd]
    N, C = 70, 3
    p = _particles(rng, N, nd)
    S = SR.Splat(nd, res, dom, radius, 4.0, 1000.0, nsize, clip, mode, discrete=torch.float64)
    assert not bool(S.near_tie(p).any())
    p64 = p.double()[None].requires_grad_()
    attr = torch.tensor(rng.uniform(-1, 1, (N, C)).astype(np.float32))
    pd = torch.tensor(rng.uniform(800, 1200, (N,)).astype(np.float32))
    a64 = attr.double()[None].requires_grad_()
    d64 = pd.double()[None, :, None].requires_grad_()
    g = torch.tensor(rng.randn(*res, 1 if mode == 0 else C))
    if mode == 0:
        ref = O.p2g(p64, dom, res, radius, 1000.0, nsize, is_2d=nd == 2, clip=clip)
        out = S.p2g(p)
        assert _close(out["grid"], ref[0])
        (gp,) = torch.autograd.grad(ref, p64, g[None])
        b = S.p2g_bwd(p, g)
        assert _close(b["g_p"], gp[0])
    elif mode == 1:
        for use_pd in (False, True):
            ref = O.p2g(p64, dom, res, radius, 1000.0, nsize, pc=a64, pd=d64 if use_pd else None, is_2d=nd == 2, clip=clip)
            out = S.p2g(p, attr, pd if use_pd else None)
            assert _close(out["grid"], ref[0])
            grads = torch.autograd.grad(ref, (p64, a64) + ((d64,) if use_pd else ()), g[None])
            b = S.p2g_bwd(p, g, attr, pd if use_pd else None)
            assert _close(b["g_p"], grads[0][0]) and _close(b["g_attr"], grads[1][0])
            if use_pd:
                assert _close(b["g_pd"], grads[2][0, :, 0])
    else:
        ref = O.p2g_wavg(p64, a64, dom, res, radius, nsize, is_2d=nd == 2, clip=clip)
        out = S.p2g(p, attr)
        fin, _, _ = SR.wavg_finish(out["grid"], out["wsum"])
        assert _close(fin, ref[0])
        gp, ga = torch.autograd.grad(ref, (p64, a64), g[None])
        g_xs, _, g_ws, _ = SR.wavg_finish_bwd(out["grid"], out["wsum"], g)
        b = S.p2g_bwd(p, g_xs, attr, g_wsum=g_ws)
        assert _close(b["g_p"], gp[0], 1e-11) and _close(b["g_attr"], ga[0], 1e-11)
    assert bool((out["bound"] >= 0).all())


@pytest.mark.parametrize("nd", [2, 3])
def test_float32_decisions_match_float64_away_from_ties(nd):
    """with no particle near a tie and none clamped, the float32 discrete part gives the oracle's float64 result"""
    rng = np.random.RandomState(7 + nd)
    res, dom, radius = GEOM[nd]
    p = _particles(rng, 200, nd)
    S = SR.Splat(nd, res, dom, radius, 4.0, 1000.0, 1, False, 0)
    p = p[~S.near_tie(p)]
    ref = O.p2g(p.double()[None], dom, res, radius, 1000.0, 1, is_2d=nd == 2, clip=False)
    assert _close(S.p2g(p)["grid"], ref[0])


def test_restatement_matches_numpy_loops():
    rng = np.random.RandomState(3)
    res, dom, radius = GEOM[3]
    p = _particles(rng, 40, 3)
    S = SR.Splat(3, res, dom, radius, 4.0, 1000.0, 1, False, 0)
    p = p[~S.near_tie(p)]
    ref = O.p2g_numpy_loops(p.double().numpy(), dom, res, radius, 1000.0, 1, is_2d=False)
    assert _close(S.p2g(p)["grid"], torch.tensor(ref.copy())[0], 1e-12)
    res2, dom2, radius2 = GEOM[2]
    p2 = _particles(rng, 40, 2)
    S2 = SR.Splat(2, res2, dom2, radius2, 4.0, 1000.0, 3, False, 0)
    ref2 = O.p2g_numpy_loops(p2.double().numpy(), dom2, res2, radius2, 1000.0, 3, is_2d=True)
    assert _close(S2.p2g(p2)["grid"], torch.tensor(ref2.copy())[0], 1e-12)


@pytest.mark.parametrize("g2p_case", list(itertools.product([2, 3], [False, True])))
def test_g2p_matches_oracle(g2p_case):
    nd, cubic = g2p_case
    rng = np.random.RandomState(5)
    for dims in ([4, 6, 5][:nd], [1, 2, 3][:nd], [3, 1, 2][:nd]):
        g = torch.tensor(rng.randn(*dims, 3).astype(np.float32))
        p = _particles(rng, 80, nd, -0.3, 1.3)
        out, bound = SR.g2p(g, p, cubic, discrete=torch.float64)
        ref = O.g2p(g.double()[None], p.double()[None], is_2d=nd == 2, is_linear=not cubic)
        assert _close(out, ref[0])
        assert bool((bound > 0).all())


# ---- hand-made particles: arithmetic exact in float32 ---------------------------------------------------------------------

def test_hand_made_particles_dom_12():
    """dom = 12 (hi = 12 - 1e-6 rounds to the float32 below 12), res = 12, cell = 1, 2-D"""
    S = SR.Splat(2, [12, 12], [12.0, 12.0], 0.5, 4.0, 1000.0, 1, True, 0)
    hi = float(f32(12.0) - f32(1e-6))
    assert hi < 12.0
    p = torch.tensor([[0.25, 0.5],          # v = (3, 6): on cell faces -> the upper cells (3, 6), r = -0.5
                      [0.125 + 1 / 24, 0.375],  # not exact: replaced below
                      [0.0, 0.0],           # exactly 0: cell 0, gradient passes (tie included)
                      [1.0, 1.5],           # v = 12, 18: clamped to hi, cell 11, no gradient
                      [-0.25, hi / 12.0]],  # below 0: clamped, no gradient; axis 1 AT hi if the product is exact
                     dtype=torch.float32)
    p[1] = torch.tensor([3.5 / 12.0, 4.5 / 12.0])      # cell centres up to the rounding of 3.5 / 12
    L = S.locate(p)
    assert L["idx"][0].tolist() == [3, 6] and L["r"][0].tolist() == [-0.5, -0.5]
    assert L["idx"][2].tolist() == [0, 0] and L["grad_ok"][2].tolist() == [True, True]
    assert L["idx"][3].tolist() == [11, 11] and L["grad_ok"][3].tolist() == [False, False]
    assert L["idx"][4].tolist()[0] == 0 and L["grad_ok"][4].tolist()[0] is False
    assert L["idx"][1].tolist() == [3, 4]
    # an exact centre: v = 4.5 from p = 0.375 exactly
    assert float(L["r"][1, 1]) == 0.0
    # zero position gradient at a centre: one particle at the centre of cell (4, 4), uniform grid gradient
    pc = torch.tensor([[0.375, 0.375]], dtype=torch.float32)
    g = torch.tensor(np.random.RandomState(0).randn(12, 12, 1))
    b = S.p2g_bwd(pc, g)
    Lc = S.locate(pc)
    assert Lc["r"].abs().max() == 0
    # the centre cell's own term vanishes (dist = 0); the neighbours' terms remain and are finite
    assert torch.isfinite(b["g_p"]).all()
    ones = S.p2g_bwd(pc, torch.ones(12, 12, 1, dtype=torch.float64))
    assert float(ones["g_p"].abs().max()) <= 1e-9      # symmetric neighbourhood around a centre: gradients cancel


def test_clip_gradient_ties_pass_where_the_oracle_halves_them():
    """TF's clip_by_value passes the gradient where 0 <= v <= hi, ties included; torch.minimum in the oracle splits
    a tie in half.  p = hi / dom exactly (dom = 8: the product is exact) sits ON the upper clamp."""
    dom = [8.0, 8.0]
    S = SR.Splat(2, [8, 8], dom, 0.5, 4.0, 1000.0, 1, True, 0, discrete=torch.float64)
    hi64 = 8.0 - 1e-6
    p = torch.tensor([[hi64 / 8.0, 0.3]], dtype=torch.float64)
    assert float(p[0, 0] * 8.0) == hi64
    g = torch.tensor(np.random.RandomState(1).randn(8, 8, 1))
    b = S.p2g_bwd(p, g)
    p64 = p[None].clone().requires_grad_()
    (go,) = torch.autograd.grad(O.p2g(p64, dom, [8, 8], 0.5, 1000.0, 1, is_2d=True, clip=True), p64, g[None])
    assert S.locate(p)["grad_ok"].tolist() == [[True, True]]
    assert abs(float(go[0, 0, 0]) - 0.5 * float(b["g_p"][0, 0])) <= 1e-12 * abs(float(b["g_p"][0, 0]))
    assert abs(float(go[0, 0, 1]) - float(b["g_p"][0, 1])) <= 1e-12 * abs(float(b["g_p"][0, 1]))
    # the float32 kernel's tie: dom = 8, hi32 = 8 - 2^-20 rounded; p = hi32 / 8 is exact
    S32 = SR.Splat(2, [8, 8], dom, 0.5, 4.0, 1000.0, 1, True, 0)
    hi32 = f32(8.0) - f32(1e-6)
    p32 = torch.tensor([[float(hi32) / 8.0, 0.3]], dtype=torch.float32)
    L = S32.locate(p32)
    assert float(L["v"][0, 0]) == float(hi32) and L["grad_ok"].tolist() == [[True, True]] and L["idx"][0, 0] == 7


def test_hand_made_particles_dom_200():
    """dom = 200: in float32 200 - 1e-6 == 200, so a clamped particle's own cell is index res, OUTSIDE the grid; only
    the lower neighbours (offset -1 along that axis) receive anything.  The reference's float32 graph does the same."""
    assert float(f32(200.0) - f32(1e-6)) == 200.0
    S = SR.Splat(3, [200, 300, 200], [200.0, 300.0, 200.0], 0.5, 4.0, 1000.0, 1, True, 0)
    p = torch.tensor([[1.0, 0.5, 0.5], [1.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.0, 1.0, 0.25]], dtype=torch.float32)
    L = S.locate(p)
    assert L["idx"][0].tolist() == [200, 150, 100] and L["grad_ok"][0].tolist() == [True, True, True]   # v == hi: tie passes
    assert L["idx"][1].tolist() == [200, 150, 100] and L["grad_ok"][1].tolist() == [False, True, True]
    assert L["idx"][2].tolist() == [100, 150, 100]
    assert L["idx"][3].tolist() == [0, 300, 50] and L["grad_ok"][3].tolist() == [True, True, True]
    assert L["r"][0].tolist() == [-0.5, -0.5, -0.5]
    out = S.p2g(p[:1])["grid"]
    nz = out[..., 0].nonzero()
    assert set(nz[:, 0].tolist()) == {199}                      # only the plane below the own cell
    # the float64 decision puts the same particle IN cell 199: the two differ, and the product keeps the float32 one
    S64 = SR.Splat(3, [200, 300, 200], [200.0, 300.0, 200.0], 0.5, 4.0, 1000.0, 1, True, 0, discrete=torch.float64)
    assert S64.locate(p[:1])["idx"][0].tolist() == [199, 150, 100]
    # without clip the particle at v == dom is invalid and splats nothing
    S0 = SR.Splat(3, [200, 300, 200], [200.0, 300.0, 200.0], 0.5, 4.0, 1000.0, 1, False, 0)
    assert S0.locate(p)["valid"].tolist() == [False, False, True, False]
    assert float(S0.p2g(p[:2])["grid"].abs().sum()) == 0.0


def test_h_flip_axis():
    """one particle: the flipped axis is 0 in 2-D and 1 in 3-D"""
    S = SR.Splat(2, [4, 6], [4.0, 6.0], 0.25, 4.0, 1000.0, 0, False, 0)
    out = S.p2g(torch.tensor([[0.125 + 1 / 64, 0.25 + 1 / 64]]))["grid"][..., 0]
    assert out.nonzero().tolist() == [[3, 1]]
    S = SR.Splat(3, [4, 6, 5], [4.0, 6.0, 5.0], 0.25, 4.0, 1000.0, 0, False, 0)
    out = S.p2g(torch.tensor([[0.125 + 1 / 64, 0.25 + 1 / 64, 0.5]]))["grid"][..., 0]
    assert out.nonzero().tolist() == [[0, 4, 2]]


# ---- bounds ----------------------------------------------------------------------------------------------------------------

def _case(mode, nd=3, N=300, seed=11, clip=True):
    rng = np.random.RandomState(seed)
    res, dom, radius = GEOM[nd]
    S = SR.Splat(nd, res, dom, radius, 4.0, 1000.0, 1, clip, mode)
    p = _particles(rng, N, nd)
    p = p[~S.near_tie(p)]
    N = p.shape[0]
    attr = None if mode == 0 else torch.tensor(rng.uniform(-1, 1, (N, 2)).astype(np.float32))
    pd = torch.tensor(rng.uniform(800, 1200, (N,)).astype(np.float32)) if mode == 1 else None
    return S, p, attr, pd, rng


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bounds_are_positive_and_grow_with_input_error(mode):
    S, p, attr, pd, rng = _case(mode)
    o0 = S.p2g(p, attr, pd)
    touched = o0["terms"]["acc"] > 0
    assert bool((o0["bound"][touched[..., :o0["bound"].shape[-1]]] > 0).all())
    if mode == 0:
        assert bool(((o0["grid"] == 0) | (o0["bound"] > 0)).all())
    o1 = S.p2g(p, attr, pd, v_err=1e-4)
    assert torch.equal(o0["terms"]["quant"], o1["terms"]["quant"])     # the budget goes to the position term
    assert bool((o1["terms"]["r"] >= o0["terms"]["r"]).all()) and float(o1["bound"].sum()) > float(o0["bound"].sum())
    # roundings alone are small: the bound stays below 1e-4 of the largest cell
    assert float(o0["bound"].max()) < 1e-4 * float(o0["grid"].abs().max())
    C = 1 if mode == 0 else 2
    g = torch.tensor(rng.randn(*S.res, C))
    gw = torch.tensor(rng.randn(*S.res, 1)) if mode == 2 else None
    b0 = S.p2g_bwd(p, g, attr, pd, gw)
    ge = torch.full_like(g, 1e-5)
    b1 = S.p2g_bwd(p, g, attr, pd, gw, g_err=ge)
    assert float(b0["g_p_terms"]["input"].abs().max()) == 0.0
    moved = b0["g_p"].abs() > 0
    assert bool((b0["g_p_bound"][moved] > 0).all()) and bool((b0["g_p_bound"][~moved & ~(b0["g_p_bound"] > 0)] == 0).all())
    assert bool((b1["g_p_bound"] >= b0["g_p_bound"]).all()) and float(b1["g_p_bound"].sum()) > float(b0["g_p_bound"].sum())
    if mode != 0:
        assert bool((b1["g_attr_bound"] >= b0["g_attr_bound"]).all())
        assert float(b1["g_attr_bound"].sum()) > float(b0["g_attr_bound"].sum())
    if mode == 1:
        assert float(b1["g_pd_bound"].sum()) > float(b0["g_pd_bound"].sum())


def test_finish_bounds_and_the_eps_switch():
    rng = np.random.RandomState(2)
    xs = torch.tensor(rng.randn(5, 6, 2).astype(np.float32))
    ws = torch.tensor(rng.uniform(0, 2, (5, 6, 1)).astype(np.float32))
    ws[0, 0, 0] = 1e-6 * 0.5
    ws[0, 1, 0] = float(f32(1e-6))         # w == eps: NOT above it
    ws[0, 2, 0] = float(np.nextafter(f32(1e-6), f32(1)))
    out, b0, dec = SR.wavg_finish(xs, ws)
    assert torch.equal(out[0, 0], xs[0, 0].double()) and torch.equal(out[0, 1], xs[0, 1].double())
    assert _close(out[0, 2], xs[0, 2].double() / ws[0, 2].double())
    assert bool(dec[0, 0]) and not bool(dec[0, 1, 0])
    _, b1, dec1 = SR.wavg_finish(xs, ws, x_err=torch.full_like(xs, 1e-6), w_err=torch.full_like(ws, 1e-6))
    assert bool((b1 > b0).all()) and bool((b0 >= 0).all())
    assert not bool(dec1[0, 0, 0]) and not bool(dec1[0, 2, 0]) and bool(dec1[1:].all())
    g = torch.tensor(rng.randn(5, 6, 2))
    gx, gxb, gw, gwb = SR.wavg_finish_bwd(xs, ws, g)
    x64, w64 = xs.double().requires_grad_(), ws.double().requires_grad_()
    safe = torch.where(w64 > float(f32(1e-6)), w64, torch.ones_like(w64))
    o = torch.where(w64 > float(f32(1e-6)), x64 / safe, x64)
    ax, aw = torch.autograd.grad(o, (x64, w64), g)
    assert _close(gx, ax) and _close(gw, aw)
    assert float(gw[0, 0, 0]) == 0.0 and float(gwb[0, 0, 0]) == 0.0


def test_box_volumes():
    """the restatement's box computation: 256 particles in one 3-D cell -> (1 + 2 nsize)^3 clipped to the grid"""
    S = SR.Splat(3, [20, 20, 20], [20.0, 20.0, 20.0], 0.5, 4.0, 1000.0, 1, False, 0)
    p = torch.full((300, 3), 0.5125, dtype=torch.float32)
    p[256:] = torch.tensor([0.0125, 0.5125, 0.9875])           # second block: at two grid borders
    p[299] = torch.tensor([2.0, 0.5, 0.5])                      # invalid: ignored
    assert S.block_boxes(p).tolist() == [27, 2 * 3 * 2]
    p[:256, 0] = -1.0
    assert S.block_boxes(p).tolist() == [0, 12]


# ---- float32 replay of the kernel's own order of operations ------------------------------------------------------------------

def _replay(S, p, attr, pd, g, gw):
    """p2g_fwd_kernel / p2g_bwd_kernel statement by statement in NumPy float32, particles in order, cells in the order
    of the generic loop"""
    nd, ns = S.nd, S.nsize
    dom = np.asarray(S.domain, f32)
    cell = f32(dom[0] / f32(S.res[0]))
    h, sigma, mass, rho = f32(S.h), f32(S.sigma), f32(S.mass), f32(S.rest_density)
    C = 1 if attr is None else attr.shape[1]
    grid = np.zeros((S.cells, C), f32)
    wsum = np.zeros(S.cells, f32)
    N = p.shape[0]
    g_p, g_a, g_d = np.zeros((N, nd), f32), np.zeros((N, C), f32), np.zeros(N, f32)

    def cw(q):
        if q > 1: return f32(0)
        if q <= f32(0.5): return f32(sigma * f32(f32(6) * f32(f32(q * q * q) - f32(q * q)) + f32(1)))
        t = f32(f32(1) - q)
        return f32(f32(sigma * f32(2)) * f32(f32(t * t) * t))

    def cdw(q):
        if q > 1: return f32(0)
        if q <= f32(0.5): return f32(f32(sigma * f32(6)) * f32(f32(f32(3) * f32(q * q)) - f32(f32(2) * q)))
        t = f32(f32(1) - q)
        return f32(f32(-sigma * f32(6)) * f32(t * t))

    for a in range(N):
        valid, idx, r, ok = True, [], [], []
        for k in range(nd):
            v = f32(p[a, k] * dom[k])
            if S.clip:
                hi = f32(dom[k] - f32(1e-6))
                ok.append(bool(v >= 0 and v <= hi))
                v = min(max(v, f32(0)), hi)
            else:
                ok.append(True)
                valid = valid and bool(v >= 0 and v < dom[k])
            fl = np.floor(f32(v / cell))
            idx.append(int(fl)); r.append(f32(v - f32(f32(fl + f32(0.5)) * cell)))
        if not valid:
            continue
        pdv = f32(pd[a]) if pd is not None else rho
        coef = f32(1) if S.mode == 2 else (mass if S.mode == 0 else f32(mass / pdv))
        gp, ga, gd = np.zeros(nd, f32), np.zeros(C, f32), f32(0)
        for n in itertools.product(range(-ns, ns + 1), repeat=nd):
            rr = [f32(r[k] - f32(f32(n[k]) * cell)) for k in range(nd)]
            d2 = f32(0)
            for k in range(nd):
                d2 = f32(d2 + f32(rr[k] * rr[k]))
            dist = f32(np.sqrt(d2))
            q = f32(dist / h)
            c = [idx[k] + n[k] for k in range(nd)]
            if any(c[k] < 0 or c[k] >= S.res[k] for k in range(nd)) or q > 1:
                continue
            lin = 0
            for k in range(nd):
                lin = lin * S.res[k] + (S.res[k] - 1 - c[k] if k == S.hax else c[k])
            w = cw(q)
            if S.mode == 0:
                grid[lin, 0] = f32(grid[lin, 0] + f32(coef * w))
                gwv = f32(coef * g[lin, 0])
            else:
                dot = f32(0)
                for ch in range(C):
                    grid[lin, ch] = f32(grid[lin, ch] + f32(f32(coef * w) * attr[a, ch]))
                    dot = f32(dot + f32(attr[a, ch] * g[lin, ch]))
                    ga[ch] = f32(ga[ch] + f32(f32(coef * w) * g[lin, ch]))
                gwv = f32(coef * dot)
                if S.mode == 1: gd = f32(gd - f32(f32(f32(coef * w) * dot) / pdv))
                if S.mode == 2:
                    wsum[lin] = f32(wsum[lin] + w)
                    gwv = f32(gwv + gw[lin])
            if dist > 0:
                f = f32(f32(gwv * cdw(q)) / f32(dist * h))
                for k in range(nd):
                    gp[k] = f32(gp[k] + f32(f * rr[k]))
        for k in range(nd):
            g_p[a, k] = f32(gp[k] * dom[k]) if ok[k] else f32(0)
        g_a[a], g_d[a] = ga, gd
    return grid, wsum, g_p, g_a, g_d


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("nd,nsize", [(3, 1), (2, 2), (2, 0)])
@pytest.mark.parametrize("clip", [False, True])
def test_float32_replay_stays_inside_the_bounds(mode, nd, nsize, clip):
    rng = np.random.RandomState(40 + mode + 3 * nd + nsize)
    if nd == 3:
        res, dom, radius = [5, 7, 6], [200.0, 280.0, 240.0], 20.0        # a large domain: the position term at work
    else:
        res, dom, radius = GEOM[2]
    S = SR.Splat(nd, res, dom, radius, 4.0, 1000.0, nsize, clip, mode)
    p = _particles(rng, 90, nd)
    p = p[~S.near_tie(p)]
    N = p.shape[0]
    attr = None if mode == 0 else torch.tensor(rng.uniform(-1, 1, (N, 2)).astype(np.float32))
    pd = torch.tensor(rng.uniform(800, 1200, (N,)).astype(np.float32)) if mode == 1 else None
    C = 1 if mode == 0 else 2
    g = torch.tensor(rng.randn(*res, C).astype(np.float32))
    gw = torch.tensor(rng.randn(*res, 1).astype(np.float32)) if mode == 2 else None
    grid, wsum, g_p, g_a, g_d = _replay(S, p.numpy(), None if attr is None else attr.numpy(),
                                        None if pd is None else pd.numpy(), g.numpy().reshape(-1, C),
                                        None if gw is None else gw.numpy().reshape(-1))
    o = S.p2g(p, attr, pd)
    r = [SR.err_ratio((torch.tensor(grid).reshape(o["grid"].shape).double() - o["grid"]).abs(), o["bound"])]
    if mode == 2:
        r.append(SR.err_ratio((torch.tensor(wsum).reshape(o["wsum"].shape).double() - o["wsum"]).abs(), o["wsum_bound"]))
    b = S.p2g_bwd(p, g, attr, pd, gw)
    r.append(SR.err_ratio((torch.tensor(g_p).double() - b["g_p"]).abs(), b["g_p_bound"]))
    if mode != 0:
        r.append(SR.err_ratio((torch.tensor(g_a).double() - b["g_attr"]).abs(), b["g_attr_bound"]))
    if mode == 1:
        r.append(SR.err_ratio((torch.tensor(g_d).double() - b["g_pd"]).abs(), b["g_pd_bound"]))
    assert max(r) <= 1.0, r
    assert max(r) > 1e-3, r            # and the bounds are not vacuous: the replay uses a visible part of them

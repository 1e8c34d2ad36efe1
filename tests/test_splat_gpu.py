"""The SPH splat cell by cell: every kernel of csrc/splat.hip, every compiled (nd, nsize) instance and the generic
forms, against the float64 restatement of tests/splat_ref.py, each cell / particle component within its own error
bound.  Every test prints, per kind of check, the largest err / bound it saw, the case it came from and the bound
term that carried it (pytest -s)."""
import itertools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import splat_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda"

# The (nd, nsize) pairs with a compile-time instance, written down here by hand and NOT read from the library:
# csrc/splat.hip keeps its own one list (with_instance), and test_instance_list_is_the_librarys holds the two equal,
# so an instance added there without an entry here fails that test instead of going untested.
INSTANCES = [(3, 1), (3, 2), (2, 1), (2, 2), (2, 3), (2, 4)]
# what falls through to the generic loops: any other nsize, 0 included
GENERIC = [(3, 3), (2, 5), (3, 0), (2, 0)]

# non-cubic grids, three different extents, cell = 0.5 in 3-D and 0.05 in 2-D (the dambreak driver's)
GEOM = {3: dict(res=[24, 40, 32], domain=[12.0, 20.0, 16.0], radius=0.25),
        2: dict(res=[48, 80], domain=[2.4, 4.0], radius=0.025)}
# (mode, C, per-particle density): density; colour with C = 1, 3, 4 with and without pd; raw sums with C = 1, 2, 3
MODES = [(0, 1, False)] + [(1, c, d) for c in (1, 3, 4) for d in (False, True)] + [(2, c, False) for c in (1, 2, 3)]


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


class Report:
    """largest err / bound per kind of check of one test, printed once"""

    def __init__(self, name):
        self.name, self.worst = name, {}

    def check(self, kind, case, got, ref, bound, terms=None):
        err = (got.double() - ref.double()).abs()
        r = SR.err_ratio(err, bound)
        term = SR.dominant(terms, err, bound) if terms else "-"
        if r >= self.worst.get(kind, (-1.0,))[0]:
            self.worst[kind] = (r, case, term)
        assert r <= 1.0, (self.name, kind, case, r, term)
        return r

    def done(self):
        for kind, (r, case, term) in self.worst.items():
            print("%-34s %-18s max err/bound %-9.3g term %-6s %s" % (self.name, kind, r, term, case))


def splat(nd, nsize, clip, mode, **over):
    g = dict(GEOM[nd]); g.update(over)
    return SR.Splat(nd, g["res"], g["domain"], g["radius"], 4.0, 1000.0, nsize, clip, mode)


def drop_ties(S, p, limit=0.01):
    """leave out particles whose cell is a rounding decision; at most 1 % of a case"""
    tie = S.near_tie(p)
    assert float(tie.double().mean()) <= limit, float(tie.double().mean())
    return p[~tie].contiguous()


def uniform_set(rng, N, nd):
    """about 5 % outside [0, 1) on each side of every axis"""
    return torch.tensor(rng.uniform(-0.055, 1.055, (N, nd)).astype(np.float32), device=DEV)


def tie_free(S, rng, N, lo=-0.055, hi=1.055):
    """N particles, uniform in [lo, hi), none of them a rounding decision (for the sets whose COUNT is the point: a tie
    is drawn again instead of dropped)"""
    p = torch.tensor(rng.uniform(lo, hi, (N, S.nd)).astype(np.float32), device=DEV)
    for _ in range(50):
        tie = S.near_tie(p)
        if not bool(tie.any()):
            return p
        p[tie] = torch.tensor(rng.uniform(lo, hi, (int(tie.sum()), S.nd)).astype(np.float32), device=DEV)
    raise AssertionError("no tie-free set")


def border_set(rng, N, nd, S):
    """every particle within half a support of a grid border along at least one axis; the 2^nd corners included"""
    dom = np.asarray(S.domain)
    half = 0.5 * S.h / dom
    p = rng.uniform(0, 1, (N, nd))
    for a in range(N):
        axes = [k for k in range(nd) if rng.rand() < 0.5] or [rng.randint(nd)]
        for k in axes:
            u = rng.uniform(0, half[k])
            p[a, k] = u if rng.rand() < 0.5 else 1.0 - u
    for j, corner in enumerate(itertools.product([0, 1], repeat=nd)):
        u = rng.uniform(0, half)
        p[j] = np.where(np.asarray(corner) == 0, u, 1.0 - u)
    return torch.tensor(p.astype(np.float32), device=DEV)


def dense_set(rng, S):
    """4-8 particles in every cell, liquid-like: many lanes add to one LDS address"""
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in S.res], indexing="ij"), -1).reshape(-1, S.nd)
    k = rng.randint(4, 9, len(cells))
    c = np.repeat(cells, k, 0)
    p = (c + rng.uniform(0.02, 0.98, c.shape)) / np.asarray(S.res)
    return torch.tensor(p.astype(np.float32), device=DEV)


def orders(p, S, rng):
    """(tag, permutation): brick order (transform.grid_order, as Styler.run sorts) and shuffled"""
    import neural_flow_style_amd.transform as T
    yield "brick", T.grid_order(p.clamp(0, 1), S.res)
    yield "shuffled", torch.tensor(rng.permutation(p.shape[0]), device=DEV)


def attrs(rng, N, C, mode, use_pd):
    a = None if mode == 0 else torch.tensor(rng.uniform(-1, 1, (N, C)).astype(np.float32), device=DEV)
    pd = torch.tensor(rng.uniform(800, 1200, (N,)).astype(np.float32), device=DEV) if use_pd else None
    return a, pd


def grads(rng, S, C):
    g = torch.tensor(rng.randn(*S.res, C).astype(np.float32), device=DEV)
    gw = torch.tensor(rng.randn(*S.res, 1).astype(np.float32), device=DEV) if S.mode == 2 else None
    return g, gw


def run_case(ops, rep, S, p, a, pd, g, gw, case, combos=True, lds_instance=True):
    """forward, adjoint (every combination of outputs the mode allows), and in mode 2 the finish, its adjoint and the
    one-launch adjoint, all against the restatement"""
    cfg = S.ops_cfg(ops)
    C = 1 if a is None else a.shape[1]
    ref = S.p2g(p, a, pd)
    if S.mode == 2:
        xs, ws = ops.p2g_fwd(p, cfg, attr=a)
        rep.check("fwd xsum", case, xs, ref["grid"], ref["bound"], {k: t[..., :C] for k, t in ref["terms"].items()})
        rep.check("fwd wsum", case, ws, ref["wsum"], ref["wsum_bound"], {k: t[..., C:] for k, t in ref["terms"].items()})
    else:
        out = ops.p2g_fwd(p, cfg, attr=a, pd=pd)
        rep.check("fwd", case, out, ref["grid"], ref["bound"], ref["terms"])
    b = S.p2g_bwd(p, g, a, pd, gw)
    names = ["p"] + (["attr"] if S.mode != 0 else []) + (["pd"] if S.mode == 1 else [])
    sets = [c for n in range(1, len(names) + 1) for c in itertools.combinations(names, n)] if combos else [tuple(names)]
    for need in sets:
        gp, ga, gd = ops.p2g_bwd(p, cfg, g, attr=a, pd=pd, g_wsum=gw, need_p="p" in need, need_attr="attr" in need,
                                 need_pd="pd" in need)
        assert (gp is None) == ("p" not in need) and (ga is None) == ("attr" not in need) and (gd is None) == ("pd" not in need)
        if gp is not None:
            rep.check("bwd g_p", case, gp, b["g_p"], b["g_p_bound"], b["g_p_terms"])
        if ga is not None:
            rep.check("bwd g_attr", case, ga, b["g_attr"], b["g_attr_bound"])
        if gd is not None:
            rep.check("bwd g_pd", case, gd, b["g_pd"], b["g_pd_bound"])
    if S.mode != 2:
        return
    # the finish on the kernel's own sums (the switch w > eps is then exact), and on the restatement's sums with the
    # forward bounds as budgets, cells whose switch is undecided left out (at most 1 %)
    fin = ops.p2g_wavg_finish(xs, ws)
    f0, fb0, _ = SR.wavg_finish(xs, ws)
    rep.check("finish", case, fin, f0, fb0)
    f1, fb1, dec = SR.wavg_finish(ref["grid"], ref["wsum"], x_err=ref["bound"], w_err=ref["wsum_bound"])
    assert float((~dec).double().mean()) <= 0.01
    keep = dec.expand_as(f1)
    rep.check("finish (ref sums)", case, fin[keep], f1[keep], fb1[keep])
    gx, gxw = ops.p2g_wavg_finish_bwd(xs, ws, g)
    rx, rxb, rw, rwb = SR.wavg_finish_bwd(xs, ws, g)
    rep.check("finish_bwd g_xsum", case, gx, rx, rxb)
    rep.check("finish_bwd g_wsum", case, gxw, rw, rwb)
    gp2, ga2, _ = ops.p2g_bwd(p, cfg, gx, attr=a, g_wsum=gxw, need_p=True, need_attr=True)
    b2 = S.p2g_bwd(p, gx, a, None, gxw)
    rep.check("wavg bwd g_p", case, gp2, b2["g_p"], b2["g_p_bound"], b2["g_p_terms"])
    rep.check("wavg bwd g_attr", case, ga2, b2["g_attr"], b2["g_attr_bound"])
    # the same from the float64 finish adjoint, its bounds as input budgets: the whole adjoint chain in float64
    b3 = S.p2g_bwd(p, rx, a, None, rw, g_err=rxb, gw_err=rwb)
    rep.check("wavg bwd g_p (f64 chain)", case, gp2, b3["g_p"], b3["g_p_bound"], b3["g_p_terms"])
    one = ops.p2g_wavg_bwd(p, cfg, xs, ws, g, a)
    if lds_instance:
        assert one is not None and torch.equal(one[0], gp2) and torch.equal(one[1], ga2), case
        only_p = ops.p2g_wavg_bwd(p, cfg, xs, ws, g, a, need_attr=False)
        assert only_p[1] is None and torch.equal(only_p[0], gp2)
    else:
        assert one is None, case


# ---- the instance matrix ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("nd,nsize", INSTANCES + GENERIC)
def test_instance_matrix(ops, nd, nsize, clip):
    rep = Report("matrix (%d,%d) clip=%d" % (nd, nsize, clip))
    rng = np.random.RandomState(1000 + 100 * nd + 10 * nsize + clip)
    N = 2500 if (nd, nsize) != (3, 3) else 1200
    for mode, C, use_pd in MODES:
        S = splat(nd, nsize, clip, mode)
        p0 = drop_ties(S, uniform_set(rng, N, nd))
        a0, pd0 = attrs(rng, p0.shape[0], C, mode, use_pd)
        g, gw = grads(rng, S, C)
        for tag, perm in orders(p0, S, rng):
            p = p0[perm].contiguous()
            a = None if a0 is None else a0[perm].contiguous()
            pd = None if pd0 is None else pd0[perm].contiguous()
            run_case(ops, rep, S, p, a, pd, g, gw, "mode %d C %d pd %d %s" % (mode, C, use_pd, tag),
                     combos=(tag == "brick"), lds_instance=(nd, nsize) in INSTANCES)
    rep.done()


def test_instance_list_is_the_librarys(ops):
    """nfs_p2g_has_instance, the predicate the dispatchers of splat.hip use, against the hand-written list.  The
    query also answers 0 for every pair when the process runs under NFS_SPLAT_LDS=0: a failure of this test in such a
    process says nothing about the list."""
    for nd in (2, 3):
        for nsize in range(9):
            assert ops.p2g_has_instance(splat(nd, nsize, False, 2).ops_cfg(ops)) == ((nd, nsize) in INSTANCES), (nd, nsize)
    for nd, nsize in GENERIC:
        assert not ops.p2g_has_instance(splat(nd, nsize, False, 2).ops_cfg(ops))


# ---- particle sets ---------------------------------------------------------------------------------------------------------

SET_MODES = [(0, 1, False), (1, 3, True), (2, 2, False)]
SET_INSTANCES = INSTANCES + [(3, 3), (2, 5)]


def _both_orders(ops, rep, S, p0, rng, C, use_pd, case, lds_instance):
    a0, pd0 = attrs(rng, p0.shape[0], C, S.mode, use_pd)
    g, gw = grads(rng, S, C)
    for tag, perm in orders(p0, S, rng):
        run_case(ops, rep, S, p0[perm].contiguous(), None if a0 is None else a0[perm].contiguous(),
                 None if pd0 is None else pd0[perm].contiguous(), g, gw, "%s %s" % (case, tag), combos=False,
                 lds_instance=lds_instance)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("nd,nsize", SET_INSTANCES)
def test_border_particles(ops, nd, nsize, clip):
    rep = Report("border (%d,%d) clip=%d" % (nd, nsize, clip))
    rng = np.random.RandomState(2000 + 100 * nd + 10 * nsize + clip)
    for mode, C, use_pd in SET_MODES:
        S = splat(nd, nsize, clip, mode)
        p0 = drop_ties(S, border_set(rng, 1500 if (nd, nsize) != (3, 3) else 700, nd, S))
        _both_orders(ops, rep, S, p0, rng, C, use_pd, "mode %d" % mode, (nd, nsize) in INSTANCES)
    rep.done()


@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("nd,nsize", INSTANCES + [(3, 3), (2, 0)])
def test_partial_last_block(ops, nd, nsize, N):
    """N % 256 in {1, 255}, and a single particle: the lanes beyond N take part in the block's reductions"""
    rep = Report("N=%d (%d,%d)" % (N, nd, nsize))
    rng = np.random.RandomState(3000 + 100 * nd + 10 * nsize + N)
    for clip in (False, True):
        for mode, C, use_pd in SET_MODES:
            S = splat(nd, nsize, clip, mode)
            p0 = tie_free(S, rng, N) if N > 1 else tie_free(S, rng, 1, 0.1, 0.9)
            _both_orders(ops, rep, S, p0, rng, C, use_pd, "mode %d clip %d" % (mode, clip), (nd, nsize) in INSTANCES)
    rep.done()


BIG = {3: dict(res=[50, 75, 40], domain=[200.0, 300.0, 160.0], radius=2.0),
       2: dict(res=[100, 150], domain=[200.0, 300.0], radius=1.0)}


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("nd,nsize", INSTANCES + [(3, 3), (2, 0)])
def test_block_outside_the_domain(ops, nd, nsize, big):
    """the first whole block of 256 lies beyond the upper border: without clip it has no valid particle (the forward
    returns, the adjoint writes zeros); with clip it is clamped -- for dom <= 32 into the last cell, for dom = 200, where
    float32 dom - 1e-6 is dom, onto index res: outside the grid, only the lower neighbours receive anything"""
    rep = Report("outside (%d,%d) %s" % (nd, nsize, "dom 200" if big else "dom<=32"))
    rng = np.random.RandomState(4000 + 100 * nd + 10 * nsize + big)
    geo = BIG[nd] if big else {}
    for clip in (False, True):
        for mode, C, use_pd in SET_MODES:
            S = splat(nd, nsize, clip, mode, **geo)
            assert (float(np.float32(S.domain[0]) - np.float32(1e-6)) == S.domain[0]) == big
            out = tie_free(S, rng, 256, 1.05, 1.3)
            out[:, 1:] = tie_free(S, rng, 256)[:, 1:]
            p = torch.cat([out, tie_free(S, rng, 300, 0.01, 0.99)]).contiguous()
            L = S.locate(p)
            if clip:
                assert bool((L["idx"][:256, 0] == (S.res[0] if big else S.res[0] - 1)).all())
            else:
                assert not bool(L["valid"][:256].any())
            a, pd = attrs(rng, p.shape[0], C, mode, use_pd)
            g, gw = grads(rng, S, C)
            run_case(ops, rep, S, p, a, pd, g, gw, "mode %d clip %d" % (mode, clip), combos=False,
                     lds_instance=(nd, nsize) in INSTANCES)
            if not clip:
                gp, _, _ = ops.p2g_bwd(p, S.ops_cfg(ops), g, attr=a, pd=pd, g_wsum=gw)
                assert float(gp[:256].abs().max()) == 0.0
    rep.done()


@pytest.mark.parametrize("nd,nsize", INSTANCES + [(3, 3), (2, 0)])
def test_hand_made_exact_particles(ops, nd, nsize):
    """particles whose arithmetic is exact in float32 are NOT filtered and must match: on cell faces, at cell centres,
    at 0, at hi and beyond it under clip -- with dom <= 16 (hi = dom - 1e-6 lies below dom) and dom = 200 (it is dom)"""
    rep = Report("exact (%d,%d)" % (nd, nsize))
    rng = np.random.RandomState(4500 + 10 * nd + nsize)
    small = {3: dict(res=[8, 16, 12], domain=[8.0, 16.0, 12.0], radius=0.5),
             2: dict(res=[16, 24], domain=[8.0, 12.0], radius=0.25)}[nd]        # cell 1 and 0.5: v / cell is exact
    for tag, geo in (("dom<=16", small), ("dom 200", BIG[nd])):
        for clip in (False, True):
            for mode, C, use_pd in SET_MODES:
                S = splat(nd, nsize, clip, mode, **geo)
                rows = [[0.25, 0.5, 0.75], [0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [1.5, 0.5, 0.5], [-0.25, 0.25, 0.5],
                        [0.5, 1.0, 1.0], [0.5, 0.5, 0.5], [0.375, 0.625, 0.125], [1.0, 1.0, 1.0]]
                hi = [float(np.float32(d) - np.float32(1e-6)) / d for d in S.domain]   # exactly on the clamp where p dom is exact
                rows.append([hi[0], 0.5, hi[-1]])
                centre = [(3 + 0.5) * S.cell / d for d in S.domain]                   # a cell centre (exact: powers of two)
                rows.append(centre + [0.0] * (3 - nd))
                p = torch.tensor(rows, dtype=torch.float32, device=DEV)[:, :nd].contiguous()
                p = torch.cat([p, tie_free(S, rng, 300, 0.02, 0.98)]).contiguous()
                a, pd = attrs(rng, p.shape[0], C, mode, use_pd)
                g, gw = grads(rng, S, C)
                run_case(ops, rep, S, p, a, pd, g, gw, "%s mode %d clip %d" % (tag, mode, clip), combos=False,
                         lds_instance=(nd, nsize) in INSTANCES)
    rep.done()


def _edge_extents(res, ns, per_cell, limit):
    """own-cell extents e (placed ns cells off the low border, so nothing clips) whose widened box holds at most
    ``limit`` values, and does not once ONE axis grows by one cell; the fullest such box"""
    best = None
    for e in itertools.product(*[range(1, n - 2 * ns) for n in res]):
        vol = int(np.prod([v + 2 * ns for v in e])) * per_cell
        if vol > limit:
            continue
        for k in range(len(res)):
            e2 = list(e); e2[k] += 1
            if e2[k] + 2 * ns <= res[k] and int(np.prod([v + 2 * ns for v in e2])) * per_cell > limit:
                if best is None or vol > best[0]:
                    best = (vol, e, tuple(e2))
    return best


def _box_block(rng, S, ext):
    """256 particles whose own cells span exactly ext (from cell nsize on every axis)"""
    nd = S.nd
    c = np.stack([rng.randint(0, ext[k], 256) for k in range(nd)], -1)
    c[0] = 0
    c[1] = np.asarray(ext) - 1
    return (S.nsize + c + rng.uniform(0.1, 0.9, c.shape)) / np.asarray(S.res)


FIT_GEOM = {3: {}, 2: dict(res=[96, 160], domain=[4.8, 8.0])}           # (a 2-D box needs > 12288 cells to overflow)


@pytest.mark.parametrize("mode,C", [(0, 1), (2, 2)])
@pytest.mark.parametrize("nd,nsize", INSTANCES)
def test_lds_box_fits_and_overflows_by_one_cell(ops, nd, nsize, mode, C):
    """blocks whose box just fits the LDS limit next to blocks one row of cells too large, for the forward's 8192
    accumulators and the adjoint's 12288 floats separately: some blocks of one launch stage, others fall back"""
    rep = Report("box edge (%d,%d) mode %d" % (nd, nsize, mode))
    rng = np.random.RandomState(5000 + 100 * nd + 10 * nsize + mode)
    S = splat(nd, nsize, False, mode, **FIT_GEOM[nd])
    nf, nb = S.channels(C)
    blocks, kinds = [], []
    for per_cell, limit in ((nf, SR.SPL_LDS), (nb, SR.SPB_LDS)):
        e = _edge_extents(S.res, nsize, per_cell, limit)
        assert e is not None, (S.res, nsize, per_cell, limit)
        blocks += [_box_block(rng, S, e[1]), _box_block(rng, S, e[2])]
        kinds += [(per_cell, limit, True), (per_cell, limit, False)]
    blocks.append(_box_block(rng, S, e[1])[:100])                       # and a short last block
    p = torch.tensor(np.concatenate(blocks).astype(np.float32), device=DEV)
    assert not bool(S.near_tie(p).any())
    vol = S.block_boxes(p).tolist()
    for b, (per_cell, limit, fits) in enumerate(kinds):                 # the set holds both kinds, for both limits
        assert (vol[b] * per_cell <= limit) == fits, (b, vol[b], per_cell, limit)
    assert any(v * nf <= SR.SPL_LDS for v in vol) and any(v * nf > SR.SPL_LDS for v in vol)
    assert any(v * nb <= SR.SPB_LDS for v in vol) and any(v * nb > SR.SPB_LDS for v in vol)
    a, pd = attrs(rng, p.shape[0], C, mode, False)
    g, gw = grads(rng, S, C)
    run_case(ops, rep, S, p, a, pd, g, gw, "boxes %s" % vol, combos=False)
    rep.done()


@pytest.mark.parametrize("nd,nsize", INSTANCES)
def test_dense_particles(ops, nd, nsize):
    rep = Report("dense (%d,%d)" % (nd, nsize))
    rng = np.random.RandomState(6000 + 100 * nd + 10 * nsize)
    for mode, C, use_pd in SET_MODES:
        S = splat(nd, nsize, True, mode)
        p0 = drop_ties(S, dense_set(rng, S))
        _both_orders(ops, rep, S, p0, rng, C, use_pd, "mode %d" % mode, True)
    rep.done()


@pytest.mark.parametrize("span", [6, 12])
@pytest.mark.parametrize("nd,nsize", INSTANCES)
def test_attribute_magnitudes_within_a_block(ops, nd, nsize, span):
    """attributes from 10^-span to 1 inside every block: the magnitude follows the position x in [0, 8) inside each
    8-cell brick along the last axis -- 1 in the first cell, a ramp over the second, 10^-span from there on (a block of
    256 particles in brick order covers whole rows of a brick).  The block's fixed-point scale is set by the largest;
    the cells in the middle of the plateau receive only small contributions (the support is two cells), and with
    span = 12 they are the ones whose bound the quantum carries: at 1e-6 the position term still leads"""
    rep = Report("attr 1e-%d..1 (%d,%d)" % (span, nd, nsize))
    rng = np.random.RandomState(7000 + 100 * nd + 10 * nsize + span)
    import neural_flow_style_amd.transform as T
    for mode, C in ((1, 3), (2, 2)):
        S = splat(nd, nsize, True, mode)
        p = drop_ties(S, dense_set(rng, S))
        p = p[T.grid_order(p.clamp(0, 1), S.res)].contiguous()
        x = torch.remainder(p[:, -1].double() * S.res[-1], 8.0)
        frac = (x - 1.0).clamp(0.0, 1.0)
        sign = torch.tensor(rng.choice([-1.0, 1.0], (p.shape[0], C)), device=DEV)
        a = (sign * (10.0 ** (-span * frac))[:, None] * torch.tensor(rng.uniform(0.5, 1.0, (p.shape[0], C)), device=DEV)).float()
        g, gw = grads(rng, S, C)
        run_case(ops, rep, S, p, a, None, g, gw, "mode %d" % mode, combos=False)
        ref = S.p2g(p, a)
        t = ref["terms"]
        lead = (t["quant"] > torch.maximum(torch.maximum(t["r"], t["eval"]), t["acc"]))[..., :C]
        print("%-34s mode %d: the quantum is the largest term of the bound in %.1f %% of the touched cells"
              % (rep.name, mode, 100.0 * float(lead.double().sum()) / max(1.0, float((ref["bound"] > 0).double().sum()))))
        if span == 12:
            assert bool(lead.any())
    rep.done()


# ---- the 64-bit index path --------------------------------------------------------------------------------------------------

class _Rows(SR.Splat):
    """the restatement on a window [a, b) of own-cell rows along axis 0 of a grid too large to hold in float64: cells
    outside the window are dropped; row j of the window is row j + res0 - b of the real (flipped) grid"""

    def __init__(self, full, a, b):
        self.__dict__.update(full.__dict__)
        self.full_res0, self.a, self.b = full.res[0], a, b
        self.res = [b - a] + full.res[1:]
        self.cells = int(np.prod(self.res))

    def lin(self, c):
        c = c.clone()
        c[:, 0] -= self.a
        return SR.Splat.lin(self, c)


def test_grid_of_2_to_the_31_cells(ops):
    """a 2-D grid of exactly 2^31 cells takes p2g_fwd_kernel and p2g_bwd_kernel with 64-bit cell indices (the LDS forms
    keep them in 32 bits): particles in the first and the last rows, compared on the rows they touch; sampled other
    rows stay zero"""
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip("needs 24 GiB of free device memory, %.1f GiB free" % (free / 2 ** 30))
    t0 = time.time()
    rep = Report("2^31 cells")
    R0, R1, K = 32768, 65536, 8
    full = SR.Splat(2, [R0, R1], [float(R0), float(R1)], 0.5, 4.0, 1000.0, 2, False, 0)
    assert full.cells == 2 ** 31
    rng = np.random.RandomState(8000)
    N = 300
    # positions on a lattice that float32 holds exactly (v in 1/64ths along axis 0, 1/128ths along axis 1, fractions
    # away from the faces): at v ~ 3e4 .. 6e4 four ulp are 0.02 .. 0.03 of a cell and random positions would lose
    # more than 1 % to the tie filter
    p = np.empty((2 * N, 2))
    u = rng.randint(0, K - 3, 2 * N) + rng.randint(8, 57, 2 * N) / 64.0       # own rows 0 .. K-4: neighbours stay inside K
    p[:N, 0] = u[:N] / R0
    p[N:, 0] = (R0 - u[N:]) / R0
    p[:, 1] = (rng.randint(-600, R1 + 600, 2 * N) + rng.randint(16, 113, 2 * N) / 128.0) / R1
    p[0] = [0.5 / R0, 0.5 / R1]                                     # the grid's corners
    p[1] = [0.5 / R0, 1 - 0.5 / R1]
    p[N] = [1 - 0.5 / R0, 0.5 / R1]
    p[N + 1] = [1 - 0.5 / R0, 1 - 0.5 / R1]
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    p = torch.tensor(p[rng.permutation(2 * N)].astype(np.float32), device=DEV)
    tie = full.near_tie(p)
    assert float(tie.double().mean()) <= 0.01
    p = p[~tie].contiguous()
    cfg = full.ops_cfg(ops)
    out = ops.p2g_fwd(p, cfg)
    assert out.shape == (R0, R1, 1)
    g = torch.zeros(R0, R1, 1, device=DEV)
    wins = [_Rows(full, 0, K), _Rows(full, R0 - K, R0)]
    gen = torch.Generator(device=DEV).manual_seed(1)
    for w in wins:
        lo = R0 - w.b
        g[lo:lo + K] = torch.randn(K, R1, 1, device=DEV, generator=gen)
    touched = 0
    gp_ref, gp_bound, gp_terms = 0, 0, None
    for w in wins:
        lo = R0 - w.b
        ref = w.p2g(p)
        rep.check("fwd rows", "rows %d..%d" % (lo, lo + K), out[lo:lo + K], ref["grid"], ref["bound"], ref["terms"])
        touched += int((out[lo:lo + K] != 0).sum())
        b = w.p2g_bwd(p, g[lo:lo + K])
        gp_ref, gp_bound = gp_ref + b["g_p"], gp_bound + b["g_p_bound"]
        gp_terms = b["g_p_terms"] if gp_terms is None else {k: gp_terms[k] + b["g_p_terms"][k] for k in gp_terms}
    assert touched > 0
    for r in [K, K + 1, R0 // 2 - 1, R0 // 2, R0 - K - 1] + rng.randint(K, R0 - K, 64).tolist():
        assert int((out[r] != 0).sum()) == 0, r
    assert int(torch.count_nonzero(out)) == touched                # and nothing anywhere else
    gp, _, _ = ops.p2g_bwd(p, cfg, g)
    rep.check("bwd g_p", "both windows", gp, gp_ref, gp_bound, gp_terms)
    torch.cuda.synchronize()
    rep.done()
    print("%-34s %.1f s" % (rep.name, time.time() - t0))


# ---- NFS_SPLAT_LDS=0: read once per process, hence a fresh child ----------------------------------------------------------------

_LDS_OFF_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
import neural_flow_style_amd.ops as ops
d = np.load(sys.argv[1])
dev = lambda k: torch.tensor(d[k], device="cuda") if k in d else None
out = {}
for mode in (0, 1, 2):
    t = "m%%d_" %% mode
    cfg = ops.make_splat_cfg(3, d["res"], d["domain"], float(d["radius"]), 4.0, 1000.0, 1, True, mode)
    p, a, pd, g, gw = dev("p"), dev(t + "a"), dev(t + "pd"), dev(t + "g"), dev(t + "gw")
    f = ops.p2g_fwd(p, cfg, attr=a, pd=pd)
    if mode == 2:
        out[t + "xs"], out[t + "ws"] = f[0].cpu().numpy(), f[1].cpu().numpy()
        out[t + "one_launch_is_none"] = np.array(ops.p2g_wavg_bwd(p, cfg, f[0], f[1], g, a) is None)
    else:
        out[t + "grid"] = f.cpu().numpy()
    gp, ga, gd = ops.p2g_bwd(p, cfg, g, attr=a, pd=pd, g_wsum=gw, need_p=True, need_attr=mode != 0, need_pd=mode == 1)
    for k, v in (("gp", gp), ("ga", ga), ("gd", gd)):
        if v is not None:
            out[t + k] = v.cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[2], **out)
"""


def test_lds_switched_off_in_a_child_process(ops, tmp_path):
    """NFS_SPLAT_LDS=0: the (3,1) forward sends every contribution to the grid with global atomics, the adjoint runs the
    generic gather, the one-launch weighted-average adjoint declines; same bounds"""
    rep = Report("NFS_SPLAT_LDS=0")
    rng = np.random.RandomState(9000)
    import neural_flow_style_amd.transform as T
    S0 = splat(3, 1, True, 0)
    p = drop_ties(S0, uniform_set(rng, 3000, 3))
    p = p[T.grid_order(p.clamp(0, 1), S0.res)].contiguous()
    data = dict(p=p.cpu().numpy(), res=np.asarray(S0.res), domain=np.asarray(S0.domain, np.float32), radius=np.float32(S0.radius))
    cases = {}
    for mode, C, use_pd in SET_MODES:
        S = splat(3, 1, True, mode)
        a, pd = attrs(rng, p.shape[0], C, mode, use_pd)
        g, gw = grads(rng, S, C)
        cases[mode] = (S, a, pd, g, gw)
        for k, v in (("a", a), ("pd", pd), ("g", g), ("gw", gw)):
            if v is not None:
                data["m%d_%s" % (mode, k)] = v.cpu().numpy()
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, **data)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ); env["NFS_SPLAT_LDS"] = "0"
    subprocess.run([sys.executable, "-c", _LDS_OFF_SCRIPT % root, fin, fout], check=True, env=env, timeout=300)
    o = np.load(fout)
    t = lambda k: torch.tensor(o[k], device=DEV)
    for mode, (S, a, pd, g, gw) in cases.items():
        ref = S.p2g(p, a, pd)
        b = S.p2g_bwd(p, g, a, pd, gw)
        m = "m%d_" % mode
        C = 1 if a is None else a.shape[1]
        if mode == 2:
            rep.check("fwd xsum", "mode 2", t(m + "xs"), ref["grid"], ref["bound"], {k: v[..., :C] for k, v in ref["terms"].items()})
            rep.check("fwd wsum", "mode 2", t(m + "ws"), ref["wsum"], ref["wsum_bound"])
            assert bool(o[m + "one_launch_is_none"])
        else:
            rep.check("fwd", "mode %d" % mode, t(m + "grid"), ref["grid"], ref["bound"], ref["terms"])
        rep.check("bwd g_p", "mode %d" % mode, t(m + "gp"), b["g_p"], b["g_p_bound"], b["g_p_terms"])
        if mode != 0:
            rep.check("bwd g_attr", "mode %d" % mode, t(m + "ga"), b["g_attr"], b["g_attr_bound"])
        if mode == 1:
            rep.check("bwd g_pd", "mode 1", t(m + "gd"), b["g_pd"], b["g_pd_bound"])
    rep.done()


# ---- g2p -------------------------------------------------------------------------------------------------------------------

G2P_DIMS = {2: [(16, 23), (1, 9), (2, 3), (3, 1), (7, 2)], 3: [(9, 12, 7), (1, 5, 6), (4, 2, 3), (3, 6, 1), (2, 1, 3)]}


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("cubic", [False, True])
@pytest.mark.parametrize("nd", [2, 3])
def test_g2p(ops, nd, cubic, C):
    rep = Report("g2p nd=%d %s C=%d" % (nd, "cubic" if cubic else "linear", C))
    rng = np.random.RandomState(9500 + 10 * nd + cubic + 100 * C)
    for dims in G2P_DIMS[nd]:
        g = torch.tensor(rng.randn(*dims, C).astype(np.float32), device=DEV)
        n = np.asarray(dims, np.float64)
        rand = rng.uniform(-0.3, 1.3, (1500, nd))
        # exact in float32: cell centres (k + 0.5) / n and faces k / n need n a power of two; take the float32 roundings
        # of them and let the filter drop those that became rounding decisions -- and keep exact ones by hand
        centres = (rng.randint(0, 64, (200, nd)) % n + 0.5) / n
        faces = (rng.randint(0, 64, (200, nd)) % (n + 1)) / n
        p = torch.tensor(np.concatenate([rand, centres, faces]).astype(np.float32), device=DEV)
        tie = SR.g2p_near_tie(p, dims)
        assert float(tie[:1500].double().mean()) <= 0.01
        n64 = torch.tensor(n, device=DEV)
        exact_x = ((p.double() * n64).float().double() == p.double() * n64).all(-1)   # x = p n exact in float32: kept
        p = p[~tie | exact_x].contiguous()
        exact = torch.tensor([[0.0] * nd, [1.0] * nd, [0.5] * nd, [-0.25] * nd, [1.25] * nd], device=DEV)
        p = torch.cat([p, exact]).contiguous()
        out = ops.g2p_fwd(g, p, cubic=cubic)
        ref, bound = SR.g2p(g, p, cubic)
        rep.check("g2p", str(dims), out, ref, bound)
    rep.done()

"""Float64 restatement of the SPH splat (csrc/splat.hip) -- p2g in its three modes, the weighted-average finish, their
adjoints in closed form, and g2p -- with a per-element bound on what a float32 kernel may differ from it by.

torch float64 on the device of the inputs: the CPU tests run it small, the GPU tests run it on the GPU.  It takes the
float32 tensors the kernel takes.

What is DISCRETE is decided the way the kernel decides it, in float32 from the same float32 inputs (``Splat.locate``):
v = p * dom, the clamp against the float32 value of dom - 1e-6 (which IS dom for every dom above 32: a clamped
particle then has its own cell at index res, outside the grid, and only its lower neighbours receive anything),
validity 0 <= v < dom, cell = dom[0] / res[0], the cell index floor(v / cell).  With nsize * cell below the kernel
support the neighbourhood truncates the kernel, so the cell index changes the result discontinuously and cannot be
left to a tolerance.  Everything continuous (r, q, W, dW, the sums) is float64.  ``discrete=torch.float64`` takes the
discrete decisions in float64 too: that is oracle.p2g run in float64, which the CPU test pins this file against.

Adjoints are written out, not taken by autograd: zero position gradient at a cell centre (the project's safe square
root); under ``clip`` the gradient of an axis passes where 0 <= v <= hi, TIES INCLUDED (TF's clip_by_value gradient,
reference transform.py:1321; torch.minimum in oracle._splat_common halves a tie instead).

Error bounds are first-order sums of the float32 roundings the kernels make, EPS = 2^-24 per correctly rounded
operation.  The constants, counted in splat.hip:

* K_V = 1, K_CENTRE = 2 (load_particle): v = p * dom is one rounding of v; (fl + 0.5) * cell carries the rounding of
  cell = dom[0] / res[0] and of the product (fl + 0.5 is exact); the subtraction adds one rounding of r.  At dom = 200
  these absolute errors (~ 3 EPS x 200) are the largest term of everything that depends on the position.
* K_OFF = 2 (Hood::init): r - n cell: the rounding of cell again and of the product n cell; + one rounding of the result.
* K_Q = 10 (weight(), p2g_bwd_box_kernel): d2 is nd squares and nd - 1 sums (5 roundings of d2 in 3-D: 2.5 of its
  root), v_rsq_f32 is within 2 ulp = 4 EPS, d2 * rsq one, 1 / h and the product by it two: 9.5.  The generic kernels
  (sqrtf, one division) make fewer.
* K_W = 8 (cubic_w, q <= 0.5): q q, q q q (two), the difference, x 6, + 1, x sigma, and sigma's own rounding, against
  terms of magnitude <= 1.5 sigma / 1.5: absolute 8 EPS sigma.  K_W1 = 6 (q > 0.5): 1 - q is exact (Sterbenz), t t t,
  x 2, x sigma, sigma: relative 6 EPS.  cubic_dw: the same counts.
* K_P = 5 (contribution): mass (one), mass / pd (one), coef w, x attribute, and in the LDS form the flush's conversion.
* accumulation: n contributions added in float in any order: n EPS sum |contribution| (the LDS form adds integers
  exactly and only its flush and the cross-block atomics round: covered).
* fixed point (p2g_fwd_lds_kernel): every contribution is truncated to a multiple of 2^-kexp of its block of 256
  particles, kexp = 62 - exponent(256 sigma cmax), cmax the block's largest |coefficient x attribute| (>= 1 x
  coefficient in mode 2, which also accumulates the bare weights): one quantum per contribution.
* K_G = 16 + C (adjoint, per cell): coef (two), the C products and sums of the dot product, coef x dot, cubic_dw
  (six), rsq (four), x 1 / h (two), f (two products), f r_k (one).
"""
import itertools
import math

import numpy as np
import torch

EPS = 2.0 ** -24
K_V = 1
K_CENTRE = 2
K_OFF = 2
K_Q = 10
K_W = 8
K_W1 = 6
K_P = 5
K_G = 16
K_FIN = 4          # finish adjoint, per channel: g x, w w, the division, the running sum
K_CR = 10          # g2p weights: t t, t t t, and per weight three products and two sums, against max(1, |t|)^3

SPL_LDS = 8192     # splat.hip: 64-bit accumulators of the forward's box
SPB_LDS = 12288    # splat.hip: floats of the adjoint's staged box
BLOCK = 256

f32 = np.float32


def _W(q, sigma):
    inner = torch.where(q <= 0.5, 6 * (q ** 3 - q ** 2) + 1, 2 * (1 - q).clamp(min=0) ** 3)
    return torch.where(q > 1, torch.zeros_like(q), sigma * inner)


def _dW(q, sigma):
    inner = torch.where(q <= 0.5, 6 * (3 * q * q - 2 * q), -6 * (1 - q) ** 2)
    return torch.where(q > 1, torch.zeros_like(q), sigma * inner)


def _D(q, sigma):
    """dW/dq / q (finite at 0) and a bound on |d/dq| of it"""
    qs = q.clamp(min=0.5)
    D = torch.where(q <= 0.5, 6 * (3 * q - 2), -6 * (1 - qs) ** 2 / qs)
    dD = torch.where(q <= 0.5, torch.full_like(q, 18.0), 6 * (1 / qs ** 2 - 1))
    out = q > 1
    return torch.where(out, torch.zeros_like(q), sigma * D), torch.where(out, torch.zeros_like(q), sigma * dD)


class Splat:
    """one splat configuration (the fields of nfs_splat_cfg), float32 parameters as the kernel reads them"""

    def __init__(self, nd, res, domain, radius, support=4.0, rest_density=1000.0, nsize=1, clip=True, mode=0,
                 discrete=torch.float32):
        self.nd, self.nsize, self.clip, self.mode = int(nd), int(nsize), bool(clip), int(mode)
        self.res = [int(v) for v in res[:nd]]
        self.domain = [float(f32(v)) for v in domain[:nd]]
        self.radius, self.support = float(f32(radius)), float(f32(support))
        self.rest_density = float(f32(rest_density))
        self.h = float(f32(radius) * f32(support))
        self.sigma = 8 / math.pi / self.h ** 3 if nd == 3 else 40 / 7 / math.pi / self.h ** 2
        self.mass = 0.8 * (2 * self.radius) ** nd * self.rest_density
        self.res0 = self.res[0]                       # cell = dom[0] / res[0], in float32 in _v and in float64 here
        self.cell = self.domain[0] / self.res0
        self.discrete = discrete
        self.hax = 0 if nd == 2 else 1
        self.cells = int(np.prod(self.res))

    def ops_cfg(self, ops):
        return ops.make_splat_cfg(self.nd, self.res, self.domain, self.radius, self.support, self.rest_density,
                                  self.nsize, self.clip, self.mode)

    def offsets(self):
        return itertools.product(range(-self.nsize, self.nsize + 1), repeat=self.nd)

    # ---- discrete part ----------------------------------------------------------------------------------------------
    def _v(self, p):
        dt = self.discrete
        dom = torch.tensor(self.domain, dtype=dt, device=p.device)
        v = p.to(dt) * dom
        hi = dom - torch.tensor(1e-6, dtype=dt, device=p.device)
        cell = dom[0] / torch.tensor(float(self.res0), dtype=dt, device=p.device)
        return v, dom, hi, cell

    def locate(self, p, v_err=0.0):
        """p [N,nd] float32 -> dict: idx [N,nd] own cell (may lie outside the grid), valid [N], grad_ok [N,nd],
        r [N,nd] float64 offset from the own cell's centre, dr [N,nd] bound on a float32 kernel's error of r
        (+ v_err, an error budget of v in domain units)"""
        v, dom, hi, cell = self._v(p)
        if self.clip:
            grad_ok = (v >= 0) & (v <= hi)
            v = torch.minimum(torch.clamp_min(v, 0), hi)
            valid = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
        else:
            grad_ok = torch.ones_like(v, dtype=torch.bool)
            valid = ((v >= 0) & (v < dom)).all(-1)
        fl = torch.floor(v / cell)
        v64 = p.double() * dom.double()
        if self.clip:
            v64 = torch.minimum(v64.clamp(min=0), hi.double())
        centre = (fl.double() + 0.5) * self.cell
        r = v64 - centre
        dr = EPS * (K_V * v64.abs() + K_CENTRE * centre.abs() + r.abs()) + v_err
        return dict(idx=fl.long(), valid=valid, grad_ok=grad_ok, r=r, dr=dr, v=v)

    def near_tie(self, p, ulps=4):
        """particles whose cell, validity or clamp is a rounding decision: float32 v / cell within ``ulps`` ulp of an
        integer, or v within ``ulps`` ulp of 0 (in ulp of a cell), hi or dom"""
        v, dom, hi, cell = self._v(p.float() if self.discrete == torch.float32 else p)
        u = ulps * 2.0 ** -23
        t = (v / cell).double()
        tie = (t - torch.round(t)).abs() <= u * t.abs().clamp(min=1.0)
        v = v.double()
        tie |= (v.abs() <= u * float(cell)) | ((v - hi.double()).abs() <= u * hi.double()) | \
               ((v - dom.double()).abs() <= u * dom.double())
        return tie.any(-1)

    def lin(self, c):
        """cells c [N,nd] -> (linear index with the H flip, inside-the-grid mask); outside cells are dropped, as
        TF's GPU scatter_nd drops them (oracle._scatter_nd)"""
        ok = torch.ones(c.shape[0], dtype=torch.bool, device=c.device)
        lin = torch.zeros(c.shape[0], dtype=torch.long, device=c.device)
        for k, n in enumerate(self.res):
            ck = c[:, k]
            ok = ok & (ck >= 0) & (ck < n)
            ck = ck.clamp(0, n - 1)
            if k == self.hax:
                ck = n - 1 - ck
            lin = lin * n + ck
        return lin, ok

    def block_boxes(self, p):
        """per block of 256 consecutive particles: the volume (cells) of the box of its valid particles' own cells,
        widened by nsize and clipped to the grid -- what the kernels compare with SPL_LDS / SPB_LDS (x channels);
        0 for a block with no valid particle"""
        L = self.locate(p)
        N = p.shape[0]
        nb = (N + BLOCK - 1) // BLOCK
        blk = torch.arange(N, device=p.device) // BLOCK
        vol = torch.ones(nb, dtype=torch.long, device=p.device)
        anyv = torch.zeros(nb, dtype=torch.bool, device=p.device).index_put_((blk[L["valid"]],), torch.tensor(True, device=p.device))
        for k, n in enumerate(self.res):
            i = L["idx"][:, k]
            big = 2 ** 31 - 1
            lo = torch.full((nb,), big, dtype=torch.long, device=p.device).scatter_reduce(
                0, blk, torch.where(L["valid"], i, torch.full_like(i, big)), "amin")
            hi = torch.full((nb,), -1, dtype=torch.long, device=p.device).scatter_reduce(
                0, blk, torch.where(L["valid"], i, torch.full_like(i, -1)), "amax")
            ext = torch.minimum(hi + self.nsize, torch.tensor(n - 1, device=p.device)) - (lo - self.nsize).clamp(min=0) + 1
            vol = vol * ext.clamp(min=1)
        return torch.where(anyv, vol, torch.zeros_like(vol))

    def channels(self, C):
        """(forward accumulators, adjoint floats) per cell of the LDS boxes"""
        return (1 if self.mode == 0 else (C + 1 if self.mode == 2 else C)), (C + 1 if self.mode == 2 else C)

    # ---- shared per-offset geometry -----------------------------------------------------------------------------------
    def _hood(self, L, n):
        dev = L["r"].device
        nn = torch.tensor(n, dtype=torch.float64, device=dev)
        rr = L["r"] - nn * self.cell
        drr = L["dr"] + EPS * (K_OFF * nn.abs() * self.cell + rr.abs())
        dist = (rr * rr).sum(-1).sqrt()
        q = dist / self.h
        dq_r = L["dr"].sum(-1) / self.h                                    # the part of q's error that r's error makes
        dq = drr.sum(-1) / self.h + K_Q * EPS * q
        lin, ok = self.lin(L["idx"] + torch.tensor(n, device=dev))
        ok = ok & L["valid"] & (q <= 1 + dq)                               # (a kernel's q may fall inside where q > 1)
        return rr, drr, dist, q, dq_r, dq, lin, ok

    def _coef(self, L, attr, pd):
        """coefficient [N] and channel factors A [N,Ch] of the forward (mode 2: the bare weight is the last channel)"""
        N, dev = L["r"].shape[0], L["r"].device
        one = torch.ones(N, 1, dtype=torch.float64, device=dev)
        if self.mode == 0:
            return torch.full((N,), self.mass, dtype=torch.float64, device=dev), one
        if self.mode == 1:
            den = pd.double().reshape(-1) if pd is not None else torch.full((N,), self.rest_density, dtype=torch.float64, device=dev)
            return self.mass / den, attr.double()
        return torch.ones(N, dtype=torch.float64, device=dev), torch.cat([attr.double(), one], -1)

    def _W_err(self, q, dq, dq_r):
        """W, and a kernel's error of it split in (from r's error, from everything else)"""
        s = self.sigma
        W, dWa = _W(q, s), _dW(q, s).abs()
        ev = torch.where(q <= 0.5, torch.full_like(q, K_W * EPS * s), K_W1 * EPS * W)
        return W, dWa * dq_r, dWa * (dq - dq_r) + 6 * s * dq * dq + ev

    def quantum(self, L, coef, A):
        """[N]: fixed-point quantum 2^-kexp of each particle's block (0 where the block takes the float path)"""
        N, dev = coef.shape[0], coef.device
        am = A.abs().amax(-1) if self.mode != 0 else torch.ones_like(coef)
        cm = torch.where(L["valid"], coef.abs() * am, torch.zeros_like(coef))
        nb = (N + BLOCK - 1) // BLOCK
        blk = torch.arange(N, device=dev) // BLOCK
        cmax = torch.zeros(nb, dtype=torch.float64, device=dev).scatter_reduce(0, blk, cm, "amax")
        bnd = 256 * self.sigma * cmax * (1 + 8 * EPS)                      # (the kernel forms it in float32: round up)
        _, e = torch.frexp(bnd)
        quant = torch.where(bnd > 0, torch.ldexp(torch.ones_like(bnd), e - 62), torch.zeros_like(bnd))
        return quant[blk]

    # ---- forward ------------------------------------------------------------------------------------------------------
    def p2g(self, p, attr=None, pd=None, v_err=0.0):
        """-> dict(grid [*res,C], bound, terms {name: [*res,C]}) and, mode 2, wsum / wsum_bound [*res,1] (grid is xsum).
        terms: 'r' position error, 'eval' the arithmetic of q, W and the products, 'acc' float accumulation,
        'quant' the LDS fixed-point quanta"""
        L = self.locate(p, v_err)
        dev = p.device
        coef, A = self._coef(L, attr, pd)
        ca = coef[:, None] * A
        Ch = A.shape[1]
        z = lambda: torch.zeros(self.cells, Ch, dtype=torch.float64, device=dev)
        val, e_r, e_ev, S, cnt, Q = z(), z(), z(), z(), z(), z()
        quant = self.quantum(L, coef, A)
        for n in self.offsets():
            rr, drr, dist, q, dq_r, dq, lin, ok = self._hood(L, n)
            W, w_r, w_ev = self._W_err(q, dq, dq_r)
            i = lin[ok]
            c = ca[ok]
            val.index_add_(0, i, c * W[ok, None])
            e_r.index_add_(0, i, c.abs() * w_r[ok, None])
            e_ev.index_add_(0, i, c.abs() * (w_ev + K_P * EPS * W)[ok, None])
            S.index_add_(0, i, c.abs() * W[ok, None])
            cnt.index_add_(0, i, torch.ones_like(c))
            Q.index_add_(0, i, quant[ok, None].expand_as(c))
        terms = dict(r=e_r, eval=e_ev, acc=cnt * EPS * S, quant=Q)
        bound = sum(terms.values())
        shp = tuple(self.res)
        out = dict(terms={k: t.reshape(shp + (Ch,)) for k, t in terms.items()})
        if self.mode == 2:
            C = Ch - 1
            out.update(grid=val[:, :C].reshape(shp + (C,)), bound=bound[:, :C].reshape(shp + (C,)),
                       wsum=val[:, C:].reshape(shp + (1,)), wsum_bound=bound[:, C:].reshape(shp + (1,)))
        else:
            out.update(grid=val.reshape(shp + (Ch,)), bound=bound.reshape(shp + (Ch,)))
        return out

    # ---- adjoint ------------------------------------------------------------------------------------------------------
    def p2g_bwd(self, p, g_grid, attr=None, pd=None, g_wsum=None, g_err=None, gw_err=None):
        """closed-form adjoints at the grid gradient g_grid [*res,C] (mode 2: and g_wsum [*res,1]); g_err / gw_err:
        per-cell error budgets of those inputs (same shapes).  -> dict(g_p, g_p_bound, g_p_terms, and where the mode
        has them g_attr, g_attr_bound, g_pd, g_pd_bound)"""
        L = self.locate(p)
        dev, N, nd = p.device, p.shape[0], self.nd
        s, h = self.sigma, self.h
        coef, _ = self._coef(L, attr, pd)
        C = 1 if self.mode == 0 else attr.shape[1]
        at = torch.ones(N, 1, dtype=torch.float64, device=dev) if self.mode == 0 else attr.double()
        G = g_grid.double().reshape(self.cells, C)
        GE = torch.zeros_like(G) if g_err is None else g_err.double().reshape(self.cells, C)
        if self.mode == 2:
            GW = g_wsum.double().reshape(self.cells)
            GWE = torch.zeros_like(GW) if gw_err is None else gw_err.double().reshape(self.cells)
        zp = lambda: torch.zeros(N, nd, dtype=torch.float64, device=dev)
        zc = lambda: torch.zeros(N, C, dtype=torch.float64, device=dev)
        gp, p_r, p_ev, p_in, p_S = zp(), zp(), zp(), zp(), zp()
        ga, a_e, a_S = zc(), zc(), zc()
        gd, d_e, d_S = (torch.zeros(N, dtype=torch.float64, device=dev) for _ in range(3))
        cnt = torch.zeros(N, dtype=torch.float64, device=dev)
        pdv = pd.double().reshape(-1) if (self.mode == 1 and pd is not None) else \
            torch.full((N,), self.rest_density if self.mode == 1 else 1.0, dtype=torch.float64, device=dev)
        for n in self.offsets():
            rr, drr, dist, q, dq_r, dq, lin, ok = self._hood(L, n)
            m = ok.double()
            gv, ge = G[lin] * m[:, None], GE[lin] * m[:, None]
            dot, dotm, dote = (at * gv).sum(-1), (at * gv).abs().sum(-1), (at.abs() * ge).sum(-1)
            gw, gwm, gwe = coef * dot, coef.abs() * dotm, coef.abs() * dote
            if self.mode == 2:
                gw, gwm, gwe = gw + GW[lin] * m, gwm + (GW[lin] * m).abs(), gwe + GWE[lin] * m
            cnt += m
            # position: f r_k with f = gw D(q) / h^2, D = dW/dq / q; no term at the cell centre (safe square root)
            D, dD = _D(q, s)
            live = (dist > 0).double()
            fm = gwm * live / (h * h)
            gp += (gw * live * D / (h * h))[:, None] * rr
            Da, ra = D.abs()[:, None], rr.abs()
            p_r += fm[:, None] * (Da * L["dr"] + ra * (dD * dq_r)[:, None])
            p_ev += fm[:, None] * (Da * (drr - L["dr"]) + ra * (dD * (dq - dq_r) + 48 * s * dq * dq)[:, None]
                                   + (K_G + C) * EPS * Da * ra)
            p_in += (gwe * live / (h * h))[:, None] * Da * ra
            p_S += fm[:, None] * Da * ra
            if self.mode != 0:
                W, w_r, w_ev = self._W_err(q, dq, dq_r)
                dW_all = w_r + w_ev
                cw = (coef * W)[:, None]
                ga += cw * gv
                a_e += (coef.abs() * dW_all)[:, None] * gv.abs() + cw.abs() * (ge + K_P * EPS * gv.abs())
                a_S += cw.abs() * gv.abs()
                if self.mode == 1:
                    gd -= coef * W * dot / pdv
                    d_e += (coef.abs() * (dW_all * dotm + W * (dote + (K_P + C + 1) * EPS * dotm))) / pdv.abs()
                    d_S += coef.abs() * W * dotm / pdv.abs()
        dom = torch.tensor(self.domain, dtype=torch.float64, device=dev)
        okf = L["grad_ok"].double()
        terms = dict(r=p_r * dom * okf, eval=(p_ev + EPS * gp.abs()) * dom * okf, input=p_in * dom * okf,
                     acc=cnt[:, None] * EPS * p_S * dom * okf)
        out = dict(g_p=gp * dom * okf, g_p_bound=sum(terms.values()), g_p_terms=terms)
        if self.mode != 0:
            out.update(g_attr=ga, g_attr_bound=a_e + cnt[:, None] * EPS * a_S)
        if self.mode == 1:
            out.update(g_pd=gd, g_pd_bound=d_e + cnt * EPS * d_S)
        return out


# ---- weighted-average finish ------------------------------------------------------------------------------------------

def _eps32(eps):
    return float(f32(eps))


def wavg_finish(xsum, wsum, eps=1e-6, x_err=None, w_err=None):
    """out = xsum / wsum where wsum > eps else xsum.  -> (out, bound, decided): with error budgets of the sums, a cell
    whose |wsum - eps| lies inside w_err is undecided (the switch changes its value by 1e6) and left out by the caller"""
    x, w = xsum.double(), wsum.double()
    xe = torch.zeros_like(x) if x_err is None else x_err.double()
    we = torch.zeros_like(w) if w_err is None else w_err.double()
    e = _eps32(eps)
    on = w > e
    ws = torch.where(on, w, torch.ones_like(w))
    out = torch.where(on, x / ws, x)
    bound = torch.where(on, xe / ws + x.abs() * we / (ws * ws) / (1 - (we / ws).clamp(max=0.5)), xe) + EPS * out.abs()
    decided = (w - e).abs() > we
    return out, bound, decided


def wavg_finish_bwd(xsum, wsum, g_out, eps=1e-6):
    """adjoint of wavg_finish at g_out: g_xsum = g / w, g_wsum = -sum_c g x / w^2 where w > eps; g and 0 elsewhere.
    -> (g_xsum, g_xsum_bound, g_wsum, g_wsum_bound)"""
    x, w, g = xsum.double(), wsum.double(), g_out.double()
    on = w > _eps32(eps)
    ws = torch.where(on, w, torch.ones_like(w))
    gx = torch.where(on, g / ws, g)
    t = g * x / (ws * ws)
    gw = torch.where(on[..., 0], -t.sum(-1), torch.zeros_like(w[..., 0]))[..., None]
    gwb = torch.where(on[..., 0], K_FIN * EPS * t.abs().sum(-1), torch.zeros_like(w[..., 0]))[..., None]
    return gx, torch.where(on, EPS * gx.abs(), torch.zeros_like(gx)), gw, gwb


# ---- g2p --------------------------------------------------------------------------------------------------------------

def _g2p_axis(pk, n, cubic, discrete):
    x = (pk.to(discrete) * torch.tensor(float(n), dtype=discrete, device=pk.device))
    b = torch.floor(x - 0.5).long()                                       # float32: the kernel's floorf(x - 0.5f)
    x64 = pk.double() * n
    if not cubic:
        i0, i1 = b.clamp(0, n - 1), (b + 1).clamp(0, n - 1)
        dx = x64 - (i0.double() + 0.5)
        e = EPS * (x64.abs() + 2 * dx.abs() + 1)                          # x, the subtraction, 1 - dx
        return [i0, i1], [1 - dx, dx], [e, e]
    idx = [(b + k).clamp(0, n - 1) for k in (-1, 0, 1, 2)]
    t = x64 - (idx[1].double() + 0.5)
    dt = EPS * (x64.abs() + t.abs())
    t2, t3 = t * t, t * t * t
    w = [-0.5 * t3 + t2 - 0.5 * t, 1.5 * t3 - 2.5 * t2 + 1.0, -1.5 * t3 + 2.0 * t2 + 0.5 * t, 0.5 * t3 - 0.5 * t2]
    a = t.abs()
    dw = [1.5 * t2 + 2 * a + 0.5, 4.5 * t2 + 5 * a, 4.5 * t2 + 4 * a + 0.5, 1.5 * t2 + a]       # >= |dw_j / dt|
    mag = a.clamp(min=1.0) ** 3
    return idx, w, [d * dt + K_CR * EPS * mag for d in dw]


def g2p_near_tie(p, dims, ulps=4):
    """particles whose floor(x - 0.5) is a rounding decision"""
    n = torch.tensor([float(v) for v in dims], dtype=torch.float32, device=p.device)
    x = p.float() * n
    y = (x - 0.5).double()
    u = ulps * 2.0 ** -23
    return ((y - torch.round(y)).abs() <= u * x.double().abs().clamp(min=1.0)).any(-1)


def g2p(g, p, cubic=True, discrete=torch.float32):
    """g [X,Y,(Z),C], p [N,nd] -> (out [N,C], bound)"""
    nd = p.shape[1]
    dims = list(g.shape[:nd])
    C = g.shape[-1]
    gf = g.double().reshape(-1, C)
    ax = [_g2p_axis(p[:, a], dims[a], cubic, discrete) for a in range(nd)]
    out = torch.zeros(p.shape[0], C, dtype=torch.float64, device=p.device)
    err = torch.zeros_like(out)
    S = torch.zeros_like(out)
    taps = 4 if cubic else 2
    for combo in itertools.product(range(taps), repeat=nd):
        flat, w, we = 0, None, None
        for a in range(nd):
            wa, ea = ax[a][1][combo[a]], ax[a][2][combo[a]]
            flat = flat * dims[a] + ax[a][0][combo[a]]
            if w is None:
                w, we = wa, ea
            else:
                w, we = w * wa, we * wa.abs() + ea * w.abs() + we * ea
        gv = gf[flat]
        out += w[:, None] * gv
        err += (we + nd * EPS * w.abs())[:, None] * gv.abs()
        S += w.abs()[:, None] * gv.abs()
    return out, err + (taps ** nd) * EPS * S


def err_ratio(err, bound):
    """largest err / bound (elements with bound 0 must have err 0)"""
    err, bound = err.double(), bound.double()
    if bool(((bound == 0) & (err != 0)).any()):
        return math.inf
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


def dominant(terms, err, bound):
    """name of the largest bound term at the element with the largest err / bound"""
    r = torch.where(bound > 0, err.double() / bound.clamp(min=1e-300), torch.zeros_like(bound)).reshape(-1)
    if r.numel() == 0:
        return "-"
    i = int(r.argmax())
    return max(terms, key=lambda k: float(terms[k].reshape(-1)[i]))

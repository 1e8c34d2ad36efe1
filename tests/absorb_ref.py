"""Float64 restatement of the liquid colour render's derivative in the density it is seen through (include/nfs_absorb.h,
engine.ColourRenderLoss.loss_and_grad(absorb=True), target_field 'pc' of styler_3p): the closed form of g_S per ray, a
per-element bound on what a float32 kernel may differ from it by, in tests/colour_liquid_ref.py's style and on
tests/view_ref.py's constants, and the joint frame loss (v, c) -> loss of the particle stylizer.

The model (tests/colour_liquid_ref.py: rays along axis 0, the far end z = D - 1 first), S the samples of the absorbing
volume, Q [D,...,C] the samples of the emission, g [...,C] the gradient at J = sum_z w Q + t bg:
    a[z] = sum_c g[c] Q[z,c]      b = sum_c g[c] bg[c]      P[z] = sum_{z'' < z} a[z''] w[z'']
    psi(x) = phi'(x) / phi(x) = 1 / (e^x - 1) - 1 / x,  psi(0) = -1/2
    g_S[z] = tau (a[z] w[z] psi(tau S[z]) - P[z] - t b)

The bound (``absorb``), a first-order sum of the float32 roundings a kernel can make.  s, es: the samples of d and their
bound; Q, eQ: those of q; w, e_w, t, e_t: LR.ray's (the kernel reads the float32 w and t that nfs_liquid_weights wrote,
each within its own bound of the float64 value used here):
* a: C products and C - 1 sums, each rounding against at most sum_c |g Q|: e_a = sum_c |g| eQ + 2 C EPS sum_c |g Q|.
* aw = a w: e_aw = |w| e_a + |a| e_w + EPS |a w|, + TINY where the product underflows.
* psi.  K_PSI = 8, ABSOLUTE (|psi| <= 1/2), from the kernel's branches as csrc/absorb.hip states them: below x = 1 a
  five-term alternating series in Horner form -- truncation below x^9 / 47900160 < 2.1e-8 (0.35 EPS), four inner
  roundings against values below 1/12 and the last sum's against 1/2: under 2 EPS; from 1 to 32 the difference
  1 / expm1(x) - 1 / x with quotients at most 0.582 and 1 -- expm1 within 2 ulp (4 EPS) and its quotient's rounding:
  5 EPS x 0.582 = 2.9 EPS, the second quotient EPS, the difference EPS / 2: 4.4 EPS; from 32 on -1 / x, leaving out
  less than 1.3e-14: under EPS.  x = tau s carries its own rounding, passed on by |x psi'(x)| <= 0.18: 0.2 EPS.  8 EPS
  covers each branch with slack.  psi passes the sample's error on by |d psi / d s| = tau |psi'| <= tau / 12.
* aw psi: e_1 = |psi| e_aw + |aw| e_psi + EPS |aw psi|.
* P, a sequential float32 sum of at most D terms: e_P = sum_{z'' < z} e_aw + D EPS sum_{z'' < z} |aw|.
* t b: b is C products and sums of exact numbers, e_b = 2 C EPS sum_c |g bg|; e_tb = |b| e_t + t e_b + EPS |t b|.
* the two differences and the product by tau: 3 EPS tau (|aw psi| + |P| + |t b|).
Nothing here is fitted to the kernel."""
import numpy as np
import torch

from oracle import nfs_oracle as O
from tests import colour_liquid_ref as LR
from tests import colour_ref as CR
from tests import view_ref as VR

EPS = VR.EPS
K_PSI = 8
TINY = LR.TINY
PSI_SERIES_BELOW = 1.0               # the kernel's change of form (csrc/absorb.hip); the tests put samples on both sides


def psi_series(x, terms=5):
    """-1/2 + x/12 - x^3/720 + x^5/30240 - x^7/1209600 (B_n x^(n-1) / n!)"""
    coef = [-0.5, 1.0 / 12, -1.0 / 720, 1.0 / 30240, -1.0 / 1209600][:terms]
    out = torch.full_like(x, coef[0])
    for k, c in enumerate(coef[1:]):
        out = out + c * x ** (2 * k + 1)
    return out


def psi_quotient(x):
    return 1.0 / torch.expm1(x) - 1.0 / x


def psi(x):
    """1 / (e^x - 1) - 1 / x in float64 with the limit -1/2 at 0 (and at -0.0): below 0.05 the five-term series, whose
    truncation x^9 / 47900160 is under 5e-20; above it the quotient, whose cancellation costs 2 ulp / x < 1e-14"""
    small = x.abs() < 0.05
    xs = torch.where(small, torch.ones_like(x), x)
    return torch.where(small, psi_series(x), psi_quotient(xs))


def _prefix_exclusive(x):
    return torch.cumsum(x, 0) - x


def closed_form(S, Q, g, bg, tau):
    """S [D,...] samples, Q [D,...,C], g [...,C], bg [C] (float64) -> g_S [D,...] by the formula above, with w and t
    formed from S"""
    B = VR._suffix(S) - S
    w = tau * torch.exp(-tau * B) * LR.phi(tau * S)
    t = torch.exp(-tau * S.sum(0))
    a = (Q * g.unsqueeze(0)).sum(-1)
    b = (g * bg).sum(-1)
    aw = a * w
    return tau * (aw * psi(tau * S) - _prefix_exclusive(aw) - t * b)


def absorb(s, es, Q, eQ, g, bg, tau):
    """one view: s, es [D,H,W]; Q, eQ [D,H,W,C]; g [H,W,C]; bg [C] -> dict g_s, e_g_s [D,H,W] and the ray quantities w,
    e_w, t, e_t of LR.ray"""
    D, C = s.shape[0], Q.shape[-1]
    r = LR.ray(s, es, tau)
    w, e_w, t, e_t = r["w"], r["e_w"], r["t"], r["e_t"]
    gq = Q * g.unsqueeze(0)
    a = gq.sum(-1)
    e_a = (eQ * g.abs().unsqueeze(0)).sum(-1) + 2 * C * EPS * gq.abs().sum(-1)
    aw = a * w
    e_aw = w.abs() * e_a + a.abs() * e_w + EPS * aw.abs() + TINY
    x = tau * s
    ps = psi(x)
    e_ps = K_PSI * EPS + tau / 12.0 * es
    t1 = aw * ps
    e_1 = ps.abs() * e_aw + aw.abs() * e_ps + EPS * t1.abs()
    P = _prefix_exclusive(aw)
    Pabs = _prefix_exclusive(aw.abs())
    e_P = _prefix_exclusive(e_aw) + D * EPS * Pabs
    gb = g * bg
    b = gb.sum(-1)
    e_b = 2 * C * EPS * gb.abs().sum(-1)
    tb = t * b
    e_tb = b.abs() * e_t + t * e_b + EPS * tb.abs()
    g_s = tau * (t1 - P - tb)
    e = tau * (e_1 + e_P + e_tb) + 3 * EPS * tau * (t1.abs() + P.abs() + tb.abs())
    # a ray whose gradient is exactly zero is exact zeros whatever the roundings
    dead = (g == 0).all(-1).unsqueeze(0).expand_as(e)
    e = torch.where(dead, torch.zeros_like(e), e)
    return dict(g_s=g_s, e_g_s=e, w=w, e_w=e_w, t=t, e_t=e_t, aw=aw)


def view(st, d, q, g, bg, tau):
    """``absorb`` of one view from its view_ref.Stencil: d [D,H,W], q [D,H,W,C], g [H,W,C] (float64)"""
    s, es = st.sample(d)
    QS = [st.sample(q[..., c]) for c in range(q.shape[-1])]
    return absorb(s, es, torch.stack([x[0] for x in QS], -1), torch.stack([x[1] for x in QS], -1), g, bg, tau), s, es


# ---- the model in torch float64, differentiable in the density ---------------------------------------------------------

def model_image(S, Q, bg, tau):
    """J [...,C] of samples S [D,...] and Q [D,...,C] on LR's formulas (S may require grad)"""
    B = VR._suffix(S) - S
    w = tau * torch.exp(-tau * B) * LR.phi(tau * S)
    t = torch.exp(-tau * S.sum(0))
    return (w.unsqueeze(-1) * Q).sum(0) + t.unsqueeze(-1) * bg


# ---- target_field 'pc': the joint frame loss --------------------------------------------------------------------------

def raw_volume(x, cfg, res):
    """p2g(x) / rest_density [1,D,H,W,1] (differentiable in x)"""
    return O.p2g(x.unsqueeze(0), cfg["domain"], res, cfg["radius"], cfg["rest_density"], cfg["nsize"], is_2d=False,
                 clip=cfg["clip"], support=cfg["support"]) / cfg["rest_density"]


def pressure_loss(d_raw, cfg):
    if not cfg.get("w_pressure", 0):
        return 0.0
    pr = torch.where(d_raw > 0, d_raw - 1, torch.zeros_like(d_raw))
    return (pr ** 2).mean() * cfg["w_pressure"]


def joint_frame_loss(p, r, v, c, cfg, res, R, weights_, style_feats, absorbing=True):
    """one frame's loss of the displacements v [N,3] and colours c [N,3] through ONE view batch R [v,3,3]: both splats at
    p + v -> smoothing -> liquid weights and image over the background -> clamp -> loss network, no mask; plus the pressure
    term.  ``absorbing=False`` detaches the absorbing volume (what a gradient that left the new path out would see)"""
    x = p + v
    d_raw = raw_volume(x, cfg, res)
    e = O.smooth3d_relu(d_raw, cfg["k"])[0, ..., 0]
    if not absorbing:
        e = e.detach()
    q = CR.colour_volume(x, r, c, cfg, res)
    w, t, _ = LR.weights(e, R, LR.tau_of(cfg))
    img = torch.clamp(LR.image(q, R, w, t, LR.background_of(cfg)), 0, 1)
    assert not cfg.get("style_mask")
    return CR.image_loss(img, None, cfg, weights_, style_feats) + pressure_loss(d_raw, cfg)


def joint_loss_and_grad(p, r, v, c, cfg, res, R, weights_, style_feats, absorbing=True):
    """(loss, d loss / d v, d loss / d c) by autograd, float64; R [V,3,3] is cut into view batches of cfg['v_batch'] whose
    losses add (the pressure term once per evaluation, as the stylizer adds it)"""
    v64 = torch.as_tensor(np.asarray(v, np.float64)).clone().requires_grad_()
    c64 = torch.as_tensor(np.asarray(c, np.float64)).clone().requires_grad_()
    R = torch.as_tensor(np.asarray(R, np.float32)).double()
    nopress = dict(cfg, w_pressure=0)
    l = 0.0
    for k, Rb in enumerate(LR._view_batches(cfg, R)):
        l = l + joint_frame_loss(p, r, v64, c64, cfg if k == 0 else nopress, res, Rb, weights_, style_feats, absorbing)
    g_v, g_c = torch.autograd.grad(l, [v64, c64])
    return float(l.detach()), g_v, g_c

"""Float64 restatement of the smoke colour render at a fixed exposure (include/nfs_exposure.h,
engine.ColourRenderLoss(render="exposure")) -- the ray weights w, the grey image, the image J and the closed form of the
derivative g_S in the density -- with a counted per-element bound on what a float32 kernel may differ from it by, in
tests/absorb_ref.py's style and on tests/view_ref.py's constants; and the frame losses of the stylizers under it.

The model, rays along axis 0, the far end z = D - 1 first, S the samples of the absorbing volume, Q [D,...,C] those of the
emission, tau the transmit coefficient, kappa the exposure:
    T[z] = exp(-tau sum_{z' >= z} S[z'])   (inclusive)        w[z] = kappa tau T[z]
    J[c] = sum_z w[z] Q[z,c]                                   grey = sum_z w[z] S[z]   <= kappa (1 - exp(-tau sum_z S))
and at the gradient g [...,C] of J, q held constant, a[z] = sum_c g[c] Q[z,c]:
    g_S[z] = -tau sum_{z' <= z} a[z'] w[z']                    (inclusive prefix from z = 0)
J is linear in q with the weights w, so the projection and its transpose are tests/colour_ref.py's (``CR.image``).

The bounds, first-order sums of the float32 roundings a kernel can make, counted from the operations.  s, es: the samples
of d and their bound (view_ref.Stencil.sample); EPS = 2^-24; TINY = 2^-126 wherever a result may underflow (the hardware
exp2 returns no denormals).
``ray`` (the weights and the grey image):
* the running sum A[z] = sum_{z' >= z} s, a sequential float32 sum of at most D samples: the samples' own errors add, and
  each of at most D additions rounds against a partial sum of at most sum_{z' >= z} |s|:
      e_A = sum_{z' >= z} es + D EPS sum_{z' >= z} |s|.
* T = exp2(A * (-tau log2 e)): the constant's rounding and the product's (2 EPS relative in the exponent, tau |A| at most:
  4 EPS tau sum |s| with slack, as view_ref counts it) and the hardware exp2 with its argument's rounding (K_EXP EPS, ONE
  exponential):  e_T = T (tau (e_A + 4 EPS sum_{z' >= z} |s|) + K_EXP EPS) + TINY.
* w = (kappa tau) T: the product kappa tau rounds once, its product with T once: e_w = kappa tau e_T + 2 EPS w + TINY.
* grey = sum_z w s, D products (or fused multiply-adds: fewer roundings) and a sequential sum of D terms:
      e_grey = sum_z (|s| e_w + w es) + (D + 1) EPS sum_z |w s|.
``absorb`` (g_S; the kernel reads the float32 w that nfs_exposure_weights wrote, within e_w of the float64 w used here):
* a: C products and C - 1 sums, each rounding against at most sum_c |g Q|, and the samples' errors eQ:
      e_a = sum_c |g| eQ + 2 C EPS sum_c |g Q|                 (absorb_ref's count)
* a w: e_aw = |w| e_a + |a| e_w + EPS |a w| + TINY.
* the prefix P[z] = sum_{z' <= z} a w, a sequential sum of at most D terms: e_P = sum_{z' <= z} e_aw + D EPS sum_{z' <= z} |a w|.
* g_S = (-tau) P: one product (the negation is exact): e = tau e_P + EPS tau |P| + TINY.
A ray whose gradient is exactly zero gives exact zeros.  Nothing here is fitted to the kernel."""
import numpy as np
import torch

from oracle import nfs_oracle as O
from tests import absorb_ref as AR
from tests import colour_grid_ref as GR
from tests import colour_liquid_ref as LR
from tests import colour_ref as CR
from tests import view_ref as VR

EPS = VR.EPS
TINY = LR.TINY


def _prefix(x):
    return torch.cumsum(x, 0)


def weights_of(S, tau, kappa):
    """S [D,...] (float64) -> w [D,...] = kappa tau exp(-tau sum_{z' >= z} S)"""
    return kappa * tau * torch.exp(-tau * VR._suffix(S))


def model_image(S, Q, tau, kappa):
    """J [...,C] of samples S [D,...] and Q [D,...,C] (S may require grad)"""
    return (weights_of(S, tau, kappa).unsqueeze(-1) * Q).sum(0)


def grey_of(S, tau, kappa):
    return (weights_of(S, tau, kappa) * S).sum(0)


def closed_form(S, Q, g, tau, kappa):
    """S [D,...], Q [D,...,C], g [...,C] (float64) -> g_S [D,...] = -tau sum_{z' <= z} a w, w formed from S"""
    a = (Q * g.unsqueeze(0)).sum(-1)
    return -tau * _prefix(a * weights_of(S, tau, kappa))


def ray(s, es, tau, kappa):
    """s [D,...] samples along axis 0 (float64), es their error bound -> dict w, e_w [D,...], grey, e_grey, t [...]"""
    D = s.shape[0]
    sa = s.abs()
    A, Aabs = VR._suffix(s), VR._suffix(sa)
    eA = VR._suffix(es) + D * EPS * Aabs
    T = torch.exp(-tau * A)
    eT = T * (tau * (eA + 4 * EPS * Aabs) + VR.K_EXP * EPS) + TINY
    w = kappa * tau * T
    e_w = kappa * tau * eT + 2 * EPS * w + TINY
    ws = w * s
    grey = ws.sum(0)
    e_grey = (sa * e_w + w * es).sum(0) + (D + 1) * EPS * ws.abs().sum(0)
    return dict(w=w, e_w=e_w, grey=grey, e_grey=e_grey, t=torch.exp(-tau * s.sum(0)))


def absorb(w, e_w, Q, eQ, g, tau):
    """one view: w, e_w [D,H,W] (``ray``'s); Q, eQ [D,H,W,C]; g [H,W,C] -> dict g_s, e_g_s [D,H,W], aw"""
    D, C = w.shape[0], Q.shape[-1]
    gq = Q * g.unsqueeze(0)
    a = gq.sum(-1)
    e_a = (eQ * g.abs().unsqueeze(0)).sum(-1) + 2 * C * EPS * gq.abs().sum(-1)
    aw = a * w
    e_aw = w.abs() * e_a + a.abs() * e_w + EPS * aw.abs() + TINY
    P = _prefix(aw)
    e_P = _prefix(e_aw) + D * EPS * _prefix(aw.abs())
    g_s = -tau * P
    e = tau * e_P + EPS * tau * P.abs() + TINY
    dead = (g == 0).all(-1).unsqueeze(0).expand_as(e)
    e = torch.where(dead, torch.zeros_like(e), e)
    return dict(g_s=g_s, e_g_s=e, aw=aw)


def view(st, d, q, g, tau, kappa):
    """``ray`` and ``absorb`` of one view from its view_ref.Stencil: d [D,H,W], q [D,H,W,C], g [H,W,C] (float64) ->
    (ray dict, absorb dict, s, es)"""
    s, es = st.sample(d)
    r = ray(s, es, tau, kappa)
    QS = [st.sample(q[..., c]) for c in range(q.shape[-1])]
    ab = absorb(r["w"], r["e_w"], torch.stack([x[0] for x in QS], -1), torch.stack([x[1] for x in QS], -1), g, tau)
    return r, ab, s, es


# ---- the whole model in torch float64 (differentiable in d and in q) -------------------------------------------------

def tau_of(cfg):
    return LR.tau_of(cfg)


def kappa_of(cfg):
    """the float32 value the kernels receive"""
    return float(np.float32(cfg.get("colour_exposure", 1.0)))


def weights(d, R, tau, kappa):
    """d [D,H,W] float64, R [V,3,3] -> (w [V,D,H,W], grey [V,H,W], S [V,D,H,W] the rotated samples)"""
    S = CR.rotate(d.unsqueeze(-1), R)[..., 0]
    w = kappa * tau * torch.exp(-tau * torch.flip(torch.cumsum(torch.flip(S, [1]), 1), [1]))
    return w, (w * S).sum(1), S


def batch_loss(d, q, cfg, R, weights_, style_feats):
    """the loss of ONE view batch R [v,3,3] of the emission q [D,H,W,3] seen through the grey volume d; the style mask is
    clip(grey, 0, 1)"""
    w, grey, _ = weights(d, R, tau_of(cfg), kappa_of(cfg))
    img = torch.clamp(CR.image(q, R, w), 0, 1)
    return CR.image_loss(img, torch.clamp(grey, 0, 1).unsqueeze(-1), cfg, weights_, style_feats)


# ---- grid_variable 'c' ------------------------------------------------------------------------------------------------

def grid_loss_and_grad(d, c, cfg, rot_mats, weights_, style_feats):
    """(loss, d loss / d c [D,H,W,3]) of one frame by autograd, float64"""
    e = GR.grey(d, cfg["k"])
    c64 = torch.as_tensor(np.asarray(c, np.float64)).clone().requires_grad_()
    R = torch.as_tensor(np.asarray(rot_mats, np.float32)).double()
    l = sum(batch_loss(e, GR.emission(c64, e), cfg, Rb, weights_, style_feats) for Rb in LR._view_batches(cfg, R))
    (g,) = torch.autograd.grad(l, c64)
    return float(l.detach()), g


def grid_sequence_run(cfg, d_frames, u_frames, weights_, style_feats, rot_mats, c_init):
    """colour_liquid_ref.grid_sequence_run around this module's frame loss (that loop calls its module's by name)"""
    F_, interp = cfg["num_frames"], cfg.get("interp", 1)
    keys = list(range(0, F_, interp))
    u = torch.as_tensor(np.asarray(u_frames, np.float64)) if u_frames is not None else None
    g_opt = {t: torch.as_tensor(np.asarray(c_init[t], np.float64)) for t in keys}
    Wm = O.temporal_filter_matrix(len(keys), cfg["window_sigma"]) if (cfg["window_sigma"] > 0 and F_ > 1) else None
    opt_, hist = {}, []
    for _ in range(cfg["iter"]):
        upd, h = {}, []
        for t in keys:
            l, g = grid_loss_and_grad(d_frames[t], g_opt[t], cfg, rot_mats, weights_, style_feats)
            opt = opt_.setdefault(t // cfg["frames_per_opt"], O.TFAdam())
            upd[t] = torch.nan_to_num(opt.step(g_opt[t].clone(), g, cfg["lr"])) - g_opt[t]
            h.append(l)
        hist.append(h)
        for j, t in enumerate(keys):
            if Wm is None:
                g_opt[t] = g_opt[t] + upd[t]
                continue
            acc = torch.zeros_like(upd[t])
            for jj, s in enumerate(keys):
                if Wm[j, jj] != 0.0:
                    acc = acc + float(Wm[j, jj]) * O.transport(upd[s][None], u, s, t,
                                                               recursive=cfg.get("transport_recursive", True))[0]
            g_opt[t] = g_opt[t] + acc
    return hist, g_opt


# ---- target_field 'c' and 'pc' ----------------------------------------------------------------------------------------

def particle_frame_loss(p, r, c, cfg, res, R, weights_, style_feats):
    """one frame's loss of the colours c [N,3] through ONE view batch R [v,3,3] (the smoothed grey volume is a constant)"""
    return batch_loss(CR.grey_volume(p, cfg, res), CR.colour_volume(p, r, c, cfg, res), cfg, R, weights_, style_feats)


def joint_frame_loss(p, r, v, c, cfg, res, R, weights_, style_feats, absorbing=True):
    """absorb_ref.joint_frame_loss with the fixed-exposure image over black, no mask.  ``absorbing=False`` detaches the
    absorbing volume (what a gradient that left the new path out would see)"""
    x = p + v
    d_raw = AR.raw_volume(x, cfg, res)
    e = O.smooth3d_relu(d_raw, cfg["k"])[0, ..., 0]
    if not absorbing:
        e = e.detach()
    q = CR.colour_volume(x, r, c, cfg, res)
    w, _, _ = weights(e, R, tau_of(cfg), kappa_of(cfg))
    img = torch.clamp(CR.image(q, R, w), 0, 1)
    assert not cfg.get("style_mask")
    return CR.image_loss(img, None, cfg, weights_, style_feats) + AR.pressure_loss(d_raw, cfg)


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

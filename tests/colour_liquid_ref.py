"""Float64 restatement of the liquid colour render (include/nfs_liquid.h, engine.ColourRenderLoss(render="liquid")) -- the
ray weights w, the ray's transmittance t, the image J over a background and the frame losses of both colour stylizers --
with per-element bounds on what a float32 kernel may differ from it by, in tests/view_ref.py's style and on its constants.

The model, rays along D, the far end z = D - 1 first, S = rotate(d, R_v):
    B[z] = sum_{z' > z} S[z']          w[z] = tau exp(-tau B[z]) phi(tau S[z]),  phi(x) = (1 - exp(-x)) / x,  phi(0) = 1
    t = exp(-tau sum_z S[z])           J = sum_z w[z] rotate(q, R_v)[z] + t bg;   the grey image is 1 - t
J is linear in q with the weights w, so the projection and its transpose are tests/colour_ref.py's (``CR.project``,
``CR.transpose``, ``CR.image``) and the grid loop tests/colour_grid_ref.py's, unchanged.

The bounds (``ray``), first-order sums of the float32 roundings a kernel can make, s the samples and es their own bound:
* the running sum.  B[z] is a sequential float32 sum of at most D samples: e_B = sum_{z' > z} es + D EPS sum_{z' > z} |s|
  (view_ref's e_raysum restricted to the samples in front).
* E = exp(-tau B) through exp2: view_ref's transmittance bound with ONE exponential, E (tau (e_B + 4 EPS sum |s|) +
  K_EXP EPS) -- the 4 EPS sum |s| covers the rounding of -tau log2(e) and of its product with B.  The hardware exp2
  returns no denormals: a result below the smallest normal float32, TINY = 2^-126, may come out as 0, so every exponential
  carries + TINY.
* phi.  K_PHI = 8: for x >= 2^-5 the kernel may take -expm1(-x) / x -- expm1 within 2 ulp (4 EPS), the quotient's rounding
  (EPS), and the rounding of x = tau s (EPS) which phi passes on with |x phi'(x) / phi(x)| < 1: 6 EPS; below 2^-5 a
  four-term alternating series whose truncation is below x^4 / 120 <= 2^-26.9 (0.13 EPS) and whose Horner steps round three
  times against values <= 1 (3 EPS) plus x's own rounding: under 5 EPS.  8 EPS covers either with slack.  phi passes the
  sample's error on by |d phi / d s| = tau |phi'| <= tau / 2 max(1, exp(-x)) (phi = int_0^1 exp(-x u) du).
* w = tau E phi: two more products (3 EPS w with slack) and the underflow of either: (tau phi + 1) TINY.
* t as E over the whole ray; the grey image 1 - t adds the subtraction's rounding of a value <= 1, EPS.
Nothing here is fitted to the kernel."""
import numpy as np
import torch

from oracle import nfs_oracle as O
from tests import colour_grid_ref as GR
from tests import colour_ref as CR
from tests import view_ref as VR

EPS = VR.EPS
K_PHI = 8
TINY = 2.0 ** -126


def phi(x):
    """(1 - exp(-x)) / x in float64 with the limit 1 at 0 (and at -0.0): below 1e-5 the series 1 - x/2 + x^2/6, whose
    truncation x^3 / 24 is under 5e-17"""
    small = x.abs() < 1e-5
    xs = torch.where(small, torch.ones_like(x), x)
    return torch.where(small, 1 - x / 2 + x * x / 6, -torch.expm1(-xs) / xs)


def ray(s, es, tau):
    """s [D,...] samples along axis 0 (float64), es their error bound -> dict w, e_w [D,...], t, e_t, grey, e_grey [...]"""
    D = s.shape[0]
    sa = s.abs()
    B = VR._suffix(s) - s
    Babs = VR._suffix(sa) - sa
    eB = VR._suffix(es) - es + D * EPS * Babs
    E = torch.exp(-tau * B)
    x = tau * s
    ph = phi(x)
    eE = E * (tau * (eB + 4 * EPS * Babs) + VR.K_EXP * EPS) + TINY
    ePh = K_PHI * EPS * ph + 0.5 * tau * torch.exp((-x).clamp(min=0)) * es
    w = tau * E * ph
    e_w = tau * (eE * ph + E * ePh) + 3 * EPS * w + (tau * ph + 1) * TINY
    S, Sabs = s.sum(0), sa.sum(0)
    eS = es.sum(0) + D * EPS * Sabs
    t = torch.exp(-tau * S)
    e_t = t * (tau * (eS + 4 * EPS * Sabs) + VR.K_EXP * EPS) + TINY
    return dict(w=w, e_w=e_w, t=t, e_t=e_t, grey=1 - t, e_grey=e_t + EPS)


# ---- the whole model in torch float64 (differentiable in q; d is a constant) ----------------------------------------

def weights(d, R, tau):
    """d [D,H,W] float64, R [V,3,3] -> (w [V,D,H,W], t [V,H,W], S [V,D,H,W] the rotated samples)"""
    S = CR.rotate(d.unsqueeze(-1), R)[..., 0]
    B = torch.flip(torch.cumsum(torch.flip(S, [1]), 1), [1]) - S
    return tau * torch.exp(-tau * B) * phi(tau * S), torch.exp(-tau * S.sum(1)), S


def image(q, R, w, t, bg):
    """J [V,H,W,C] = sum_z w rotate(q) + t bg"""
    bg = torch.as_tensor(np.asarray(bg, np.float64))
    return CR.image(q, R, w) + t.unsqueeze(-1) * bg


def tau_of(cfg):
    """the float32 value the kernels receive"""
    return float(np.float32(cfg["transmit"]))


def background_of(cfg):
    return [float(np.float32(x)) for x in cfg.get("colour_background", (1.0, 1.0, 1.0))]


def batch_loss(d, q, cfg, R, weights_, style_feats):
    """the loss of ONE view batch R [v,3,3] of the emission q [D,H,W,3] seen through the grey volume d; the style mask is
    the grey liquid image 1 - t"""
    w, t, _ = weights(d, R, tau_of(cfg))
    img = torch.clamp(image(q, R, w, t, background_of(cfg)), 0, 1)
    return CR.image_loss(img, (1 - t).unsqueeze(-1), cfg, weights_, style_feats)


def _view_batches(cfg, R):
    vb = max(int(cfg["v_batch"]), 1)
    vb = vb if (R.shape[0] > vb and R.shape[0] % vb == 0) else R.shape[0]
    return [R[lo:lo + vb] for lo in range(0, R.shape[0], vb)]


# ---- grid_variable 'c' (tests/colour_grid_ref.py with the liquid image) ----------------------------------------------

def grid_frame_loss(e, c, cfg, rot_mats, weights_, style_feats):
    R = torch.as_tensor(np.asarray(rot_mats, np.float32)).double()
    return sum(batch_loss(e, GR.emission(c, e), cfg, Rb, weights_, style_feats) for Rb in _view_batches(cfg, R))


def grid_loss_and_grad(d, c, cfg, rot_mats, weights_, style_feats):
    """(loss, d loss / d c [D,H,W,3]) of one frame by autograd, float64"""
    e = GR.grey(d, cfg["k"])
    c64 = torch.as_tensor(np.asarray(c, np.float64)).clone().requires_grad_()
    l = grid_frame_loss(e, c64, cfg, rot_mats, weights_, style_feats)
    (g,) = torch.autograd.grad(l, c64)
    return float(l.detach()), g


def grid_sequence_run(cfg, d_frames, u_frames, weights_, style_feats, rot_mats, c_init):
    """colour_grid_ref.sequence_run with the liquid frame loss (that loop calls its module's loss_and_grad by name, so
    it is restated around this module's): TF-Adam per key frame on the summed view losses, upd = nan_to_num(new) - old,
    the temporally filtered updates carried between frames by the oracle's transport"""
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


# ---- target_field 'c' (tests/colour_ref.py's frame with the liquid image) --------------------------------------------

def particle_frame_loss(p, r, c, cfg, res, R, weights_, style_feats, d=None):
    """one frame's loss of the colours c [N,3] through ONE view batch R [v,3,3]: clamp -> splat -> liquid image -> clamp ->
    loss network (d: the smoothed grey volume of the positions, a constant)"""
    if d is None:
        d = CR.grey_volume(p, cfg, res)
    return batch_loss(d, CR.colour_volume(p, r, c, cfg, res), cfg, R, weights_, style_feats)

"""Float64 restatement of the colour view path -- the ray weights w, the projection A(w, R) of a colour volume, its
transpose and the one-frame loss of a per-particle colour -- with per-element bounds on what a float32 kernel may differ
from it by, in tests/view_ref.py's style and on its constants.

The model (include/nfs_colour.h): a grey density d absorbs, a colour volume q emits,
    S_v = rotate(d, R_v);  T_v[z] = exp(-tau sum_{z' >= z} S_v[z']);  I_v = sum_z S_v T_v;  M_g = max of I over group g
    w = T_v / M_g(v);  J_v = sum_z w[v,z] rotate(q, R_v)[z]

Bounds are first-order sums of the roundings a kernel can make:
* w: the transmittance's bound of view_ref.ray (K_EXP and the running sum) over the maximum, plus the division's rounding
  and the share of the maximum's own error;
* J per ray and channel: sum_z |w| err_sample + |sample| err_w, plus D roundings of the accumulation (an fma per step and
  the running sum: 2 D EPS sum |w| |sample|);
* the transpose: view_ref's scatter bound at the sample gradient g w, whose own error is |g| err_w plus the product's
  rounding.
"""
import math

import numpy as np
import torch

from oracle import nfs_oracle as O
from tests import view_ref as VR

EPS = VR.EPS


def ray_weights(s, es, tau, m, em=0.0):
    """s [D,H,W] the rotated grey samples of one view (float64), es their error bound, m the group's maximum and em
    its error bound -> (w, e_w)"""
    r = VR.ray(s, es, tau)
    w = r["T"] / m
    return w, r["e_T"] / m + w * (em / m) + 2 * EPS * w


def project(st, q, w, e_w):
    """one view: st its view_ref.Stencil, q [D,H,W,C], w / e_w [D,H,W] -> (J [H,W,C], e_J)"""
    D = q.shape[0]
    J, eJ = [], []
    for c in range(q.shape[-1]):
        s, es = st.sample(q[..., c])
        J.append((w * s).sum(0))
        eJ.append((w.abs() * es + s.abs() * e_w).sum(0) + 2 * D * EPS * (w.abs() * s.abs()).sum(0))
    return torch.stack(J, -1), torch.stack(eJ, -1)


def project_all(R, q, w, e_w=None):
    """R [V,3,3], q [D,H,W,C], w [V,D,H,W] (float64) -> (J [V,H,W,C], e_J)"""
    out = [project(VR.Stencil(R[v], tuple(q.shape[:3])), q, w[v], torch.zeros_like(w[v]) if e_w is None else e_w[v])
           for v in range(R.shape[0])]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def transpose(R, g, w, e_w=None):
    """the adjoint of project_all at g [V,H,W,C]: per channel the summed view_ref scatter dict of the sample gradient
    g w (its own error: |g| e_w and one rounding of the product).  -> list of C dicts (ref, m1, dw, count)"""
    V = R.shape[0]
    shape = tuple(w.shape[1:])
    sts = [VR.Stencil(R[v], shape) for v in range(V)]
    out = []
    for c in range(g.shape[-1]):
        acc = None
        for v in range(V):
            G = w[v] * g[v, ..., c]
            eG = EPS * G.abs()
            if e_w is not None:
                eG = eG + g[v, ..., c].abs() * e_w[v]
            acc = VR.add_scatters(acc, sts[v].scatter(G, eG))
        out.append(acc)
    return out


def transpose_ref(R, g, w):
    return torch.stack([sc["ref"] for sc in transpose(R, g, w)], -1)


# ---- the whole model in torch float64 (differentiable in q; d is a constant) ----------------------------------------

def rotate(vol, R):
    """vol [D,H,W,C], R [V,3,3] -> [V,D,H,W,C] by the oracle's rotate (float64)"""
    return O.rotate(vol.unsqueeze(0), R.to(vol.dtype))


def weights(d, R, tau, v_batch):
    """d [D,H,W] float64, R [V,3,3] -> (w [V,D,H,W], I [V,H,W] the grey render, M [V] each view's group maximum); groups
    are max(V // v_batch, 1) runs of consecutive views, as nfs_maxnorm_fwd's"""
    S = rotate(d.unsqueeze(-1), R)[..., 0]
    T = torch.exp(-tau * torch.flip(torch.cumsum(torch.flip(S, [1]), 1), [1]))
    I = (S * T).sum(1)
    V = R.shape[0]
    G = max(V // v_batch, 1)
    M = I.reshape(G, -1).amax(1).repeat_interleave(V // G)
    return T / M.reshape(V, 1, 1, 1), I, M


def image(q, R, w):
    """J [V,H,W,C] = sum_z w rotate(q)"""
    return (rotate(q, R) * w.unsqueeze(-1)).sum(1)


def colour_volume(p, r, c, cfg, res):
    """q [D,H,W,3] = p2g(p, pc=clip(c,0,1), pd=r, is_2d=False) (transform.py:1429-1441); p [N,3], r [N,1], c [N,3]"""
    return O.p2g(p.unsqueeze(0), cfg["domain"], res, cfg["radius"], cfg["rest_density"], cfg["nsize"],
                 pc=torch.clamp(c, 0, 1).unsqueeze(0), pd=r.unsqueeze(0), is_2d=False, clip=cfg["clip"],
                 support=cfg["support"])[0]


def grey_volume(p, cfg, res):
    """d [D,H,W] = smooth_relu(p2g(p) / rest_density, k): styler_3p's 'p' path at zero displacement"""
    d = O.p2g(p.unsqueeze(0), cfg["domain"], res, cfg["radius"], cfg["rest_density"], cfg["nsize"], is_2d=False,
              clip=cfg["clip"], support=cfg["support"]) / cfg["rest_density"]
    return O.smooth3d_relu(d, cfg["k"])[0, ..., 0].detach()


def image_loss(img, d_gray, cfg, weights_, style_feats):
    """the loss of a clipped colour image batch img [V,H,W,3]: style (masked by d_gray [V,H,W,1] with style_mask) + TV,
    as engine.ImageStyleLoss sums it over the batch"""
    d_img = O.plugin_to_loss_net(img, cfg.get("resize_scale", 1.0), is_color=True)
    feats = O.loss_net_features(d_img, weights_, O.last_layer(cfg["style_layer"], cfg), cfg)
    l, _ = O.style_loss(feats, style_feats, cfg["style_layer"], cfg["w_style_layer"], cfg["w_style"],
                        d_gray=d_gray if cfg.get("style_mask") else None)
    if cfg.get("w_tv", 0):
        l = l + O.tv_loss(d_img) * cfg["w_tv"]
    return l


def frame_loss(p, r, c, cfg, res, R, weights_, style_feats, d=None):
    """one frame's loss of the colours c [N,3] through the views R [V,3,3] (one view batch: ONE maximum group per
    v_batch views): clamp -> splat -> A(w, R) -> clamp -> loss network"""
    if d is None:
        d = grey_volume(p, cfg, res)
    w, I, M = weights(d, R, cfg["transmit"], cfg["v_batch"])
    d_gray = torch.clamp(I / M.reshape(-1, 1, 1), 0, 1).unsqueeze(-1)
    q = colour_volume(p, r, c, cfg, res)
    img = torch.clamp(image(q, R, w), 0, 1)
    return image_loss(img, d_gray, cfg, weights_, style_feats)


# ---- shared set-up of the colour tests -------------------------------------------------------------------------------

def _ry(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rz(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def views(device="cpu"):
    """identity, Ry(10) Rz(-5), Ry(45) Rz(20) and 1.4 I (every border sample clamped), as float32 values"""
    m = [np.eye(3), _ry(10) @ _rz(-5), _ry(45) @ _rz(20), 1.4 * np.eye(3)]
    return torch.tensor(np.asarray(m, np.float32), device=device)


SHAPES = [(3, 4, 5), (17, 6, 9), (16, 5, 70)]


def splat_cfg(res, k=0):
    return dict(domain=[float(v) for v in res], radius=0.5, rest_density=1000.0, nsize=1, clip=False, support=4, k=k)


def particles(n, seed, rest_density=1000.0):
    """n seeded particles in the unit cube (a margin off the faces), densities in [0.8, 1.2] rho0, colours in [0,1]"""
    rng = np.random.RandomState(seed)
    p = rng.uniform(0.08, 0.92, (n, 3))
    r = rng.uniform(0.8, 1.2, (n, 1)) * rest_density
    c = rng.uniform(0.0, 1.0, (n, 3))
    return (torch.tensor(p.astype(np.float32)).double(), torch.tensor(r.astype(np.float32)).double(),
            torch.tensor(c.astype(np.float32)).double())

"""NumPy / torch restatement of the 2-D grid stylizer (include/nfs_grid2d.h "stylising a 2-D grid", grid2d.py).

Fields: density d [H,W] float32; a velocity is [H,W,2] in nfs_advect2d_fwd's own units (component k moves along array axis
k, one cell along an axis of n nodes is 2/(n-1)).  The variables are the D = 1 restriction of the 3-D definitions with the
D component dropped; D_A is the forward difference along array axis A, the last slice replicated:

    'v'   vel [H,W,2]                                          itself
    's'   psi [H,W] (channel s2 of the 3-D stream function)    vel0 = -D_W psi, vel1 = D_H psi
    'p'   phi [H,W]                                            vel0 = D_H phi,  vel1 = D_W phi
    'sp'  a [H,W,2] = (psi, phi)                               each part formed as above, then added once

``velocity`` / ``velocity_T`` work in the dtype handed in: float32 in gives every difference rounded once and one sum, the
kernels' arithmetic bit for bit (the minus of 's' is the difference with its ends exchanged, not a negation: +0 where the
two samples are equal); float64 in gives the reference.  The differences are those of tests/potential_ref.py.

``sequence_run`` is the float64 reference loop of a 2-D sequence, from oracle pieces: advect2d / advect_maccormack ->
clip(., 0, 1) -> plugin_to_loss_net -> vgg19_features -> style_loss -> TFAdam per optimiser group -> the updates aligned
with ``transport2d`` (written from advect2d as oracle.transport is from advect) and temporal_filter_matrix."""
import numpy as np
import torch

from oracle import nfs_oracle as O
from tests import potential_ref as PR

KINDS = ("v", "s", "p", "sp")
AXIS_H, AXIS_W = 0, 1


def var_shape(kind, H, W):
    return {"v": (H, W, 2), "s": (H, W), "p": (H, W), "sp": (H, W, 2)}[kind]


def _stream(psi):
    return np.stack([PR.diff(-psi, AXIS_W), PR.diff(psi, AXIS_H)], axis=-1)


def _potential(phi):
    return np.stack([PR.diff(phi, AXIS_H), PR.diff(phi, AXIS_W)], axis=-1)


def velocity(kind, x):
    """the velocity [H,W,2] the variable stands for, in the dtype of ``x``"""
    if kind == "v":
        return x.copy()
    if kind == "s":
        return _stream(x)
    if kind == "p":
        return _potential(x)
    return _stream(x[..., 0]) + _potential(x[..., 1])


def velocity_T(kind, g, absolute=False):
    """the transpose of ``velocity`` applied to g [H,W,2], summed H then W: g_psi = D_H^T g1 - D_W^T g0, g_phi =
    D_H^T g0 + D_W^T g1.  ``absolute``: every coefficient +1 and |g| in place of g (A of the rounding bounds)"""
    if kind == "v":
        return np.abs(g) if absolute else g.copy()
    t = lambda k, ax: PR.diff_T(g[..., k], ax, absolute)
    gs = t(1, AXIS_H) + t(0, AXIS_W) if absolute else t(1, AXIS_H) - t(0, AXIS_W)
    gp = t(0, AXIS_H) + t(1, AXIS_W)
    return gs if kind == "s" else gp if kind == "p" else np.stack([gs, gp], axis=-1)


def _inner(v):
    H, W = v.shape[:2]
    return (slice(0, H - 2), slice(0, W - 2))


def divergence(vel):
    """D_H vel0 + D_W vel1 in float64 on the pixels with index <= n - 3 on both axes (no replicated slice within reach)"""
    v = np.asarray(vel, np.float64)
    if min(v.shape[:2]) < 3:
        return np.zeros((0,), np.float64)
    c = _inner(v)
    return PR.diff(v[..., 0], AXIS_H)[c] + PR.diff(v[..., 1], AXIS_W)[c]


def rotation(vel):
    """D_H vel1 - D_W vel0 in float64 on the same pixels"""
    v = np.asarray(vel, np.float64)
    if min(v.shape[:2]) < 3:
        return np.zeros((0,), np.float64)
    c = _inner(v)
    return PR.diff(v[..., 1], AXIS_H)[c] - PR.diff(v[..., 0], AXIS_W)[c]


def max_forward_difference(x):
    x = np.asarray(x, np.float64)
    return max(float(np.abs(PR.diff(x, ax)).max()) for ax in (AXIS_H, AXIS_W))


def divergence_bound(psi):
    """max |div| <= 2^-22 * M for a float32 stream velocity of psi, M the largest |forward difference of psi|: the
    divergence D_H vel0 + D_W vel1 at a pixel is (vel0[h+1,w] - vel0[h,w]) + (vel1[h,w+1] - vel1[h,w]), FOUR stored
    differences of psi (-D_W psi at two rows, D_H psi at two columns) that cancel exactly in exact arithmetic since forward
    differences commute; each was rounded once on storing, to within half an ulp of a value <= M, i.e. 2^-24 * M, and
    the 2-D components are single differences (no second rounding as in 3-D, where a component is a difference of two):
    4 * 2^-24 * M.  The divergence itself is evaluated in float64."""
    return 2.0 ** -22 * max_forward_difference(psi)


def rotation_bound(phi):
    """potential_ref.rotation_bound's 2^-22 * M: D_H vel1 - D_W vel0 is four stored differences of phi likewise"""
    return 2.0 ** -22 * max_forward_difference(phi)


def make_var(kind, H, W, cells, seed):
    """a smooth variable (Gaussian-filtered noise as in potential_ref) whose velocity peaks at ``cells`` cells; float32"""
    x = PR._noise((H, W), seed, channels=2 if kind in ("v", "sp") else None)
    if kind == "sp":
        cell = np.asarray([2.0 / (H - 1), 2.0 / (W - 1)])
        x[..., 0] /= np.abs(_stream(x[..., 0]) / cell).max()
        x[..., 1] /= np.abs(_potential(x[..., 1]) / cell).max()
    peak = float(np.abs(velocity(kind, x) / np.asarray([2.0 / (H - 1), 2.0 / (W - 1)])).max())
    return (x * (cells / peak)).astype(np.float32)


# ---- torch (differentiable) --------------------------------------------------------------------------------------------------
def _tdiff(a, axis):
    n = a.shape[axis]
    d = a.narrow(axis, 1, n - 1) - a.narrow(axis, 0, n - 1)
    return torch.cat([d, d.narrow(axis, n - 2, 1)], dim=axis)


def torch_velocity(kind, x):
    """``velocity`` on a torch tensor, differentiable"""
    if kind == "v":
        return x
    st = lambda psi: torch.stack([-_tdiff(psi, 1), _tdiff(psi, 0)], dim=-1)
    po = lambda phi: torch.stack([_tdiff(phi, 0), _tdiff(phi, 1)], dim=-1)
    if kind == "s":
        return st(x)
    if kind == "p":
        return po(x)
    return st(x[..., 0]) + po(x[..., 1])


def transport2d(g, v, a, b, recursive=True):
    """oracle.transport written from advect2d: move g [1,H,W,C] from frame a to frame b through v [F,H,W,2]"""
    if a < b:
        if recursive:
            for i in range(a, b):
                g = O.advect2d(g, v[i:i + 1])
        else:
            g = O.advect2d(g, v[a:a + 1] * (b - a))
    elif a > b:
        if recursive:
            for i in reversed(range(b, a)):
                g = O.advect2d(g, -v[i:i + 1])
        else:
            g = O.advect2d(g, -v[a - 1:a] * (a - b))
    return g


def advected(kind, d, var, adv_order=1):
    """d^ [1,H,W,1] of the chain: d [1,H,W,1], var in its own shape (torch)"""
    if kind == "d":
        return var.reshape(d.shape)
    vel = torch_velocity(kind, var)[None]
    return O.advect_maccormack(d, vel) if adv_order == 2 else O.advect2d(d, vel)


def frame_loss(kind, d, var, cfg, weights, style_feats):
    """(loss, img) of one frame: advect -> clip -> loss network -> style loss"""
    img = torch.clamp(advected(kind, d, var, cfg.get("adv_order", 1)), 0.0, 1.0)
    d_img = O.plugin_to_loss_net(img, cfg.get("resize_scale", 1.0))
    feats = O.vgg19_features(d_img, weights, cfg["upto"])
    loss, _ = O.style_loss(feats, style_feats, cfg["style_layer"], cfg["w_style_layer"], cfg.get("w_style", 1.0))
    return loss, img


def style_features(style_img, cfg, weights, dtype=torch.float64):
    return O.style_target_features(torch.tensor(np.asarray(style_img), dtype=dtype)[None], weights, cfg["style_layer"],
                                   upto=cfg["upto"])


def loss_and_gradient(kind, d, var, cfg, weights, style_feats, dtype=torch.float64):
    """float64 autograd of the chain at one frame: (loss, dL/dvar) from numpy d [H,W] and var"""
    dt = torch.tensor(np.asarray(d), dtype=dtype)[None, ..., None]
    x = torch.tensor(np.asarray(var), dtype=dtype).requires_grad_()
    loss, _ = frame_loss(kind, dt, x, cfg, weights, style_feats)
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g.numpy()


def sequence_run(cfg, d_frames, u_frames, weights, style_img, init=None, dtype=torch.float64):
    """The reference loop of a 2-D sequence (the loop of oracle.grid_sequence_run on the 2-D chain).  cfg: grid_variable,
    num_frames, interp, frames_per_opt, window_sigma, transport_recursive, iter, lr, adv_order, style_layer,
    w_style_layer, w_style, upto, resize_scale.  d_frames [F][H,W], u_frames [F][H,W,2], init [F] variables or None.
    Returns (loss history [iter][key frame], variables per frame, velocities per frame (None for 'd'), clipped images per
    frame [H,W,1])"""
    F_, interp, kind = cfg["num_frames"], cfg.get("interp", 1), cfg.get("grid_variable", "v")
    d = [torch.tensor(np.asarray(x), dtype=dtype)[None, ..., None] for x in d_frames]
    u = torch.tensor(np.asarray(u_frames), dtype=dtype) if u_frames is not None else None
    sfe = style_features(style_img, cfg, weights, dtype)
    H, W = d[0].shape[1:3]

    def initial(t):
        if kind == "d":
            return d[t][0].clone()
        if init is not None:
            return torch.tensor(np.asarray(init[t]), dtype=dtype)
        return torch.zeros(var_shape(kind, H, W), dtype=dtype)

    keys = list(range(0, F_, interp))
    g_opt = {t: initial(t) for t in keys}
    Wm = O.temporal_filter_matrix(len(keys), cfg["window_sigma"]) if (cfg["window_sigma"] > 0 and F_ > 1) else None
    opt_, hist = {}, []
    for _ in range(cfg["iter"]):
        upd, h = {}, []
        for t in keys:
            var = g_opt[t].clone().requires_grad_()
            opt = opt_.setdefault(t // cfg["frames_per_opt"], O.TFAdam())
            loss, _ = frame_loss(kind, d[t], var, cfg, weights, sfe)
            (g,) = torch.autograd.grad(loss, var)
            dl = torch.nan_to_num(opt.step(var.detach(), g, cfg["lr"])) - g_opt[t]
            if kind == "d":
                dl = dl * d[t][0]
            upd[t] = dl
            h.append(float(loss.detach()))
        hist.append(h)
        for j, t in enumerate(keys):
            if Wm is None:
                g_opt[t] = g_opt[t] + upd[t]
                continue
            acc = torch.zeros_like(upd[t])
            for jj, s in enumerate(keys):
                if Wm[j, jj] != 0.0:
                    field = upd[s].reshape(1, H, W, -1)
                    acc = acc + float(Wm[j, jj]) * transport2d(field, u, s, t, cfg.get("transport_recursive", True)
                                                               ).reshape(upd[t].shape)
            g_opt[t] = g_opt[t] + acc
    full = dict(g_opt)
    if interp > 1:
        w = np.linspace(0, 1, interp + 1)
        for t in range(0, F_ - 1, interp):
            for i in range(1, interp):
                if t + interp < F_:
                    full[t + i] = full[t] * float(1 - w[i]) + full[t + interp] * float(w[i])
    outs, vels, imgs = [], [], []
    for t in range(F_):
        var = full[t] if t in full else initial(t)
        imgs.append(torch.clamp(advected(kind, d[t], var, cfg.get("adv_order", 1)), 0.0, 1.0)[0].numpy())
        outs.append(var.numpy())
        vels.append(None if kind == "d" else torch_velocity(kind, var).numpy())
    return hist, outs, vels, imgs

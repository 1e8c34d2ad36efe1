"""Float64 restatement of the colour grid path (``grid_variable 'c'`` of styler_grid, engine.ColourGridStylizer), composed
from what exists: the oracle's smoothing, TF-Adam, transport and temporal filter, and the colour view model of
tests/colour_ref.py.

    e = smooth3d_relu(d, k)                            absorbs and emits; a constant of the step
    w, I, M = CR.weights(e, R, transmit, v_batch)      d_gray = clip(I / M, 0, 1)
    q = clip(c, 0, 1) * e                              (torch.clamp passes the gradient where 0 <= c <= 1, ends included)
    img = clip(CR.image(q, R, w), 0, 1)  ->  CR.image_loss

one loss per view batch of ``v_batch`` views (one maximum each), summed.  ``sequence_run`` is the loop of
oracle.grid_sequence_run with the emission in place of the advect and no mask on the update.

Also the two emission formulas in float32 numpy, element by element (``emission_fwd_np`` / ``emission_bwd_np``), and the
checks that hold any restatement of them to float64 (``fwd_agrees`` / ``bwd_agrees``): a product of two float32 values is
exact in float64, so the float32 result IS the float64 one rounded once -- equality, no tolerance."""
import numpy as np
import torch

from oracle import nfs_oracle as O
from tests import colour_ref as CR


def grey(d, k):
    """d [D,H,W] -> e = smooth3d_relu(d, k) [D,H,W] (float64, detached)"""
    d = torch.as_tensor(np.asarray(d, np.float64))
    return O.smooth3d_relu(d[None, ..., None], k)[0, ..., 0].detach()


def emission(c, e):
    return torch.clamp(c, 0, 1) * e.unsqueeze(-1)


def batch_loss(e, c, cfg, R, weights_, style_feats):
    """the loss of ONE view batch R [v,3,3] (one maximum group per cfg['v_batch'] views)"""
    w, I, M = CR.weights(e, R, cfg["transmit"], cfg["v_batch"])
    d_gray = torch.clamp(I / M.reshape(-1, 1, 1), 0, 1).unsqueeze(-1)
    img = torch.clamp(CR.image(emission(c, e), R, w), 0, 1)
    return CR.image_loss(img, d_gray, cfg, weights_, style_feats)


def frame_loss(e, c, cfg, rot_mats, weights_, style_feats):
    """the summed loss of all views, taken cfg['v_batch'] at a time as the engine's loss-net batches are"""
    R = torch.as_tensor(np.asarray(rot_mats, np.float32)).double()
    vb = max(int(cfg["v_batch"]), 1)
    vb = vb if (R.shape[0] > vb and R.shape[0] % vb == 0) else R.shape[0]
    total = 0.0
    for lo in range(0, R.shape[0], vb):
        total = total + batch_loss(e, c, cfg, R[lo:lo + vb], weights_, style_feats)
    return total


def loss_and_grad(d, c, cfg, rot_mats, weights_, style_feats):
    """(loss, d loss / d c [D,H,W,3]) of one frame by autograd, float64"""
    e = grey(d, cfg["k"])
    c64 = torch.as_tensor(np.asarray(c, np.float64)).clone().requires_grad_()
    l = frame_loss(e, c64, cfg, rot_mats, weights_, style_feats)
    (g,) = torch.autograd.grad(l, c64)
    return float(l.detach()), g


def sequence_run(cfg, d_frames, u_frames, weights_, style_feats, rot_mats, c_init):
    """the frame loop: per key frame one TF-Adam step (one state per t // frames_per_opt) on the summed view losses,
    upd = nan_to_num(new) - old (no mask), the temporally filtered updates carried between frames by the oracle's
    transport.  -> (loss history [iter][key frame], {key frame: variable [D,H,W,3]})"""
    F_, interp = cfg["num_frames"], cfg.get("interp", 1)
    keys = list(range(0, F_, interp))
    u = torch.as_tensor(np.asarray(u_frames, np.float64)) if u_frames is not None else None
    g_opt = {t: torch.as_tensor(np.asarray(c_init[t], np.float64)) for t in keys}
    Wm = O.temporal_filter_matrix(len(keys), cfg["window_sigma"]) if (cfg["window_sigma"] > 0 and F_ > 1) else None
    opt_, hist = {}, []
    for _ in range(cfg["iter"]):
        upd, h = {}, []
        for t in keys:
            l, g = loss_and_grad(d_frames[t], g_opt[t], cfg, rot_mats, weights_, style_feats)
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


# ---- the two emission formulas element by element, float32 -----------------------------------------------------------

def emission_fwd_np(c, e):
    """c [n,C], e [n] float32 -> q[i,ch] = min(max(c, 0), 1) * e[i]; a NaN colour clamps to 0 (fmaxf(NaN, 0) = 0)"""
    c, e = np.asarray(c, np.float32), np.asarray(e, np.float32)
    cl = np.where(np.isnan(c), np.float32(0), np.minimum(np.maximum(c, np.float32(0)), np.float32(1)))
    return (cl * e[:, None]).astype(np.float32)


def emission_bwd_np(g_q, c, e):
    """g_c[i,ch] = g_q[i,ch] * e[i] where 0 <= c[i,ch] <= 1 (ends included; a NaN colour is outside), else +0"""
    g_q, c, e = np.asarray(g_q, np.float32), np.asarray(c, np.float32), np.asarray(e, np.float32)
    with np.errstate(invalid="ignore"):
        inside = (c >= 0) & (c <= 1)
    return np.where(inside, g_q * e[:, None], np.float32(0)).astype(np.float32)


def check_inputs(n=105, C=3, seed=3):
    """colours with exact 0, exact 1, -0.0, values outside on both sides and a NaN; e with +0.0, -0.0 and positive values;
    every special colour meets a positive e and a non-zero gradient"""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-0.3, 1.3, (n, C)).astype(np.float32)
    e = rng.uniform(0.1, 2.0, n).astype(np.float32)
    g = rng.uniform(0.5, 1.5, (n, C)).astype(np.float32) * np.where(rng.rand(n, C) < 0.5, -1, 1).astype(np.float32)
    special = [0.0, 1.0, -0.0, -0.25, 1.25, np.nan, 0.5]
    for i, s in enumerate(special):
        c[i, i % C] = s
    e[len(special)] = 0.0
    e[len(special) + 1] = -0.0
    c[len(special), 0], c[len(special) + 1, 0] = 0.5, 1.5
    return c, e, g


def fwd_agrees(fn, c, e):
    """does ``fn(c, e)`` give the float64 emission rounded once in every element?  (compared as values, zero of either
    sign alike: what max(-0.0, +0.0) returns is the implementation's choice)"""
    c64 = torch.tensor(np.nan_to_num(c.astype(np.float64), nan=0.0))       # (a NaN colour clamps to 0)
    ref = emission(c64, torch.tensor(e.astype(np.float64))).numpy().astype(np.float32)
    got = np.asarray(fn(c, e), np.float32)
    return got.shape == ref.shape and np.array_equal(got, ref)


def bwd_agrees(fn, g, c, e):
    """does ``fn(g, c, e)`` give the float64 autograd gradient of sum(g * emission(c, e)) rounded once?  (compared as
    values, zero of either sign alike: autograd's zero carries no sign convention)"""
    c64 = torch.tensor(np.nan_to_num(c.astype(np.float64), nan=-1.0), requires_grad=True)    # (a NaN colour: outside)
    (ref,) = torch.autograd.grad((emission(c64, torch.tensor(e.astype(np.float64))) * torch.tensor(g.astype(np.float64))).sum(),
                                 c64)
    ref = ref.numpy().astype(np.float32)
    got = np.asarray(fn(g, c, e), np.float32)
    return got.shape == ref.shape and np.array_equal(got, ref)

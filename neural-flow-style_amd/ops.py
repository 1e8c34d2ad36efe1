"""Tensor-level bindings of the C ABI (include/nfs_hip.h).

PyTorch is plumbing only: it owns device memory and the stream.  Every function
takes contiguous float32 CUDA tensors, passes raw pointers + the current stream
through ctypes and returns freshly allocated (or caller-supplied) outputs.
There is no CPU path: a non-CUDA tensor raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import SplatCfg


def _ptr(t):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("expected a contiguous float32 CUDA tensor, got %s %s contiguous=%s"
                         % (t.device, t.dtype, t.is_contiguous()))
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device=None):
    """the current HIP stream's handle (the raw getter is ~20x cheaper than building a torch.cuda.Stream object: the
    one-view and small-grid steps are bound by what the host needs per launch)"""
    if _raw_stream is not None:
        idx = torch.cuda.current_device() if device is None or device.index is None else device.index
        return _raw_stream(idx)
    return torch.cuda.current_stream(device).cuda_stream


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _zeros(shape, like):
    return torch.zeros(shape, dtype=torch.float32, device=like.device)


# ---- A2 / A3 / A11 ------------------------------------------------------------------

def warp3d_fwd(imgs, coords):
    B, X, Y, Z, Cn = imgs.shape
    out = _empty(imgs.shape, imgs)
    _lib.call("nfs_warp3d_fwd", _ptr(imgs), _ptr(coords), _ptr(out), B, X, Y, Z, Cn, _stream())
    return out


def warp3d_bwd(imgs, coords, g_out, need_coords=True):
    B, X, Y, Z, Cn = imgs.shape
    g_imgs = _zeros(imgs.shape, imgs)
    g_coords = _empty(coords.shape, imgs) if need_coords else None
    _lib.call("nfs_warp3d_bwd", _ptr(imgs), _ptr(coords), _ptr(g_out), _ptr(g_imgs), _ptr(g_coords),
              B, X, Y, Z, Cn, _stream())
    return g_imgs, g_coords


def rotate_fwd(d, rot):
    """d [D,H,W,C], rot [V,3,3] -> [V,D,H,W,C]"""
    D, H, W, Cn = d.shape
    V = rot.shape[0]
    out = _empty((V, D, H, W, Cn), d)
    _lib.call("nfs_rotate_fwd", _ptr(d), _ptr(rot), _ptr(out), V, D, H, W, Cn, _stream())
    return out


_workspaces = {}


def workspace(device):
    """small per-device scratch (64 floats) for entry points that need a device-side scalar"""
    if torch.cuda.is_current_stream_capturing():
        # a capture owns what it allocates (its private pool keeps it for the replays); a buffer cached here would be
        # shared by every later capture on the same capture stream, whatever became of the graph that allocated it
        return torch.zeros(64, dtype=torch.float32, device=device)
    key = (device.type, device.index, _stream(device))   # one per stream
    if key not in _workspaces:
        _workspaces[key] = torch.zeros(64, dtype=torch.float32, device=device)
    return _workspaces[key]


def rotate_bwd(g_out, rot, g_d_acc=None, tiled=True, g_max=None, overwrite=False):
    """g_max: optional device scalar max|g_out| (render_bwd(..., want_max=True)): skips the pre-pass.
    overwrite (tiled adjoint, C == 1): g_d_acc is written, not accumulated into (no zero fill needed)"""
    V, D, H, W, Cn = g_out.shape
    if tiled and Cn == 1:
        # the scratch word holds the pre-pass maximum: with g_max given it is not touched (inside a capture workspace() is a
        # fresh zero-filled tensor, i.e. a fill launch in every replay: not needed here)
        ws = _empty((64,), g_out) if (g_max is not None and torch.cuda.is_current_stream_capturing()) else workspace(g_out.device)
    else:
        ws = None
    if g_d_acc is None:
        overwrite = ws is not None                 # a fresh buffer: let the kernel write every voxel
        g_d_acc = _empty((D, H, W, Cn), g_out) if overwrite else _zeros((D, H, W, Cn), g_out)
    _lib.call("nfs_rotate_bwd", _ptr(g_out), _ptr(rot), _ptr(g_d_acc), V, D, H, W, Cn, _ptr(ws), _ptr(g_max),
              int(bool(overwrite)), _stream())
    return g_d_acc


def live_mask(D, H, W, like):
    """buffer for the live mask of a [D,H,W] volume: nfs_live_mask_words 64-bit words, bit = linear voxel index, held as
    float32 storage like every buffer that crosses the C-ABI here (``.view(torch.int64)`` to look at the words)"""
    return torch.zeros(2 * int(_lib.lib().nfs_live_mask_words(D, H, W)), dtype=torch.float32, device=like.device)


def advect_fwd(d, vel, out=None, live=None):
    """``live`` (optional, ``live_mask``; scalar field only): also write the mask of the voxels whose back-traced density
    corners differ, i.e. where the velocity gradient can be non-zero (see rotate_bwd_coef)"""
    D, H, W, Cn = d.shape
    if out is None:
        out = _empty(d.shape, d)
    if live is not None:
        assert Cn == 1
        _lib.call("nfs_advect_fwd_live", _ptr(d), _ptr(vel), _ptr(out), _ptr(live), D, H, W, _stream())
        _written(live)
    else:
        _lib.call("nfs_advect_fwd", _ptr(d), _ptr(vel), _ptr(out), D, H, W, Cn, _stream())
    return out


def advect_bwd(d, vel, g_out, need_d=True, need_vel=True, g_d_acc=None, g_vel=None):
    D, H, W, Cn = d.shape
    if need_d and g_d_acc is None:
        g_d_acc = _zeros(d.shape, d)
    if need_vel and g_vel is None:
        g_vel = _empty(vel.shape, d)
    _lib.call("nfs_advect_bwd", _ptr(d), _ptr(vel), _ptr(g_out), _ptr(g_d_acc if need_d else None),
              _ptr(g_vel if need_vel else None), D, H, W, Cn, _stream())
    return g_d_acc, g_vel


def advect_bwd_adam(d, vel, g_out, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, adv_next=None, live_next=None, ever=None):
    """velocity gradient of advect consumed on the spot by the TF-Adam update of vel (vel, m, v in place);
    ``adv_next`` [D,H,W] (optional): advect(d, updated vel), the next iteration's forward sample, written in the same pass;
    ``live_next`` (optional, with adv_next): the live mask of that sample (``advect_fwd``);
    ``ever`` (optional, with live_next, which must then hold the CURRENT mask on entry): the OR of every mask since m and v
    were zeroed -- waves of voxels that never were live are left out altogether (ApplyAdam is an exact no-op there)"""
    D, H, W, Cn = d.shape
    assert Cn == 1
    # each optional buffer that is present (in this order; one that is absent ends the list) adds its pointer after v and
    # its suffix to the entry point's name
    name, extra = "nfs_advect_bwd_adam", []
    for suffix, t in (("_fwd", adv_next), ("_live", live_next), ("_ever", ever)):
        if t is None:
            break
        name += suffix
        extra.append(t)
    if extra:
        assert adv_next.is_contiguous() and adv_next.numel() == D * H * W
    if len(extra) == 3:
        assert ever.numel() == live_next.numel()
    _lib.call(name, _ptr(d), _ptr(vel), _ptr(g_out), _ptr(m), _ptr(v), *map(_ptr, extra), D, H, W, float(lr_t),
              float(beta1), float(beta2), float(eps), _stream())
    _written(*extra[1:])
    _written(vel, m, v, adv_next)


def advect_fwd_slab(d, vel_slab, z0, out=None):
    """planes [z0, z0 + nz) of advect(d, vel): d the WHOLE density [D,H,W], vel_slab [nz,H,W,3] -> [nz,H,W]"""
    D, H, W = d.shape
    nz = vel_slab.shape[0]
    if out is None:
        out = _empty((nz, H, W), d)
    _lib.call("nfs_advect_fwd_slab", _ptr(d), _ptr(vel_slab), _ptr(out), D, H, W, int(z0), nz, _stream())
    return out


def advect_bwd_adam_slab(d, vel_slab, g_slab, m_slab, v_slab, z0, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, adv_next=None):
    """advect_bwd_adam on the planes [z0, z0 + nz) only (vel_slab, m_slab, v_slab [nz,H,W,3] in place, g_slab [nz,H,W]);
    d is the whole density [D,H,W]; ``adv_next`` [nz,H,W] (optional) as in advect_bwd_adam"""
    D, H, W = d.shape
    nz = vel_slab.shape[0]
    extra = [] if adv_next is None else [adv_next]
    if extra:
        assert adv_next.is_contiguous() and adv_next.numel() == nz * H * W
    _lib.call("nfs_advect_bwd_adam_fwd_slab" if extra else "nfs_advect_bwd_adam_slab", _ptr(d), _ptr(vel_slab), _ptr(g_slab),
              _ptr(m_slab), _ptr(v_slab), *map(_ptr, extra), D, H, W, int(z0), nz, float(lr_t), float(beta1), float(beta2),
              float(eps), _stream())
    _written(vel_slab, m_slab, v_slab, adv_next)


def warp2d_fwd(imgs, coords, out=None):
    """imgs [B,X,Y,C], coords [B,2,X,Y] -> [B,X,Y,C]  (transform.py:206-236, 280-341)"""
    B, X, Y, Cn = imgs.shape
    if out is None:
        out = _empty(imgs.shape, imgs)
    _lib.call("nfs_warp2d_fwd", _ptr(imgs), _ptr(coords), _ptr(out), B, X, Y, Cn, _stream())
    return out


def warp2d_bwd(imgs, coords, g_out, need_imgs=True, need_coords=True, out_coords=None):
    B, X, Y, Cn = imgs.shape
    g_imgs = _zeros(imgs.shape, imgs) if need_imgs else None
    g_coords = (_empty(coords.shape, imgs) if out_coords is None else out_coords) if need_coords else None
    _lib.call("nfs_warp2d_bwd", _ptr(imgs), _ptr(coords), _ptr(g_out), _ptr(g_imgs), _ptr(g_coords), B, X, Y, Cn,
              _stream())
    return g_imgs, g_coords


def advect2d_fwd(d, vel):
    """d [H,W,C], vel [H,W,2] -> [H,W,C]  (transform.py:583-588)"""
    H, W, Cn = d.shape
    out = _empty(d.shape, d)
    _lib.call("nfs_advect2d_fwd", _ptr(d), _ptr(vel), _ptr(out), H, W, Cn, _stream())
    return out


def advect2d_bwd(d, vel, g_out, need_d=True, need_vel=True):
    H, W, Cn = d.shape
    g_d = _zeros(d.shape, d) if need_d else None
    g_vel = _empty(vel.shape, d) if need_vel else None
    _lib.call("nfs_advect2d_bwd", _ptr(d), _ptr(vel), _ptr(g_out), _ptr(g_d), _ptr(g_vel), H, W, Cn, _stream())
    return g_d, g_vel


def maccormack_mask(shape, like):
    """buffer for the limiter's keep mask of a field of ``shape`` = [D,H,W,C] or [H,W,C]: nfs_maccormack_mask_words 64-bit
    words, bit e = element e of the advected field kept its first-order value; float32 storage like ``live_mask``"""
    D, H, W, Cn = (1,) * (4 - len(shape)) + tuple(shape)
    return torch.zeros(2 * int(_lib.lib().nfs_maccormack_mask_words(D, H, W, Cn)), dtype=torch.float32, device=like.device)


def advect_maccormack(d, vel, keep=None, d_fwd=None):
    """order-2 (MacCormack) advection with the extrema limiter (transform.py:570-582, 590-607 as intended);
    d [D,H,W,C] + vel [D,H,W,3], or d [H,W,C] + vel [H,W,2].  ``keep`` (optional, ``maccormack_mask``): also write the
    limiter's decisions; ``d_fwd`` (optional, shaped like d): receives the first-order sample the scheme starts from --
    the two things ``advect_maccormack_bwd`` differentiates by.  The result is the same bits with and without them."""
    nd = vel.shape[-1]
    if d_fwd is not None:
        assert d_fwd.shape == d.shape and d_fwd.is_contiguous()
    if nd == 3:
        D, H, W, Cn = d.shape
        d_fwd = advect_fwd(d, vel, out=d_fwd)
    else:
        (H, W, Cn), D = d.shape, 1
        if d_fwd is None:
            d_fwd = advect2d_fwd(d, vel)
        else:
            _lib.call("nfs_advect2d_fwd", _ptr(d), _ptr(vel), _ptr(d_fwd), H, W, Cn, _stream())
    out = _empty(d.shape, d)
    if keep is None:
        _lib.call("nfs_advect_maccormack", _ptr(d), _ptr(vel), _ptr(d_fwd), _ptr(out), D, H, W, Cn, nd, _stream())
    else:
        assert keep.numel() == 2 * int(_lib.lib().nfs_maccormack_mask_words(D, H, W, Cn))
        _lib.call("nfs_advect_maccormack_keep", _ptr(d), _ptr(vel), _ptr(d_fwd), _ptr(out), _ptr(keep), D, H, W, Cn, nd,
                  _stream())
        _written(keep)
    return out


def advect_maccormack_bwd(d, vel, d_fwd, keep, g_out, need_d=True, need_vel=True, g_d_acc=None, g_vel=None):
    """adjoint of ``advect_maccormack`` on the forward's own ``d_fwd`` and ``keep``: (g_d, g_vel) in the style of
    ``advect_bwd`` (g_d_acc is accumulated into, g_vel overwritten).  g_vel is bit-identical from call to call and with
    ``need_d`` on or off (fixed-point sums; include/nfs_hip.h)."""
    nd = vel.shape[-1]
    if nd == 3:
        D, H, W, Cn = d.shape
    else:
        (H, W, Cn), D = d.shape, 1
    if need_d and g_d_acc is None:
        g_d_acc = _zeros(d.shape, d)
    if need_vel and g_vel is None:
        g_vel = _empty(vel.shape, d)
    nws = int(_lib.lib().nfs_advect_maccormack_bwd_workspace_floats(D, H, W, Cn, nd))
    if nws < 0:
        raise ValueError("advect_maccormack_bwd: unsupported shape %s / %s" % (tuple(d.shape), tuple(vel.shape)))
    ws = _empty((nws,), d)
    _lib.call("nfs_advect_maccormack_bwd", _ptr(d), _ptr(vel), _ptr(d_fwd), _ptr(keep), _ptr(g_out),
              _ptr(g_d_acc if need_d else None), _ptr(g_vel if need_vel else None), _ptr(ws), nws, D, H, W, Cn, nd,
              _stream())
    return (g_d_acc if need_d else None), (g_vel if need_vel else None)


def curl_fwd(s):
    """s [H,W] -> [H,W,2] or s [D,H,W,3] -> [D,H,W,3]  (transform.py:517-555)"""
    if s.dim() == 2:
        (H, W), D, nd = s.shape, 1, 2
        out = _empty((H, W, 2), s)
    else:
        (D, H, W, _), nd = s.shape, 3
        out = _empty(s.shape, s)
    _lib.call("nfs_curl_fwd", _ptr(s), _ptr(out), D, H, W, nd, _stream())
    return out


def curl_bwd(g_out):
    if g_out.shape[-1] == 2:
        (H, W, _), D, nd = g_out.shape, 1, 2
        g_s = _empty((H, W), g_out)
    else:
        (D, H, W, _), nd = g_out.shape, 3
        g_s = _empty(g_out.shape, g_out)
    _lib.call("nfs_curl_bwd", _ptr(g_out), _ptr(g_s), D, H, W, nd, _stream())
    return g_s


# ---- stylising through a stream function (include/nfs_hip.h: grid variable 's') ---------------------------------------

def stream_velocity(s):
    """stream velocity of a stream function s [D,H,W,3]: its curl with the channels reversed, so that component k moves
    along array axis k as ``advect_fwd`` wants -- divergence-free in forward differences"""
    return curl_fwd(s).flip(-1).contiguous()


def stream_velocity_bwd(g_vel):
    """adjoint of ``stream_velocity``: g_s = curl^T(reverse(g_vel))"""
    return curl_bwd(g_vel.flip(-1).contiguous())


def advect_source_takes(D, H, W):
    """the shapes ``nfs_advect_stream_fwd`` / ``_bwd`` and their potential and Helmholtz twins take (the four-voxel advect
    kernel's, include/nfs_hip.h)"""
    return min(D, H, W) >= 2 and (D * H * W) % 4 == 0 and D * H * W < (1 << 30)


advect_stream_takes = advect_source_takes          # (the name the stream-function variable introduced it under)


def advect_stream_fwd(d, s, out=None, live=None):
    """advect_fwd(d, stream_velocity(s)) for a scalar field d [D,H,W,1], the velocity never stored (one kernel; the same
    bits).  ``live`` as in ``advect_fwd``.  Shapes the fused kernel does not take run the composition."""
    return advect_source_fwd("s", d, s, out=out, live=live)


def advect_stream_bwd(d, s, g_out, g_vel=None):
    """velocity gradient [D,H,W,3] (advect's channel order) of ``advect_stream_fwd``, the velocity recomputed from s:
    the bits of advect_bwd(d, stream_velocity(s), g_out, need_d=False)"""
    return advect_source_bwd("s", d, s, g_out, g_vel=g_vel)


def stream_bwd_adam(g_vel, s, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    """g_s = stream_velocity_bwd(g_vel) consumed on the spot by the TF-Adam update of s (s, m, v [D,H,W,3] in place)"""
    source_bwd_adam("s", g_vel, s, m, v, lr_t, beta1, beta2, eps)


# ---- the gradient of a potential and stylising through it (include/nfs_hip.h: grid variables 'p', 'sp') ------------------

def grad_fwd(p):
    """p [D,H,W] -> [D,H,W,3] = (dx, dy, dz): forward differences, last slice replicated (transform.py:508-515)"""
    D, H, W = p.shape
    out = _empty((D, H, W, 3), p)
    _lib.call("nfs_grad_fwd", _ptr(p), _ptr(out), D, H, W, _stream())
    return out


def grad_bwd(g_out):
    """adjoint of ``grad_fwd``: g_out [D,H,W,3] -> [D,H,W] (a gather: deterministic)"""
    D, H, W, _ = g_out.shape
    g_p = _empty((D, H, W), g_out)
    _lib.call("nfs_grad_bwd", _ptr(g_out), _ptr(g_p), D, H, W, _stream())
    return g_p


def potential_velocity(phi):
    """potential velocity of phi [D,H,W]: its gradient with the channels reversed, so that component k moves along array
    axis k as ``advect_fwd`` wants -- irrotational in forward differences"""
    return grad_fwd(phi).flip(-1).contiguous()


def potential_velocity_bwd(g_vel):
    """adjoint of ``potential_velocity``: g_phi = grad^T(reverse(g_vel))"""
    return grad_bwd(g_vel.flip(-1).contiguous())


def helmholtz_velocity(a):
    """velocity of a Helmholtz variable a [D,H,W,4] = (psi, phi): stream_velocity(psi) + potential_velocity(phi)"""
    assert a.shape[-1] == 4
    return stream_velocity(a[..., :3].contiguous()) + potential_velocity(a[..., 3].contiguous())


def helmholtz_velocity_bwd(g_vel):
    """adjoint of ``helmholtz_velocity``: [D,H,W,4] = (stream_velocity_bwd(g_vel), potential_velocity_bwd(g_vel))"""
    return torch.cat([stream_velocity_bwd(g_vel), potential_velocity_bwd(g_vel).unsqueeze(-1)], dim=-1)


# what stands for the velocity under each grid variable: (shape of the variable given (D, H, W), velocity, its adjoint,
# the fused forward / adjoint / update entry points)
_SOURCES = {
    "s": (lambda D, H, W: (D, H, W, 3), stream_velocity, stream_velocity_bwd,
          "nfs_advect_stream_fwd", "nfs_advect_stream_bwd", "nfs_stream_bwd_adam"),
    "p": (lambda D, H, W: (D, H, W), potential_velocity, potential_velocity_bwd,
          "nfs_advect_potential_fwd", "nfs_advect_potential_bwd", "nfs_potential_bwd_adam"),
    "sp": (lambda D, H, W: (D, H, W, 4), helmholtz_velocity, helmholtz_velocity_bwd,
           "nfs_advect_helmholtz_fwd", "nfs_advect_helmholtz_bwd", "nfs_helmholtz_bwd_adam"),
}


def source_shape(kind, D, H, W):
    """shape of the variable of kind 's' (stream function), 'p' (potential) or 'sp' (Helmholtz pair) on a [D,H,W] grid"""
    return _SOURCES[kind][0](D, H, W)


def source_velocity(kind, x):
    """the velocity the variable ``x`` of that kind stands for [D,H,W,3]"""
    return _SOURCES[kind][1](x)


def source_velocity_bwd(kind, g_vel):
    """its adjoint: the gradient of the variable from the gradient of the velocity"""
    return _SOURCES[kind][2](g_vel)


def advect_source_fwd(kind, d, x, out=None, live=None):
    """advect_fwd(d, source_velocity(kind, x)) for a scalar field d [D,H,W,1], the velocity never stored (one kernel; the
    same bits).  ``live`` as in ``advect_fwd``.  Shapes the fused kernel does not take run the composition."""
    D, H, W, Cn = d.shape
    assert Cn == 1 and tuple(x.shape) == source_shape(kind, D, H, W) and x.is_contiguous()
    if not advect_source_takes(D, H, W):
        return advect_fwd(d, source_velocity(kind, x), out=out, live=live)
    if out is None:
        out = _empty(d.shape, d)
    _lib.call(_SOURCES[kind][3], _ptr(d), _ptr(x), _ptr(out), _ptr(live), D, H, W, _stream())
    _written(live)
    return out


def advect_source_bwd(kind, d, x, g_out, g_vel=None):
    """velocity gradient [D,H,W,3] (advect's channel order) of ``advect_source_fwd``, the velocity recomputed from x: the
    bits of advect_bwd(d, source_velocity(kind, x), g_out, need_d=False)"""
    D, H, W, Cn = d.shape
    assert Cn == 1 and tuple(x.shape) == source_shape(kind, D, H, W) and x.is_contiguous()
    if not advect_source_takes(D, H, W):
        return advect_bwd(d, source_velocity(kind, x), g_out, need_d=False, g_vel=g_vel)[1]
    if g_vel is None:
        g_vel = _empty((D, H, W, 3), d)
    _lib.call(_SOURCES[kind][4], _ptr(d), _ptr(x), _ptr(g_out), _ptr(g_vel), D, H, W, _stream())
    return g_vel


def source_bwd_adam(kind, g_vel, x, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    """g_x = source_velocity_bwd(kind, g_vel) consumed on the spot by the TF-Adam update of x (x, m, v in place)"""
    D, H, W, _ = g_vel.shape
    assert g_vel.shape[-1] == 3 and tuple(x.shape) == tuple(m.shape) == tuple(v.shape) == source_shape(kind, D, H, W)
    _lib.call(_SOURCES[kind][5], _ptr(g_vel), _ptr(x), _ptr(m), _ptr(v), D, H, W, float(lr_t), float(beta1),
              float(beta2), float(eps), _stream())
    _written(x, m, v)


def advect_potential_fwd(d, phi, out=None, live=None):
    """``advect_stream_fwd`` along the potential velocity of phi [D,H,W]"""
    return advect_source_fwd("p", d, phi, out=out, live=live)


def advect_potential_bwd(d, phi, g_out, g_vel=None):
    return advect_source_bwd("p", d, phi, g_out, g_vel=g_vel)


def advect_helmholtz_fwd(d, a, out=None, live=None):
    """``advect_stream_fwd`` along the Helmholtz velocity of a [D,H,W,4]"""
    return advect_source_fwd("sp", d, a, out=out, live=live)


def advect_helmholtz_bwd(d, a, g_out, g_vel=None):
    return advect_source_bwd("sp", d, a, g_out, g_vel=g_vel)


def potential_bwd_adam(g_vel, phi, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    """``stream_bwd_adam`` for a potential: phi, m, v [D,H,W] in place"""
    source_bwd_adam("p", g_vel, phi, m, v, lr_t, beta1, beta2, eps)


def helmholtz_bwd_adam(g_vel, a, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    """``stream_bwd_adam`` for a Helmholtz variable: a, m, v [D,H,W,4] in place"""
    source_bwd_adam("sp", g_vel, a, m, v, lr_t, beta1, beta2, eps)


def lap_down(x, k):
    """x [D,H,W,C] (3-D, k [5,5,5]) or [H,W,C] (2-D, k [5,5]) -> stride-2 'SAME' smoothing (util.py:60-66)"""
    nd = 3 if x.dim() == 4 else 2
    D, (H, W, Cn) = (x.shape[0] if nd == 3 else 1), x.shape[-3:]
    shp = (((D + 1) // 2,) if nd == 3 else ()) + ((H + 1) // 2, (W + 1) // 2, Cn)
    out = _empty(shp, x)
    _lib.call("nfs_lap_down", _ptr(x), _ptr(k), _ptr(out), D, H, W, Cn, nd, _stream())
    return out


def lap_up(lo, k, out_shape, scale, addend=None):
    """scale * conv_transpose(lo, k, out_shape, stride 2) + addend (util.py:62-65, 80-83)"""
    nd = 3 if lo.dim() == 4 else 2
    out = _empty(tuple(out_shape), lo)
    D, (H, W, Cn) = (out_shape[0] if nd == 3 else 1), tuple(out_shape)[-3:]
    _lib.call("nfs_lap_up", _ptr(lo), _ptr(k), float(scale), _ptr(addend), _ptr(out), D, H, W, Cn, nd, _stream())
    return out


def lap_up_rms_parts(out_shape):
    """partial sums ``lap_up_rms`` writes for an output of this shape; 0 where only ``lap_up`` applies"""
    nd = 3 if len(out_shape) == 4 else 2
    D, (H, W, Cn) = (out_shape[0] if nd == 3 else 1), tuple(out_shape)[-3:]
    return int(_lib.lib().nfs_lap_up_rms_parts(int(D), int(H), int(W), int(Cn), nd))


def lap_up_rms(lo, k, out_shape, scale, addend=None, addend_part=None, eps=1e-10, want_part=False):
    """``lap_up`` with the RMS normalisation of pyramid levels riding in it (nfs_hip.h: nfs_lap_up_rms): ``addend_part``
    (the partial sums of addend^2 an earlier call returned): the addend enters divided by max(rms(addend), eps);
    ``want_part``: also return the partial sums of out^2.  -> out, or (out, part)"""
    nd = 3 if lo.dim() == 4 else 2
    out = _empty(tuple(out_shape), lo)
    D, (H, W, Cn) = (out_shape[0] if nd == 3 else 1), tuple(out_shape)[-3:]
    part = _empty((lap_up_rms_parts(out_shape),), lo) if want_part else None
    _lib.call("nfs_lap_up_rms", _ptr(lo), _ptr(k), float(scale), _ptr(addend), _ptr(addend_part),
              0 if addend_part is None else addend_part.numel(), 0 if addend is None else addend.numel(), float(eps),
              _ptr(out), _ptr(part), D, H, W, Cn, nd, _stream())
    return (out, part) if want_part else out


def normalize_mean(x, use_abs=False, eps=1e-10):
    """x / max(sqrt(mean(x^2)), eps)  (normalize_std, util.py:86-90)  or  x / max(mean|x|, eps)"""
    out = _empty(x.shape, x)
    ws = _empty((1024,), x)
    _lib.call("nfs_normalize_mean", _ptr(x), _ptr(out), x.numel(), int(bool(use_abs)), float(eps), _ptr(ws), 1024,
              _stream())
    return out


def transport_step(g, u, scale=1.0, w_g=1.0, addend=None, w_addend=0.0, out=None):
    """out = w_g*advect(g, scale*u) + w_addend*addend: one frame crossing of ``_transport`` (styler_base.py:59-89) for the
    C-channel field g [D,H,W,C] with the temporal filter's accumulation fused in"""
    D, H, W, Cn = g.shape
    if out is None:
        out = _empty(g.shape, g)
    _lib.call("nfs_transport_step", _ptr(g), _ptr(u), float(scale), float(w_g), _ptr(addend), float(w_addend), _ptr(out),
              D, H, W,
              Cn, _stream())
    return out


# ---- stylising a 2-D grid (include/nfs_grid2d.h, libnfs_grid2d.so; engine: grid2d.py) -----------------------------------
# the 2-D rows of the ``_SOURCES`` table: kind -> (``src`` of the entry points, channels of the variable; 0 = no channel axis)
_SOURCES2D = {"v": (0, 2), "s": (1, 0), "p": (2, 0), "sp": (3, 2)}


def source2d_shape(kind, H, W):
    """shape of the 2-D variable of kind 'v' (velocity [H,W,2]), 's' (psi [H,W]), 'p' (phi [H,W]) or 'sp' ([H,W,2] =
    (psi, phi)) on an [H,W] grid"""
    ch = _SOURCES2D[kind][1]
    return (H, W, ch) if ch else (H, W)


def _var2d(kind, x, H, W):
    assert tuple(x.shape) == source2d_shape(kind, H, W) and x.is_contiguous(), (kind, tuple(x.shape), (H, W))
    return _SOURCES2D[kind][0]


def source2d_velocity(kind, x, out=None):
    """the velocity [H,W,2] (``advect2d_fwd``'s units and channel order) the 2-D variable ``x`` of that kind stands for"""
    H, W = x.shape[:2]
    src = _var2d(kind, x, H, W)
    if out is None:
        out = _empty((H, W, 2), x)
    _lib.call("nfs_source2d_velocity_fwd", _ptr(x), src, _ptr(out), H, W, _stream())
    _written(out)
    return out


def source2d_velocity_bwd(kind, g_vel):
    """its adjoint: the gradient of the variable from the gradient g_vel [H,W,2] of the velocity (a gather: deterministic)"""
    H, W, _ = g_vel.shape
    g_x = _empty(source2d_shape(kind, H, W), g_vel)
    _lib.call("nfs_source2d_velocity_bwd", _ptr(g_vel), _SOURCES2D[kind][0], _ptr(g_x), H, W, _stream())
    return g_x


def advect2d_source_fwd(kind, d, x, out=None):
    """advect2d_fwd(d, source2d_velocity(kind, x)) for a density d [H,W], the velocity never stored (the same bits)"""
    H, W = d.shape
    src = _var2d(kind, x, H, W)
    if out is None:
        out = _empty((H, W), d)
    _lib.call("nfs_advect2d_source_fwd", _ptr(d), _ptr(x), src, _ptr(out), H, W, _stream())
    _written(out)
    return out


def advect2d_source_bwd(kind, d, x, g_out, g_vel=None):
    """velocity gradient [H,W,2] of ``advect2d_source_fwd``: the bits of advect2d_bwd(d, velocity, g_out)'s g_vel"""
    H, W = d.shape
    src = _var2d(kind, x, H, W)
    if g_vel is None:
        g_vel = _empty((H, W, 2), d)
    _lib.call("nfs_advect2d_source_bwd", _ptr(d), _ptr(x), src, _ptr(g_out), _ptr(g_vel), H, W, _stream())
    return g_vel


def advect2d_bwd_adam(d, vel, g_out, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, adv_next=None):
    """the velocity gradient of advect2d(d [H,W], vel [H,W,2]) consumed by TF ApplyAdam on vel, m, v in place;
    ``adv_next`` [H,W] (optional) receives advect2d(d, updated vel)"""
    H, W = d.shape
    assert tuple(vel.shape) == tuple(m.shape) == tuple(v.shape) == (H, W, 2)
    _lib.call("nfs_advect2d_bwd_adam_fwd", _ptr(d), _ptr(vel), _ptr(g_out), _ptr(m), _ptr(v), _ptr(adv_next), H, W,
              float(lr_t), float(beta1), float(beta2), float(eps), _stream())
    _written(vel, m, v, adv_next)


def transport_step2d(g, u, scale=1.0, w_g=1.0, addend=None, w_addend=0.0, out=None):
    """``transport_step`` for a C-channel 2-D field g [H,W,C] and a simulation velocity u [H,W,2]"""
    H, W, Cn = g.shape
    if out is None:
        out = _empty(g.shape, g)
    _lib.call("nfs_transport_step2d", _ptr(g), _ptr(u), float(scale), float(w_g), _ptr(addend), float(w_addend), _ptr(out),
              H, W, Cn, _stream())
    return out


# ---- descent along a normalised gradient (include/nfs_descent.h, libnfs_descent.so; engine.LapDescentState) --------------

def descent_step(x, g, lr):
    """x <- fma(-lr, g, x) in place, one rounding per element (any shape; g shaped like x)"""
    assert x.numel() == g.numel()
    _lib.call("nfs_descent_step", _ptr(x), _ptr(g), x.numel(), float(lr), _stream())
    _written(x)


def advect_descent(d, vel, g, lr, adv_next, live_next=None):
    """the velocity variable's step fused with the next forward sample: vel [D,H,W,3] <- fma(-lr, g, vel) (the bits of
    ``descent_step``), ``adv_next`` [D,H,W] = advect(d, new vel) and ``live_next`` (optional, ``live_mask``) its live mask
    (the bits of ``advect_fwd`` on the new velocity); d [D,H,W] or [D,H,W,1]"""
    D, H, W = d.shape[:3]
    assert d.numel() == D * H * W and tuple(vel.shape) == (D, H, W, 3) and g.numel() == vel.numel()
    assert adv_next.is_contiguous() and adv_next.numel() == D * H * W
    _lib.call("nfs_advect_descent_fwd", _ptr(d), _ptr(vel), _ptr(g), float(lr), _ptr(adv_next), _ptr(live_next), D, H, W,
              _stream())
    _written(vel, adv_next, live_next)


def advect2d_descent(d, vel, g, lr, adv_next):
    """the 2-D twin: vel [H,W,2] <- fma(-lr, g, vel), ``adv_next`` [H,W] = advect2d(d [H,W], new vel)"""
    H, W = d.shape
    assert tuple(vel.shape) == (H, W, 2) and g.numel() == vel.numel() and adv_next.numel() == H * W
    _lib.call("nfs_advect2d_descent_fwd", _ptr(d), _ptr(vel), _ptr(g), float(lr), _ptr(adv_next), H, W, _stream())
    _written(vel, adv_next)


# ---- A9 -----------------------------------------------------------------------------

def smooth3d_relu_fwd(d, k, out=None):
    D, H, W = d.shape
    if out is None:
        out = _empty(d.shape, d)
    _lib.call("nfs_smooth3d_relu_fwd", _ptr(d), _ptr(out), D, H, W, float(k), _stream())
    return out


def smooth3d_relu_bwd(out, g_out, k, g_d=None):
    D, H, W = out.shape
    if g_d is None:
        g_d = _empty(out.shape, out)
    _lib.call("nfs_smooth3d_relu_bwd", _ptr(out), _ptr(g_out), _ptr(g_d), D, H, W, float(k), _stream())
    return g_d


# ---- A4 -----------------------------------------------------------------------------

def render_fwd(d, tau, liquid=False):
    """d [V,D,H,W] -> (img [V,H,W] un-normalised, raysum [V,H,W])"""
    V, D, H, W = d.shape
    img = _empty((V, H, W), d); rs = _empty((V, H, W), d)
    _lib.call("nfs_render_fwd", _ptr(d), _ptr(img), _ptr(rs), V, D, H, W, float(tau), int(liquid), _stream())
    return img, rs


def render_bwd(d, raysum, g_img, tau, liquid=False, g_d=None, want_max=False):
    """want_max: also return the device scalar max|g_d| (a by-product of the same pass) for rotate_bwd(g_max=...)"""
    V, D, H, W = d.shape
    if g_d is None:
        g_d = _empty(d.shape, d)
    gmax = _empty((1,), d) if want_max else None
    _lib.call("nfs_render_bwd", _ptr(d), _ptr(raysum), _ptr(g_img), _ptr(g_d), V, D, H, W, float(tau),
              int(liquid), _ptr(gmax), _stream())
    return (g_d, gmax) if want_max else g_d


def rotate_render_fwd(d, rot, tau, liquid=False, img=None, raysum=None, d_rot=None):
    """d [D,H,W], rot [V,3,3] -> (img [V,H,W], raysum [V,H,W]); d_rot [V,D,H,W] (optional) is filled
    with the rotated samples for the two-pass adjoint"""
    D, H, W = d.shape
    V = rot.shape[0]
    if img is None:
        img = _empty((V, H, W), d)
    if raysum is None:
        raysum = _empty((V, H, W), d)
    _lib.call("nfs_rotate_render_fwd", _ptr(d), _ptr(rot), _ptr(img), _ptr(raysum), _ptr(d_rot), V, D, H, W,
              float(tau), int(liquid), _stream())
    return img, raysum


_coef_layouts = {}


def render_coef_layout(V, D, H, W):
    """(nseg, seg_len) of the u / coefficient form of the rotate + render adjoint (transmittance mode), or None when the
    shape is outside the segmented forward kernel -- the caller then keeps the rotated samples and runs render_bwd"""
    key = (int(V), int(D), int(H), int(W))
    if key not in _coef_layouts:
        import ctypes
        nseg, seg_len = ctypes.c_int(0), ctypes.c_int(0)
        rc = _lib.lib().nfs_render_coef_layout(key[0], key[1], key[2], key[3], ctypes.byref(nseg), ctypes.byref(seg_len))
        _coef_layouts[key] = (nseg.value, seg_len.value) if rc == 0 else None
    return _coef_layouts[key]


def rotate_render_fwd_coef(d, rot, tau, img=None, raysum=None, u_rot=None, seg=None):
    """d [D,H,W], rot [V,3,3] -> (img [V,H,W], raysum [V,H,W], u_rot [V,D,H,W], seg [3,V,nseg,H,W]): the forward of
    rotate_render_fwd (transmittance) that keeps u = t + tau i per sample instead of the sample (see nfs_hip.h)"""
    D, H, W = d.shape
    V = rot.shape[0]
    nseg, _ = render_coef_layout(V, D, H, W)
    if img is None:
        img = _empty((V, H, W), d)
    if raysum is None:
        raysum = _empty((V, H, W), d)
    if u_rot is None:
        u_rot = _empty((V, D, H, W), d)
    if seg is None:
        seg = _empty((3, V, nseg, H, W), d)
    _lib.call("nfs_rotate_render_fwd_coef", _ptr(d), _ptr(rot), _ptr(img), _ptr(raysum), _ptr(u_rot), _ptr(seg), V, D, H, W,
              float(tau), _stream())
    return img, raysum, u_rot, seg


def render_ray_coef(g_img, seg, tau, ab=None, bounds=None):
    """image gradient g_img [V,H,W] + the forward's seg -> (ab [V,nseg,H,W,2], bounds [nblocks]: per-block bounds on
    max |sample gradient|, reduced by the consumer)"""
    V, H, W = g_img.shape
    nseg = seg.shape[2]
    if ab is None:
        ab = _empty((V, nseg, H, W, 2), g_img)
    if bounds is None:
        bounds = _empty((_lib.lib().nfs_render_ray_coef_bounds(V, H, W),), g_img)
    _lib.call("nfs_render_ray_coef", _ptr(g_img), _ptr(seg), _ptr(ab), _ptr(bounds), V, H, W, float(tau), _stream())
    return ab, bounds


_LIVE_WS = {}      # (device, D, H, W, stream) -> workspace of nfs_rotate_bwd_coef_live


def rotate_bwd_coef(u_rot, ab, rot, bounds, g_d_acc=None, overwrite=False, live=None, dilate=1):
    """the tiled rotate adjoint with the sample gradient A u - B formed on the fly; g_d_acc [D,H,W] (+=, or written).
    ``live`` (``advect_fwd(live=...)``): only the voxels within ``dilate`` cells of a live voxel get their sums (the rest
    of g_d is multiplied by an exact zero in the advect adjoint): tiles without any return at once"""
    V, D, H, W = u_rot.shape
    nseg, seg_len = render_coef_layout(V, D, H, W)
    if g_d_acc is None:
        overwrite = True
        g_d_acc = _empty((D, H, W), u_rot)
    if live is not None:
        # (one per stream: view groups on side streams run this adjoint concurrently, and a launch owns its ticket)
        key = (u_rot.device, D, H, W, int(_stream(u_rot.device) or 0))
        ws = _LIVE_WS.get(key)
        if ws is None:      # zeroed once: every launch leaves its ticket zero again (and a captured graph keeps the address)
            ws = _LIVE_WS[key] = _zeros((int(_lib.lib().nfs_rotate_live_workspace_ints(D, H, W)),), u_rot)
        _lib.call("nfs_rotate_bwd_coef_live", _ptr(u_rot), _ptr(ab), _ptr(rot), _ptr(g_d_acc), V, D, H, W, nseg, seg_len,
                  _ptr(bounds), int(bounds.numel()), int(bool(overwrite)), _ptr(live), int(dilate), _ptr(ws), _stream())
    else:
        _lib.call("nfs_rotate_bwd_coef", _ptr(u_rot), _ptr(ab), _ptr(rot), _ptr(g_d_acc), V, D, H, W, nseg, seg_len,
                  _ptr(bounds), int(bounds.numel()), int(bool(overwrite)), _stream())
    return g_d_acc


def rotate_render_bwd(d, rot, raysum, g_img, tau, liquid=False, g_d_acc=None):
    D, H, W = d.shape
    V = rot.shape[0]
    if g_d_acc is None:
        g_d_acc = _zeros(d.shape, d)
    _lib.call("nfs_rotate_render_bwd", _ptr(d), _ptr(rot), _ptr(raysum), _ptr(g_img), _ptr(g_d_acc), V, D, H, W,
              float(tau), int(liquid), _stream())
    return g_d_acc


def maxnorm_fwd(img, groups, out=None, gmax=None):
    n = img.numel() // groups
    if out is None:
        out = _empty(img.shape, img)
    if gmax is None:
        gmax = _empty((groups,), img)
    _lib.call("nfs_maxnorm_fwd", _ptr(img), _ptr(out), _ptr(gmax), groups, n, _stream())
    return out, gmax


def maxnorm_bwd(img, gmax, g_out, g_img=None):
    groups = gmax.numel()
    n = img.numel() // groups
    if g_img is None:
        g_img = _empty(img.shape, img)
    ws = _empty((_lib.lib().nfs_maxnorm_workspace_floats(groups),), img)     # partial sums of the multi-block path
    _lib.call("nfs_maxnorm_bwd", _ptr(img), _ptr(gmax), _ptr(g_out), _ptr(g_img), groups, n, _ptr(ws), _stream())
    return g_img


def maxnorm_input_fwd(img, groups, out=None, gmax=None):
    """img [V,H,W] (grey render) -> (x [V,H,W,3] = (img / max) * 255 - mean, gmax [groups]): nfs_maxnorm_fwd +
    nfs_loss_net_input_fwd in one pass (loss net at the render's size)"""
    V, H, W = img.shape
    x = _empty((V, H, W, 3), img) if out is None else out
    if gmax is None:
        gmax = _empty((groups,), img)
    _lib.call("nfs_maxnorm_input_fwd", _ptr(img), _ptr(x), _ptr(gmax), groups, img.numel() // groups, _stream())
    return x, gmax


def maxnorm_input_bwd(img, gmax, g_x, out=None):
    """adjoint of maxnorm_input_fwd: g_x [V,H,W,3] -> g_img [V,H,W]"""
    groups = gmax.numel()
    g_img = _empty(img.shape, img) if out is None else out
    ws = _empty((_lib.lib().nfs_maxnorm_workspace_floats(groups),), img)
    _lib.call("nfs_maxnorm_input_bwd", _ptr(img), _ptr(gmax), _ptr(g_x), _ptr(g_img), groups, img.numel() // groups,
              _ptr(ws), _stream())
    return g_img


# ---- colour rendering through the views (include/nfs_colour.h) -------------------------------------------------------

def ray_weights(d_rot, tau, gmax, out=None):
    """d_rot [V,D,H,W] (rotate_render_fwd(d_rot=...)), gmax [G] (maxnorm_fwd of the grey image) ->
    w [V,D,H,W] = exp(-tau sum_{z' >= z} d_rot) / gmax[view's group]; ``out`` may be d_rot itself (in place)"""
    V, D, H, W = d_rot.shape
    if out is None:
        out = _empty(d_rot.shape, d_rot)
    _lib.call("nfs_ray_weights", _ptr(d_rot), float(tau), _ptr(gmax), int(gmax.numel()), _ptr(out), V, D, H, W, _stream())
    _written(out)
    return out


def colour_project_fwd(q, rot, w, out=None):
    """q [D,H,W,C] (C in 1..4), rot [V,3,3], w [V,D,H,W] -> img [V,H,W,C] = sum_z w rotate(q)[z] (no rotated volume)"""
    D, H, W, Cn = q.shape
    V = rot.shape[0]
    assert tuple(w.shape) == (V, D, H, W), (tuple(w.shape), (V, D, H, W))
    if out is None:
        out = _empty((V, H, W, Cn), q)
    _lib.call("nfs_colour_project_fwd", _ptr(q), _ptr(rot), _ptr(w), _ptr(out), V, D, H, W, Cn, _stream())
    return out


COLOUR_BWD_ROUTES = ("atomic", "tiled", "coef")


COLOUR_ATOMIC_UPTO = 1 << 19           # samples V D H W up to which the scatter kernel is the default
COLOUR_COEF_FROM = 1 << 23             # samples from which the coefficient form is (where the shape has a layout)


def colour_bwd_route(V, D, H, W):
    """the route colour_project_bwd takes when none is named, as measured at C = 3 (tools/colour_bench.py,
    profiles/colour_ab.txt, first / second run).  The scatter kernel runs at the float atomics' rate
    (25.6 ms against 1.2 ms at 200^3 x 8 views), so it is the default only where the transpose is bound by its launches:
    it wins up to 16 x 64 x 64 x 8 = 2^19 samples (177.5 / 177.5 against 239.7 / 241.8 us), no longer at 16 x 64 x 96 x 8
    (260.0 / 264.0 against 255.3 / 254.6 us) and loses from 2^20 (344 against 266 us).  Above, the output-stationary
    adjoint per channel: through the materialised product (nfs_rotate_bwd), or, from 64 x 128 x 128 x 8 = 2^23 samples
    and where the shape has a coefficient layout (D >= 16), nfs_rotate_bwd_coef, which wins there and at every larger
    size measured (307 against 339 us; 1.21 against 1.44 ms at 6.4e7) and loses by 10 us at 32 x 100 x 100 x 8 = 2.6e6
    and below.  Between 2^19 and 7.9e5 and between 2.6e6 and 2^23 samples nothing was measured."""
    n = V * D * H * W
    if n <= COLOUR_ATOMIC_UPTO:
        return "atomic"
    return "coef" if (n >= COLOUR_COEF_FROM and render_coef_layout(V, D, H, W) is not None) else "tiled"


def colour_project_bwd(g_img, rot, w, g_q=None, route=None):
    """the transpose of colour_project_fwd: g_img [V,H,W,C] -> g_q [D,H,W,C] (written when None is passed, else +=).
    route: 'atomic'  nfs_colour_project_bwd (any shape; not bit-reproducible);
           'tiled'   per channel, the product g w materialised and nfs_rotate_bwd's output-stationary form (any shape);
           'coef'    per channel, nfs_rotate_bwd_coef with u = w, A = g_img[..., c], B = 0 (shapes with a coefficient
                     layout: D >= 16); both compositions are bit-reproducible and end in an interleave of the planes"""
    V, H, W, Cn = g_img.shape
    D = w.shape[1]
    assert tuple(w.shape) == (V, D, H, W), (tuple(w.shape), (V, D, H, W))
    route = route or colour_bwd_route(V, D, H, W)
    if route == "atomic":
        overwrite = g_q is None
        if overwrite:
            g_q = _empty((D, H, W, Cn), g_img)
        _lib.call("nfs_colour_project_bwd", _ptr(g_img), _ptr(rot), _ptr(w), _ptr(g_q), int(overwrite), V, D, H, W, Cn,
                  _stream())
        _written(g_q)
        return g_q
    if route == "coef":
        layout = render_coef_layout(V, D, H, W)
        if layout is None:
            raise ValueError("colour_project_bwd(route='coef'): no coefficient layout for %s (D >= 16 needed)"
                             % ((V, D, H, W),))
        wmax = w.amax()
    elif route != "tiled":
        raise ValueError("colour_project_bwd: route %r is none of %s" % (route, COLOUR_BWD_ROUTES))
    planes = []
    for c in range(Cn):
        gc = g_img[..., c]
        if route == "tiled":
            planes.append(rotate_bwd((w * gc.unsqueeze(1)).unsqueeze(-1), rot, tiled=True).squeeze(-1))
        else:
            ab = _zeros((V, layout[0], H, W, 2), g_img)
            ab[..., 0] = gc.unsqueeze(1)
            # >= every |sample gradient| = |g| w (and positive: the fixed-point scale is derived from it)
            bounds = (gc.abs().amax() * wmax).clamp_min(1e-30).reshape(1).contiguous()
            planes.append(rotate_bwd_coef(w, ab, rot, bounds))
    out = torch.stack(planes, -1)
    if g_q is None:
        return out
    g_q += out
    return g_q


# ---- the ray weights of a liquid colour render (include/nfs_liquid.h) -------------------------------------------------

def liquid_weights(d, rot, tau, w=None, grey=None, t_total=None):
    """d [D,H,W], rot [V,3,3] -> (w [V,D,H,W], grey [V,H,W], t_total [V,H,W]) in one pass over the rays:
    w = tau exp(-tau B) phi(tau S) with S = rotate(d) gathered on the fly and B the sum of the samples in front,
    t_total = exp(-tau sum_z S), grey = 1 - t_total (rotate_render_fwd(liquid=True)'s image).  sum_z w S + t_total = 1."""
    D, H, W = d.shape
    V = int(rot.shape[0])
    if w is None:
        w = _empty((V, D, H, W), d)
    if grey is None:
        grey = _empty((V, H, W), d)
    if t_total is None:
        t_total = _empty((V, H, W), d)
    assert tuple(w.shape) == (V, D, H, W) and tuple(grey.shape) == (V, H, W) == tuple(t_total.shape)
    _lib.call("nfs_liquid_weights", _ptr(d), _ptr(rot), float(tau), _ptr(w), _ptr(grey), _ptr(t_total), V, D, H, W,
              _stream())
    _written(w, grey, t_total)
    return w, grey, t_total


# ---- the liquid colour render's derivative in the density (include/nfs_absorb.h) -------------------------------------

def liquid_absorb_bwd(g_J, q, d, rot, w, t_total, bg, tau, out=None):
    """g_J [V,H,W,C], q [D,H,W,C] (C in 1..4), d [D,H,W], rot [V,3,3], w [V,D,H,W] and t_total [V,H,W] as
    ``liquid_weights`` wrote them, bg [C] (device) -> g_S [V,D,H,W] = d loss / d rotate(d) of J = sum_z w rotate(q) + t bg
    with q held constant (``rotate_bwd`` of it is the gradient in d).  ``out`` may be ``w`` itself: the weights are then
    overwritten."""
    D, H, W = d.shape
    V, C = int(rot.shape[0]), int(q.shape[-1])
    if tuple(q.shape) != (D, H, W, C) or tuple(g_J.shape) != (V, H, W, C) or tuple(w.shape) != (V, D, H, W) \
            or tuple(t_total.shape) != (V, H, W) or int(bg.numel()) != C:
        raise ValueError("liquid_absorb_bwd: g_J %s, q %s, w %s, t_total %s, bg %s do not fit d %s through %d views"
                         % (tuple(g_J.shape), tuple(q.shape), tuple(w.shape), tuple(t_total.shape), tuple(bg.shape),
                            tuple(d.shape), V))
    if out is None:
        out = _empty((V, D, H, W), d)
    assert tuple(out.shape) == (V, D, H, W)
    _lib.call("nfs_liquid_absorb_bwd", _ptr(g_J), _ptr(q), _ptr(d), _ptr(rot), _ptr(w), _ptr(t_total), _ptr(bg), float(tau),
              _ptr(out), V, D, H, W, C, _stream())
    _written(out)
    return out


# ---- the smoke colour render at a fixed exposure and its derivative in the density (include/nfs_exposure.h) ----------

def exposure_weights(d, rot, tau, gain=1.0, w=None, grey=None):
    """d [D,H,W], rot [V,3,3] -> (w [V,D,H,W], grey [V,H,W]) in one pass over the rays: w = gain tau exp(-tau sum_{z' >= z} S)
    with S = rotate(d) gathered on the fly (the smoke render's transmittance, no maximum), grey = sum_z w S <= gain (1 - t)."""
    D, H, W = d.shape
    V = int(rot.shape[0])
    if w is None:
        w = _empty((V, D, H, W), d)
    if grey is None:
        grey = _empty((V, H, W), d)
    assert tuple(w.shape) == (V, D, H, W) and tuple(grey.shape) == (V, H, W)
    _lib.call("nfs_exposure_weights", _ptr(d), _ptr(rot), float(tau), float(gain), _ptr(w), _ptr(grey), V, D, H, W,
              _stream())
    _written(w, grey)
    return w, grey


def exposure_absorb_bwd(g_J, q, rot, w, tau, out=None):
    """g_J [V,H,W,C], q [D,H,W,C] (C in 1..4), rot [V,3,3], w [V,D,H,W] as ``exposure_weights`` wrote it ->
    g_S [V,D,H,W] = -tau sum_{z' <= z} w sum_c g_J[c] rotate(q)[z',c] = d loss / d rotate(d) of J = sum_z w rotate(q) with q
    held constant (``rotate_bwd`` of it is the gradient in d).  ``out`` may be ``w`` itself: the weights are then
    overwritten."""
    D, H, W, C = (int(x) for x in q.shape)
    V = int(rot.shape[0])
    if tuple(g_J.shape) != (V, H, W, C) or tuple(w.shape) != (V, D, H, W):
        raise ValueError("exposure_absorb_bwd: g_J %s, w %s do not fit q %s through %d views"
                         % (tuple(g_J.shape), tuple(w.shape), tuple(q.shape), V))
    if out is None:
        out = _empty((V, D, H, W), w)
    assert tuple(out.shape) == (V, D, H, W)
    _lib.call("nfs_exposure_absorb_bwd", _ptr(g_J), _ptr(q), _ptr(rot), _ptr(w), float(tau), _ptr(out), V, D, H, W, C,
              _stream())
    _written(out)
    return out


# ---- the emission of a colour grid (include/nfs_emission.h) -----------------------------------------------------------

def _emission_dims(c, e):
    Cn = int(c.shape[-1])
    if tuple(c.shape[:-1]) != tuple(e.shape):
        raise ValueError("emission: the colours %s are not the grey volume %s with a channel axis"
                         % (tuple(c.shape), tuple(e.shape)))
    return int(e.numel()), Cn


def emission_fwd(c, e, out=None):
    """c [..., C] (C in 1..4), e [...] -> q = clamp01(c) * e, e broadcast over the channels"""
    n, Cn = _emission_dims(c, e)
    if out is None:
        out = _empty(c.shape, c)
    _lib.call("nfs_emission_fwd", _ptr(c), _ptr(e), _ptr(out), n, Cn, _stream())
    _written(out)
    return out


def emission_bwd(g_q, c, e, out=None):
    """the adjoint of emission_fwd in c: g_c = g_q * e where 0 <= c <= 1, else +0"""
    n, Cn = _emission_dims(c, e)
    assert g_q.shape == c.shape, (tuple(g_q.shape), tuple(c.shape))
    if out is None:
        out = _empty(c.shape, c)
    _lib.call("nfs_emission_bwd", _ptr(g_q), _ptr(c), _ptr(e), _ptr(out), n, Cn, _stream())
    _written(out)
    return out


def emission_bwd_adam(g_q, c, e, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    """emission_bwd consumed by TF ApplyAdam on (c, m, v) in place: bit-equal to emission_bwd + adam_tf_step"""
    n, Cn = _emission_dims(c, e)
    assert g_q.shape == c.shape == m.shape == v.shape
    _lib.call("nfs_emission_bwd_adam", _ptr(g_q), _ptr(c), _ptr(e), _ptr(m), _ptr(v), n, Cn, float(lr_t), float(beta1),
              float(beta2), float(eps), _stream())
    _written(c, m, v)


# ---- A5 -----------------------------------------------------------------------------

def loss_net_input_fwd(img, H2=None, W2=None, want_d_img=True, want_x=True, out_d_img=None, out_x=None):
    """img [B,H,W,Cin] in [0,1] -> (d_img [B,H2,W2,3] 0..255, x = d_img - mean)"""
    B, H, W, Cin = img.shape
    H2 = H if H2 is None else H2
    W2 = W if W2 is None else W2
    d_img = (_empty((B, H2, W2, 3), img) if out_d_img is None else out_d_img) if want_d_img else None
    x = (_empty((B, H2, W2, 3), img) if out_x is None else out_x) if want_x else None
    _lib.call("nfs_loss_net_input_fwd", _ptr(img), _ptr(d_img), _ptr(x), B, H, W, Cin, H2, W2, _stream())
    return d_img, x


def loss_net_input_bwd(g_x, H, W, Cin, out=None):
    B, H2, W2, _ = g_x.shape
    g_img = _empty((B, H, W, Cin), g_x) if out is None else out
    _lib.call("nfs_loss_net_input_bwd", _ptr(g_x), _ptr(g_img), B, H, W, Cin, H2, W2, _stream())
    return g_img


# ---- A6 -----------------------------------------------------------------------------

def gemm_mode(mode=None):
    """Arithmetic of the batched Winograd GEMMs (process-wide): 1 = split-limb form, the default (float32 operands as
    three exact bf16 limbs, six limb products on the bf16 MFMA, float32 accumulation: float32-equivalent accuracy at 2.67x
    the matrix-pipe rate), 0 = float32-input MFMA.  Returns the previous mode; ``None`` only queries."""
    return int(_lib.lib().nfs_gemm_mode(-1 if mode is None else int(mode)))


def conv3x3_pack(w_hwio, kind):
    """w [3,3,Ci,Co] -> packed device buffer for kind 0 (fwd) / 1 (dgrad)"""
    _, _, Ci, Co = w_hwio.shape
    n = _lib.lib().nfs_conv3x3_packed_floats(Ci, Co, kind)
    packed = _empty((n,), w_hwio)
    _lib.call("nfs_conv3x3_pack", _ptr(w_hwio), _ptr(packed), Ci, Co, kind, _stream())
    return packed


_conv_ws = {}


def conv_workspace(device, floats):
    """split-K scratch, grown on demand and shared by all conv calls of a device (calls on one stream
    are ordered, so sharing is safe)"""
    if torch.cuda.is_current_stream_capturing():
        # (see ``workspace``: a capture owns its scratch.)  A fresh buffer per call: the graph's private pool hands the
        # block back to later allocations of the same capture in stream order and keeps it for the replays
        return torch.empty(int(floats), dtype=torch.float32, device=device)
    key = (device.type, device.index, _stream(device))   # one per stream
    cur = _conv_ws.get(key)
    if cur is None or cur.numel() < floats:
        cur = torch.empty(int(floats), dtype=torch.float32, device=device)
        _conv_ws[key] = cur
    return cur


def _conv_ws_for(B, H, W, Ci, Co, device, splitk):
    if not splitk:
        return None, 0
    want = _lib.lib().nfs_conv3x3_workspace_floats(B, H, W, Ci, Co)   # split-K partials or Winograd V/M buffers
    ws = conv_workspace(device, want)
    return ws, ws.numel()


def conv3x3_relu_bits_words(B, H, W, Ci, Co, pooled):
    return int(_lib.lib().nfs_conv3x3_relu_bits_words(B, H, W, Ci, Co, int(bool(pooled))))


def conv3x3_relu_bits(B, H, W, Ci, Co, pooled, device):
    """buffer for a layer's ReLU bit cache (raw 32-bit words, held in a float32 tensor), or None when the layer does
    not keep one: pass it to the layer's conv3x3_fwd / conv3x3_fwd_pool and later to its conv3x3_dgrad / _pool"""
    n = _lib.lib().nfs_conv3x3_relu_bits_words(B, H, W, Ci, Co, int(bool(pooled)))
    return torch.empty(n, dtype=torch.float32, device=device) if n > 0 else None


CONV_FAMILIES = ("c3_generic", "c3_mfma", "direct", "wg4_three", "wg4_single", "wg5")


def conv3x3_plan(B, H, W, K, N, pooled=False):
    """which kernels the conv call for K input / N output channels of its kernel runs with a full workspace (forward:
    K = Ci, N = Co; data gradient: K = Co, N = Ci; pooled: 0 plain, 1 a fused-pool form, 2 the pooled gradient masked
    from the float output), by the launch code's own rules; launches nothing.  ``no_ws``: the
    direct implicit GEMM the same call runs without one (splitk=False)."""
    buf = (C.c_int * 12)()
    _lib.call("nfs_conv3x3_plan", B, H, W, K, N, int(pooled), C.addressof(buf))
    v = list(buf)
    return dict(family=CONV_FAMILIES[v[0]], ragged=bool(v[1]), in_waves=v[2], out_waves=v[3], kparts=v[4], tiles=v[5],
                blocks=v[6], Z=v[7] if v[0] >= 3 else 0, bn=v[7] if v[0] == 2 else 0,
                no_ws=dict(bn=v[8], kparts=v[9], ragged=bool(v[10]), tiles=v[11]))


def conv3x3_fwd(x, packed, bias, Co, relu=True, out=None, splitk=True, relu_bits=None):
    B, H, W, Ci = x.shape
    if out is None:
        out = _empty((B, H, W, Co), x)
    ws, nws = _conv_ws_for(B, H, W, Ci, Co, x.device, splitk)
    _lib.call("nfs_conv3x3_fwd", _ptr(x), _ptr(packed), _ptr(bias), _ptr(out), B, H, W, Ci, Co, int(relu),
              _ptr(ws), nws, _ptr(relu_bits if splitk else None), _stream())
    return out


def conv3x3_dgrad(gy, packed, Ci, x_in=None, addend=None, out=None, splitk=True, relu_bits=None,
                  addend_unmasked=False):
    B, H, W, Co = gy.shape
    if out is None:
        out = _empty((B, H, W, Ci), gy)
    ws, nws = _conv_ws_for(B, H, W, Ci, Co, gy.device, splitk)
    _lib.call("nfs_conv3x3_dgrad", _ptr(gy), _ptr(packed), _ptr(x_in), _ptr(addend), _ptr(out), B, H, W, Ci, Co,
              _ptr(ws), nws, _ptr(relu_bits if (splitk and x_in is not None) else None), int(bool(addend_unmasked)),
              _stream())
    return out


def conv3x3_fwd_pool(x, packed, bias, Co, relu=True, relu_bits=None, want_y=True, out=None, out_pool=None):
    """conv + bias + ReLU and its 2x2 VALID average pool in one pass -> (y [B,H,W,Co], y_pool [B,H/2,W/2,Co]);
    with a ReLU bit cache and want_y=False the full-resolution output is not written at all (y = None)"""
    B, H, W, Ci = x.shape
    if not (want_y or relu_bits is None):
        out = None
    elif out is None:
        out = _empty((B, H, W, Co), x)
    pooled = _empty((B, H // 2, W // 2, Co), x) if out_pool is None else out_pool
    ws, nws = _conv_ws_for(B, H, W, Ci, Co, x.device, True)
    _lib.call("nfs_conv3x3_fwd_pool", _ptr(x), _ptr(packed), _ptr(bias), _ptr(out), _ptr(pooled), B, H, W, Ci, Co,
              int(relu), _ptr(ws), nws, _ptr(relu_bits), _stream())
    return out, pooled


def conv3x3_dgrad_pool(gy_pool, x_out, packed, Ci, x_in=None, addend=None, relu_bits=None, hw=None,
                       addend_unmasked=False, out=None):
    """data gradient of a conv followed by ReLU + 2x2 average pool, from the gradient at the POOLED resolution
    gy_pool [B,H/2,W/2,Co] and the conv's own output x_out [B,H,W,Co] -> gx [B,H,W,Ci]; x_out may be None when the
    layer's ReLU bit cache is given (``hw`` = its (H, W) then)"""
    if x_out is not None:
        B, H, W, Co = x_out.shape
    else:
        assert relu_bits is not None and hw is not None
        B, Co = gy_pool.shape[0], gy_pool.shape[-1]
        H, W = hw
    if out is None:
        out = _empty((B, H, W, Ci), gy_pool)
    ws, nws = _conv_ws_for(B, H, W, Ci, Co, gy_pool.device, True)
    _lib.call("nfs_conv3x3_dgrad_pool", _ptr(gy_pool), _ptr(x_out), _ptr(packed), _ptr(x_in), _ptr(addend), _ptr(out),
              B, H, W, Ci, Co, _ptr(ws), nws, _ptr(relu_bits), int(bool(addend_unmasked)), _stream())
    return out


def avgpool2_fwd(x, out=None):
    B, H, W, Cn = x.shape
    if out is None:
        out = _empty((B, H // 2, W // 2, Cn), x)
    _lib.call("nfs_avgpool2_fwd", _ptr(x), _ptr(out), B, H, W, Cn, _stream())
    return out


def avgpool2_bwd(gy, x_shape, x=None, addend=None, out=None):
    B, H, W, Cn = x_shape
    if out is None:
        out = _empty(tuple(x_shape), gy)
    _lib.call("nfs_avgpool2_bwd", _ptr(gy), _ptr(x), _ptr(addend), _ptr(out), B, H, W, Cn, _stream())
    return out


# ---- A7 / A12 -----------------------------------------------------------------------

def gram_fwd(F, scale, scale_dev=None, G=None, two_pass=True):
    """F [B,h,w,C] (or [B,HW,C]) -> G [B,C,C] = scale * F^T F"""
    B, Cn = F.shape[0], F.shape[-1]
    HW = F.numel() // (B * Cn)
    ws, nws = None, 0
    if two_pass:
        nws = _lib.lib().nfs_gram_workspace_floats(B, HW, Cn)
        ws = conv_workspace(F.device, nws)      # shared scratch (calls on one stream are ordered)
        nws = ws.numel()
    if G is None:
        G = _empty((B, Cn, Cn), F) if two_pass else _zeros((B, Cn, Cn), F)
    elif not two_pass:
        G.zero_()
    _lib.call("nfs_gram_fwd", _ptr(F), _ptr(G), B, HW, Cn, _ptr(scale_dev), float(scale), _ptr(ws), nws, _stream())
    return G


def style_loss_fwd(G, Gs, weight, loss_acc, Dmat=None):
    B, Cn, _ = G.shape
    if Dmat is None:
        Dmat = _empty(G.shape, G)
    _lib.call("nfs_style_loss_fwd", _ptr(G), _ptr(Gs), _ptr(loss_acc), _ptr(Dmat), B, Gs.shape[0], Cn, float(weight),
              _stream())
    return Dmat


def gram_style_group(Fs, Gss, weights, relu_masks, want_G=False, channels=None):
    """Gram matrix, style loss and Gram gradient of SEVERAL style layers in three launches (the loop of
    styler_base.py:152-185): ``Fs`` list of [B,h,w,C] activations, ``Gss`` their style Grams [Bs,C,C] (scaled by
    1/(2 h w C) like G), ``weights`` w_layer * w_style, ``relu_masks`` whether dF carries the layer's ReLU mask.
    Returns (loss_parts [P,B] -- the style loss of image b is loss_parts[:, b].sum(), every entry written, no atomics --,
    list of dF, list of G or None)."""
    n = len(Fs)
    if n > 8:                                          # the descriptor table of one launch holds 8 layers
        a = gram_style_group(Fs[:8], Gss[:8], weights[:8], relu_masks[:8], want_G, channels and channels[:8])
        b = gram_style_group(Fs[8:], Gss[8:], weights[8:], relu_masks[8:], want_G, channels and channels[8:])
        return torch.cat([a[0], b[0]]), a[1] + b[1], (a[2] + b[2] if want_G else None)
    arr = (_lib.GramLayer * n)()
    keep = []
    B = Fs[0].shape[0]
    for l, (F, Gs, w, rm) in enumerate(zip(Fs, Gss, weights, relu_masks)):
        Cn = F.shape[-1]
        HW = F.numel() // (B * Cn)
        Dm = _empty((B, Cn, Cn), F)
        dF = _empty(F.shape, F)
        G = _empty((B, Cn, Cn), F) if want_G else None
        keep.append((Dm, dF, G))
        y = arr[l]
        y.F, y.Gs, y.G, y.Dmat, y.dF = _ptr(F), _ptr(Gs), _ptr(G), _ptr(Dm), _ptr(dF)
        y.B, y.Bs, y.HW, y.C = B, Gs.shape[0], HW, Cn
        # (rows padded with zero channels -- Inception module outputs --: the denominator counts the logical ones)
        y.scale, y.weight, y.relu_mask = 1.0 / (2.0 * HW * (channels[l] if channels else Cn)), float(w), int(bool(rm))
    L = _lib.lib()
    P = L.nfs_gram_style_group_parts(arr, n)
    nws = L.nfs_gram_style_group_workspace_floats(arr, n)
    if P < 0 or nws < 0:
        raise ValueError("gram_style_group: 1..8 layers of one batch size with C a multiple of 64")
    ws = conv_workspace(Fs[0].device, max(nws, 1))      # shared scratch (calls on one stream are ordered)
    parts = _empty((P, B), Fs[0])
    _lib.call("nfs_gram_style_group_fwd", arr, n, _ptr(parts), _ptr(ws), ws.numel(), _stream())
    _lib.call("nfs_gram_group_bwd", arr, n, _stream())
    return parts, [k[1] for k in keep], ([k[2] for k in keep] if want_G else None)


def content_loss(F, weight, loss_acc, g_acc, channel=0, target=None, amp=100.0, signed=False):
    """content loss of the post-ReLU activation F [B,h,w,C] (styler_base.py:135-150): with ``target`` [Bt,h,w,C]
    mean((F - amp*target)^2), else channel maximisation (channel != 0) or -mean(F); loss_acc [B] and
    g_acc [B,h,w,C] (gradient wrt the pre-activation) are accumulated into"""
    B, Cn = F.shape[0], F.shape[-1]
    HW = F.numel() // (B * Cn)
    mode = 2 if target is not None else (0 if channel else 1)
    Bt = target.shape[0] if target is not None else 0
    # ``signed``: F is not a ReLU output (an Inception '*_pre_relu' tensor): |F| proper, gradient wrt F itself
    _lib.call("nfs_content_loss_signed" if signed else "nfs_content_loss", _ptr(F), _ptr(target), _ptr(loss_acc),
              _ptr(g_acc), B, Bt, HW, Cn, int(channel or 0),
              mode, float(weight), float(amp), _stream())
    return g_acc


def resize_bicubic_tf1(x, oh, ow, out=None):
    """TF-1 legacy bicubic resize of x [B,H,W,C] -> [B,oh,ow,C] (styler_base.py:166), forward only"""
    B, H, W, Cn = x.shape
    if out is None:
        out = _empty((B, oh, ow, Cn), x)
    _lib.call("nfs_resize_bicubic_tf1", _ptr(x), _ptr(out), B, H, W, Cn, int(oh), int(ow), _stream())
    return out


RESIZE_METHODS = {"nearest": 0, "bilinear": 1}


def resize3d(x, size, method="bilinear", align_corners=False, scale=1.0):
    """TF-1 legacy resize of a volume x [D,H,W] or [D,H,W,C] -> ``size`` = (oD, oH, oW), times ``scale``: over (H, W) of
    every depth slice, then over D (util.py:128-143 with is_3d); forward only.  ``method``: 'nearest' or 'bilinear'."""
    if method not in RESIZE_METHODS:
        raise ValueError("resize3d method %r: 'nearest' or 'bilinear'" % (method,))
    if x.dim() not in (3, 4):
        raise ValueError("resize3d takes [D,H,W] or [D,H,W,C], got %s" % (tuple(x.shape),))
    D, H, W = x.shape[:3]
    Cn = x.shape[3] if x.dim() == 4 else 1
    oD, oH, oW = (int(s) for s in size)
    out = _empty((oD, oH, oW) + tuple(x.shape[3:]), x)
    _lib.call("nfs_resize3d", _ptr(x), _ptr(out), D, H, W, Cn, oD, oH, oW, RESIZE_METHODS[method],
              int(bool(align_corners)), float(scale), _stream())
    return out


def style_mask_apply(F, mask):
    """F [B,h,w,C], mask [B,h,w,1] -> (F * mask, scale [B] = 1 / (2 * sum(mask) * C))  (styler_base.py:167-169)"""
    B, Cn = F.shape[0], F.shape[-1]
    HW = F.numel() // (B * Cn)
    Fm = _empty(F.shape, F)
    scale = _empty((B,), F)
    _lib.call("nfs_style_mask_apply", _ptr(F), _ptr(mask), _ptr(Fm), _ptr(scale), B, HW, Cn, _stream())
    return Fm, scale


def style_mask_bwd(dFm, mask, F):
    """dFm * mask * (F > 0)"""
    B, Cn = F.shape[0], F.shape[-1]
    HW = F.numel() // (B * Cn)
    out = _empty(F.shape, F)
    _lib.call("nfs_style_mask_bwd", _ptr(dFm), _ptr(mask), _ptr(F), _ptr(out), B, HW, Cn, _stream())
    return out


import os as _os
_HIST_WIDE = _os.environ.get("NFS_HIST_WIDE", "1") != "0"   # 0: per-channel kernel for every C > 4 (timing comparisons)


def hist_loss(F, templ, weight, loss_acc, g_acc=None, relu_mask=False, mask=None):
    """histogram loss of F [B,h,w,C] against the template features templ [Bt,ht,wt,C] (styler_base.py:187-209,
    util.py:317-399): loss_acc [B] += weight * sum((F - matched)^2); g_acc [B,h,w,C] += 2 weight (F - matched).
    ``mask`` [B,h,w(,1)]: the masked branch (styler_base.py:104-125, 196-201) -- pixels where it is 0 leave the source."""
    B, Cn = F.shape[0], F.shape[-1]
    HW = F.numel() // (B * Cn)
    Bt = templ.shape[0]
    HWt = templ.numel() // (Bt * Cn)
    assert templ.shape[-1] == Cn
    if mask is not None:
        assert mask.numel() == B * HW and mask.is_contiguous(), "mask must be [B,h,w] of the feature's size"
    if Cn <= 4 or (Cn % 4 == 0 and Cn <= 128 and _HIST_WIDE):
        # few channels (the default hist layer is the 3-channel loss-net input): one block per (image, channel) would
        # leave the chip idle -- the pixel-parallel form, its per-channel state in a workspace (300 x 450 x 3: 0.73 ->
        # 0.075 ms, 512 x 1024 x 3: 3.9 -> 0.10 ms).  Up to 128 channels it also beats the per-channel kernel's
        # channel-strided reads (150 x 225 x 64: 0.37 -> 0.21 ms); beyond that there are enough (image, channel) blocks
        nws = _lib.lib().nfs_hist_loss_wide_workspace_floats(B, Cn, HW, HWt)
        ws = conv_workspace(F.device, nws)
        _lib.call("nfs_hist_loss_wide", _ptr(F), _ptr(templ), _ptr(mask), _ptr(loss_acc), _ptr(g_acc), _ptr(ws), nws, B,
                  Bt, HW, HWt, Cn, float(weight), int(bool(relu_mask)), _stream())
        return g_acc
    if mask is not None:
        _lib.call("nfs_hist_loss_masked", _ptr(F), _ptr(templ), _ptr(mask), _ptr(loss_acc), _ptr(g_acc), B, Bt, HW, HWt,
                  Cn, float(weight), int(bool(relu_mask)), _stream())
        return g_acc
    _lib.call("nfs_hist_loss", _ptr(F), _ptr(templ), _ptr(loss_acc), _ptr(g_acc), B, Bt, HW, HWt, Cn, float(weight),
              int(bool(relu_mask)), _stream())
    return g_acc


def gram_bwd(F, Dmat, scale, scale_dev=None, relu_mask=True, out=None):
    B, Cn = F.shape[0], F.shape[-1]
    HW = F.numel() // (B * Cn)
    if out is None:
        out = _empty(F.shape, F)
    _lib.call("nfs_gram_bwd", _ptr(F), _ptr(Dmat), _ptr(out), B, HW, Cn, _ptr(scale_dev), float(scale),
              int(relu_mask), _stream())
    return out


def tv_loss(d_img, weight, loss_acc, g_acc=None):
    B, H, W, Cn = d_img.shape
    _lib.call("nfs_tv_loss", _ptr(d_img), _ptr(loss_acc), _ptr(g_acc), B, H, W, Cn, float(weight), _stream())


# ---- A8 -----------------------------------------------------------------------------

def make_splat_cfg(nd, res, domain, radius, support, rest_density, nsize, clip, mode):
    c = SplatCfg()
    c.nd = nd
    for k in range(3):
        c.res[k] = int(res[k]) if k < nd else 1
        c.domain[k] = float(domain[k]) if k < nd else 1.0
    c.radius = float(radius); c.support = float(support); c.rest_density = float(rest_density)
    c.nsize = int(nsize); c.clip = int(bool(clip)); c.mode = int(mode)
    return c


def p2g_fwd(p, cfg, attr=None, pd=None):
    """p [N,nd]; returns grid [res..., C] (mode 0/1) or (xsum, wsum) (mode 2)"""
    N = p.shape[0]
    Cn = 1 if attr is None else attr.shape[-1]
    res = [cfg.res[k] for k in range(cfg.nd)]
    grid = _zeros(tuple(res) + (Cn,), p)
    wsum = _zeros(tuple(res) + (1,), p) if cfg.mode == 2 else None
    _lib.call("nfs_p2g_fwd", _ptr(p), _ptr(attr), _ptr(pd), _ptr(grid), _ptr(wsum), N, Cn, C.byref(cfg), _stream())
    return (grid, wsum) if cfg.mode == 2 else grid


def p2g_bwd(p, cfg, g_grid, attr=None, pd=None, g_wsum=None, need_p=True, need_attr=False, need_pd=False):
    N = p.shape[0]
    Cn = 1 if attr is None else attr.shape[-1]
    g_p = _empty(p.shape, p) if need_p else None
    g_attr = _empty(attr.shape, p) if need_attr else None
    g_pd = _empty((N,), p) if need_pd else None
    _lib.call("nfs_p2g_bwd", _ptr(p), _ptr(attr), _ptr(pd), _ptr(g_grid), _ptr(g_wsum), _ptr(g_p), _ptr(g_attr),
              _ptr(g_pd), N, Cn, C.byref(cfg), _stream())
    return g_p, g_attr, g_pd


def p2g_has_instance(cfg):
    """whether the one-launch adjoint forms exist for this configuration (the library's own predicate)"""
    rc = _lib.lib().nfs_p2g_has_instance(C.byref(cfg))
    if rc < 0:
        raise _lib.NfsError("nfs_p2g_has_instance", rc, _lib.lib().nfs_last_error().decode())
    return bool(rc)


def p2g_wavg_bwd(p, cfg, xsum, wsum, g_out, attr, eps=1e-6, need_p=True, need_attr=True):
    """adjoint of the weighted-average splat in one launch (finish adjoint folded into the gather); None where the
    library has no such form for the configuration (nfs_p2g_has_instance: the caller takes p2g_wavg_finish_bwd +
    p2g_bwd)"""
    if not p2g_has_instance(cfg):
        return None
    N = p.shape[0]
    Cn = attr.shape[-1]
    g_p = _empty(p.shape, p) if need_p else None
    g_attr = _empty(attr.shape, p) if need_attr else None
    _lib.call("nfs_p2g_wavg_bwd", _ptr(p), _ptr(attr), _ptr(xsum), _ptr(wsum), _ptr(g_out), _ptr(g_p), _ptr(g_attr), N,
              Cn, float(eps), C.byref(cfg), _stream())
    return g_p, g_attr


def p2g_wavg_finish(xsum, wsum, eps=1e-6):
    Cn = xsum.shape[-1]
    n = wsum.numel()
    out = _empty(xsum.shape, xsum)
    _lib.call("nfs_p2g_wavg_finish", _ptr(xsum), _ptr(wsum), _ptr(out), n, Cn, float(eps), _stream())
    return out


def p2g_wavg_finish_bwd(xsum, wsum, g_out, eps=1e-6):
    Cn = xsum.shape[-1]
    n = wsum.numel()
    g_x = _empty(xsum.shape, xsum); g_w = _empty(wsum.shape, xsum)
    _lib.call("nfs_p2g_wavg_finish_bwd", _ptr(xsum), _ptr(wsum), _ptr(g_out), _ptr(g_x), _ptr(g_w), n, Cn,
              float(eps), _stream())
    return g_x, g_w


# ---- A10 ----------------------------------------------------------------------------

def _written(*tensors):
    """the kernels write through raw pointers: tell torch's version counters (views share them), so that anything keyed on
    ``tensor._version`` -- the stylizer's stored forward advect, autograd's saved-tensor checks -- sees the write"""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def adam_tf_step(x, m, v, g, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    _lib.call("nfs_adam_tf_step", _ptr(x), _ptr(m), _ptr(v), _ptr(g), x.numel(), float(lr_t), float(beta1),
              float(beta2), float(eps), _stream())
    _written(x, m, v)


def slab_pack(gpad, pack, D, world, cs):
    """send buffer of the D-slab reduce-scatter: pack [world, cs+5, H, W] <- overlapping plane ranges of gpad [D+5, H, W]
    (nfs_hip.h: nfs_slab_pack)"""
    assert gpad.is_contiguous() and pack.is_contiguous() and gpad.shape[0] == D + 5
    assert tuple(pack.shape) == (world, cs + 5) + tuple(gpad.shape[1:])
    _lib.call("nfs_slab_pack", _ptr(gpad), _ptr(pack), int(D), int(gpad[0].numel()), int(world), int(cs), _stream())
    return pack


def _iptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
    return t.data_ptr()


def colour_clamp_gather(var, order=None, out=None):
    """clip(var, 0, 1) read through a permutation (int64 [N], None = identity): var [N,C] -> [N,C]"""
    if out is None:
        out = _empty(var.shape, var)
    _lib.call("nfs_colour_clamp_gather", _ptr(var), _iptr(order), _ptr(out), var.shape[0], var.shape[1], _stream())
    return out


def clamp01_bwd(g, x, out=None):
    """adjoint of clip(x, 0, 1): g where 0 <= x <= 1, else 0"""
    if out is None:
        out = _empty(g.shape, g)
    _lib.call("nfs_clamp01_bwd", _ptr(g), _ptr(x), _ptr(out), g.numel(), _stream())
    return out


def colour_clamp_scatter_bwd(g_cc, var, order=None, out=None):
    """adjoint of colour_clamp_gather: g_var[order[i]] = g_cc[i] where 0 <= var[order[i]] <= 1, else 0"""
    g_var = _empty(var.shape, var) if out is None else out
    _lib.call("nfs_colour_clamp_scatter_bwd", _ptr(g_cc), _iptr(order), _ptr(var), _ptr(g_var), var.shape[0], var.shape[1],
              _stream())
    return g_var


def iterate_update(x, g_opt):
    """g_opt += nan_to_num(x) - g_opt (styler_2p.py:259-262) in place, and x <- the new g_opt"""
    assert x.shape == g_opt.shape
    _lib.call("nfs_iterate_update", _ptr(x), _ptr(g_opt), x.numel(), _stream())
    _written(x, g_opt)


def fill(x, value):
    _lib.call("nfs_fill", _ptr(x), float(value), x.numel(), _stream())


def axpy(y, x, a):
    _lib.call("nfs_axpy", _ptr(y), _ptr(x), float(a), x.numel(), _stream())


# ---- SURVEY 8(f)-1 -------------------------------------------------------------------

def g2p_fwd(g, p, cubic=True):
    """g [X,Y,(Z),C] cell-centred grid, p [N,nd] in [0,1] -> [N,C]  (transform.py:771-1231, forward only)"""
    nd = p.shape[-1]
    assert g.dim() == nd + 1 and nd in (2, 3)
    N, Cn = p.shape[0], g.shape[-1]
    out = _empty((N, Cn), g)
    X, Y = g.shape[0], g.shape[1]
    Z = g.shape[2] if nd == 3 else 1
    _lib.call("nfs_g2p_fwd", _ptr(g), _ptr(p), _ptr(out), nd, X, Y, Z, Cn, N, int(bool(cubic)), _stream())
    return out


# ---- particles moved by a displacement field on a carrier grid, and the transpose (include/nfs_carrier.h) -------------

def _carrier_dims(dims, nd):
    dims = [int(v) for v in dims]
    if nd not in (2, 3) or len(dims) != nd:
        raise ValueError("carrier: a grid of %d axes for positions of %d components (nd is 2 or 3)" % (len(dims), nd))
    return dims[0], dims[1], dims[2] if nd == 3 else 1


def carrier_displace(u, p, cubic=True, want_v=True):
    """u [X,Y,(Z),nd] cell-centred displacement field in the units of p, p [N,nd] in [0,1] -> (p + v, v) with
    v = g2p_fwd(u, p) bit for bit, in one launch; v is None unless ``want_v``"""
    nd = int(p.shape[-1])
    if u.dim() != nd + 1 or int(u.shape[-1]) != nd:
        raise ValueError("carrier_displace: u %s is not a field of %d-vectors on a %d-D grid for p %s"
                         % (tuple(u.shape), nd, nd, tuple(p.shape)))
    X, Y, Z = _carrier_dims(u.shape[:nd], nd)
    N = int(p.shape[0])
    p_out = _empty((N, nd), p)
    v = _empty((N, nd), p) if want_v else None
    _lib.call("nfs_carrier_displace", _ptr(u), _ptr(p), _ptr(p_out), _ptr(v), nd, X, Y, Z, N, int(bool(cubic)), _stream())
    return p_out, v


def carrier_bwd(g_v, p, dims, cubic=True, route=0, count=False):
    """g_v [N,C], p [N,nd] -> g_u [*dims,C]: the transpose of ``g2p_fwd`` in the grid, g_u[cell,c] = sum over the taps that
    land on the cell of w g_v[i,c].  Any particle order is correct; grid order (transform.grid_order) is fast: a block of
    256 consecutive particles sums the box of cells it touches in LDS and adds each once.  ``route`` 1: every block issues
    one global atomic per tap instead.  ``count``: also the number of blocks that took the box route (an int32 device
    tensor of one element)"""
    nd = int(p.shape[-1])
    X, Y, Z = _carrier_dims(dims, nd)
    N, Cn = int(p.shape[0]), int(g_v.shape[-1])
    if tuple(g_v.shape) != (N, Cn):
        raise ValueError("carrier_bwd: g_v %s is not [N,C] for p %s" % (tuple(g_v.shape), tuple(p.shape)))
    g_u = _empty(tuple(int(v) for v in dims) + (Cn,), p)
    n_box = torch.empty(1, dtype=torch.int32, device=p.device) if count else None
    _lib.call("nfs_carrier_bwd", _ptr(g_v), _ptr(p), _ptr(g_u), None if n_box is None else n_box.data_ptr(), nd, X, Y, Z, Cn,
              N, int(bool(cubic)), int(route), _stream())
    return (g_u, n_box) if count else g_u


# ---- particles carried along a flow of the carrier field, and the sweep back along the path (include/nfs_flow.h) --------

def _flow_dims(who, u, nd):
    if u.dim() != nd + 1 or int(u.shape[-1]) != nd:
        raise ValueError("%s: u %s is not a field of %d-vectors on a %d-D grid" % (who, tuple(u.shape), nd, nd))
    return _carrier_dims(u.shape[:nd], nd)


def flow_fwd(u, p, steps, cubic=True):
    """u [X,Y,(Z),nd] a velocity over one unit of pseudo-time on the carrier grid, p [N,nd] -> path [steps+1,N,nd]:
    path[0] = p, path[k+1] = path[k] + h g2p_fwd(u, path[k]) with h = 1 / steps, in one launch.  Bit for bit those
    operators (the float32 product h v, then the float32 sum); ``steps`` 1 gives ``carrier_displace``'s p_out as path[1]"""
    nd, K = int(p.shape[-1]), int(steps)
    X, Y, Z = _flow_dims("flow_fwd", u, nd)
    N = int(p.shape[0])
    path = _empty((max(K, 0) + 1, N, nd), p)
    _lib.call("nfs_flow_fwd", _ptr(u), _ptr(p), _ptr(path), nd, X, Y, Z, N, K, int(bool(cubic)), _stream())
    return path


def flow_bwd(u, path, g_out, cubic=True):
    """u, path [K+1,N,nd] of ``flow_fwd``, g_out [N,nd] the gradient in path[K] -> lam [K+1,N,nd]: lam[K] = g_out,
    lam[k] = lam[k+1] + h J(path[k])^T lam[k+1], one launch, a pure gather.  lam[0] is the gradient in p"""
    if path.dim() != 3 or int(path.shape[0]) < 2 or tuple(g_out.shape) != tuple(path.shape[1:]):
        raise ValueError("flow_bwd: path %s is not [K+1,N,nd] with K >= 1 for g_out %s [N,nd]"
                         % (tuple(path.shape), tuple(g_out.shape)))
    K, N, nd = (int(v) for v in path.shape)
    K -= 1
    X, Y, Z = _flow_dims("flow_bwd", u, nd)
    lam = _empty((K + 1, N, nd), path)
    _lib.call("nfs_flow_bwd", _ptr(u), _ptr(path), _ptr(g_out), _ptr(lam), nd, X, Y, Z, N, K, int(bool(cubic)), _stream())
    return lam


def flow_grad(u, path, g_out, cubic=True, route=0):
    """the gradients of a flow in its field and in its starting positions -> (g_u [like u], g_p [N,nd]): the sweep
    (``flow_bwd``), then g_u = h sum_k g2p^T(lam[k+1]; path[k]) as ONE ``carrier_bwd`` over the K N positions path[0:K]
    with the gradients lam[1:K+1] (contiguous slices; ``route`` is that call's) and one scale of the grid by h"""
    lam = flow_bwd(u, path, g_out, cubic=cubic)
    K, N, nd = int(path.shape[0]) - 1, int(path.shape[1]), int(path.shape[2])
    g_u = carrier_bwd(lam[1:].reshape(K * N, nd), path[:K].reshape(K * N, nd), tuple(u.shape[:nd]), cubic=cubic,
                      route=route)
    if K > 1:
        g_u.mul_(1.0 / K)
    return g_u, lam[0]



# ---- node types of the Inception-v1 loss network ------------------------------------------------------
# Operands are channel RANGES of contiguous [B,H,W,ld] buffers: (tensor, first channel, channels).

def _rows(t):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4):
        raise ValueError("expected a contiguous float32 CUDA tensor [B,H,W,ld]")
    return t


def same_out(n, k, stride):
    """TF SAME: (output size, padding before)"""
    out = -(-n // stride)
    return out, max((out - 1) * stride + k - n, 0) // 2


def conv2d_pack(w_hwio, transpose=False):
    """HWIO filters -> the layout ``conv2d_fwd`` reads; ``transpose``: the data-gradient filters of a stride-1 conv"""
    w = w_hwio.contiguous()
    kh, kw, Ci, Co = w.shape
    n = _lib.lib().nfs_conv2d_packed_floats(kh, kw, Ci, Co, int(transpose))
    packed = _empty((n,), w)
    _lib.call("nfs_conv2d_pack", _ptr(w), _ptr(packed), kh, kw, Ci, Co, int(transpose), _stream())
    return packed


def conv2d_fwd(x, cx, Cin, packed, bias, y, cy, Cout, kh, kw, stride=1, relu=True, y_pre=None, cp=0, x_mask=None, cm=0,
               accumulate=False):
    """y[..., cy:cy+Cout] (+)= relu(conv_SAME(x[..., cx:cx+Cin] * (x_mask[..., cm:cm+Cin] > 0)) + bias);
    y_pre[..., cp:cp+Cout] = the value before the ReLU"""
    _rows(x), _rows(y)
    B, H, W, ldx = x.shape
    Ho, _ = same_out(H, kh, stride)
    Wo, _ = same_out(W, kw, stride)
    assert tuple(y.shape[:3]) == (B, Ho, Wo), (tuple(y.shape), (B, Ho, Wo))
    assert cx + Cin <= ldx and cy + Cout <= y.shape[3]
    xm = None if x_mask is None else _rows(x_mask).data_ptr() + 4 * cm
    yp = None if y_pre is None else _rows(y_pre).data_ptr() + 4 * cp
    if x_mask is not None:
        assert tuple(x_mask.shape[:3]) == (B, H, W) and cm + Cin <= x_mask.shape[3]
    if y_pre is not None:
        assert tuple(y_pre.shape[:3]) == (B, Ho, Wo) and cp + Cout <= y_pre.shape[3]
    nws = _lib.lib().nfs_conv2d_workspace_floats(B, H, W, Cin, Cout, kh, kw, stride)
    ws = conv_workspace(x.device, nws) if nws > 0 else None     # shared scratch (calls on one stream are ordered)
    _lib.call("nfs_conv2d_fwd", x.data_ptr() + 4 * cx, ldx, xm, 0 if x_mask is None else x_mask.shape[3], _ptr(packed),
              _ptr(bias), y.data_ptr() + 4 * cy, y.shape[3], yp, 0 if y_pre is None else y_pre.shape[3], B, H, W, Cin,
              Cout, kh, kw, stride, int(relu), int(accumulate), _ptr(ws), 0 if ws is None else ws.numel(), _stream())
    return y


_group_ws = {}


def conv2d_group(problems):
    """Several stride-1 SAME convolutions of one batch in one launch.  ``problems``: dicts with the arguments of
    ``conv2d_fwd`` (x, cx, Cin, packed, bias, y, cy, Cout, k, relu, y_pre, cp, x_mask, cm, accumulate) and
    ``sum_with_prev`` (added to the previous problem's result: same pixels, Cout and output range)"""
    arr, n, B = conv2d_group_descs(problems)
    x = problems[0]["x"]
    key = (B,) + tuple((q.H, q.W, q.Cin, q.Cout, q.kh, q.sum_with_prev) for q in arr)
    nws = _group_ws.get(key)
    if nws is None:
        nws = _lib.lib().nfs_conv2d_group_workspace_floats(arr, n, B)
        if nws < 0:
            _lib.call("nfs_conv2d_group", arr, n, B, None, 0, _stream())     # raises with the planner's message
        _group_ws[key] = nws
    ws = conv_workspace(x.device, nws) if nws > 0 else None
    if _lib.PROFILE is not None:                          # (bench: the shapes behind this call's event pair)
        _lib.PROFILE.setdefault("shapes:nfs_conv2d_group", []).append(
            [(B, q.H, q.W, q.Cin, q.Cout, q.kh, q.kw) for q in arr])
    _lib.call("nfs_conv2d_group", arr, n, B, _ptr(ws), 0 if ws is None else ws.numel(), _stream())


def conv2d_group_descs(problems):
    """(descriptor array, n, B) of the problems of ``conv2d_group``"""
    n = len(problems)
    arr = (_lib.ConvDesc * n)()
    B = problems[0]["x"].shape[0]
    for q, pr in zip(arr, problems):
        x, y = _rows(pr["x"]), _rows(pr["y"])
        assert x.shape[0] == B and tuple(y.shape[:3]) == tuple(x.shape[:3])
        cx, cy, Cin, Cout = pr.get("cx", 0), pr.get("cy", 0), pr["Cin"], pr["Cout"]
        assert cx + Cin <= x.shape[3] and cy + Cout <= y.shape[3]
        xm, yp = pr.get("x_mask"), pr.get("y_pre")
        q.x, q.ldx = x.data_ptr() + 4 * cx, x.shape[3]
        q.y, q.ldy = y.data_ptr() + 4 * cy, y.shape[3]
        q.x_mask, q.ldm = (None, 0) if xm is None else (_rows(xm).data_ptr() + 4 * pr.get("cm", 0), xm.shape[3])
        q.y_pre, q.ldp = (None, 0) if yp is None else (_rows(yp).data_ptr() + 4 * pr.get("cp", 0), yp.shape[3])
        q.packed, q.bias = _ptr(pr["packed"]), _ptr(pr.get("bias"))
        q.H, q.W, q.Cin, q.Cout, q.kh, q.kw = x.shape[1], x.shape[2], Cin, Cout, pr["k"], pr["k"]
        q.relu, q.accumulate = int(bool(pr.get("relu", True))), int(bool(pr.get("accumulate", False)))
        q.sum_with_prev = int(bool(pr.get("sum_with_prev", False)))
    return arr, n, B


def conv2d_plan(B, H, W, Cin, Cout, kh, kw, stride=1):
    """which instance ``conv2d_fwd`` runs for these shapes and how it cuts K (``ksplit``: with the workspace that
    ``conv2d_fwd`` passes), by the launch code's own rules; launches nothing"""
    buf = (C.c_int * 8)()
    _lib.call("nfs_conv2d_plan", B, H, W, Cin, Cout, kh, kw, stride, C.addressof(buf))
    return dict(zip(("bm", "cmode", "ksplit", "cps", "nchunks", "cchunks", "mtiles", "ntiles"), buf))


def conv2d_group_plan(descs, B):
    """how ``conv2d_group`` lays out a descriptor array (``conv2d_group_descs``): per problem ksplit, cps, partial,
    zbase, ztotal and its position in the launch order; launches nothing, raises with the planner's refusal"""
    n = len(descs)
    buf = (C.c_int * (6 * n))()
    _lib.call("nfs_conv2d_group_plan", descs, n, B, C.addressof(buf))
    return [dict(zip(("ksplit", "cps", "partial", "zbase", "ztotal", "position"), buf[6 * j:6 * j + 6])) for j in range(n)]


def conv2d_dgrad_small(gy, cg, Co, w_hwio, in_hw, stride, y_act=None, ca=0):
    """data gradient of a convolution with <= 4 input channels down to the image [B,H,W,Ci]"""
    _rows(gy)
    kh, kw, Ci, Co_w = w_hwio.shape
    assert Co_w == Co
    B = gy.shape[0]
    H, W = in_hw
    assert tuple(gy.shape[1:3]) == (same_out(H, kh, stride)[0], same_out(W, kw, stride)[0])
    gx = _empty((B, H, W, Ci), gy)
    ya = None if y_act is None else _rows(y_act).data_ptr() + 4 * ca
    _lib.call("nfs_conv2d_dgrad_small", gy.data_ptr() + 4 * cg, gy.shape[3], ya, 0 if y_act is None else y_act.shape[3],
              _ptr(w_hwio.contiguous()), _ptr(gx), B, H, W, Ci, Co, kh, kw, stride, _stream())
    return gx


def maxpool3_fwd(x, stride):
    """3x3 SAME max pool over every float of the rows: (y [B,Ho,Wo,ld], arg uint8 [B,Ho,Wo,ld])"""
    _rows(x)
    B, H, W, ld = x.shape
    Ho, Wo = same_out(H, 3, stride)[0], same_out(W, 3, stride)[0]
    y = _empty((B, Ho, Wo, ld), x)
    arg = torch.empty((B, Ho, Wo, ld), dtype=torch.uint8, device=x.device)
    _lib.call("nfs_maxpool3_fwd", _ptr(x), _ptr(y), arg.data_ptr(), B, H, W, ld, stride, _stream())
    return y, arg


def maxpool3_bwd(gy, arg, in_hw, stride, gx=None, relu_of=None):
    """gx (+)= the pool adjoint; ``gx`` given: accumulate into it; ``relu_of`` (the pooled tensor, a ReLU output): the
    result also carries that ReLU's adjoint"""
    _rows(gy)
    B, Ho, Wo, ld = gy.shape
    H, W = in_hw
    acc = gx is not None
    if gx is None:
        gx = _empty((B, H, W, ld), gy)
    assert tuple(gx.shape) == (B, H, W, ld) and arg.dtype == torch.uint8 and arg.is_contiguous()
    assert relu_of is None or tuple(relu_of.shape) == tuple(gx.shape)
    _lib.call("nfs_maxpool3_bwd", _ptr(gy), arg.data_ptr(), _ptr(gx), B, H, W, ld, stride, int(acc), _ptr(relu_of),
              _stream())
    return gx


def lrn_fwd(x, C, radius, bias, alpha, beta):
    """tf.nn.lrn over the first C channels of the rows: (y, scale), both shaped like x (padding channels zero)"""
    _rows(x)
    ld = x.shape[3]
    y = _zeros(x.shape, x) if ld > C else _empty(x.shape, x)
    scale = _empty(x.shape, x)
    _lib.call("nfs_lrn_fwd", _ptr(x), _ptr(y), _ptr(scale), x.numel() // ld, C, ld, int(radius), float(bias),
              float(alpha), float(beta), _stream())
    return y, scale


def lrn_bwd(x, y, scale, gy, C, radius, alpha, beta, gx=None):
    _rows(gy)
    ld = x.shape[3]
    acc = gx is not None
    if gx is None:
        gx = _zeros(x.shape, x) if ld > C else _empty(x.shape, x)
    _lib.call("nfs_lrn_bwd", _ptr(x), _ptr(y), _ptr(scale), _ptr(gy), _ptr(gx), x.numel() // ld, C, ld, int(radius),
              float(alpha), float(beta), int(acc), _stream())
    return gx


def avgpool_valid_fwd(x, k):
    """k x k average pool, stride 1, VALID, over every float of the rows"""
    _rows(x)
    B, H, W, ld = x.shape
    y = _empty((B, H - k + 1, W - k + 1, ld), x)
    _lib.call("nfs_avgpool_valid_fwd", _ptr(x), _ptr(y), B, H, W, ld, int(k), _stream())
    return y


def avgpool_valid_bwd(gy, in_hw, k, gx=None):
    _rows(gy)
    B, _, _, ld = gy.shape
    H, W = in_hw
    acc = gx is not None
    if gx is None:
        gx = _empty((B, H, W, ld), gy)
    _lib.call("nfs_avgpool_valid_bwd", _ptr(gy), _ptr(gx), B, H, W, ld, int(k), int(acc), _stream())
    return gx


def relu_mask_add(g, cg, act, ca, addend, cadd, C, out=None, co=0):
    """out[..., co:co+C] = g[..., cg:cg+C] * (act[..., ca:ca+C] > 0) + addend[..., cadd:cadd+C]; g / act / addend may
    be None"""
    ref = g if g is not None else addend
    _rows(ref)
    npix = ref.numel() // ref.shape[3]
    if out is None:
        out = _empty(tuple(ref.shape[:3]) + (C,), ref)
        co = 0

    def at(t, c):
        return (None, 0) if t is None else (_rows(t).data_ptr() + 4 * c, t.shape[3])
    (pg, lg), (pa, la), (pd, ldd) = at(g, cg), at(act, ca), at(addend, cadd)
    _lib.call("nfs_relu_mask_add", pg, lg, pa, la, pd, ldd, out.data_ptr() + 4 * co, out.shape[3], npix, C, _stream())
    return out

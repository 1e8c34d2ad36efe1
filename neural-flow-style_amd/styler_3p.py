"""3-D particle stylizer -- host-side mirror of the reference's ``styler_3p.Styler``
(styler_3p.py:14-439): same constructor / ``run(params) -> dict`` surface and the same
outer loop (octaves x iterations x frame batches x views, TF-Adam per ``opt_id``, update
masking, temporal Gaussian smoothing of the per-particle updates, frame interpolation,
final inference), driving the HIP kernels instead of a TF-1.15 graph.

Forward graph per frame (styler_3p.py:42-164):
  'd': r + clip(r_opt,-1,1) -> sum_k p2g_wavg(p, r_k, support / kernel_scale^k)
  'p': p + v              -> p2g(p) / rest_density        (+ pressure loss, 96-98)
  'c': the grey field of 'p' at zero displacement absorbs, q = p2g(p, pc=clip(c,0,1), pd=r) [D,H,W,3] emits
       (transform.py:1429-1441, the colour branch of the 3-D splat that no reference driver calls); the colour image
       of a view is clip(sum_z T/M rotate(q), 0, 1) -> x255 -> loss network: ``engine.ColourRenderLoss`` (build
       extension; conventions of styler_2p).  ``--colour_render liquid``: the image is
       clip(sum_z w rotate(q) + t bg, 0, 1), front-to-back alpha compositing over ``--colour_background`` (w, t:
       include/nfs_liquid.h); 'r' and 'd_intm' are then over the background.  ``--colour_render exposure``: the smoke
       model with the fixed exposure ``--colour_exposure`` in place of the maximum M (include/nfs_exposure.h), over black.
       The grey volume is smoothed by k and q is not, so rotate(q) / rotate(d) can exceed the particles' colour and the
       clip takes it
  'pc': positions AND colours of a liquid (or, with ``--colour_render exposure``, of smoke) in one variable [N,6] =
       (v, c / colour_lr_scale) (build extension): the grey field of 'p' at p + v absorbs, q = p2g(p + v, pc=clip(c,0,1), pd=r) emits, the image is the
       liquid colour render's or the fixed-exposure smoke render's (``--colour_render liquid`` / ``exposure``; the
       weights of the latter are one launch, ``ops.exposure_weights``).  The geometry moves, so nothing of a frame is
       kept across steps but its densities r and the splat configurations: an evaluation forms the ray weights, and
       ``engine.ColourRenderLoss.loss_and_grad(absorb=True)`` returns the gradient in the emission AND in the absorbing
       volume (include/nfs_absorb.h, include/nfs_exposure.h); both reach the positions through the splat's adjoint.  One
       optimiser step of ``lr`` moves a colour by ``colour_lr_scale * lr``.  ``w_pressure`` acts as for 'p'; ``style_mask`` and the max-normalised
       smoke colour render ('' / 'smoke') are refused (the mask and the maximum would depend on the variable)
  'g': the 'p' path with the displacement sampled from a CARRIER GRID (build extension; the reference
       has no such path): the variable of a key frame is u [Gd,Gh,Gw,3] (``--carrier_resolution``), a displacement field
       in the units of p, cell-centred over the whole domain, starting at zero or at ``params['u_init'][t]``;
       p' = p + g2p(u, p) (``--carrier_interp`` cubic / linear, one launch: ``ops.carrier_displace``), then splat, smooth,
       views, render, loss network and ``w_pressure`` exactly as for 'p'.  The gradient in the displacements reaches u
       through the transpose of the sampling (``ops.carrier_bwd``, include/nfs_carrier.h).  The variable has one shape
       whatever a frame holds, so the frames of a sequence may hold DIFFERENT particle sets (each in its own grid order,
       returned in the caller's), the sampling kernel ties neighbouring particles together, and the result moves any
       particle set (``Styler.apply_carrier``).  Temporal smoothing, ``interp`` and ``frames_per_opt`` act on the grids
       in place: there is NO transport between frames (particle ``params`` carry no grid velocity), a frame's field is
       filtered with its neighbours' cell by cell.  The carrier resolution is the same at every octave and u is in domain
       units, so it carries over unchanged.  ``result['opt']`` are the fields, ``result['v']`` the sampled per-particle
       displacements, ``result['p']`` = p + v.  ``w_density`` and a process group are refused.
       ``--carrier_steps`` K > 1 (include/nfs_flow.h): the one-sample map folds once grad u reaches about 1 per unit of p
       (particles cross, pile up and leave holes), so u becomes a VELOCITY over one unit of pseudo-time and the particles
       are carried through it in K explicit Euler steps of 1 / K, path[k+1] = path[k] + g2p(u, path[k]) / K
       (``T.carrier_flow``, one launch: ``ops.flow_fwd``); the gradient sweeps the stored path back
       (``ops.flow_bwd``: lam[k] = lam[k+1] + J(path[k])^T lam[k+1] / K, the Jacobian of the sampling in the position)
       and reaches u through ONE transpose over the K N positions of the path (``ops.flow_grad``).  ``result['p']`` =
       path[K], ``result['v']`` = path[K] - p, ``apply_carrier`` integrates with the same K: a field stylised at K must
       be applied at that K, and K = 1 is the displacement above, launch for launch.  Euler steps only; with another
       ``target_field`` K > 1 is refused
  -> 3x3x3 smoothing conv -> max(.,0) = d_out -> [rotate] -> render -> max-normalise
  -> x255, grey->3ch = d_img -> VGG-19 -> Gram style loss (+TV).
The particle side runs through ``torch.autograd`` (custom Functions wrapping the splat
kernels); the render/VGG/loss side is the explicit ``engine.RenderStyleLoss`` chain.

Differences from the reference, all deliberate and documented:
  * ``views_mode='sum'`` (build extension): one Adam step on the gradient of the summed view
    losses; the reference-faithful default is ``'sequential'`` (one step per view-batch, iterates
    averaged, styler_3p.py:326-352).
  * the sqrt in the SPH kernel has zero gradient at 0 (analytic limit) instead of NaN-then-
    ``nan_to_num`` (styler_3p.py:337,340,360).
  * ``batch_size`` must be 1 (as every reference driver sets it): with batch_size>1 the reference
    couples the frames of a batch through the global max of the render (styler_3p.py:158).
"""
from __future__ import annotations

import numpy as np
import torch

from . import engine, ops, parallel
from . import transform as T
from . import vgg as vggmod
from .config import check_carrier, check_carrier_steps, check_colour_render, check_optimizer, colour_exposure
from .styler_base import StylerBase
from .util import temporal_weights


class _SmoothRelu(torch.autograd.Function):
    """conv3d SAME with [1,k,1]^3/(k+2)^3 then tf.maximum(d,0) (styler_3p.py:112-125)"""

    @staticmethod
    def forward(ctx, d, k):
        out = ops.smooth3d_relu_fwd(d.contiguous().reshape(d.shape[1:4]), k)
        ctx.k = k
        ctx.save_for_backward(out)
        ctx.shape = d.shape
        return out.reshape(d.shape)

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        gd = ops.smooth3d_relu_bwd(out, g.contiguous().reshape(out.shape), ctx.k)
        return gd.reshape(ctx.shape), None


class Styler(StylerBase):
    _colour = False                                  # target_field 'c' (set by the constructor)
    _joint = False                                   # target_field 'pc' (set by the constructor)
    _carrier = False                                 # target_field 'g' (set by the constructor)
    _carrier_steps = 1                               # carrier_steps of 'g' (set by the constructor)

    def __init__(self, self_dict):
        check_optimizer(self_dict, grid=False)
        check_colour_render(self_dict, colour=getattr(self_dict, "target_field", "") in ("c", "pc"))
        if getattr(self_dict, "target_field", "") == "pc":
            self._check_joint(self_dict)
        if getattr(self_dict, "target_field", "") == "g":
            self._check_carrier(self_dict)
        steps = check_carrier_steps(self_dict)
        if steps > 1 and getattr(self_dict, "target_field", "") != "g":
            raise ValueError("--carrier_steps %d with target_field %r: the steps are those of the carrier flow, which "
                             "belongs to --target_field g (pass --carrier_steps 1)"
                             % (steps, getattr(self_dict, "target_field", "")))
        if getattr(self_dict, "target_field", "") == "c":
            # the colour path renders by emission-absorption only and has no auxiliary field terms (refused before the
            # base class loads a network)
            if getattr(self_dict, "render_liquid", False):
                raise ValueError("target_field 'c': render_liquid is the grey liquid render and is not built for the "
                                 "colour render (pass --render_liquid false; the liquid colour render is "
                                 "--colour_render liquid)")
            if getattr(self_dict, "ray_mode", ""):
                raise ValueError("target_field 'c': ray_mode %r is not built for the colour render (leave --ray_mode empty)"
                                 % (self_dict.ray_mode,))
            if (getattr(self_dict, "w_pressure", 0) or 0) > 0:
                raise ValueError("target_field 'c': w_pressure acts on moved positions and the colours move none (pass "
                                 "--w_pressure 0)")
            if (getattr(self_dict, "w_density", 0) or 0) > 0:
                raise ValueError("target_field 'c': w_density acts on the density variable (pass --w_density 0)")
            if getattr(self_dict, "style_mask_on_ref", False):
                raise ValueError("target_field 'c': style_mask_on_ref is not built for the colour render (pass "
                                 "--style_mask_on_ref false)")
        StylerBase.__init__(self, self_dict)
        assert self.batch_size == 1, "batch_size > 1 is not supported (see module docstring)"
        self._colour = self.target_field == "c"
        self._joint = self.target_field == "pc"
        self._carrier = self.target_field == "g"
        if self._carrier:
            self.carrier_resolution, self._carrier_cubic = check_carrier(self)
            self._carrier_steps = steps
        if self.rotate:
            self.rot_mat_, self.views = T.rot_mat(self.phi0, self.phi1, self.phi_unit, self.theta0, self.theta1,
                                                  self.theta_unit, sample_type=self.sample_type, rng=self.rng,
                                                  nv=self.n_views)
            if self.n_views is None:
                self.n_views = len(self.views)
            print("# vps:", self.n_views)
            assert self.n_views % self.v_batch == 0
        # one loss chain per stylizer: the grey render's, or for 'c' the colour render's around an image loss
        self.loss = None if (self._colour or self._joint) else self._make_loss(rotate=self.rotate)
        self.colour = self._make_colour_loss() if (self._colour or self._joint) else None
        self._graph_loss = None                      # engine.GraphedLoss, decided at the first loss call
        self._identity = T.rot_to_device([np.identity(3)], self.device)
        # multi-GPU (set by the driver): ``pg`` = the process group; ``shard_by`` = 'views' (views=sum: the views of every
        # frame over the ranks, ONE all-reduce of the variable's gradient + loss per frame step) or 'frames' (SURVEY 8(e)
        # "Frames (config 4/5)": contiguous blocks of key frames per rank, full view batches per rank, and the only
        # exchange is the halo of per-frame updates the temporal filter reaches, point-to-point)
        self.pg = None
        self.shard_by = getattr(self, "shard_by", None) or "views"

    @staticmethod
    def _check_joint(cfg):
        """the refusals of target_field 'pc', before the base class loads a network: a ValueError naming the flag"""
        if (getattr(cfg, "colour_render", "") or "") not in ("liquid", "exposure"):
            raise ValueError("target_field 'pc': colour_render %r -- the joint variable moves the density, and only the "
                             "liquid and the fixed-exposure colour renders have an adjoint in it: the smoke render's "
                             "maximum couples every ray (pass --colour_render liquid, or --colour_render exposure for smoke)"
                             % (getattr(cfg, "colour_render", ""),))
        if getattr(cfg, "style_mask", False):
            raise ValueError("target_field 'pc': style_mask -- the mask 1 - t would depend on the variable and the "
                             "gradient through it is not built (pass --style_mask false)")
        if getattr(cfg, "render_liquid", False):
            raise ValueError("target_field 'pc': render_liquid is the grey liquid render and is not built for the colour "
                             "render (pass --render_liquid false; the liquid colour render is --colour_render liquid)")
        if getattr(cfg, "ray_mode", ""):
            raise ValueError("target_field 'pc': ray_mode %r is not built for the colour render (leave --ray_mode empty)"
                             % (cfg.ray_mode,))
        if (getattr(cfg, "w_density", 0) or 0) > 0:
            raise ValueError("target_field 'pc': w_density acts on the density variable (pass --w_density 0)")
        if getattr(cfg, "style_mask_on_ref", False):
            raise ValueError("target_field 'pc': style_mask_on_ref is not built for the colour render (pass "
                             "--style_mask_on_ref false)")
        if getattr(cfg, "pg", None) is not None:
            raise ValueError("target_field 'pc' over a process group (pg): sharding the colour path over ranks is not "
                             "built (run it on one GPU)")
        scale = getattr(cfg, "colour_lr_scale", 1.0)
        if not float(1.0 if scale is None else scale) > 0:
            raise ValueError("--colour_lr_scale %r: the step of a colour relative to a displacement must be positive"
                             % (scale,))

    @staticmethod
    def _check_carrier(cfg):
        """the refusals of target_field 'g', before the base class loads a network: a ValueError naming the flag"""
        check_carrier(cfg)
        if (getattr(cfg, "w_density", 0) or 0) > 0:
            raise ValueError("target_field 'g': w_density acts on the density variable (pass --w_density 0)")
        if getattr(cfg, "pg", None) is not None:
            raise ValueError("target_field 'g' over a process group (pg): sharding the carrier grid over ranks is not "
                             "built (run it on one GPU)")

    @property
    def _moves(self):
        """the variable moves the positions: 'p', 'pc' (its displacement columns) and 'g' (the carrier grid sampled at
        the particles)"""
        return "p" in self.target_field or self._carrier

    def apply_carrier(self, u, p):
        """a result of target_field 'g' applied to ANY particle set: u [Gd,Gh,Gw,3] (an entry of result['opt']), p [N,3]
        in the normalised domain, array order -> p + g2p(u, p) with this stylizer's ``carrier_interp``, or with
        ``carrier_steps`` K > 1 the end of the K-step flow through u (``ops.flow_fwd``) -- a field stylised at K means
        that map and no other; numpy in, numpy out (device tensors stay on the device).  That is how a field stylised on
        a low-resolution set reaches a resampled one"""
        cubic, steps = check_carrier(self)[1], check_carrier_steps(self)
        as_np = not torch.is_tensor(p)
        u_, p_ = (x.to(self.device).float().contiguous() if torch.is_tensor(x) else self._dev(x) for x in (u, p))
        if steps == 1:
            out = ops.carrier_displace(u_, p_, cubic=cubic, want_v=False)[0]
        else:
            out = ops.flow_fwd(u_, p_, steps, cubic=cubic)[steps]
        return out.cpu().numpy() if as_np else out

    def _make_colour_loss(self):
        w_layers = list(self.w_style_layer)
        if len(w_layers) == 1 and len(self.style_layer) > 1:
            w_layers = w_layers * len(self.style_layer)
        image_loss = engine.ImageStyleLoss(self.net, self.style_layer, w_layers, self.w_style, w_tv=self.w_tv,
                                           resize_scale=self.resize_scale, style_mask=getattr(self, "style_mask", False),
                                           w_content=getattr(self, "w_content", 0),
                                           content_layer=getattr(self, "content_layer", None),
                                           content_channel=getattr(self, "content_channel", 0),
                                           w_content_amp=getattr(self, "w_content_amp", 100),
                                           w_hist=getattr(self, "w_hist", 0), hist_layer=getattr(self, "hist_layer", ()),
                                           w_hist_layer=getattr(self, "w_hist_layer", ()))
        render, background = check_colour_render(self, colour=True)
        return engine.ColourRenderLoss(image_loss, self.transmit, self.v_batch if self.rotate else 1, render=render,
                                       background=background,
                                       exposure=colour_exposure(getattr(self, "colour_exposure", 1.0)))

    # ---- the colour path (target_field 'c'): what a step does not change is formed once -------------------------
    _COLOUR_CTX_FLOATS = 1 << 30          # ray weights kept across steps (4 GiB); beyond it a context is formed per call

    def _colour_frame(self, p, r, res):
        """the frame's constants for this octave: its grid order, positions and densities in that order, the splat
        configuration and the grey volume d [D,H,W] (the 'p' path at zero displacement)"""
        frames = self.__dict__.setdefault("_cframes", {})
        key = (p.data_ptr(), p.shape[0], tuple(res))
        if key not in frames:
            order = self.__dict__.get("_orders", {}).get((p.data_ptr(), p.shape[0]))
            with torch.no_grad():
                _, d_out, _ = self._field(p, None, None, res)
            pp, rr = (p, r) if order is None else (p[order].contiguous(), r[order].contiguous())
            cfg = ops.make_splat_cfg(3, list(res), list(self.domain), self.radius, self.support, self.rest_density,
                                     self.nsize, self.clip, 1)
            frames[key] = {"order": order, "p": pp, "r": rr.reshape(-1).contiguous(), "cfg": cfg,
                           "d3": d_out.detach().reshape(d_out.shape[1:4]).contiguous(), "ctx": {}}
        return frames[key]

    def _colour_ctx(self, fr, rot):
        """ray weights, grey image and mask of a frame for one view set: kept until the views are re-sampled (the set is
        identified by its matrices' device buffer: ``_rot`` caches them per slice of the current view list)"""
        key = (rot.data_ptr(), int(rot.shape[0]))
        ctx = fr["ctx"].get(key)
        if ctx is None:
            ctx = self.colour.prepare(fr["d3"], rot)
            held = self.__dict__.get("_cctx_floats", 0) + ctx["w"].numel()
            if held <= self._COLOUR_CTX_FLOATS:
                ctx["held"] = rot                    # (keeps the key's address alive as long as the entry)
                fr["ctx"][key] = ctx
                self._cctx_floats = held
        return ctx

    def _colour_volume(self, fr, var):
        cc = ops.colour_clamp_gather(var.contiguous(), fr["order"])
        return cc, ops.p2g_fwd(fr["p"], fr["cfg"], attr=cc, pd=fr["r"])

    def _colour_value_and_grad(self, p, r, var, res, rot):
        """per-view losses and d loss / d c of one frame: clamp -> splat -> ColourRenderLoss -> splat adjoint -> clamp
        adjoint, on the C-ABI operators (as styler_2p's explicit chain)"""
        fr = self._colour_frame(p, r, res)
        ctx = self._colour_ctx(fr, rot)
        cc, q = self._colour_volume(fr, var)
        losses, g_q = self.colour.loss_and_grad(q, ctx)
        _, g_cc, _ = ops.p2g_bwd(fr["p"], fr["cfg"], g_q, attr=cc, pd=fr["r"], need_p=False, need_attr=True)
        return losses, ops.colour_clamp_scatter_bwd(g_cc, var.contiguous(), fr["order"])

    def _colour_d_img(self, p, r, var, res):
        """the colour image at the identity view, [1,H',W',3] 0..255"""
        fr = self._colour_frame(p, r, res)
        return self.colour.d_img(self._colour_volume(fr, var)[1], self._colour_ctx(fr, self._identity))

    def _colour_reset(self, views_only=False):
        for fr in self.__dict__.get("_cframes", {}).values():
            fr["ctx"] = {}
        self._cctx_floats = 0
        self._rot_cache = {}
        if not views_only:
            self._cframes = {}

    # ---- the joint path (target_field 'pc'): the geometry moves, nothing but r and the splat cfgs outlives a call ----
    def _joint_cfgs(self, res):
        cfgs = self.__dict__.setdefault("_jcfgs", {})
        key = tuple(res)
        if key not in cfgs:
            mk = lambda rho, mode: ops.make_splat_cfg(3, list(res), list(self.domain), self.radius, self.support, rho,
                                                      self.nsize, self.clip, mode)
            cfgs[key] = (mk(1.0, 0), mk(self.rest_density, 1))     # (unit rest density: d / rest_density, as _field)
        return cfgs[key]

    def _joint_forward(self, p, r, var, res):
        """positions x = p + v in their grid order o, the raw and the smoothed grey volume, the clamped colours in that
        order and the emission q; var [N,6] = (v, c / colour_lr_scale)"""
        cfg_d, cfg_q = self._joint_cfgs(res)
        x = p + var[:, 0:3]
        order = self._particle_order(p, x.unsqueeze(0))
        xo = (x if order is None else x[order]).contiguous()
        ro = (r if order is None else r[order]).reshape(-1).contiguous()
        c = (var[:, 3:6] * float(self.colour_lr_scale)).contiguous()
        d_raw = ops.p2g_fwd(xo, cfg_d)[..., 0].contiguous()
        e = ops.smooth3d_relu_fwd(d_raw, float(self.k) if self.k > 0 else 0.0)
        cc = ops.colour_clamp_gather(c, order)
        q = ops.p2g_fwd(xo, cfg_q, attr=cc, pd=ro)
        return dict(x=x, order=order, xo=xo, ro=ro, c=c, d_raw=d_raw, e=e, cc=cc, q=q, cfg_d=cfg_d, cfg_q=cfg_q)

    def _joint_value_and_grad(self, p, r, var, res, rot):
        """per-view losses and d loss / d var [N,6] of one frame on the C-ABI operators: splats -> smoothing -> liquid
        weights -> ColourRenderLoss(absorb=True) -> smoothing adjoint -> the two splat adjoints -> clamp adjoint"""
        s = float(self.colour_lr_scale)
        f = self._joint_forward(p, r, var.contiguous(), res)
        ctx = self.colour.prepare(f["e"], rot)
        losses, g_q, g_e = self.colour.loss_and_grad(f["q"], ctx, absorb=True)
        g_raw = ops.smooth3d_relu_bwd(f["e"], g_e.contiguous(), float(self.k) if self.k > 0 else 0.0)
        if self.w_pressure > 0:
            # the mean over ALL voxels of (d_raw - 1)^2 where d_raw > 0, as _field forms it (styler_base.py:228-230)
            d_raw = f["d_raw"]
            pressure = torch.where(d_raw > 0, d_raw - 1, torch.zeros_like(d_raw))
            losses = losses + (pressure ** 2).mean() * self.w_pressure / losses.numel()
            g_raw = g_raw + pressure * (2.0 * self.w_pressure / d_raw.numel())
        g_x, g_cc, _ = ops.p2g_bwd(f["xo"], f["cfg_q"], g_q.contiguous(), attr=f["cc"], pd=f["ro"], need_p=True,
                                   need_attr=True)
        g_xd, _, _ = ops.p2g_bwd(f["xo"], f["cfg_d"], g_raw.unsqueeze(-1).contiguous(), need_p=True)
        g_x = g_x + g_xd
        g = torch.empty_like(var)
        if f["order"] is None:
            g[:, 0:3] = g_x
        else:
            g[f["order"], 0:3] = g_x
        g_c = ops.colour_clamp_scatter_bwd(g_cc, f["c"], f["order"])
        g[:, 3:6] = g_c if s == 1.0 else g_c * s
        return losses, g

    def _joint_d_img(self, p, r, var, res):
        """the colour image at the identity view, [1,H',W',3] 0..255 (over the background)"""
        f = self._joint_forward(p, r, var.contiguous(), res)
        return self.colour.d_img(f["q"], self.colour.prepare(f["e"], self._identity))

    # ---- forward graph: variable -> d_out [1,D,H,W,1] (autograd) ---------------------------------
    def _field(self, p, r, var, res):
        """p [N,3], r [N,nk] device tensors; var = the optimised tensor ([N,3] or [N,nk]).
        Returns (positions, d_out, extra) with extra = the auxiliary loss terms on the field / variable
        (pressure loss, styler_base.py:226-230; density-preservation loss, styler_base.py:215-223) or None"""
        pressure = None
        extra = None
        p_ = p.unsqueeze(0)
        if self._carrier:
            # ('g': the carrier grid sampled at the frame's constant positions; autograd carries the positions' gradient
            # into the grid through the transpose, ops.carrier_bwd)
            # (carrier_steps K > 1: var is a velocity and the positions are the end of its K-step flow, T.carrier_flow)
            p_ = (T.carrier_displace(var, p, self._carrier_cubic) if self._carrier_steps == 1 else
                  T.carrier_flow(var, p, self._carrier_steps, self._carrier_cubic)).unsqueeze(0)
        elif self._moves:
            p_ = p_ + (var[:, 0:3] if self._joint else var).unsqueeze(0)     # ('pc': the displacement columns)
        p_all = p_                                   # ('c': the positions as they came; var is not read)
        # a sequence keeps ONE particle order for all frames (frame 0's: the temporal filter needs particle i to be the
        # same particle everywhere), so by frame 60 of a flowing liquid the neighbours of that order have dispersed and
        # the splat would fall back to scattered global atomics; it therefore sees every frame through that frame's
        # own grid order (a gather of the positions in, the scatter of their gradient out -- the splat does not care
        # about the order of its particles)
        order = self._particle_order(p, p_)
        if order is not None:
            p_ = T.permute_particles(p_, order)
        if "d" in self.target_field:
            r_opt = torch.clamp(var.unsqueeze(0), -1, 1)                    # "necessary!" (styler_3p.py:74)
            r_ = r.unsqueeze(0) + r_opt
            if order is not None:
                r_ = T.permute_particles(r_, order)
            if getattr(self, "w_density", 0) > 0:
                # density preservation on the clipped offsets (self.d[i], styler_3p.py:75; styler_base.py:217-223)
                d_loss = r_opt[0].sum() ** 2
                d_pres = (-torch.log(r_opt[0].abs() + 1e-6)).sum()
                extra = (d_loss + d_pres * 1e3) * self.w_density
            d_ = None
            for k in range(self.num_kernels):
                support = self.support / self.kernel_scale ** k
                d_hat = T.p2g_wavg(p_, r_[..., k:k + 1], self.domain, res, self.radius, self.nsize, kernel="cubic",
                                   support=support, clip=self.clip, is_2d=False)
                d_ = d_hat if d_ is None else d_ + d_hat
        else:
            # d / rest_density (styler_3p.py:96): the particle mass is linear in rest_density (transform.py:1348-1352), so
            # the quotient is the splat with unit rest density -- no 32 MB scaling pass forward, none backward
            d_ = T.p2g(p_, self.domain, res, self.radius, 1.0, self.nsize, support=self.support,
                       clip=self.clip, is_2d=False)
            if self.w_pressure > 0:
                pressure = torch.where(d_ > 0, d_ - 1, torch.zeros_like(d_))
                extra = (pressure ** 2).mean() * self.w_pressure           # styler_base.py:228-230
        d_out = _SmoothRelu.apply(d_, float(self.k)) if self.k > 0 else _SmoothRelu.apply(d_, 0.0)
        return p_all[0], d_out, extra

    def _particle_order(self, p, p_now):
        """the permutation the splat sees frame ``p`` through, or None (= the caller's order).  Frames beyond the first
        get their own grid order at run start (``_orders``).  With the POSITIONS as the variable the particles drift away
        from the order they were put in -- 0.4 cells per step at lr 0.002 on a 200^3 grid; after 100 steps the boxes of
        consecutive particles no longer fit the splat's LDS accumulators and the forward splat runs at half speed
        (tools/chocolate_iter_profile.py: 213 us against 116 in grid order) -- so the order of a frame is recomputed from
        the CURRENT positions every ``reorder_every`` evaluations (default 10; 0 = never).  The splat does not care
        about the order of its particles; autograd scatters the gradient back through the gather.  The sort is STABLE
        (32-bit keys: the radix path either way), so two runs, or two ranks of a view-sharded run, that hold the same
        positions build the same layout and feed identically rounded sums to the blocks that fall back to float
        atomics."""
        orders = self.__dict__.setdefault("_orders", {})
        key = (p.data_ptr(), p.shape[0])
        every = int(getattr(self, "reorder_every", 10) or 0)
        if not self._moves or every <= 0 or not getattr(self, "sort_particles", True) or p.shape[0] < 2:
            return orders.get(key)
        ages = self.__dict__.setdefault("_order_age", {})
        age = ages.get(key, 0) + 1
        if age >= every:
            orders[key] = T.grid_order(p_now[0].detach(), self.resolution, stable=True)
            age = 0
        ages[key] = age
        return orders.get(key)

    def _value_and_grad(self, p, r, var, res, rot, view_shard=True):
        """loss (per view, device) and d loss / d var for one frame.  ``view_shard``: the views are sharded over the
        ranks of ``self.pg`` (then only rank 0 adds the view-independent terms)"""
        if self._colour:
            return self._colour_value_and_grad(p, r, var, res, rot if (self.rotate and rot is not None) else self._identity)
        if self._joint:
            return self._joint_value_and_grad(p, r, var, res, rot if (self.rotate and rot is not None) else self._identity)
        v = var.detach().clone().requires_grad_(True)
        _, d_out, extra = self._field(p, r, v, res)
        d3 = d_out.detach().reshape(d_out.shape[1:4]).contiguous()
        nviews = int(rot.shape[0]) if (self.rotate and rot is not None) else 1
        if self._graph_loss is None:
            # hipGraph replay of the loss chain where the host cannot keep up with it: tried (and timed against eager
            # submission) with one or two views per call; NFS_GRAPH=0 / 1 forces it off / on.  The GraphedLoss object is
            # made once; whether THIS call goes through it depends on this call's view count (it keys its capture on
            # the shapes and starts over when they change)
            self._graph_loss = engine.GraphedLoss.from_env(self.loss)
        if self._graph_loss and (self._graph_loss.force or nviews <= 2):
            losses, g_d = self._graph_loss(d3, rot)
            losses = losses.clone()
        else:
            losses, g_d = engine.loss_gradient(self.loss, d3, rot)
        # view-independent terms (pressure / density preservation) belong to the iteration, not to a view: with the
        # views sharded over ranks (views=sum) only rank 0 adds them, so that the all-reduced loss and gradient
        # contain them ONCE (every rank would otherwise contribute a copy: world x the single-rank weight)
        if extra is not None and view_shard and self._rank_world()[0] != 0:
            extra = None
        if extra is not None:
            losses = losses + extra.detach() / losses.numel()
        heads, grads = [d_out], [g_d.reshape(d_out.shape)]
        if extra is not None:
            heads.append(extra); grads.append(torch.ones_like(extra))
        torch.autograd.backward(heads, grads)
        return losses, v.grad

    def _rot(self, lo, hi):
        if self._colour:
            # one device buffer per slice of the current view list: the colour contexts are keyed on it
            cache = self.__dict__.setdefault("_rot_cache", {})
            if (lo, hi) not in cache:
                cache[(lo, hi)] = T.rot_to_device(self.rot_mat_[lo:hi], self.device)
            return cache[(lo, hi)]
        return T.rot_to_device(self.rot_mat_[lo:hi], self.device)

    def _resample_views(self):
        if "uniform" not in self.sample_type:
            if self._colour:
                self._colour_reset(views_only=True)       # new views: new ray weights
            self.rot_mat_, self.views = T.rot_mat(self.phi0, self.phi1, self.phi_unit, self.theta0, self.theta1,
                                                  self.theta_unit, sample_type=self.sample_type, rng=self.rng,
                                                  nv=self.n_views)

    def _dev(self, a):
        return torch.as_tensor(np.asarray(a, np.float32)).to(self.device).contiguous()

    def _var_shape(self, n):
        """the shape of a frame's variable: the carrier grid's for 'g', per particle otherwise"""
        if self._carrier:
            return tuple(self.carrier_resolution) + (3,)
        return (n, 6 if self._joint else 3 if (self._moves or self._colour) else self.num_kernels)

    # ---- debug helper: rendered images of the un-stylised input ------------------------------------
    def render_test(self, params):
        imgs = []
        for t in range(self.num_frames):
            p = self._dev(params["p"][t])
            n = p.shape[0]
            if self._colour:
                # mid-grey particles at rest density through the colour render (as styler_2p.render_test)
                r = torch.full((n, 1), float(self.rest_density), device=self.device)
                with torch.no_grad():
                    dimg = self._colour_d_img(p, r, torch.full((n, 3), 0.5, device=self.device), list(self.resolution))
                imgs.append(dimg[0].cpu().numpy().astype(np.uint8))
                self._colour_reset()
                continue
            if self._joint:
                r = torch.full((n, 1), float(self.rest_density), device=self.device)
                var = torch.zeros(n, 6, device=self.device)
                var[:, 3:6] = 0.5 / float(self.colour_lr_scale)
                with torch.no_grad():
                    dimg = self._joint_d_img(p, r, var, list(self.resolution))
                imgs.append(dimg[0].cpu().numpy().astype(np.uint8))
                continue
            r = self._dev(params["r"][t]) if "d" in self.target_field else None
            var = torch.zeros(*self._var_shape(n), device=self.device)
            with torch.no_grad():
                _, d_out, _ = self._field(p, r, var, list(self.resolution))
                dimg = self.loss.d_img(d_out.reshape(d_out.shape[1:4]).contiguous(), self._identity)
            imgs.append(dimg[0].cpu().numpy().astype(np.uint8))
        return imgs

    # ---- the optimisation loop (styler_3p.py:229-439) ----------------------------------------------
    def run(self, params):
        if (self._colour or self._joint) and self.pg is not None:
            raise ValueError("target_field %r over a process group: sharding the colour path over ranks is not built "
                             "(run it on one GPU)" % (self.target_field,))
        if self._carrier and self.pg is not None:
            raise ValueError("target_field 'g' over a process group (pg): sharding the carrier grid over ranks is not built "
                             "(run it on one GPU)")
        if abs(self.lr_scale - 1) > 1e-7 and not isinstance(self.lr, list):
            self.lr = [self.lr / self.lr_scale ** i for i in range(self.octave_n)]

        oct_size = []
        dhw = np.array(self.resolution)
        for _ in range(self.octave_n):
            oct_size.append(dhw)
            dhw = (dhw // self.octave_scale).astype(int)
        oct_size.reverse()
        print("input size for each octave", oct_size)

        p = [self._dev(x) for x in params["p"]]
        r = [self._dev(x) for x in params["r"]] if "d" in self.target_field else [None] * self.num_frames
        c_init = None
        if self._colour or self._joint:
            # per-particle densities [N,1] (the first kernel's column; rest_density where the frames carry none) and the
            # colour start: noise around the VGG mean / 255 (styler_2p.py:189-192) unless the caller brings one
            if params.get("r") is not None:
                r = [self._dev(np.asarray(x, np.float32).reshape(len(x), -1)[:, :1]) for x in params["r"]]
            else:
                r = [torch.full((x.shape[0], 1), float(self.rest_density), device=self.device) for x in p]
            if params.get("c_init") is not None:
                c_init = np.asarray([np.asarray(x, np.float32) for x in params["c_init"]], np.float32)
            else:
                assert len(set(int(x.shape[0]) for x in p)) == 1, "the drawn colour start needs the same particles in every frame (or pass params['c_init'])"
                c_init = self.rng.uniform(-5, 5, [self.num_frames, p[0].shape[0], 3]).astype(np.float32)
                c_init += np.array([vggmod._R_MEAN, vggmod._G_MEAN, vggmod._B_MEAN], np.float32)
                c_init /= 255
            if self._colour:
                self._colour_reset()
        # Particles in grid-cell order (one permutation for all frames, from the first frame's positions: the temporal
        # filter and the frame interpolation need particle i to be the same particle in every frame).  A block of
        # consecutive particles then touches a small box of cells and the splat accumulates it in LDS
        # (5e5 particles on 200^3: 0.69 ms unordered, 0.37 ordered with global atomics, 0.16 in LDS); the outputs are
        # returned in the caller's order.
        inv = None
        invs = None
        if self._carrier:
            # 'g': the variable has one shape whatever a frame holds, so the frames may hold different particles: each is
            # put into its OWN grid order (what the splat and the transpose of the sampling are fast in) and comes back
            # through its own inverse permutation
            invs = [None] * self.num_frames
            if getattr(self, "sort_particles", True):
                for t, x in enumerate(p):
                    if x.shape[0] > 1:
                        perm = T.grid_order(x, self.resolution)
                        invs[t] = torch.empty_like(perm)
                        invs[t][perm] = torch.arange(perm.numel(), device=self.device)
                        p[t] = x[perm].contiguous()
        elif getattr(self, "sort_particles", True) and len(set(int(x.shape[0]) for x in p)) == 1 and p[0].shape[0] > 1:
            perm = T.grid_order(p[0], self.resolution)
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(perm.numel(), device=self.device)
            p = [x[perm].contiguous() for x in p]
            r = [x[perm].contiguous() if x is not None else None for x in r]
        self._orders, self._order_age = {}, {}
        if getattr(self, "sort_particles", True) and self.num_frames > 1 and not self._carrier:
            for x in p[1:]:                                  # (frame 0 is in its own order already)
                if x.shape[0] > 1:
                    self._orders[(x.data_ptr(), x.shape[0])] = T.grid_order(x, self.resolution)
        g_opt = [torch.zeros(*self._var_shape(p[i].shape[0]), device=self.device) for i in range(self.num_frames)]
        if self._carrier and params.get("u_init") is not None:
            g_opt = [self._dev(params["u_init"][i]) for i in range(self.num_frames)]
            assert all(tuple(g.shape) == self._var_shape(0) for g in g_opt), "params['u_init'][t] is [Gd,Gh,Gw,3]"
        if self._colour:
            g_opt = [self._dev(c_init[i]) for i in range(self.num_frames)]
            if inv is not None:
                g_opt = [g[perm].contiguous() for g in g_opt]
        if self._joint:
            # (v, c / colour_lr_scale): the displacements start at zero, the colours as for 'c'
            for i in range(self.num_frames):
                c0 = self._dev(c_init[i])
                g_opt[i][:, 3:6] = (c0 if inv is None else c0[perm]) / float(self.colour_lr_scale)
        mode = getattr(self, "views_mode", "sequential")
        if getattr(self, "optimizer", "adam") == "lbfgs" and self.rotate and mode == "sequential" \
                and self.n_views > self.v_batch:
            raise ValueError("optimizer=lbfgs with views_mode='sequential': every step sees a different view batch, i.e. "
                             "a different objective -- gradient differences across them are not curvature pairs.  Use "
                             "views_mode='sum' (one objective per iteration) or optimizer=adam")

        # key frames (304-309) and who stylises them.  Frame sharding follows SURVEY 8(e): contiguous blocks of optimiser
        # groups per rank (one Adam state never straddles ranks), every rank keeps full view batches for its frames.
        keys = list(range(0, self.num_frames, self.batch_size * self.interp))
        rank, world = self._rank_world()
        by_frames = self.pg is not None and world > 1 and self.shard_by == "frames"
        if by_frames:
            plan = parallel.plan_frames(self.num_frames, self.batch_size * self.interp, self.frames_per_opt, world)
            owner = {t: rk for rk, ts in enumerate(plan) for t in ts}
        else:
            owner = {t: rank for t in keys}
        mine = [t for t in keys if owner[t] == rank]
        # the temporal Gaussian over the per-frame updates (382-383: scipy gaussian_filter along the frame axis, reflect,
        # truncate 4 sigma) as its matrix (util.temporal_weights == util.denoise, pinned to the reference's own function
        # by tests/golden/util_reference.npz): evaluated on the device, and -- frames sharded -- only the frames inside a
        # rank's filter window travel (point-to-point halo, parallel.exchange_frames)
        Wt = temporal_weights(len(keys), self.window_sigma) if (self.window_sigma > 0 and len(keys) > 1) else None
        if Wt is not None and not self._carrier:
            assert len(set(int(x.shape[0]) for x in p)) == 1, "temporal smoothing needs the same particles in every frame"
        need_by_rank = []
        for rk in range(world):
            nd = set(t for t in keys if owner[t] == rk) if by_frames else set(keys)
            if Wt is not None:
                for t in list(nd):
                    nd |= set(keys[jj] for jj in np.nonzero(Wt[keys.index(t)])[0])
            need_by_rank.append(nd)
        like = torch.zeros(*self._var_shape(p[0].shape[0]), device=self.device)

        def sync_all(g):
            """every rank receives every key frame's variable (octave ends, final inference: a few MB per frame)"""
            if not by_frames:
                return g
            got = parallel.exchange_frames({t: g[t] for t in mine}, set(keys), owner, like, group=self.pg,
                                           need_by_rank=[set(keys)] * world)
            for t in keys:
                g[t] = got[t]
            return g

        loss_history, d_intm, opt_ = [], [], {}
        for octave in range(self.octave_n):
            loss_history_o, d_intm_o = [], []
            res = [int(v) for v in oct_size[octave]]
            loss_net = self.colour.image_loss if (self._colour or self._joint) else self.loss   # (who holds the image targets)
            if self.style_img is not None:
                loss_net.set_style_image(self._style_feature(self.style_img, res[1:]))
                if getattr(self, "w_hist", 0) > 0:                # styler_3p.py:288-293
                    loss_net.set_hist_image(self._hist_feature(self.style_img, res[1:]))
            if self.content_img is not None:                     # styler_3p.py:277-279
                loss_net.set_content_image(self._content_feature(self.content_img, res[1:]), top_k=self._content_top_k())
            if self._colour:
                self._colour_reset()                             # the frames' grey volumes and ray weights are per octave
            lr = self.lr[octave] if isinstance(self.lr, list) else self.lr

            for step in range(self.iter):
                g_tmp = {}
                l_step = torch.zeros(len(keys), device=self.device)
                for j, t in enumerate(keys):
                    if owner[t] != rank:
                        # every rank draws the same view sequence whoever owns the frame (344-349)
                        if self.rotate:
                            self._resample_views()
                        continue
                    var = g_opt[t].clone()                       # variable re-assigned from g_opt (312)
                    opt_id = engine.optimizer_slot(getattr(self, "optimizer", "adam"), t, self.frames_per_opt)
                    if opt_id not in opt_:
                        opt_[opt_id] = engine.make_optimizer(getattr(self, "optimizer", "adam"))
                    adam = opt_[opt_id]

                    if self.rotate and mode == "sequential":
                        acc, l_ = None, []
                        for i in range(0, self.n_views, self.v_batch):
                            losses, g = self._value_and_grad(p[t], r[t], var, res, self._rot(i, i + self.v_batch),
                                                             view_shard=False)     # (the sequential mode never shards views)
                            adam.step(var, g.contiguous(), lr)
                            l_.append(losses.sum())
                            cur = torch.nan_to_num(var)
                            acc = cur.clone() if acc is None else acc + cur
                        l_step[j] = torch.stack(l_).mean()
                        self._resample_views()
                        new = acc / (self.n_views / self.v_batch)
                    else:
                        if self.rotate:
                            nvw = len(self.rot_mat_)
                            rot = self._rot(0, nvw)
                            if self.pg is not None and not by_frames:
                                rot = rot[rank::world].contiguous()
                        else:
                            rot = self._identity
                        losses, g = self._value_and_grad(p[t], r[t], var, res, rot,
                                                         view_shard=self.pg is not None and not by_frames)
                        total = losses.sum()
                        if self.pg is not None and not by_frames:
                            g = g.contiguous()
                            parallel.all_reduce_sum_([g, total], group=self.pg)
                        adam.step(var, g.contiguous(), lr)
                        l_step[j] = total
                        if self.rotate:
                            self._resample_views()
                        new = torch.nan_to_num(var)

                    upd = new - g_opt[t]
                    if "d" in self.target_field:
                        upd = upd * r[t][..., 0:1]                  # masking by original density (361-363)
                    g_tmp[t] = upd

                    if step == self.iter - 1 and octave < self.octave_n - 1 and not by_frames:
                        with torch.no_grad():
                            if self._colour:
                                dimg = self._colour_d_img(p[t], r[t], var, res)
                            elif self._joint:
                                dimg = self._joint_d_img(p[t], r[t], var, res)
                            else:
                                _, d_out, _ = self._field(p[t], r[t], var, res)
                                dimg = self.loss_d_img(d_out)
                        d_intm_o.append(dimg.cpu().numpy().astype(np.uint8))

                if by_frames:
                    parallel.all_reduce_sum_([l_step], group=self.pg)
                loss_history_o.extend(float(x) for x in l_step.cpu())
                if Wt is not None:
                    got = parallel.exchange_frames(g_tmp, need_by_rank[rank], owner, like, group=self.pg,
                                                   need_by_rank=need_by_rank) if by_frames else g_tmp
                    for t in mine:
                        jrow = Wt[keys.index(t)]
                        f = None
                        for jj in np.nonzero(jrow)[0]:
                            term = got[keys[jj]] * float(jrow[jj])
                            f = term if f is None else f.add_(term)
                        g_opt[t] = g_opt[t] + f
                else:
                    for t in mine:
                        g_opt[t] = g_opt[t] + g_tmp[t]

            loss_history.append(loss_history_o)
            if by_frames:
                g_opt = sync_all(g_opt)
                if octave < self.octave_n - 1:                   # (every rank renders every key frame: same d_intm everywhere)
                    for t in keys:
                        with torch.no_grad():
                            _, d_out, _ = self._field(p[t], r[t], g_opt[t], res)
                            dimg = self.loss_d_img(d_out)
                        d_intm_o.append(dimg.cpu().numpy().astype(np.uint8))
            if octave < self.octave_n - 1:
                d_intm.append(np.concatenate(d_intm_o, axis=0))

        if self.interp > 1:
            w = np.linspace(0, 1, self.interp + 1)
            for t in range(0, self.num_frames - 1, self.interp):
                for i in range(1, self.interp):
                    if t + self.interp < self.num_frames:
                        g_opt[t + i] = g_opt[t] * float(1 - w[i]) + g_opt[t + self.interp] * float(w[i])

        result = {"l": loss_history, "d_intm": d_intm, "v": None, "c": None}
        res = [int(v) for v in oct_size[-1]]
        p_sty, v_sty, d_sty, r_sty = [], [], [], []
        for t in range(self.num_frames):
            with torch.no_grad():
                p_out, d_out, _ = self._field(p[t], r[t], g_opt[t], res)
                dimg = self._colour_d_img(p[t], r[t], g_opt[t], res) if self._colour else \
                    self._joint_d_img(p[t], r[t], g_opt[t], res) if self._joint else self.loss_d_img(d_out)
            if self._carrier:
                # (the sampled displacements beside the positions they make: p + v is result['p'], float for float)
                inv = invs[t]
                if self._carrier_steps == 1:
                    p_out, v_t = ops.carrier_displace(g_opt[t].contiguous(), p[t], cubic=self._carrier_cubic)
                else:
                    # (the end of the flow, float for float what apply_carrier returns, and the displacement it amounts to)
                    p_out = ops.flow_fwd(g_opt[t].contiguous(), p[t], self._carrier_steps,
                                         cubic=self._carrier_cubic)[self._carrier_steps]
                    v_t = p_out - p[t]
                v_sty.append((v_t if inv is None else v_t[inv]).cpu().numpy())
            p_sty.append((p_out if inv is None else p_out[inv]).cpu().numpy())
            if "p" in self.target_field:
                v_t = g_opt[t][:, 0:3] if self._joint else g_opt[t]
                v_sty.append((v_t if inv is None else v_t[inv]).cpu().numpy())
            d_sty.append(torch.abs(d_out[0]).cpu().numpy())      # abs(): drop the sign-bit mask of -0.0
            r_sty.append(dimg[0].cpu().numpy().astype(np.uint8))
        result["p"] = p_sty
        if self._moves:
            result["v"] = v_sty
        result["d"] = np.array(d_sty)
        result["r"] = np.array(r_sty)
        if self._joint:
            # 'opt' in natural units: (v, c), the colour columns times colour_lr_scale
            unit = torch.tensor([1.0] * 3 + [float(self.colour_lr_scale)] * 3, device=self.device)
            g_opt = [g * unit for g in g_opt]
        if self._carrier:
            inv = None                                       # (the fields have no particle axis)
            result["carrier_resolution"] = list(self.carrier_resolution)
        result["opt"] = [(g if inv is None else g[inv]).cpu().numpy() for g in g_opt]   # build extension: the variables
        if self._colour or self._joint:
            # the colours as styler_2p returns them: clipped, and faded by the particle's density (styler_2p.py:297-300)
            cols = [g[:, 3:6] if self._joint else g for g in g_opt]
            result["c"] = [((torch.clamp(cols[t], 0, 1) * torch.clamp(r[t] / self.rest_density, 0, 1))
                            [slice(None) if inv is None else inv]).cpu().numpy() for t in range(self.num_frames)]
            result["c_init"] = c_init
            if self._colour:
                self._colour_reset()
        self._orders, self._order_age = {}, {}   # keyed by device address: the frame tensors die with this call
        return result

    def loss_d_img(self, d_out):
        """d_img with the identity rotation (styler_3p.py:366-369, 416-420)"""
        d3 = d_out.reshape(d_out.shape[1:4]).contiguous()
        return self.loss.d_img(d3, self._identity)

    def _rank_world(self):
        return (0, 1) if self.pg is None else parallel.rank_world(self.pg)

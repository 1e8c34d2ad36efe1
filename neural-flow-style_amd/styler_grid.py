"""Grid-sequence stylizer (BASELINE ``configs[3]``: a frame sequence on a 3-D smoke grid with semi-Lagrangian
transport of the stylised field) -- the Eulerian counterpart of ``styler_3p.Styler.run``.

The mounted reference branch keeps the loop for particles (styler_3p.py:229-439) and the grid operators as
leftovers: ``advect`` (transform.py:557-569) and ``StylerBase._transport`` (styler_base.py:59-89), which moves a grid
field from frame a to frame b through the simulation velocities.  This module assembles them exactly the way the
particle loop is built:

  per key frame t (styler_3p.py:304-363), variable re-assigned from ``g_opt[t]`` (312), one TF-Adam state per
  ``opt_id = t // frames_per_opt`` (315-323):
        d^_t = advect(d_t, v^_t)            ('v': stylisation velocity [D,H,W,3];  'd': the density itself;
                                             's': a stream function [D,H,W,3], v^_t = its stream velocity;
                                             'p': a potential [D,H,W], v^_t = its forward differences;
                                             'sp': both [D,H,W,4], v^_t = the sum of the two)
        -> 3x3x3 smooth + max(.,0) -> rotate (all views, ``views=sum``) -> render -> VGG-19 -> Gram style loss
        -> adjoint chain -> one Adam step;      upd_t = new - g_opt[t]   ('d': masked by the original density, 361-363)
  temporal alignment of the updates (380-386).  Per-particle attributes ride on the particles, so the reference filters
  them along the frame axis in place (``denoise``: SciPy Gaussian, reflect, 4 sigma).  A grid field has to be carried
  to the frame it is added to:
        D_t = sum_s W[t,s] * transport(upd_s, u, s -> t)
  with W the very matrix of that Gaussian filter (util.temporal_weights; for u == 0 this IS ``denoise``) and
  ``transport`` = ``_transport`` (recursive chain of ``advect`` by +u_i forwards / -u_i backwards, or its one-step
  ``recursive=False`` form).  ``advect`` is linear in the advected field, so the sum over s is evaluated in Horner
  form -- R advects per side and frame instead of R(R+1)/2:
        S = W[t,t-R] upd_{t-R};  S = advect(S, u_{t-k}) + W[t,t-k+1] upd_{t-k+1} ...;  D_t^- = advect(S, u_{t-1})
  then ``g_opt[t] += D_t`` (386), frame interpolation (392-397), final inference.

Frames shard over ranks: contiguous blocks of optimiser groups per rank
(parallel.plan_frames), every rank keeps full view batches, and the only exchange is the halo of per-frame updates
the temporal filter reaches (point-to-point, parallel.exchange_frames) plus a handful of loss scalars.  The sharded
run reproduces the single-rank trajectory (tests: world-2 gloo, two ranks on one GPU).

Octaves (``octave_n`` > 1, sizes as in the particle loop, styler_3p.py:240-247, 271-296): the loop runs coarsest first on the
density frames and simulation velocities resampled from the full-resolution originals (``ops.resize3d``: the reference's
``util.resize_tf`` of a volume, util.py:128-143), and hands the variable of every key frame to the next octave by the
same resample.  The grid is corner-aligned (one cell = 2/(n-1) in ``advect``), so every resample is bilinear with
``align_corners``: node 0 and node n-1 are the same points of the domain at every octave, and a velocity in advect units
is the same displacement at every octave (factor 1).  A potential or stream function is differentiated per CELL
(``ops.source_velocity``), so its resample carries the factor f = mean over the axes of (n_out-1)/(n_in-1), which keeps
the flow it stands for; on an anisotropic grid the three ratios differ slightly and that warm start is approximate.
Every octave starts with fresh optimiser state (Adam moments, L-BFGS pairs: their shapes belong to the old grid) and a
fresh ``engine.GridStylizer``.

Colour (``grid_variable 'c'``, 3-D only; a build extension like the 2-D sequences: the reference has no such path).  The
variable of key frame t is a colour field c_t [D,H,W,3] seen through the frame's own grey volume:
        e_t = smooth3d_relu(d_t, k)         what the 'd' path renders at zero change: absorbs AND emits, constant in c_t
        ctx_t = ColourRenderLoss.prepare(e_t, rot): ray weights w = T / M, the grey image, d_gray = clip(I / M, 0, 1),
                                            one maximum per ``v_batch`` views
        q = clamp01(c_t) * e_t  ->  J = sum_z w rotate(q), img = clip(J, 0, 1)  ->  ImageStyleLoss (style, TV, content,
                                            histogram; ``style_mask`` masks by d_gray)
        g_c = g_q * e_t where 0 <= c_t <= 1 (a colour exactly 0 or 1 passes its gradient), else 0
        one optimiser step on the summed view losses;  upd_t = nan_to_num(new) - g_opt[t], NOT masked: where e_t == 0 the
                                            gradient is an exact zero (e_t may carry -0.0, which compares equal to zero)
(``engine.ColourGridStylizer``, kernels: include/nfs_emission.h).  Temporal alignment, ``frames_per_opt``, ``interp``,
``lr_decay``, the octaves (a colour resamples with factor 1) and frame sharding are the loop below on a three-channel field.

Optimisers: TF-Adam (the reference's), L-BFGS (3-D), and ``optimizer='lapnorm'``: Laplacian-normalised descent, the
update rule of a transport-based stylizer built from the reference's unused ``lap_normalize`` (``engine.LapDescentState``).
The learning rate of every optimiser follows the reference's unused ``cosine_decay`` within an octave (``lr_decay``,
default 1: constant).  Nothing is carried across octaves.
"""
from __future__ import annotations

import numpy as np
import torch

from . import engine, grid2d, ops, parallel
from . import transform as T
from .config import check_colour_render, check_optimizer, colour_exposure
from .styler_base import StylerBase
from .util import cosine_decay, temporal_weights


class Styler(StylerBase):
    """``Styler(config).run(params)`` with ``params['d']`` = F density frames [D,H,W] and ``params['v']`` = F
    simulation velocities [D,H,W,3] in ``advect`` units (normalised: one cell = 2/(n-1), component k along array
    axis k).  ``config.grid_variable`` = 'v' (default), 'd', or 's': a stream function whose
    stream velocity (``ops.stream_velocity``, divergence-free) advects the density; it starts from zero or
    ``params['s_init'][t]``, and the result carries it as ``'s'`` / ``'opt'`` beside the stream velocities ``'v'``.
    'p': a potential [D,H,W] (``ops.potential_velocity``, irrotational; ``params['p_init'][t]``), 'sp': the Helmholtz pair
    [D,H,W,4] = (stream function, potential) (``ops.helmholtz_velocity``; ``params['sp_init'][t]``): ``'opt'`` is the
    variable, ``'v'`` the velocity it stands for, ``'s'`` its stream-function part ('s', 'sp') and ``'phi'`` its potential
    ('p', 'sp'); ``'p'`` stays the reference's particle-position key (None on the grid path).
    ``octave_n`` > 1 (module docstring; not with 'd'): ``run`` is ``prepare``, then per octave ``next_octave()`` (from the
    second on) and ``iter`` x ``iterate()``, then ``finish()``.  The result's ``'l'`` is one list per octave, ``'l_frames'``
    the per-iteration rows of all octaves in order, ``'d_intm'`` per octave but the last the uint8 identity-rotation
    renders of the key frames this rank holds (concatenated along axis 0, styler_3p.py:365-390), ``'opt_octave'`` per
    octave {own key frame: the variable as the octave left it, at that octave's size}, ``'octave_sizes'`` the sizes;
    everything else is at full resolution.

    ``len(config.resolution) == 2`` selects the 2-D path (``grid2d.GridStylizer2D``): ``params['d']`` frames [H,W],
    ``params['v']`` [H,W,2], ``v_init`` [H,W,2] / ``s_init`` [H,W] / ``p_init`` [H,W] / ``sp_init`` [H,W,2] = (psi, phi).  The
    frame loop, sharding, temporal weights, ``interp``, ``frames_per_opt``, the 'd' mask and the octaves are the code
    below unchanged (``ops.transport_step2d`` crosses frames, ``ops.resize3d`` resamples the depth-1 volume); the result
    holds ``'d'`` float32 [F,H,W,1] (the clipped image), ``'r'`` uint8 [F,H,W,3], ``'v'`` [H,W,2], ``'s'`` / ``'phi'``
    [H,W].  ``config.optimizer`` = 'lapnorm' (2-D and 3-D, with ``config.lap_n`` pyramid levels): Laplacian-normalised
    descent (``engine.LapDescentState``) in place of Adam, everything else -- octaves, frame sharding, ``frames_per_opt``,
    ``interp``, the 'd' mask, the temporal alignment -- unchanged; ``lr`` is then a length in the variable's units (for 'v',
    lr = c * 2/(n-1) is about c cells per pyramid level and step, at every octave alike).  ``config.lr_decay`` (every
    optimiser): iteration i of an octave runs at ``util.cosine_decay(i, iter, lr[o], lr_decay)``.
    ``grid_variable`` = 'c' (3-D): a colour field [D,H,W,3] per key frame, emitted by the frame's smoothed density (module
    docstring).  It starts from the resample of ``params['c_init'][t]`` [D,H,W,3] or, where that is missing, from ONE seeded
    field shared by all frames, drawn once at full resolution from ``self.rng``: (uniform(-5, 5) + the VGG means) / 255 (a
    sharded run passes ``c_init`` for every frame or for none, so that every rank draws alike).  The result holds ``'c'``:
    clamp01(opt) * clip(e, 0, 1) per present frame (the masked colour, as styler_2p returns it), ``'opt'`` the raw
    variables, ``'r'`` uint8 colour images [F,H,W,3], ``'d'`` = abs(e) [F,D,H,W,1], ``'d_intm'`` in colour, ``'c_init'``
    what the run started from, ``'v'`` / ``'s'`` / ``'phi'`` / ``'p'`` None.  ``adv_order`` is accepted and has no effect
    (as with 'd'); an attribute ``colour_bwd_route`` on the config names the route of the projection's transpose ('tiled':
    bit-reproducible).  ``colour_render`` = 'liquid': the frame's image is clip(sum_z w rotate(q) + t bg, 0, 1), front-to-back
    alpha compositing over ``colour_background`` (include/nfs_liquid.h; ``engine.ColourRenderLoss``); ``'r'`` and
    ``'d_intm'`` are then over the background, everything else of the path unchanged.  Refused with a ValueError naming
    the flag: a two-entry ``resolution``, ``render_liquid``, a non-empty ``ray_mode``, ``style_mask_on_ref``,
    ``w_density`` > 0, a ``colour_render`` outside '' / 'smoke' / 'liquid' / 'exposure' (and 'liquid' or 'exposure' with
    another variable), a ``colour_exposure`` that is not finite and positive, a
    ``colour_background`` that is not three numbers in [0,1].  Eager launches only.
    Not built in 2-D: ``rotate`` (ValueError: there are no views), L-BFGS (ValueError), dead-region masks, slab
    sharding, a MacCormack transport between frames, ``batch_size > 1``, a root-level driver (the reference has none for
    grids)."""

    def __init__(self, self_dict):
        check_optimizer(self_dict, grid=True)
        check_colour_render(self_dict, colour=getattr(self_dict, "grid_variable", "") == "c")
        if getattr(self_dict, "grid_variable", "") == "c":
            # the colour grid renders by emission-absorption through an image loss and has no auxiliary field terms
            # (refused before the base class loads a network)
            if len(self_dict.resolution) == 2:
                raise ValueError("grid_variable 'c' with a two-entry resolution %s: 2-D colour grids are not built"
                                 % (list(self_dict.resolution),))
            if getattr(self_dict, "render_liquid", False):
                raise ValueError("grid_variable 'c': render_liquid is the grey liquid render and is not built for the "
                                 "colour render (pass --render_liquid false; the liquid colour render is "
                                 "--colour_render liquid)")
            if getattr(self_dict, "ray_mode", ""):
                raise ValueError("grid_variable 'c': ray_mode %r is not built for the colour render (leave --ray_mode empty)"
                                 % (self_dict.ray_mode,))
            if getattr(self_dict, "style_mask_on_ref", False):
                raise ValueError("grid_variable 'c': style_mask_on_ref is not built for the colour render (pass "
                                 "--style_mask_on_ref false)")
            if (getattr(self_dict, "w_density", 0) or 0) > 0:
                raise ValueError("grid_variable 'c': w_density acts on a density variable (pass --w_density 0)")
        StylerBase.__init__(self, self_dict)
        assert self.batch_size == 1, "batch_size > 1 is not supported (styler_3p module docstring)"
        self.target = getattr(self, "grid_variable", "") or "v"
        assert self.target in ("v", "d", "c") + engine.SOURCED
        self.adv_order = int(getattr(self, "adv_order", 1) or 1)       # config.py adv_order: 1 = SL, 2 = MacCormack
        self.octave_n = int(self.octave_n)
        if self.target == "d" and self.octave_n > 1:
            raise ValueError("grid_variable='d' with octave_n=%d: the variable is the density itself, and resampling it to "
                             "a coarser octave would discard the fine detail of the input -- use octave_n=1"
                             % self.octave_n)
        if abs(getattr(self, "lr_scale", 1) - 1) > 1e-7 and not isinstance(self.lr, list):
            self.lr = [self.lr / self.lr_scale ** i for i in range(self.octave_n)]      # styler_3p.py:236-238
        self.is2d = len(self.resolution) == 2                          # an [H,W] grid: the 2-D path (grid2d.py)
        if self.is2d and self.rotate:
            raise ValueError("rotate=True with a 2-D resolution %s: a 2-D density is its own image, there are no views"
                             % (list(self.resolution),))
        if self.is2d and getattr(self, "optimizer", "adam") == "lbfgs":
            raise ValueError("optimizer='lbfgs' is not built for the 2-D grid path: use 'adam' or 'lapnorm'")
        self.lap_n, self.lr_decay = int(getattr(self, "lap_n", 3)), float(getattr(self, "lr_decay", 1))
        self.octave_sizes = octave_sizes(self.resolution, self.octave_n, self.octave_scale)
        if self.octave_n > 1 and min(self.octave_sizes[0]) < 2:
            raise ValueError("octave_n=%d at octave_scale=%g takes resolution %s down to %s: every octave needs at least "
                             "two nodes per axis" % (self.octave_n, self.octave_scale, list(self.resolution),
                                                     self.octave_sizes[0]))
        if self.rotate:
            self.rot_mat_, self.views = T.rot_mat(self.phi0, self.phi1, self.phi_unit, self.theta0, self.theta1,
                                                  self.theta_unit, sample_type=self.sample_type, rng=self.rng,
                                                  nv=self.n_views)
            if self.n_views is None:
                self.n_views = len(self.views)
        if self.target == "c":
            # the colour render around an image loss (styler_3p's 'c' path); the image targets live in the image loss
            render, background = check_colour_render(self, colour=True)
            self.loss = engine.ColourRenderLoss(self._make_image_loss(), self.transmit, self.v_batch if self.rotate else 1,
                                                render=render, background=background,
                                                exposure=colour_exposure(getattr(self, "colour_exposure", 1.0)))
            self.colour_bwd_route = getattr(self, "colour_bwd_route", None)   # ('tiled': bit-reproducible steps)
        else:
            self.loss = self._make_image_loss() if self.is2d else self._make_loss(rotate=self.rotate)
        self._rot_dev = self._rot_src = None
        self._identity = T.rot_to_device([np.identity(3)], self.device)
        self.recursive = bool(getattr(self, "transport_recursive", True))
        self.pg = None          # set by the driver: frames shard over the ranks of this group

    # ---- helpers ---------------------------------------------------------------------------------------------------
    def _dev(self, a):
        return torch.as_tensor(np.asarray(a, np.float32)).to(self.device).contiguous()

    def _make_image_loss(self):
        """the 2-D path's loss: ``engine.ImageStyleLoss`` on the clipped density as a one-channel image"""
        w_layers = list(self.w_style_layer)
        if len(w_layers) == 1 and len(self.style_layer) > 1:
            w_layers = w_layers * len(self.style_layer)
        return engine.ImageStyleLoss(self.net, self.style_layer, w_layers, self.w_style, w_tv=self.w_tv,
                                     resize_scale=self.resize_scale, style_mask=getattr(self, "style_mask", False),
                                     w_content=getattr(self, "w_content", 0),
                                     content_layer=getattr(self, "content_layer", None),
                                     content_channel=getattr(self, "content_channel", 0),
                                     w_content_amp=getattr(self, "w_content_amp", 100),
                                     w_hist=getattr(self, "w_hist", 0), hist_layer=getattr(self, "hist_layer", ()),
                                     w_hist_layer=getattr(self, "w_hist_layer", ()))

    def _rank_world(self):
        return (0, 1) if self.pg is None else parallel.rank_world(self.pg)

    def _rot(self):
        if not self.rotate:
            return self._identity
        if self.target == "c":
            # ONE device tensor per drawn view list: the colour stylizer keeps its ray weights while the views stand
            if self._rot_src is not self.rot_mat_:
                self._rot_dev, self._rot_src = T.rot_to_device(self.rot_mat_, self.device), self.rot_mat_
            return self._rot_dev
        return T.rot_to_device(self.rot_mat_, self.device)

    def _resample_views(self):
        if self.rotate and "uniform" not in self.sample_type:
            self.rot_mat_, self.views = T.rot_mat(self.phi0, self.phi1, self.phi_unit, self.theta0, self.theta1,
                                                  self.theta_unit, sample_type=self.sample_type, rng=self.rng,
                                                  nv=self.n_views)

    def aligned_update(self, t, upd, u, W, keys):
        """D_t = sum_s W[t,s] transport(upd_s, u, s -> t) over the key frames s.  ``upd`` {frame: [D,H,W,C]} must hold
        every frame with a non-zero weight; ``u`` {frame: [D,H,W,3]} the simulation velocities.  Every frame crossing
        is one ``nfs_transport_step`` launch (advect + weighted accumulation fused); ``transport`` is
        ``StylerBase._transport`` (styler_base.py:59-74):
          recursive   a < b: g <- advect(g, +u_i), i = a..b-1;   a > b: g <- advect(g, -u_i), i = a-1..b   (Horner form)
          one-step    a < b: advect(g, +u_a (b-a));              a > b: advect(g, -u_{a-1} (a-b))          (direct sum)"""
        step = ops.transport_step2d if self.is2d else ops.transport_step     # (2-D: upd [H,W,C], u [H,W,2])
        j = keys.index(t)
        out, w_out = upd[t], float(W[j, j])          # running result = w_out * out (scaled lazily by the next launch)
        if not self.recursive:
            for jj in range(len(keys)):
                s = keys[jj]
                if jj == j or W[j, jj] == 0.0:
                    continue
                a, scale = (s, float(t - s)) if s < t else (s - 1, -float(s - t))
                out = step(upd[s], u[a], scale, float(W[j, jj]), out, w_out)
                w_out = 1.0
            return out if w_out == 1.0 else out * w_out
        for sign in (+1, -1):
            # sign +1: frames s < t carried forwards; sign -1: frames s > t carried backwards
            far = [jj for jj in (range(0, j) if sign > 0 else range(len(keys) - 1, j, -1)) if W[j, jj] != 0.0]
            if not far:
                continue
            jj = far[0]
            S, w_S = upd[keys[jj]], float(W[j, jj])  # carried sum = w_S * S
            while jj != j:
                s, nxt = keys[jj], jj + sign
                s2 = keys[nxt]
                cross = list(range(s, s2)) if sign > 0 else list(range(s - 1, s2 - 1, -1))
                for n_, i in enumerate(cross):
                    add, w_add = None, 0.0
                    if n_ == len(cross) - 1:         # arriving at key frame s2: add its own (weighted) update
                        if nxt == j:
                            add, w_add = out, w_out
                        elif W[j, nxt] != 0.0:
                            add, w_add = upd[s2], float(W[j, nxt])
                    S = step(S, u[i], float(sign), w_S, add, w_add)
                    w_S = 1.0
                jj = nxt
            out, w_out = S, 1.0
        return out if w_out == 1.0 else out * w_out

    # ---- the optimisation loop: prepare -> iterate x iter -> finish ------------------------------------------------------
    def _frames(self, x, wanted):
        """params entry (list indexed by frame, or {frame: array}) -> {frame: device tensor} for the wanted frames"""
        if x is None:
            return None
        get = (lambda t: x[t]) if not isinstance(x, dict) else (lambda t: x.get(t))
        return {t: self._dev(get(t)) for t in wanted if get(t) is not None}

    def frames_needed(self, rank=None, world=None):
        """(density frames, simulation-velocity frames) rank ``rank`` of ``world`` touches in a sharded run: its own
        key frames, and the velocities of every frame crossing its temporal filter makes (the non-zero columns of the
        ``denoise`` matrix).  A pure function of the configuration: a driver can load exactly these frames and pass
        ``prepare(params, frames_on_device=densities)``.  A rank beyond the number of optimiser groups gets two empty
        sets (it still takes part in the collectives)."""
        if rank is None or world is None:
            rank, world = self._rank_world()
        F_ = int(self.num_frames)
        keys = list(range(0, F_, self.interp))
        plan = parallel.plan_frames(F_, self.interp, self.frames_per_opt, world)
        mine = plan[rank]
        if not mine:
            return set(), set()
        need = set(mine)
        if self.window_sigma > 0 and F_ > 1:
            Wt = temporal_weights(len(keys), self.window_sigma)
            for t in mine:
                need |= set(keys[jj] for jj in np.nonzero(Wt[keys.index(t)])[0])
            return set(mine), set(range(max(min(need) - 1, 0), min(max(need) + 1, F_)))
        return set(mine), set()

    def prepare(self, params, frames_on_device=None):
        """Put this rank's share of the sequence on the device and set up the loop state.  ``params['d']`` /
        ``params['v']`` / ``params['v_init']``: list over frames or {frame: array}; a sharded run only needs the
        frames this rank touches (``frames_needed(rank, world)``; ``frames_on_device`` = its density frames)."""
        F_ = int(self.num_frames)
        rank, world = self._rank_world()
        st = self._st = argparse_ns()
        st.F, st.rank, st.world = F_, rank, world
        st.keys = list(range(0, F_, self.interp))
        st.plan = parallel.plan_frames(F_, self.interp, self.frames_per_opt, world)
        st.owner = {t: r for r, ts in enumerate(st.plan) for t in ts}
        st.mine = st.plan[rank]
        st.Wt = temporal_weights(len(st.keys), self.window_sigma) if (self.window_sigma > 0 and F_ > 1) else None
        # which frames' updates this rank's filter reaches (non-zero weights only), and the velocities in between
        def need_of(r):
            nd = set(st.plan[r])
            if st.Wt is not None:
                for t in st.plan[r]:
                    j = st.keys.index(t)
                    nd |= set(st.keys[jj] for jj in np.nonzero(st.Wt[j])[0])
            return nd

        st.need_by_rank = [need_of(r) for r in range(world)]       # a pure function of plan and filter: no exchange
        st.need = st.need_by_rank[rank]
        want_d = set(range(F_)) if frames_on_device is None else set(frames_on_device) | set(st.mine)
        want_u = set(range(F_)) if frames_on_device is None else \
            set(range(max(min(st.need) - 1, 0), min(max(st.need) + 1, F_))) if st.need else set()
        st.d_full = {t: x.reshape(tuple(self.resolution)) for t, x in self._frames(params["d"], sorted(want_d)).items()}
        st.u_full = self._frames(params.get("v"), sorted(want_u))
        if st.Wt is not None and st.mine and not st.u_full:
            raise ValueError("params['v'] (simulation velocities) is needed to align the updates of a sequence")
        st.u_full = st.u_full or {}
        st.C = ({"v": 2, "sp": 2} if self.is2d else {"v": 3, "s": 3, "sp": 4, "c": 3}).get(self.target, 1)
        # the variable per key frame: stylisation velocity (zero, or params['v_init'][t]) / the density itself.
        # NOTE: at velocity == 0 every back-traced point sits exactly on a grid node, where the trilinear stencil has a
        # kink -- the first gradient is a one-sided derivative whose side depends on float rounding
        st.v_init = params.get(self.target + "_init" if self.target in engine.SOURCED + ("c",) else "v_init")
        st.c_noise = None
        if self.target == "c" and not self._has_every(st.v_init, range(F_)):
            # ONE seeded field for all frames, drawn once at full resolution by every rank alike: noise around the VGG
            # mean / 255 (styler_2p.py:189-192, with its commented "same noise" choice: no flicker is seeded)
            from . import vgg as vggmod
            noise = self.rng.uniform(-5, 5, tuple(int(n) for n in self.resolution) + (3,)).astype(np.float32)
            noise += np.array([vggmod._R_MEAN, vggmod._G_MEAN, vggmod._B_MEAN], np.float32)
            noise /= 255
            st.c_noise = noise
        st.hist, st.hist_octave, st.d_intm, st.opt_octave = [], [], [], []
        st.octave = 0
        self._enter_octave(None)
        return st

    def _resample(self, x, size, factor=1.0):
        """a volume [D,H,W] or [D,H,W,C] at ``size``: the corner-aligned bilinear resample of the octaves (the very tensor
        where the size is its own: one octave issues no resize)"""
        if tuple(x.shape[:len(size)]) == tuple(size):
            return x
        if self.is2d:                      # the depth-1 volume: bilinear over (H, W), nothing to do over D
            return ops.resize3d(x.contiguous().unsqueeze(0), (1,) + tuple(size), "bilinear", align_corners=True,
                                scale=factor).squeeze(0)
        return ops.resize3d(x.contiguous(), size, "bilinear", align_corners=True, scale=factor)

    def _factor(self, n_in, n_out):
        """what a resampled variable is multiplied by: 1 for a velocity; a potential or stream function is differenced
        per cell, so it takes the mean over the axes of (n_out-1)/(n_in-1) (float64, cast to float32 once)"""
        if self.target not in engine.SOURCED or tuple(n_in) == tuple(n_out):
            return 1.0
        return float(np.float32(np.mean([(float(o) - 1.0) / (float(i) - 1.0) for i, o in zip(n_in, n_out)],
                                        dtype=np.float64)))

    def _enter_octave(self, prev):
        """set the loop state up for octave ``st.octave``: inputs resampled from the full-resolution originals, the loss
        targets at the octave's [H,W], its learning rate, the variable of every own key frame (octave 0: zero or the
        resampled ``'_init'``; later: ``g_opt`` resampled from the size ``prev``), fresh optimiser state and stylizer"""
        st = self._st
        o = st.octave
        size = tuple(int(n) for n in self.octave_sizes[o])
        H, W_ = size[-2:]
        st.d = {t: self._resample(x, size) for t, x in st.d_full.items()}
        st.u = {t: self._resample(x, size) for t, x in st.u_full.items()}
        st.shape = size + (st.C,)
        targets = self.loss.image_loss if self.target == "c" else self.loss      # (who holds the image targets)
        if self.style_img is not None:
            targets.set_style_image(self._style_feature(self.style_img, [H, W_]))
            if getattr(self, "w_hist", 0) > 0:
                targets.set_hist_image(self._hist_feature(self.style_img, [H, W_]))
        if self.content_img is not None:
            targets.set_content_image(self._content_feature(self.content_img, [H, W_]), top_k=self._content_top_k())
        st.lr = self.lr[o] if isinstance(self.lr, list) else self.lr
        if prev is None:
            st.g_opt = {t: self._initial(t) for t in st.mine}
        else:
            f = self._factor(prev, size)
            st.g_opt = {t: self._resample(st.g_opt[t], size, f) for t in st.mine}
        st.work = torch.zeros(st.shape, device=self.device)     # the variable (re-assigned per frame, 312)
        # (a rank beyond the number of optimiser groups owns no frame: it only takes part in the collectives)
        first = st.d[st.mine[0]] if st.mine else (next(iter(st.d.values())) if st.d else
                                                  torch.zeros(size, device=self.device))
        if self.target == "c":
            st.gs = engine.ColourGridStylizer(self.loss, first, k=self.k, lr=st.lr,
                                              optimizer=getattr(self, "optimizer", "adam"), lap_n=self.lap_n,
                                              bwd_route=self.colour_bwd_route)
        elif self.is2d:
            st.gs = grid2d.GridStylizer2D(self.loss, first, target=self.target, lr=st.lr,
                                          optimizer=getattr(self, "optimizer", "adam"), adv_order=self.adv_order,
                                          lap_n=self.lap_n)
        else:
            st.gs = engine.GridStylizer(self.loss, first, k=self.k, target=self.target, lr=st.lr,
                                        optimizer=getattr(self, "optimizer", "adam"), adv_order=self.adv_order,
                                        lap_n=self.lap_n)
        st.opt_ = {}
        st.hist_octave.append([])

    def _initial(self, t):
        """the variable of frame t before the first step, at the current octave's size (``'_init'`` comes at full
        resolution)"""
        st = self._st
        if self.target == "d":
            return st.d[t].reshape(st.shape).clone()
        if st.v_init is not None:
            vi = st.v_init[t] if not isinstance(st.v_init, dict) else st.v_init.get(t)
            if vi is not None:
                full = tuple(int(n) for n in self.resolution)
                vi = self._dev(vi).reshape(full + (st.C,))
                return self._resample(vi, st.shape[:-1], self._factor(full, st.shape[:-1])).reshape(st.shape).clone()
        if self.target == "c":
            return self._resample(self._dev(st.c_noise), st.shape[:-1]).reshape(st.shape).clone()
        return torch.zeros(st.shape, device=self.device)

    @staticmethod
    def _has_every(x, frames):
        """does the params entry (list or {frame: array}) hold every one of ``frames``?"""
        if x is None:
            return False
        get = (lambda t: x[t] if t < len(x) else None) if not isinstance(x, dict) else (lambda t: x.get(t))
        return all(get(t) is not None for t in frames)

    def _infer(self, t, var):
        """frame t through its variable: (velocity the variable stands for or None, smoothed density, render with the
        identity rotation [1,H,W,3])"""
        st = self._st
        if self.is2d:
            return self._infer2d(t, var)
        if self.target == "c":
            return self._infer_colour(t, var)
        D, H, W_, _ = st.shape
        sourced = self.target in engine.SOURCED
        if self.target == "p":
            var = var.reshape(D, H, W_)
        vel = ops.source_velocity(self.target, var) if sourced else var
        if self.target != "d":
            # (the order the loop optimised through)
            advect = ops.advect_maccormack if self.adv_order == 2 else ops.advect_fwd
            d_adv = advect(st.d[t].unsqueeze(-1), vel).squeeze(-1)
        else:
            d_adv = var.reshape(D, H, W_)
        d_out = ops.smooth3d_relu_fwd(d_adv.contiguous(), float(self.k))
        return (vel if sourced else None), d_out, self.loss.d_img(d_out, self._identity)

    def _infer_colour(self, t, var):
        """``_infer`` of a colour frame: (None, the grey volume e_t, the colour image at the identity rotation [1,H,W,3]
        0..255).  Through the loop's own stylizer bound to the frame (the loop re-binds before every step)"""
        st = self._st
        st.gs.bind(st.d[t], var.reshape(st.shape).contiguous())
        return None, st.gs.grey(), st.gs.d_img(self._identity)

    def _infer2d(self, t, var):
        """``_infer`` on the 2-D path: (velocity [H,W,2] or None, the clipped image [H,W], its 0..255 rendering [1,H,W,3])"""
        st = self._st
        H, W_, _ = st.shape
        vel = None
        if self.target != "d":
            var = var.reshape(self._var_shape()).contiguous()
            if self.adv_order == 2 or self.target in engine.SOURCED:
                vel = var if self.target == "v" else ops.source2d_velocity(self.target, var)
            if self.adv_order == 2:
                d_adv = ops.advect_maccormack(st.d[t].unsqueeze(-1), vel).squeeze(-1)
            else:
                d_adv = ops.advect2d_source_fwd(self.target, st.d[t], var)
        else:
            d_adv = var.reshape(H, W_)
        img = ops.colour_clamp_gather(d_adv.reshape(H * W_, 1).contiguous())
        r, _ = ops.loss_net_input_fwd(img.view(1, H, W_, 1), want_x=False)
        return (vel if self.target in engine.SOURCED else None), img.view(H, W_), r

    def _var_shape(self):
        """the variable as the stylizer takes it and the result holds it"""
        st = self._st
        if self.is2d:
            return st.shape if self.target == "d" else ops.source2d_shape(self.target, *st.shape[:2])
        return st.shape[:3] if self.target == "p" else st.shape

    def _octave_variables(self):
        """what an octave leaves behind: the variable of every own key frame at the octave's size"""
        st = self._st
        shp = self._var_shape()
        return {t: st.g_opt[t].reshape(shp).cpu().numpy() for t in st.mine}

    def next_octave(self):
        """close the current octave (its key-frame renders go to ``d_intm``, its variables to ``opt_octave``) and set up
        the next, finer one: returns its size [D,H,W].  No exchange between ranks: every rank resamples its own frames
        and variables."""
        st = self._st
        if st.octave >= self.octave_n - 1:
            raise ValueError("next_octave(): octave %d of %d is the last" % (st.octave, self.octave_n))
        st.opt_octave.append(self._octave_variables())
        imgs = [self._infer(t, st.g_opt[t])[2].cpu().numpy().astype(np.uint8) for t in st.mine]
        st.d_intm.append(np.concatenate(imgs, axis=0) if imgs else np.zeros((0,) + st.shape[-3:-1] + (3,), np.uint8))
        prev = st.shape[:-1]
        st.octave += 1
        self._enter_octave(prev)
        return list(st.shape[:-1])

    def iterate(self):
        """one iteration of the frame loop (styler_3p.py:301-386): a stylisation step per own key frame, the halo
        exchange of the updates, their temporal alignment, ``g_opt += `` -- returns the per-key-frame losses (device
        tensor, summed over ranks)"""
        st = self._st
        losses = torch.zeros(len(st.keys), device=self.device)
        upd = {}
        # the reference's cosine schedule over the octave's iterations (util.py:49-53): lr_decay * lr at the first one, down
        # to lr; at the default factor 1 it returns lr * 1.0, the very number (every optimiser of the grid path)
        st.gs.lr = float(cosine_decay(len(st.hist_octave[-1]), max(int(self.iter), 1), st.lr, self.lr_decay))
        for j, t in enumerate(st.keys):
            if st.owner[t] == st.rank:
                slot = engine.optimizer_slot(getattr(self, "optimizer", "adam"), t, self.frames_per_opt)
                adam = st.opt_.get(slot)
                if adam is None:
                    adam = st.opt_[slot] = engine.make_optimizer(getattr(self, "optimizer", "adam"), lap_n=self.lap_n)
                st.work.copy_(st.g_opt[t])
                if self.is2d:
                    st.gs.bind(st.d[t], st.work.view(st.shape[:2] if self.target == "d" else self._var_shape()), adam)
                    losses[j] = st.gs.step()
                else:
                    st.gs.bind(st.d[t], st.work.view(st.shape if st.C > 1 else st.shape[:3]), adam)
                    losses[j] = st.gs.step(self._rot())
                dlt = torch.nan_to_num(st.gs.var.reshape(st.shape)) - st.g_opt[t]
                if self.target == "d":
                    dlt = dlt * st.d[t].reshape(st.shape)          # masking by original density (361-363)
                upd[t] = dlt
            # every rank draws the same view sequence whoever owns the frame (344-349)
            self._resample_views()
        if st.world > 1:
            parallel.all_reduce_sum_([losses], group=self.pg)
        if st.Wt is not None:
            got = parallel.exchange_frames(upd, st.need, st.owner, st.work, group=self.pg,
                                           need_by_rank=st.need_by_rank)
            for t in st.mine:
                st.g_opt[t] = st.g_opt[t] + self.aligned_update(t, got, st.u, st.Wt, st.keys)
        else:
            for t in st.mine:
                st.g_opt[t] = st.g_opt[t] + upd[t]
        st.hist.append(losses)
        st.hist_octave[-1].append(losses)
        return losses

    def key_frame_variables(self):
        """the variable of every key frame as the loop has left it, {frame: tensor} on every rank (a collective when the
        frames are sharded over ranks: every rank calls it)"""
        st = self._st
        if st.world > 1:
            return parallel.exchange_frames(st.g_opt, set(st.keys), st.owner, st.work, group=self.pg,
                                            need_by_rank=[set(st.keys)] * st.world)
        return st.g_opt

    def finish(self):
        """frame interpolation (392-397) + final inference of every frame whose density this rank holds: all of them
        in an unsharded run (or a sharded one prepared with every frame), the rank's own frames after
        ``prepare(frames_on_device=...)`` -- ``result['frames']`` lists which entries of ``d`` / ``r`` / ``v`` these
        are"""
        st = self._st
        allv = self.key_frame_variables()
        full = {t: allv[t] for t in st.keys}
        if self.interp > 1:
            w = np.linspace(0, 1, self.interp + 1)
            for t in range(0, st.F - 1, self.interp):
                for i in range(1, self.interp):
                    if t + self.interp < st.F:
                        full[t + i] = full[t] * float(1 - w[i]) + full[t + self.interp] * float(w[i])
        d_sty, r_sty, v_sty, u_sty = [], [], [], []        # (u_sty: the velocities of a run whose variable stands for one)
        c_sty = []                                         # ('c': the masked colours, as styler_2p returns them)
        sourced = self.target in engine.SOURCED
        present = [t for t in range(st.F) if t in st.d]
        for t in present:
            var = full.get(t)
            if var is None:                                        # trailing frames past the last key frame
                var = self._initial(t)
            if self.target == "p" or self.is2d:
                var = var.reshape(self._var_shape())               # (the potential in the shape of params['p_init'][t])
            vel, d_out, dimg = self._infer(t, var)
            d_sty.append(torch.abs(d_out).unsqueeze(-1).cpu().numpy())   # abs(): drop the sign-bit mask of -0.0
            r_sty.append(dimg[0].cpu().numpy().astype(np.uint8))
            v_sty.append(var.cpu().numpy())
            if self.target == "c":
                c_sty.append((torch.clamp(var, 0, 1) * torch.clamp(torch.abs(d_out), 0, 1).unsqueeze(-1)).cpu().numpy())
            if sourced:
                u_sty.append(vel.cpu().numpy())
        hist = [[float(x) for x in l_.cpu()] for l_ in st.hist]
        per_octave = [[float(x) for l_ in h for x in l_.cpu()] for h in st.hist_octave]
        return {"l": per_octave, "l_frames": hist, "d_intm": list(st.d_intm), "opt_octave": st.opt_octave + [self._octave_variables()],
                "octave_sizes": [[int(n) for n in sz] for sz in self.octave_sizes],
                "d": np.array(d_sty), "r": np.array(r_sty), "v": v_sty if self.target == "v" else u_sty if sourced else None,
                "s": v_sty if self.target == "s" else [a[..., 0] if self.is2d else a[..., :3] for a in v_sty] if self.target == "sp" else None,
                "phi": v_sty if self.target == "p" else [a[..., -1] for a in v_sty] if self.target == "sp" else None,
                "opt": v_sty, "p": None, "c": c_sty if self.target == "c" else None, "frames": present,
                **({"c_init": self._c_init_result()} if self.target == "c" else {})}

    def _c_init_result(self):
        """what a colour run started from, per frame at full resolution: the caller's ``c_init`` where given, else the one
        drawn field (the same array for every frame)"""
        st = self._st
        out = []
        for t in range(st.F):
            vi = None
            if st.v_init is not None:
                vi = st.v_init.get(t) if isinstance(st.v_init, dict) else (st.v_init[t] if t < len(st.v_init) else None)
            out.append(np.asarray(vi, np.float32) if vi is not None else st.c_noise)
        return out

    def run(self, params):
        self.prepare(params)
        for o in range(self.octave_n):
            if o:
                self.next_octave()
            for _ in range(self.iter):
                self.iterate()
        return self.finish()


def octave_sizes(resolution, octave_n, octave_scale):
    """the octaves' grid sizes, coarsest first, the last one ``resolution`` itself (styler_3p.py:240-247)"""
    sizes, dhw = [], np.array(resolution)
    for _ in range(int(octave_n)):
        sizes.append(dhw)
        dhw = (dhw // octave_scale).astype(int)
    sizes.reverse()
    return [[int(n) for n in sz] for sz in sizes]


class argparse_ns(object):
    """plain attribute bag for the loop state"""

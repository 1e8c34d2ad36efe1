"""The 2-D grid stylizer: the 2-D branches of the reference's TNST leftovers -- ``advect`` (transform.py:583-607),
``curl(is_2d=True)`` (517-527), ``grad`` (508-515) -- assembled the way ``engine.GridStylizer`` assembles the 3-D ones.

Per step, for a density d0 [H,W] (float32) and a variable of one of the kinds of ``ops.source2d_shape``:

    d^  = advect2d(d0, vel(var))             order 1; ``adv_order=2``: MacCormack on it (``ops.advect_maccormack``, nd = 2);
                                             target 'd': d^ = var, there is no advect
    img = clip(d^, 0, 1) as [1,H,W,1]        the reference's "value clipping for rendering" (styler_2p.py:88)
    ``engine.ImageStyleLoss`` on img         x255, grey -> 3 channels, - mean, optional ``resize_scale``; the loss network; style,
                                             TV, content, histogram, ``style_mask`` with d_gray = img
    TF ApplyAdam on the variable             one expression, the project's (``engine.TFAdamState``); or, with
                                             ``optimizer='lapnorm'``, Laplacian-normalised descent
                                             (``engine.LapDescentState``: ``lr`` a length in the variable's units)

A 2-D density is its own image: there is no smoothing, no render and no max-normalisation, and ``k`` is not read.
Velocities are [H,W,2] in ``ops.advect2d_fwd``'s units: component k moves along array axis k, one cell along an axis of n
nodes is 2/(n-1).  The variables ('v', 's', 'p', 'sp') are the D = 1 restriction of the 3-D ones (include/nfs_grid2d.h).

Not built in 2-D (say so here, where a user looks): dead-region masks and never-live skipping, slab sharding, L-BFGS, a
MacCormack transport between frames, ``batch_size > 1``."""
from __future__ import annotations

import os

import torch

from . import ops
from .engine import (SOURCED, LapDescentState, Replay, Stamp, TFAdamState, graph_from_env, holds, loss_capture_key,
                     make_optimizer)


class GridStylizer2D(object):
    """The part of ``engine.GridStylizer``'s surface that ``styler_grid`` uses -- ``var``, ``adam``, ``bind``, ``step``,
    ``gradient`` and the current advected density ``d_adv`` -- on an [H,W] grid.  Order 1 never stores the velocity of
    's', 'p', 'sp' (``ops.advect2d_source_fwd`` / ``_bwd``); 'v' takes the fused update (``ops.advect2d_bwd_adam``, which
    also writes the next step's forward sample), the others ``ops.source2d_velocity_bwd`` + ``ops.adam_tf_step``; order 2
    the unfused one throughout (the velocity materialised, ``ops.advect_maccormack`` / ``_bwd``).
    ``optimizer='lapnorm'`` (``lap_n`` pyramid levels): all five targets and both orders through ``variable_gradient`` ->
    ``LapDescentState.step`` over the variable as [H,W,C]; 'v' at order 1 takes the fused kernel
    (``ops.advect2d_descent``: update + next forward sample; ``NFS_FUSE_ADVECT=0`` turns it off).
    ``graph``: replay the loss chain as a captured hipGraph (``engine.Replay``); None: as ``NFS_GRAPH`` says, eager when
    it is unset."""

    def __init__(self, loss, d0, target="v", lr=0.1, optimizer="adam", adv_order=1, graph=None, lap_n=3):
        assert target in ("v", "d") + SOURCED, \
            "target is 'v' (velocity), 's' (stream function), 'p' (potential), 'sp' (both) or 'd' (density)"
        if optimizer == "lbfgs":
            raise ValueError("optimizer='lbfgs' is not built for the 2-D grid stylizer (GridStylizer2D): use 'adam'")
        assert int(adv_order) in (1, 2), "adv_order is 1 (semi-Lagrangian) or 2 (MacCormack)"
        assert d0.dim() == 2, "d0 is a 2-D density [H,W]"
        self.loss = loss
        self.d0 = d0.contiguous()
        self.target = target
        self.lr = float(lr)
        self.adam = make_optimizer(optimizer, lap_n=lap_n)
        if isinstance(self.adam, LapDescentState):
            self.adam.nd = 2
        self.fuse_advect = os.environ.get("NFS_FUSE_ADVECT", "1") != "0"     # (read by the 'lapnorm' step only)
        self.adv_order = int(adv_order)
        self.use_graph = bool(graph_from_env() if graph is None else graph)
        self._replay = None                          # (None: before the eager call that precedes a capture)
        self._pending = None
        self._owns_buffers = False
        H, W = d0.shape
        self.var = self.d0.clone() if target == "d" else \
            torch.zeros(ops.source2d_shape(target, H, W), dtype=torch.float32, device=d0.device)
        self.d_adv = self.img = None                 # the advected density / the clipped image of the current forward
        # order 1: advect2d(d0, vel(var)) in a fixed buffer (a captured graph reads it by address; the fused 'v' update
        # writes the next step's sample into it), and the stamp of what it was computed from
        self._adv_buf = torch.empty(H, W, dtype=torch.float32, device=d0.device)
        self._adv_src = None
        # order 2: the first-order sample, the limiter's decisions and the velocity of the CURRENT forward (the adjoint's)
        self._mc_fwd = self._mc_keep = self._mc_vel = None

    # ---- frames -----------------------------------------------------------------------------------------------------------
    def bind(self, d0, var=None, adam=None):
        """Re-point the stylizer at another frame of the same shape (takes effect at the next step / gradient): a pointer
        swap, or with hipGraph replay a copy into the private buffers the captured graph has baked in."""
        assert tuple(d0.shape) == tuple(self.d0.shape)
        self._pending = (d0, var)
        if adam is not None:
            if not isinstance(adam, (TFAdamState, LapDescentState)):
                raise ValueError("the 2-D grid stylizer steps with TF ApplyAdam or 'lapnorm' (L-BFGS is not built)")
            self.adam = adam
            if isinstance(adam, LapDescentState):
                adam.nd = 2

    def _apply_binding(self):
        if self._pending is None:
            return
        d0, var = self._pending
        self._pending = None
        if self.use_graph:
            if not self._owns_buffers:
                self.d0, self.var = self.d0.clone(), self.var.clone()
                self._owns_buffers = True
            self.d0.copy_(d0)
            if var is not None:
                self.var.copy_(var.reshape(self.var.shape))
        else:
            self.d0 = d0.contiguous()
            if var is not None:
                assert tuple(var.shape) == tuple(self.var.shape) and var.is_contiguous()
                self.var = var

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def velocity(self):
        """the velocity [H,W,2] the density is advected along"""
        assert self.target != "d", "the density variable has no velocity"
        return self.var if self.target == "v" else ops.source2d_velocity(self.target, self.var)

    def _stored(self):
        return self.target != "d" and self.adv_order == 1

    def _advect_now(self):
        """order 1: advect2d(d0, vel(var)) -- what the previous step's Adam kernel left when it is still current"""
        if not holds(self._adv_src, self.var, self.d0):
            ops.advect2d_source_fwd(self.target, self.d0, self.var, out=self._adv_buf)
            self._adv_src = Stamp(self.var, self.d0)
        return self._adv_buf

    def _advect_order2(self):
        d3 = self.d0.unsqueeze(-1)
        if self._mc_fwd is None:
            self._mc_fwd = torch.empty_like(d3)
            self._mc_keep = ops.maccormack_mask(d3.shape, d3)
        vel = self.var
        if self.target in SOURCED:
            if self._mc_vel is None:
                self._mc_vel = torch.empty(tuple(self.d0.shape) + (2,), dtype=torch.float32, device=self.d0.device)
            vel = ops.source2d_velocity(self.target, self.var, out=self._mc_vel)
        return ops.advect_maccormack(d3, vel, keep=self._mc_keep, d_fwd=self._mc_fwd).squeeze(-1)

    def forward_field(self):
        """d_adv [H,W] and img = clip(d_adv, 0, 1) [1,H,W,1] of the current variable"""
        self._apply_binding()
        if self.target == "d":
            self.d_adv = self.var
        elif self.adv_order == 2:
            self.d_adv = self._advect_order2()
        else:
            self.d_adv = self._advect_now()
        H, W = self.d0.shape
        self.img = ops.colour_clamp_gather(self.d_adv.reshape(H * W, 1)).view(1, H, W, 1)
        return self.img

    def _chain(self):
        """forward + adjoint down to the advected density: (loss [1], dL/d d_adv [H,W])"""
        img = self.forward_field()
        loss, g_img = self.loss.loss_and_grad(img, img)
        return loss, ops.clamp01_bwd(g_img.view(self.d_adv.shape), self.d_adv.contiguous())

    def _capture_key(self):
        return loss_capture_key(self.loss) + (int(self.d0.data_ptr()), int(self.var.data_ptr()), self.target,
                                              self.adv_order)

    def _chain_graphed(self):
        """``_chain`` as one hipGraph: the first call runs eagerly (lazy state: packed filters, workspaces), the second is
        captured, later ones replay; a change of what the capture bakes in drops the graph.  The captured chain starts
        from the stored forward sample (order 1), which is brought up to date eagerly."""
        self._apply_binding()
        if self._stored():
            self._advect_now()
        key = self._capture_key()
        if self._replay is None or self._replay.stale(key):
            self._replay = Replay()
            return self._chain()
        return self._replay(key, (), self._chain)

    def _loss_gradient(self):
        return self._chain_graphed() if self.use_graph else self._chain()

    # ---- adjoint and update ---------------------------------------------------------------------------------------------------
    def _velocity_gradient(self, g_adv):
        """dL/d(velocity) [H,W,2] from dL/d(advected density), along the forward's own velocity"""
        if self.adv_order == 2:
            vel = self.var if self.target == "v" else self._mc_vel
            return ops.advect_maccormack_bwd(self.d0.unsqueeze(-1), vel, self._mc_fwd, self._mc_keep,
                                             g_adv.unsqueeze(-1), need_d=False, need_vel=True)[1]
        return ops.advect2d_source_bwd(self.target, self.d0, self.var, g_adv)

    def variable_gradient(self, g_adv):
        if self.target == "d":
            return g_adv
        g_vel = self._velocity_gradient(g_adv)
        return g_vel if self.target == "v" else ops.source2d_velocity_bwd(self.target, g_vel)

    def gradient(self):
        """one forward + backward: (loss [1], gradient with respect to the variable)"""
        loss, g_adv = self._loss_gradient()
        return loss, self.variable_gradient(g_adv)

    def step(self):
        """one iteration: loss, gradient, the update; returns the loss (a 0-d device tensor of its own)"""
        loss, g_adv = self._loss_gradient()
        total = loss.sum()
        if isinstance(self.adam, LapDescentState):
            g = self.variable_gradient(g_adv).reshape(self.var.shape)
            if self.target == "v" and self.adv_order == 1 and self.fuse_advect:
                self.adam.step_through_advect2d(self.var, self.d0, g, self.lr, self._adv_buf)
                self._adv_src = Stamp(self.var, self.d0)
            else:
                self.adam.step(self.var, g, self.lr, nd=2)
        elif self.target != "d" and self.adv_order == 1:
            _, hyper = self.adam._begin_step(self.var, self.lr)
            if self.target == "v":
                ops.advect2d_bwd_adam(self.d0, self.var, g_adv, self.adam.m, self.adam.v, *hyper, adv_next=self._adv_buf)
                self._adv_src = Stamp(self.var, self.d0)
            else:
                ops.adam_tf_step(self.var, self.adam.m, self.adam.v,
                                 ops.source2d_velocity_bwd(self.target, self._velocity_gradient(g_adv)), *hyper)
        else:
            self.adam.step(self.var, self.variable_gradient(g_adv).reshape(self.var.shape), self.lr)
        return total

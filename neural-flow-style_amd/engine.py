"""The stylisation step: density volume -> (rotate+)render -> loss net -> Gram style
loss, and the whole adjoint chain back to the volume, on the HIP kernels.

This is the body of one ``sess.run(train_op)`` of the reference (styler_3p.py:147-164 +
styler_base.py:33-57,127-231) with views batched: all V local views go through the
renderer and VGG as one batch, the field gradient accumulates over views in one buffer.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from . import ops, parallel
from .config import COLOUR_RENDERS, colour_background, colour_exposure

HOST_BOUND = 0.85       # issue time over this share of the wall time: the GPU finished as soon as the host had issued the work


class Stamp(object):
    """what a stored result was computed from: the tensors' identities and their torch version counters.  An in-place
    torch op on one of them (also through a ``detach()`` view, which shares the counter) or another tensor in its place
    makes it stale; a write that bypasses the counter (``tensor.data``, a kernel called on ``data_ptr()``) is not seen."""
    __slots__ = ("seen",)

    def __init__(self, *tensors):
        self.seen = tuple((t, t._version) for t in tensors)


def holds(stamp, *tensors):
    """do these same tensors, unmodified, still stand where ``stamp`` was taken?  (None or an empty stamp: never)"""
    seen = stamp.seen if stamp is not None else ()
    if not seen or len(seen) != len(tensors):
        return False
    for (t0, version), t in zip(seen, tensors):
        if t0 is not t or version != t._version:
            return False
    return True


class Replay(object):
    """one captured hipGraph of ``body(*inputs)``, the key it was captured under and the static copies of its tensor
    inputs (None entries pass through).  Called with ``(key, inputs, body)`` it drops a graph captured under another key,
    captures where there is none, copies in the inputs that changed and replays; it returns what ``body`` returned under
    capture (valid until the next replay).  Warm-up calls and the eager / graph choice are the caller's."""

    def __init__(self):
        self.graph = self.key = self.static = self.stamps = self.out = None

    def stale(self, key):                # (a graph captured under ANOTHER key is held)
        return self.graph is not None and key != self.key

    def __call__(self, key, inputs, body):
        if self.stale(key):
            self.__init__()
        if self.graph is None:
            self.static = [None if t is None else t.clone() for t in inputs]
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.out = body(*self.static)
            self.graph, self.key = g, key
            self.stamps = [None if t is None else Stamp(t) for t in inputs]
        for i, t in enumerate(inputs):
            # (the static buffer itself, or the same unmodified tensor as last time -- as just after a capture: no copy launch)
            if t is not None and t is not self.static[i] and not holds(self.stamps[i], t):
                self.static[i].copy_(t)
                self.stamps[i] = Stamp(t)
        self.graph.replay()
        return self.out


def issue_and_wall(fn):
    """one call of ``fn`` between two synchronisations -> seconds (the host needed to issue it, until the GPU finished it)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    return t_issue, time.perf_counter() - t0


def graph_from_env():
    """``NFS_GRAPH`` as True ('1': hipGraph replay forced on), None (unset: the choice is measured) or False (else: off)"""
    env = os.environ.get("NFS_GRAPH")
    return None if env is None else env == "1"


def _channels(acts, name, F):
    """logical channel count of a loss-network tensor: Inception module outputs come in rows padded to a multiple of 64
    floats (``acts.channels``); VGG activations are what their shape says"""
    ch = getattr(acts, "channels", None)
    return int(ch[name]) if ch is not None and name in ch else int(F.shape[-1])


def _post_relu(name):
    """True for tensors that are ReLU outputs (or pools / concatenations of them): a gradient injected there may carry
    the ReLU mask.  The Inception graph's '*_pre_relu' tensors are not."""
    return not (name.endswith("_pre_relu") or name.endswith("_pre_activation"))


def _logical(acts, name):
    """(contiguous tensor of the logical channels, padded?)"""
    F = acts[name]
    c = _channels(acts, name, F)
    return (F, False) if c == F.shape[-1] else (F[..., :c].contiguous(), True)


def _add_logical(sg, name, F, g_log):
    """add a gradient over the logical channels into the (padded) entry of the adjoint chain"""
    g = sg.get(name)
    if g is None:
        g = sg[name] = torch.zeros_like(F)
    g[..., :g_log.shape[-1]].add_(g_log)


class RenderStyleLoss(object):
    """loss(d) = w_style * sum_v sum_l w_l * || G_l(vgg(render(rotate(d, R_v)))) - G_l^style ||^2
    (+ w_tv * TV).  ``loss_and_grad`` returns the per-view losses and ADDS dL/dd to ``g_d``."""

    def __init__(self, net, style_layer, w_style_layer, w_style=1.0, transmit=0.01, render_liquid=False,
                 resize_scale=1.0, rotate=True, w_tv=0.0, v_batch=1, w_content=0.0, content_layer=None,
                 content_channel=0, w_content_amp=100.0, w_hist=0.0, hist_layer=(), w_hist_layer=(), ray_mode=""):
        self.net = net
        # styler_base.py:152: the style term exists only with w_style != 0 (the semantic-transfer runs of run.bat:14-20
        # have w_style 0, the flag default, and no style image)
        self.layers = list(style_layer) if float(w_style) else []
        self.w_layers = [float(w) for w in w_style_layer][:len(self.layers)] if self.layers else []
        assert len(self.layers) == len(self.w_layers)
        self.w_style = float(w_style)
        self.tau = float(transmit)
        # ray integral: the reference's transmittance (smoke, max-normalised) / liquid forms, or -- north_star's "per-ray
        # max / mean" -- reduce_max (the line the reference keeps commented out, styler_3p.py:149) / reduce_mean along the
        # ray; like the liquid form these are not max-normalised
        if ray_mode not in ("", None, "transmit", "liquid", "max", "mean"):
            raise ValueError("ray_mode %r: '', 'transmit', 'liquid', 'max' or 'mean'" % (ray_mode,))
        self.mode = {"max": 2, "mean": 3, "liquid": 1, "transmit": 0}.get(ray_mode or "", 1 if render_liquid else 0)
        self.resize_scale = float(resize_scale)
        self.rotate = bool(rotate)
        self.w_tv = float(w_tv)
        self.v_batch = int(v_batch)
        self.two_pass_adjoint = True   # False: single fused adjoint with global atomics (less memory)
        # optional: view groups that run concurrently through VGG on separate HIP streams (>= 4 local views).
        # With the direct conv kernels two groups overlapped each other's launch tails (7.32 -> 7.01 ms/step);
        # with the Winograd path one batch of all views on one stream is fastest (8 views of 200^2: 1 stream
        # 4.73 ms/step, 2 streams 4.79, 4 streams 6.38), so that is the default.
        # all style layers' Gram work as three launches after the forward pass (default) / per layer (side stream)
        self.gram_grouped = os.environ.get("NFS_GRAM_GROUP", "1") != "0"
        self.gram_side_stream = os.environ.get("NFS_GRAM_STREAM", "1") != "0"
        self._side = None
        self.vgg_streams = int(os.environ.get("NFS_VGG_STREAMS", "1"))
        self.view_groups = int(os.environ.get("NFS_VIEW_GROUPS", "1"))
        self._streams = []
        order = [s[0] for s in net.seq]
        # content term on a layer of the same network (styler_base.py:135-150): channel maximisation, -mean, or the
        # distance to a content image's features (set_content_image)
        self.w_content = float(w_content) if content_layer else 0.0
        self.content_layer = content_layer if self.w_content else None
        self.content_channel = int(content_channel or 0)
        self.w_content_amp = float(w_content_amp)
        self.content_feature = None
        if self.content_layer is not None:
            kinds = dict((s[0], s[1]) for s in net.seq)
            if kinds.get(self.content_layer) != "conv":
                raise KeyError("content_layer %r is not a conv layer of the loss network" % (self.content_layer,))
        # histogram term (styler_base.py:187-209): layers of the loss network and / or 'input' (= d_img)
        self.w_hist = float(w_hist)
        self.hist_layers = list(hist_layer) if self.w_hist else []
        self.w_hist_layers = [float(w) for w in w_hist_layer] if self.w_hist else []
        if len(self.w_hist_layers) == 1 and len(self.hist_layers) > 1:
            self.w_hist_layers = self.w_hist_layers * len(self.hist_layers)
        if len(self.w_hist_layers) != len(self.hist_layers):
            raise ValueError("w_hist_layer has %d entries for %d hist layers (one weight, or one per layer)"
                             % (len(self.w_hist_layers), len(self.hist_layers)))
        for name in self.hist_layers:
            if "input" not in name and name not in order:
                raise KeyError("hist_layer %r is not a layer of the loss network" % (name,))
        self.hist_targets = None
        vgg_hist = [n for n in self.hist_layers if "input" not in n]
        wanted = self.layers + vgg_hist + ([self.content_layer] if self.content_layer else [])
        if not wanted:
            raise ValueError("no loss term reaches the loss network: w_style 0 (or no style layer) and no content / "
                             "histogram layer")
        for n in wanted:
            if n not in order:
                raise KeyError("%r is not a tensor of the loss network" % (n,))
        self.top = max(wanted, key=order.index)
        self.style_grams = None

    @property
    def liquid(self):
        """True for every ray integral that is not max-normalised (all but the transmittance form)"""
        return self.mode != 0

    @liquid.setter
    def liquid(self, on):
        self.mode = (1 if on else 0) if self.mode < 2 else self.mode

    def set_hist_image(self, style_img):
        """template features of the histogram term: style_img float32 [h,w,3] in 0..255 at the loss-net input size
        (styler_base.py:280-309: the style image fed at d_img, each hist layer fetched)"""
        if not self.hist_layers:
            self.hist_targets = None
            return None
        dev = self.net.device
        s = torch.as_tensor(np.asarray(style_img, np.float32)).to(dev)
        mean = torch.tensor([0.485 * 255, 0.456 * 255, 0.406 * 255], dtype=torch.float32, device=dev)
        vgg_hist = [n for n in self.hist_layers if "input" not in n]
        acts = {}
        if vgg_hist:
            order = [q[0] for q in self.net.seq]
            acts = self.net.forward((s - mean).unsqueeze(0).contiguous(), max(vgg_hist, key=order.index))
        self.hist_targets = {n: (s.unsqueeze(0).contiguous() if "input" in n else _logical(acts, n)[0].clone())
                             for n in self.hist_layers}
        return self.hist_targets

    def _hist_job(self, acts, sg, loss, d_gray=None):
        """histogram losses on layers of the loss network: per-view losses into ``loss``, gradients (ReLU-masked) into
        the layers' entries of ``sg``.  ``d_gray`` [B,H,W,1]: the masked branch (styler_base.py:196-201) -- the density
        mask, bicubic-resized to each layer, removes its zero pixels from the source of the match.

        Deliberate divergence from the mounted reference (documented in DESIGN.md section 5, INTEGRATION.md and the
        hist.hip header): the template of a layer is the style image's features OF THAT LAYER and the weight is
        ``w_hist_layer`` -- the reference's lines 203 / 207 read the stale ``style_feature`` / ``w_style_layer`` left
        over from the style loop (the last style layer's placeholder and weight), which only coincide with this when
        hist_layer == [style_layer[-1]] and w_hist_layer == [w_style_layer[-1]]."""
        for name, wl in zip(self.hist_layers, self.w_hist_layers):
            if "input" in name:
                continue
            assert self.hist_targets is not None, "call set_hist_image first"
            F, padded = _logical(acts, name)
            m = None if d_gray is None else ops.resize_bicubic_tf1(d_gray.contiguous(), F.shape[1], F.shape[2])
            if padded:
                g = torch.zeros_like(F)
            else:
                g = sg.get(name)
                if g is None:
                    g = sg[name] = torch.zeros_like(F)
            ops.hist_loss(F, self.hist_targets[name], wl * self.w_hist, loss, g, relu_mask=_post_relu(name), mask=m)
            if padded:
                _add_logical(sg, name, acts[name], g)

    def _hist_input(self, dimg, loss, g_x, d_gray=None):
        """hist_layer 'input': the term on d_img itself (gradient wrt d_img = gradient wrt the mean-subtracted x)"""
        for name, wl in zip(self.hist_layers, self.w_hist_layers):
            if "input" in name:
                assert self.hist_targets is not None, "call set_hist_image first"
                m = None if d_gray is None else ops.resize_bicubic_tf1(d_gray.contiguous(), dimg.shape[1], dimg.shape[2])
                ops.hist_loss(dimg, self.hist_targets[name], wl * self.w_hist, loss, g_x, relu_mask=False, mask=m)

    def set_content_image(self, content_img, top_k=0):
        """content_img: float32 [h,w,3] in 0..255 at the loss-net input size, or None (styler_base.py:232-247);
        ``top_k`` > 0 (with the classifier logits as content layer): only the k largest |logits| of every row of the
        fetched feature survive, the others are zeroed (styler_base.py:240-245)"""
        if content_img is None or self.content_layer is None:
            self.content_feature = None
            return None
        dev = self.net.device
        s = torch.as_tensor(np.asarray(content_img, np.float32)).to(dev)
        mean = torch.tensor([0.485 * 255, 0.456 * 255, 0.406 * 255], dtype=torch.float32, device=dev)
        acts = self.net.forward((s - mean).unsqueeze(0).contiguous(), self.content_layer)
        cf = _logical(acts, self.content_layer)[0].clone()
        if top_k and top_k > 0:
            if "softmax2_pre_activation" not in self.content_layer:
                raise AssertionError("top_k > 0 needs content_layer softmax2_pre_activation (styler_base.py:241)")
            rows = cf.reshape(-1, cf.shape[-1])
            keep = torch.zeros_like(rows, dtype=torch.bool)
            keep.scatter_(1, rows.abs().topk(int(top_k), dim=1).indices, True)
            cf = (rows * keep).reshape(cf.shape).contiguous()
        self.content_feature = cf
        return self.content_feature

    # -- style targets (styler_base.py:249-278: the style image enters at d_img) -------------
    def out_hw(self, H, W):
        if np.isclose(self.resize_scale, 1):
            return H, W
        # int(float32(scale) * float32(dim)) as the TF graph computes it (styler_base.py:36-37)
        return int(np.float32(self.resize_scale) * np.float32(H)), int(np.float32(self.resize_scale) * np.float32(W))

    def set_style_image(self, style_img):
        """style_img: float32 [h,w,3] in 0..255 already at the loss-net input size"""
        dev = self.net.device
        s = torch.as_tensor(np.asarray(style_img, np.float32)).to(dev)
        mean = torch.tensor([0.485 * 255, 0.456 * 255, 0.406 * 255], dtype=torch.float32, device=dev)
        x = (s - mean).unsqueeze(0).contiguous()
        acts = self.net.forward(x, self.top)
        self.style_grams = {}
        for name in self.layers:
            F = acts[name]
            _, h, w, _ = F.shape
            self.style_grams[name] = ops.gram_fwd(F, 1.0 / (2.0 * h * w * _channels(acts, name, F)))
        return self.style_grams

    # -- forward only (rendered image, used for the final inference) ------------------------
    def _coef_form(self, V, shape):
        """transmittance rendering of a shape the segmented forward takes: the adjoint runs without the render-adjoint
        pass over the rotated volume (K4a; ``NFS_RENDER_COEF=0`` keeps that pass)"""
        return (self.mode == 0 and os.environ.get("NFS_RENDER_COEF", "1") != "0"
                and ops.render_coef_layout(V, *shape) is not None)

    def render(self, d, rot, keep_rotated=False, normalise=True):
        self.d_rot = None
        self._seg = None
        if self.rotate:
            if keep_rotated:
                self.d_rot = torch.empty((rot.shape[0],) + tuple(d.shape), dtype=torch.float32, device=d.device)
            if self.mode >= 2:                       # max / mean: rotate, then the ray reduction on the kept volume
                self.d_rot = ops.rotate_fwd(d.unsqueeze(-1), rot).squeeze(-1)
                img, rs = ops.render_fwd(self.d_rot, self.tau, self.mode)
                if not keep_rotated:
                    self.d_rot = None
            elif keep_rotated and self._coef_form(rot.shape[0], d.shape):
                # the kept volume holds u, not the samples: the rotate adjoint forms the sample gradient from it
                img, rs, _, self._seg = ops.rotate_render_fwd_coef(d, rot, self.tau, u_rot=self.d_rot)
            else:
                img, rs = ops.rotate_render_fwd(d, rot, self.tau, self.mode, d_rot=self.d_rot)
        else:
            img, rs = ops.render_fwd(d.unsqueeze(0), self.tau, self.mode)
        gmax = None
        V = img.shape[0]
        if self.liquid:
            norm = img
        elif normalise:
            norm, gmax = ops.maxnorm_fwd(img, max(V // self.v_batch, 1))
        else:
            norm = None                              # (the caller normalises: _chain's fused max-norm + loss-net input)
        return img, rs, norm, gmax

    def d_img(self, d, rot):
        """the 0..255 3-channel image the loss net sees (``self.d_img`` of the reference)"""
        _, _, norm, _ = self.render(d, rot)
        V, H, W = norm.shape
        H2, W2 = self.out_hw(H, W)
        dimg, _ = ops.loss_net_input_fwd(norm.unsqueeze(-1), H2, W2, want_x=False)
        return dimg

    def _gram_job(self, name, F, loss, unmasked=None, channels=None):
        """Gram matrix, style loss and the Gram gradient dF of one style layer.  dF carries the layer's ReLU mask unless
        the data gradient that will add it applies that mask anyway (then the name is recorded in ``unmasked`` and the
        GEMM epilogue does not read F a second time)."""
        wl = self.w_layers[self.layers.index(name)]
        _, h, w, c = F.shape
        scale = 1.0 / (2.0 * h * w * (channels or c))
        G = ops.gram_fwd(F, scale)
        Dm = ops.style_loss_fwd(G, self.style_grams[name], wl * self.w_style, loss)
        defer = unmasked is not None and self._defers_mask(name, F)
        if defer:
            unmasked.add(name)
        return ops.gram_bwd(F, Dm, scale, relu_mask=_post_relu(name) and not defer)

    def _defers_mask(self, name, F):
        """True when dF of style layer ``name`` is handed over WITHOUT its ReLU mask: the data gradient that adds it
        applies that very mask to the sum anyway ("Deferred ReLU mask")"""
        return (name != self.top and name != self.content_layer and os.environ.get("NFS_NO_DEFER_MASK") is None
                and self.net.masks_addend_of(name, F.shape))

    def _vgg_loss_grad(self, x, total_out=None):
        """x [B,h,w,3] (mean-subtracted) -> (dL/dx, per-image losses [B] of the style / content / histogram terms).

        Default: the Gram work of ALL style layers runs after the forward pass as three launches (tile pairs of every
        layer, slab reduction with the style loss folded in, the five Gram gradients as one batched GEMM launch:
        ``ops.gram_style_group``); the loss leaves the kernels as per-block partial sums (no atomics) and is summed
        here.  ``NFS_GRAM_GROUP=0`` restores the per-layer chain (Gram -> loss -> dF per layer), which can run on a
        side stream as soon as a layer exists (``gram_side_stream``)."""
        sg = {}
        unmasked = set()                            # style layers whose dF is handed over without its ReLU mask
        if not self.layers:                          # content / histogram terms only (run.bat:14-20: w_style 0)
            acts = self.net.forward(x, self.top, keep=self._keep())
            loss = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
            self._content_job(acts, sg, loss)
            self._hist_job(acts, sg, loss)
            return self.net.backward(acts, sg, self.top, unmasked=unmasked), loss
        if self.gram_grouped:
            acts = self.net.forward(x, self.top, keep=self._keep())
            Fs = [acts[n] for n in self.layers]
            masks = []
            for n, F in zip(self.layers, Fs):
                d = self._defers_mask(n, F)
                if d:
                    unmasked.add(n)
                masks.append(_post_relu(n) and not d)
            parts, dFs, _ = ops.gram_style_group(Fs, [self.style_grams[n] for n in self.layers],
                                                 [w * self.w_style for w in self.w_layers], masks,
                                                 channels=[_channels(acts, n, F) for n, F in zip(self.layers, Fs)])
            sg.update(zip(self.layers, dFs))
            if total_out is not None:                # (sums_total(): no other loss term) the total straight from the
                torch.sum(parts.view(-1), dim=0, keepdim=True, out=total_out)     # per-block partial sums: one launch
                return self.net.backward(acts, sg, self.top, unmasked=unmasked), None
            loss = parts.sum(0)
            self._content_job(acts, sg, loss)
            self._hist_job(acts, sg, loss)
            return self.net.backward(acts, sg, self.top, unmasked=unmasked), loss
        loss = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
        if not self.gram_side_stream:
            acts = self.net.forward(x, self.top, keep=self._keep())
            for name in self.layers:
                sg[name] = self._gram_job(name, acts[name], loss, unmasked, _channels(acts, name, acts[name]))
            self._content_job(acts, sg, loss)
            self._hist_job(acts, sg, loss)
            return self.net.backward(acts, sg, self.top, unmasked=unmasked), loss
        main = torch.cuda.current_stream(x.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=x.device)
        side = self._side
        side.wait_stream(main)                      # style targets were produced on the main stream

        top_inline = os.environ.get("NFS_GRAM_TOP_INLINE", "1") != "0"

        def on_layer(name, F):
            if name not in self.layers:
                return
            if name == self.top and top_inline:
                # nothing follows the top layer on the main stream: its Gram work is the critical path, run it in
                # place (no event hand-over to the side stream and back)
                sg[name] = self._gram_job(name, F, loss, unmasked)
                return
            ev = torch.cuda.Event()
            ev.record(main)
            side.wait_event(ev)
            capturing = torch.cuda.is_current_stream_capturing()
            if not capturing:                       # a captured step owns its buffers: nothing to tell the allocator
                F.record_stream(side)
            with torch.cuda.stream(side):
                sg[name] = self._gram_job(name, F, loss, unmasked)
            if not capturing:
                sg[name].record_stream(main)

        acts = self.net.forward(x, self.top, on_layer=on_layer, keep=self._keep())
        main.wait_stream(side)
        self._content_job(acts, sg, loss)
        self._hist_job(acts, sg, loss)
        return self.net.backward(acts, sg, self.top, unmasked=unmasked), loss

    def _batch_views(self, V):
        """views per loss-net batch of the reference graph: v_batch (RenderStyleLoss: a property of the run, not of
        the shard -- a rank holding fewer views still divides by v_batch); the whole image batch for the 2-D loss
        (``v_batch is None``: one sess.run sees every image)"""
        return float(V) if self.v_batch is None else float(max(int(self.v_batch), 1))

    def _keep(self):
        """the activations the loss itself reads: the forward pass need not materialise the full-resolution output
        of a pooled layer that is not among them"""
        return (set(self.layers) | ({self.content_layer} if self.content_layer else set())
                | set(n for n in getattr(self, "hist_layers", []) if "input" not in n))

    def _content_job(self, acts, sg, loss):
        """adds the content term's per-view losses into ``loss`` and its gradient into the layer's entry of ``sg``"""
        if self.content_layer is None:
            return
        F, padded = _logical(acts, self.content_layer)
        V = F.shape[0]
        # the reference's means run over one loss-net batch (v_batch views); here all V views share the batch
        w = self.w_content * V / self._batch_views(V)
        if padded:
            g = torch.zeros_like(F)
        else:
            g = sg.get(self.content_layer)
            if g is None:
                g = sg[self.content_layer] = torch.zeros_like(F)
        ops.content_loss(F, w, loss, g, channel=self.content_channel, target=self.content_feature,
                         amp=self.w_content_amp, signed=not _post_relu(self.content_layer))
        if padded:
            _add_logical(sg, self.content_layer, acts[self.content_layer], g)

    # -- the hot step -----------------------------------------------------------------------
    accepts_live = True       # loss_and_grad(..., live=, dilate=): see ops.rotate_bwd_coef

    def _chain(self, d, rot, g_d, overwrite=False, total_out=None, live=None, dilate=1):
        """render -> loss net -> Gram losses -> full adjoint for the views ``rot`` on the CURRENT stream;
        g_d [D,H,W] += dL/dd (= with ``overwrite``, two-pass rotate adjoint only); returns the per-view losses"""
        D, H, W = d.shape
        H2, W2 = self.out_hw(H, W)
        hist_in = any("input" in n for n in self.hist_layers)
        # smoke render at the loss net's own size with nothing reading d_img: max-normalisation and the loss-net input
        # in one pass each way (same arithmetic; two launches and the [V,H,W] intermediates less per direction)
        fused_in = (not self.liquid and (H2, W2) == (H, W) and not (self.w_tv > 0 or hist_in)
                    and os.environ.get("NFS_FUSE_INPUT", "1") != "0")
        img, rs, norm, gmax = self.render(d, rot, keep_rotated=self.two_pass_adjoint, normalise=not fused_in)
        d_rot, seg = self.d_rot, self._seg
        self.d_rot = self._seg = None
        V = img.shape[0]
        if fused_in:
            dimg = None
            x, gmax = ops.maxnorm_input_fwd(img, max(V // self.v_batch, 1))
        else:
            dimg, x = ops.loss_net_input_fwd(norm.unsqueeze(-1), H2, W2, want_d_img=self.w_tv > 0 or hist_in)
        g_x, loss = self._vgg_loss_grad(x, total_out=total_out)
        if hist_in:
            self._hist_input(dimg, loss, g_x)
        if self.w_tv > 0:
            # the reference's batch mean runs over one loss-net batch (v_batch views, styler_base.py:211-213); with
            # all V local views in one batch the weight is rescaled so that the term is w_tv * sum_v TV_v / v_batch
            # whatever the number of views this rank holds -- ALSO when a rank holds fewer views than one loss-net
            # batch (8 views over 8 ranks with v_batch 2): the divisor is v_batch, never the local V, so that sharded
            # runs sum to the single-rank value
            tv = torch.zeros(1, dtype=torch.float32, device=d.device)
            ops.tv_loss(dimg, self.w_tv * V / self._batch_views(V), tv, g_x)
            loss = loss + tv / V
        if fused_in:
            g_img = ops.maxnorm_input_bwd(img, gmax, g_x)
        else:
            g_norm = ops.loss_net_input_bwd(g_x, H, W, 1).reshape(V, H, W)
            g_img = g_norm if self.liquid else ops.maxnorm_bwd(img, gmax, g_norm)
        if self.rotate and d_rot is not None and seg is not None:
            # u form: per-(ray, segment) coefficients from the image gradient, then the rotate adjoint alone
            ab, bounds = ops.render_ray_coef(g_img, seg, self.tau)
            ops.rotate_bwd_coef(d_rot, ab, rot, bounds, g_d_acc=g_d, overwrite=overwrite, live=live, dilate=dilate)
        elif self.rotate and d_rot is not None:
            # two-pass adjoint: streaming render adjoint on the kept rotated volume (re-using its
            # buffer for the per-sample gradient) + LDS-tiled output-stationary rotate adjoint
            g_rot, g_max = ops.render_bwd(d_rot, rs, g_img, self.tau, self.mode, g_d=d_rot, want_max=True)
            ops.rotate_bwd(g_rot.unsqueeze(-1), rot, g_d_acc=g_d.unsqueeze(-1), g_max=g_max, overwrite=overwrite)
        elif self.rotate:
            assert self.mode < 2, "the max / mean ray modes use the two-pass adjoint"
            ops.rotate_render_bwd(d, rot, rs, g_img, self.tau, self.mode, g_d_acc=g_d)
        elif overwrite:
            # one unrotated view: the render adjoint IS dL/dd -- written straight into g_d (no zero fill, no add pass)
            ops.render_bwd(d.unsqueeze(0), rs, g_img, self.tau, self.mode, g_d=g_d.unsqueeze(0))
        else:
            g_d.add_(ops.render_bwd(d.unsqueeze(0), rs, g_img, self.tau, self.mode)[0])
        return loss

    def writes_gradient(self, V):
        """True when loss_and_grad(..., overwrite=True) can write g_d without a zero fill: one view batch through the
        tiled rotate adjoint, whose tiles partition the volume -- or the single unrotated view, whose render adjoint is
        the gradient itself"""
        if not self.rotate:
            return True
        ngroups = self.view_groups if (V >= 4 and self.rotate and self.v_batch == 1) else 1
        return bool(self.two_pass_adjoint and min(ngroups, V) <= 1)

    def sums_total(self, V):
        """True when loss_and_grad(..., total_out=slot) can write the TOTAL loss of the view batch into ``slot`` itself (and
        return None instead of the per-view losses): the grouped Gram chain is the only loss term and the batch is one
        chain -- the total is then one reduction of the kernels' partial sums instead of a per-view reduction here and a
        second one over the views at the caller"""
        ngroups = self.view_groups if (V >= 4 and self.rotate and self.v_batch == 1) else 1
        return bool(self.gram_grouped and self.layers and not self.w_tv and not self.hist_layers
                    and not self.content_layer and min(ngroups, V) <= 1)

    def loss_and_grad(self, d, rot, g_d, overwrite=False, total_out=None, live=None, dilate=1):
        """d [D,H,W] (output of smooth3d_relu), rot [V,3,3] device tensor, g_d [D,H,W] += dL/dd.
        Returns loss per view [V] (device tensor).

        ``live`` (``ops.live_mask`` written by the forward advect; velocity variable only): g_d is needed only within
        ``dilate`` cells of a live voxel -- everywhere else the caller multiplies it by an exact zero -- and the rotate
        adjoint of the coefficient form leaves it unsummed there (``ops.rotate_bwd_coef``).

        With >= 4 local views (and per-view normalisation, v_batch == 1) the views are split into groups
        whose whole chains run on separate HIP streams: the MFMA-bound conv launches of one group overlap
        the VALU/LDS-bound render and rotate-adjoint kernels and the fill/drain phases of the other."""
        assert self.style_grams is not None or not self.layers, "call set_style_image first"
        V = rot.shape[0] if self.rotate else 1
        ngroups = self.view_groups if (V >= 4 and self.rotate and self.v_batch == 1) else 1
        ngroups = min(ngroups, V)
        if ngroups <= 1:
            return self._chain(d, rot, g_d, overwrite=overwrite and self.writes_gradient(V),
                               total_out=total_out if (total_out is not None and self.sums_total(V)) else None,
                               live=live, dilate=dilate)
        assert not overwrite, "overwrite needs a single view batch (see writes_gradient)"
        assert total_out is None, "total_out needs a single view batch (see sums_total)"
        nst = min(self.vgg_streams, ngroups)
        main = torch.cuda.current_stream(d.device)
        if len(self._streams) < nst:
            self._streams = [torch.cuda.Stream(d.device) for _ in range(nst)]
        loss = torch.empty(V, dtype=torch.float32, device=d.device)
        g_parts = [torch.zeros_like(g_d) for _ in range(nst)]     # one accumulator per stream (plain RMW inside)
        bounds = [V * i // ngroups for i in range(ngroups + 1)]
        for si in range(nst):
            self._streams[si].wait_stream(main)
        for gi in range(ngroups):
            si = gi % nst
            with torch.cuda.stream(self._streams[si]):
                lo, hi = bounds[gi], bounds[gi + 1]
                loss[lo:hi].copy_(self._chain(d, rot[lo:hi].contiguous(), g_parts[si], live=live, dilate=dilate))
        for si in range(nst):
            main.wait_stream(self._streams[si])
        for gp in g_parts:
            ops.axpy(g_d, gp, 1.0)
        return loss


def loss_capture_key(L):
    """what a captured graph of ``L.loss_and_grad`` has baked in by address or by value (style / content / histogram
    targets are device tensors, the loss weights are kernel arguments)"""
    grams = tuple(int(t.data_ptr()) for t in (L.style_grams or {}).values())
    cf = getattr(L, "content_feature", None)
    hyper = tuple(getattr(L, a, None) for a in ("w_style", "tau", "mode", "resize_scale", "rotate", "w_tv",
                                                "v_batch", "w_content", "content_layer", "content_channel",
                                                "w_content_amp"))
    # histogram term: template tensors by address, its weights and layer list by value
    hist = (tuple(sorted((n, int(t.data_ptr())) for n, t in (getattr(L, "hist_targets", None) or {}).items())),
            getattr(L, "w_hist", 0.0), tuple(getattr(L, "hist_layers", ())), tuple(getattr(L, "w_hist_layers", ())),
            getattr(L, "style_mask", False))
    return (grams, tuple(getattr(L, "layers", ())), tuple(getattr(L, "w_layers", ())), hyper,
            None if cf is None else int(cf.data_ptr()), hist, id(getattr(L, "net", None)))


def loss_gradient(loss, d, second, g_d=None, **kw):
    """(losses, dL/dd) of ``loss`` at ``d``, the gradient in a buffer of its own (or in ``g_d``, which is overwritten).
    ``second``: the view matrices of a RenderStyleLoss / the mask ``d_gray`` of an ImageStyleLoss; ``kw``: further
    keywords of ``RenderStyleLoss.loss_and_grad``.  Where the loss can write the gradient without a zero fill
    (``writes_gradient``) it gets the buffer as it is and ``overwrite=True``, otherwise a zeroed one to add into."""
    if isinstance(loss, ImageStyleLoss):                 # (d, d_gray) -> (losses, gradient)
        return loss.loss_and_grad(d, second)
    if hasattr(loss, "writes_gradient") and loss.writes_gradient(1 if second is None else int(second.shape[0])):
        g_d = torch.empty_like(d) if g_d is None else g_d
        return loss.loss_and_grad(d, second, g_d, overwrite=True, **kw), g_d
    g_d = torch.zeros_like(d) if g_d is None else g_d.zero_()
    return loss.loss_and_grad(d, second, g_d, **kw), g_d


class GraphedLoss(object):
    """``loss.loss_and_grad(d, rot, g_d)`` of a few views, replayed as ONE hipGraph where the host cannot keep up with
    it.  A one-view chain is 60-110 small launches: on a box with a slow host the host needs 1.1-1.4 ms to issue what
    the GPU runs in 0.58-0.97 (tools/loss_chain_host.py: the chocolate-scale VGG chain 1.39 -> 0.58 ms, the reference
    smokegun configuration on Inception-v1 1.11 -> 0.97 ms); on a box whose host keeps up, eager submission is the
    faster of the two by ~10 % (graph nodes do not overlap their launch latencies the way back-to-back stream packets
    do).  Hosts differ by 2x between boxes of one pool, so the choice is MEASURED: call 1 runs eagerly (lazy state:
    packed filters, tile tuner, workspaces); calls 2-4 eagerly too, each timed by ``issue_and_wall`` -- if the GPU
    finished as soon as the host did (``HOST_BOUND``; the MEDIAN ratio decides, so that one-off lazy work in one of them
    does not) the chain is host-bound and calls 5.. are replays of a captured graph, otherwise it stays eager (``mode``
    = 'graph' | 'eager'; ``force`` = True / False skips the trial: ``NFS_GRAPH=0/1`` is the reproducible setting, the
    measured choice can differ between hosts and runs).  A change of anything the capture bakes in
    (``loss_capture_key``, shapes) starts over.  Changed inputs are copied into static buffers (``Replay``); the returned
    loss and gradient tensors are valid until the next call."""

    def __init__(self, loss, force=None):
        self.loss = loss
        self.force = force
        self._reset()

    @classmethod
    def from_env(cls, loss):
        """as ``NFS_GRAPH`` has it (``graph_from_env``): forced on, left to the trial, or False -- no replay at all"""
        force = graph_from_env()
        return False if force is False else cls(loss, force=force)

    def _reset(self):
        self._replay = Replay()
        self._key = None
        self._calls = 0
        self.mode = None if self.force is None else ("graph" if self.force else "eager")
        self.trial = None
        self._trials = []

    @property
    def _graph(self):
        return self._replay.graph

    def __call__(self, d, rot):
        key = (loss_capture_key(self.loss), tuple(d.shape), None if rot is None else tuple(rot.shape))
        if self._key is not None and key != self._key:
            self._reset()
        self._key = key
        self._calls += 1
        if self.mode == "eager" or self._calls == 1:
            return loss_gradient(self.loss, d, rot)
        if self.mode is None:
            # three timed eager calls (2, 3, 4), the median ratio decides: one trial can catch one-off lazy work
            out = []
            self._trials.append(issue_and_wall(lambda: out.append(loss_gradient(self.loss, d, rot))))
            if len(self._trials) == 3:
                self.trial = sorted(self._trials, key=lambda tw: tw[0] / tw[1])[1]
                self.mode = "graph" if self.trial[0] > HOST_BOUND * self.trial[1] else "eager"
                if os.environ.get("NFS_VERBOSE"):
                    print("GraphedLoss: %s (issue %.3f ms of %.3f ms wall, median of 3; NFS_GRAPH=0/1 fixes the choice)"
                          % (self.mode, 1e3 * self.trial[0], 1e3 * self.trial[1]))
            return out[0]
        return self._replay(key, (d, rot), lambda d_, rot_: loss_gradient(self.loss, d_, rot_))


class argparse_ns(object):
    """plain attribute bag"""


class TFAdamState(object):
    """tf.compat.v1.train.AdamOptimizer state (m, v, beta powers) living on the device; one
    instance per ``opt_id`` (styler_3p.py:315-323), persisting across frames/views/octaves."""

    def __init__(self, beta1=0.9, beta2=0.999, eps=1e-8):
        self.b1, self.b2, self.eps = np.float32(beta1), np.float32(beta2), np.float32(eps)
        self.b1p, self.b2p = np.float32(1.0), np.float32(1.0)
        self.m = None
        self.v = None
        # OR of every live mask since m and v were zeroed (step_through_advect with a mask): voxels outside it still have
        # m = v = +0.  Usable only while nothing but that kernel has written m or v (their stamp, ``_ever_of``, says)
        self._ever = None
        self._ever_of = None

    def ever_mask(self):
        """the mask above, or None when m or v have been rebound or written by anything else since they were zeroed (a
        write that bypasses their version counters, see ``Stamp``, is not seen: set ``_ever = None`` after one)"""
        if self._ever is None or not holds(self._ever_of, self.m, self.v):
            self._ever = None
        return self._ever

    def advance(self):
        """the beta powers of one more step (float32 variables multiplied once per step in TF), without an update"""
        self.b1p = np.float32(self.b1p * self.b1)
        self.b2p = np.float32(self.b2p * self.b2)

    def _begin_step(self, x, lr):
        """the scalar half of ApplyAdam for a variable of ``x``'s shape: m and v zeroed when missing or of another shape, the
        beta powers advanced.  -> (fresh: m and v are new, (lr_t, beta1, beta2, eps) as the kernels take them)"""
        fresh = self.m is None or self.m.shape != x.shape
        if fresh:
            self.m = torch.zeros_like(x)
            self.v = torch.zeros_like(x)
        self.advance()
        lr_t = np.float32(lr) * np.sqrt(np.float32(1.0) - self.b2p) / (np.float32(1.0) - self.b1p)
        return fresh, (float(lr_t), float(self.b1), float(self.b2), float(self.eps))

    def step(self, x, g, lr):
        _, hyper = self._begin_step(x, lr)
        ops.adam_tf_step(x, self.m, self.v, g, *hyper)

    def step_through_source(self, kind, x, g_vel, lr):
        """the same update for a variable ``x`` the velocity is a function of -- ``kind`` 's': a stream function [D,H,W,3],
        'p': a potential [D,H,W], 'sp': the Helmholtz pair [D,H,W,4] -- given the gradient ``g_vel`` of that velocity
        (``ops.source_velocity``): g_x = ``ops.source_velocity_bwd(kind, g_vel)`` is gathered and consumed inside one kernel"""
        _, hyper = self._begin_step(x, lr)
        ops.source_bwd_adam(kind, g_vel, x, self.m, self.v, *hyper)

    def step_through_emission(self, c, e, g_q, lr):
        """the same update for the colours ``c`` [D,H,W,C] of an emission q = clamp01(c) e (``ops.emission_fwd``) given
        dL/dq: g_c = ``ops.emission_bwd(g_q, c, e)`` is formed and consumed inside one kernel"""
        _, hyper = self._begin_step(c, lr)
        ops.emission_bwd_adam(g_q, c, e, self.m, self.v, *hyper)

    def step_through_advect(self, vel, d0, g_adv, lr, adv_next=None, live_next=None, live_current=False):
        """the same update for the velocity variable of ``advect(d0, vel)`` given dL/d(advected density): the
        velocity gradient is formed and consumed inside one kernel (never written to HBM).  ``adv_next`` [D,H,W]
        (optional) receives advect(d0, updated vel) -- the next iteration's forward sample -- in the same pass, ``live_next``
        its live mask.  ``live_current``: ``live_next`` holds the mask of the CURRENT sample on entry (and ``adv_next`` that
        sample) -- the waves whose voxels never were live are then left out (``ever_mask``)"""
        fresh, hyper = self._begin_step(vel, lr)
        if fresh:                            # (fresh state: m = v = +0 everywhere, the empty mask covers them)
            self._ever = None if live_next is None else torch.zeros_like(live_next)
            self._ever_of = Stamp(self.m, self.v)
        ever = self.ever_mask() if (live_current and live_next is not None and adv_next is not None) else None
        ops.advect_bwd_adam(d0, vel, g_adv, self.m, self.v, *hyper, adv_next=adv_next, live_next=live_next, ever=ever)
        if ever is not None:
            self._ever_of = Stamp(self.m, self.v)                    # (our own write: the mask stays usable)
        else:
            self._ever = None                                        # (a step without the mask update: it no longer covers m, v)

    def step_through_advect_slab(self, vel_slab, d0, g_adv_slab, z0, lr, adv_next=None):
        """``step_through_advect`` on the planes [z0, z0 + nz) only: the moments exist for these planes alone (the Adam
        state of a D-slab-sharded run is sharded with the variable)"""
        _, hyper = self._begin_step(vel_slab, lr)
        ops.advect_bwd_adam_slab(d0, vel_slab, g_adv_slab, self.m, self.v, z0, *hyper, adv_next=adv_next)


class LBFGSState(object):
    """Limited-memory BFGS for the outer loop (north_star names L-BFGS beside Adam; the mounted reference only has Adam):
    one quasi-Newton step per ``step(x, g, lr)`` from the gradient the HIP chain delivers -- two-loop recursion over the
    last ``history`` (s, y) pairs, initial Hessian scale y.s / y.y, a pair kept only when y.s > 1e-10, fixed step
    ``lr`` (the first step min(1, 1/|g|_1) lr), no line search: the arithmetic of ``torch.optim.LBFGS(lr, max_iter=1,
    history_size=history, line_search_fn=None)`` called once per iteration, against which tests/test_optim_cpu.py holds
    it.  Everything stays on the variable's device (elementwise torch kernels and reductions); same call surface as
    ``TFAdamState.step``, so the stylizers take either."""

    def __init__(self, history=10, tolerance_grad=1e-7, tolerance_change=1e-9):
        self.history = int(history)
        # torch.optim.LBFGS's stopping tests, applied per call: nothing moves when max|g| <= tolerance_grad (an empty or
        # fully masked frame has g = 0: the first step's 1/|g|_1 would divide by zero) or when the quasi-Newton direction
        # is not a descent direction (g.d > -tolerance_change)
        self.tol_g, self.tol_c = float(tolerance_grad), float(tolerance_change)
        self.n = 0
        self.S, self.Y, self.ro = [], [], []
        self.d = self.prev_g = None
        self.t = None
        self.H = 1.0

    def step(self, x, g, lr):
        g = g.reshape(-1)
        if self.prev_g is not None and self.prev_g.numel() != g.numel():
            raise ValueError("LBFGSState: the variable changed size (%d -> %d elements): the curvature history belongs to "
                             "ONE variable -- use one state per variable (engine.optimizer_slot)"
                             % (self.prev_g.numel(), g.numel()))
        if float(g.abs().max()) <= self.tol_g if g.numel() else True:
            return
        self.n += 1
        if self.n == 1:
            d = g.neg()
            self.H = 1.0
        else:
            y = g - self.prev_g
            s_ = self.d * self.t
            ys = float(y.dot(s_))                          # (dot products, as torch.optim.LBFGS forms them: a sum of
            # products in another order can land on the other side of the 1e-10 curvature test)
            if ys > 1e-10:
                if len(self.S) == self.history:
                    self.S.pop(0); self.Y.pop(0); self.ro.pop(0)
                self.S.append(s_); self.Y.append(y); self.ro.append(1.0 / ys)
                self.H = ys / float(y.dot(y))
            q = g.neg()
            al = [0.0] * len(self.S)
            for i in range(len(self.S) - 1, -1, -1):
                al[i] = float(self.S[i].dot(q)) * self.ro[i]
                q.add_(self.Y[i], alpha=-al[i])
            d = q.mul(self.H)
            for i in range(len(self.S)):
                be = float(self.Y[i].dot(d)) * self.ro[i]
                d.add_(self.S[i], alpha=al[i] - be)
        self.prev_g = g.clone()
        self.t = min(1.0, 1.0 / float(g.abs().sum())) * float(lr) if self.n == 1 else float(lr)
        self.d = d
        if float(g.dot(d)) > -self.tol_c:
            self.t = 0.0                 # (no move; the pair of the next call is then s = 0: y.s = 0, not kept)
            return
        x.reshape(-1).add_(d, alpha=self.t)


class LapDescentState(object):
    """Laplacian-normalised descent, the update rule of a transport-based stylizer (the reference ships its pieces --
    ``util.lap_normalize``, util.py:95-110, and ``cosine_decay``, 49-53 -- and calls neither):

        g^ = lap_normalize(g, scale_n=lap_n)       over ALL channels of the variable at once; lap_n = 0: g / max(mean|g|, 1e-7)
        x  <- fma(-lr, g^, x)                       one fused multiply-add per element (``ops.descent_step``)

    Every pyramid level enters with RMS 1, so ``lr`` is a length in the variable's own units, whatever the loss weights
    are: for a velocity, lr = c * 2/(n-1) moves a voxel by about c cells per level and step, at every octave alike; a stream
    function or potential is differenced per cell, so the same lr is a displacement.  A zero gradient gives a zero update
    (0 / max(0, eps) = 0).  There is no state besides ``lap_n`` (no moments): ``optimizer_slot`` keys it as it keys Adam.
    The reference's k5x5x5 / k5x5 tables exist for some channel counts only; they are one kernel times an identity, and the
    per-channel kernels behind ``util.lap_normalize`` take any C (C = 4 and the 2-D counts run the generic gather forms).
    ``nd`` (3 or 2): the grid's dimension, which a [H,W,2] velocity and a [D,H,W] potential do not tell apart; the
    stylizers set it.  Same call surface as ``TFAdamState.step``."""

    def __init__(self, lap_n=3, nd=None):
        if int(lap_n) < 0:
            raise ValueError("lap_n=%r: the number of pyramid levels is 0 (mean-|g| normalisation) or more" % (lap_n,))
        self.lap_n = int(lap_n)
        self.nd = nd

    def advance(self):
        """(nothing to advance: the call an idle rank makes on ``TFAdamState``)"""

    def _nd(self, x, nd):
        nd = nd or self.nd or {4: 3, 2: 2}.get(x.dim())
        if nd not in (2, 3):
            raise ValueError("LapDescentState: a %d-d variable does not say whether its grid is 2-D or 3-D: pass nd" % x.dim())
        return nd

    def normalized(self, g, nd=None):
        """g^ of a gradient shaped like the variable -> [grid..., C]"""
        from . import util
        nd = self._nd(g, nd)
        grid = tuple(g.shape[:nd])
        c = g.numel() // max(int(np.prod(grid)), 1)
        return util.lap_normalize(g.reshape(grid + (c,)), scale_n=self.lap_n, is_3d=nd == 3, c=c)

    def step(self, x, g, lr, nd=None):
        ops.descent_step(x, self.normalized(g.reshape(x.shape), nd), lr)

    def step_through_advect(self, vel, d0, g, lr, adv_next, live_next=None):
        """the same update of the velocity variable [D,H,W,3] of ``advect(d0, vel)``, and in the same pass ``adv_next`` =
        advect(d0, updated vel) -- the next iteration's forward sample -- and ``live_next`` (optional) its live mask"""
        ops.advect_descent(d0, vel, self.normalized(g, 3), lr, adv_next, live_next)

    def step_through_advect2d(self, vel, d0, g, lr, adv_next):
        """the 2-D twin: vel [H,W,2], d0 [H,W]"""
        ops.advect2d_descent(d0, vel, self.normalized(g, 2), lr, adv_next)


def optimizer_slot(kind, t, frames_per_opt):
    """key of the optimiser state frame ``t`` steps with.  Adam: ``t // frames_per_opt`` -- one (m, v, step count) shared
    by the frames of a group, updated by them in turn (styler_3p.py:315-323; the moments are running averages and
    tolerate it).  L-BFGS: one state PER FRAME -- its (s, y) pairs are differences of consecutive gradients of one
    variable; pairs mixed across frames (or across particle counts) are not curvature of anything.  'lapnorm' has no
    per-variable state and is keyed as Adam is."""
    return ("lbfgs", int(t)) if kind == "lbfgs" else int(t) // int(frames_per_opt)


def make_optimizer(kind="adam", lap_n=3):
    """one optimiser state per ``opt_id`` (styler_3p.py:315-323): TF ApplyAdam (the reference), L-BFGS or Laplacian-
    normalised descent with ``lap_n`` pyramid levels (config.optimizer, config.lap_n)"""
    if kind in (None, "", "adam"):
        return TFAdamState()
    if kind == "lbfgs":
        return LBFGSState()
    if kind == "lapnorm":
        return LapDescentState(lap_n=lap_n)
    raise ValueError("optimizer %r: 'adam', 'lbfgs' or 'lapnorm'" % (kind,))


SOURCED = ("s", "p", "sp")      # the grid variables a velocity is a function of (ops.source_velocity)


class GridStylizer(object):
    """TNST-style grid path assembled from the reference's operators:
        d^ = advect(d0, vel)  ->  smooth+max  ->  RenderStyleLoss
    with the velocity field ``vel`` [D,H,W,3] (target 'v'), a stream function ``psi`` [D,H,W,3] whose stream velocity
    (``ops.stream_velocity``: the channel-reversed curl, divergence-free by construction) is that field (target 's'), or
    the density itself (target 'd') as the Adam variable.  Views shard over ranks (``views=sum``): each rank evaluates its slice
    of the rotation matrices; the exchange is ONE all-reduce's worth of link traffic per iteration,
    split around the field work so that this work is sharded too (``slab`` mode, the default for the
    velocity variable): reduce-scatter of the density-field gradient over D-slabs -> slab-local smooth
    adjoint, advect adjoint + ApplyAdam, advect, smooth -> all-gather of the smoothed density (see
    ``_slab_setup``).  Otherwise the gradient is all-reduced and every rank applies the identical step.
    ``bind`` swaps the frame (density, variable, Adam state) under the same
    stylizer: the frame loop of a sequence (styler_grid.py) re-uses one instance.
    ``adv_order`` (config.py adv_order; velocity variable): 1 = semi-Lagrangian advect, 2 = MacCormack with the extrema
    limiter, forward and adjoint (``ops.advect_maccormack`` / ``advect_maccormack_bwd``).  Order 2 takes the unfused
    update (adjoint, then the optimiser's step) and, over ranks, the all-reduce mode: every rank repeats the field work
    on the summed density gradient and, the adjoint being bit-reproducible, arrives at the identical variable.  With
    ``target='d'`` there is no advect: ``adv_order`` is accepted and has no effect.
    ``target='s'``: order 1 advects along the stream velocity without storing it (``ops.advect_stream_fwd`` / ``_bwd``) and
    the Adam step gathers curl^T inside the update (``TFAdamState.step_through_source``); the next forward sample and its
    live mask are written by a launch of their own at the end of ``step()`` and are then handled exactly as the velocity
    variable's (dead-region skipping, hipGraph replay starting from the stored sample).  Order 2 materialises the
    velocity.  Over ranks: the all-reduce mode.
    ``target='p'``: a potential ``phi`` [D,H,W] whose forward differences are the velocity (``ops.potential_velocity``:
    irrotational by construction -- local sources and sinks); ``target='sp'``: the Helmholtz pair ``a`` [D,H,W,4] =
    (psi, phi) with v = stream_velocity(psi) + potential_velocity(phi) (``ops.helmholtz_velocity``).  Both run exactly as
    's' does, through ``ops.advect_source_fwd`` / ``_bwd`` and ``ops.source_bwd_adam`` of their kind.
    ``optimizer='lapnorm'`` (``lap_n`` pyramid levels): Laplacian-normalised descent (``LapDescentState``) for all five
    targets and both orders.  ``lr`` is then a length in the variable's units (every pyramid level enters with RMS 1): for
    'v', lr = c * 2/(n-1) moves a voxel by about c cells per level and step; a stream function or potential is differenced
    per cell, so the same lr is a displacement.  The loss chain, its hipGraph replay and the dead-region skipping of the
    rotate adjoint ('v') are as with Adam; the update is outside the capture.  'v' at order 1 takes the fused kernel
    (``ops.advect_descent``: update + next forward sample + its live mask, handled like ``advect_bwd_adam``'s
    ``adv_next`` / ``live_next``; ``NFS_FUSE_ADVECT=0`` turns it off), every other case ``variable_gradient`` ->
    ``LapDescentState.step`` and, where a fixed forward buffer is in use, ``_advect_now()``.  Never-live skipping is
    Adam's and does not apply.  Over ranks: the all-reduce mode only (the normalisation is non-local and non-linear: it
    must see the summed gradient), every rank computing the identical update; the D-slab mode is not entered."""

    def __init__(self, loss, d0, k=3, target="v", lr=0.1, process_group=None, graph=None, optimizer="adam", adv_order=1,
                 lap_n=3):
        assert target in ("v", "d") + SOURCED, \
            "target is 'v' (velocity), 's' (stream function), 'p' (potential), 'sp' (both) or 'd' (density)"
        self.loss = loss
        self.d0 = d0.contiguous()
        self.k = float(k)
        self.target = target
        self.lr = float(lr)
        self.pg = process_group
        self.adam = make_optimizer(optimizer, lap_n=lap_n)   # (named after the reference's optimiser; L-BFGS / 'lapnorm' on request)
        if isinstance(self.adam, LapDescentState):
            self.adam.nd = 3
        # the advect adjoint consumed inside the Adam kernel: only when the optimiser IS Adam
        self.fuse_adam = os.environ.get("NFS_FUSE_ADAM", "1") != "0" and isinstance(self.adam, TFAdamState)
        assert int(adv_order) in (1, 2), "adv_order is 1 (semi-Lagrangian) or 2 (MacCormack)"
        self.adv_order = int(adv_order)
        if self.adv_order == 2 and target == "v":
            # the fused kernels (adjoint + Adam + next forward, slab forms, live mask) are those of the order-1 stencil
            self.fuse_adam = False
        # order 2: the first-order sample and the limiter's decisions of the CURRENT forward, which the adjoint reads (fixed
        # buffers: a captured forward writes them at every replay, the adjoint outside the capture reads what it wrote)
        self._mc_fwd = None
        self._mc_keep = None
        self._mc_vel = None                          # (targets 's', 'p', 'sp': the velocity that forward was advected along)
        # hipGraph replay of the forward + adjoint (about 130 launches a step; the host needs 1.25 ms to issue
        # them one by one, which is the whole step at one view per rank)
        # (measured: 200^3 x 8 views 3.98 -> 3.90 ms, 200^3 x 1 view 1.35 -> 1.41 ms, 100^3 x 1 view 1.20 -> 1.06 ms:
        # it pays where the step is shorter than the 1.15 ms the host needs to issue it).  None = decide at the first
        # step from the problem size; NFS_GRAPH=0/1 or the constructor argument override.
        self.use_graph = graph_from_env() if graph is None else bool(graph)
        self.graph_trial = None                      # (t_issue, t_wall) of the measured choice, once it has been made
        self._steps_seen = 0
        self._replay = None                          # (None: before the eager call that precedes a capture)
        self.d_s = self.d_adv = None                 # the smoothed / advected density of the current forward
        self._for_variable = target != "d"           # (step(), gradient(): see field_gradient)
        self._pending = None
        self._owns_buffers = False
        # advect(d0, var) of the NEXT iteration written by the Adam kernel of this one (ops.advect_bwd_adam(adv_next=...)):
        # the buffer, and the stamp of what it was computed from (any in-place torch op on the variable or the density, a
        # bind() or a re-assignment makes it stale and the forward advect runs by itself)
        self.fuse_advect = os.environ.get("NFS_FUSE_ADVECT", "1") != "0"
        self._adv_buf = None
        self._adv_src = None
        # Dead-region skipping (velocity variable): the kernels that write the forward advect also write the mask of the
        # voxels whose back-traced density corners differ; everywhere else the advect adjoint multiplies the incoming
        # gradient by an exact zero, so step() / gradient() let the rotate adjoint skip what only feeds those voxels.
        # The update is bit-identical with it on and off (tests/test_dead_skip_gpu.py); NFS_DEAD_SKIP=0 turns it off.
        self.dead_skip = os.environ.get("NFS_DEAD_SKIP", "1") != "0"
        self._live_buf = None
        self._live_shape = None
        self._live_mark = None                       # the stamp (``_adv_src`` itself) of the advect that wrote the mask
        D, H, W = d0.shape
        if target == "v":
            self.var = torch.zeros(D, H, W, 3, dtype=torch.float32, device=d0.device)
        elif target in SOURCED:
            self.var = torch.zeros(ops.source_shape(target, D, H, W), dtype=torch.float32, device=d0.device)
        else:
            self.var = d0.clone()
        # field gradient and the summed loss share one buffer: the multi-rank exchange is ONE all-reduce
        # (the loss rides in the slot behind the gradient)
        n = D * H * W
        self.slab = None
        if self.pg is not None and os.environ.get("NFS_SLAB_SHARD", "1") != "0":
            self._slab_setup()
        if self.slab is None:
            self._gbuf = torch.zeros(n + 4, dtype=torch.float32, device=d0.device)
            self.g_ds = self._gbuf[:n].view(D, H, W)
            self._loss_slot = self._gbuf[n:n + 1]

    # ---- D-slab sharding of the replicated field work (view-sharded runs) ---------------------------------------------------
    def _slab_setup(self):
        """Strong scaling of the 8-view problem is capped by what every rank repeats: advect, smooth, their adjoints and
        ApplyAdam on the whole field (~0.2 ms of a 1.1 ms one-view step).  All of it is LOCAL in z up to a one-plane
        stencil, so the all-reduce of the density gradient is taken apart into its two halves with that work in between:

            reduce-scatter(g_ds)      rank k receives the summed gradient of ITS slab of planes, with a two-plane halo
                                      (the chunks of the send buffer overlap: no separate halo exchange)
            smooth adjoint            on slab +- 2 planes -> valid on slab +- 1
            advect adjoint + Adam     on slab +- 1: the variable, its moments and the update exist per slab (+ one plane
                                      each side, computed identically by both neighbours -- deterministic kernels)
            advect, smooth            next iteration's field on slab +- 1 -> valid smoothed density on the slab
            all-gather(d_s)           every rank holds the whole smoothed density for its views' rotate + render

        Same bytes over the links as the all-reduce it replaces (+ 4 halo planes per chunk); d0 stays replicated and
        constant (the back-traced points leave the slab).  The loss rides in an extra plane of every chunk.  Off when
        the variable is the density itself, when a slab would be thinner than two planes, or with NFS_SLAB_SHARD=0."""
        rank, world = parallel.rank_world(self.pg)
        D, H, W = self.d0.shape
        force = os.environ.get("NFS_SLAB_SHARD") == "2"           # also on a one-rank group (RCCL smoke test on one GPU)
        if (world <= 1 and not force) or self.target != "v" or not self.fuse_adam or D // world < 2 or (H * W) % 4 \
                or min(D, H, W) < 2:
            return
        dev = self.d0.device
        cs, plan = parallel.slab_plan(D, world)
        z0, z1 = plan[rank]
        sl = argparse_ns()
        sl.rank, sl.world, sl.cs, sl.z0, sl.z1 = rank, world, cs, z0, z1
        sl.lo, sl.hi = max(z0 - 1, 0), min(z1 + 1, D)                     # planes whose variable this rank maintains
        # padded gradient volume: planes [2, D + 2) = g_ds, two zero planes either side, one more for the loss
        self._gpad = torch.zeros(D + 5, H, W, dtype=torch.float32, device=dev)
        self.g_ds = self._gpad[2:D + 2]
        self._loss_slot = self._gpad[D + 4].view(-1)[:1]
        sl.idx = torch.tensor(parallel.slab_pack_index(D, world), dtype=torch.int64, device=dev)    # (NFS_SLAB_PACK=torch)
        sl.pack = torch.empty(world, cs + 5, H, W, dtype=torch.float32, device=dev)
        sl.recv = torch.empty(cs + 5, H, W, dtype=torch.float32, device=dev)
        # padded smoothed density: planes [2, 2 + world * cs) are gathered, d_s = planes [2, 2 + D)
        sl.ds_full = torch.zeros(world * cs + 4, H, W, dtype=torch.float32, device=dev)
        sl.stage = torch.zeros(cs, H, W, dtype=torch.float32, device=dev)
        self.slab = sl

    def gather_variable(self):
        """slab mode: every rank keeps only its planes of the variable current -- all-gather them into ``self.var``
        (results, checkpoints); a no-op otherwise"""
        sl = self.slab
        if sl is None:
            return self.var
        D, H, W = self.d0.shape
        mine = torch.zeros(sl.cs, H, W, 3, dtype=torch.float32, device=self.var.device)
        if sl.z1 > sl.z0:
            mine[:sl.z1 - sl.z0] = self.var[sl.z0:sl.z1]
        full = torch.empty(sl.world, sl.cs, H, W, 3, dtype=torch.float32, device=self.var.device)
        parallel.all_gather_into(full, mine, group=self.pg)
        self.var.copy_(full.view(sl.world * sl.cs, H, W, 3)[:D])
        return self.var

    def _forward_field_slab(self):
        sl = self.slab
        assert self._pending is None, "bind() is not available with the D-slab sharding (one frame per stylizer)"
        D, H, W = self.d0.shape
        if sl.z1 > sl.z0:
            self.d_adv = self._advect_now()
            d_s_ext = ops.smooth3d_relu_fwd(self.d_adv, self.k)        # exact on the slab (cut planes are one further out)
            own = d_s_ext[sl.z0 - sl.lo: sl.z0 - sl.lo + (sl.z1 - sl.z0)]
            if sl.z1 - sl.z0 == sl.cs:
                src = own
            else:
                sl.stage[:sl.z1 - sl.z0].copy_(own)
                src = sl.stage
        else:
            src = sl.stage                                             # an idle rank contributes zero planes
        parallel.all_gather_into(sl.ds_full[2:2 + sl.world * sl.cs].view(sl.world, sl.cs, H, W), src, group=self.pg)
        self.d_s = sl.ds_full[2:2 + D]
        return self.d_s

    def _step_slab(self, rot_local):
        """one iteration with the field work sharded over D-slabs (see ``_slab_setup``)"""
        sl = self.slab
        D, H, W = self.d0.shape
        if self.use_graph:
            self._forward_field_slab()                                  # (holds a collective: outside the graph)
            self._field_gradient_graphed(rot_local, with_field=False)
        else:
            losses, _ = self.field_gradient(rot_local)
            torch.sum(losses, dim=0, keepdim=True, out=self._loss_slot)
        if os.environ.get("NFS_SLAB_PACK") == "torch":                  # (the gather by index table the copy kernel replaced)
            torch.index_select(self._gpad, 0, sl.idx, out=sl.pack.view(-1, H, W))
        else:
            ops.slab_pack(self._gpad, sl.pack, D, sl.world, sl.cs)
        parallel.reduce_scatter_sum(sl.recv, sl.pack, group=self.pg)
        total = sl.recv[sl.cs + 4].view(-1)[0].clone()
        if sl.z1 > sl.z0:
            # chunk planes = global [z0 - 2, z0 + cs + 2); the same planes of the padded smoothed density
            g_adv = ops.smooth3d_relu_bwd(sl.ds_full[sl.z0:sl.z0 + sl.cs + 4], sl.recv[:sl.cs + 4], self.k)
            off = sl.lo - (sl.z0 - 2)
            adv = self._adv_target()
            self.adam.step_through_advect_slab(self.var[sl.lo:sl.hi], self.d0, g_adv[off:off + (sl.hi - sl.lo)], sl.lo,
                                               self.lr, adv_next=adv)
            if adv is not None:
                self._adv_mark()
        else:
            self.adam.advance()                                         # (an idle rank keeps the step count)
        return total

    def bind(self, d0, var=None, adam=None):
        """Re-point the stylizer at another frame of the same shape (takes effect at the next step / gradient).
        Without hipGraph replay this is a pointer swap; a captured graph has the addresses of ``d0`` and ``var`` baked
        in, so there the stylizer keeps private buffers and the frame's data is copied into them."""
        assert tuple(d0.shape) == tuple(self.d0.shape)
        self._pending = (d0, var)
        if adam is not None:
            self.adam = adam
            self.fuse_adam = self.fuse_adam and isinstance(adam, TFAdamState)
            if isinstance(adam, LapDescentState):
                adam.nd = 3

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
                self.var = var

    # ---- the forward advect of iteration i + 1 rides in the Adam kernel of iteration i ---------------------------------------
    def _adv_target(self):
        """the buffer the fused Adam kernel ('v') or the launch after the update ('s', 'p', 'sp') writes the next forward sample into
        (None: fusion off / not applicable)"""
        if not (self.fuse_advect and (self._fused_step_ok() or self._source_stored() or self._fused_descent_ok())):
            return None
        sl = self.slab
        shape = tuple(self.d0.shape) if sl is None else (sl.hi - sl.lo,) + tuple(self.d0.shape[1:])
        if self._adv_buf is None or tuple(self._adv_buf.shape) != shape:
            self._adv_buf = torch.empty(shape, dtype=torch.float32, device=self.d0.device)
            self._adv_src = None
        return self._adv_buf

    def _fused_step_ok(self):
        """may step() consume the advect adjoint inside the Adam kernel (``nfs_advect_bwd_adam*``: volumes of at least two
        cells a side whose cell count is a multiple of 4)?  The stored forward advect exists only then: any other shape
        updates the variable through ``TFAdamState.step``, which writes no next forward sample."""
        D, H, W = self.d0.shape
        return self.target == "v" and self.fuse_adam and min(D, H, W) >= 2 and (D * H * W) % 4 == 0

    def _fused_descent_ok(self):
        """optimizer 'lapnorm', velocity variable, order 1: may step() take ``LapDescentState.step_through_advect``, whose
        kernel writes the next forward sample and its live mask?  On the shapes ``_fused_step_ok`` names, so that the stored
        sample and the mask are handled exactly as the fused Adam step's"""
        D, H, W = self.d0.shape
        return (self.target == "v" and self.adv_order == 1 and isinstance(self.adam, LapDescentState)
                and min(D, H, W) >= 2 and (D * H * W) % 4 == 0)

    def _source_stored(self):
        """stream-function, potential or Helmholtz variable, order 1, on the shapes the fused advect takes: the forward sample
        lives in the fixed buffer as the velocity variable's does (written by ``_advect_now``, which ``step()`` calls after
        the update)"""
        return self.target in SOURCED and self.adv_order == 1 and ops.advect_source_takes(*self.d0.shape)

    def velocity(self):
        """the velocity the density is advected along: the variable itself ('v'), its stream velocity ('s'), its potential
        velocity ('p') or the sum of both parts ('sp')"""
        assert self.target == "v" or self.target in SOURCED, "the density variable has no velocity"
        return self.var if self.target == "v" else ops.source_velocity(self.target, self.var)

    def _adv_mark(self, live=False):
        self._adv_src = Stamp(self.var, self.d0)
        self._live_mark = self._adv_src if live else None

    def _live_target(self):
        """the mask buffer the advect kernels fill beside the stored forward advect (None: skipping off / not applicable:
        whole-volume velocity runs whose loss takes a mask; slab-sharded ranks hold only their planes' velocity)"""
        if not (self.dead_skip and self.slab is None and getattr(self.loss, "accepts_live", False)
                and self._adv_target() is not None):
            return None
        if self._live_buf is None or self._live_shape != tuple(self.d0.shape):
            self._live_buf = ops.live_mask(*self.d0.shape, like=self.d0)
            self._live_shape = tuple(self.d0.shape)
            self._live_mark = None
        return self._live_buf

    def _live_valid(self):
        """the mask belongs to exactly the advect that wrote it, and that advect is still current"""
        return (self._live_buf is not None and self._live_mark is not None and self._live_mark is self._adv_src
                and self._adv_valid())

    def _live_kw(self):
        """keyword arguments for loss_and_grad when the mask of the CURRENT forward advect exists"""
        if self._live_target() is None or not self._live_valid():
            return {}
        return {"live": self._live_buf, "dilate": 1 if self.k > 0 else 0}

    def invalidate_forward(self):
        """forget the stored forward advect.  In-place torch ops on ``var`` / ``d0``, ``bind()`` and re-assignment are
        noticed by themselves; a write that bypasses the version counter (see ``Stamp``) is not: call this after one."""
        self._adv_src = None

    def _adv_valid(self):
        return self._adv_buf is not None and holds(self._adv_src, self.var, self.d0)

    def _advect_now(self):
        """d_adv = advect(d0, var) -- from the previous step's Adam kernel when it is still current, else computed here
        (into the same buffer: a captured graph reads it by address)"""
        if self.adv_order == 2:
            return self._advect_now_order2()
        sl = self.slab
        buf = self._adv_target()
        live = self._live_target()
        if buf is not None and self._adv_valid() and (live is None or self._live_valid()):
            return buf
        if self.target in SOURCED:
            out = ops.advect_source_fwd(self.target, self.d0.unsqueeze(-1), self.var,
                                        out=None if buf is None else buf.unsqueeze(-1), live=live).squeeze(-1)
        elif sl is None:
            out = ops.advect_fwd(self.d0.unsqueeze(-1), self.var, out=None if buf is None else buf.unsqueeze(-1),
                                 live=live).squeeze(-1)
        else:
            out = ops.advect_fwd_slab(self.d0, self.var[sl.lo:sl.hi], sl.lo, out=buf)
        if buf is not None:
            self._adv_mark(live=live is not None)
        return out

    def _advect_now_order2(self):
        """d_adv = MacCormack(d0, var); d_fwd and the keep mask stay on the stylizer for ``variable_gradient``"""
        d4 = self.d0.unsqueeze(-1)
        if self._mc_fwd is None or self._mc_fwd.shape != d4.shape:
            self._mc_fwd = torch.empty_like(d4)
            self._mc_keep = ops.maccormack_mask(d4.shape, d4)
        vel = self.var
        if self.target in SOURCED:
            if self._mc_vel is None or self._mc_vel.shape[:3] != self.var.shape[:3]:
                self._mc_vel = torch.empty(tuple(self.d0.shape) + (3,), dtype=torch.float32, device=self.d0.device)
            vel = self._mc_vel.copy_(ops.source_velocity(self.target, self.var))
        return ops.advect_maccormack(d4, vel, keep=self._mc_keep, d_fwd=self._mc_fwd).squeeze(-1)

    def forward_field(self):
        if self.slab is not None:
            return self._forward_field_slab()
        self._apply_binding()
        self.d_adv = self._advect_now() if self._for_variable else self.var
        self.d_s = ops.smooth3d_relu_fwd(self.d_adv, self.k)
        return self.d_s

    def field_gradient(self, rot_local, total=False, for_variable=False):
        """forward + adjoint down to the smoothed density: (loss_per_view, dL/d d_s of the LOCAL views); ``total``: see
        _loss_gradient.  ``for_variable``: the caller only takes the gradient on to the variable (step(), gradient()) --
        with a velocity variable dL/d d_s is then left unsummed where the advect adjoint multiplies it by zero"""
        d_s = self.forward_field()
        return self._loss_gradient(d_s, rot_local, total=total, live_kw=self._live_kw() if for_variable else None)

    def _loss_gradient(self, d_s, rot_local, total=False, live_kw=None):
        """total: let the loss write the summed loss of the local views into the loss slot where it can (then None is
        returned instead of the per-view losses)"""
        kw = dict(live_kw or ())
        if total and hasattr(self.loss, "sums_total") and self.loss.sums_total(rot_local.shape[0]):
            kw["total_out"] = self._loss_slot
        return loss_gradient(self.loss, d_s, rot_local, g_d=self.g_ds, **kw)

    def variable_gradient(self, g_ds):
        """adjoint of smooth+max and advect: dL/d variable from dL/d d_s (deterministic kernels: every
        rank computes the identical result from the all-reduced g_ds)"""
        g_adv = ops.smooth3d_relu_bwd(self.d_s, g_ds, self.k)
        if self.target in SOURCED:
            return ops.source_velocity_bwd(self.target, self._source_velocity_gradient(g_adv))
        if self.target == "v" and self.adv_order == 2:
            _, g_var = ops.advect_maccormack_bwd(self.d0.unsqueeze(-1), self.var, self._mc_fwd, self._mc_keep,
                                                 g_adv.unsqueeze(-1), need_d=False, need_vel=True)
            return g_var
        if self.target == "v":
            _, g_var = ops.advect_bwd(self.d0.unsqueeze(-1), self.var, g_adv.unsqueeze(-1), need_d=False,
                                      need_vel=True)
            return g_var
        return g_adv

    def _source_velocity_gradient(self, g_adv):
        """targets 's', 'p', 'sp': dL/d(velocity) from dL/d(advected density), along the forward's own velocity"""
        d4 = self.d0.unsqueeze(-1)
        if self.adv_order == 2:
            return ops.advect_maccormack_bwd(d4, self._mc_vel, self._mc_fwd, self._mc_keep, g_adv.unsqueeze(-1),
                                             need_d=False, need_vel=True)[1]
        return ops.advect_source_bwd(self.target, d4, self.var, g_adv.unsqueeze(-1))

    def gradient(self, rot_local):
        """one forward+backward over the local views; returns (loss_per_view, grad wrt variable)"""
        losses, g_ds = self.field_gradient(rot_local, for_variable=self._for_variable)
        return losses, self.variable_gradient(g_ds)

    def _capture_key(self, rot_local):
        """everything a captured graph has baked in by address or by value: a mismatch forces a re-capture
        (set_style_image / set_content_image / set_hist_image allocate new targets; loss weights are kernel
        arguments)"""
        return loss_capture_key(self.loss) + (int(self.d0.data_ptr()), int(self.var.data_ptr()),
                                              tuple(rot_local.shape), self.k, self.target)

    def _field_gradient_graphed(self, rot_local, with_field=True):
        """field_gradient as one hipGraph: the first call runs eagerly (lazy state: packed Winograd filters, side
        streams, workspaces), the second is captured, later ones replay (``with_field=False``: the graph without the
        field ops -- slab mode, their all-gather stays outside the capture).  The capture is keyed on what it bakes in
        (style / content targets, loss hyper-parameters, the addresses of d0 and the variable, the number of views):
        when any of that changes the graph is dropped and, after one more eager call, captured again.  The view matrices
        are copied into a static buffer where they changed (``Replay``)."""
        def body(r):
            losses, _ = (self.field_gradient(r, total=True, for_variable=self._for_variable) if with_field
                         else self._loss_gradient(self.d_s, r, total=True))
            if losses is not None:        # (None: the loss chain has written the total into the slot itself)
                torch.sum(losses, dim=0, keepdim=True, out=self._loss_slot)     # one kernel: reduce straight into the slot
        if with_field and self._for_variable and self._adv_target() is not None:
            # the captured forward starts from the advected density in its fixed buffer: bring it up to date eagerly when
            # the previous step's Adam kernel has not left it there (first step, a re-bound frame, a variable set by hand)
            self._apply_binding()
            self._advect_now()
        key = self._capture_key(rot_local) + (with_field, self._adv_target() is not None,
                                              with_field and bool(self._live_kw()))
        if self._replay is None or self._replay.stale(key):
            self._replay = Replay()       # (one eager call before the first capture and after every dropped graph)
            body(rot_local)
        else:
            self._replay(key, (rot_local,), body)
        return self._loss_slot, self.g_ds

    @property
    def _graph(self):
        return None if self._replay is None else self._replay.graph

    def step(self, rot_local, loss_view=False):
        """one iteration: loss + gradient of the local views, the exchange, the update; returns the summed loss (a 0-d
        device tensor of its own).  ``loss_view=True`` (single rank): return a VIEW of the loss slot instead -- no copy
        launch behind the step (5 us + a 9-us gap of the 1-ms one-view step) -- valid only until the next step()
        overwrites it: read it (``float()``) or clone it before stepping again"""
        if self.use_graph is None:
            nv = max(int(rot_local.shape[0]), 1)
            if self.d0.numel() * nv <= (2 << 20):    # small volumes, few views: the host needs longer than the GPU
                self.use_graph = True
            else:
                # Large volumes: ~80 launches per step.  At 8 views the GPU needs 2.7 ms for them and a fast host 2.0 ms to
                # issue them (tools/step_host_time.py: 35 us per C-ABI call, i.e. the HIP launches themselves) -- kernel-
                # bound, but a host of the same pool that is 2x slower (measured: 20 us per launch instead of 9) turns
                # the very same step host-bound, at 8 views as at 1.  So the choice is measured at the second step (the
                # first has built the lazy state); until then the step runs eagerly.
                # (by one extra evaluation of the loss chain: host-bound is where a hipGraph replay would be faster)
                self._steps_seen += 1
                if self._steps_seen == 2 and self.d_s is not None:
                    t_issue, t_wall = self.graph_trial = issue_and_wall(lambda: self._loss_gradient(self.d_s, rot_local))
                    self.use_graph = t_issue > HOST_BOUND * t_wall
        if self.slab is not None:
            return self._step_slab(rot_local)
        self._apply_binding()
        total = None                      # (None: the total of the local views is in the loss slot)
        if self.use_graph:
            _, g_ds = self._field_gradient_graphed(rot_local)
        else:
            losses, g_ds = self.field_gradient(rot_local, total=True, for_variable=self._for_variable)
            if losses is not None and self.pg is None:
                total = losses.sum()                                         # (one kernel, a fresh tensor: no slot, no copy)
            elif losses is not None:
                torch.sum(losses, dim=0, keepdim=True, out=self._loss_slot)  # (one kernel: reduce straight into the slot)
        if self.pg is not None:
            # The one exchange step (RCCL over xGMI): ONE all-reduce of gradient + loss.  The reduction is placed on
            # the 4*G^3-byte density gradient, not on the 12*G^3-byte velocity gradient: everything below it is
            # linear and replicated, so reducing early moves 3x fewer bytes over the links.
            parallel.all_reduce_sum_([self._gbuf], group=self.pg)
        if total is None:
            total = self._loss_slot[0] if (loss_view and self.pg is None) else self._loss_slot[0].clone()
        if isinstance(self.adam, LapDescentState):
            # Laplacian-normalised descent: the normalisation is non-local, so the gradient of the variable is formed
            # first (from the all-reduced g_ds: every rank computes the identical update); the velocity variable at order
            # 1 then takes the fused kernel, which leaves the next forward sample and its mask as the fused Adam step does
            g = self.variable_gradient(g_ds)
            adv = self._adv_target() if self._fused_descent_ok() else None
            if adv is not None:
                live = self._live_target()
                self.adam.step_through_advect(self.var, self.d0, g, self.lr, adv_next=adv, live_next=live)
                self._adv_mark(live=live is not None)
            else:
                self.adam.step(self.var, g, self.lr, nd=3)
                if self._adv_target() is not None:
                    self._advect_now()    # (a sourced variable's next forward sample and its mask, into the fixed buffers)
                else:
                    self._adv_src = None
        elif self._fused_step_ok():
            g_adv = ops.smooth3d_relu_bwd(self.d_s, g_ds, self.k)
            adv = self._adv_target()
            live = self._live_target()
            # (the mask buffer holds the CURRENT sample's mask when the adjoint above could use it: the Adam kernel may
            # then leave out the voxels that never were live)
            self.adam.step_through_advect(self.var, self.d0.unsqueeze(-1), g_adv.unsqueeze(-1), self.lr, adv_next=adv,
                                          live_next=live, live_current=live is not None and self._live_valid())
            if adv is not None:
                self._adv_mark(live=live is not None)
        elif self.target in SOURCED and self.fuse_adam:
            g_adv = ops.smooth3d_relu_bwd(self.d_s, g_ds, self.k)
            self.adam.step_through_source(self.target, self.var, self._source_velocity_gradient(g_adv), self.lr)
            if self._adv_target() is not None:
                self._advect_now()        # (the next forward sample and its mask, into the fixed buffers)
        else:
            self.adam.step(self.var, self.variable_gradient(g_ds), self.lr)
            self._adv_src = None          # (the variable moved and nothing wrote advect(d0, var) for it)
        return total


# --------------------------------------------------------------------------------------
# 2-D colour path (styler_2p.py:91-102 + styler_base.py:152-185, 211-213)
# --------------------------------------------------------------------------------------

class ImageStyleLoss(object):
    """Style (+TV) loss of a colour image d [B,H,W,3] in [0,1] (the 2-D colour stylizer):
    d*255 -> VGG -> Gram; with ``style_mask`` the features are multiplied by the bicubic-resized
    density mask and the Gram denominator becomes 2*area*C (styler_base.py:165-169)."""

    def __init__(self, net, style_layer, w_style_layer, w_style=1.0, w_tv=0.0, resize_scale=1.0,
                 style_mask=False, style_mask_on_ref=False, w_content=0.0, content_layer=None, content_channel=0,
                 w_content_amp=100.0, w_hist=0.0, hist_layer=(), w_hist_layer=()):
        assert not style_mask_on_ref, "style_mask_on_ref is not used by any reference driver"
        self.net = net
        self.layers = list(style_layer) if float(w_style) else []        # (styler_base.py:152: no style term at w_style 0)
        self.w_layers = [float(w) for w in w_style_layer][:len(self.layers)] if self.layers else []
        self.w_style, self.w_tv = float(w_style), float(w_tv)
        self.resize_scale = float(resize_scale)
        self.style_mask = bool(style_mask)
        order = [s[0] for s in net.seq]
        self.w_content = float(w_content) if content_layer else 0.0
        self.content_layer = content_layer if self.w_content else None
        self.content_channel = int(content_channel or 0)
        self.w_content_amp = float(w_content_amp)
        self.content_feature = None
        if self.content_layer is not None and dict((s[0], s[1]) for s in net.seq).get(self.content_layer) != "conv":
            raise KeyError("content_layer %r is not a conv layer of the loss network" % (self.content_layer,))
        self.v_batch = None                         # the content means run over the whole image batch (one sess.run)
        self.w_hist = float(w_hist)
        self.hist_layers = list(hist_layer) if self.w_hist else []
        self.w_hist_layers = [float(w) for w in w_hist_layer] if self.w_hist else []
        if len(self.w_hist_layers) == 1 and len(self.hist_layers) > 1:
            self.w_hist_layers = self.w_hist_layers * len(self.hist_layers)
        if len(self.w_hist_layers) != len(self.hist_layers):
            raise ValueError("w_hist_layer has %d entries for %d hist layers (one weight, or one per layer)"
                             % (len(self.w_hist_layers), len(self.hist_layers)))
        self.hist_targets = None
        vgg_hist = [n for n in self.hist_layers if "input" not in n]
        wanted = self.layers + vgg_hist + ([self.content_layer] if self.content_layer else [])
        if not wanted:
            raise ValueError("no loss term reaches the loss network: w_style 0 (or no style layer) and no content / "
                             "histogram layer")
        self.top = max(wanted, key=order.index)
        self.style_grams = None

    set_style_image = RenderStyleLoss.set_style_image
    set_content_image = RenderStyleLoss.set_content_image
    set_hist_image = RenderStyleLoss.set_hist_image
    _hist_job = RenderStyleLoss._hist_job
    _hist_input = RenderStyleLoss._hist_input
    _content_job = RenderStyleLoss._content_job
    _keep = RenderStyleLoss._keep
    _batch_views = RenderStyleLoss._batch_views
    out_hw = RenderStyleLoss.out_hw

    def d_img(self, d):
        B, H, W, _ = d.shape
        H2, W2 = self.out_hw(H, W)
        dimg, _ = ops.loss_net_input_fwd(d.contiguous(), H2, W2, want_x=False)
        return dimg

    def loss_and_grad(self, d, d_gray=None):
        """d [B,H,W,3], or [B,H,W,1] (a grey image: the 2-D grid stylizer's clipped density); d_gray [B,H,W,1] (mask,
        constant).  Returns (loss per image [B], dL/dd)."""
        B, H, W, Cin = d.shape
        H2, W2 = self.out_hw(H, W)
        hist_in = any("input" in n for n in self.hist_layers)
        dimg, x = ops.loss_net_input_fwd(d.contiguous(), H2, W2, want_d_img=self.w_tv > 0 or hist_in)
        acts = self.net.forward(x, self.top, keep=self._keep())
        loss = torch.zeros(B, dtype=torch.float32, device=d.device)
        sg = {}
        for name, wl in zip(self.layers, self.w_layers):
            F = acts[name]
            _, h, w, cpad = F.shape
            c = _channels(acts, name, F)
            if self.style_mask:
                if not _post_relu(name):
                    raise NotImplementedError("style_mask on a '*_pre_relu' style layer (the mask adjoint folds the ReLU in)")
                m = ops.resize_bicubic_tf1(d_gray.contiguous(), h, w)      # [B,h,w,1], constant (no gradient to it)
                Fm, scale_dev = ops.style_mask_apply(F, m)                 # F * m, 1 / (2 area C)
                if c != cpad:
                    scale_dev = scale_dev * (float(cpad) / float(c))       # (rows padded with zero channels)
                G = ops.gram_fwd(Fm, 1.0, scale_dev=scale_dev)
                Dm = ops.style_loss_fwd(G, self.style_grams[name], wl * self.w_style, loss)
                dFm = ops.gram_bwd(Fm, Dm, 1.0, scale_dev=scale_dev, relu_mask=False)
                sg[name] = ops.style_mask_bwd(dFm, m, F)
            else:
                scale = 1.0 / (2.0 * h * w * c)
                G = ops.gram_fwd(F, scale)
                Dm = ops.style_loss_fwd(G, self.style_grams[name], wl * self.w_style, loss)
                sg[name] = ops.gram_bwd(F, Dm, scale, relu_mask=_post_relu(name))
        self._content_job(acts, sg, loss)
        hmask = d_gray if self.style_mask else None     # masked histogram branch (styler_base.py:196-201)
        self._hist_job(acts, sg, loss, hmask)
        g_x = self.net.backward(acts, sg, self.top)
        if hist_in:
            self._hist_input(dimg, loss, g_x, hmask)
        if self.w_tv > 0:
            tv = torch.zeros(1, dtype=torch.float32, device=d.device)
            ops.tv_loss(dimg, self.w_tv, tv, g_x)
            loss = loss + tv / B
        g_d = ops.loss_net_input_bwd(g_x, H, W, Cin)
        return loss, g_d


# --------------------------------------------------------------------------------------
# 3-D colour path: a colour volume seen through the views of a grey density (include/nfs_colour.h)
# --------------------------------------------------------------------------------------

class ColourRenderLoss(object):
    """The loss of a colour volume q [D,H,W,3] rendered through V views whose absorption is a grey density d [D,H,W]
    (target_field 'c' of the 3-D particle stylizer), around an ``ImageStyleLoss``:

        w = T / M (ops.ray_weights), J = sum_z w rotate(q) (ops.colour_project_fwd), img = clip(J, 0, 1) -> image loss

    d does not depend on the variable, so everything of it -- the weights, the grey image and the style mask
    d_gray = clip(I / M, 0, 1) -- is formed once per frame and view set (``prepare``); a step is the projection, the
    image loss and the projection's transpose.  The maximum M is taken per ``v_batch`` views (nfs_maxnorm_fwd's groups)
    and the image loss sees the views v_batch at a time, as one loss-net batch of the reference graph does: the total
    over V views is the sum of the view batches' losses whichever ``views_mode`` presents them.  Eager launches only.

    ``render="liquid"`` (include/nfs_liquid.h; '' and 'smoke' are the model above, every launch and bit of it unchanged):
    front-to-back alpha compositing over ``background`` (three numbers in [0,1], default white).  With S = rotate(d),
    B[z] the sum of the samples in front of z and t = exp(-tau sum_z S) the ray's transmittance,

        w = tau exp(-tau B) phi(tau S) (ops.liquid_weights, one pass, no maximum),  J = sum_z w rotate(q) + t bg

    still linear in q, so the projection, its transposes and the image loss are the ones above; the context carries
    ``t_total``, the constant image ``bg_img`` = t (x) bg [V,H,W,3], ``grey`` = 1 - t (the reference's liquid image),
    ``d_gray`` = (1 - t)[..., None] and ``gmax`` = None; ``v_batch`` only groups the image-loss batches.  sum_z w S + t = 1,
    so a uniform colour c0 (q = c0 d) renders c0 (1 - t) + t bg, the reference's commented line styler_3p.py:153.  The
    clip and its adjoint (``ops.clamp01_bwd``) see J with the background in it.  The weights are non-negative and at most
    tau, so the 'coef' route's bound max |g| max w on the sample gradient (``ops.colour_project_bwd``,
    nfs_rotate_bwd_coef in nfs_hip.h) holds as it does for T / M.  On the particle path d is smoothed by ``k`` and the
    emission q is not (as in the smoke mode), so rotate(q) / S can exceed the particles' colour there and the clip takes
    what is above 1; smoothing the emission is not built.

    ``render="exposure"`` (include/nfs_exposure.h): the smoke model at a fixed ``exposure`` kappa > 0 in place of the maximum,

        w = kappa tau T (ops.exposure_weights, one pass, one launch),  J = sum_z w rotate(q)  over black

    so a weight depends on its own ray alone and the brightness of a sequence no longer follows each frame's brightest
    pixel.  The context carries ``grey`` = sum_z w S <= kappa (1 - t), ``d_gray`` = clip(grey, 0, 1)[..., None] and
    ``gmax`` = None; ``background`` has no effect; ``v_batch`` only groups the image-loss batches.  At kappa = 1 a uniform
    colour c0 (q = c0 d) renders at most c0 (1 - t) and is never clipped.  The weights are at most kappa tau.

    ``loss_and_grad(..., absorb=True)`` (liquid or exposure render, no ``style_mask``; include/nfs_absorb.h,
    include/nfs_exposure.h) also returns the gradient
    in the volume d given to ``prepare`` with q held constant -- the joint variable of target_field 'pc', where d moves
    with the particles.  It is formed after the projection's transpose, which needs the weights: ``ops.liquid_absorb_bwd``
    (exposure render: ``ops.exposure_absorb_bwd``, g_S = -tau times the inclusive prefix of a w from the near end)
    writes g_S over ``ctx["w"]`` and ``ops.rotate_bwd`` (tiled, bit-reproducible) takes it to d, so the context is SPENT
    afterwards (``ctx["spent"]``; a second call with it raises).  Two cases are refused with a ValueError: the smoke
    render, whose maximum M couples every ray (its adjoint in the density is not built), and ``style_mask``, whose mask
    1 - t would depend on the variable (the gradient through it is not built)."""

    RENDERS = COLOUR_RENDERS

    def __init__(self, image_loss, transmit, v_batch=1, render="", background=(1, 1, 1), exposure=1.0):
        if render not in self.RENDERS:
            raise ValueError("colour_render %r is none of %s" % (render, self.RENDERS))
        self.image_loss = image_loss
        self.tau = float(transmit)
        self.v_batch = max(int(v_batch or 1), 1)
        self.liquid = render == "liquid"
        self.fixed_exposure = render == "exposure"
        self.background = colour_background(background)
        self.exposure = colour_exposure(exposure)
        self._bg_dev = None

    def _prepare_exposure(self, d3, rot):
        w, grey = ops.exposure_weights(d3, rot, self.tau, self.exposure)
        return {"rot": rot, "w": w, "grey": grey, "gmax": None,
                "d_gray": torch.clamp(grey, 0, 1).unsqueeze(-1).contiguous()}

    def _prepare_liquid(self, d3, rot):
        w, grey, t = ops.liquid_weights(d3, rot, self.tau)
        if self._bg_dev is None or self._bg_dev.device != d3.device:
            self._bg_dev = torch.tensor(self.background, dtype=torch.float32, device=d3.device)
        bg_img = (t.unsqueeze(-1) * self._bg_dev).contiguous()
        return {"rot": rot, "w": w, "grey": grey, "gmax": None, "d_gray": grey.unsqueeze(-1).contiguous(), "t_total": t,
                "bg_img": bg_img, "d3": d3}

    def prepare(self, d3, rot):
        """d3 [D,H,W], rot [V,3,3] -> the frame's context: ray weights w [V,D,H,W], the grey image, d_gray [V,H,W,1]
        (liquid: also t_total [V,H,W], bg_img [V,H,W,3] and ``d3`` itself, for ``loss_and_grad(absorb=True)``)"""
        if self.liquid:
            return self._prepare_liquid(d3, rot)
        if self.fixed_exposure:
            return self._prepare_exposure(d3, rot)
        V = int(rot.shape[0])
        w = torch.empty((V,) + tuple(d3.shape), dtype=torch.float32, device=d3.device)
        grey, _ = ops.rotate_render_fwd(d3, rot, self.tau, False, d_rot=w)
        norm, gmax = ops.maxnorm_fwd(grey, max(V // self.v_batch, 1))
        ops.ray_weights(w, self.tau, gmax, out=w)                # in place: the samples are not needed again
        d_gray = torch.clamp(norm, 0, 1).unsqueeze(-1).contiguous()
        return {"rot": rot, "w": w, "grey": grey, "gmax": gmax, "d_gray": d_gray}

    def _batches(self, V):
        vb = self.v_batch if (V > self.v_batch and V % self.v_batch == 0) else V
        return [(lo, lo + vb) for lo in range(0, V, vb)]

    def project(self, q, ctx):
        """(J [V,H,W,C] before the clip, clip(J, 0, 1))"""
        J = ops.colour_project_fwd(q, ctx["rot"], ctx["w"])
        if self.liquid:
            J += ctx["bg_img"]                           # (t bg: one small add per step)
        return J, torch.clamp(J, 0, 1)

    def loss_and_grad(self, q, ctx, route=None, absorb=False):
        """q [D,H,W,3] -> (losses [V], g_q [D,H,W,3]); ``route``: the transpose's (``ops.colour_project_bwd``; None: by size).
        ``absorb``: -> (losses, g_q, g_d [D,H,W]), g_d the gradient in the volume ``prepare`` was given (liquid or exposure
        render without style_mask only); the context's weights are overwritten and the context marked spent"""
        if absorb:
            if not (self.liquid or self.fixed_exposure):
                raise ValueError("absorb=True on the smoke colour render: the maximum M of w = T / M couples every ray and "
                                 "its adjoint in the density is not built (use colour_render 'liquid' or 'exposure')")
            if self.image_loss.style_mask:
                raise ValueError("absorb=True with style_mask: the mask 1 - t would depend on the density and the gradient "
                                 "through it is not built (pass style_mask false)" if self.liquid else
                                 "absorb=True with style_mask: the mask clip(grey, 0, 1) would depend on the density and "
                                 "the gradient through it is not built (pass style_mask false)")
        if ctx.get("spent"):
            raise ValueError("this colour context is spent: loss_and_grad(absorb=True) overwrote its ray weights (prepare "
                             "a new one)")
        J, img = self.project(q, ctx)
        V = J.shape[0]
        losses, grads = [], []
        for lo, hi in self._batches(V):
            l, g = self.image_loss.loss_and_grad(img[lo:hi].contiguous(), ctx["d_gray"][lo:hi].contiguous())
            losses.append(l); grads.append(g)
        g_img = grads[0] if len(grads) == 1 else torch.cat(grads, 0)
        g_J = ops.clamp01_bwd(g_img.contiguous(), J)
        g_q = ops.colour_project_bwd(g_J, ctx["rot"], ctx["w"], route=route)
        losses = losses[0] if len(losses) == 1 else torch.cat(losses, 0)
        if not absorb:
            return losses, g_q
        ctx["spent"] = True                              # (the weights are dead from here on: g_S goes over them)
        if self.fixed_exposure:
            g_S = ops.exposure_absorb_bwd(g_J, q, ctx["rot"], ctx["w"], self.tau, out=ctx["w"])
            return losses, g_q, ops.rotate_bwd(g_S.unsqueeze(-1), ctx["rot"], tiled=True).squeeze(-1)
        g_S = ops.liquid_absorb_bwd(g_J, q, ctx["d3"], ctx["rot"], ctx["w"], ctx["t_total"], self._bg_dev[:q.shape[-1]],
                                    self.tau, out=ctx["w"])
        g_d = ops.rotate_bwd(g_S.unsqueeze(-1), ctx["rot"], tiled=True).squeeze(-1)
        return losses, g_q, g_d

    def d_img(self, q, ctx):
        """the 0..255 image the loss network sees, [V,H',W',3] (float32: uint8-ready)"""
        return self.image_loss.d_img(self.project(q, ctx)[1])


# --------------------------------------------------------------------------------------
# 3-D colour grid: a colour field seen through the frame's own grey volume (include/nfs_emission.h)
# --------------------------------------------------------------------------------------

class ColourGridStylizer(object):
    """One key frame of a 3-D grid sequence stylised in colour (``grid_variable 'c'`` of styler_grid), around a
    ``ColourRenderLoss``.  For the bound input density d [D,H,W]:

        e    = smooth3d_relu(d, k)          the grey volume the 'd' path renders at zero change: it absorbs AND emits, and
                                            does not depend on the variable
        ctx  = ColourRenderLoss.prepare(e, rot)      ray weights w = T / M, the grey image, d_gray = clip(I / M, 0, 1), one
                                            maximum per ``v_batch`` views
        q    = clamp01(c) * e               the emission (``ops.emission_fwd``), e broadcast over the channels; c [D,H,W,3]
                                            is the variable ``var``
        J    = sum_z w rotate(q),  img = clip(J, 0, 1)  ->  the image loss;  (losses [V], g_q) = loss_and_grad(q, ctx)
        g_c  = g_q * e  where 0 <= c <= 1, else 0     (``ops.emission_bwd``: the clamp's convention is nfs_clamp01_bwd's, a
                                            colour exactly 0 or 1 passes its gradient)

    and one optimiser step on the summed view losses (``views = sum``, as every grid variable).  Where e == 0 the gradient
    is an exact zero; e may carry the -0.0 with which nfs_smooth3d_relu_fwd marks the voxels its ReLU cut, which compares
    equal to zero everywhere it is used.
    The surface is the one styler_grid's frame loop uses on ``GridStylizer``: ``var``, ``lr``, ``bind(d0, var, adam)``,
    ``step(rot)`` -> the summed loss (0-d device tensor), ``gradient(rot)`` -> (losses [V], g_c) without an update.
    e and the context are formed anew whenever the bound density or the view tensor is not the one they were formed from
    (``Stamp`` / ``holds``): a one-frame run with fixed views forms them once, redrawn views form the context every step.
    Adam takes the fused update (``TFAdamState.step_through_emission``; ``NFS_FUSE_ADAM=0``: ``ops.emission_bwd`` then
    ``step``), L-BFGS and 'lapnorm' (nd = 3) ``ops.emission_bwd`` then their own ``step``.  ``bwd_route``: the route of the
    projection's transpose (``ops.colour_project_bwd``; None: by size); with 'tiled' a step is bit-reproducible.
    Eager launches only.  Not built: hipGraph replay, dead-region masks, slab sharding, a view process group."""

    def __init__(self, colour_loss, d0, k=3, lr=0.1, optimizer="adam", lap_n=3, bwd_route=None):
        if bwd_route is not None and bwd_route not in ops.COLOUR_BWD_ROUTES:
            raise ValueError("bwd_route %r is none of %s" % (bwd_route, ops.COLOUR_BWD_ROUTES))
        self.loss = colour_loss
        self.k = float(k)
        self.lr = float(lr)
        self.bwd_route = bwd_route
        self.adam = make_optimizer(optimizer, lap_n=lap_n)
        if isinstance(self.adam, LapDescentState):
            self.adam.nd = 3
        self.fuse_adam = os.environ.get("NFS_FUSE_ADAM", "1") != "0" and isinstance(self.adam, TFAdamState)
        self.d0 = d0.contiguous()
        D, H, W = d0.shape
        self.var = torch.zeros(D, H, W, 3, dtype=torch.float32, device=d0.device)
        self.e = self._e_of = None                  # smooth3d_relu(d0, k) and the stamp of the density it was formed from
        self.ctx = self._ctx_of = None              # the frame's context and the stamp of (e, rot)
        self.contexts_formed = 0

    def bind(self, d0, var=None, adam=None):
        """re-point the stylizer at another frame of the same shape: a pointer swap"""
        assert tuple(d0.shape) == tuple(self.d0.shape)
        self.d0 = d0.contiguous()
        if var is not None:
            assert tuple(var.shape) == tuple(self.var.shape), (tuple(var.shape), tuple(self.var.shape))
            self.var = var
        if adam is not None:
            self.adam = adam
            self.fuse_adam = self.fuse_adam and isinstance(adam, TFAdamState)
            if isinstance(adam, LapDescentState):
                adam.nd = 3

    def grey(self):
        """e = smooth3d_relu(d0, k) of the bound density (kept while that density stands unmodified)"""
        if not holds(self._e_of, self.d0):
            self.e = ops.smooth3d_relu_fwd(self.d0, self.k)
            self._e_of = Stamp(self.d0)
        return self.e

    def context(self, rot):
        e = self.grey()
        if not holds(self._ctx_of, e, rot):
            self.ctx = self.loss.prepare(e, rot)
            self._ctx_of = Stamp(e, rot)
            self.contexts_formed += 1
        return self.ctx

    def emission(self):
        """q [D,H,W,3] of the current variable"""
        return ops.emission_fwd(self.var, self.grey())

    def _loss_gradient(self, rot):
        ctx = self.context(rot)
        return self.loss.loss_and_grad(self.emission(), ctx, route=self.bwd_route)

    def gradient(self, rot):
        """(losses [V], d sum(losses) / d c [D,H,W,3]) without an update"""
        losses, g_q = self._loss_gradient(rot)
        return losses, ops.emission_bwd(g_q.contiguous(), self.var, self.grey())

    def step(self, rot):
        losses, g_q = self._loss_gradient(rot)
        g_q = g_q.contiguous()
        if self.fuse_adam:
            self.adam.step_through_emission(self.var, self.grey(), g_q, self.lr)
        else:
            self.adam.step(self.var, ops.emission_bwd(g_q, self.var, self.grey()), self.lr)
        return losses.sum()

    def d_img(self, rot):
        """the 0..255 colour image of the current variable through ``rot``, [V,H',W',3]"""
        return self.loss.d_img(self.emission(), self.context(rot))

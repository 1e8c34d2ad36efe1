"""Timing of the liquid colour render (csrc/liquid.hip, engine.ColourRenderLoss(render="liquid")) on one GPU, in
tools/colour_grid_bench.py's way: device events around windows of about half a second, every form warmed up first, the forms
alternated in one process.

  1. the frame's context at 200^3 x 8 views and at 200 x 300 x 200 x 9, on a smoke density of compact support, tau = 0.2:
       fused        nfs_liquid_weights (w, grey and t_total in one pass; 4 V D H W bytes written plus the gathers of d)
       composition  nfs_rotate_render_fwd(liquid = 1, d_rot =) followed by torch's flip / cumsum / exp / expm1 / divide
       smoke        the smoke context's own prepare on the same inputs (rotate + render, maximum, T / M)
  2. one liquid 'c' step beside one smoke 'c' step, on the grid stylizer and on the particle stylizer, 200^3 x 8 views
     (conv1_1 .. conv5_1, eager).

    python tools/colour_liquid_bench.py [--out profiles/colour_liquid_ab.txt] [--append] [--no-steps]

The spread is what repeating the identical command gives: run it twice (the second time with --append) and compare.  The
fused kernel stays where it beats the composition by more than the largest difference between the two runs."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from colour_bench import LAYERS, WINDOW, alternate       # noqa: E402

TAU = 0.2


def density(shape):
    """a smoke ball of compact support with some structure, any shape (about a third of the volume is non-zero)"""
    z, y, x = torch.meshgrid(*[torch.linspace(-1, 1, n, device="cuda") for n in shape], indexing="ij")
    r2 = (z / 0.8) ** 2 + (y / 0.7) ** 2 + (x / 0.7) ** 2
    return (torch.clamp(1 - r2, min=0) ** 2 * (0.6 + 0.4 * torch.cos(9 * x + 5 * y))).contiguous()


def contexts(lines, shape, V):
    from neural_flow_style_amd import engine, ops
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    D, H, W = shape
    n = D * H * W
    where = "%dx%dx%d x %d" % (D, H, W, V)
    rot = T.rot_to_device(S.uniform_views(V), "cuda:0")
    d = ops.smooth3d_relu_fwd(density(shape), 3.0)
    w = torch.empty((V, D, H, W), device="cuda")
    grey, t = torch.empty((V, H, W), device="cuda"), torch.empty((V, H, W), device="cuda")
    s_rot, raysum = torch.empty_like(w), torch.empty_like(grey)
    smoke = engine.ColourRenderLoss(None, TAU, v_batch=1)

    def composed():
        g, rs = ops.rotate_render_fwd(d, rot, TAU, True, img=grey, raysum=raysum, d_rot=s_rot)
        B = torch.flip(torch.cumsum(torch.flip(s_rot, [1]), 1), [1]) - s_rot
        x = s_rot * TAU
        phi = torch.where(x > 0, -torch.expm1(-x) / x, torch.ones((), device="cuda"))
        return torch.exp(B * -TAU) * phi * TAU, g, torch.exp(rs * -TAU)

    # (the two forms agree: the composition is the restatement the tests hold the kernel to, in float32)
    wk, gk, tk = ops.liquid_weights(d, rot, TAU, w=w, grey=grey.clone(), t_total=t)
    wc, gc, tc = composed()
    assert float((wk - wc).abs().max()) <= 1e-5 and float((tk - tc).abs().max()) <= 1e-5, "the two forms disagree"
    del wk, wc, gk, gc, tk, tc
    st = alternate([lambda: ops.liquid_weights(d, rot, TAU, w=w, grey=grey, t_total=t), composed,
                    lambda: smoke.prepare(d, rot)])
    names = ["nfs_liquid_weights", "rotate_render_fwd(liquid, d_rot) + torch", "smoke prepare (rotate_render, max, T / M)"]
    nbytes = 4 * V * n + 4 * n + 8 * V * H * W
    for name, (m, lo, hi) in zip(names, st):
        lines.append("%-18s %-10s %-44s %9.1f us [%9.1f, %9.1f]" % (where, "context", name, m * 1e6, lo * 1e6, hi * 1e6))
    lines.append("%-18s %-10s nfs_liquid_weights moves %.1f MB (w, grey, t written, d read once): %.2f TB/s"
                 % (where, "context", nbytes / 1e6, nbytes / st[0][0] / 1e12))


def _cfg(over):
    from neural_flow_style_amd.config import get_config
    cfg, _ = get_config([])
    base = dict(network="vgg_19.ckpt", data_dir="/nonexistent", synthetic_weights=True, k=3, num_frames=1, batch_size=1,
                frames_per_opt=1, window_sigma=0, interp=1, lr=0.002, iter=1, octave_n=1, style_layer=LAYERS,
                w_style_layer=[1] * 5, w_style=1.0, w_content=0, transmit=TAU, rotate=True, v_batch=1,
                sample_type="uniform", resize_scale=1.0, w_tv=0)
    base.update(over)
    for k, v in base.items():
        setattr(cfg, k, v)
    cfg.rng = np.random.RandomState(cfg.seed)
    return cfg


def grid_steps(lines, G, V):
    """one 'c' step of the grid stylizer (loss chain, gradient, fused Adam) with the liquid and with the smoke render"""
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd.styler_grid import Styler
    rng = np.random.RandomState(123)
    d0 = density((G, G, G)).cpu().numpy()
    simg = S.style_image(G, G, rng)
    fns = []
    for render in ("liquid", ""):
        st = Styler(_cfg(dict(resolution=[G, G, G], n_views=V, style_target=simg, grid_variable="c", colour_render=render)))
        st.rot_mat_ = [np.asarray(m, np.float32) for m in S.uniform_views(V)]
        st.load_img([G, G])
        S_ = st.prepare({"d": [d0], "c_init": [np.full((G, G, G, 3), 0.5, np.float32)]})
        S_.work.copy_(S_.g_opt[0])
        S_.gs.bind(S_.d[0], S_.work.view(S_.shape), None)
        fns.append(lambda gs=S_.gs, rot=st._rot(): gs.step(rot))
    (a, alo, ahi), (b, blo, bhi) = alternate(fns, rounds=2, warm=3)
    lines.append("%d^3 x %d views, grid: one liquid 'c' step %8.3f ms [%8.3f, %8.3f]   one smoke 'c' step %8.3f ms [%8.3f, %8.3f]"
                 % (G, V, a * 1e3, alo * 1e3, ahi * 1e3, b * 1e3, blo * 1e3, bhi * 1e3))


def particle_steps(lines, G, V, n_particles=500000):
    """one 'c' step of the particle stylizer (views summed, the contexts kept) with the liquid and with the smoke render"""
    from neural_flow_style_amd import engine
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    from neural_flow_style_amd.styler_3p import Styler
    rng = np.random.RandomState(3)
    p = S.blob_particles(n_particles, rng)
    simg = S.style_image(G, G, rng)
    fns = []
    for render in ("liquid", ""):
        st = Styler(_cfg(dict(resolution=[G, G, G], domain=[G, G, G], radius=0.5, nsize=1, support=4, rest_density=1000,
                              clip=False, target_field="c", n_views=V, views_mode="sum", style_target=simg, num_kernels=1,
                              w_pressure=0, w_density=0, colour_render=render)))
        st.load_img([G, G])
        st.colour.image_loss.set_style_image(st._style_feature(st.style_img, [G, G]))
        pd = st._dev(p)
        pd = pd[T.grid_order(pd, [G, G, G])].contiguous()
        r = torch.full((pd.shape[0], 1), 1000.0, device=st.device)
        var = torch.full((pd.shape[0], 3), 0.5, device=st.device)
        rot = st._rot(0, V)
        adam = engine.make_optimizer("adam")

        def step(st=st, pd=pd, r=r, var=var, rot=rot, adam=adam):
            _, gr = st._value_and_grad(pd, r, var, [G, G, G], rot, view_shard=False)
            adam.step(var, gr.contiguous(), 0.002)
        fns.append(step)
    (a, alo, ahi), (b, blo, bhi) = alternate(fns, rounds=2, warm=2)
    lines.append("%d^3 x %d views, %d particles: one liquid 'c' step %8.3f ms [%8.3f, %8.3f]   one smoke 'c' step %8.3f ms "
                 "[%8.3f, %8.3f]" % (G, V, n_particles, a * 1e3, alo * 1e3, ahi * 1e3, b * 1e3, blo * 1e3, bhi * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_liquid_ab.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--size", type=int, default=200)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/colour_liquid_bench.py on %s: per call, mean [min, max] over alternated windows of about %.1f s"
             % (torch.cuda.get_device_name(0), WINDOW)]
    G = a.size
    for shape, V in (((G, G, G), 8), ((G, G * 3 // 2, G), 9)):
        contexts(lines, shape, V)
        torch.cuda.empty_cache()
    if not a.no_steps:
        grid_steps(lines, G, 8)
        torch.cuda.empty_cache()
        particle_steps(lines, G, 8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

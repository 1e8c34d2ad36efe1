"""Timing of the colour grid path (csrc/emission.hip, engine.ColourGridStylizer) on one GPU, in tools/colour_bench.py's way:
device events around windows of about half a second, every form warmed up first, the forms alternated in one process.

  1. at 200^3 voxels, C = 3, on a smoke density (synthetic.blob_density: e == 0 in the empty part) and on a dense one:
       forward     nfs_emission_fwd             | torch: clamp(c, 0, 1) * e[..., None]
       adjoint     nfs_emission_bwd             | torch: where((c >= 0) & (c <= 1), g * e[..., None], 0)
       update      nfs_emission_bwd_adam        | nfs_emission_bwd + nfs_adam_tf_step
     each with the bytes it moves, from the shapes, over its time;
  2. one 'c' step of the grid stylizer at 200^3 x 8 views (conv1_1 .. conv5_1, eager) beside one 'v' step on the same volume
     and views, and inside the 'c' step the projection and its transpose by themselves.

    python tools/colour_grid_bench.py [--out profiles/colour_grid_ab.txt] [--append] [--no-steps]

The spread is what repeating the identical command gives: run it twice (the second time with --append) and compare.  A
fused form stays where it beats its composition by more than the largest difference between the two runs."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from colour_bench import LAYERS, WINDOW, alternate, report       # noqa: E402


def kernels(lines, G, dense):
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import synthetic as S
    C, n = 3, G ** 3
    gen = torch.Generator(device="cuda").manual_seed(2)
    if dense:
        d = torch.rand((G, G, G), device="cuda", generator=gen) * 0.9 + 0.1
    else:
        d = torch.tensor(S.blob_density(G, np.random.RandomState(123)), device="cuda")
    e = ops.smooth3d_relu_fwd(d.contiguous(), 3.0)
    live = float((e > 0).float().mean())
    where = "%d^3 %s (%.0f%% live)" % (G, "dense" if dense else "smoke", 100 * live)
    c = torch.rand((G, G, G, C), device="cuda", generator=gen) * 1.3 - 0.15
    g = torch.randn((G, G, G, C), device="cuda", generator=gen)
    q, g_c = torch.empty_like(c), torch.empty_like(c)
    e1 = e.unsqueeze(-1)

    st = alternate([lambda: ops.emission_fwd(c, e, out=q), lambda: torch.clamp(c, 0, 1) * e1])
    # kernel: c and e read, q written; torch: the clamp reads c and writes a volume, the product reads it and e and writes q
    report(lines, where, "forward", ["nfs_emission_fwd", "torch clamp(c, 0, 1) * e"], st,
           [4 * n * (2 * C + 1), 4 * n * (4 * C + 1)])

    def bwd_torch():
        return torch.where((c >= 0) & (c <= 1), g * e1, torch.zeros((), device="cuda"))
    st = alternate([lambda: ops.emission_bwd(g, c, e, out=g_c), bwd_torch])
    # torch: two compares (c read twice, two byte masks written), their and (two read, one written), the product (g and e
    # read, a volume written), the select (mask and product read, the result written)
    report(lines, where, "adjoint", ["nfs_emission_bwd", "torch where(0 <= c <= 1, g * e, 0)"], st,
           [4 * n * (3 * C + 1), 4 * n * (2 * C + 1 + 3 * C) + n * C * 6])

    x, m, v = c.clone(), torch.zeros_like(c), torch.zeros_like(c)
    x2, m2, v2 = c.clone(), torch.zeros_like(c), torch.zeros_like(c)
    hyper = (1e-6, 0.9, 0.999, 1e-8)              # (a tiny step: the colours stay where their mask is)

    def composed():
        ops.emission_bwd(g, x2, e, out=g_c)
        ops.adam_tf_step(x2, m2, v2, g_c, *hyper)
    st = alternate([lambda: ops.emission_bwd_adam(g, x, e, m, v, *hyper), composed])
    report(lines, where, "update", ["nfs_emission_bwd_adam", "nfs_emission_bwd + nfs_adam_tf_step"], st,
           [4 * n * (7 * C + 1), 4 * n * (3 * C + 1) + 4 * n * 7 * C])


def steps(lines, G, V):
    """one 'c' step beside one 'v' step of the grid stylizer on the same volume and views: the loss chain, the variable's
    gradient and one Adam step (``st.gs.step``), and the colour projection and its transpose of that step by themselves"""
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd.config import get_config
    from neural_flow_style_amd.styler_grid import Styler
    rng = np.random.RandomState(123)
    d0 = S.blob_density(G, rng)
    simg = S.style_image(G, G, rng)
    fns = {}
    for kind in ("c", "v"):
        cfg, _ = get_config([])
        over = dict(network="vgg_19.ckpt", data_dir="/nonexistent", synthetic_weights=True, resolution=[G, G, G], k=3,
                    num_frames=1, batch_size=1, frames_per_opt=1, window_sigma=0, interp=1, lr=0.002, iter=1, octave_n=1,
                    style_layer=LAYERS, w_style_layer=[1] * 5, w_style=1.0, w_content=0, transmit=0.01, rotate=True,
                    n_views=V, v_batch=1, sample_type="uniform", resize_scale=1.0, style_target=simg, grid_variable=kind,
                    w_tv=0)
        for k, v in over.items():
            setattr(cfg, k, v)
        cfg.rng = np.random.RandomState(cfg.seed)
        st = Styler(cfg)
        st.rot_mat_ = [np.asarray(m, np.float32) for m in S.uniform_views(V)]      # bench.py's 8-view lattice
        st.load_img([G, G])
        S_ = st.prepare({"d": [d0], "c_init": [np.full((G, G, G, 3), 0.5, np.float32)],
                         "v_init": [(rng.randn(G, G, G, 3) * 0.3 / (G - 1)).astype(np.float32)]})
        S_.work.copy_(S_.g_opt[0])
        S_.gs.bind(S_.d[0], S_.work.view(S_.shape), None)
        rot = st._rot()
        fns[kind] = (lambda gs=S_.gs, rot=rot: gs.step(rot)), st
    gs = fns["c"][1]._st.gs
    gs.step(fns["c"][1]._rot())
    ctx, q = gs.ctx, gs.emission()
    g_img = torch.randn((V, G, G, 3), device="cuda") * 1e-3

    stats = alternate([fns["c"][0], fns["v"][0], lambda: ops.colour_project_fwd(q, ctx["rot"], ctx["w"]),
                       lambda: ops.colour_project_bwd(g_img, ctx["rot"], ctx["w"], route=gs.bwd_route)], rounds=2, warm=3)
    (c, clo, chi), (v, vlo, vhi), (pf, _, _), (pb, _, _) = stats
    lines.append("%d^3 x %d views: one 'c' step %8.3f ms [%8.3f, %8.3f]   one 'v' step %8.3f ms [%8.3f, %8.3f]"
                 % (G, V, c * 1e3, clo * 1e3, chi * 1e3, v * 1e3, vlo * 1e3, vhi * 1e3))
    lines.append("%d^3 x %d views: inside the 'c' step, projection %8.3f ms + transpose (%s) %8.3f ms = %.0f%% of the step"
                 % (G, V, pf * 1e3, ops.colour_bwd_route(V, G, G, G), pb * 1e3, 100 * (pf + pb) / c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_grid_ab.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--size", type=int, default=200)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/colour_grid_bench.py on %s: per call, mean [min, max] over alternated windows of about %.1f s"
             % (torch.cuda.get_device_name(0), WINDOW)]
    for dense in (False, True):
        kernels(lines, a.size, dense)
        torch.cuda.empty_cache()
    if not a.no_steps:
        steps(lines, a.size, 8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

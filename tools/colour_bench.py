"""Timing of the colour view path (csrc/colour.hip, engine.ColourRenderLoss) on one GPU:

  1. each entry point of libnfs_colour.so against the composition of existing entry points it stands for, alternated in
     one process: device events around windows of about half a second, every form warmed up first, and the bytes each form
     moves, from the shapes.  200^3 x 8 views and 200 x 300 x 200 x 9 views, C = 3:
       forward     nfs_colour_project_fwd       | rotate_fwd(C=3) times w, summed over z (torch)
       weights     nfs_ray_weights              | torch flip / cumsum / exp / divide on d_rot
       transpose   nfs_colour_project_bwd       | per channel: the product materialised + nfs_rotate_bwd (tiled)
                   ('atomic')                   | per channel: nfs_rotate_bwd_coef with u = w, A = g, B = 0
                                                | rotate_bwd(C=3) (float atomics) on the materialised product
     the transpose also at eleven smaller volumes, around the sizes where ops.colour_bwd_route changes its answer;
  2. one 'c' step of the 3-D particle stylizer at 8 views beside one 'p' step on the same particles (conv1_1 .. conv5_1).

    python tools/colour_bench.py [--out profiles/colour_ab.txt] [--append] [--no-steps]

The spread is what repeating the identical command gives: run it twice (the second time with --append) and compare.  A
kernel stays ops' default where it beats the composition by more than the larger spread between the two runs."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 0.5               # seconds
LAYERS = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def alternate(fns, rounds=3, warm=3):
    """seconds per call of every form: windows of about WINDOW seconds each, the forms alternated; (mean, min, max)"""
    for f in fns:
        for _ in range(warm):
            f()
        torch.cuda.synchronize()
    counts = [max(int(WINDOW / max(window(f, 2), 1e-7)), 2) for f in fns]
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            times[i].append(window(f, counts[i]))
    return [(float(np.mean(t)), float(np.min(t)), float(np.max(t))) for t in times]


def report(lines, where, op, names, stats, nbytes):
    for name, (m, lo, hi), nb in zip(names, stats, nbytes):
        lines.append("%-18s %-10s %-44s %9.1f us [%9.1f, %9.1f]  %7.1f MB moved  %6.2f TB/s"
                     % (where, op, name, m * 1e6, lo * 1e6, hi * 1e6, nb / 1e6, nb / m / 1e12))


def kernels(lines, shape, V, transpose_only=False):
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    D, H, W = shape
    C = 3
    n, rays = D * H * W, H * W
    where = "%dx%dx%d x %d" % (D, H, W, V)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rot = T.rot_to_device(S.uniform_views(V), "cuda:0")
    d_rot = torch.rand((V, D, H, W), device="cuda", generator=gen) * 0.5
    gmax = torch.rand((V,), device="cuda", generator=gen) + 0.5
    q = torch.rand((D, H, W, C), device="cuda", generator=gen)
    g = torch.randn((V, H, W, C), device="cuda", generator=gen)
    tau = 0.01

    w = torch.empty_like(d_rot)
    if transpose_only:
        ops.ray_weights(d_rot, tau, gmax, out=w)
        return transpose(lines, where, ops, rot, w, g, V, D, H, W, C)

    # ---- weights: read d_rot, write w

    def weights_torch():
        acc = torch.flip(torch.cumsum(torch.flip(d_rot, [1]), 1), [1])
        return torch.exp(acc * -tau) / gmax.reshape(V, 1, 1, 1)
    st = alternate([lambda: ops.ray_weights(d_rot, tau, gmax, out=w), weights_torch])
    # (torch: two flips, the cumsum, the scale, the exp and the divide each read and write the volume)
    report(lines, where, "weights", ["nfs_ray_weights", "torch flip/cumsum/exp/divide"], st, [8 * V * n, 6 * 8 * V * n])

    # ---- forward
    img = torch.empty((V, H, W, C), device="cuda")

    def fwd_composed():
        return (ops.rotate_fwd(q, rot) * w.unsqueeze(-1)).sum(1)
    st = alternate([lambda: ops.colour_project_fwd(q, rot, w, out=img), fwd_composed])
    # kernel: w once, q once (gathers that hit in cache), the image; composed: the rotated [V,D,H,W,3] volume written, read
    # for the product with w, the product written and read by the sum
    report(lines, where, "forward", ["nfs_colour_project_fwd", "rotate_fwd(C=3) * w summed over z"], st,
           [4 * V * n + 4 * C * n + 4 * C * V * rays, 4 * C * n + 4 * 4 * C * V * n + 4 * V * n + 4 * C * V * rays])

    transpose(lines, where, ops, rot, w, g, V, D, H, W, C)


def transpose(lines, where, ops, rot, w, g, V, D, H, W, C):
    n, rays = D * H * W, H * W

    def bwd_rotate3():
        return ops.rotate_bwd((w.unsqueeze(-1) * g.unsqueeze(1)).contiguous(), rot, tiled=False)
    forms = [("nfs_colour_project_bwd (atomic)", lambda: ops.colour_project_bwd(g, rot, w, route="atomic")),
             ("per channel: g w + nfs_rotate_bwd tiled", lambda: ops.colour_project_bwd(g, rot, w, route="tiled"))]
    if ops.render_coef_layout(V, D, H, W) is not None:
        forms.append(("per channel: nfs_rotate_bwd_coef (u=w, A=g)", lambda: ops.colour_project_bwd(g, rot, w, route="coef")))
    forms.append(("g w materialised + rotate_bwd(C=3) atomic", bwd_rotate3))
    st = alternate([f for _, f in forms])
    atomics = 8 * C * 4 * V * n                      # added bytes: 8 corners x C channels per sample
    nbytes = {"nfs_colour_project_bwd (atomic)": 4 * V * n + 4 * C * V * rays + atomics,
              # per channel: the product written, the pre-pass and the tiled kernel read it, the plane written; + interleave
              "per channel: g w + nfs_rotate_bwd tiled": C * (4 * V * n + 3 * 4 * V * n + 4 * n) + 2 * 4 * C * n,
              "per channel: nfs_rotate_bwd_coef (u=w, A=g)": C * (4 * V * n + 4 * n) + 2 * 4 * C * n,
              "g w materialised + rotate_bwd(C=3) atomic": 4 * V * n + 2 * 4 * C * V * n + atomics}
    report(lines, where, "transpose", [k for k, _ in forms], st, [nbytes[k] for k, _ in forms])
    lines.append("%-18s %-10s float atomic adds of the scatter forms: %.2f GB of added bytes" % (where, "transpose", atomics / 1e9))


def steps(lines, G, V, n_particles=200000):
    """one 'c' step beside one 'p' step on the same particles: the views summed, the variable's gradient and one Adam step"""
    from neural_flow_style_amd import engine
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    from neural_flow_style_amd.config import get_config
    from neural_flow_style_amd.styler_3p import Styler
    rng = np.random.RandomState(3)
    p = S.blob_particles(n_particles, rng)
    simg = S.style_image(G, G, rng)
    out = {}
    for target in ("c", "p"):
        cfg, _ = get_config([])
        over = dict(network="vgg_19.ckpt", data_dir="/nonexistent", synthetic_weights=True, resolution=[G, G, G],
                    domain=[G, G, G], radius=0.5, nsize=1, support=4, rest_density=1000, k=3, clip=False,
                    target_field=target, num_frames=1, batch_size=1, frames_per_opt=1, window_sigma=0, interp=1,
                    lr=0.002, iter=1, octave_n=1, style_layer=LAYERS, w_style_layer=[1] * 5, w_style=1.0, w_content=0,
                    transmit=0.01, rotate=True, n_views=V, v_batch=1, sample_type="uniform", resize_scale=1.0,
                    views_mode="sum", style_target=simg, num_kernels=1, w_pressure=0, w_density=0, w_tv=0)
        for k, v in over.items():
            setattr(cfg, k, v)
        cfg.rng = np.random.RandomState(cfg.seed)
        st = Styler(cfg)
        st.load_img([G, G])
        (st.colour.image_loss if target == "c" else st.loss).set_style_image(st._style_feature(st.style_img, [G, G]))
        pd = st._dev(p)
        pd = pd[T.grid_order(pd, [G, G, G])].contiguous()          # (as Styler.run orders them)
        r = torch.full((pd.shape[0], 1), 1000.0, device=st.device)
        var = torch.full((pd.shape[0], 3), 0.5, device=st.device) if target == "c" else torch.zeros(pd.shape[0], 3, device=st.device)
        rot = st._rot(0, V)
        adam = engine.make_optimizer("adam")

        def step(st=st, pd=pd, r=r, var=var, rot=rot, adam=adam):
            _, gr = st._value_and_grad(pd, r, var, [G, G, G], rot, view_shard=False)
            adam.step(var, gr.contiguous(), 0.002)
        out[target] = (step, st)
    (c, clo, chi), (pp, plo, phi) = alternate([out["c"][0], out["p"][0]], rounds=2, warm=2)
    lines.append("%d^3 x %d views, %d particles: one 'c' step %8.3f ms [%8.3f, %8.3f]   one 'p' step %8.3f ms [%8.3f, %8.3f]"
                 % (G, V, n_particles, c * 1e3, clo * 1e3, chi * 1e3, pp * 1e3, plo * 1e3, phi * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_ab.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/colour_bench.py on %s: per call, mean [min, max] over alternated windows of about %.1f s"
             % (torch.cuda.get_device_name(0), WINDOW)]
    for shape, V in (((200, 200, 200), 8), ((200, 300, 200), 9)):
        kernels(lines, shape, V)
        torch.cuda.empty_cache()
    # where ops.colour_bwd_route changes its answer: small volumes (launch-bound) and volumes without a coefficient layout
    # (the last three lie between the sizes at which the coefficient form loses and wins against the materialised product)
    for shape, V in (((17, 12, 12), 3), ((16, 32, 32), 8), ((16, 64, 64), 8), ((16, 64, 96), 8), ((16, 64, 128), 8),
                     ((16, 100, 100), 8), ((32, 100, 100), 8), ((12, 200, 200), 8), ((64, 128, 128), 8),
                     ((100, 150, 150), 8), ((128, 200, 200), 8)):
        kernels(lines, shape, V, transpose_only=True)
    if not a.no_steps:
        steps(lines, 200, 8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

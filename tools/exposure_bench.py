"""Timing of the two kernels of libnfs_exposure.so (csrc/exposure.hip) beside their neighbours on one GPU, in
tools/absorb_bench.py's way: device events around windows of about half a second, every form warmed up first and alternated
in one process, on tools/colour_liquid_bench.py's smoke ball of compact support, tau = 0.2, C = 3.

    python tools/exposure_bench.py [--out profiles/exposure_ab.txt] [--append] [--size 200] [--views 8]

nfs_exposure_weights stands beside the smoke render's route to its weights -- rotate_render_fwd(d_rot), maxnorm_fwd, then
ray_weights in place: three launches that write the [V,D,H,W] samples, read them and write them again -- and beside
nfs_liquid_weights, its twin with one more special function per sample.  nfs_exposure_absorb_bwd stands beside
nfs_liquid_absorb_bwd, which gathers the density as well and evaluates psi; both write a buffer of their own (over w itself,
as the joint path runs them, the loads and stores are the same).  The bytes are each volume once.  The spread is what
repeating the identical command gives: run it twice (the second time with --append) and compare."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from colour_bench import WINDOW, alternate              # noqa: E402
from colour_liquid_bench import TAU, density            # noqa: E402


def kernels(lines, shape, V, C=3):
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    D, H, W = shape
    n, rays = D * H * W, H * W
    where = "%dx%dx%d x %d" % (D, H, W, V)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rot = T.rot_to_device(S.uniform_views(V), "cuda:0")
    d = ops.smooth3d_relu_fwd(density(shape), 3.0)
    q = (torch.rand((D, H, W, C), device="cuda", generator=gen) * d.unsqueeze(-1)).contiguous()
    g = torch.randn((V, H, W, C), device="cuda", generator=gen)
    bg = torch.tensor([0.2, 0.6, 0.05, 0.4][:C], device="cuda")
    w, w_smoke, w_liquid = (torch.empty((V, D, H, W), device="cuda") for _ in range(3))
    grey, grey_l, t = (torch.empty((V, H, W), device="cuda") for _ in range(3))

    def smoke_route():
        gr, _ = ops.rotate_render_fwd(d, rot, TAU, False, d_rot=w_smoke)
        _, gmax = ops.maxnorm_fwd(gr, V)
        ops.ray_weights(w_smoke, TAU, gmax, out=w_smoke)

    ops.exposure_weights(d, rot, TAU, 1.0, w=w, grey=grey)
    ops.liquid_weights(d, rot, TAU, w=w_liquid, grey=grey_l, t_total=t)
    g_s = torch.empty_like(w)
    st = alternate([lambda: ops.exposure_weights(d, rot, TAU, 1.0, w=w, grey=grey),
                    smoke_route,
                    lambda: ops.liquid_weights(d, rot, TAU, w=w_liquid, grey=grey_l, t_total=t),
                    lambda: ops.exposure_absorb_bwd(g, q, rot, w, TAU, out=g_s),
                    lambda: ops.liquid_absorb_bwd(g, q, d, rot, w_liquid, t, bg, TAU, out=g_s)])
    names = ["nfs_exposure_weights", "rotate_render_fwd + maxnorm + ray_weights", "nfs_liquid_weights",
             "nfs_exposure_absorb_bwd (C = %d)" % C, "nfs_liquid_absorb_bwd (C = %d)" % C]
    img = 4 * V * rays
    nbytes = [4 * V * n + 4 * n + img, 12 * V * n + 4 * n + 3 * img, 4 * V * n + 4 * n + 2 * img,
              8 * V * n + 4 * n * C + img * C, 8 * V * n + 4 * n * (1 + C) + img * (1 + C)]
    for name, (m, lo, hi), nb in zip(names, st, nbytes):
        lines.append("%-18s %-44s %9.1f us [%9.1f, %9.1f]  %7.1f MB (each volume once)  %5.2f TB/s"
                     % (where, name, m * 1e6, lo * 1e6, hi * 1e6, nb / 1e6, nb / m / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_ab.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--views", type=int, default=8)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/exposure_bench.py on %s: per call, mean [min, max] over alternated windows of about %.1f s"
             % (torch.cuda.get_device_name(0), WINDOW)]
    kernels(lines, (a.size, a.size, a.size), a.views)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

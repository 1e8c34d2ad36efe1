"""Timing of nfs_liquid_absorb_bwd (csrc/absorb.hip) beside its forward twin nfs_liquid_weights (csrc/liquid.hip) on one GPU,
in tools/colour_liquid_bench.py's way: device events around windows of about half a second, both kernels warmed up first and
alternated in one process, on that tool's smoke ball of compact support, tau = 0.2, C = 3.

    python tools/absorb_bench.py [--out profiles/absorb_ab.txt] [--append] [--size 200] [--views 8]

The forward kernel writes 4 V D H W bytes of w; the adjoint reads them and writes as many of g_s (here over w itself, as the
joint path runs it) and gathers q beside d.  The spread is what repeating the identical command gives: run it twice (the
second time with --append) and compare."""
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
    n = D * H * W
    where = "%dx%dx%d x %d" % (D, H, W, V)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rot = T.rot_to_device(S.uniform_views(V), "cuda:0")
    d = ops.smooth3d_relu_fwd(density(shape), 3.0)
    q = (torch.rand((D, H, W, C), device="cuda", generator=gen) * d.unsqueeze(-1)).contiguous()
    g = torch.randn((V, H, W, C), device="cuda", generator=gen)
    bg = torch.tensor([0.2, 0.6, 0.05, 0.4][:C], device="cuda")
    w = torch.empty((V, D, H, W), device="cuda")
    grey, t = torch.empty((V, H, W), device="cuda"), torch.empty((V, H, W), device="cuda")
    g_s = torch.empty_like(w)
    ops.liquid_weights(d, rot, TAU, w=w, grey=grey, t_total=t)
    # (over w itself the kernel reads what the last call wrote: the same loads and stores, other numbers)
    st = alternate([lambda: ops.liquid_weights(d, rot, TAU, w=w, grey=grey, t_total=t),
                    lambda: ops.liquid_absorb_bwd(g, q, d, rot, w, t, bg, TAU, out=g_s)])
    names = ["nfs_liquid_weights", "nfs_liquid_absorb_bwd (C = %d)" % C]
    nbytes = [4 * V * n + 4 * n + 8 * V * H * W, 8 * V * n + 4 * n * (1 + C) + 4 * V * H * W * (1 + C)]
    for name, (m, lo, hi), nb in zip(names, st, nbytes):
        lines.append("%-18s %-34s %9.1f us [%9.1f, %9.1f]  %7.1f MB (each volume once)  %5.2f TB/s"
                     % (where, name, m * 1e6, lo * 1e6, hi * 1e6, nb / 1e6, nb / m / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absorb_ab.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--views", type=int, default=8)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/absorb_bench.py on %s: per call, mean [min, max] over alternated windows of about %.1f s"
             % (torch.cuda.get_device_name(0), WINDOW)]
    kernels(lines, (a.size, a.size, a.size), a.views)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

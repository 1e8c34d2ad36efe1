"""Timing of optimizer 'lapnorm' (csrc/descent.hip, engine.LapDescentState) on one GPU:

  1. each fused kernel against the composition it replaces, alternated in one process: device events around windows of
     about half a second, every case warmed up first; algorithmic bytes per voxel of both and the achieved share of the
     HBM peak.  3-D at 200^3 (with and without the live mask), 2-D at 512 x 1024;
  2. one 'lapnorm' step at 200^3 x 8 views (the flagship's loss: conv1_1 .. conv5_1) for each target, next to the Adam
     step of the same target, and the time the calls of ``util.lap_normalize`` take inside the step (device events around
     every C-ABI call of one step: the pyramid's down, up, up_rms and normalize_mean calls).

    python tools/lapnorm_bench.py [--out profiles/lapnorm_ab.txt] [--append] [--grid 200] [--views 8]

The spread is what repeating the identical command gives: run it twice (the second time with --append) and compare."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X
WINDOW = 0.5               # seconds
LAYERS = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]
LAP_CALLS = ("nfs_lap_", "nfs_normalize_mean")


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def alternate(fa, fb, rounds=3, warm=10):
    """seconds per call of fa and fb: windows of about WINDOW seconds each, alternated; (mean, min, max) of the windows"""
    out = []
    for f in (fa, fb):
        for _ in range(warm):
            f()
        torch.cuda.synchronize()
    na, nb = (max(int(WINDOW / max(window(f, 5), 1e-7)), 5) for f in (fa, fb))
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, na))
        tb.append(window(fb, nb))
    for t in (ta, tb):
        out.append((float(np.mean(t)), float(np.min(t)), float(np.max(t))))
    return out


def row(lines, where, name, a, b, ba, bb, n):
    (a, alo, ahi), (b, blo, bhi) = a, b
    lines.append("%-10s %-30s fused %8.2f us [%8.2f, %8.2f]  composed %8.2f us [%8.2f, %8.2f]  bytes/voxel %d / %d  "
                 "HBM share %.1f %% / %.1f %%" % (where, name, a * 1e6, alo * 1e6, ahi * 1e6, b * 1e6, blo * 1e6, bhi * 1e6,
                                                  ba, bb, 100 * ba * n / a / HBM_PEAK, 100 * bb * n / b / HBM_PEAK))


def kernels(lines, G):
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import synthetic as S
    rng = np.random.RandomState(1)
    d = torch.tensor(S.blob_density(G, rng)).cuda()
    n = G ** 3
    g = (torch.randn(G, G, G, 3, device="cuda") * (0.5 / G)).contiguous()
    v1 = (torch.randn(G, G, G, 3, device="cuda") * (1.0 / G)).contiguous()
    v2 = v1.clone()
    adv1, adv2 = torch.empty(G, G, G, device="cuda"), torch.empty(G, G, G, device="cuda")
    lr = 1e-6                                     # (the velocity stays where it is over the thousands of calls of a window)
    d4 = d.unsqueeze(-1)
    for live in (False, True):
        m1 = ops.live_mask(G, G, G, like=d) if live else None
        m2 = ops.live_mask(G, G, G, like=d) if live else None

        def composed():
            ops.descent_step(v2, g, lr)
            ops.advect_fwd(d4, v2, out=adv2.unsqueeze(-1), live=m2)
        a, b = alternate(lambda: ops.advect_descent(d, v1, g, lr, adv1, m1), composed)
        # per voxel: g 12 + velocity in 12 + out 12 + density gather 4 + sample 4 (+ 1/8 mask); composed: 12 more (re-read)
        row(lines, "%d^3" % G, "advect_descent_fwd" + (" + live mask" if live else ""), a, b, 44, 56, n)
    H, W = 512, 1024
    d2 = torch.tensor(S.blob_density2d(H, W, rng)).cuda()
    g2 = (torch.randn(H, W, 2, device="cuda") * (0.5 / W)).contiguous()
    w1 = (torch.randn(H, W, 2, device="cuda") * (1.0 / W)).contiguous()
    w2 = w1.clone()
    o1 = torch.empty(H, W, device="cuda")

    def composed2():
        ops.descent_step(w2, g2, lr)
        ops.advect2d_fwd(d2.unsqueeze(-1), w2)
    a, b = alternate(lambda: ops.advect2d_descent(d2, w1, g2, lr, o1), composed2, warm=50)
    row(lines, "%dx%d" % (H, W), "advect2d_descent_fwd", a, b, 8 + 8 + 8 + 4 + 4, 8 + 8 + 8 + 8 + 4 + 4, H * W)


def steps(lines, G, V):
    from neural_flow_style_amd import _lib, engine, vgg
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    rng = np.random.RandomState(123)
    d0 = torch.tensor(S.blob_density(G, rng)).cuda()
    vel = torch.tensor(S.curl_velocity(G, rng, max_cells=2.0)).cuda()
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv5_1"), "cuda:0")
    loss = engine.RenderStyleLoss(net, LAYERS, [1.0] * 5, 1.0, transmit=0.01)
    loss.set_style_image(S.style_image(G, G, rng))
    rot = T.rot_to_device(S.uniform_views(V), "cuda:0")
    for kind in ("v", "s", "p", "sp", "d"):
        def make(optimizer):
            gs = engine.GridStylizer(loss, d0, k=3, target=kind, lr=1e-4 if optimizer == "lapnorm" else 1e-3,
                                     optimizer=optimizer, graph=False)
            if kind == "v":
                gs.var.copy_(vel)
            elif kind != "d":
                gs.var.normal_(0, 0.3 / G)
            for _ in range(3):
                gs.step(rot)
            return gs
        lap, adam = make("lapnorm"), make("adam")
        (a, alo, ahi), (b, blo, bhi) = alternate(lambda: lap.step(rot), lambda: adam.step(rot), rounds=2, warm=2)
        _lib.PROFILE = {}
        lap.step(rot)
        torch.cuda.synchronize()
        prof, _lib.PROFILE = _lib.PROFILE, None
        t_lap = sum(e0.elapsed_time(e1) for k, v in prof.items() if k.startswith(LAP_CALLS) for (e0, e1, _) in v)
        t_upd = sum(e0.elapsed_time(e1) for k, v in prof.items() if "descent" in k for (e0, e1, _) in v)
        lines.append("%d^3 x %d views  step %-2s lapnorm %8.3f ms [%8.3f, %8.3f]  adam %8.3f ms [%8.3f, %8.3f]  "
                     "lap_normalize in the step %.3f ms, the update kernel %.3f ms (C = %d)"
                     % (G, V, kind, a * 1e3, alo * 1e3, ahi * 1e3, b * 1e3, blo * 1e3, bhi * 1e3, t_lap, t_upd,
                        lap.var.numel() // d0.numel()))
        del lap, adam
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lapnorm_ab.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--no-steps", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/lapnorm_bench.py on %s: per call, mean [min, max] over alternated windows of about %.1f s"
             % (torch.cuda.get_device_name(0), WINDOW)]
    kernels(lines, a.grid)
    if not a.no_steps:
        steps(lines, a.grid, a.views)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

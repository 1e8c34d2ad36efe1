"""Timing of the 2-D grid path (csrc/grid2d.hip, grid2d.GridStylizer2D) on one GPU:

  1. each fused kernel against the composition it replaces, alternated in one process: device events around windows of
     at least half a second, every shape warmed up first; algorithmic bytes per pixel of both and the achieved share of
     the HBM peak;
  2. one stylisation step per target (style layers conv2_1, conv3_1): time, C-ABI calls per step and the share of the
     step spent in field kernels (everything but the loss network's calls);
  3. the step with hipGraph replay on against off.

    python tools/grid2d_bench.py [--out profiles/grid2d_ab.txt] [--append]

The spread is what repeating the identical command gives: run it twice (the second time with --append) and compare."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X
SIZES = [(512, 1024), (256, 256)]
WINDOW = 0.5               # seconds


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def alternate(fa, fb, rounds=3):
    """seconds per call of fa and fb: windows of >= WINDOW seconds each, alternated; (mean, min, max) of the windows"""
    out = []
    for f in (fa, fb):
        for _ in range(20):
            f()
        torch.cuda.synchronize()
    na, nb = (max(int(WINDOW / max(window(f, 50), 1e-7)), 50) for f in (fa, fb))
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, na))
        tb.append(window(fb, nb))
    for t in (ta, tb):
        out.append((float(np.mean(t)), float(np.min(t)), float(np.max(t))))
    return out


def kernels(lines):
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import synthetic as S
    for (H, W) in SIZES:
        rng = np.random.RandomState(1)
        d = torch.tensor(S.blob_density2d(H, W, rng)).cuda()
        g = torch.randn(H, W, device="cuda")
        d3, g3 = d.unsqueeze(-1), g.unsqueeze(-1)
        n = H * W
        for kind, ch in (("s", 1), ("p", 1), ("sp", 2)):
            x = (torch.randn(ops.source2d_shape(kind, H, W), device="cuda") * (0.5 / W)).contiguous()
            out, vel, gv = torch.empty(H, W, device="cuda"), torch.empty(H, W, 2, device="cuda"), torch.empty(H, W, 2, device="cuda")
            # bytes per pixel, algorithmic: fused forward = variable + d + out; composed = that + velocity written and read
            cases = [
                ("advect2d_source_fwd %s" % kind, lambda: ops.advect2d_source_fwd(kind, d, x, out=out),
                 lambda: ops.advect2d_fwd(d3, ops.source2d_velocity(kind, x, out=vel)), 4 * ch + 8, 4 * ch + 8 + 16),
                ("advect2d_source_bwd %s" % kind, lambda: ops.advect2d_source_bwd(kind, d, x, g, g_vel=gv),
                 lambda: ops.advect2d_bwd(d3, ops.source2d_velocity(kind, x, out=vel), g3, need_d=False),
                 4 * ch + 8 + 8, 4 * ch + 8 + 8 + 16),
            ]
            for name, fa, fb, ba, bb in cases:
                (a, alo, ahi), (b, blo, bhi) = alternate(fa, fb)
                lines.append("%-4dx%-5d %-26s fused %7.2f us [%7.2f, %7.2f]  composed %7.2f us [%7.2f, %7.2f]  "
                             "bytes/pixel %d / %d  HBM share %.1f %% / %.1f %%"
                             % (H, W, name, a * 1e6, alo * 1e6, ahi * 1e6, b * 1e6, blo * 1e6, bhi * 1e6, ba, bb,
                                100 * ba * n / a / HBM_PEAK, 100 * bb * n / b / HBM_PEAK))
        vel0 = (torch.randn(H, W, 2, device="cuda") * (0.5 / W)).contiguous()
        v1, m1, u1 = vel0.clone(), torch.zeros_like(vel0), torch.zeros_like(vel0)
        v2, m2, u2 = vel0.clone(), torch.zeros_like(vel0), torch.zeros_like(vel0)
        adv = torch.empty(H, W, device="cuda")
        hy = (1e-4, 0.9, 0.999, 1e-8)

        def composed():
            _, gvel = ops.advect2d_bwd(d3, v2, g3, need_d=False)
            ops.adam_tf_step(v2, m2, u2, gvel, *hy)
            ops.advect2d_fwd(d3, v2)
        (a, alo, ahi), (b, blo, bhi) = alternate(lambda: ops.advect2d_bwd_adam(d, v1, g, m1, u1, *hy, adv_next=adv), composed)
        ba, bb = 4 + 4 + 48 + 4, 4 + 4 + 8 + 8 + 8 + 48 + 8 + 4 + 4
        lines.append("%-4dx%-5d %-26s fused %7.2f us [%7.2f, %7.2f]  composed %7.2f us [%7.2f, %7.2f]  "
                     "bytes/pixel %d / %d  HBM share %.1f %% / %.1f %%"
                     % (H, W, "advect2d_bwd_adam_fwd", a * 1e6, alo * 1e6, ahi * 1e6, b * 1e6, blo * 1e6, bhi * 1e6, ba, bb,
                        100 * ba * n / a / HBM_PEAK, 100 * bb * n / b / HBM_PEAK))


LOSS_CALLS = ("nfs_conv", "nfs_gram", "nfs_style", "nfs_avgpool", "nfs_loss_net", "nfs_content", "nfs_hist", "nfs_tv")


def steps(lines):
    from neural_flow_style_amd import _lib, engine, vgg
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd.grid2d import GridStylizer2D
    layers = ["conv2_1", "conv3_1"]
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv3_1"), "cuda:0")
    for (H, W) in SIZES:
        rng = np.random.RandomState(2)
        d = torch.tensor(S.blob_density2d(H, W, rng)).cuda()
        loss = engine.ImageStyleLoss(net, layers, [1.0, 1.0], 1.0)
        loss.set_style_image(S.style_image(H, W, rng))
        for kind in ("v", "d", "s", "p", "sp"):
            def make(graph):
                gs = GridStylizer2D(loss, d, target=kind, lr=1e-4, graph=graph)
                if kind != "d":
                    gs.var.normal_(0, 0.3 / W)
                for _ in range(3):
                    gs.step()
                return gs
            eager, replay = make(False), make(True)
            (a, alo, ahi), (b, blo, bhi) = alternate(eager.step, replay.step, rounds=2)
            _lib.PROFILE = {}
            eager.step()
            torch.cuda.synchronize()
            prof, _lib.PROFILE = _lib.PROFILE, None
            calls = sum(len(v) for v in prof.values())
            t_all = sum(e0.elapsed_time(e1) for v in prof.values() for (e0, e1, _) in v)
            t_field = sum(e0.elapsed_time(e1) for k, v in prof.items() if not k.startswith(LOSS_CALLS) for (e0, e1, _) in v)
            lines.append("%-4dx%-5d step %-2s eager %8.1f us [%8.1f, %8.1f]  replay %8.1f us [%8.1f, %8.1f]  "
                         "C-ABI calls %d, field kernels %.1f %% of the summed call times"
                         % (H, W, kind, a * 1e6, alo * 1e6, ahi * 1e6, b * 1e6, blo * 1e6, bhi * 1e6, calls,
                            100 * t_field / max(t_all, 1e-9)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid2d_ab.txt"))
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["# tools/grid2d_bench.py on %s: us per call, mean [min, max] over alternated windows of >= %.1f s"
             % (torch.cuda.get_device_name(0), WINDOW)]
    kernels(lines)
    steps(lines)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

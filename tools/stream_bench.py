"""Stream-function variable at 200^3: each fused kernel against the composition it replaces, and one GridStylizer
iteration with target='s' beside target='v'.

    python tools/stream_bench.py [--grid 200] [--views 8] [--out profiles/stream_function_ab.txt]

Device events, one process; per pair the two variants alternate, five repeats of 20 launches each after a warm-up; median
and spread (max - min over the repeats) per variant, bytes/s on the algorithmic bytes.  A fused kernel "stays" when its
median beats the composition's by more than the larger of the two spreads."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import neural_flow_style_amd.ops as ops
from neural_flow_style_amd import engine, vgg
from neural_flow_style_amd import synthetic as S
from neural_flow_style_amd import transform as T

REPEATS, LAUNCHES = 5, 20
LAYERS = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]


def smooth_psi(G, cells, seed=0):
    """a smooth stream function (9^3 white noise per channel, trilinearly interpolated to G^3) scaled so that the largest
    stream-velocity component is ``cells`` cells (one cell = 2 / (G - 1))"""
    gen = torch.Generator().manual_seed(seed)
    coarse = torch.randn(1, 3, 9, 9, 9, generator=gen)
    s = torch.nn.functional.interpolate(coarse, size=(G, G, G), mode="trilinear", align_corners=True)[0]
    s = s.permute(1, 2, 3, 0).contiguous().cuda()
    peak = float(ops.stream_velocity(s).abs().max()) / (2.0 / (G - 1))
    return (s * (cells / peak)).contiguous()


def time_once(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


def ab(variants):
    """{name: callable} -> {name: (median ms, spread ms)}, the variants alternating within every repeat"""
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, f in variants.items():
            t[k].append(time_once(f))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in t.items()}


def report(say, what, res, nbytes, n):
    (mf, sf), (mc, sc) = res["fused"], res["composed"]
    for k, (m, sp) in res.items():
        say("%-28s %-9s %.4f ms (spread %.4f)  %6.0f GB/s on %3d B/voxel" % (what, k, m, sp, nbytes[k] * n / m / 1e6, nbytes[k]))
    say("%-28s fused stays: %s (composed - fused = %.4f ms, larger spread %.4f ms)" % (what, mc - mf > max(sf, sc), mc - mf,
                                                                                      max(sf, sc)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G, n = a.grid, a.grid ** 3
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("stream-function kernels at %d^3 (device events, %d x %d launches per variant, alternating)" % (G, REPEATS, LAUNCHES))
    rng = np.random.RandomState(0)
    d0 = S.blob_density(G, rng)
    d = torch.tensor(d0, device="cuda")[..., None].contiguous()
    g = torch.randn(G, G, G, 1, device="cuda")
    out, gv, vel = torch.empty_like(d), torch.empty(G, G, G, 3, device="cuda"), torch.empty(G, G, G, 3, device="cuda")
    for cells in (0.02, 2.0):
        s = smooth_psi(G, cells)
        tag = "psi at %.2f cell" % cells

        def fwd_composed():
            ops.advect_fwd(d, ops.stream_velocity(s), out=out)

        def fwd_kernels_only():
            # the composition's two kernels alone, without the channel flip and copy between them (a curl kernel writing
            # advect's order would need no glue): advect on a stored velocity + the curl kernel, the 44 B/voxel floor
            ops.advect_fwd(d, vel, out=out)
            ops.curl_fwd(s)

        report(say, "forward, " + tag, ab({"fused": lambda: ops.advect_stream_fwd(d, s, out=out), "composed": fwd_composed}),
               {"fused": 20, "composed": 44}, n)
        vel.copy_(ops.stream_velocity(s))
        r = ab({"fused": lambda: ops.advect_stream_fwd(d, s, out=out), "composed": fwd_kernels_only})
        say("%-28s curl + advect kernels without the channel flip: %.4f ms (spread %.4f)" % ("forward, " + tag, *r["composed"]))
        report(say, "adjoint, " + tag,
               ab({"fused": lambda: ops.advect_stream_bwd(d, s, g, g_vel=gv),
                   "composed": lambda: ops.advect_bwd(d, ops.stream_velocity(s), g, need_d=False, g_vel=gv)}),
               {"fused": 32, "composed": 56}, n)
    g_vel = torch.randn(G, G, G, 3, device="cuda")
    s = smooth_psi(G, 0.02)
    m, v = torch.zeros_like(s), torch.zeros_like(s)
    s2, m2, v2 = s.clone(), torch.zeros_like(s), torch.zeros_like(s)
    report(say, "update",
           ab({"fused": lambda: ops.stream_bwd_adam(g_vel, s, m, v, 1e-9),
               "composed": lambda: ops.adam_tf_step(s2, m2, v2, ops.stream_velocity_bwd(g_vel), 1e-9)}),
           {"fused": 84, "composed": 108}, n)
    r = ab({"fused": lambda: ops.stream_bwd_adam(g_vel, s, m, v, 1e-9),
            "composed": lambda: ops.adam_tf_step(s2, m2, v2, ops.curl_bwd(g_vel), 1e-9)})
    say("%-28s curl_bwd + adam kernels without the channel flip: %.4f ms (spread %.4f)" % ("update", *r["composed"]))
    del g, out, gv, vel, g_vel, s, m, v, s2, m2, v2

    # one iteration of the stylizer, 's' beside 'v' on the same box ('v' has its fused adjoint + Adam + next forward and the
    # never-live skipping: 's' is expected to be slower; recorded, not gated)
    V = a.views
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv5_1"), "cuda")
    loss = engine.RenderStyleLoss(net, LAYERS, [1.0] * 5, 1.0, transmit=0.01)
    loss.set_style_image(S.style_image(G, G, rng))
    rot = T.rot_to_device(S.uniform_views(V), "cuda")
    psi = smooth_psi(G, 0.5)
    steps = {}
    for target in ("s", "v", "s", "v"):
        gs = engine.GridStylizer(loss, torch.tensor(d0, device="cuda"), k=3, target=target, lr=1e-3)
        gs.var.copy_(psi if target == "s" else ops.stream_velocity(psi))
        for _ in range(4):
            gs.step(rot, loss_view=True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                gs.step(rot, loss_view=True)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 5)
        steps.setdefault(target, []).extend(ts)
        del gs
    for target, ts in steps.items():
        say("GridStylizer step %d^3 x %d views, target='%s': %.3f ms median (min %.3f ... max %.3f over %d windows of 5 steps)"
            % (G, V, target, float(np.median(ts)), min(ts), max(ts), len(ts)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

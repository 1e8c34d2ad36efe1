"""Stream-function, potential and Helmholtz variables at 200^3: each of the nine fused kernels against the composition it
replaces, and one GridStylizer iteration with target='s', 'p' and 'sp' beside 'v'.

    python tools/source_bench.py [--grid 200] [--views 8] [--out profiles/source_ops_ab.txt]

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

# algorithmic bytes per voxel, fused / composed (the composition's kernels alone, without torch's flips, slices and sums
# between them): forward = variable + 4 d + 4 out against the velocity written (12 per operator, + 36 for the sum of two)
# and read again; adjoint = + 4 g_out + 12 g_vel; update = 12 g_vel + 6 x the variable against the gradient written and read
BYTES = {"s": {"forward": (20, 44), "adjoint": (32, 56), "update": (84, 108)},
         "p": {"forward": (12, 36), "adjoint": (24, 48), "update": (36, 44)},
         "sp": {"forward": (24, 96), "adjoint": (36, 108), "update": (108, 152)}}


def smooth_variable(kind, G, cells, seed=0):
    """a smooth variable of that kind (9^3 white noise per channel, trilinearly interpolated to G^3) scaled so that the
    largest component of its velocity is ``cells`` cells (one cell = 2 / (G - 1))"""
    gen = torch.Generator().manual_seed(seed)
    C = {"s": 3, "p": 1, "sp": 4}[kind]
    coarse = torch.randn(1, C, 9, 9, 9, generator=gen)
    x = torch.nn.functional.interpolate(coarse, size=(G, G, G), mode="trilinear", align_corners=True)[0]
    x = x.permute(1, 2, 3, 0).contiguous().cuda()
    x = x[..., 0].contiguous() if kind == "p" else x
    peak = float(ops.source_velocity(kind, x).abs().max()) / (2.0 / (G - 1))
    return (x * (cells / peak)).contiguous()


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

    say("stream-function ('s'), potential ('p') and Helmholtz ('sp') kernels at %d^3 (device events, %d x %d launches per "
        "variant, alternating)" % (G, REPEATS, LAUNCHES))
    rng = np.random.RandomState(0)
    d0 = S.blob_density(G, rng)
    d = torch.tensor(d0, device="cuda")[..., None].contiguous()
    g = torch.randn(G, G, G, 1, device="cuda")
    out, gv, vel = torch.empty_like(d), torch.empty(G, G, G, 3, device="cuda"), torch.empty(G, G, G, 3, device="cuda")
    g_vel = torch.randn(G, G, G, 3, device="cuda")
    for kind in ("s", "p", "sp"):
        nb = {k: {"fused": f, "composed": c} for k, (f, c) in BYTES[kind].items()}
        for cells in (0.02, 2.0):
            x = smooth_variable(kind, G, cells)
            tag = "'%s' at %.2f cell" % (kind, cells)
            report(say, "forward, " + tag,
                   ab({"fused": lambda: ops.advect_source_fwd(kind, d, x, out=out),
                       "composed": lambda: ops.advect_fwd(d, ops.source_velocity(kind, x), out=out)}), nb["forward"], n)
            report(say, "adjoint, " + tag,
                   ab({"fused": lambda: ops.advect_source_bwd(kind, d, x, g, g_vel=gv),
                       "composed": lambda: ops.advect_bwd(d, ops.source_velocity(kind, x), g, need_d=False, g_vel=gv)}),
                   nb["adjoint"], n)
            if kind == "s":
                # the composition's two kernels alone, without the channel flip and copy between them (a curl kernel writing
                # advect's order would need no glue): advect on a stored velocity + the curl kernel, the 44 B/voxel floor
                vel.copy_(ops.stream_velocity(x))
                r = ab({"fused": lambda: ops.advect_stream_fwd(d, x, out=out),
                        "composed": lambda: (ops.advect_fwd(d, vel, out=out), ops.curl_fwd(x))})
                say("%-28s curl + advect kernels without the channel flip: %.4f ms (spread %.4f)" % ("forward, " + tag, *r["composed"]))
        x = smooth_variable(kind, G, 0.02)
        m, v = torch.zeros_like(x), torch.zeros_like(x)
        x2, m2, v2 = x.clone(), torch.zeros_like(x), torch.zeros_like(x)
        report(say, "update, '%s'" % kind,
               ab({"fused": lambda: ops.source_bwd_adam(kind, g_vel, x, m, v, 1e-9),
                   "composed": lambda: ops.adam_tf_step(x2, m2, v2, ops.source_velocity_bwd(kind, g_vel), 1e-9)}),
               nb["update"], n)
        if kind == "s":
            r = ab({"fused": lambda: ops.stream_bwd_adam(g_vel, x, m, v, 1e-9),
                    "composed": lambda: ops.adam_tf_step(x2, m2, v2, ops.curl_bwd(g_vel), 1e-9)})
            say("%-28s curl_bwd + adam kernels without the channel flip: %.4f ms (spread %.4f)" % ("update, 's'", *r["composed"]))
        del x, m, v, x2, m2, v2
    del g, out, gv, vel, g_vel

    # one iteration of the stylizer, the four variables on the same box ('v' has its fused adjoint + Adam + next forward and
    # the never-live skipping: the others are expected to be slower; recorded, not gated)
    V = a.views
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv5_1"), "cuda")
    loss = engine.RenderStyleLoss(net, LAYERS, [1.0] * 5, 1.0, transmit=0.01)
    loss.set_style_image(S.style_image(G, G, rng))
    rot = T.rot_to_device(S.uniform_views(V), "cuda")
    steps = {}
    for target in ("s", "p", "sp", "v") * 2:
        gs = engine.GridStylizer(loss, torch.tensor(d0, device="cuda"), k=3, target=target, lr=1e-3)
        gs.var.copy_(ops.stream_velocity(smooth_variable("s", G, 0.5)) if target == "v" else smooth_variable(target, G, 0.5))
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

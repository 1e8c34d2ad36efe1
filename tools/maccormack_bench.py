"""MacCormack advection (adv_order = 2) at 200^3, C = 1: what the keep mask costs the forward, the hand-written adjoint
against the same adjoint composed from the order-1 entry points, and what the second order costs a GridStylizer step.

    python tools/maccormack_bench.py --out profiles/maccormack_adjoint          # timings (device events)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/maccormack_bench.py --trace adjoint
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/maccormack_bench.py --trace step2 | step1
    python tools/maccormack_bench.py --report DIR_adjoint DIR_step2 DIR_step1 --out profiles/maccormack_adjoint

Data: SURVEY 8(d)'s synthetic density and 2-cell curl velocity (bench.py's problem, seed 123); g = the smooth adjoint's
output of a real order-2 step.  Variants alternate inside one process; every figure is a median over the rounds with the
spread (min ... max) beside it.  Algorithmic bytes per cell (include/nfs_hip.h, docs/kernels/field_ops.md): pass 1 reads
g 4 + vel 12 + d_fwd 4 + mask 1/8, writes g_vel 12; pass 2 reads g 4 + accumulator 8 + d 4 + vel 12 + g_vel 12, writes
12; the accumulators' zero fill 8, the max|g| pre-pass 4, and pass 1's global atomics (8 bytes each: the cells of every
tile and its halo, csrc/warp.hip MT_*; zero cells are skipped, so this is an upper count) come on top."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

HBM_PEAK = 8.0e12            # B/s, spec (MI355X); 6.3e12 is what a float4 copy reaches
ATOMIC_RATE = 1.3e12         # B/s of added bytes, chip-wide, measured for float atomics of a favourable shape
LAYERS = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]
PASS1_BYTES, PASS2_BYTES = 4 + 12 + 4 + 0.125 + 12, 4 + 8 + 4 + 12 + 12 + 12
TILE, HALO = (8, 8, 32), 3   # pass 1's tile and halo (csrc/warp.hip: MT_Z, MT_Y, MT_X, MT_R)


def problem(G, V, device, adv_order, env=None):
    from neural_flow_style_amd import engine, vgg
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    rng = np.random.RandomState(123)
    d0 = S.blob_density(G, rng)
    vel = S.curl_velocity(G, rng, max_cells=2.0)
    simg = S.style_image(G, G, rng)
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv5_1"), device)
    loss = engine.RenderStyleLoss(net, LAYERS, [1.0] * 5, 1.0, transmit=0.01)
    loss.set_style_image(simg)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:                                                     # (the switches are read when the stylizer is built)
        gs = engine.GridStylizer(loss, torch.tensor(d0, device=device), k=3, target="v", lr=1e-3, adv_order=adv_order)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    gs.var.copy_(torch.tensor(vel))
    return gs, T.rot_to_device(S.uniform_views(V), device)


def alternate(variants, window, rounds):
    """variants {name: callable}: per round each variant runs for >= ``window`` seconds between two device events, the
    variants taking turns; returns {name: [ms per call, one per round]}"""
    reps = {}
    for name, f in variants.items():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            f()
        e1.record()
        torch.cuda.synchronize()
        reps[name] = max(5, int(np.ceil(window * 1e3 / max(e0.elapsed_time(e1) / 5, 1e-3))))
    out = {name: [] for name in variants}
    for _ in range(rounds):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[name]):
                f()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps[name])
    return out


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "rounds": len(ms)}


def adjoint_inputs(G, V, device):
    """d, vel, d_fwd, keep, g [G,G,G,1] of a real order-2 step at the benchmark's variable"""
    from neural_flow_style_amd import ops
    gs, rot = problem(G, V, device, 2)
    _, g_ds = gs.field_gradient(rot, for_variable=True)
    g = ops.smooth3d_relu_bwd(gs.d_s, g_ds, gs.k).unsqueeze(-1).contiguous().clone()
    return gs.d0.unsqueeze(-1).contiguous(), gs.var, gs._mc_fwd, gs._mc_keep, g


def composed_adjoint(ops, d, vel, d_fwd, keep_b, g):
    """the same velocity gradient from what the library exported before: two order-1 adjoints and torch glue"""
    gB = torch.where(keep_b, torch.zeros_like(g), g) * -0.5
    sB, hB = ops.advect_bwd(d_fwd, -vel, gB)                # scatter of gB at x + v;  d/d(-v) of the B half
    _, hD = ops.advect_bwd(d, vel, g + sB, need_d=False)
    return hD - hB


def run_timings(args, device):
    from neural_flow_style_amd import ops
    G, n = args.G, float(args.G) ** 3
    d, vel, d_fwd, keep, g = adjoint_inputs(G, args.views, device)
    words = keep.view(torch.int64)
    bit = torch.arange(64, device=device, dtype=torch.int64)
    keep_b = (((words[:, None] >> bit[None, :]) & 1) != 0).reshape(-1)[:int(n)].reshape(G, G, G, 1)
    fired = float(keep_b.float().mean())
    res = {"G": G, "views": args.views, "limiter_fires": fired, "window_s": args.window}
    fwd_buf, keep2 = torch.empty_like(d), torch.zeros_like(keep)
    t = alternate({"forward": lambda: ops.advect_maccormack(d, vel, d_fwd=fwd_buf),
                   "forward_with_mask": lambda: ops.advect_maccormack(d, vel, keep=keep2, d_fwd=fwd_buf)},
                  args.window, args.rounds)
    res["forward"] = {k: summary(v) for k, v in t.items()}
    gv = torch.empty_like(vel)
    new = ops.advect_maccormack_bwd(d, vel, d_fwd, keep, g, need_d=False)[1]
    ref = composed_adjoint(ops, d, vel, d_fwd, keep_b, g)
    res["adjoint_vs_composed_rel_l2"] = float((new.double() - ref.double()).norm() / ref.double().norm())
    t = alternate({"adjoint": lambda: ops.advect_maccormack_bwd(d, vel, d_fwd, keep, g, need_d=False, g_vel=gv),
                   "adjoint_with_g_d": lambda: ops.advect_maccormack_bwd(d, vel, d_fwd, keep, g, g_vel=gv),
                   "composed_from_order_1": lambda: composed_adjoint(ops, d, vel, d_fwd, keep_b, g),
                   "order_1_adjoint": lambda: ops.advect_bwd(d, vel, g, need_d=False, g_vel=gv)},
                  args.window, args.rounds)
    res["adjoint"] = {k: summary(v) for k, v in t.items()}
    a, c = res["adjoint"]["adjoint"], res["adjoint"]["composed_from_order_1"]
    res["adjoint"]["speedup_over_composed"] = c["median_ms"] / a["median_ms"]
    res["adjoint"]["wins_beyond_spread"] = bool(a["max_ms"] < c["min_ms"])
    res["adjoint"]["algorithmic_bytes_per_cell"] = PASS1_BYTES + PASS2_BYTES
    res["adjoint"]["algorithmic_GBps_at_median"] = (PASS1_BYTES + PASS2_BYTES) * n / (a["median_ms"] * 1e-3) / 1e9
    del d, vel, d_fwd, keep, g
    like = {"NFS_FUSE_ADAM": "0", "NFS_FUSE_ADVECT": "0", "NFS_DEAD_SKIP": "0"}
    steps = {}
    for name, order, env in (("order_2", 2, None), ("order_1_like_for_like", 1, like), ("order_1_default", 1, None)):
        gs, rot = problem(G, args.views, device, order, env)
        steps[name] = (lambda gs=gs, rot=rot: gs.step(rot, loss_view=True))
    t = alternate(steps, args.window, args.rounds)
    res["step"] = {k: summary(v) for k, v in t.items()}
    return res


def run_trace(args, device):
    """the work one profiler run looks at, a few repetitions of it"""
    from neural_flow_style_amd import ops
    if args.trace == "adjoint":
        d, vel, d_fwd, keep, g = adjoint_inputs(args.G, args.views, device)
        gv = torch.empty_like(vel)
        for _ in range(args.trace_reps):
            ops.advect_maccormack_bwd(d, vel, d_fwd, keep, g, need_d=False, g_vel=gv)
    else:
        gs, rot = problem(args.G, args.views, device, 2 if args.trace == "step2" else 1)
        for _ in range(args.trace_reps):
            gs.step(rot)
    torch.cuda.synchronize()


def kernel_stats(directory):
    """{kernel name: (calls, average ns)} of a rocprofv3 --kernel-trace --stats run"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def report(args):
    """per-pass kernel time, bytes, share of the HBM peak and pass 1's atomic traffic from the adjoint trace; the kernels
    of an order-2 step that are not nfs:: and that the order-1 step does not launch too"""
    adj, s2, s1 = (kernel_stats(d) for d in args.report)
    n = float(args.G) ** 3
    with open(args.out + ".json") as f:
        res = json.load(f)
    rep = {}
    for key, needle, nbytes in (("pass_1", "maccormack_bwd1_tiled_kernel", PASS1_BYTES), ("pass_2", "maccormack_bwd2x4_kernel", PASS2_BYTES),
                                ("zero_fill", "zero_words_kernel", 8.0), ("absmax", "absmax_kernel", 4.0)):
        hit = [(k, v) for k, v in adj.items() if needle in k]
        if not hit:
            continue
        calls, avg_ns = hit[0][1]
        sec = avg_ns * 1e-9
        rep[key] = {"kernel": hit[0][0].split("(")[0], "calls": calls, "avg_us": avg_ns / 1e3, "algorithmic_bytes_per_cell": nbytes,
                    "algorithmic_GBps": nbytes * n / sec / 1e9, "share_of_hbm_peak": nbytes * n / sec / HBM_PEAK}
    if "pass_1" in rep:
        tiles = np.prod([-(-args.G // t) for t in TILE])
        atomic_bytes = 8.0 * tiles * np.prod([t + 2 * HALO for t in TILE])   # upper count: every cell of every tile + halo
        sec = rep["pass_1"]["avg_us"] * 1e-6
        rep["pass_1"]["atomic_bytes_upper"] = float(atomic_bytes)
        rep["pass_1"]["atomic_GBps_upper"] = atomic_bytes / sec / 1e9
        rep["pass_1"]["time_at_guide_atomic_rate_us"] = atomic_bytes / ATOMIC_RATE * 1e6
        rep["pass_1"]["time_at_hbm_peak_us"] = PASS1_BYTES * n / HBM_PEAK * 1e6
        rep["pass_1"]["bound_by"] = ("atomics" if rep["pass_1"]["time_at_guide_atomic_rate_us"] > rep["pass_1"]["time_at_hbm_peak_us"]
                                     else "HBM")
    base = lambda k: k.split("(")[0].replace("void ", "")
    foreign2 = sorted({base(k) for k in s2 if "nfs::" not in k})
    foreign1 = {base(k) for k in s1 if "nfs::" not in k}
    rep["order_2_step_kernels_outside_nfs"] = foreign2
    rep["of_those_not_in_the_order_1_step"] = [k for k in foreign2 if k not in foreign1]
    res["trace"] = rep
    write(args.out, res)


def write(out, res):
    with open(out + ".json", "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    lines = ["MacCormack advection at %d^3, C = 1, %d views; limiter fires on %.1f %% of the cells; windows of >= %.1f s, "
             "median (min ... max) over the rounds" % (res["G"], res["views"], 100 * res["limiter_fires"], res["window_s"])]
    for group in ("forward", "adjoint", "step"):
        for k, v in sorted(res.get(group, {}).items()):
            if isinstance(v, dict):
                lines.append("%-8s %-24s %8.4f ms (%.4f ... %.4f)" % (group, k, v["median_ms"], v["min_ms"], v["max_ms"]))
            else:
                lines.append("%-8s %-24s %s" % (group, k, v))
    lines.append("adjoint against the composition, relative L2 of g_vel: %.2e" % res["adjoint_vs_composed_rel_l2"])
    for k, v in sorted(res.get("trace", {}).items()):
        lines.append("trace    %-24s %s" % (k, json.dumps(v, sort_keys=True)))
    with open(out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=200)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="maccormack_adjoint")
    ap.add_argument("--trace", choices=["adjoint", "step2", "step1"])
    ap.add_argument("--trace-reps", type=int, default=5)
    ap.add_argument("--report", nargs=3, metavar="DIR")
    args = ap.parse_args()
    if args.report:
        return report(args)
    if not torch.cuda.is_available():
        raise SystemExit("maccormack_bench: needs the GPU (there is no CPU path to time)")
    device = torch.device("cuda")
    if args.trace:
        return run_trace(args, device)
    write(args.out, run_timings(args, device))


if __name__ == "__main__":
    main()

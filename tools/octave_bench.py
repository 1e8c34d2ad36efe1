"""Grid octaves on the MI355X: what the 3-D resize costs, what a stylisation step costs at the octave sizes of 200^3,
and what coarse-to-fine buys at an equal number of steps.

  python tools/octave_bench.py [--grid 200] [--steps 30] [--frames 2] [--seeds 3]

1. nfs_resize3d (corner-aligned bilinear, the octaves' resample) 200^3 -> 111^3 and 111^3 -> 200^3 for C = 1, 3, 4:
   device events around windows of back-to-back launches, shapes warmed first; the algorithmic bytes (every input and
   output element once) over that time, as a share of the HBM peak.
2. one engine.GridStylizer step ('v', 8 views, the problem of bench.py) at 61^3, 111^3 and 200^3.
3. the loss of the last full-resolution iteration of two styler_grid runs of equal total step count on the same seeded
   synthetic sequence: 1 octave x N steps against 3 octaves x N/3 steps.
Every figure comes with the spread of its repeats.  No bar is set on any of them."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                       # noqa: E402  (the flagship problem and its constants)
from neural_flow_style_amd import ops                              # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def event_windows(f, windows=7, reps=50, warm=10):
    """ms per call: ``windows`` windows of ``reps`` back-to-back calls, each between two device events"""
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def resize_part(sizes):
    print("== nfs_resize3d, bilinear, align_corners (ms per launch: median [min .. max] of 7 windows x 50 launches)")
    for n_in, n_out in sizes:
        for C in (1, 3, 4):
            x = torch.randn(n_in, n_in, n_in, C, device="cuda")
            ms, lo, hi = spread(event_windows(lambda: ops.resize3d(x, (n_out,) * 3, "bilinear", True, 1.0)))
            nbytes = 4.0 * C * (n_in ** 3 + n_out ** 3)
            print("resize3d %d^3 -> %d^3 C=%d  %.4f [%.4f .. %.4f] ms  %.1f MB algorithmic  %.0f GB/s = %.1f %% of the "
                  "%.0f GB/s HBM peak" % (n_in, n_out, C, ms, lo, hi, nbytes / 1e6, nbytes / ms / 1e6,
                                          100.0 * nbytes / ms / 1e6 / bench.HBM_PEAK_GBS, bench.HBM_PEAK_GBS))


def step_part(sizes, views):
    print("== one GridStylizer step, 'v', %d views (ms per step: median [min .. max] of 5 windows x 20 steps, host clock "
          "around a synchronised window, 30 steps of warm-up)" % views)
    device = torch.device("cuda")
    for G in sizes:
        gs, rot, _ = bench.build_problem(G, views, device, 0, 1)
        for _ in range(30):
            gs.step(rot)
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(20):
                gs.step(rot)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / 20 * 1e3)
        m, lo, hi = spread(ms)
        print("step %d^3 (voxels %% 4 = %d: %s update)  %.3f [%.3f .. %.3f] ms" %
              (G, G ** 3 % 4, "fused" if gs._fused_step_ok() else "unfused", m, lo, hi))
        del gs
        torch.cuda.empty_cache()


def sequence(G, frames, views, octave_n, iters, seed):
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd.config import get_config
    from neural_flow_style_amd.styler_grid import Styler
    rng = np.random.RandomState(seed)
    d0 = S.blob_density(G, rng)
    vel = S.curl_velocity(G, rng, max_cells=2.0)
    simg = S.style_image(G, G, rng)
    cfg, _ = get_config([])
    for k, v in dict(network="vgg_19.ckpt", data_dir="/nonexistent", synthetic_weights=True, resolution=[G, G, G], k=3,
                     num_frames=frames, batch_size=1, frames_per_opt=1, window_sigma=1.0, interp=1, lr=1e-3, iter=iters,
                     octave_n=octave_n, octave_scale=1.8, style_layer=bench.STYLE_LAYERS, w_style_layer=[1.0] * 5,
                     w_style=1.0, w_content=0, transmit=0.01, rotate=True, n_views=views, v_batch=1,
                     sample_type="uniform", resize_scale=1.0, style_target=simg, grid_variable="v").items():
        setattr(cfg, k, v)
    cfg.rng = np.random.RandomState(seed)
    st = Styler(cfg)
    st.rot_mat_ = [np.asarray(m, np.float32) for m in S.uniform_views(views)]
    st.load_img([G, G])
    params = {"d": [np.roll(d0, 3 * t, axis=2) for t in range(frames)], "v": [np.roll(vel, 3 * t, axis=2) for t in range(frames)],
              "v_init": [vel * 0.1 for _ in range(frames)]}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = st.run(params)
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def loss_part(G, frames, views, steps, seeds):
    assert steps % 3 == 0
    print("== %d frames of %d^3, %d views, lr 1e-3: loss (summed over frames) of the first and the last full-resolution "
          "iteration, wall time of run() with its set-up" % (frames, G, views))
    rows = {1: [], 3: []}
    for seed in range(seeds):
        for octave_n in (1, 3):
            res, dt = sequence(G, frames, views, octave_n, steps // octave_n, 100 + seed)
            full = np.asarray(res["l_frames"])[-(steps // octave_n):].sum(1)
            rows[octave_n].append((full[0], full[-1], dt))
            print("seed %d  %d octave(s) x %d steps  sizes %s  first %.6g  last %.6g  %.2f s" %
                  (100 + seed, octave_n, steps // octave_n, [s[0] for s in res["octave_sizes"]], full[0], full[-1], dt))
    for octave_n in (1, 3):
        last = spread([r[1] for r in rows[octave_n]])
        secs = spread([r[2] for r in rows[octave_n]])
        print("%d octave(s): last full-resolution loss median %.6g [%.6g .. %.6g] over %d seeds; run() %.2f [%.2f .. %.2f] s"
              % ((octave_n,) + last + (seeds,) + secs))
    ratio = [b[1] / a[1] for a, b in zip(rows[1], rows[3])]
    print("last loss, 3 octaves over 1 octave, per seed: %s" % ", ".join("%.4f" % r for r in ratio))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--steps", type=int, default=30, help="total steps per frame of either run (a multiple of 3)")
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("octave_bench.py measures on the GPU: no device found")
    from neural_flow_style_amd.styler_grid import octave_sizes
    sizes = [s[0] for s in octave_sizes([a.grid] * 3, 3, 1.8)]               # 200 -> 61, 111, 200
    print("device %s, octave sizes of %d^3 at scale 1.8: %s" % (torch.cuda.get_device_name(0), a.grid, sizes))
    resize_part([(sizes[2], sizes[1]), (sizes[1], sizes[2])])
    step_part(sizes, a.views)
    loss_part(a.grid, a.frames, a.views, a.steps, a.seeds)


if __name__ == "__main__":
    main()

"""Timing of the carrier-grid kernels (csrc/carrier.hip, include/nfs_carrier.h) on one GPU:

  1. nfs_carrier_bwd in route 0 (per block: the box in LDS where it fits) and route 1 (one global atomic per tap),
     nfs_carrier_displace and nfs_g2p_fwd, alternated in one process: device events around windows of about half a second,
     every form warmed up first.  5e5 blob particles in the grid order of 200^3, a 25^3 carrier, C = 3, cubic and linear;
     the blocks that took the box route are counted, and the two routes' results compared;
  2. one 'g' iteration of the 3-D particle stylizer beside one 'p' iteration of the same configuration (8 views summed,
     conv1_1 .. conv5_1, the same particles).

    python tools/carrier_bench.py [--out profiles/carrier_ab.txt] [--append] [--no-steps] [--n 500000] [--grid 200]

The spread is what repeating the identical command gives: run it twice (the second time with --append) and compare."""
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


def kernels(lines, N, G, carrier):
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    rng = np.random.RandomState(5)
    p = torch.tensor(S.blob_particles(N, rng), device="cuda")
    p = p[T.grid_order(p, [G, G, G])].contiguous()                       # (as Styler.run orders them)
    dims = (carrier,) * 3
    u = torch.tensor(rng.randn(*dims, 3).astype(np.float32) * 0.01, device="cuda")
    g = torch.tensor(rng.randn(N, 3).astype(np.float32), device="cuda")
    for cubic in (True, False):
        taps = 64 if cubic else 8
        out0, n0 = ops.carrier_bwd(g, p, dims, cubic=cubic, route=0, count=True)
        out1 = ops.carrier_bwd(g, p, dims, cubic=cubic, route=1)
        diff = float((out0 - out1).abs().max()) / float(out1.abs().max())
        names = ["nfs_carrier_bwd route 0 (box in LDS)", "nfs_carrier_bwd route 1 (per-tap atomics)",
                 "nfs_carrier_displace", "nfs_g2p_fwd"]
        stats = alternate([lambda: ops.carrier_bwd(g, p, dims, cubic=cubic, route=0),
                           lambda: ops.carrier_bwd(g, p, dims, cubic=cubic, route=1),
                           lambda: ops.carrier_displace(u, p, cubic=cubic),
                           lambda: ops.g2p_fwd(u, p, cubic=cubic)])
        where = "%d particles, %d^3 carrier, %s" % (N, carrier, "cubic" if cubic else "linear")
        for name, (m, lo, hi) in zip(names, stats):
            lines.append("%-44s %-44s %9.1f us [%9.1f, %9.1f]" % (where, name, m * 1e6, lo * 1e6, hi * 1e6))
        lines.append("%-44s box-route blocks %d of %d; %d taps x 3 channels per particle = %.3g contributions; "
                     "max |route 0 - route 1| / max |g_u| = %.2g"
                     % (where, int(n0), (N + 255) // 256, taps, float(N) * taps * 3, diff))


def steps(lines, N, G, carrier, views=8):
    from neural_flow_style_amd import engine
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    from neural_flow_style_amd.config import get_config
    from neural_flow_style_amd.styler_3p import Styler
    rng = np.random.RandomState(6)
    p = S.blob_particles(N, rng)
    simg = S.style_image(G, G, rng)

    def styler(target):
        cfg, _ = get_config([])
        kw = dict(network="vgg_19.ckpt", data_dir="/nonexistent", synthetic_weights=True, resolution=[G, G, G],
                  domain=[G, G, G], radius=0.5, nsize=1, support=4, rest_density=1000, k=3, clip=False, target_field=target,
                  num_frames=1, batch_size=1, frames_per_opt=1, window_sigma=0, interp=1, lr=0.002, iter=1, octave_n=1,
                  style_layer=list(LAYERS), w_style_layer=[1] * len(LAYERS), w_style=1.0, w_content=0, transmit=0.05,
                  rotate=True, n_views=views, v_batch=views, sample_type="uniform", phi0=-5, phi1=5, phi_unit=10,
                  theta0=-10, theta1=10, theta_unit=int(20 // max(views // 2 - 1, 1)), resize_scale=1.0, views_mode="sum",
                  w_pressure=0, w_density=0, w_tv=0, style_mask=False, style_target=simg,
                  carrier_resolution=[carrier] * 3)
        for k, v in kw.items():
            setattr(cfg, k, v)
        cfg.rng = np.random.RandomState(cfg.seed)
        st = Styler(cfg)
        st.load_img([G, G])
        st.loss.set_style_image(st._style_feature(st.style_img, [G, G]))
        return st

    forms, names = [], []
    for target in ("p", "g"):
        st = styler(target)
        pd = st._dev(p)
        pd = pd[T.grid_order(pd, [G, G, G])].contiguous()
        var = torch.zeros(*st._var_shape(N), device="cuda")
        rot = st._rot(0, len(st.rot_mat_))
        adam = engine.make_optimizer("adam")

        def one(st=st, pd=pd, var=var, rot=rot, adam=adam):
            _, g = st._value_and_grad(pd, None, var, [G, G, G], rot, view_shard=False)
            adam.step(var, g.contiguous(), 0.002)
        forms.append(one)
        names.append("target_field '%s': value, gradient and Adam step, %d views" % (target, len(st.rot_mat_)))
    stats = alternate(forms, rounds=3, warm=2)
    where = "%d particles, %d^3, %d^3 carrier" % (N, G, carrier)
    for name, (m, lo, hi) in zip(names, stats):
        lines.append("%-44s %-52s %9.2f ms [%9.2f, %9.2f]" % (where, name, m * 1e3, lo * 1e3, hi * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--carrier", type=int, default=25)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("carrier_bench.py times kernels on the GPU: no GPU visible (there is no CPU path)")
    lines = ["# tools/carrier_bench.py on %s; windows of %.1f s, 3 rounds alternated: mean [min, max]"
             % (torch.cuda.get_device_name(0), WINDOW)]
    kernels(lines, a.n, a.grid, a.carrier)
    if not a.no_steps:
        steps(lines, a.n, a.grid, a.carrier)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

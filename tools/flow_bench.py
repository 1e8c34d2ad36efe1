"""Timing of the carrier-flow kernels (csrc/flow.hip, include/nfs_flow.h) on one GPU, measured the way
tools/carrier_bench.py measures (its ``alternate``: device events around windows of about half a second, every form warmed
up first, the forms alternated, mean [min, max]):

  1. nfs_flow_fwd at K = 1 beside nfs_carrier_displace, nfs_flow_fwd and nfs_flow_bwd at K = 4 and 8, and the ONE transpose
     over the K N positions of the path (nfs_carrier_bwd, route 0) beside the transpose of N particles, with the share of
     its blocks that took the box route.  5e5 blob particles in the grid order of 200^3, a 25^3 carrier, cubic and linear;
  2. one 'g' iteration of the 3-D particle stylizer at --carrier_steps 1 (the branch that stood before the flag) and at
     --carrier_steps 4, the same configuration otherwise (8 views summed, conv1_1 .. conv5_1).

    python tools/flow_bench.py [--out profiles/flow_ab.txt] [--append] [--no-steps] [--n 500000] [--grid 200]

The spread is what repeating the identical command gives: run it twice (the second time with --append) and compare."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from carrier_bench import LAYERS, WINDOW, alternate  # noqa: E402

STEPS = (4, 8)


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
        where = "%d particles, %d^3 carrier, %s" % (N, carrier, "cubic" if cubic else "linear")
        paths = {K: ops.flow_fwd(u, p, K, cubic=cubic) for K in STEPS}
        lams = {K: ops.flow_bwd(u, paths[K], g, cubic=cubic) for K in STEPS}
        names = ["nfs_carrier_displace", "nfs_flow_fwd K = 1", "nfs_carrier_bwd route 0, N particles"]
        forms = [lambda: ops.carrier_displace(u, p, cubic=cubic, want_v=False), lambda: ops.flow_fwd(u, p, 1, cubic=cubic),
                 lambda: ops.carrier_bwd(g, p, dims, cubic=cubic)]
        for K in STEPS:
            pk, lk = paths[K][:K].reshape(K * N, 3), lams[K][1:].reshape(K * N, 3)
            names += ["nfs_flow_fwd K = %d" % K, "nfs_flow_bwd K = %d" % K,
                      "nfs_carrier_bwd route 0, K N = %d x N particles" % K, "ops.flow_grad K = %d (sweep, transpose, scale)" % K]
            forms += [lambda K=K: ops.flow_fwd(u, p, K, cubic=cubic), lambda K=K: ops.flow_bwd(u, paths[K], g, cubic=cubic),
                      lambda pk=pk, lk=lk: ops.carrier_bwd(lk, pk, dims, cubic=cubic),
                      lambda K=K: ops.flow_grad(u, paths[K], g, cubic=cubic)]
        for name, (m, lo, hi) in zip(names, alternate(forms)):
            lines.append("%-44s %-52s %9.1f us [%9.1f, %9.1f]" % (where, name, m * 1e6, lo * 1e6, hi * 1e6))
        for K in STEPS:
            pk, lk = paths[K][:K].reshape(K * N, 3), lams[K][1:].reshape(K * N, 3)
            _, n0 = ops.carrier_bwd(lk, pk, dims, cubic=cubic, route=0, count=True)
            lines.append("%-44s K = %d: box-route blocks of the one transpose %d of %d"
                         % (where, K, int(n0), (K * N + 255) // 256))


def steps(lines, N, G, carrier, views=8):
    from neural_flow_style_amd import engine
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    from neural_flow_style_amd.config import get_config
    from neural_flow_style_amd.styler_3p import Styler
    rng = np.random.RandomState(6)
    p = S.blob_particles(N, rng)
    simg = S.style_image(G, G, rng)

    def styler(K):
        cfg, _ = get_config([])
        kw = dict(network="vgg_19.ckpt", data_dir="/nonexistent", synthetic_weights=True, resolution=[G, G, G],
                  domain=[G, G, G], radius=0.5, nsize=1, support=4, rest_density=1000, k=3, clip=False, target_field="g",
                  num_frames=1, batch_size=1, frames_per_opt=1, window_sigma=0, interp=1, lr=0.002, iter=1, octave_n=1,
                  style_layer=list(LAYERS), w_style_layer=[1] * len(LAYERS), w_style=1.0, w_content=0, transmit=0.05,
                  rotate=True, n_views=views, v_batch=views, sample_type="uniform", phi0=-5, phi1=5, phi_unit=10,
                  theta0=-10, theta1=10, theta_unit=int(20 // max(views // 2 - 1, 1)), resize_scale=1.0, views_mode="sum",
                  w_pressure=0, w_density=0, w_tv=0, style_mask=False, style_target=simg,
                  carrier_resolution=[carrier] * 3, carrier_steps=K)
        for k, v in kw.items():
            setattr(cfg, k, v)
        cfg.rng = np.random.RandomState(cfg.seed)
        st = Styler(cfg)
        st.load_img([G, G])
        st.loss.set_style_image(st._style_feature(st.style_img, [G, G]))
        return st

    forms, names = [], []
    for K in (1, 4):
        st = styler(K)
        pd = st._dev(p)
        pd = pd[T.grid_order(pd, [G, G, G])].contiguous()
        var = torch.zeros(*st._var_shape(N), device="cuda")
        rot = st._rot(0, len(st.rot_mat_))
        adam = engine.make_optimizer("adam")

        def one(st=st, pd=pd, var=var, rot=rot, adam=adam):
            _, g = st._value_and_grad(pd, None, var, [G, G, G], rot, view_shard=False)
            adam.step(var, g.contiguous(), 0.002)
        forms.append(one)
        names.append("'g' at carrier_steps %d: value, gradient, Adam step, %d views" % (K, len(st.rot_mat_)))
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
        raise SystemExit("flow_bench.py times kernels on the GPU: no GPU visible (there is no CPU path)")
    lines = ["# tools/flow_bench.py on %s; windows of %.1f s, 3 rounds alternated: mean [min, max]"
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

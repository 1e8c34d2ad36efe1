"""Every entry point of csrc/render.hip on the smallest shapes that reach each of its code paths, from host-seeded numpy
inputs, all outputs into one .npz:  python tools/render_bits.py OUT.npz

Run it on two builds of the library (two checkouts, or NFS_LIB_PATH) and compare the files with --compare A.npz B.npz:
every array must be equal bit for bit (np.array_equal on the raw words, so NaNs and signed zeros count).  Used to hold
a refactor of render.hip to the parent commit's results (profiles/render_refactor.txt)."""
import os
import sys

import numpy as np

TAU = 0.35


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        x, y = A[k], B[k]
        if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            bad.append(k)
    print("%d arrays, %d values, %d differ%s" % (len(A.files), sum(A[k].size for k in A.files), len(bad),
                                                  (": " + ", ".join(bad[:20])) if bad else ""))
    return 1 if bad else 0


def main(out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import neural_flow_style_amd.ops as ops
    import neural_flow_style_amd.transform as T

    out = {}

    def keep(name, *tensors):
        for i, t in enumerate(tensors):
            out["%s.%d" % (name, i)] = t.detach().float().cpu().numpy().copy()

    def cu(a):
        return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")

    # the identity, then rotations large enough that the plane-advance carry of the march does not apply
    mats = [np.eye(3), T.rot_y_3d(-35.0) @ T.rot_z_3d(20.0), T.rot_y_3d(80.0) @ T.rot_z_3d(5.0)]

    # ---- segmented forward, coefficient form, ray coefficients ---------------------------------------------------
    for D, H, W in ((16, 4, 16), (17, 9, 10), (29, 15, 35), (33, 20, 16)):
        for V in (1, 3):
            rng = np.random.RandomState(100 * D + V)
            d = cu(rng.rand(D, H, W))
            rot = T.rot_to_device(mats[:V], "cuda")
            tag = "seg_%dx%dx%d_v%d" % (D, H, W, V)
            for liquid in (False, True):
                keep("%s.fwd.l%d" % (tag, liquid), *ops.rotate_render_fwd(d, rot, TAU, liquid))
                d_rot = torch.zeros(V, D, H, W, device="cuda")
                keep("%s.fwd_keep.l%d" % (tag, liquid), *ops.rotate_render_fwd(d, rot, TAU, liquid, d_rot=d_rot), d_rot)
            img, rs, u_rot, seg = ops.rotate_render_fwd_coef(d, rot, TAU)
            keep(tag + ".coef", img, rs, u_rot, seg)
            g = rng.randn(V, H, W).astype(np.float32)
            g[:, 1] = 0.0
            g[:, H - 1] = 0.0                                            # two zero rows
            keep(tag + ".ray_coef", *ops.render_ray_coef(cu(g), seg, TAU))

    # ---- one thread per ray: the generic fused forward and the fused adjoint ------------------------------------------
    for H, W in ((12, 10), (12, 1)):
        D, V = 14, 3
        rng = np.random.RandomState(7 + W)
        d = cu(rng.rand(D, H, W))
        rot = T.rot_to_device(mats, "cuda")
        for liquid in (False, True):
            d_rot = torch.zeros(V, D, H, W, device="cuda")
            img, rs = ops.rotate_render_fwd(d, rot, TAU, liquid, d_rot=d_rot)
            keep("ray_14x%dx%d.fwd.l%d" % (H, W, liquid), img, rs, d_rot)
            # (the fused adjoint adds with float atomics, in any order: only the identity view is compared, with a gradient
            # on every third ray each way, so that no two rays' stencils meet in a voxel and the bits are reproducible)
            g = np.zeros((1, H, W), np.float32)
            g[0, ::3, ::3] = rng.randn(*g[0, ::3, ::3].shape)
            keep("ray_14x%dx%d.bwd.l%d" % (H, W, liquid),
                 ops.rotate_render_bwd(d, rot[:1].contiguous(), rs[:1].contiguous(), cu(g), TAU, liquid))

    # ---- render_fwd / render_bwd, modes 0-3, a tie on one ray --------------------------------------------------------
    V, D, H, W = 2, 9, 7, 6
    rng = np.random.RandomState(11)
    dn = rng.rand(V, D, H, W).astype(np.float32) - 0.2
    dn[1, 2, 3, 4] = dn[1, 7, 3, 4] = 2.0
    g = cu(rng.randn(V, H, W))
    for mode in range(4):
        d = cu(dn)
        img, rs = ops.render_fwd(d, TAU, mode)
        gd, gm = ops.render_bwd(d, rs, g, TAU, mode, want_max=True)
        d2 = d.clone()
        ops.render_bwd(d2, rs, g, TAU, mode, g_d=d2)
        keep("render_2x9x7x6.m%d" % mode, img, rs, gd, gm, d2)

    # ---- render adjoint: segmented with 4 / 8 segments, out of place and in place, with the maximum ----------------------
    for D in (18, 64):
        V, H, W = 2, 5, 13
        rng = np.random.RandomState(D)
        d = cu(rng.rand(V, D, H, W) * 1.2 - 0.2)
        g = cu(rng.randn(V, H, W))
        img, rs = ops.render_fwd(d, TAU, 0)
        gd, gm = ops.render_bwd(d, rs, g, TAU, 0, want_max=True)
        d2 = d.clone()
        _, gm2 = ops.render_bwd(d2, rs, g, TAU, 0, g_d=d2, want_max=True)
        keep("render_bwd_2x%dx5x13" % D, img, rs, gd, gm, d2, gm2)

    # ---- max-normalisation, plain and loss-net-input forms, forward and adjoint --------------------------------------
    for G, n in ((1, 1), (3, 16383), (3, 16384), (1, 16387), (3, 16387)):
        rng = np.random.RandomState(1000 * G + n % 1000)
        x = rng.rand(G, n).astype(np.float32) + 0.1
        x[G - 1] *= -1.0                                                 # the last group all negative
        if n > 1:                                                        # a two-way tie at the maximum of group 0
            x[0, 5] = x[0, n - 2] = 2.0 if G > 1 else 0.5 * x[0].max()
        xt = cu(x)
        y, gmax = ops.maxnorm_fwd(xt, G)
        keep("maxnorm_%dx%d.fwd" % (G, n), y, gmax)
        keep("maxnorm_%dx%d.bwd" % (G, n), ops.maxnorm_bwd(xt, gmax, cu(rng.randn(G, n))))
        img = xt.reshape(G, 1, n)
        xi, gmax_i = ops.maxnorm_input_fwd(img, G)
        keep("maxnorm_%dx%d.input_fwd" % (G, n), xi, gmax_i)
        keep("maxnorm_%dx%d.input_bwd" % (G, n), ops.maxnorm_input_bwd(img, gmax_i, cu(rng.randn(G, 1, n, 3))))

    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print("render_bits: %d arrays, %d values -> %s" % (len(out), sum(a.size for a in out.values()), out_path))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))

"""The Winograd transform kernels (csrc/winograd.hip, winograd5.hip: F(4x4) and F(5x5), plain and pooled) on the smallest
shapes that reach each of their paths, from host-seeded numpy inputs, all outputs and the ReLU bit-cache words into one
.npz:  python tools/conv_transform_bits.py OUT.npz

Run it on two builds of the library (two checkouts, or NFS_LIB_PATH) with NFS_GEMM_TUNE=0 and compare the files with
--compare A.npz B.npz: every array must be equal as raw 32-bit words.  The schedule of the transforms (six / seven waves per
tile, or one thread per tile and channel[-pair]) is chosen once per process: run it once with the default thresholds (the
wave schedules, at these sizes) and once with NFS_W4_WAVES6_MAX=0 NFS_W5_WAVES7_MAX=0 (the thread schedules).  Used to hold
a refactor of the transforms to the parent commit's results (profiles/winograd_transform_refactor.txt)."""
import os
import sys

import numpy as np

# (B, H, W, Ci, Co); which family a shape takes is checked below from nfs_conv3x3_executed_flops
F4 = [(2, 13, 11, 256, 128), (2, 8, 8, 128, 256), (1, 12, 12, 512, 512)]      # ragged both ways; aligned; 9 tiles, two K parts
F4_POOLED = [(2, 13, 11, 256, 256), (1, 12, 12, 512, 512)]                    # odd sides floor in the pool; two K parts
F5 = [(2, 9, 14, 128, 256), (1, 10, 10, 512, 512), (1, 25, 25, 256, 512)]     # ragged; 4 tiles, two K parts; 25 tiles


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
    from neural_flow_style_amd import _lib

    out = {}

    def keep(name, t):
        a = t.detach().cpu().numpy()
        out[name] = a.view(np.uint32).copy()

    def cu(a):
        return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")

    def family(B, H, W, K, N, pooled):
        """4 or 5: from the MFMA flops the call executes (2 * 36 * T4 * K * N or 2 * 49 * T5 * K * N); never the
        single-kernel path (its channel counts are 64 / 128 both ways)"""
        assert not (K in (64, 128) and N in (64, 128))
        fl = _lib.lib().nfs_conv3x3_executed_flops(B, H, W, K, N, int(pooled))
        t4, t5 = B * ((H + 3) // 4) * ((W + 3) // 4), B * ((H + 4) // 5) * ((W + 4) // 5)
        assert 36 * t4 != 49 * t5, "the flop count cannot tell the families apart at this shape"
        return {2.0 * 36 * t4 * K * N: 4, 2.0 * 49 * t5 * K * N: 5}[fl]

    def inputs(shape, seed):
        B, H, W, Ci, Co = shape
        rng = np.random.RandomState(seed)
        x = cu(np.maximum(rng.randn(B, H, W, Ci), 0))                   # a post-ReLU activation (zeros included)
        w = cu(rng.randn(3, 3, Ci, Co) * 0.05)
        b = cu(rng.randn(Co) * 0.1)
        gy = cu(rng.randn(B, H, W, Co))
        add = cu(rng.randn(B, H, W, Ci))
        gp = cu(rng.randn(B, H // 2, W // 2, Co))
        return x, b, gy, add, gp, ops.conv3x3_pack(w, 0), ops.conv3x3_pack(w, 1)

    def bits_of(shape, pooled, dev):
        rb = ops.conv3x3_relu_bits(*shape, pooled, dev)
        assert rb is not None
        rb.zero_()
        return rb

    # ---- plain layers: forward with / without ReLU and bit cache, data gradient under three masks x three addend forms -----
    for fam, shapes in ((4, F4), (5, F5)):
        for shape in shapes:
            B, H, W, Ci, Co = shape
            assert family(B, H, W, Ci, Co, 0) == fam and family(B, H, W, Co, Ci, 0) == fam, shape
            tag = "f%d_%dx%dx%dx%dx%d" % ((fam,) + shape)
            x, b, gy, add, _, wf, wd = inputs(shape, 7 * H + Ci)
            rb = None
            for relu in (True, False):
                for cache in (False, True):
                    rb = bits_of(shape, False, x.device) if cache else None
                    keep("%s.fwd.relu%d.bits%d" % (tag, relu, cache), ops.conv3x3_fwd(x, wf, b, Co, relu, relu_bits=rb))
                    if cache:
                        keep("%s.fwd.relu%d.words" % (tag, relu), rb)
            # (rb: the cache of the last forward; the mask of x does not depend on relu)
            for mask, kw in (("bits", dict(x_in=x, relu_bits=rb)), ("float", dict(x_in=x)), ("none", dict(x_in=None))):
                keep("%s.dgrad.%s.noadd" % (tag, mask), ops.conv3x3_dgrad(gy, wd, Ci, **kw))
                keep("%s.dgrad.%s.add" % (tag, mask), ops.conv3x3_dgrad(gy, wd, Ci, addend=add, **kw))
                if mask != "none":                                       # (an addend not yet through the mask needs one)
                    keep("%s.dgrad.%s.add_unmasked" % (tag, mask),
                         ops.conv3x3_dgrad(gy, wd, Ci, addend=add, addend_unmasked=True, **kw))

    # ---- pooled layers (F(4x4) only): forward with and without the full-resolution output, both pooled data gradients -------
    for shape in F4_POOLED:
        B, H, W, Ci, Co = shape
        assert family(B, H, W, Ci, Co, 1) == 4 and family(B, H, W, Co, Ci, 1) == 4, shape
        tag = "f4pool_%dx%dx%dx%dx%d" % shape
        x, b, _, add, gp, wf, wd = inputs(shape, 11 * H + Co)
        y0, p0 = ops.conv3x3_fwd_pool(x, wf, b, Co, True)
        keep(tag + ".fwd.nobits.y", y0)
        keep(tag + ".fwd.nobits.pool", p0)
        rb = bits_of(shape, True, x.device)
        y1, p1 = ops.conv3x3_fwd_pool(x, wf, b, Co, True, relu_bits=rb)
        keep(tag + ".fwd.bits.y", y1)
        keep(tag + ".fwd.bits.pool", p1)
        keep(tag + ".fwd.bits.words", rb)
        rb2 = bits_of(shape, True, x.device)
        y2, p2 = ops.conv3x3_fwd_pool(x, wf, b, Co, True, relu_bits=rb2, want_y=False)
        assert y2 is None
        keep(tag + ".fwd.pool_only.pool", p2)
        keep(tag + ".fwd.pool_only.words", rb2)
        for name, kw in (("noadd", {}), ("add", dict(addend=add)), ("add_unmasked", dict(addend=add, addend_unmasked=True))):
            keep("%s.dgrad.pooled1.%s" % (tag, name),                    # the mask of the layer's output from the bit cache
                 ops.conv3x3_dgrad_pool(gp, None, wd, Ci, x_in=x, relu_bits=rb, hw=(H, W), **kw))
            keep("%s.dgrad.pooled2.%s" % (tag, name),                    # ... from the float output
                 ops.conv3x3_dgrad_pool(gp, y0, wd, Ci, x_in=x, **kw))

    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print("conv_transform_bits: %d arrays, %d values -> %s" % (len(out), sum(a.size for a in out.values()), out_path))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))

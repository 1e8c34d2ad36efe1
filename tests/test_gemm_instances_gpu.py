"""Every kernel instance of the batched Winograd GEMM (winograd.hip, launch_batched_gemm), one at a time.

The dispatcher picks the kernel family by shape and, within a family, the tile by timing on the live operands (the tile
tuner).  That is sound only because every tile of a family computes the identical result: the k order of a product does
not depend on the tile.  Which instance a normal run takes is whatever wins the timing on that box, so this module pins
each one in turn through the test hook nfs_gemm_force, reads back what really ran (nfs_gemm_last: after every
applicability fallback) and checks
  - within a class of instances, identical bits (conv products in both arithmetics, the Gram gradient, the grouped Gram
    gradient against the per-layer one);
  - each class against a float64 reference of the same operation;
  - the tuner's own invariants with the hook off (the trial's result = the tuned result; a graph captured before the
    shape was tuned = the eager tuned call);
  - at the end, that every instance of the table below was launched at least once.
The CPU checks at the bottom keep the table equal to the instances launch_gemm_tile can launch, and the hook out of
the package."""
import contextlib
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (variant, bm, bn, nbuf, pre): 3 split-limb rb16s (pre 0 float pack, 1 limb planes), 2 rb16, 1 register-B f32,
# 0 LDS-B f32 (nbuf 1 | 2)
RB16_TILES = [(80, 64), (80, 128), (80, 256), (48, 64), (48, 128), (48, 256), (112, 64), (112, 128), (112, 256),
              (208, 64), (208, 128)]
INSTANCES = ([(3, bm, bn, 0, pre) for bm, bn in RB16_TILES for pre in (0, 1)]
             + [(2, bm, bn, 0, 0) for bm, bn in RB16_TILES]
             + [(1, bm, bn, 0, 0) for bm in (64, 128) for bn in (64, 128)]
             + [(0, bm, bn, nbuf, 0) for bm in (64, 128) for bn in (64, 128) for nbuf in (1, 2)])
V3 = [i for i in INSTANCES if i[0] == 3]
V2 = [i for i in INSTANCES if i[0] == 2]
V1 = [i for i in INSTANCES if i[0] == 1]
V0 = [i for i in INSTANCES if i[0] == 0]
# instances whose result must be identical bits: the same MFMA and the same k order
FAMILY = {3: "split-limb 16x16x32 bf16", 2: "f32 16x16x4", 1: "f32 32x32x2", 0: "f32 32x32x2"}

_SEEN = set()          # instances recorded as launched by this module (the coverage check at the end)
_KEYS = ("variant", "bm", "bn", "nbuf", "pre", "ksplit", "T", "K", "N", "Z", "trialled")


@contextlib.contextmanager
def forced(inst):
    """every batched GEMM launch inside runs on instance ``inst``; always off again on the way out"""
    from neural_flow_style_amd import _lib
    _lib.call("nfs_gemm_force", *inst)
    try:
        yield
    finally:
        _lib.lib().nfs_gemm_force(-1, 0, 0, 0, 0)


@contextlib.contextmanager
def gemm_mode(mode):
    from neural_flow_style_amd import ops
    prev = ops.gemm_mode(mode)
    try:
        yield
    finally:
        ops.gemm_mode(prev)


def last_gemm():
    """the record of the most recent batched GEMM launch (nfs_gemm_last) as a dict"""
    from neural_flow_style_amd import _lib
    buf = (ctypes.c_longlong * 11)()
    _lib.call("nfs_gemm_last", buf)
    rec = dict(zip(_KEYS, (int(v) for v in buf)))
    inst = tuple(rec[k] for k in _KEYS[:5])
    assert inst in INSTANCES, rec
    _SEEN.add(inst)
    rec["inst"] = inst
    return rec


def _check_forced(inst, rec):
    """what ran is the forced instance, or one of the dispatcher's documented fallbacks"""
    got = rec["inst"]
    if got == inst:
        return
    v = inst[0]
    if v == 1 and got[0] == 0 and got[1:3] == inst[1:3]:
        return                           # register-B without the 32x32 fragment pack (F(5x5)) / masked: LDS-B, same tile
    if v >= 2 and got[0] == 0 and rec["N"] % inst[2]:
        return                           # N % bn != 0: the LDS-B kernel on the planner's tile
    if v <= 1 and got[0] == 0 and rec["N"] % inst[2]:
        return
    raise AssertionError("forced %s, ran %s" % (inst, rec))


# ---- conv products ---------------------------------------------------------------------------------------------------

def _unfold64(x, H, W):
    """[B,H,W,C] (device) -> float64 [B, C*9, H*W] patches of the 3x3 'same' convolution"""
    return torch.nn.functional.unfold(x.double().permute(0, 3, 1, 2), 3, padding=1)


def _conv64(x, w_oi33):
    """float64 3x3 'same' convolution on the device: x [B,H,W,Ci], w [Co,Ci,3,3] -> [B,H,W,Co]"""
    B, H, W, _ = x.shape
    y = w_oi33.reshape(w_oi33.shape[0], -1) @ _unfold64(x, H, W)
    return y.reshape(B, -1, H, W).permute(0, 2, 3, 1)


# (B, H, W, Ci, Co) -> what the shape is for, and the (Z, T, K parts) the record must show for (fwd, dgrad)
CONV_SHAPES = [
    ((1, 12, 12, 512, 512), "F(4x4), T = 9, K parts = 2", (36, 9, 2), (36, 9, 2)),
    ((8, 12, 12, 512, 512), "T = 72, conv5_1 at 8 views", (36, 72, 1), (36, 72, 1)),
    ((3, 28, 28, 256, 256), "F(4x4), T = 147", (36, 147, 1), (36, 147, 1)),
    ((2, 25, 25, 256, 512), "F(5x5), T = 50; dgrad K = 512, so K parts = 2", (49, 50, 1), (49, 50, 2)),
    ((1, 50, 50, 256, 256), "F(5x5), T = 100", (49, 100, 1), (49, 100, 1)),
    ((8, 25, 25, 512, 512), "T = 200, the headline conv4_x", (49, 200, 1), (49, 200, 1)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,why,want_fwd,want_dgrad", CONV_SHAPES, ids=[str(s[0]) for s in CONV_SHAPES])
def test_conv_gemm_instances_agree_and_are_float32_accurate(shape, why, want_fwd, want_dgrad):
    """ops.conv3x3_fwd and ops.conv3x3_dgrad (with x_in and addend) under every applicable instance, in both
    arithmetics: identical bits within a class, the unforced call equal to its class, and each class within 2x the
    unforced path's error against a float64 convolution (per element: |y - ref| / the convolution of the magnitudes, the
    measure of test_ops_gpu.py::test_split_limb_gemm_is_float32_accurate; both arithmetics land on the same float32
    floor there, within 1.5x)."""
    from neural_flow_style_amd import ops
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(((B * 97 + H) * 89 + W) * 7 + Ci + Co)
    x = torch.randn(B, H, W, Ci, generator=g).cuda()
    w = torch.randn(3, 3, Ci, Co, generator=g).cuda()
    bias = torch.randn(Co, generator=g).cuda()
    gy = torch.randn(B, H, W, Co, generator=g).cuda()
    x_in = torch.randn(B, H, W, Ci, generator=g).cuda()
    addend = torch.randn(B, H, W, Ci, generator=g).cuda()
    pk_f, pk_d = ops.conv3x3_pack(w, 0), ops.conv3x3_pack(w, 1)

    w_f = w.double().permute(3, 2, 0, 1)                      # [Co,Ci,3,3]
    w_d = w.double().flip(0, 1).permute(2, 3, 0, 1)           # [Ci,Co,3,3]: the data gradient as a 'same' conv of gy
    mask = (x_in > 0).double()
    refs = {"fwd": (_conv64(x, w_f) + bias.double(), _conv64(x.abs(), w_f.abs()) + bias.double().abs()),
            "dgrad": (_conv64(gy, w_d) * mask + addend.double(),
                      _conv64(gy.abs(), w_d.abs()) * mask + addend.double().abs())}
    run = {"fwd": lambda: ops.conv3x3_fwd(x, pk_f, bias, Co, relu=False),
           "dgrad": lambda: ops.conv3x3_dgrad(gy, pk_d, Ci, x_in=x_in, addend=addend)}
    want = {"fwd": (Ci, Co) + want_fwd, "dgrad": (Co, Ci) + want_dgrad}

    def err(y, op):
        ref, mag = refs[op]
        return float(((y.double() - ref).abs() / mag).max())

    for op in ("fwd", "dgrad"):
        K, N, Z, T, ksplit = want[op]
        cls, default, default_err = {}, [], {}
        for mode, insts in ((1, V3), (0, V2 + V1 + V0)):
            with gemm_mode(mode):
                y = run[op]()
                rec = last_gemm()
                assert (rec["Z"], rec["T"], rec["K"], rec["N"]) == (Z, T, K, N), (why, op, rec)
                default.append((FAMILY[rec["variant"]], y))
                default_err[mode] = err(y, op)
                for inst in insts:
                    with forced(inst):
                        y = run[op]()
                    rec = last_gemm()
                    _check_forced(inst, rec)
                    assert (rec["Z"], rec["T"], rec["K"], rec["N"]) == (Z, T, K, N), (why, op, inst, rec)
                    assert rec["ksplit"] == (ksplit if rec["variant"] >= 2 else 1), (why, op, inst, rec)
                    fam = FAMILY[rec["variant"]]
                    if fam not in cls:
                        cls[fam] = (rec["inst"], y)
                    else:
                        first, y0 = cls[fam]
                        assert torch.equal(y, y0), "%s %s %s: %s differs from %s (%s)" % (
                            shape, op, fam, rec["inst"], first, float((y - y0).abs().max()))
        for fam, y in default:
            assert torch.equal(y, cls[fam][1]), "%s %s: the unforced call differs from its class %s" % (shape, op, fam)
        assert max(default_err.values()) < 5e-3, (shape, op, default_err)   # (the floors of the split-limb test)
        bound = 2.0 * max(default_err.values())
        for fam, (inst, y) in cls.items():
            e = err(y, op)
            assert e <= bound, "%s %s %s (%s): float64 error %.3g, unforced %s" % (shape, op, fam, inst, e, default_err)
        assert set(cls) >= {FAMILY[3], FAMILY[2], FAMILY[0]}, (shape, op, list(cls))


# ---- the Gram gradient -----------------------------------------------------------------------------------------------

GRAM_SHAPES = [(1, 1, 128), (1, 15, 64), (3, 49, 256), (1, 81, 512), (2, 129, 256), (3, 209, 512)]   # HW one past a tile


def _symmetric(B, C, g):
    A = torch.randn(B, C, C, generator=g)
    return ((A + A.transpose(1, 2)) / 2).cuda()      # exactly symmetric: a + b == b + a in float32


@pytest.mark.gpu
@pytest.mark.parametrize("B,HW,C", GRAM_SHAPES)
def test_gram_gradient_instances_agree_and_are_float32_accurate(B, HW, C):
    """ops.gram_bwd (dF = 2 scale F D, masked by F > 0) under every variant-2 and variant-0 instance, with and without
    the mask, with the scalar scale and with scale_dev: identical bits within a class, each class within K 2^-24 of the
    sum of |terms| of a float64 product (the worst-case float32 bound: a tile bug misses it by orders of magnitude).
    Forcing the split-limb or the register-B form on this masked / scaled / symmetric launch runs 2 / 0."""
    from neural_flow_style_amd import ops
    g = torch.Generator().manual_seed(1000 * B + HW + C)
    F = torch.randn(B, HW, C, generator=g).cuda()
    D = _symmetric(B, C, g)
    sd = (torch.rand(B, generator=g) + 0.5).cuda()
    prod = F.double() @ D.double()
    mag = F.double().abs() @ D.double().abs()
    for relu_mask in (0, 1):
        m = (F > 0).double() if relu_mask else torch.ones_like(prod)
        for scale, scale_dev in ((0.375, None), (0.5, sd)):
            a = 2.0 * scale * (scale_dev.double()[:, None, None] if scale_dev is not None else 1.0)
            ref, bound = prod * a * m, mag * abs(a) * m * (C * 2.0 ** -24)
            cls = {}
            for inst in V2 + V0 + [(3, 80, 64, 0, 1), (3, 208, 128, 0, 0), (1, 64, 64, 0, 0), (1, 128, 128, 0, 0)]:
                with forced(inst):
                    y = ops.gram_bwd(F, D, scale, scale_dev=scale_dev, relu_mask=bool(relu_mask))
                rec = last_gemm()
                assert (rec["Z"], rec["T"], rec["K"], rec["N"], rec["ksplit"]) == (B, HW, C, C, 1), (inst, rec)
                if inst[0] == 3:         # split-limb on a masked / scaled / symmetric launch: the same tile in f32
                    assert rec["inst"] == (2,) + inst[1:3] + (0, 0) or (C % inst[2] and rec["variant"] == 0), (inst, rec)
                elif inst[0] == 1:       # register-B without a fragment pack of B: the LDS-B kernel
                    assert rec["variant"] == 0, (inst, rec)
                    _check_forced(inst, rec)
                else:
                    _check_forced(inst, rec)
                fam = FAMILY[rec["variant"]]
                if fam not in cls:
                    cls[fam] = (rec["inst"], y)
                    d = (y.double() - ref).abs()
                    assert bool((d <= bound).all()), "%s relu %d scale_dev %s %s: %.3g of the bound" % (
                        (B, HW, C), relu_mask, scale_dev is not None, rec["inst"], float((d / (bound + 1e-300)).max()))
                else:
                    assert torch.equal(y, cls[fam][1]), "%s relu %d: %s differs from %s" % (
                        (B, HW, C), relu_mask, rec["inst"], cls[fam][0])
            assert set(cls) == {FAMILY[2], FAMILY[0]}, list(cls)


@pytest.mark.gpu
def test_grouped_gram_gradient_equals_the_per_layer_one_bit_for_bit():
    """nfs_gram_group_bwd (all layers in one launch of the 80 x 64 16-row f32 form) against ops.gram_bwd of each layer
    on the SAME F and D under every variant-2 tile: identical bits (winograd.hip, gram_bwd_gemm_group: same per-tile
    arithmetic)"""
    from neural_flow_style_amd import _lib, ops
    g = torch.Generator().manual_seed(77)
    B = 2
    layers = [(81, 512, 1), (129, 256, 0), (209, 128, 1), (15, 64, 1)]      # (HW, C, relu_mask)
    arr = (_lib.GramLayer * len(layers))()
    keep = []
    for l, (HW, C, rm) in enumerate(layers):
        F = torch.randn(B, HW, C, generator=g).cuda()
        D = _symmetric(B, C, g)
        dF = torch.full_like(F, float("nan"))
        keep.append((F, D, dF))
        y = arr[l]
        y.F, y.Dmat, y.dF = F.data_ptr(), D.data_ptr(), dF.data_ptr()
        y.B, y.Bs, y.HW, y.C = B, B, HW, C
        y.scale, y.weight, y.relu_mask = 1.0 / (2.0 * HW * C), 1.0, rm
    _lib.call("nfs_gram_group_bwd", arr, len(layers), ops._stream())
    for (HW, C, rm), (F, D, dF), y in zip(layers, keep, arr):
        assert bool(torch.isfinite(dF).all())
        compared = 0
        for inst in V2:
            with forced(inst):
                out = ops.gram_bwd(F, D, y.scale, relu_mask=bool(rm))
            rec = last_gemm()
            if rec["variant"] != 2:
                assert C % inst[2], (inst, rec)      # (only where the tile does not divide C)
                continue
            compared += 1
            assert torch.equal(out, dF), "layer (HW %d, C %d): %s differs from the grouped launch (%.3g)" % (
                HW, C, rec["inst"], float((out - dF).abs().max()))
        assert compared >= 4, (HW, C, compared)


# ---- the tuner, hook off ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_tuner_trial_leaves_the_tuned_result(mode):
    """The first launch of a shape times every candidate and leaves the LAST candidate's result in place; the second
    runs the winner.  Both must be the same bits.  (1, 20, 36, 384, 640) is used by no other test: T = 45 rows, four
    16-row candidates (80 / 48 rows x 128 / 64 columns)."""
    from neural_flow_style_amd import ops
    B, H, W, Ci, Co = 1, 20, 36, 384, 640
    g = torch.Generator().manual_seed(5 + mode)
    x = torch.randn(B, H, W, Ci, generator=g).cuda()
    w = torch.randn(3, 3, Ci, Co, generator=g).cuda()
    pk = ops.conv3x3_pack(w, 0)
    with gemm_mode(mode):
        y1 = ops.conv3x3_fwd(x, pk, None, Co, relu=False)
        r1 = last_gemm()
        y2 = ops.conv3x3_fwd(x, pk, None, Co, relu=False)
        r2 = last_gemm()
    assert r1["trialled"] == 1, ("the first launch of a fresh shape was not tuned", r1)
    assert r2["trialled"] == 0 and r2["T"] == 45, r2
    assert torch.equal(y1, y2), (r1, r2, float((y1 - y2).abs().max()))


@pytest.mark.gpu
def test_graph_captured_before_tuning_equals_the_tuned_eager_call():
    """A conv captured into a graph before its shape was tuned runs the untrialled default tile; the eager calls after it
    run the tuned one.  Replays and eager calls must agree bit for bit.  (1, 28, 20, 384, 640): T = 35, used by no
    other test."""
    from neural_flow_style_amd import ops
    B, H, W, Ci, Co = 1, 28, 20, 384, 640
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, H, W, Ci, generator=g).cuda()
    w = torch.randn(3, 3, Ci, Co, generator=g).cuda()
    bias = torch.randn(Co, generator=g).cuda()
    pk = ops.conv3x3_pack(w, 0)
    ops.conv3x3_fwd(torch.randn(1, 8, 8, Ci).cuda(), pk, bias, Co)     # (the library's kernels loaded before capturing)
    out = torch.empty(B, H, W, Co, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.conv3x3_fwd(x, pk, bias, Co, relu=False, out=out)
    rc = last_gemm()
    assert rc["trialled"] == 0 and rc["T"] == 35, rc
    graph.replay()
    torch.cuda.synchronize()
    y_graph = out.clone()
    y_trial = ops.conv3x3_fwd(x, pk, bias, Co, relu=False)
    rt = last_gemm()
    y_tuned = ops.conv3x3_fwd(x, pk, bias, Co, relu=False)
    assert rt["trialled"] == 1, rt
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_graph, y_trial) and torch.equal(y_graph, y_tuned) and torch.equal(out, y_graph), (rc, rt)


# ---- coverage (runs last in this module) -----------------------------------------------------------------------------

@pytest.mark.gpu
def test_every_instance_was_launched():
    """every row of the instance table was recorded as launched by the tests above (run the whole module)"""
    missing = sorted(set(INSTANCES) - _SEEN)
    assert not missing, "never launched: %s" % missing


# ---- CPU checks ------------------------------------------------------------------------------------------------------

def _instance_table():
    """winograd.hip's source and the rows of its instance table kGemmInsts, in table order"""
    src = open(os.path.join(ROOT, "neural-flow-style_amd", "csrc", "winograd.hip")).read()
    m = re.search(r"\nstatic const GemmRow kGemmInsts\[\] = \{\n(.*?)\n\};\n", src, re.S)
    assert m, "kGemmInsts not found"
    rows = [tuple(int(v) for v in r) for r in re.findall(r"gemm_row<(\d+), (\d+), (\d+), (\d+), (\d+)>\(\)", m.group(1))]
    return src, rows


def test_dispatch_table_rows_are_exactly_the_instances():
    """the rows of the dispatcher's instance table (kGemmInsts: what launch_gemm_tile launches, the tuner tries and
    nfs_gemm_force accepts) are exactly INSTANCES: a new one cannot be added without coverage"""
    src, rows = _instance_table()
    assert len(rows) == len(set(rows)), "an instance listed twice"
    assert set(rows) == set(INSTANCES), (sorted(set(rows) - set(INSTANCES)), sorted(set(INSTANCES) - set(rows)))
    assert len(INSTANCES) == 45
    # both forms of B behind every split-limb tile
    for v, bm, bn, _, _ in rows:
        if v == 3:
            assert {(3, bm, bn, 0, 0), (3, bm, bn, 0, 1)} <= set(rows), (bm, bn)
    # nothing launches an instance past the table: on the host side only launch_gemm_inst (a row's launcher) names the
    # kernels of the instances
    host = src[src.index("// ---- host side"):]
    m = re.search(r"\nstatic void launch_gemm_inst\(.*?\n}\n", host, re.S)
    assert m, "launch_gemm_inst not found"
    for kernel in ("winograd_gemm_kernel<", "winograd_gemm_rb_kernel<", "winograd_gemm_rb16_kernel<",
                   "winograd_gemm_rb16s_kernel<"):
        assert host.count(kernel) == m.group(0).count(kernel) == 1, kernel


def test_gemm_force_accepts_exactly_the_instances():
    """nfs_gemm_force takes every row of the table and refuses what names no instance (no GPU needed: it only sets the
    process-wide choice)"""
    from neural_flow_style_amd import _lib
    L = _lib.lib()
    try:
        for inst in INSTANCES:
            assert L.nfs_gemm_force(*inst) == 0, inst
        for bad in [(3, 208, 256, 0, 0), (2, 208, 256, 0, 0), (2, 64, 64, 0, 0), (3, 80, 128, 0, 2), (3, 80, 128, 1, 0),
                    (0, 80, 64, 1, 0), (0, 64, 64, 0, 0), (0, 64, 64, 3, 0), (1, 64, 256, 0, 0), (1, 64, 64, 2, 0),
                    (2, 80, 128, 0, 1), (4, 64, 64, 0, 0), (-2, 64, 64, 0, 0)]:
            assert L.nfs_gemm_force(*bad) == -1, bad
    finally:
        assert L.nfs_gemm_force(-1, 0, 0, 0, 0) == 0


def test_product_never_calls_the_gemm_force_hook():
    """the hook is for tests: nothing in the package or in bench.py names nfs_gemm_force, other than its definition
    (winograd.hip); the binding reads its declaration from include/nfs_hip.h"""
    pkg = os.path.join(ROOT, "neural-flow-style_amd")
    files = [os.path.join(ROOT, "bench.py")]
    for dirpath, _, names in os.walk(pkg):
        files += [os.path.join(dirpath, f) for f in names if f.endswith((".py", ".hip", ".h", ".cpp"))]
    for path in files:
        src = open(path).read()
        if path.endswith(os.path.join("csrc", "winograd.hip")):
            continue
        assert "nfs_gemm_force" not in src, path

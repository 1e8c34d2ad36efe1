"""Every kernel path that only an environment switch reaches, held to the references of the default paths.

tests/test_conv_gpu.py closes the set of paths the launch code reaches WITHOUT an environment toggle; this module is its
complement.  The C-side switches are read once per process, so each configuration runs one battery of
tests/switch_runs.py in ONE fresh child process (never an exec; one child at a time; at most 16 in the module) and

  (a) the child exits 0,
  (b) the path really changed, by what the library itself reported (nfs_conv3x3_plan, nfs_gemm_last,
      nfs_conv3x3_relu_bits_words, nfs_gram_workspace_floats, nfs_gemm_mode),
  (c) every output lies within the per-element float64 bound tests/conv_ref.py, view_ref.py, field_ref.py and loss_ref.py
      give for the family that actually ran (exact inputs on the direct kernels must EQUAL float64),
  (d) outputs are bit-identical with this process's default-environment run wherever the source claims it.

NFS_RT_XCD and NFS_EVER_LANES select a block order / a kernel instance the library has no query for: (b) cannot be
asserted for them, only (a), (c) and (d).

If a child ends with a signal, an abort, a time limit or a GPU fault, every later test of the module fails at once and
starts no process: such an ending is a finding to be read, not to be repeated.

``pytest -s`` prints, per configuration, the paths reported and the largest err / bound.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import conv_ref as R
from tests import loss_ref as LR
from tests import switch_runs as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
_TROUBLE = []            # what ended a child badly; once set, no further process is started
_CHILDREN = []           # the configurations started (at most 16)
_OURS = [k for k, v in SR.SWITCHES.items() if v[0] == "test" and v[1].startswith(SR.GPU)]
U = R.U


# ---- children ----------------------------------------------------------------------------------------------------------------
def child(battery, env, tmp_path):
    """one fresh child process running ``battery`` under ``env`` -> (outputs, report)"""
    if _TROUBLE:
        pytest.fail("an earlier child ended in trouble (%s): no further process is started" % _TROUBLE[0])
    assert len(_CHILDREN) < 16
    _CHILDREN.append((battery, env))
    path = str(tmp_path / "out.npz")
    e = {k: v for k, v in os.environ.items() if k not in _OURS}
    e.update(env, PYTHONPATH=ROOT)
    try:
        r = subprocess.run([sys.executable, "-m", "tests.switch_runs", battery, path], cwd=ROOT, env=e, timeout=CHILD_TIMEOUT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _TROUBLE.append("%s %s: no end within %d s" % (battery, env, CHILD_TIMEOUT))
        pytest.fail(_TROUBLE[0])
    text = r.stdout[-3000:] + r.stderr[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stdout + r.stderr:
        _TROUBLE.append("%s %s: exit status %d" % (battery, env, r.returncode))
        pytest.fail(_TROUBLE[0] + "\n" + text)
    assert r.returncode == 0, text                                                      # (a)
    return SR.load(path)


@pytest.fixture(scope="module")
def ops():
    assert not [k for k in _OURS if k in os.environ], "this process must run the default environment"
    import neural_flow_style_amd.ops as ops
    return ops


@functools.lru_cache(maxsize=None)
def default_run(battery, gemm_mode=None):
    """this process's run of a battery (read only); ``gemm_mode``: under ops.gemm_mode(gemm_mode)"""
    import neural_flow_style_amd.ops as ops
    prev = ops.gemm_mode(gemm_mode) if gemm_mode is not None else None
    try:
        return SR.run(battery)
    finally:
        if prev is not None:
            ops.gemm_mode(prev)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def assert_same_bits(theirs, ours, keys, what):
    keys = list(keys)
    assert keys, what
    differ = [k for k in keys if not same_bits(theirs[k], ours[k])]
    assert not differ, "%s: %d of %d outputs differ from the default run's bits, the first: %s" % (
        what, len(differ), len(keys), differ[:6])


# ---- conv: references (float64, once per shape) and the bound of the family that ran ---------------------------------------------
def tile_of(plan):
    """the Winograd tile of a reported plan (2 | 4 | 5), 0 for the direct kernels"""
    if plan["family"] == "wg5":
        return 5
    if plan["family"] == "wg4_single":
        return 4
    if plan["family"] == "wg4_three":
        return 2 if plan["Z"] == 16 else 4
    return 0


@functools.lru_cache(maxsize=None)
def _plain_ref(shape, exact):
    d = SR.exact_inputs(shape) if exact else dict(R.layer_inputs(shape))
    x_in = d["x_in"] if exact else d["x"]
    pre, S = R.conv(d["x"], d["w"], d["bias"])
    wd = R.dgrad_filters(d["w"])
    g, Sg = R.conv(d["gy"], wd)
    if exact:
        R.exact_units(S, 3.0)
        R.exact_units(Sg, 3.0)
    mask = x_in > 0
    return dict(d=d, pre=pre, y=np.maximum(pre, 0.0), S=S, wd=wd, g=g, Sg=Sg, mask=mask,
                g_m=R.layer_dgrad(g, mask=mask, addend=d["addend"]))


@functools.lru_cache(maxsize=None)
def _aw(shape, exact, direction, m, pooled=False):
    """the magnitude part of the bound: 1.01 (K + c) u AW of F(m x m), or 1.01 (9 K + 20) u S of the direct kernels"""
    if pooled:
        d = R.layer_inputs(shape, pooled=True)
        a, f = d["x"], d["w"]
        assert direction == "fwd"
        S = None
    else:
        ref = _plain_ref(shape, exact)
        a, f = (ref["d"]["x"], ref["d"]["w"]) if direction == "fwd" else (ref["d"]["gy"], ref["wd"])
        S = ref["S"] if direction == "fwd" else ref["Sg"]
    if m == 0:
        if S is None:
            S = R.conv(a, f)[1]
        return R.direct_bound(S, a.shape[-1], 0.0)
    return R.wino_bound(a, f, m, 0.0)


def inside(what, got, ref, bound, m, worst):
    report = R.first_mismatches(got, ref, bound, m or 4)
    assert not report, "%s\n%s" % (what, report)
    worst[0] = max(worst[0], R.err_ratio(np.abs(R.f64(got) - ref), bound))


def equal(what, got, ref, m=4):
    report = R.first_mismatches(got, ref, 0.0, m)
    assert not report, "%s must equal float64\n%s" % (what, report)


def check_conv(name, out, rep, parts=("plain", "pooled", "c3")):
    """(c) for a conv battery's outputs, each against the bound of the family its own report names; returns what ran"""
    worst, ran = [0.0], set()
    for shape in SR.CONV_PLAIN if "plain" in parts else ():
        r = rep["plain"][SR.sid(shape)]
        mf, mg = tile_of(r["fwd"]), tile_of(r["dgrad"])
        ran |= {"%s Z%d" % (r["fwd"]["family"], r["fwd"]["Z"]), "%s Z%d" % (r["dgrad"]["family"], r["dgrad"]["Z"])}
        for exact in (False, True):
            tag = ("e_" if exact else "p_") + SR.sid(shape)
            if tag + "_y" not in out:
                assert exact and shape in SR.CONV_NO_EXACT
                continue
            ref = _plain_ref(shape, exact)
            what = "%s %s %s" % (name, shape, "integers" if exact else "realistic")
            for key, m, want, fam in (("_y", mf, ref["y"], r["fwd"]["family"]), ("_gx", mg, ref["g"], r["dgrad"]["family"])):
                direction = "fwd" if key == "_y" else "dgrad"
                if exact and m == 0:
                    equal("%s %s (%s)" % (what, direction, fam), out[tag + key], want)
                else:
                    inside("%s %s (%s)" % (what, direction, fam), out[tag + key], want,
                           _aw(shape, exact, direction, m) + U * np.abs(want), m, worst)
            if exact and mg == 0:
                equal(what + " masked dgrad + addend", out[tag + "_gxf"], ref["g_m"])
            else:
                inside(what + " masked dgrad + addend", out[tag + "_gxf"], ref["g_m"],
                       (_aw(shape, exact, "dgrad", mg) + U * np.abs(ref["g_m"])) * ref["mask"], mg, worst)
            if tag + "_gxb" in out:
                assert same_bits(out[tag + "_gxb"], out[tag + "_gxf"]), what + ": bit-cache and float-mask gradients differ"
    for shape in SR.CONV_POOLED if "pooled" in parts else ():
        r = rep["pooled"][SR.sid(shape)]
        tag = "q_" + SR.sid(shape)
        what = "%s %s pooled" % (name, shape)
        mf, mg = tile_of(r["fwd"]), tile_of(r["dgrad_float"])
        ran |= {"pooled %s Z%d" % (r["fwd"]["family"], r["fwd"]["Z"])}
        d = R.layer_inputs(shape, pooled=True)
        pre, _ = R.conv(d["x"], d["w"], d["bias"])
        y = np.maximum(pre, 0.0)
        by = _aw(shape, False, "fwd", mf, pooled=True) + U * np.abs(y)
        yp = R.avgpool2(y)
        inside(what + " y", out[tag + "_y"], y, by, mf, worst)
        inside(what + " y_pool", out[tag + "_yp"], yp, R.pool_bound(by, yp), 2, worst)
        und = R.undecided(pre, by)
        mk = out[tag + "_y"] > 0
        wrong = (mk != (pre > 0)) & ~und
        assert not wrong.any(), what + ": a decided ReLU mask differs"
        # the pooled gradient: only on undecided entries does the reference take the kernel's own mask
        g_y = R.pooled_gy(d["gy"], np.where(und, mk, pre > 0))
        wd = R.dgrad_filters(d["w"])
        g, Sg = R.conv(g_y, wd)
        mask = d["x"] > 0
        g_m = R.layer_dgrad(g, mask=mask, addend=d["addend"])
        bg = R.direct_bound(Sg, g_y.shape[-1], 0.0) if mg == 0 else R.wino_bound(g_y, wd, mg, 0.0)
        inside(what + " masked dgrad + addend, float output", out[tag + "_gxf"], g_m, (bg + U * np.abs(g_m)) * mask, mg, worst)
        if tag + "_gxb" in out:
            assert same_bits(out[tag + "_gxb"], out[tag + "_gxf"]), what + ": bit-cache and float-mask gradients differ"
    for bhw in SR.CONV_C3 if "c3" in parts else ():
        r = rep["c3"][SR.sid(bhw)]
        ran |= {"conv1_1 %s" % r["fwd"]["family"]}
        ref = _plain_ref(tuple(bhw) + (3, 64), True)
        equal("%s conv1_1 %s forward (%s)" % (name, bhw, r["fwd"]["family"]), out["c_%s_y" % SR.sid(bhw)], ref["y"], (8, 16))
        equal("%s conv1_1 %s gradient (%s)" % (name, bhw, r["dgrad"]["family"]), out["c_%s_gx" % SR.sid(bhw)], ref["g"],
              (14, 14))
    print("\n%-34s ran %s; largest err / bound %.5f" % (name, ", ".join(sorted(ran)), worst[0]))
    return worst[0]


def plans(rep):
    """{(shape id, direction): plan key} of a conv report"""
    out = {}
    for s, r in rep["plain"].items():
        out[s, "fwd"], out[s, "dgrad"] = R.plan_key(r["fwd"]), R.plan_key(r["dgrad"])
    for s, r in rep["pooled"].items():
        out[s, "pool fwd"], out[s, "pool dgrad bits"], out[s, "pool dgrad float"] = (
            R.plan_key(r["fwd"]), R.plan_key(r["dgrad_bits"]), R.plan_key(r["dgrad_float"]))
    return out


def keys_of(out, sids, prefixes=("p_", "e_", "q_")):
    return [k for k in out if any(k.startswith(p + s + "_") for p in prefixes for s in sids)]


def test_default_conv_battery_is_inside_its_bounds(ops):
    """this process's run, which the configurations below are compared with: the default families, as test_conv_gpu.py
    names them, each output inside its bound"""
    out, rep = default_run("conv")
    p = plans(rep)
    fams = {v.split("/")[0] for v in p.values()}
    assert fams == {"wg4_three", "wg4_single", "wg5"}, fams
    assert rep["first_gemm_mode"] == 1
    assert all(r["words"] > 0 for r in list(rep["plain"].values()) + list(rep["pooled"].values()))
    assert any(k.endswith("_gxb") for k in out)
    wrap = rep["c3"][SR.sid(SR.CONV_C3[1])]
    assert wrap["fwd"]["blocks"] < wrap["fwd"]["tiles"] and wrap["dgrad"]["blocks"] < wrap["dgrad"]["tiles"]
    check_conv("default", out, rep)


def test_winograd_tile_2(ops, tmp_path):
    """NFS_WINOGRAD_TILE=2: the F(2x2) three-kernel family.  Read before it ran (winograd.hip, vgg.hip):
      - winograd_conv sets Uq / Uq16 / Ub16 only for m == 4.  With all three null launch_batched_gemm has rows16 == false
        (it needs Uq16), gemm_rb_applies == false (it needs Uq), so the tuner tries variant 0 alone and launch_gemm_tile's
        fallback branch picks GemmInst{0, ...}: winograd_gemm_kernel, which dereferences only V, U and M.  A forced
        16-row instance falls back the same way (gemm_rb16_applies needs Uq16).
      - U is read at a.wp + 9 K N with strides (K N, 32 N, 32): what winograd_pack_kernel writes ([16][K/32][N][32]);
        winograd_packed_floats reserves 36 K N for it whatever the tile.  B rows need N % BN == 0 (pick_gemm_tile and the
        tuner both test it), A rows are guarded by m < T, M stores by m < T.
      - winograd_workspace_floats, winograd_plan and winograd_conv all take m from winograd_tile(): V is 16 T K floats,
        M follows it with 16 T N, the workspace holds 16 T (K + N ksplit) >= that.
      - winograd_input_kernel / winograd_output_kernel guard every pixel by H and W and every thread by T * C / 4.
      - takes_fused_pool is false, so the pooled calls run conv + nfs_avgpool2_fwd and nfs_avgpool2_bwd + conv, no bit
        cache is sized (words == 0) and addend_unmasked is refused; launch_conv passes no bit pointers.
    Bound: conv_ref's F(2x2) model (c2 = 12), not F(4x4)'s."""
    out, rep = child("conv", {"NFS_WINOGRAD_TILE": "2"}, tmp_path)
    for s, r in rep["plain"].items():
        for k in ("fwd", "dgrad"):
            assert (r[k]["family"], r[k]["Z"], r[k]["kparts"]) == ("wg4_three", 16, 1), (s, k, r[k])
        assert r["words"] == 0, s
        for last in (r["last_fwd"], r["last_dgrad"]):
            assert (last["Z"], last["variant"], last["ksplit"]) == (16, 0, 1), (s, last)
    for s, r in rep["pooled"].items():
        assert r["words"] == 0 and all((r[k]["family"], r[k]["Z"]) == ("wg4_three", 16) for k in ("fwd", "dgrad_bits", "dgrad_float")), (s, r)
        assert same_bits(out["q_%s_yp" % s], out["q_%s_pool_of_y" % s]), "%s: y_pool is not nfs_avgpool2_fwd(y)" % s
    assert not any(k.endswith("_gxb") for k in out)
    check_conv("NFS_WINOGRAD_TILE=2", out, rep)


def test_no_winograd(ops, tmp_path):
    """NFS_NO_WINOGRAD=1: the direct implicit GEMM with the workspace of nfs_conv3x3_workspace_floats (split-K planned by
    plan_conv from that size; the battery hands over a workspace of exactly it).  Read: takes_winograd is the only reader,
    launch_conv then requires no pooled pointers, and the pooled entry points take their unfused branches (takes_fused_pool
    implies takes_winograd).  Exact on integers, split or not."""
    out, rep = child("conv", {"NFS_NO_WINOGRAD": "1"}, tmp_path)
    p = plans(rep)
    assert {v.split("/")[0] for v in p.values()} == {"direct"}, p
    split = [k for k, v in p.items() if not v.endswith("/k1")]
    assert split, "no case splits K: %s" % p
    assert all(r["words"] == 0 for r in list(rep["plain"].values()) + list(rep["pooled"].values()))
    print("\nNFS_NO_WINOGRAD=1: %d of %d calls split K" % (len(split), len(p)))
    check_conv("NFS_NO_WINOGRAD=1", out, rep)


def test_wg5_and_fused_off(ops, tmp_path):
    """NFS_WG5=0 NFS_WG_FUSED=0: the F(5x5) and the single-kernel shapes take the three-kernel F(4x4) family.  Read:
    winograd5_takes / winograd_fused_takes return false first thing, so winograd_plan, winograd_workspace_floats (the F(4x4)
    size is always part of the maximum) and winograd_conv agree; the packs of both families are still written."""
    out, rep = child("conv", {"NFS_WG5": "0", "NFS_WG_FUSED": "0"}, tmp_path)
    ours, theirs = plans(default_run("conv")[1]), plans(rep)
    moved = [k for k, v in ours.items() if v.split("/")[0] in ("wg5", "wg4_single")]
    assert len(moved) >= 8
    assert all(theirs[k].startswith("wg4_three") for k in moved), {k: theirs[k] for k in moved}
    assert {v.split("/")[0] for v in theirs.values()} == {"wg4_three"}
    check_conv("NFS_WG5=0 NFS_WG_FUSED=0", out, rep)


def test_wg_fused_rag_off(ops, tmp_path):
    """NFS_WG_FUSED_RAG=0: ragged narrow shapes go back to three kernels, aligned ones stay on the single kernel and keep
    their bits.  Read: winograd_fused_takes is the one reader; plan, workspace and launch all go through it."""
    out, rep = child("conv", {"NFS_WG_FUSED_RAG": "0"}, tmp_path)
    dflt = default_run("conv")
    ours, theirs = plans(dflt[1]), plans(rep)
    single = [k for k, v in ours.items() if v.startswith("wg4_single")]
    ragged = [k for k in single if "/ragged/" in ours[k]]
    assert ragged and len(single) > len(ragged)
    for k in single:
        assert theirs[k].startswith("wg4_three" if k in ragged else "wg4_single"), (k, theirs[k])
    unchanged = sorted({s for s, _ in ours if all(theirs[k] == ours[k] for k in ours if k[0] == s)})
    assert SR.sid((4, 64, 64, 128, 128)) in unchanged and SR.sid((3, 9, 7, 64, 64)) not in unchanged
    assert_same_bits(out, dflt[0], keys_of(out, unchanged), "NFS_WG_FUSED_RAG=0, shapes whose plan did not change")
    check_conv("NFS_WG_FUSED_RAG=0", out, rep)


def test_no_pool_fusion(ops, tmp_path):
    """NFS_NO_POOL_FUSION=1: the pooled entry points run the plain convolution and the separate pool kernels; no layer keeps
    a bit cache (takes_fused_pool sizes it).  y_pool is bit for bit nfs_avgpool2_fwd of the y of the same call, and y that of
    the unpooled call.  Read: nfs_conv3x3_dgrad_pool's unfused branch needs workspace >= B H W Co and hands the convolution
    the rest, whichever family then fits."""
    out, rep = child("conv", {"NFS_NO_POOL_FUSION": "1"}, tmp_path)
    for s, r in rep["pooled"].items():
        assert r["words"] == 0, s
        assert same_bits(out["q_%s_yp" % s], out["q_%s_pool_of_y" % s]), "%s: y_pool is not nfs_avgpool2_fwd(y)" % s
        assert same_bits(out["q_%s_y" % s], out["q_%s_y_plain" % s]), "%s: y differs from the unpooled call's" % s
    assert plans(rep) != plans(default_run("conv")[1])          # (the float-mask gradient's own schedule is gone)
    check_conv("NFS_NO_POOL_FUSION=1", out, rep)


def test_no_relu_bits(ops, tmp_path):
    """NFS_NO_RELU_BITS=1: nfs_conv3x3_relu_bits_words returns 0 everywhere, so every call masks from the float tensors:
    bit-identical to this process's float-mask forms (and recording a cache does not change y)"""
    out, rep = child("conv", {"NFS_NO_RELU_BITS": "1"}, tmp_path)
    assert all(r["words"] == 0 for r in list(rep["plain"].values()) + list(rep["pooled"].values()))
    assert not any(k.endswith("_gxb") for k in out)
    assert plans(rep) == plans(default_run("conv")[1])
    assert_same_bits(out, default_run("conv")[0], out.keys(), "NFS_NO_RELU_BITS=1")
    check_conv("NFS_NO_RELU_BITS=1", out, rep)


def test_c3_old(ops, tmp_path):
    """NFS_C3_OLD=1: conv1_1 on the generic three-channel kernels at Co = 64 too.  Read: c3_old() guards the MFMA branch in
    the plan, the forward and the gradient alike; the generic kernels take 27 Co floats of LDS (6.9 KB at Co = 64).
    Exact on integers."""
    out, rep = child("c3", {"NFS_C3_OLD": "1"}, tmp_path)
    for s, r in rep["c3"].items():
        assert r["fwd"]["family"] == "c3_generic" and r["dgrad"]["family"] == "c3_generic", (s, r)
    check_conv("NFS_C3_OLD=1", out, rep, parts=("c3",))


@pytest.mark.parametrize("per_cu", [0, 1])
def test_c3_blocks(ops, tmp_path, per_cu):
    """NFS_C3F_BLOCKS / NFS_C3D_BLOCKS = 0: one block per tile; = 1: 256 blocks walk the 1080 / 720 tiles of the wrapping
    shape.  The same tiles, walked by other blocks: bit-identical to the default (4 and 2 per CU).  Read: c3_grid bounds
    blocks by ntiles and the kernels stride their tile walk by gridDim.x; a negative value is clamped to 0 on the host
    (tests/test_switches_cpu.py holds the clamp through the plan query)."""
    out, rep = child("c3", {"NFS_C3F_BLOCKS": str(per_cu), "NFS_C3D_BLOCKS": str(per_cu)}, tmp_path)
    for s, r in rep["c3"].items():
        for k in ("fwd", "dgrad"):
            assert r[k]["family"] == "c3_mfma"
            assert r[k]["blocks"] == (r[k]["tiles"] if per_cu == 0 else min(256, r[k]["tiles"])), (s, k, r[k])
    wrap = rep["c3"][SR.sid(SR.CONV_C3[1])]
    if per_cu:
        assert wrap["fwd"]["blocks"] == 256 < wrap["fwd"]["tiles"] and wrap["dgrad"]["blocks"] == 256 < wrap["dgrad"]["tiles"]
    assert_same_bits(out, default_run("conv")[0], out.keys(), "NFS_C3*_BLOCKS=%d" % per_cu)
    check_conv("NFS_C3F/D_BLOCKS=%d" % per_cu, out, rep, parts=("c3",))


def test_winograd_min_ch_128(ops, tmp_path):
    """NFS_WINOGRAD_MIN_CH=128: layers with a 64-channel side run the direct kernel (exact on integers), the others keep
    their plan and their bits.  Read: winograd_eligible is used by the packed size, the pack, the workspace size and
    takes_winograd alike; values below 64 are clamped to 64 on the host."""
    out, rep = child("conv", {"NFS_WINOGRAD_MIN_CH": "128"}, tmp_path)
    dflt = default_run("conv")
    ours, theirs = plans(dflt[1]), plans(rep)
    narrow = {SR.sid(s) for s in SR.CONV_PLAIN if 64 in s[3:]}
    assert len(narrow) == 2
    for k in ours:
        if k[0] in narrow:
            assert theirs[k].startswith("direct"), (k, theirs[k])
        else:
            assert theirs[k] == ours[k], (k, theirs[k], ours[k])
    assert_same_bits(out, dflt[0], keys_of(out, sorted({s for s, _ in ours} - narrow)), "NFS_WINOGRAD_MIN_CH=128, wide layers")
    check_conv("NFS_WINOGRAD_MIN_CH=128", out, rep)


def test_gemm_mode_0_from_the_environment(ops, tmp_path):
    """NFS_GEMM_MODE=0 presets what nfs_gemm_mode(0) sets: the child's first query returns 0 and its conv battery is
    bit-identical to this process's run under ops.gemm_mode(0)"""
    out, rep = child("conv", {"NFS_GEMM_MODE": "0"}, tmp_path)
    assert rep["first_gemm_mode"] == 0 and rep["gemm_mode"] == 0
    ours, orep = default_run("conv", 0)
    assert orep["gemm_mode"] == 0 and ops.gemm_mode() == 1
    batched = [r["last_fwd"]["variant"] for r in rep["plain"].values() if r["fwd"]["family"] in ("wg4_three", "wg5")]
    assert batched and all(v != 3 for v in batched), batched            # (no split-limb launch)
    assert any(r["last_fwd"]["variant"] == 3 for r in default_run("conv")[1]["plain"].values())
    assert_same_bits(out, ours, out.keys(), "NFS_GEMM_MODE=0")
    check_conv("NFS_GEMM_MODE=0", out, rep)


# ---- rotate ------------------------------------------------------------------------------------------------------------------
def test_default_rotate_battery_is_inside_its_bounds(ops):
    """this process's run of the rotate battery, voxel by voxel against tests/view_ref.py (the bounds of
    tests/test_view_path_gpu.py): the tiled adjoint, overwrite and accumulate, and the coefficient form where the shape
    has one.  The NFS_RT_XCD runs must then only reproduce these bits."""
    from tests import view_ref as VR
    out, rep = default_run("rotate")
    assert rep["coef"], "no shape of the battery takes the coefficient form"
    worst = 0.0

    def ratio(name, got, ref, bound):
        r = VR.err_ratio((torch.tensor(got, device="cuda").double() - ref).abs(), bound)
        assert r <= 1.0, (name, r)
        return r

    for shape in SR.ROT_SHAPES:
        for kind in SR.ROT_VIEWS:
            c = SR.rot_inputs(shape, kind)
            tag = "%s_%s" % (SR.sid(shape), kind)
            Rm = torch.tensor(c["R"], device="cuda")
            g, init = torch.tensor(c["g"], device="cuda"), torch.tensor(c["init"], device="cuda").double()

            def scatter(fields, errs=None):
                acc = None
                for v in range(Rm.shape[0]):
                    acc = VR.add_scatters(acc, VR.Stencil(Rm[v], shape).scatter(fields[v], None if errs is None else errs[v]))
                return acc

            sc = scatter(g.double())
            q = VR.fixed_point_quantum(float(g.abs().max()), Rm, shape)
            worst = max(worst, ratio(tag + " tiled", out[tag + "_w"][..., 0], sc["ref"], VR.adjoint_bound(sc, False, q)),
                        ratio(tag + " tiled +=", out[tag + "_acc"][..., 0], sc["ref"] + init,
                              VR.adjoint_bound(sc, False, q, init=init)))
            if tag in rep["coef"]:
                _, seg_len = ops.render_coef_layout(Rm.shape[0], *shape)
                u, ab = (torch.tensor(out["%s_coef_%s" % (tag, k)], device="cuda").double() for k in ("u", "ab"))
                pairs = [VR.coef_grad(u[v], ab[v], seg_len) for v in range(Rm.shape[0])]
                acc = scatter([p[0] for p in pairs], [p[1] for p in pairs])
                q = VR.fixed_point_quantum(float(out[tag + "_coef_bounds"].max()), Rm, shape)
                worst = max(worst, ratio(tag + " coef", out[tag + "_coef_w"], acc["ref"], VR.adjoint_bound(acc, False, q)),
                            ratio(tag + " coef +=", out[tag + "_coef_acc"], acc["ref"] + init,
                                  VR.adjoint_bound(acc, False, q, init=init)))
    print("\nrotate battery, default order: %d outputs, coefficient form on %s; largest err / bound %.3g" % (
        len(out), rep["coef"], worst))


@pytest.mark.parametrize("order", [1, 2])
def test_rt_xcd(ops, tmp_path, order):
    """NFS_RT_XCD=1 | 2: every XCD owns a contiguous range of (z, y) tile columns.  Read (rotate_bwd_tiled_kernel,
    rotate_bwd_tiled_launch): the grid is 8 ceil(cols / 8) tiles_x blocks; block b is XCD b % 8, item b / 8; XCD x owns
    columns [x cpx, x cpx + nc), nc = min(cpx, cols - x cpx), and returns -- the whole block, before any barrier -- when
    nc <= 0 or item >= nc tiles_x; item -> (x tile, column) is a bijection onto nc x tiles_x, and the x-border-first
    reordering is a permutation of 0 .. tiles_x - 1 (tiles_x == 1: the identity).  So every tile is taken exactly once.
    The live-mask launch ignores the order.  A value outside 0 .. 2 is the default order (host clamp).  The sums are
    64-bit fixed point, which does not depend on the order (warp.hip, above absmax_kernel): bit-identical to the default,
    which test_default_rotate_battery_is_inside_its_bounds holds to the float64 bounds.  (29, 43, 35) has 12 columns of
    two x tiles: two XCDs own nothing, the others two columns.  The library reports nothing about the order it took."""
    out, rep = child("rotate", {"NFS_RT_XCD": str(order)}, tmp_path)
    ours, orep = default_run("rotate")
    assert rep["coef"] == orep["coef"] and sorted(out) == sorted(ours)
    assert_same_bits(out, ours, out.keys(), "NFS_RT_XCD=%d" % order)
    print("\nNFS_RT_XCD=%d: %d outputs bit-identical to the default order" % (order, len(out)))


# ---- ever --------------------------------------------------------------------------------------------------------------------
def test_ever_lanes_off(ops, tmp_path):
    """NFS_EVER_LANES=0: advect1_kernel<2, true> (waves skipped, no per-lane predication) where the default runs
    advect1_kernel<2, true, true>.  Read (advect1_launch): only the kernel instance changes, grid and arguments are the
    same, and <2, true> is the instance every call without an ever mask already runs.  Bit-identical to the default on
    vel, m, v, adv_next and both masks over three steps; in this process the ever run also equals the run without the
    mask, which tests/test_field_gpu.py holds to field_ref."""
    out, _ = child("ever", {"NFS_EVER_LANES": "0"}, tmp_path)
    ours, _ = default_run("ever")
    assert sorted(out) == sorted(ours) and any(k.endswith("_ever") for k in out)
    assert_same_bits(out, ours, out.keys(), "NFS_EVER_LANES=0")
    for k in ours:                                        # keys: <shape>_<kind>_<ever on>_<step>_<what>
        case, ever_on, step, what = k.rsplit("_", 3)
        if ever_on == "1" and what != "ever":
            assert same_bits(ours[k], ours["%s_0_%s_%s" % (case, step, what)]), k
    moved = [k for k in ours if k.endswith("_2_vel") and not same_bits(ours[k], ours[k.replace("_2_vel", "_0_vel")])]
    assert moved, "no velocity moved between the steps"
    print("\nNFS_EVER_LANES=0: %d outputs bit-identical to the default; %d runs move the velocity" % (len(out), len(moved)))


# ---- gram --------------------------------------------------------------------------------------------------------------------
def nslab(shape, ws):
    B, HW, C = shape
    npair = (C // 64) * (C // 64 + 1) // 2
    q, r = divmod(ws - 16384, B * npair * 4096)
    assert r == 0 and q >= 1, (shape, ws)
    return q


@functools.lru_cache(maxsize=None)
def _gram_ref(shape):
    c = SR.gram_inputs(shape)
    G, mag = LR.gram(c["F"], c["scale"])
    return c, G, mag, LR.gram_bwd(c["F"], c["D"], c["scale"], relu_mask=True)


def check_gram(name, out, rep):
    worst = 0.0

    def ratio(what, got, ref, bound):
        r = LR.err_ratio(np.abs(np.asarray(got, np.float64) - ref), bound)
        assert r <= 1.0, (name, what, r)
        return r

    slabs = {}
    for shape in SR.GRAM_SHAPES:
        tag = SR.sid(shape)
        c, G, mag, (dF, bdF) = _gram_ref(shape)
        n = slabs[tag] = nslab(shape, rep["ws"][tag])
        bG = LR.gram_bound(mag, shape[1], n)
        loss, D = LR.style_loss(G, c["Gs"], c["w"])
        bD, bL = LR.style_bounds(G, c["Gs"], c["w"], bG, 32)
        worst = max(worst, ratio(tag + " G", out[tag + "_G"], G, bG), ratio(tag + " Dmat", out[tag + "_Dm"], D, bD),
                    ratio(tag + " loss", out[tag + "_loss"], loss, bL), ratio(tag + " dF", out[tag + "_dF"], dF, bdF))
        assert np.array_equal(out[tag + "_Gx"].astype(np.float64), c["exact"]["G"]), "%s %s: G on integers != float64" % (name, tag)
    layers = SR.gram_group_inputs()
    B = layers[0]["F"].shape[0]
    P = out["group_parts"].shape[0]
    want, slack = np.zeros(B), np.zeros(B)
    for l, y in enumerate(layers):
        G, mag = LR.gram(y["F"], y["s"])
        chunks = (y["HW"] + 31) // 32
        bG = LR.gram_bound(mag, y["HW"], (chunks + 15) // 16 if chunks > 32 else 1)
        loss, D = LR.style_loss(G, y["Gs"], y["w"])
        bD, bL = LR.style_bounds(G, y["Gs"], y["w"], bG, P)
        dF, bdF = LR.gram_bwd(y["F"], D, y["s"], relu_mask=True)
        # (D's own bound reaches dF through 2 s |F|)
        bdF = bdF + 2.0 * y["s"] * np.matmul(np.abs(LR.f64(y["F"])), bD) * (y["F"] > 0)
        worst = max(worst, ratio("group G %d" % l, out["group_%d_G" % l], G, bG),
                    ratio("group dF %d" % l, out["group_%d_dF" % l], dF, bdF))
        want, slack = want + loss, slack + bL
    worst = max(worst, ratio("group loss", out["group_parts"].astype(np.float64).sum(0), want, slack))
    print("\n%-20s slabs %s; largest err / bound %.3g" % (name, slabs, worst))
    return slabs


def test_default_gram_battery_is_inside_its_bounds(ops):
    """one slab, several slabs, and a pixel count that is no multiple of the chunk, as the battery is meant to have"""
    out, rep = default_run("gram")
    slabs = check_gram("gram default", out, rep)
    assert slabs[SR.sid((8, 144, 512))] == 1 and slabs[SR.sid((3, 5003, 64))] > 1 and slabs[SR.sid((1, 1000, 128))] > 1


@pytest.mark.parametrize("cps", [4, 16])
def test_gram_cps(ops, tmp_path, cps):
    """NFS_GRAM_CPS=4 | 16 chunks of 32 pixels per slab.  Read (gram_plan): cps is capped at the image's chunks and the
    reduce fan-in bound of 256 slabs is applied AFTER the override (a small value on a long image cannot pass it:
    tests/test_switches_cpu.py); nfs_gram_workspace_floats and nfs_gram_fwd both call gram_plan, and the
    kernels take cps / nslab from the same GramArgs.  The workspace size must be the one the override implies, and differ
    from the default's where the slab count does; the forward stays inside loss_ref's bound for that slab count (and equal
    to float64 on integers); gram_bwd and the grouped chain do not read the switch: bit-identical."""
    out, rep = child("gram", {"NFS_GRAM_CPS": str(cps)}, tmp_path)
    ours, orep = default_run("gram")
    slabs = check_gram("NFS_GRAM_CPS=%d" % cps, out, rep)
    changed = 0
    for shape in SR.GRAM_SHAPES:
        tag, chunks = SR.sid(shape), (shape[1] + 31) // 32
        assert slabs[tag] == -(-chunks // min(cps, chunks)), (tag, slabs[tag])
        was = nslab(shape, orep["ws"][tag])
        assert (rep["ws"][tag] != orep["ws"][tag]) == (slabs[tag] != was)
        changed += slabs[tag] != was
    assert changed, "the override changed no plan"
    assert_same_bits(out, ours, [k for k in out if k.endswith("_dF") or k.startswith("group_")], "NFS_GRAM_CPS=%d" % cps)


# ---- the python-side switches ----------------------------------------------------------------------------------------------------
LAYERS3 = ["conv1_1", "conv2_1", "conv3_1"]
PY_SWITCHES = ["NFS_FUSE_ADAM", "NFS_FUSE_INPUT", "NFS_GRAM_GROUP", "NFS_GRAM_TOP_INLINE", "NFS_NO_DEFER_MASK",
               "NFS_RENDER_COEF", "NFS_HIST_WIDE"]


@functools.lru_cache(maxsize=None)
def _oracle():
    """the smoke case (24^3, two views, conv1_1..conv3_1) and the torch-autograd oracle's losses and gradient of it"""
    from oracle import nfs_oracle as O
    from tests.test_engine_gpu import _setup
    d0, vel0, mats, loss, cfg, w_or, sfe, T, eng = _setup(24, 2, LAYERS3)
    # the style image _setup drew (it does not hand it back): the same generator, the same draws
    from neural_flow_style_amd.synthetic import blob_density, style_image
    rng = np.random.RandomState(123)
    assert np.array_equal(blob_density(24, rng), d0)
    rng.randn(24, 24, 24, 3)
    simg = style_image(24, 24, rng)
    v = torch.tensor(vel0)[None].requires_grad_()
    total, per_view, _ = O.grid_forward(torch.tensor(d0)[None, ..., None], v, torch.tensor(np.asarray(mats, np.float32)),
                                        cfg, w_or, sfe)
    (g_o,) = torch.autograd.grad(total, v)
    return d0, vel0, mats, loss.net, T, eng, torch.stack(per_view).detach(), g_o[0], simg


def _py_run(monkeypatch, env, hist, hist_wide=True):
    """gradient() and three eager steps of the smoke stylizer built under ``env`` -> the stylizer's record"""
    import neural_flow_style_amd.ops as ops
    from neural_flow_style_amd import _lib
    d0, vel0, mats, net, T, eng, _, _, simg = _oracle()
    with monkeypatch.context() as mp:
        for k in PY_SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        mp.setattr(ops, "_HIST_WIDE", hist_wide)
        seen = dict(input_fused=0, grouped=0, masks=[], coef=0, entry=[], gram_side=[])
        for name, key in (("maxnorm_input_fwd", "input_fused"), ("gram_style_group", "grouped"), ("rotate_render_fwd_coef", "coef")):
            def spy(*a, _f=getattr(ops, name), _k=key, **kw):
                seen[_k] += 1
                if _k == "grouped":
                    seen["masks"].append(list(a[3]))
                return _f(*a, **kw)
            mp.setattr(ops, name, spy)

        def call(name, *a, _f=_lib.call, **kw):
            seen["entry"].append(name)
            return _f(name, *a, **kw)
        mp.setattr(_lib, "call", call)
        kw = dict(w_hist=0.3, hist_layer=["conv2_1"], w_hist_layer=[1.0]) if hist else {}
        loss = eng.RenderStyleLoss(net, LAYERS3, [1.0] * 3, 1.0, transmit=0.05, **kw)
        loss.set_style_image(simg)
        if hist:
            loss.set_hist_image(simg)
        main = torch.cuda.current_stream()
        job = loss._gram_job

        def gram_job(name, *a, **kw):
            seen["gram_side"].append((name, torch.cuda.current_stream() != main))
            return job(name, *a, **kw)
        mp.setattr(loss, "_gram_job", gram_job)
        rot = T.rot_to_device(mats, "cuda")
        gs = eng.GridStylizer(loss, torch.tensor(d0).cuda(), k=3, target="v", lr=1e-3, graph=False)
        gs.var.copy_(torch.tensor(vel0))
        losses, g = gs.gradient(rot)
        rec = dict(losses=losses.clone(), g=g.clone(), fuse_adam=gs.fuse_adam, grouped=loss.gram_grouped, seen=seen)
        rec["steps"] = [float(gs.step(rot)) for _ in range(3)]
        rec.update(var=gs.var.clone(), m=gs.adam.m.clone(), v=gs.adam.v.clone())
        torch.cuda.synchronize()
    return rec


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("switch", PY_SWITCHES)
def test_python_side_switch(ops, monkeypatch, switch):
    """gradient() and three eager steps of the 24^3, two-view, conv1_1..conv3_1 smoke stylizer with the switch and
    without (NFS_GRAM_TOP_INLINE with NFS_GRAM_GROUP=0 in both, where it is read; NFS_HIST_WIDE with a histogram term on
    conv2_1, through ops._HIST_WIDE since it is read at import).  First: the switch changed what ran.  Then
      NFS_HIST_WIDE   the gradient of the pixel-parallel form is claimed bit-identical to the per-channel kernel's
                      (docs/kernels/gram_losses.md): gradient(), variable, m and v equal bit for bit; the total is summed in
                      another order, so the losses are held to the bar of the histogram term's parity test (1e-4);
      NFS_FUSE_ADAM   reaches step() only; held to the bar of test_engine_gpu.py::
                      test_fused_advect_adam_equals_separate_kernels (1e-6), the compiler contracting ApplyAdam differently
                      in the two kernels;
      the others      no claim of equal bits in the header or the docs (nfs_hip.h says "to float32 rounding" of the fused
                      input): gradient() of both runs against the torch-autograd oracle chain within the bars of
                      check_gradient_parity_with_the_oracle_chain (losses 1e-4, gradient 1e-3) and against each other
                      within twice that.  Whether the bits happened to be equal is printed."""
    hist = switch == "NFS_HIST_WIDE"
    base_env = {"NFS_GRAM_GROUP": "0"} if switch == "NFS_GRAM_TOP_INLINE" else {}
    value = "1" if switch == "NFS_NO_DEFER_MASK" else "0"
    a = _py_run(monkeypatch, base_env, hist)
    b = _py_run(monkeypatch, dict(base_env, **({} if hist else {switch: value})), hist, hist_wide=not hist)
    sa, sb = a["seen"], b["seen"]
    if switch == "NFS_FUSE_ADAM":
        assert a["fuse_adam"] and not b["fuse_adam"]
        assert any(n.startswith("nfs_advect_bwd_adam") for n in sa["entry"]) and "nfs_adam_tf_step" in sb["entry"]
        assert not any(n.startswith("nfs_advect_bwd_adam") for n in sb["entry"])
    elif switch == "NFS_FUSE_INPUT":
        assert sa["input_fused"] > 0 and sb["input_fused"] == 0
    elif switch == "NFS_GRAM_GROUP":
        assert a["grouped"] and sa["grouped"] > 0 and not b["grouped"] and sb["grouped"] == 0
    elif switch == "NFS_GRAM_TOP_INLINE":
        assert ("conv3_1", False) in sa["gram_side"] and ("conv3_1", True) not in sa["gram_side"]
        assert ("conv3_1", True) in sb["gram_side"] and ("conv3_1", False) not in sb["gram_side"]
    elif switch == "NFS_NO_DEFER_MASK":
        assert any(not all(m) for m in sa["masks"]), "the default defers no mask here"
        assert sb["masks"] and all(all(m) for m in sb["masks"])
    elif switch == "NFS_RENDER_COEF":
        assert sa["coef"] > 0 and sb["coef"] == 0
    else:
        assert "nfs_hist_loss_wide" in sa["entry"] and "nfs_hist_loss" not in sa["entry"]
        assert "nfs_hist_loss" in sb["entry"] and "nfs_hist_loss_wide" not in sb["entry"]
    same = {k: torch.equal(a[k], b[k]) for k in ("var", "m", "v", "g", "losses")}
    same["step losses"] = a["steps"] == b["steps"]
    print("\n%s, bit-identical with and without: %s" % (switch, same))
    if hist:
        # the claim is about the gradient (the total is summed in another order): gradient, variable, m, v bit for bit,
        # the losses within the bar the histogram term is held to against the oracle (test_engine_gpu.py: 1e-4)
        print("  losses rel %.2e, step losses %s / %s" % (_rel(b["losses"], a["losses"]), a["steps"], b["steps"]))
        assert same["g"] and same["var"] and same["m"] and same["v"], same
        assert _rel(b["losses"], a["losses"]) < 1e-4
        np.testing.assert_allclose(a["steps"], b["steps"], rtol=1e-4)
        return
    if switch == "NFS_FUSE_ADAM":
        np.testing.assert_allclose(a["steps"], b["steps"], rtol=1e-6)
        for k in ("var", "m", "v"):
            assert _rel(a[k], b[k]) < 1e-6, k
        return
    per_view, g_o = _oracle()[6:8]
    for tag, r in (("default", a), (switch, b)):
        el, eg = _rel(r["losses"], per_view), _rel(r["g"], g_o)
        print("  %-22s losses rel %.2e, gradient rel %.2e against the oracle" % (tag, el, eg))
        assert el < 1e-4 and eg < 1e-3, (tag, el, eg)
    assert _rel(b["losses"], a["losses"]) < 2e-4 and _rel(b["g"], a["g"]) < 2e-3


_PACK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from neural_flow_style_amd import engine, vgg
from neural_flow_style_amd import synthetic as S, transform as T
world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("gloo")
D = 24
rng = np.random.RandomState(5)
d0 = S.blob_density(D, rng); vel = S.curl_velocity(D, rng, max_cells=1.0); simg = S.style_image(D, D, rng)
net = vgg.VGG(vgg.synthetic_weights(123, upto="conv2_1"), dev)
loss = engine.RenderStyleLoss(net, ["conv1_1", "conv2_1"], [1.0] * 2, 1.0, transmit=0.02)
loss.set_style_image(simg)
gs = engine.GridStylizer(loss, torch.tensor(d0, device=dev), k=3, target="v", lr=1e-3, process_group=dist.group.WORLD,
                         graph=False)
assert gs.slab is not None
gs.var.copy_(torch.tensor(vel))
rot = T.rot_to_device(S.uniform_views(4), dev)[rank::world].contiguous()
ls = [float(gs.step(rot)) for _ in range(3)]
var = gs.gather_variable()
if rank == 0:
    np.savez(sys.argv[1], l=np.asarray(ls), var=var.cpu().numpy(), pack=gs.slab.pack.cpu().numpy())
dist.barrier(); dist.destroy_process_group()
"""


def test_slab_pack_torch_equals_the_copy_kernel(ops, tmp_path):
    """NFS_SLAB_PACK=torch: the gather by index table the copy kernel replaced (test_slab_pack_is_the_index_table_gather
    says the two are the same gather).  Two gloo ranks on one GPU, three slab-sharded steps each way: the packed chunks of
    the last step, the variable and the losses are bit-identical."""
    from tests.ranks import require_gpus_for, run_ranks
    if _TROUBLE:
        pytest.fail("an earlier child ended in trouble (%s): no further process is started" % _TROUBLE[0])
    require_gpus_for(2)
    script = tmp_path / "rank.py"
    script.write_text(_PACK_SCRIPT % {"root": ROOT})
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NFS_SLAB_SHARD", "NFS_SLAB_PACK")}
    env.update(PYTHONPATH=ROOT)
    res = []
    for tag, extra in (("kernel", {}), ("torch", {"NFS_SLAB_PACK": "torch"})):
        path = tmp_path / (tag + ".npz")
        run_ranks([sys.executable, str(script), str(path)], 2, dict(env, **extra), timeout=CHILD_TIMEOUT)
        res.append(np.load(path))
    a, b = res
    assert np.abs(a["pack"]).max() > 0 and np.abs(a["var"]).max() > 0
    assert same_bits(a["pack"], b["pack"]) and same_bits(a["var"], b["var"]) and a["l"].tolist() == b["l"].tolist()
    print("\nNFS_SLAB_PACK=torch: pack, variable and losses of three steps bit-identical to the copy kernel's")

"""The unrolled K loop of the split-limb Winograd GEMM (winograd.hip, winograd_gemm_rb16s_kernel<MT16, NW16, PRE, NCH>)
against the rolled one.

A launch whose K part has 4, 8 or 16 chunks of 32 runs the instance with that chunk count as a compile-time constant
(NCH: the K loop written out, no tail prefetch); every other chunk count, and every launch of a process started with
NFS_RB16S_UNROLL=0, runs the rolled loop (NCH = 0).  The two forms do the same arithmetic in the same order, so they
must agree bit for bit.  The switch is read once per process, like the kernel's other ablation switches, so the rolled
results come from ONE child process (this file run as a script), started once for the whole module; the parent computes
the unrolled ones.  Each case drives the conv C-ABI (ops.conv3x3_fwd / conv3x3_dgrad) with the split-limb instance
pinned through the test hook nfs_gemm_force(3, bm, bn, 0, pre) and reads back what ran (nfs_gemm_last).

The forward case is a conv Ci -> 128 (K = Ci), the data gradient that of a conv 128 -> Ci (K = Ci as well), so both run
every chunk count; N = 128 either way, one 128-column block."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW = 128
TILES = [(48, 128), (80, 128)]

# (B, H, W, Ci) -> (Winograd components Z, GEMM rows T, K parts, chunks per part, what the case is for).  F(5x5) tiles
# (Z = 49) unless it says F(4x4) (Z = 36).  Rows: 16-row tiles `live` in the last block of 48 / 80 rows.
CASES = {
    (1, 45, 45, 128): (49, 81, 1, 4, "NCH 4; T = 81: a full block beside a ragged one (48: live 3, 80: live 1)"),
    (1, 45, 45, 256): (49, 81, 1, 8, "NCH 8"),
    (1, 45, 45, 512): (49, 81, 1, 16, "NCH 16"),
    (5, 10, 10, 512): (49, 20, 2, 8, "T <= 64 and K = 512: two K parts of 8 chunks"),
    (1, 45, 45, 192): (49, 81, 1, 6, "6 chunks: no unrolled instance, the rolled loop in both processes"),
    (1, 45, 45, 384): (49, 81, 1, 12, "12 chunks: the rolled loop in both processes"),
    (1, 5, 5, 256): (49, 1, 1, 8, "T = 1: live 1"),
    (5, 10, 10, 256): (49, 20, 1, 8, "T = 20: live 2"),
    (1, 30, 30, 256): (49, 36, 1, 8, "T = 36: live 3 of 80 rows, a full block of 48"),
    (1, 35, 35, 256): (49, 49, 1, 8, "T = 49: live 4 of 80 rows; 48: a full block and live 1"),
    (2, 14, 11, 256): (36, 24, 1, 8, "F(4x4), sides 14 and 11 (no multiples of 4): T = 24"),
}
_KEYS = ("variant", "bm", "bn", "nbuf", "pre", "ksplit", "T", "K", "N", "Z", "trialled")


def _last_gemm():
    from neural_flow_style_amd import _lib
    buf = (ctypes.c_longlong * 11)()
    _lib.call("nfs_gemm_last", buf)
    return dict(zip(_KEYS, (int(v) for v in buf)))


def _inputs(case):
    B, H, W, Ci = case
    g = torch.Generator().manual_seed(((B * 97 + H) * 89 + W) * 7 + Ci)
    return {"x": torch.randn(B, H, W, Ci, generator=g).cuda(),
            "w_f": torch.randn(3, 3, Ci, NARROW, generator=g).cuda(),            # the forward conv Ci -> 128
            "bias": torch.randn(NARROW, generator=g).cuda(),
            "gy": torch.randn(B, H, W, Ci, generator=g).cuda(),                   # the gradient at the output of 128 -> Ci
            "w_d": torch.randn(3, 3, NARROW, Ci, generator=g).cuda(),
            "x_in": torch.randn(B, H, W, NARROW, generator=g).cuda(),
            "addend": torch.randn(B, H, W, NARROW, generator=g).cuda()}


def _run_case(case):
    """{(op, bm, bn, pre): (output, nfs_gemm_last record)} of one case under every pinned instance"""
    from neural_flow_style_amd import _lib, ops
    t = _inputs(case)
    pk_f, pk_d = ops.conv3x3_pack(t["w_f"], 0), ops.conv3x3_pack(t["w_d"], 1)
    out = {}
    try:
        for bm, bn in TILES:
            for pre in (0, 1):
                _lib.call("nfs_gemm_force", 3, bm, bn, 0, pre)
                y = ops.conv3x3_fwd(t["x"], pk_f, t["bias"], NARROW, relu=False)
                out["fwd", bm, bn, pre] = (y, _last_gemm())
                gx = ops.conv3x3_dgrad(t["gy"], pk_d, NARROW, x_in=t["x_in"], addend=t["addend"])
                out["dgrad", bm, bn, pre] = (gx, _last_gemm())
    finally:
        _lib.lib().nfs_gemm_force(-1, 0, 0, 0, 0)
    return out


def _run_step():
    """variable and Adam moments after two GridStylizer.step calls at 24^3, 3 views, conv1_1..conv5_1 (the case of
    bench.small_parity)"""
    import numpy as np
    from neural_flow_style_amd import engine, vgg
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as T
    G, V = 24, 3
    layers = ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv5_1"]
    rng = np.random.RandomState(123)
    d0 = S.blob_density(G, rng)
    vel0 = (rng.randn(G, G, G, 3) * 0.3 / (G - 1)).astype(np.float32)
    simg = S.style_image(G, G, rng)
    rot = T.rot_to_device(S.uniform_views(V), "cuda:0")
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv5_1"), "cuda:0")
    loss = engine.RenderStyleLoss(net, layers, [1.0] * 5, 1.0, transmit=0.05)
    loss.set_style_image(simg)
    gs = engine.GridStylizer(loss, torch.tensor(d0, device="cuda:0"), k=3, target="v", lr=1e-3)
    gs.var.copy_(torch.tensor(vel0))
    for _ in range(2):
        gs.step(rot)
    torch.cuda.synchronize()
    return {"var": gs.var.clone(), "m": gs.adam.m.clone(), "v": gs.adam.v.clone()}


def _run_all():
    res = {"case": {case: _run_case(case) for case in CASES}, "step": _run_step()}
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def rolled(tmp_path_factory):
    """everything once more with the rolled loop everywhere: one child process with NFS_RB16S_UNROLL=0"""
    path = str(tmp_path_factory.mktemp("rolled") / "rolled.pt")
    env = dict(os.environ, NFS_RB16S_UNROLL="0", PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, cwd=ROOT, timeout=600)
    return torch.load(path, map_location="cuda:0", weights_only=False)


@pytest.fixture(scope="module")
def unrolled():
    assert os.environ.get("NFS_RB16S_UNROLL", "1") != "0", "this process must run the default (unrolled) form"
    return _run_all()


def _unfold64(x):
    return torch.nn.functional.unfold(x.double().permute(0, 3, 1, 2), 3, padding=1)


def _conv64(x, w_oi33):
    """float64 3x3 'same' convolution on the device: x [B,H,W,Ci], w [Co,Ci,3,3] -> [B,H,W,Co]"""
    B, H, W, _ = x.shape
    y = w_oi33.reshape(w_oi33.shape[0], -1) @ _unfold64(x)
    return y.reshape(B, -1, H, W).permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", list(CASES), ids=[str(c) for c in CASES])
def test_unrolled_and_rolled_k_loop_agree_bit_for_bit_and_are_float32_accurate(case, unrolled, rolled):
    """forward and data gradient of one case under (3, bm, 128, 0, pre) for bm 48 and 80, pre 0 and 1: what ran is the
    forced instance with the K parts and the shape the table says; the unrolled result equals the rolled one bit for
    bit; and against a float64 direct convolution the error per element, |y - ref| / the convolution of the magnitudes,
    stays below 5e-3, the floor tests/test_gemm_instances_gpu.py holds the split-limb class to."""
    Z, T, ksplit, nch, why = CASES[case]
    Ci = case[3]
    assert Ci // 32 // ksplit == nch, why
    t = _inputs(case)
    w_f = t["w_f"].double().permute(3, 2, 0, 1)                      # [Co,Ci,3,3]
    w_d = t["w_d"].double().flip(0, 1).permute(2, 3, 0, 1)           # [128,Ci,3,3]: the data gradient as a conv of gy
    mask = (t["x_in"] > 0).double()
    refs = {"fwd": (_conv64(t["x"], w_f) + t["bias"].double(), _conv64(t["x"].abs(), w_f.abs()) + t["bias"].double().abs()),
            "dgrad": (_conv64(t["gy"], w_d) * mask + t["addend"].double(),
                      _conv64(t["gy"].abs(), w_d.abs()) * mask + t["addend"].double().abs())}
    got, want = unrolled["case"][case], rolled["case"][case]
    assert set(got) == set(want) == {(op, bm, bn, pre) for op in ("fwd", "dgrad") for bm, bn in TILES for pre in (0, 1)}
    for key in sorted(got):
        op, bm, bn, pre = key
        (y, rec), (y0, rec0) = got[key], want[key]
        for r in (rec, rec0):
            assert (r["variant"], r["bm"], r["bn"], r["nbuf"], r["pre"]) == (3, bm, bn, 0, pre), (why, key, r)
            assert (r["Z"], r["T"], r["K"], r["N"], r["ksplit"]) == (Z, T, Ci, NARROW, ksplit), (why, key, r)
        assert torch.equal(y, y0), "%s %s (%s): unrolled and rolled differ by %.3g" % (
            case, key, why, float((y - y0).abs().max()))
        ref, mag = refs[op]
        e = float(((y.double() - ref).abs() / mag).max())
        print("%s %s: float64 error %.3g" % (case, key, e))
        assert e < 5e-3, (case, key, why, e)


def test_two_steps_agree_bit_for_bit(unrolled, rolled):
    """24^3, 3 views, five style layers: the variable and both Adam moments after two GridStylizer.step calls are the
    same bits with the K loops unrolled and rolled"""
    for k in ("var", "m", "v"):
        a, b = unrolled["step"][k], rolled["step"][k]
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, k
        assert torch.equal(a, b), "%s differs by %.3g" % (k, float((a - b).abs().max()))


if __name__ == "__main__":
    torch.save(_run_all(), sys.argv[1])

"""The Laplacian-pyramid kernels of csrc/warp2d.hip element by element against the float64 references of tests/lap_ref.py:
the two gather forms, lap_down3_tiled_kernel, lap_up3_row_kernel, lap_up3_cell_kernel (in a child process with
NFS_LAP_UP=cell) and the two norm_* kernels.  Every case states which kernel it runs (nfs_lap_up_rms_parts against
lap_ref.expected_parts) and runs twice: with lap_ref.tap_kernel and whole-number data, where float32 is exact and the
result must EQUAL float64 -- every one of the 125 taps is pinned to its place -- and with the production kernel and
normal data, where every element must lie inside the derived bound (err/bound <= 1; the worst ratio is printed).

Worst err/bound on the MI355X (normal data; no case above 0.5, no defect found):
    gather 2-D: down 0.09  up 0.23      gather 3-D: down 0.03  up 0.15      lap_down3_tiled 0.03
    lap_up3_row 0.14  (nfs_lap_up_rms with addend_part 0.14; sum(out_part) 0.04 of its bound)
    lap_up3_cell 0.15  (with addend_part 0.19; sum(out_part) < 0.001)
    normalize_mean RMS 0.21  mean|x| 0.28  (energy in the tail 0.16 / 0.10, under eps 0.04)
The whole file takes 11 s, the child of the cell form 4.5 s of it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from tests import lap_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
EPS_RMS = 1e-10


def _ops():
    import neural_flow_style_amd.ops as ops
    return ops


def _k(nd):
    from neural_flow_style_amd import util
    return util.lap_kernel(nd == 3)


def _cu(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _id(c):
    return "%s-C%d" % ("x".join(map(str, c[0])), c[1])


def _path(full, cell=False):
    """the number of partial sums = which kernel nfs_lap_up takes for this volume, as the library and lap_ref both see it"""
    parts = _ops().lap_up_rms_parts(full)
    assert parts == LR.expected_parts(full, cell=cell), (full, parts)
    return parts


class Worst(dict):
    def hold(self, name, kind, got, want, bound, where):
        """whole numbers: equal; otherwise inside the bound"""
        got = _np(got) if torch.is_tensor(got) else got
        assert got.dtype == np.float32 and got.shape == want.shape, (where, got.shape, want.shape)
        if kind == "int":
            assert np.array_equal(got.astype(np.float64), want), (name, where)
            return
        r = LR.check(got, want, bound)
        self[name] = max(self.get(name, 0.0), r)
        assert r <= 1.0, (name, where, r)

    def report(self, title):
        print("%s, worst err/bound: %s" % (title, "  ".join("%s %.3f" % kv for kv in sorted(self.items()))))


def _down_and_up(worst, shape, C, tag, want_parts=None):
    """nfs_lap_down and nfs_lap_up (scale 5 without and -5 with an addend; the other two combinations on the staged forms)
    of one volume, both kinds"""
    ops = _ops()
    full = tuple(shape) + (C,)
    parts = _path(full)
    assert want_parts is None or (parts > 0) == want_parts, (full, parts)
    for kind in LR.KINDS:
        k, x, lo, add, _ = LR.case(full, kind, _k(len(shape)))
        kd = _cu(k)
        worst.hold(tag + "down", kind, ops.lap_down(_cu(x), kd), LR.down(x, k), LR.down_bound(x, k), full)
        terms = LR.up_terms(lo, k, full, bound=kind != "int")
        for scale, a in ((5.0, None), (-5.0, add)) + (((-5.0, None), (5.0, add)) if parts else ()):
            want, bound = LR.up_scaled(lo, k, full, scale, a, terms)
            worst.hold(tag + "up", kind, ops.lap_up(_cu(lo), kd, full, scale, addend=_cu(a)), want, bound, (full, scale))


# ---- the gather forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
def test_gather_forms_2d(C):
    """lap_down_kernel / lap_up_kernel, nd = 2: every H, W in 1..9 -- both parities, axes shorter than the window"""
    worst = Worst()
    for shape in LR.GATHER_2D:
        _down_and_up(worst, shape, C, "", want_parts=False)
    worst.report("gather 2-D C=%d" % C)


@pytest.mark.parametrize("C", [2, 4])
def test_gather_forms_3d(C):
    """nd = 3 with the channel counts no staged form takes: every D, H, W of (1, 2, 3, 4, 5, 8, 9)"""
    worst = Worst()
    for shape in LR.GATHER_3D:
        _down_and_up(worst, shape, C, "", want_parts=False)
    worst.report("gather 3-D C=%d" % C)


@pytest.mark.parametrize("case", [(s, C) for s in LR.GATHER_3D_SMALL for C in (1, 3)] + LR.ROW_TOO_WIDE, ids=_id)
def test_lap_up_gather_form_where_the_row_form_does_not_apply(case):
    """1 and 3 channels under 4096 voxels, and rows one voxel too wide for the 60 KB of staged rows: lap_up_kernel (lap_down
    is the tiled kernel at every size)"""
    worst = Worst()
    _down_and_up(worst, case[0], case[1], "", want_parts=False)
    worst.report("gather %s" % _id(case))


# ---- lap_down3_tiled_kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(s, C) for s in LR.TILED for C in (1, 3)], ids=_id)
def test_lap_down3_tiled_kernel(case):
    ops = _ops()
    worst = Worst()
    full = tuple(case[0]) + (case[1],)
    for kind in LR.KINDS:
        k, x, _, _, _ = LR.case(full, kind, _k(3))
        got = ops.lap_down(_cu(x), _cu(k))
        worst.hold("down", kind, got, LR.down(x, k), LR.down_bound(x, k), full)
        assert torch.equal(got, ops.lap_down(_cu(x), _cu(k)))
    worst.report("lap_down3_tiled %s" % _id(case))


# ---- lap_up3_row_kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LR.ROW, ids=_id)
def test_lap_up3_row_kernel(case):
    """nfs_lap_up on the row form: with and without an addend, at scale 5 and -5 (and nfs_lap_down of the same volume)"""
    worst = Worst()
    _down_and_up(worst, case[0], case[1], "", want_parts=True)
    worst.report("lap_up3_row %s" % _id(case))


def _up_rms_checks(worst, full, cell=False, nparts_list=LR.ADDEND_NPARTS, lean=False):
    """nfs_lap_up_rms of one volume the staged form takes: want_part (the count, out bit for bit nfs_lap_up's, the sum of
    the partial sums) and addend_part (random positive parts, all the energy in one slot, whole numbers with amul = 1/2,
    a zero addend with zero parts); every result bit-identical on a second call.  lean (the 2^21-voxel volumes of the cell
    form, where a float64 comparison is a second of host time): one scale, one random and one placed set of parts"""
    ops = _ops()
    parts = _path(full, cell=cell)
    assert parts > 0
    n = int(np.prod(full))
    for kind in LR.KINDS:
        k, _, lo, add, rng = LR.case(full, kind, _k(3))
        kd, lod, addd = _cu(k), _cu(lo), _cu(add)
        terms = LR.up_terms(lo, k, full, bound=kind != "int")
        # want_part
        for scale, a, ad in ((-5.0, add, addd), (5.0, None, None))[:1 if lean else 2]:
            out, part = ops.lap_up_rms(lod, kd, full, scale, addend=ad, want_part=True)
            assert part.shape == (parts,)
            assert torch.equal(out, ops.lap_up(lod, kd, full, scale, addend=ad)), (full, kind, scale)
            want, bound = LR.up_scaled(lo, k, full, scale, a, terms)
            worst.hold("up", kind, out, want, bound, (full, scale))
            total = float((_np(out).astype(np.float64) ** 2).sum())
            got_total = float(_np(part).astype(np.float64).sum())
            assert np.isfinite(_np(part)).all() and (_np(part) >= 0).all()
            r = abs(got_total - total) / (LR.part_sum_bound(full, cell) * total)
            worst["part_sum"] = max(worst.get("part_sum", 0.0), r)
            assert r <= 1.0, (full, kind, scale, r)
            out2, part2 = ops.lap_up_rms(lod, kd, full, scale, addend=ad, want_part=True)
            assert torch.equal(out, out2) and torch.equal(part, part2)
        # addend_part
        energy = float((add.astype(np.float64) ** 2).sum())
        for nparts in nparts_list:
            if kind == "int":                            # 4 n in one slot: amul = 1 / sqrt(4) = 1/2, exact
                sets = [LR.addend_parts(rng, nparts, 4.0 * n, s) for s in (LR.energy_slots(nparts)[-1],)]
                assert float(sets[0].max()) == 4.0 * n
            else:
                slots = LR.energy_slots(nparts)
                sets = [LR.addend_parts(rng, nparts, energy, s) for s in [None] + (slots[-1:] if lean else slots)]
            for ap in sets:
                for scale in (LR.SCALES if nparts == nparts_list[0] and not lean else (5.0,)):
                    out = ops.lap_up_rms(lod, kd, full, scale, addend=addd, addend_part=_cu(ap), eps=EPS_RMS)
                    want, bound = LR.up_rms(lo, k, full, scale, add, ap, n, EPS_RMS, terms)
                    worst.hold("up_rms", kind, out, want, bound, (full, nparts, scale))
            again = ops.lap_up_rms(lod, kd, full, scale, addend=addd, addend_part=_cu(sets[-1]), eps=EPS_RMS)
            assert torch.equal(out, again)
        if lean:
            continue
        # a zero addend with zero parts: 0 / eps, finite, and scale * up(lo)
        zero = torch.zeros(full, device="cuda")
        out = ops.lap_up_rms(lod, kd, full, -5.0, addend=zero, addend_part=torch.zeros(parts, device="cuda"), eps=EPS_RMS)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out, ops.lap_up(lod, kd, full, -5.0))
        worst.hold("up_rms", kind, out, *LR.up_scaled(lo, k, full, -5.0, None, terms), (full, "zero addend"))


@pytest.mark.parametrize("case", LR.ROW, ids=_id)
def test_lap_up_rms_on_the_row_form(case):
    worst = Worst()
    _up_rms_checks(worst, tuple(case[0]) + (case[1],))
    worst.report("lap_up_rms (rows) %s" % _id(case))


def test_lap_up_rms_is_refused_where_no_staged_form_applies():
    ops = _ops()
    from neural_flow_style_amd import _lib
    for full in [(16, 16, 15, 3), (4, 4, 853, 3), (16, 16, 16, 2), (64, 64, 1)]:
        assert _path(full) == 0
        k, _, lo, _, _ = LR.case(full, "randn", _k(len(full) - 1))
        with pytest.raises(_lib.NfsError):
            ops.lap_up_rms(_cu(lo), _cu(k), full, 5.0)


# ---- lap_up3_cell_kernel: NFS_LAP_UP is read once per process --------------------------------------------------------------
def _cell_child():
    """runs with NFS_LAP_UP=cell: nfs_lap_up, nfs_lap_up_rms with want_part and with addend_part of the volumes of
    lap_ref.CELL; prints the worst ratios"""
    ops = _ops()
    assert os.environ.get("NFS_LAP_UP") == "cell"
    worst = Worst()
    for shape, C in LR.CELL:
        full = tuple(shape) + (C,)
        parts = _path(full, cell=True)
        if parts:
            _up_rms_checks(worst, full, cell=True, nparts_list=(parts,), lean=True)
            print("cell form %s: %d blocks" % (_id((shape, C)), parts))
            continue
        # under 2^21 voxels: the gather form, and no nfs_lap_up_rms
        for kind in LR.KINDS:
            k, _, lo, add, _ = LR.case(full, kind, _k(3))
            want, bound = LR.up_scaled(lo, k, full, -5.0, add, LR.up_terms(lo, k, full, bound=kind != "int"))
            worst.hold("gather_up", kind, ops.lap_up(_cu(lo), _cu(k), full, -5.0, addend=_cu(add)), want, bound, full)
        print("gather form %s" % _id((shape, C)))
    worst.report("NFS_LAP_UP=cell")
    print("CELL-OK")


def test_lap_up3_cell_kernel():
    """(127,130,129) x 3 and (129,128,128) x 1: the smallest volumes the cell form takes, both parities; (129,127,128) x 1,
    128 voxels short of 2^21, must stay on the gather form"""
    env = dict(os.environ)
    env["NFS_LAP_UP"] = "cell"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "CELL-OK" in r.stdout and r.stdout.count("cell form") == 2 and r.stdout.count("gather form") == 1


# ---- nfs_normalize_mean -----------------------------------------------------------------------------------------------------
def _normalize(x, use_abs, eps, align):
    """through ops.normalize_mean (aligned), or through the entry point with the input ('x') or the output ('out') at a
    4-byte offset from a 16-byte boundary: the scalar path of both kernels / of the scale kernel"""
    ops = _ops()
    from neural_flow_style_amd import _lib
    n = x.size
    if align == "aligned":
        xd = _cu(x)
        assert xd.data_ptr() % 16 == 0
        return _np(ops.normalize_mean(xd, use_abs=use_abs, eps=eps))
    xb, ob = torch.zeros(n + 1, device="cuda"), torch.full((n + 2,), 7.0, device="cuda")
    assert xb.data_ptr() % 16 == 0 and ob.data_ptr() % 16 == 0
    xd = xb[1:] if align == "x" else xb[:n]
    od = ob[1:n + 1] if align == "out" else ob[:n]
    xd.copy_(torch.as_tensor(x))
    ws = torch.empty(1024, device="cuda")
    _lib.call("nfs_normalize_mean", ops._ptr(xd), ops._ptr(od), n, int(use_abs), float(eps), ops._ptr(ws), 1024,
              ops._stream())
    res = _np(ob)
    assert res[n + 1] == 7.0 and (res[0] == 7.0 if align == "out" else res[n] == 7.0)     # nothing written past the end
    return _np(od)


@pytest.mark.parametrize("align", ["aligned", "x", "out"])
@pytest.mark.parametrize("use_abs", [False, True], ids=["rms", "abs"])
def test_normalize_mean(use_abs, align):
    worst = Worst()
    tag = "abs" if use_abs else "rms"
    for n in LR.NORM_NS:
        parts = LR.norm_parts(n)
        x = LR.randn(np.random.RandomState(n % 9973), (n,))
        got = _normalize(x, use_abs, 1e-10, align)
        worst.hold(tag, "randn", got, *LR.normalize_mean(x, use_abs, 1e-10), (n, align))
        assert np.array_equal(got, _normalize(x, use_abs, 1e-10, align))
        # all the energy in the last 1 .. n % 4 elements, and in the elements past parts * 2048 (the grid-stride loop wraps)
        tails = list(range(1, n % 4 + 1)) + ([n - parts * 2048] if n > parts * 2048 else [])
        for tail in tails:
            x = np.zeros(n, np.float32)
            x[n - tail:] = 3.0
            got = _normalize(x, use_abs, 1e-10, align)
            worst.hold(tag + "_tail", "randn", got, *LR.normalize_mean(x, use_abs, 1e-10), (n, tail, align))
            exact = n / tail if use_abs else np.sqrt(n / tail)
            assert abs(float(got[-1]) - exact) <= (5 + (0 if use_abs else 0.5)) * LR.EPS * exact, (n, tail, got[-1])
            assert not got[:n - tail].any()
    for n in (5, 2049):
        # eps: zeros stay zeros; |x| = 1e-12 under eps = 1e-10 gives x / eps; eps = 1e-7 with |x| = 1e-9
        assert not _normalize(np.zeros(n, np.float32), use_abs, 1e-10, align).any()
        for mag, eps in ((1e-12, 1e-10), (1e-9, 1e-7)):
            x = (np.float32(mag) * np.sign(LR.randn(np.random.RandomState(n), (n,)))).astype(np.float32)
            got = _normalize(x, use_abs, eps, align)
            want, bound = LR.normalize_mean(x, use_abs, eps)
            assert np.array_equal(want, x.astype(np.float64) / float(np.float32(eps)))
            worst.hold(tag + "_eps", "randn", got, want, bound, (n, eps, align))
    worst.report("normalize_mean %s %s" % (tag, align))


if __name__ == "__main__":
    _cell_child()

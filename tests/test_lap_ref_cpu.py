"""tests/lap_ref.py pinned without a GPU: (1) its operators composed as util.lap_normalize composes them are the oracle's
lap_normalize to 1e-12, and ``up`` is the transpose of ``down`` for every axis length; (2) its bounds are not too tight -- a
float32 numpy emulation (the same slices accumulated in float32) lies inside every one of them on the cases the GPU test
runs, and EQUALS float64 on the whole-number cases; (3) not too loose -- every planted defect leaves a bound on those
cases; the two tap-order defects pass with the production kernel (it is symmetric under every flip and axis permutation)
and fail with lap_ref.tap_kernel; (4) expected_parts on a table worked out by hand.

Largest err/bound of the float32 emulation per operator over all cases (each test prints its own):
    down 0.09   up 0.23   up_rms 0.14   normalize_mean RMS 0.21, mean|x| 0.28"""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import lap_ref as LR

f32 = np.float32


def _k(nd):
    from neural_flow_style_amd import util
    return util.lap_kernel(nd == 3)


def _id(c):
    return "%s-C%d" % ("x".join(map(str, c[0])), c[1])


# ---- float32 emulations -----------------------------------------------------------------------------------------------
def down32(x, k, **kw):
    return LR.down(x, k, dtype=f32, **kw)


def up32(lo, k, shape, scale, addend=None, mul=None, scale_last=False):
    """float32 nfs_lap_up / nfs_lap_up_rms (mul = the float32 1 / max(rms, eps)); scale_last: the planted defect"""
    s = LR.up(lo, k, shape, dtype=f32)
    a = None if addend is None else (np.asarray(addend, f32) if mul is None else f32(mul) * np.asarray(addend, f32))
    if scale_last:
        return f32(scale) * (s + a)
    s = f32(scale) * s
    return s if a is None else s + a


def amul32(part, n, eps, skip=None, no_eps=False):
    """the kernels' 1 / fmaxf(sqrtf((float)(sum / n)), eps): the sum in double; skip: a slot the sum leaves out"""
    p = np.asarray(part, np.float64).copy()
    if skip is not None and skip < p.size:
        p[skip] = 0.0
    m = np.sqrt(f32(p.sum() / float(n)))
    with np.errstate(divide="ignore"):
        return f32(1.0) / (m if no_eps else max(m, f32(eps)))


def norm32(x, use_abs, eps, drop_tail=False, no_eps=False):
    """float32 nfs_normalize_mean: float32 partial sums over norm_parts(n) chunks, their total in double"""
    x = np.asarray(x, f32).ravel()
    n = x.size
    t = np.abs(x) if use_abs else x * x
    if drop_tail:
        t = t[:n - n % 4]
    tot = sum(float(np.add.reduce(c, dtype=f32)) for c in np.array_split(t, LR.norm_parts(n)))
    m = f32(tot / n) if use_abs else np.sqrt(f32(tot / n))
    with np.errstate(divide="ignore", invalid="ignore"):
        return x * (f32(1.0) / (m if no_eps else max(m, f32(eps))))


def _down_cases():
    return ([(s, C) for s in LR.GATHER_2D for C in (1, 2)] + [(s, C) for s in LR.GATHER_3D[::7] for C in (2, 4)]
            + [(s, C) for s in LR.GATHER_3D_SMALL + LR.TILED for C in (1, 3)])


def _up_cases():
    return _down_cases() + LR.ROW + LR.ROW_TOO_WIDE


# ---- (1) the references -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 9, 10, 1), (8, 8, 8, 3), (9, 12, 11, 2), (17, 12, 3), (9, 9, 1), (8, 16, 2)])
def test_composed_reference_is_the_oracle(shape):
    """lap_split_n / normalize_std / lap_merge written with lap_ref's operators against oracle.lap_normalize in float64:
    scale_n 1 and 3, 3-D and 2-D, even and odd sizes"""
    rng = np.random.RandomState(sum(shape))
    g = rng.randn(*shape)
    nd = len(shape) - 1
    k = _k(nd).astype(np.float64)
    s = 5.0 if nd == 3 else 4.0
    for scale_n in (1, 3):
        his, cur = [], g
        for _ in range(scale_n):
            lo = LR.down(cur, k)
            his.append(cur - s * LR.up(lo, k, cur.shape))
            cur = lo
        out = LR.normalize_mean(cur, False, 1e-10)[0]
        for hi in his[::-1]:
            out = s * LR.up(out, k, hi.shape) + LR.normalize_mean(hi, False, 1e-10)[0]
        want = O.lap_normalize(torch.tensor(g, dtype=torch.float64), k, scale_n).numpy()
        assert np.abs(out - want).max() <= 1e-12 * np.abs(want).max(), (shape, scale_n)
    want0 = O.lap_normalize(torch.tensor(g, dtype=torch.float64), k, 0).numpy()
    assert np.abs(LR.normalize_mean(g, True, 1e-7)[0] - want0).max() <= 1e-12 * np.abs(want0).max()


@pytest.mark.parametrize("n", range(1, 10))
def test_up_is_the_transpose_of_down(n):
    """<down(x), y> == <x, up(y)> with a kernel of 125 distinct taps, the axis of length n in every position"""
    rng = np.random.RandomState(n)
    for shape in ((n, 3, 4, 2), (4, n, 3, 2), (3, 4, n, 2), (n, n, n, 1), (n, 5, 2), (6, n, 2)):
        k = rng.randn(*(5,) * (len(shape) - 1))
        x, y = rng.randn(*shape), rng.randn(*LR.coarse(shape))
        a, b = float((LR.down(x, k) * y).sum()), float((x * LR.up(y, k, shape)).sum())
        assert abs(a - b) <= 1e-12 * float((np.abs(LR.down(np.abs(x), np.abs(k))) * np.abs(y)).sum()), shape


def test_geometry_is_tf_same():
    assert [LR.pad_before(n) for n in range(1, 9)] == [2, 1, 2, 1, 2, 1, 2, 1]
    assert [LR.out_len(n) for n in range(1, 9)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [LR.pad_before(n) for n in range(1, 40)] == [O._tf_same_pads(n)[0] for n in range(1, 40)]
    # a centred impulse comes back as the kernel's taps of its parity: out[o] = k[2 + 2 (c - o)] for x = delta(2 c)
    k = LR.tap_kernel(2).astype(np.float64)
    x = np.zeros((9, 9, 1)); x[4, 4, 0] = 1.0
    assert np.array_equal(LR.down(x, k)[1:4, 1:4, 0], k[::2, ::2][::-1, ::-1])


# ---- (2) the bounds hold a float32 emulation -----------------------------------------------------------------------------
def test_float32_emulation_of_down_and_up_is_inside_the_bounds():
    worst = {"down": 0.0, "up": 0.0}
    for shape, C in _up_cases():
        full = tuple(shape) + (C,)
        for kind in LR.KINDS:
            k, x, lo, add, _ = LR.case(full, kind, _k(len(shape)))
            if (shape, C) in _down_cases():
                got, want = down32(x, k), LR.down(x, k)
                if kind == "int":
                    assert np.array_equal(got.astype(np.float64), want), full
                else:
                    worst["down"] = max(worst["down"], LR.check(got, want, LR.down_bound(x, k)))
            for scale, a in ((5.0, None), (-5.0, add)):
                got = up32(lo, k, full, scale, a)
                want, bound = LR.up_scaled(lo, k, full, scale, a)
                if kind == "int":
                    assert np.array_equal(got.astype(np.float64), want), full
                else:
                    worst["up"] = max(worst["up"], LR.check(got, want, bound))
    print("float32 emulation, worst err/bound: down %.3f  up %.3f" % (worst["down"], worst["up"]))
    assert 0 < worst["down"] <= 1.0 and 0 < worst["up"] <= 1.0


def test_float32_emulation_of_up_rms_is_inside_the_bound():
    worst = 0.0
    for (shape, C), nparts in zip(LR.ROW, LR.ADDEND_NPARTS + LR.ADDEND_NPARTS):
        full = tuple(shape) + (C,)
        n = int(np.prod(full))
        k, _, lo, add, rng = LR.case(full, "randn", _k(3))
        for slot in [None] + LR.energy_slots(nparts):
            part = LR.addend_parts(rng, nparts, float((add.astype(np.float64) ** 2).sum()), slot)
            got = up32(lo, k, full, 5.0, add, mul=amul32(part, n, 1e-10))
            want, bound = LR.up_rms(lo, k, full, 5.0, add, part, n, 1e-10)
            worst = max(worst, LR.check(got, want, bound))
        # whole numbers with the energy 4 n in one slot: amul = 1/2 exactly, and the result equals float64
        k, _, lo, add, rng = LR.case(full, "int", None)
        part = LR.addend_parts(rng, nparts, 4.0 * n, nparts - 1)
        assert float(part[-1]) == 4.0 * n
        got = up32(lo, k, full, -5.0, add, mul=amul32(part, n, 1e-10))
        assert np.array_equal(got.astype(np.float64), LR.up_rms(lo, k, full, -5.0, add, part, n, 1e-10)[0])
    print("float32 emulation, worst err/bound: up_rms %.3f" % worst)
    assert 0 < worst <= 1.0


def test_float32_emulation_of_normalize_mean_is_inside_the_bound():
    worst = {False: 0.0, True: 0.0}
    for n in LR.NORM_NS:
        x = LR.randn(np.random.RandomState(n % 9973), (n,))
        for use_abs in (False, True):
            want, bound = LR.normalize_mean(x, use_abs, 1e-10)
            worst[use_abs] = max(worst[use_abs], LR.check(norm32(x, use_abs, 1e-10), want, bound))
    print("float32 emulation, worst err/bound: normalize_mean RMS %.3f  mean|x| %.3f" % (worst[False], worst[True]))
    assert 0 < worst[False] <= 1.0 and 0 < worst[True] <= 1.0
    # the expected values of the energy-placement cases: a single 3.0 at the end gives sqrt(n) (RMS) and n (mean |x|)
    for n in (5, 7, 2049, 4099):
        x = np.zeros(n, f32); x[-1] = 3.0
        assert abs(LR.normalize_mean(x, False, 1e-10)[0][-1] - np.sqrt(n)) <= 1e-12 * np.sqrt(n)
        assert abs(LR.normalize_mean(x, True, 1e-10)[0][-1] - n) <= 1e-12 * n
    assert np.array_equal(LR.normalize_mean(np.zeros(5, f32), False, 1e-10)[0], np.zeros(5))
    x = np.full(7, 1e-12, f32)
    assert np.allclose(LR.normalize_mean(x, False, 1e-10)[0], x.astype(np.float64) / float(f32(1e-10)), rtol=1e-15)


# ---- (3) planted defects ---------------------------------------------------------------------------------------------------
def _rejected(got, want, bound):
    return LR.check(got, want, bound) > 1.0


@pytest.mark.parametrize("case", [((16, 16, 16), 1), ((21, 19, 37), 3), ((8, 9, 5), 2), ((8, 9), 2)], ids=_id)
def test_defect_corner_tap_dropped_on_the_last_plane(case):
    """lap_up without the corner tap k[4,4,4] on the fine plane z = D - 1 (the production kernel's corner is 9.5e-4)"""
    shape, C = case
    full = tuple(shape) + (C,)
    nd = len(shape)
    for kind in LR.KINDS:
        k, _, lo, add, _ = LR.case(full, kind, _k(nd))
        corner = np.zeros_like(k); corner[(4,) * nd] = k[(4,) * nd]
        lost = LR.up(lo, corner, full, dtype=f32)
        lost[:-1] = 0.0
        assert np.count_nonzero(lost) > 0
        want, bound = LR.up_scaled(lo, k, full, -5.0, add)
        assert not _rejected(up32(lo, k, full, -5.0, add), want, bound)
        assert _rejected(up32(lo, k, full, -5.0, add) - f32(-5.0) * lost, want, bound), (full, kind)


@pytest.mark.parametrize("parity", [0, 1], ids=["even", "odd"])
def test_defect_pad_before_off_by_one(parity):
    def pad(n):
        return LR.pad_before(n) + (1 if n % 2 == parity else 0)
    hit = 0
    for shape, C in [((8, 9), 1), ((1, 9), 2), ((4, 5, 8), 2), ((9, 7, 33), 3), ((17, 16, 16), 1), ((2, 2, 1024), 1)]:
        full = tuple(shape) + (C,)
        if not any(n % 2 == parity for n in shape):
            continue
        hit += 1
        for kind in LR.KINDS:
            k, x, lo, _, _ = LR.case(full, kind, _k(len(shape)))
            assert _rejected(down32(x, k, pad=pad), LR.down(x, k), LR.down_bound(x, k)), (full, kind)
            want, bound = LR.up_scaled(lo, k, full, 5.0)
            assert _rejected(f32(5.0) * LR.up(lo, k, full, pad=pad, dtype=f32), want, bound), (full, kind)
    assert hit >= 4


def test_defect_last_ragged_tile_left_at_zero():
    for shape, axis, tile in (((9, 7, 33), 2, 16), ((8, 9, 65), 2, 16), ((21, 19, 37), 1, 4), ((21, 19, 37), 0, 4)):
        for kind in LR.KINDS:
            k, x, _, _, _ = LR.case(shape + (3,), kind, _k(3))
            got = down32(x, k)
            cut = got.shape[axis] // tile * tile
            assert 0 < cut < got.shape[axis]
            sl = [slice(None)] * 4
            sl[axis] = slice(cut, None)
            got[tuple(sl)] = 0.0
            assert _rejected(got, LR.down(x, k), LR.down_bound(x, k)), (shape, axis, kind)


@pytest.mark.parametrize("order", ["mirrored", "exchanged"])
def test_defect_tap_order_is_seen_only_with_the_tap_kernel(order):
    """taps mirrored along one axis, or the axes a and e exchanged: the production kernel is unchanged by either (the
    blind spot of every test that uses it), the distinct-integer kernel is not"""
    def wrong(k):
        return np.ascontiguousarray(k[::-1] if order == "mirrored" else np.swapaxes(k, 0, -1))
    for nd in (2, 3):
        assert np.array_equal(wrong(_k(nd)), _k(nd))
        assert not np.array_equal(wrong(LR.tap_kernel(nd)), LR.tap_kernel(nd))
    for shape, C in [((8, 9), 1), ((5, 4), 2), ((4, 5, 8), 2), ((2, 3, 4), 3), ((9, 7, 33), 1), ((16, 16, 16), 3),
                     ((5, 8, 231), 3)]:
        full = tuple(shape) + (C,)
        k, x, lo, add, _ = LR.case(full, "randn", _k(len(shape)))
        assert not _rejected(down32(x, wrong(k)), LR.down(x, k), LR.down_bound(x, k))
        want, bound = LR.up_scaled(lo, k, full, 5.0, add)
        assert not _rejected(up32(lo, wrong(k), full, 5.0, add), want, bound)
        k, x, lo, add, _ = LR.case(full, "int", None)
        assert not np.array_equal(down32(x, wrong(k)).astype(np.float64), LR.down(x, k)), full
        assert _rejected(down32(x, wrong(k)), LR.down(x, k), LR.down_bound(x, k)), full
        want, bound = LR.up_scaled(lo, k, full, 5.0, add)
        assert not np.array_equal(up32(lo, wrong(k), full, 5.0, add).astype(np.float64), want), full
        assert _rejected(up32(lo, wrong(k), full, 5.0, add), want, bound), full


def test_defect_scale_applied_after_the_addend():
    for shape, C in [((8, 9), 2), ((4, 5, 8), 4), ((16, 16, 16), 1), ((64, 64, 1), 3)]:
        full = tuple(shape) + (C,)
        for kind in LR.KINDS:
            k, _, lo, add, _ = LR.case(full, kind, _k(len(shape)))
            for scale in LR.SCALES:
                want, bound = LR.up_scaled(lo, k, full, scale, add)
                assert _rejected(up32(lo, k, full, scale, add, scale_last=True), want, bound), (full, kind, scale)


def test_defects_of_the_addend_normalisation():
    """addend_n taken as voxels (off by C), a partial-sum slot beyond 256 ignored, eps not applied"""
    for (shape, C), nparts in (((16, 16, 16), 3), 64), (((5, 8, 231), 3), 321), (((21, 19, 37), 3), 1024):
        full = tuple(shape) + (C,)
        n = int(np.prod(full))
        k, _, lo, add, rng = LR.case(full, "randn", _k(3))
        total = float((add.astype(np.float64) ** 2).sum())
        part = LR.addend_parts(rng, nparts, total)
        want, bound = LR.up_rms(lo, k, full, 5.0, add, part, n, 1e-10)
        assert not _rejected(up32(lo, k, full, 5.0, add, mul=amul32(part, n, 1e-10)), want, bound)
        assert _rejected(up32(lo, k, full, 5.0, add, mul=amul32(part, n // C, 1e-10)), want, bound), full
    for (shape, C), nparts in (((17, 16, 16), 1), 257), (((16, 17, 65), 3), 320), (((2, 2, 1024), 1), 321), (((1, 64, 64), 3), 1024):
        full = tuple(shape) + (C,)
        n = int(np.prod(full))
        k, _, lo, add, rng = LR.case(full, "randn", _k(3))
        total = float((add.astype(np.float64) ** 2).sum())
        for slot in [s for s in LR.energy_slots(nparts) if s >= 256]:
            for placed in (None, slot):                  # random positive parts, and all the energy in that slot
                part = LR.addend_parts(rng, nparts, total, placed)
                want, bound = LR.up_rms(lo, k, full, 5.0, add, part, n, 1e-10)
                assert not _rejected(up32(lo, k, full, 5.0, add, mul=amul32(part, n, 1e-10)), want, bound)
                got = up32(lo, k, full, 5.0, add, mul=amul32(part, n, 1e-10, skip=slot))
                assert _rejected(got, want, bound), (full, nparts, slot, placed)
    # eps not applied: a zero addend with zero parts is 0 * inf
    full = (16, 16, 16, 1)
    k, _, lo, add, _ = LR.case(full, "randn", _k(3))
    zero, part = np.zeros_like(add), np.zeros(45, f32)
    want, bound = LR.up_rms(lo, k, full, 5.0, zero, part, zero.size, 1e-10)
    assert np.array_equal(want, LR.up_scaled(lo, k, full, 5.0)[0])
    assert not _rejected(up32(lo, k, full, 5.0, zero, mul=amul32(part, zero.size, 1e-10)), want, bound)
    with np.errstate(invalid="ignore"):
        assert _rejected(up32(lo, k, full, 5.0, zero, mul=amul32(part, zero.size, 1e-10, no_eps=True)), want, bound)


def test_defects_of_normalize_mean():
    """the n % 4 tail left out of the sum; eps not applied"""
    for use_abs in (False, True):
        for n in (5, 7, 2049, 4099, 1025 * 2048 + 3):
            for tail in range(1, n % 4 + 1):             # all the energy in the last 1 .. n % 4 elements
                x = np.zeros(n, f32); x[n - tail:] = 3.0
                want, bound = LR.normalize_mean(x, use_abs, 1e-10)
                assert not _rejected(norm32(x, use_abs, 1e-10), want, bound)
                assert _rejected(norm32(x, use_abs, 1e-10, drop_tail=True), want, bound), (n, tail, use_abs)
        for n in (5, 7):                                 # and on normal data, where the tail is a fair share of the sum
            x = LR.randn(np.random.RandomState(n), (n,))
            want, bound = LR.normalize_mean(x, use_abs, 1e-10)
            assert _rejected(norm32(x, use_abs, 1e-10, drop_tail=True), want, bound), (n, use_abs)
        for x, eps in ((np.zeros(2049, f32), 1e-10), (np.full(7, 1e-12, f32), 1e-10), (np.full(4099, 1e-9, f32), 1e-7)):
            want, bound = LR.normalize_mean(x, use_abs, eps)
            assert not _rejected(norm32(x, use_abs, eps), want, bound)
            assert _rejected(norm32(x, use_abs, eps, no_eps=True), want, bound), (x[0], eps, use_abs)


# ---- (4) which kernel a shape takes ---------------------------------------------------------------------------------------
def test_expected_parts_on_a_table_worked_out_by_hand():
    """cells of an axis: n = 16 -> p = 1, m = 0..8: 9; n = 4 -> 3; n = 2 -> 2; odd n -> (n + 1) / 2.
    (16,16,16): rows = 9 cell rows of y x ceil(9 / 2) = 5 pairs of z -> 45.  (4,4,852,3): 13632 voxels, 12 rows of 426 x 3
    floats = 61344 B <= 61440: 3 x ceil(3 / 2) = 6; 853 wide: 427 x 3 x 48 = 61488 B.  (2,2,2560,1): 1280 x 48 = 61440 B:
    2 x 1 = 2; 2561: 1281 x 48 = 61488 B.  Cells: (127,130,129): 64, 66, 65 cells -> 16 x 17 x 5 = 1360 blocks;
    (129,127,128) = 2097024 voxels < 2^21 = 2097152; (129,128,128): 65, 65, 65 -> 17 x 17 x 5 = 1445"""
    table = {(16, 16, 16, 3): 45, (16, 16, 16, 1): 45, (16, 16, 15, 3): 0, (4, 4, 852, 3): 6, (4, 4, 853, 3): 0,
             (2, 2, 2560, 1): 2, (2, 2, 2561, 1): 0, (17, 16, 16, 1): 45, (5, 8, 231, 3): 5 * 2, (1, 64, 64, 1): 33,
             (64, 1, 64, 3): 17, (64, 64, 1, 1): 33 * 17, (21, 19, 37, 3): 10 * 6}
    for shape, want in table.items():
        assert LR.expected_parts(shape) == want, shape
    assert LR.expected_parts((4, 4, 852, 3)) > 0 and LR.expected_parts((2, 2, 2560, 1)) > 0
    for shape in [(16, 16, 16), (64, 64, 64), (4, 4, 852)]:
        assert LR.expected_parts(shape + (2,)) == 0 and LR.expected_parts(shape + (4,)) == 0
    for shape in [(64, 64, 1), (128, 128, 3), (4096, 4096, 1)]:
        assert LR.expected_parts(shape) == 0
    cells = {(127, 130, 129, 3): 1360, (129, 127, 128, 1): 0, (129, 128, 128, 1): 1445, (16, 16, 16, 3): 0,
             (128, 128, 128, 2): 0}
    for shape, want in cells.items():
        assert LR.expected_parts(shape, cell=True) == want, shape
    # every row-form case of the GPU test is one, and the two made one voxel wider are not
    assert all(LR.expected_parts(tuple(s) + (C,)) > 0 for s, C in LR.ROW)
    assert all(LR.expected_parts(tuple(s) + (C,)) == 0 for s, C in LR.ROW_TOO_WIDE)
    assert all(LR.expected_parts(tuple(s) + (C,)) == 0 for s in LR.GATHER_3D_SMALL for C in (1, 3))

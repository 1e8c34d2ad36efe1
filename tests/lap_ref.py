"""The Laplacian-pyramid kernels (csrc/warp2d.hip: nfs_lap_down, nfs_lap_up, nfs_lap_up_rms, nfs_normalize_mean) restated in
float64 numpy from the definition, element by element, with a derived float32 bound for every element.  NumPy only; of the
package only util.lap_kernel (the production taps) is used, by the tests.

The operators.  x is [D,H,W,C] with k [5,5,5], or [H,W,C] with k [5,5]; the same k for every channel.
  * TF 'SAME' for stride 2 and window 5 on an axis of length n: out_len = ceil(n / 2), total padding
    max(2 (out_len - 1) + 5 - n, 0), ``pad_before`` its floor half (1 for even n, 2 for odd n), the rest after.
  * ``down``: the correlation  out[o] = sum_{a,b,e} k[a,b,e] x[2 o + (a,b,e) - pad]  (x zero outside the volume), written
    as one strided slice of an explicitly zero-padded array per tap: 125 (25) slices accumulated in float64.
  * ``up``: its exact transpose written as a SCATTER -- k[a,b,e] * lo is added into the strided slice of a padded array
    that ``down`` read for that tap, then the padding is cropped.  The kernels GATHER by parity (at most 3 taps per axis
    reach an output); the scatter is an independent statement of the same operator.

Bounds (EPS = 2^-24, one float32 rounding; first order, nothing fitted to a kernel's output).  A float32 sum of T products
p_t, in ANY order and with or without FMA contraction, has each product rounded at most once and passes through at most
T - 1 additions, each of which rounds a partial sum no larger than sum |p_t|: the error is at most T EPS sum |p_t|.
  * ``down_bound`` = (T + 1) EPS down(|x|, |k|), T = 125 (25): the sum, and one to spare for the store of a staged form.
  * ``up_bound``   = (T + 3) EPS (|scale| up(|lo|, |k|) + |a|), T = 27 (9) = the most taps of matching parity (3 per
    axis; a form that also adds the zero-weight taps adds exact zeros); a = the addend term as it enters the sum; the 3:
    the product by scale, the product that forms a, and the final addition (each at most EPS times the magnitudes summed).
  * ``up_rms``: a = addend * amul, amul = 1 / max(sqrt(sum(addend_part) / addend_n), eps).  The partial sums are added in
    double (no float32 rounding); the quotient is cast to float32 (1), sqrtf halves the relative error it is given and
    rounds once (1), the reciprocal (1), and the product with the addend (1): 4 EPS |addend amul| on top of up_bound.
  * ``normalize_mean``: out = x / max(m, eps), m = sqrt(mean x^2) or mean |x|.  The kernel adds ``parts`` float32 partial
    sums of about ceil(n / parts) positive terms each (parts = min(1024, ceil(n / 2048))) and adds those in double.  A sum
    of positive terms in any order is within terms * EPS relative (the squares' own roundings included: a square and its
    addition are one term's two roundings, and the tree of a block sum has fewer levels than terms); the square root
    halves that; 5 = the cast, sqrtf, the reciprocal, the product and one to spare -- (ceil(n / parts) / 2 + 5) EPS
    relative; use_abs has no square root and no squares: (ceil(n / parts) + 4) EPS.
Second-order terms in EPS are not carried.

Exact inputs.  ``tap_kernel`` is k[a][b][e] = 1 + (a 5 + b) 5 + e (2-D: 1 + b 5 + e): 125 distinct whole numbers.  With x,
lo and the addend whole numbers in -8..8 and scale = -5 or 5 every product and every partial sum is a whole number with
|sum| <= 125 * 125 * 8 * 5 < 2^24, which float32 holds exactly in any order: a kernel must EQUAL the float64 value, and a
tap read from another place (mirrored, axes exchanged, a transposed weight table) cannot.  The production kernel is
invariant under every axis permutation and flip and hides all of these."""
import numpy as np

from tests.field_ref import err_ratio

EPS = 2.0 ** -24
INT_RANGE = 8                                    # whole-number data are drawn from -8..8
ROW_MIN_VOXELS, ROW_LDS_BYTES, ROW_STAGED_ROWS = 4096, 60 * 1024, 12
CELL_MIN_VOXELS = 2 ** 21


# ---- geometry -------------------------------------------------------------------------------------------------------
def out_len(n):
    return -(-int(n) // 2)


def pad_before(n):
    return max(2 * (out_len(n) - 1) + 5 - int(n), 0) // 2


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _padded(dims, pad):
    """extent of the zero-padded array per axis: every tap of every output, and the whole volume"""
    return tuple(max(2 * (out_len(n) - 1) + 5, pad(n) + n) for n in dims)


def _tap_slices(dims, tap):
    return tuple(slice(t, t + 2 * (out_len(n) - 1) + 1, 2) for n, t in zip(dims, tap))


# ---- the operators (``pad``, ``dtype``: for the emulations and planted defects of tests/test_lap_ref_cpu.py) ---------
def down(x, k, pad=pad_before, dtype=np.float64):
    x, k = np.asarray(x, dtype=dtype), np.asarray(k, dtype=dtype)
    dims, nd = x.shape[:-1], x.ndim - 1
    assert k.shape == (5,) * nd, (x.shape, k.shape)
    P = np.zeros(_padded(dims, pad) + x.shape[-1:], dtype=dtype)
    P[tuple(slice(pad(n), pad(n) + n) for n in dims)] = x
    out = np.zeros(tuple(out_len(n) for n in dims) + x.shape[-1:], dtype=dtype)
    for tap in np.ndindex(*k.shape):
        out += k[tap] * P[_tap_slices(dims, tap)]
    return out


def up(lo, k, shape, pad=pad_before, dtype=np.float64):
    """shape: the fine volume with its channels, [D,H,W,C] or [H,W,C]"""
    lo, k = np.asarray(lo, dtype=dtype), np.asarray(k, dtype=dtype)
    shape = tuple(int(s) for s in shape)
    dims, nd = shape[:-1], len(shape) - 1
    assert k.shape == (5,) * nd and lo.shape == tuple(out_len(n) for n in dims) + shape[-1:], (lo.shape, shape)
    P = np.zeros(_padded(dims, pad) + shape[-1:], dtype=dtype)
    for tap in np.ndindex(*k.shape):
        P[_tap_slices(dims, tap)] += k[tap] * lo
    return P[tuple(slice(pad(n), pad(n) + n) for n in dims)].copy()


def taps(nd):
    return (125, 27) if nd == 3 else (25, 9)


def down_bound(x, k):
    return (taps(np.ndim(x) - 1)[0] + 1) * EPS * down(np.abs(_f64(x)), np.abs(_f64(k)))


def up_terms(lo, k, shape, bound=True):
    """(up(lo, k), up(|lo|, |k|)): what every value and bound of nfs_lap_up / nfs_lap_up_rms on one (lo, k) is made of;
    the tests that run many scales and addends on one input compute it once and pass it as ``terms``.  bound=False (the
    whole-number cases, which are held to equality): the second is a zero"""
    return up(lo, k, shape), (up(np.abs(_f64(lo)), np.abs(_f64(k)), shape) if bound else np.zeros(1))


def up_bound(lo, k, shape, scale, a=None, terms=None):
    """a: the addend term as it enters the sum (None: no addend)"""
    mag = abs(float(scale)) * (terms or up_terms(lo, k, shape))[1]
    if a is not None:
        mag = mag + np.abs(_f64(a))
    return (taps(len(shape) - 1)[1] + 3) * EPS * mag


def up_scaled(lo, k, shape, scale, addend=None, terms=None):
    """nfs_lap_up: (scale * up(lo) + addend, bound)"""
    terms = terms or up_terms(lo, k, shape)
    out = float(scale) * terms[0]
    if addend is not None:
        out = out + _f64(addend)
    return out, up_bound(lo, k, shape, scale, addend, terms)


def amul(addend_part, addend_n, eps):
    """1 / max(sqrt(sum(addend_part) / addend_n), eps) from the float32 partial sums and the float32 eps as given"""
    return 1.0 / max(float(np.sqrt(_f64(addend_part).sum() / float(addend_n))), float(np.float32(eps)))


def up_rms(lo, k, shape, scale, addend, addend_part, addend_n, eps, terms=None):
    """nfs_lap_up_rms with addend_part: (scale * up(lo) + addend / max(rms, eps), bound)"""
    terms = terms or up_terms(lo, k, shape)
    a = _f64(addend) * amul(addend_part, addend_n, eps)
    return float(scale) * terms[0] + a, up_bound(lo, k, shape, scale, a, terms) + 4 * EPS * np.abs(a)


def part_sum_bound(shape, cell=False):
    """relative bound of sum(out_part) against the float64 sum of squares of the kernel's own float32 out: a block owns at
    most 8 W C outputs (rows: 2 rows of y, 4 planes of z, all of x) or 2048 C (cells: 256 cells of 8 voxels), every term is
    positive, and the partial sums themselves are added in float64 by the test"""
    return ((2048 if cell else 8 * shape[-2]) * shape[-1] + 1) * EPS


def norm_parts(n):
    return min(1024, -(-int(n) // 2048))


def normalize_mean(x, use_abs, eps):
    """(x / max(m, eps), bound): m = mean |x| (use_abs) or sqrt(mean x^2); eps as the float32 the kernel takes"""
    x = _f64(x)
    n = x.size
    m = np.abs(x).sum() / n if use_abs else np.sqrt((x * x).sum() / n)
    out = x / max(float(m), float(np.float32(eps)))
    terms = -(-n // norm_parts(n))
    rel = (terms + 4) * EPS if use_abs else (terms / 2.0 + 5) * EPS
    return out, rel * np.abs(out)


def n_cells(n):
    """2 x 2 x 2 cells m = (p >> 1) .. floor((n - 1 + p) / 2) of an axis: the fine voxels 2 m - p and 2 m - p + 1"""
    p = pad_before(n)
    return (n - 1 + p) // 2 - (p >> 1) + 1


def expected_parts(shape, cell=False):
    """what nfs_lap_up_rms_parts must return for the fine volume ``shape`` ([D,H,W,C] / [H,W,C]) = which kernel nfs_lap_up
    takes: the row form (3-D, 1 or 3 channels, from 4096 voxels on, while its 12 staged coarse rows fit 60 KB of LDS): one
    block per cell row of y and pair of cells of z; ``cell`` (the process runs with NFS_LAP_UP=cell): the cell form from
    2^21 voxels on, one block per 16 x 4 x 4 cells, and no row form; 0: the gather form"""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 4 or shape[-1] not in (1, 3):
        return 0
    D, H, W, C = shape
    if cell:
        if D * H * W < CELL_MIN_VOXELS:
            return 0
        return -(-n_cells(W) // 16) * -(-n_cells(H) // 4) * -(-n_cells(D) // 4)
    if D * H * W < ROW_MIN_VOXELS or ROW_STAGED_ROWS * out_len(W) * C * 4 > ROW_LDS_BYTES:
        return 0
    return n_cells(H) * -(-n_cells(D) // 2)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def tap_kernel(nd):
    return (1 + np.arange(5 ** nd)).reshape((5,) * nd).astype(np.float32)


def integers(rng, shape):
    return rng.randint(-INT_RANGE, INT_RANGE + 1, tuple(shape)).astype(np.float32)


def randn(rng, shape):
    return rng.randn(*shape).astype(np.float32)


def coarse(shape):
    """the shape of down's output for the fine ``shape`` (channels last)"""
    return tuple(out_len(n) for n in shape[:-1]) + tuple(shape[-1:])


def case(shape, kind, k_prod, seed=0):
    """(k, x, lo, addend, rng) float32 for the fine volume ``shape``: kind 'int' -- tap_kernel and whole numbers, on which
    float32 is exact -- or 'randn' -- the production kernel ``k_prod`` and normal data"""
    shape = tuple(shape)
    rng = np.random.RandomState((sum(shape) * 977 + int(np.prod(shape)) * 13 + seed) % (2 ** 31))
    draw = integers if kind == "int" else randn
    k = tap_kernel(len(shape) - 1) if kind == "int" else np.asarray(k_prod, np.float32)
    return k, draw(rng, shape), draw(rng, coarse(shape)), draw(rng, shape), rng


def check(got, want, bound):
    """largest |got - want| / bound over the elements (field_ref.err_ratio: 0 where equal, inf where an error meets a zero
    bound or is not a number); the shapes must agree"""
    got, want = _f64(got), _f64(want)
    assert got.shape == want.shape == np.shape(bound), (got.shape, want.shape, np.shape(bound))
    return err_ratio(np.where(np.isfinite(got), np.abs(got - want), np.nan), bound)


# ---- the cases both test files run ------------------------------------------------------------------------------------
KINDS = ("int", "randn")
SCALES = (5.0, -5.0)
GATHER_2D = [(h, w) for h in range(1, 10) for w in range(1, 10)]                  # C = 1, 2
GATHER_3D_AXIS = (1, 2, 3, 4, 5, 8, 9)
GATHER_3D = [(d, h, w) for d in GATHER_3D_AXIS for h in GATHER_3D_AXIS for w in GATHER_3D_AXIS]      # C = 2, 4
GATHER_3D_SMALL = [(16, 16, 15), (1, 1, 1), (2, 3, 4)]                            # C = 1, 3: under the row form's threshold
# lap_down3_tiled_kernel (4 x 4 x 16 outputs a block): ceil(n / 2) either side of the tile edges, a single partial tile,
# ragged last tiles on every axis
TILED = [(1, 1, 1), (1, 1, 40), (2, 3, 4), (9, 7, 33), (8, 9, 65), (17, 16, 16), (21, 19, 37)]
# lap_up3_row_kernel: the threshold, the parity mixes, three passes of the 320-lane x loop with a ragged last and an odd
# number of z cells (C = 3 only), degenerate axes, the widest rows the plan accepts (per C)
ROW = ([(s, C) for s in [(16, 16, 16), (17, 16, 16), (16, 17, 65), (21, 19, 37)] for C in (1, 3)] + [((5, 8, 231), 3)]
       + [(s, C) for s in [(1, 64, 64), (64, 1, 64), (64, 64, 1)] for C in (1, 3)]
       + [((2, 2, 1024), 1), ((4, 4, 852), 3), ((2, 2, 2560), 1)])
# one voxel wider: the gather form; so is (2,2,1024) with three channels (12 rows of 512 x 3 floats are 72 KB)
ROW_TOO_WIDE = [((4, 4, 853), 3), ((2, 2, 2561), 1), ((2, 2, 1024), 3)]
ADDEND_NPARTS = (1, 64, 255, 256, 257, 300, 320, 321, 641, 1024)
ENERGY_SLOTS = (0, 255, 256, 319, 320, -1)
# lap_up3_cell_kernel (NFS_LAP_UP=cell, from 2^21 voxels): (129,127,128) is 128 voxels short of 2^21 and must stay on the
# gather form; (129,128,128) is the one-channel volume the cell form does take
CELL = [((127, 130, 129), 3), ((129, 127, 128), 1), ((129, 128, 128), 1)]
NORM_NS = (1, 3, 4, 5, 7, 2047, 2048, 2049, 4099, 1024 * 2048 + 5, 1025 * 2048 + 3)


def energy_slots(nparts):
    return sorted({s % nparts for s in ENERGY_SLOTS if -nparts <= s < nparts})


def addend_parts(rng, nparts, total, slot=None):
    """float32 partial sums: random positive ones scaled to add up to about ``total``, or all of it in one ``slot``"""
    if slot is None:
        p = rng.uniform(0.5, 1.5, nparts)
        return (p * (total / p.sum())).astype(np.float32)
    p = np.zeros(nparts, np.float32)
    p[slot] = total
    return p

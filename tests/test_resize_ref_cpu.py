"""tests/resize_ref.py (the NumPy restatement of nfs_resize3d and of util.resize_tf / rescale_tf) pinned by its
properties, without TensorFlow: identity at equal size, exact interpolation of what the legacy kernels interpolate
exactly, the corner alignment the grid octaves rely on, the nearest indices, the rescale sizes, and float32 against
float64."""
import numpy as np
import pytest

from tests import resize_ref as R

METHODS = ("nearest", "bilinear")


def _field(shape, seed=0):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("align", (False, True))
def test_equal_size_is_the_identity_bit_for_bit(method, align):
    for shape in ((9, 12, 10, 3), (1, 4, 3, 1), (5, 6, 7)):
        x = _field(shape)
        y = R.resize3d(x, shape[:3], method, align)
        assert y.dtype == np.float32 and y.shape == x.shape
        assert np.array_equal(y.view(np.uint32), x.view(np.uint32))


def test_bilinear_upsample_by_two_returns_the_input_at_the_even_nodes():
    x = _field((9, 12, 10, 3), 1)
    y = R.resize3d(x, (18, 24, 20), "bilinear", False)
    assert np.array_equal(y[::2, ::2, ::2].view(np.uint32), x.view(np.uint32))


def test_linear_field_is_interpolated_exactly_and_clamped_past_the_last_node():
    D, H, W = 6, 7, 5
    a, b, c, e = 3.0, -2.0, 5.0, 7.0
    lin = lambda d, h, w: a * d + b * h + c * w + e
    x = lin(*np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")).astype(np.float32)
    y = R.resize3d(x, (2 * D, 2 * H, 2 * W), "bilinear", False)
    i, j, k = np.meshgrid(np.arange(2 * D), np.arange(2 * H), np.arange(2 * W), indexing="ij")
    want = lin(np.minimum(i / 2.0, D - 1), np.minimum(j / 2.0, H - 1), np.minimum(k / 2.0, W - 1))
    assert np.array_equal(y, want.astype(np.float32))
    inside = (i / 2.0 <= D - 1) & (j / 2.0 <= H - 1) & (k / 2.0 <= W - 1)
    assert np.array_equal(y[inside], lin(i / 2.0, j / 2.0, k / 2.0)[inside].astype(np.float32))
    assert inside.sum() < inside.size                        # (the clamped part exists)


@pytest.mark.parametrize("n_in,n_out", [(7, 13), (11, 20), (13, 24), (61, 111), (111, 200)])
def test_align_corners_last_node_reads_the_last_node(n_in, n_out):
    lo, hi, t = R.axis_table(n_in, n_out, "bilinear", True)
    assert lo[0] == 0 and t[0] == 0
    assert lo[-1] == n_in - 1 and hi[-1] == n_in - 1 and t[-1] == 0
    assert ((t >= 0) & (t < 1)).all() and (hi - lo <= 1).all() and (lo <= n_in - 1).all()
    x = _field((n_in, 2, 2, 1), n_in)
    y = R.resize3d(x, (n_out, 2, 2), "bilinear", True)
    assert np.array_equal(y[-1], x[-1]) and np.array_equal(y[0], x[0])


@pytest.mark.parametrize("n_in,n_out", [(9, 5), (5, 9), (12, 7), (10, 31), (4, 1), (1, 3)])
def test_nearest_indices(n_in, n_out):
    i = np.arange(n_out, dtype=np.float32)
    s = np.float32(n_in) / np.float32(n_out)
    lo, hi, t = R.axis_table(n_in, n_out, "nearest", False)
    assert np.array_equal(lo, np.minimum(np.floor(i * s).astype(int), n_in - 1)) and np.array_equal(lo, hi)
    assert not t.any()
    sa = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else s
    lo, _, _ = R.axis_table(n_in, n_out, "nearest", True)
    p = (i * sa).astype(np.float64)
    rnd = np.where(p - np.floor(p) >= 0.5, np.floor(p) + 1, np.floor(p))       # C roundf: halves away from zero
    assert np.array_equal(lo, np.minimum(rnd.astype(int), n_in - 1))
    x = _field((n_in, 1, 1, 2), 5)
    assert np.array_equal(R.resize3d(x, (n_out, 1, 1), "nearest", True, 1.75), x[lo] * np.float32(1.75))


def test_nearest_round_is_half_away_from_zero():
    # 5 -> 9 with align_corners: s = 0.5, p = 0, .5, 1, 1.5, ...: halves go up (np.round would send 0.5 and 2.5 down)
    lo, _, _ = R.axis_table(5, 9, "nearest", True)
    assert list(lo) == [0, 1, 1, 2, 2, 3, 3, 4, 4]


def test_rescale_sizes_are_the_float32_casts():
    assert R.rescale_size((200, 111, 61), 1.8) == [int(np.float32(n) * np.float32(1.8)) for n in (200, 111, 61)]
    assert R.rescale_size((10, 10), 0.3) == [3, 3] and R.rescale_size((9, 12, 10), 2) == [18, 24, 20]
    x = _field((2, 9, 12, 10, 3), 2)
    assert R.rescale_tf(x, 0.55, is_3d=True).shape == (2, 4, 6, 5, 3)
    assert np.array_equal(R.rescale_tf(x, 0.55, is_3d=True), R.resize_tf(x, (4, 6, 5), "bilinear", True))
    assert R.rescale_tf(x[:, 0], 1.75).shape == (2, 21, 17, 3)
    # an image is a volume of depth 1
    assert np.array_equal(R.resize_tf(x[:, 0], (7, 15), "bilinear")[1], R.resize3d(x[1, :1], (1, 7, 15), "bilinear")[0])
    assert R.resize_tf(x[:, 0], (7, 15)).shape == (2, 7, 15, 3)                # (default: nearest)


@pytest.mark.parametrize("size", [(5, 6, 5), (16, 21, 18), (18, 24, 20), (2, 30, 3)])
@pytest.mark.parametrize("align", (False, True))
def test_float32_against_float64(size, align):
    """bound: three axes, each with a weight error of at most 2 n_in 2^-24 (the two float32 roundings of the coordinate)
    times a neighbour difference of at most 2 max|x|, plus the lerp roundings: (12 n_max + 16) 2^-24 max|x|"""
    x = _field((9, 12, 10, 3), 3)
    a = R.resize3d(x, size, "bilinear", align, 1.0, np.float32)
    b = R.resize3d(x, size, "bilinear", align, 1.0, np.float64)
    assert a.dtype == np.float32 and b.dtype == np.float64
    m = np.abs(x).max()
    err = np.abs(a.astype(np.float64) - b).max()
    print("float32 vs float64: %.3g of max|x| (bound %.3g)" % (err / m, (12 * 12 + 16) * 2.0 ** -24))
    assert err <= (12 * 12 + 16) * 2.0 ** -24 * m
    assert np.array_equal(R.resize3d(x, size, "nearest", align, 1.0, np.float32),
                          R.resize3d(x, size, "nearest", align, 1.0, np.float64).astype(np.float32))


def test_potential_factor_keeps_the_differences_of_a_linear_potential():
    # phi = c * node index along W at 11 nodes -> 20 nodes, corner-aligned: the forward difference is c again
    assert R.potential_factor((11, 11, 11), (20, 20, 20)) == np.float32(1.9)
    phi = np.broadcast_to(np.arange(11, dtype=np.float32) * 0.25, (11, 11, 11))
    up = R.resize3d(phi, (20, 20, 20), "bilinear", True, R.potential_factor((11, 11, 11), (20, 20, 20)))
    np.testing.assert_allclose(np.diff(up, axis=-1), 0.25, rtol=1e-5)

"""nfs_resize3d on the device: its bits equal the float32 restatement (tests/resize_ref.py), and util.resize_tf /
rescale_tf equal theirs."""
import numpy as np
import pytest
import torch

from tests import resize_ref as R

pytestmark = pytest.mark.gpu

# input -> output: the smallest shapes that still reach every branch
SHAPES = [((1, 1, 1), (1, 1, 1)),            # a single voxel
          ((2, 2, 2), (3, 3, 3)),            # one cell, upsampled
          ((9, 12, 10), (5, 6, 5)),          # the octave ratio, downwards
          ((5, 6, 5), (9, 12, 10)),          # the octave ratio, upwards
          ((4, 6, 70), (7, 11, 126)),        # rows longer than a wave
          ((16, 16, 16), (8, 8, 8)),         # an exact 2x reduction
          ((1, 4, 3), (3, 4, 5)),            # an input axis of length 1
          ((4, 5, 6), (1, 1, 1))]            # an output axis of length 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("shape,size", SHAPES, ids=["%dx%dx%d-%dx%dx%d" % (a + b) for a, b in SHAPES])
@pytest.mark.parametrize("C", (1, 3, 4, 2))
def test_kernel_bits_equal_the_float32_restatement(shape, size, C):
    from neural_flow_style_amd import ops
    x = np.random.RandomState(sum(shape) + C).randn(*shape, C).astype(np.float32)
    xd = torch.tensor(x).cuda()
    for method in ("bilinear", "nearest"):
        for align in (False, True):
            for scale in (1.0, 1.75):
                got = ops.resize3d(xd, size, method, align, scale).cpu().numpy()
                want = R.resize3d(x, size, method, align, scale, np.float32)
                assert got.shape == want.shape == tuple(size) + (C,)
                bad = _bits(got) != _bits(want)
                assert not bad.any(), (method, align, scale, int(bad.sum()), float(np.abs(got - want).max()))
    if C == 1:                                                   # [D,H,W] goes as one channel
        got = ops.resize3d(xd[..., 0].contiguous(), size, "bilinear", True, 1.75).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(R.resize3d(x[..., 0], size, "bilinear", True, 1.75)))


def test_four_channels_off_a_16_byte_boundary():
    """a contiguous view that starts 4 bytes into its storage: the 16-byte store is not taken"""
    from neural_flow_style_amd import ops
    x = np.random.RandomState(0).randn(5, 6, 5, 4).astype(np.float32)
    buf = torch.zeros(x.size + 1).cuda()
    buf[1:] = torch.tensor(x).reshape(-1).cuda()
    got = ops.resize3d(buf[1:].view(5, 6, 5, 4), (9, 12, 10), "bilinear", True).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(R.resize3d(x, (9, 12, 10), "bilinear", True)))


def test_util_resize_tf_and_rescale_tf_equal_the_restatement():
    from neural_flow_style_amd import util
    rng = np.random.RandomState(7)
    v = rng.randn(2, 9, 12, 10, 3).astype(np.float32)
    img = rng.randn(2, 12, 10, 3).astype(np.float32)
    vd, imd = torch.tensor(v).cuda(), torch.tensor(img).cuda()
    for method in ("nearest", "bilinear"):
        got = util.resize_tf(vd, (5, 6, 5), method, is_3d=True).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(R.resize_tf(v, (5, 6, 5), method, True)))
        got = util.rescale_tf(vd, 1.8, method, is_3d=True).cpu().numpy()
        assert got.shape == (2, 16, 21, 18, 3)
        assert np.array_equal(_bits(got), _bits(R.rescale_tf(v, 1.8, method, True)))
        got = util.resize_tf(imd, (7, 15), method).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(R.resize_tf(img, (7, 15), method)))
        got = util.rescale_tf(imd, 0.55, method).cpu().numpy()
        assert got.shape == (2, 6, 5, 3)
        assert np.array_equal(_bits(got), _bits(R.rescale_tf(img, 0.55, method)))
    # the defaults are the reference's: nearest for resize_tf, bilinear for rescale_tf
    assert np.array_equal(util.resize_tf(imd, (7, 15)).cpu().numpy(), R.resize_tf(img, (7, 15), "nearest"))
    assert np.array_equal(util.rescale_tf(imd, 1.75).cpu().numpy(), R.rescale_tf(img, 1.75, "bilinear"))
    # bicubic stays with the legacy bicubic kernel (images only)
    from neural_flow_style_amd import ops
    assert torch.equal(util.resize_tf(imd, (7, 15), "bicubic"), ops.resize_bicubic_tf1(imd, 7, 15))


def test_unsupported_method_raises():
    from neural_flow_style_amd import ops, util
    x = torch.zeros(2, 3, 4, 5, 1).cuda()
    with pytest.raises(ValueError):
        ops.resize3d(x[0], (2, 2, 2), "area")
    with pytest.raises(ValueError):
        util.resize_tf(x, (2, 2, 2), "lanczos3", is_3d=True)
    with pytest.raises(ValueError):
        util.resize_tf(x, (2, 2, 2), "bicubic", is_3d=True)
    with pytest.raises(ValueError):
        util.rescale_tf(x[0], 2.0, "area")

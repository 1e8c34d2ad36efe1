"""The kernels of libnfs_descent.so (csrc/descent.hip) element by element, and util.lap_normalize on the channel counts and
shapes optimizer 'lapnorm' brings.  5 x 6 x 7 and 9 x 11 x 13 have neither a multiple-of-four voxel count nor a full wave (the
reference stencil, one voxel per lane); 8 x 8 x 16 takes the lean four-voxel path.  Velocities reach three cells, so traces
leave the domain and hit the border clamp."""
import functools

import numpy as np
import pytest
import torch

from tests import lapnorm_ref as R

pytestmark = pytest.mark.gpu
SHAPES3 = [(5, 6, 7), (9, 11, 13), (8, 8, 16)]
SHAPES2 = [(7, 9), (16, 32)]
LR = 0.37


def T(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def same(a, b):
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def case(shape):
    """density with plateaus (zeros) and structure, a velocity of up to three cells per axis, a gradient of about that size"""
    rng = np.random.RandomState(sum(shape))
    d = rng.rand(*shape).astype(np.float32)
    d[d < 0.3] = 0.0
    cells = 2.0 / (np.array(shape, np.float64) - 1.0)
    vel = (rng.uniform(-3, 3, shape + (len(shape),)) * cells).astype(np.float32)
    g = (rng.randn(*shape, len(shape)) * cells * 2.0).astype(np.float32)
    return d, vel, g


# ---- nfs_descent_step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 255, 256, 1027, 4 * 256 * 3 + 2, 70001])
def test_descent_step_is_one_fused_multiply_add_per_element(n):
    from neural_flow_style_amd import ops
    rng = np.random.RandomState(n)
    x, g = rng.randn(n).astype(np.float32), (rng.randn(n) * 3).astype(np.float32)
    for off in (0, 1):                         # (a view one float into its storage: the unaligned, one-float-per-lane form)
        xb, gb = torch.zeros(n + 1).cuda(), torch.zeros(n + 1).cuda()
        xd, gd = xb[off:off + n], gb[off:off + n]
        xd.copy_(T(x)); gd.copy_(T(g))
        v0 = xd._version
        ops.descent_step(xd, gd, LR)
        ok, worst = R.one_rounding(xd.cpu().numpy(), x, LR, g)
        print("n %d offset %d: worst %.3f of the bound" % (n, off, worst))
        assert ok and xd._version > v0 and same(gd, T(g))
        if off == 0:
            assert float(xb[n]) == 0.0                         # nothing past the end
        x0 = T(x)
        ops.descent_step(x0, gd, 0.0)
        assert same(x0, T(x))                                 # lr = 0: x unchanged bit for bit


# ---- the fused kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES3)
def test_advect_descent_is_descent_step_then_advect_bit_for_bit(shape):
    from neural_flow_style_amd import ops
    d, vel, g = case(shape)
    D, H, W = shape
    takes_mask = (D * H * W) % 4 == 0          # (where nfs_advect_fwd_live does)
    want_v = T(vel)
    ops.descent_step(want_v, T(g), LR)
    assert not same(want_v, T(vel))
    live_w = ops.live_mask(D, H, W, like=want_v) if takes_mask else None
    want_a = ops.advect_fwd(T(d)[..., None], want_v, live=live_w).squeeze(-1)
    want_plain = ops.advect_fwd(T(d)[..., None], want_v).squeeze(-1)
    assert same(want_a, want_plain)
    outs = []
    for with_mask in ((True, False) if takes_mask else (False,)):
        for _ in range(2):                     # a second call with the same inputs: the same bits
            v = T(vel)
            adv = torch.full(shape, float("nan")).cuda()
            live = ops.live_mask(D, H, W, like=v) if with_mask else None
            if live is not None:
                live.view(torch.int32).fill_(-1)
            ver = (v._version, adv._version)
            ops.advect_descent(T(d), v, T(g), LR, adv, live)
            assert v._version > ver[0] and adv._version > ver[1]
            assert same(v, want_v), "vel is nfs_descent_step's"
            assert same(adv, want_a), "adv_next is nfs_advect_fwd's on the new velocity"
            if live is not None:
                assert same(live, live_w), "the mask is nfs_advect_fwd_live's"
            outs.append(adv)
    assert bool(torch.isfinite(outs[0]).all())
    if not takes_mask:
        from neural_flow_style_amd import _lib
        with pytest.raises(_lib.NfsError, match="multiple of 4"):
            ops.advect_descent(T(d), T(vel), T(g), LR, torch.empty(shape).cuda(), torch.zeros(64).cuda())


def test_traces_leave_the_domain_in_the_cases_above():
    """(what the shapes are for: some back-traced points lie outside on every axis, some cross a cell)"""
    for shape in SHAPES3 + SHAPES2:
        _, vel, g = case(shape)
        v = vel.astype(np.float64) - LR * g
        idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
        x = idx - v * (np.array(shape) - 1) / 2.0
        for k, n in enumerate(shape):
            assert (x[..., k] < 0).any() and (x[..., k] > n - 1).any(), (shape, k)


@pytest.mark.parametrize("shape", SHAPES2)
def test_advect2d_descent_is_descent_step_then_advect2d_bit_for_bit(shape):
    from neural_flow_style_amd import ops
    d, vel, g = case(shape)
    want_v = T(vel)
    ops.descent_step(want_v, T(g), LR)
    want_a = ops.advect2d_fwd(T(d)[..., None], want_v).squeeze(-1)
    for _ in range(2):
        v, adv = T(vel), torch.full(shape, float("nan")).cuda()
        ops.advect2d_descent(T(d), v, T(g), LR, adv)
        assert same(v, want_v) and same(adv, want_a)
    assert same(want_a, ops.advect2d_source_fwd("v", T(d), want_v))


# ---- util.lap_normalize on the new channel counts and shapes ---------------------------------------------------------------
@pytest.mark.parametrize("lap_n", [0, 1, 3])
@pytest.mark.parametrize("shape,is_3d", [(s + (4,), True) for s in SHAPES3] + [(s + (1,), True) for s in SHAPES3]
                         + [(s + (2,), False) for s in SHAPES2] + [(s + (1,), False) for s in SHAPES2])
def test_lap_normalize_on_the_channel_counts_of_the_grid_variables(shape, is_3d, lap_n):
    """[D,H,W,4] (the Helmholtz pair), [D,H,W,1] (a [D,H,W] potential or density), [H,W,2], [H,W,1] against the float64
    oracle at the bar tests/test_grid_ops_gpu.py holds for C = 1 and 3"""
    from neural_flow_style_amd import engine, util
    g = np.random.RandomState(len(shape) + shape[0]).randn(*shape).astype(np.float32)
    want = R.normalized(g, lap_n, is_3d)
    got = util.lap_normalize(T(g), scale_n=lap_n, is_3d=is_3d, c=shape[-1])
    r = R.rel(got.cpu().numpy(), want)
    print("%s lap_n %d: rel L2 %.2e" % (shape, lap_n, r))
    assert tuple(got.shape) == shape and r < 2e-5
    if shape[-1] == 1:                         # the variable without its channel axis, as the stylizers hold it
        st = engine.LapDescentState(lap_n=lap_n, nd=3 if is_3d else 2)
        assert same(st.normalized(T(g[..., 0])), got)
    zero = util.lap_normalize(torch.zeros(shape).cuda(), scale_n=lap_n, is_3d=is_3d, c=shape[-1])
    assert bool(torch.isfinite(zero).all()) and not bool(zero.any())

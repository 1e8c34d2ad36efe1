"""The 2-D grid stylizer's kernels (csrc/grid2d.hip) element by element: against the float64 restatements of
tests/field_ref.py and tests/grid2d_ref.py within their derived bounds, and bit for bit against the compositions they
replace.  No pixel is left out; where field_ref reports two candidates next to a cell face either is accepted.  Every
check prints the largest err / bound it saw (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

from tests import field_ref as FR
from tests import grid2d_ref as R

pytestmark = pytest.mark.gpu
# (33, 70): 2310 pixels, several blocks and a ragged tail; (64, 64): a multiple of everything
SHAPES = [(2, 2), (2, 9), (5, 7), (13, 18), (33, 70), (64, 64)]
KINDS = R.KINDS
LR_T = float(np.float32(3e-3))
ADAM = (FR.B1, FR.B2, FR.ADAM_EPS)
K_TRANSPOSE = 9 * 2.0 ** -23          # the constant the 3-D transposes are held to (tests/test_source_variables_gpu.py)


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


def T(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def same(a, b):
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def check(name, got, ref, bound):
    r = FR.err_ratio(np.abs(np.asarray(got, dtype=np.float64) - ref), bound)
    print("%-72s max err/bound %.3g" % (name, r))
    assert r <= 1.0, (name, r)


def _sid(s):
    return "x".join(map(str, s))


def density(shape, rng):
    """plateaus (clipped at 1) and exact zeros; the two smallest shapes: quarters with zeros"""
    H, W = shape
    if min(shape) < 4:
        return (rng.randint(0, 5, shape) / 4.0).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r2 = ((yy - H / 2) / (H / 3.0)) ** 2 + ((xx - W / 2) / (W / 3.0)) ** 2
    d = np.clip(2.5 * np.exp(-3.0 * r2), 0, 1).astype(np.float32)
    d[d < 0.05] = 0.0
    assert (d == 0).any() and (d == 1).any()
    return d


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(d [H,W], var, g [H,W]) float32: a smooth variable whose velocity reaches 2.5 cells, with bumps next to every border
    that trace a handful of pixels beyond it"""
    H, W = shape
    rng = np.random.RandomState(H * 131 + W * 7 + KINDS.index(kind))
    var = R.make_var(kind, H, W, 2.5, H + W + KINDS.index(kind))
    cell = np.asarray([2.0 / (H - 1), 2.0 / (W - 1)], np.float32)
    for (y, x) in ((0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1), (0, 0), (H - 1, W - 1)):
        if kind == "v":
            var[y, x] = cell * np.asarray([4.0 if y == 0 else -4.0, 4.0 if x == 0 else -4.0], np.float32)
            var[y, x] *= np.asarray([y in (0, H - 1), x in (0, W - 1)], np.float32)
        else:
            var[y, x] += np.float32(4.0 * cell.min())
    return density(shape, rng), var, rng.randn(H, W).astype(np.float32)


def test_cases_trace_beyond_every_border():
    for shape in SHAPES[2:]:
        H, W = shape
        for kind in KINDS:
            _, var, _ = case(shape, kind)
            vel = R.velocity(kind, var).astype(np.float64)
            y = (np.arange(H)[:, None] - vel[..., 0] * (H - 1) / 2)
            x = (np.arange(W)[None, :] - vel[..., 1] * (W - 1) / 2)
            assert (y < 0).any() and (y > H - 1).any() and (x < 0).any() and (x > W - 1).any(), (shape, kind)
            cells = np.abs(vel) * (np.asarray(shape) - 1) / 2
            assert cells.max() >= 2.4


# ---- 1, 2: the velocity and the forward sample -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_velocity_fwd_is_the_float32_restatement_bit_for_bit(ops, shape):
    for kind in KINDS:
        _, var, _ = case(shape, kind)
        assert same(ops.source2d_velocity(kind, T(var)), T(R.velocity(kind, var))), kind


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_advect2d_source_fwd(ops, shape):
    for kind in KINDS:
        d, var, _ = case(shape, kind)
        out = ops.advect2d_source_fwd(kind, T(d), T(var))
        vel = ops.source2d_velocity(kind, T(var))
        assert same(out, ops.advect2d_fwd(T(d[..., None]), vel)[..., 0]), kind
        s, b = FR.sample(d[..., None], N(vel))
        check("advect2d_source_fwd %s %s" % (_sid(shape), kind), N(out)[..., None], s, b)


# ---- 3: the transpose --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_velocity_bwd(ops, shape):
    H, W = shape
    g = np.random.RandomState(H + W).randn(H, W, 2).astype(np.float32)
    for kind in KINDS:
        got = ops.source2d_velocity_bwd(kind, T(g))
        assert tuple(got.shape) == R.var_shape(kind, H, W)
        ref, A = R.velocity_T(kind, g.astype(np.float64)), R.velocity_T(kind, g.astype(np.float64), absolute=True)
        check("source2d_velocity_bwd %s %s" % (_sid(shape), kind), N(got), ref, K_TRANSPOSE * A)
        assert same(got, ops.source2d_velocity_bwd(kind, T(g))), kind


# ---- 4: the velocity gradient of the advect ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_advect2d_source_bwd(ops, shape):
    for kind in KINDS:
        d, var, g = case(shape, kind)
        gv = ops.advect2d_source_bwd(kind, T(d), T(var), T(g))
        vel = ops.source2d_velocity(kind, T(var))
        none_d, gv0 = ops.advect2d_bwd(T(d[..., None]), vel, T(g[..., None]), need_d=False, need_vel=True)
        assert none_d is None and same(gv, gv0), kind
        ref = FR.advect_adjoint(d[..., None], N(vel), g[..., None])
        r = FR.vel_ratio(ref, N(gv))
        print("advect2d_source_bwd %-10s %-3s max err/bound %.3g (%d pixels with two candidates)" % (
            _sid(shape), kind, r, int(ref["unsure"].sum())))
        assert r <= 1.0, (kind, r)


# ---- 5: the fused update of the velocity variable --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_advect2d_bwd_adam_is_applyadam_on_the_kernels_own_gradient(ops, shape):
    H, W = shape
    d, v0, g = case(shape, "v")
    rng = np.random.RandomState(H * W)
    dt, vel = T(d), T(v0)
    m, u = T((rng.randn(H, W, 2) * 0.1).astype(np.float32)), T((rng.rand(H, W, 2) * 0.01).astype(np.float32))
    adv = torch.full((H, W), float("nan"), device="cuda")
    for step, scale in enumerate((1.0, 1e-7, 1.0)):                  # (the second step: gradients near 1e-7)
        gt = T((g * np.float32(scale)).astype(np.float32))
        g_vel = N(ops.advect2d_source_bwd("v", dt, vel, gt))
        x1, m1, u1, bx, bm, bv = FR.adam(N(vel), N(m), N(u), g_vel, LR_T, *ADAM)
        ops.advect2d_bwd_adam(dt, vel, gt, m, u, LR_T, *ADAM, adv_next=adv if step != 1 else None)
        name = "advect2d_bwd_adam %s step %d" % (_sid(shape), step)
        check(name + " m", N(m), m1, bm)
        check(name + " v", N(u), u1, bv)
        check(name + " vel", N(vel), x1, bx)
        if step != 1:
            assert same(adv, ops.advect2d_fwd(dt.unsqueeze(-1), vel)[..., 0])


# ---- 6: one frame crossing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_transport_step2d(ops, shape, C):
    H, W = shape
    _, u, _ = case(shape, "v")
    rng = np.random.RandomState(H + W + C)
    g, add = (rng.randn(H, W, C) * 2.0 - 0.5).astype(np.float32), rng.randn(H, W, C).astype(np.float32)
    w_g, w_add = FR.TRANSPORT_W_G, FR.TRANSPORT_W_ADD
    for scale in (1.0, -1.0, 2.0):
        for with_add in (True, False):
            got = ops.transport_step2d(T(g), T(u), scale, w_g, T(add) if with_add else None, w_add if with_add else 0.0)
            ref, b = FR.transport(g, u, scale, w_g, add if with_add else None, w_add if with_add else 0.0,
                                  stencil="lean")
            check("transport_step2d %s C%d scale %+g addend %d" % (_sid(shape), C, scale, with_add), N(got), ref, b)


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    from neural_flow_style_amd import _lib
    L, L0 = _lib.side("grid2d"), _lib.lib()       # (the error text is libnfs_hip.so's: one channel for both libraries)
    SENT = 12345.0
    H, W = 4, 6
    n = H * W

    def buf(k=2):
        return torch.full((n * k,), SENT, device="cuda")

    def P(t):
        return t.data_ptr()

    src_in = torch.zeros(n * 2, device="cuda")
    d = torch.zeros(n, device="cuda")
    h = (0.1, 0.9, 0.999, 1e-8)

    def calls(H, W, src, null):
        """every entry point with these dims / src; ``null``: its first required pointer missing"""
        outs = [buf() for _ in range(7)]
        m, v = buf(), buf()
        first = None if null else P(src_in)
        codes = [
            L.nfs_source2d_velocity_fwd(first, src, P(outs[0]), H, W, None),
            L.nfs_source2d_velocity_bwd(first, src, P(outs[1]), H, W, None),
            L.nfs_advect2d_source_fwd(None if null else P(d), P(src_in), src, P(outs[2]), H, W, None),
            L.nfs_advect2d_source_bwd(None if null else P(d), P(src_in), src, P(d), P(outs[3]), H, W, None)]
        if src == 0:                                   # (the two entry points without a src argument)
            codes += [
                L.nfs_advect2d_bwd_adam_fwd(None if null else P(d), P(outs[5]), P(d), P(m), P(v), P(outs[6]), H, W, *h,
                                            None),
                L.nfs_transport_step2d(first, P(src_in), 1.0, 1.0, None, 0.0, P(outs[6]), H, W, 1, None)]
        return outs + [m, v], codes

    for (hh, ww, src, null) in ((1, 6, 0, False), (4, 1, 0, False), (1, 6, 2, False), (H, W, 0, True), (H, W, 3, True),
                                (H, W, 4, False), (H, W, -1, False)):
        written, codes = calls(hh, ww, src, null)
        torch.cuda.synchronize()
        assert all(c == _lib.NFS_EINVAL for c in codes), (hh, ww, src, null, codes)
        assert L0.nfs_last_error(), (hh, ww, src, null)
        for t in written:
            assert bool((t == SENT).all()), (hh, ww, src, null)
    # H * W at 2^30 is refused before any launch (no tensor of that size is touched)
    assert L.nfs_advect2d_source_fwd(P(d), P(src_in), 0, P(buf()), 1 << 15, 1 << 15, None) == _lib.NFS_EINVAL
    # and the same calls with good arguments go through
    written, codes = calls(H, W, 0, False)
    torch.cuda.synchronize()
    assert all(c == 0 for c in codes), codes

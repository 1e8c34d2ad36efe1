"""tests/field_ref.py pinned without a GPU: (1) against the oracle in float64 (autograd for the adjoints; 1e-12 per element,
times the amplification A of field_ref where a stencil involved lies outside the volume), (2) its bounds are
not too tight -- the float32 oracle on the CPU lies inside every one of them on every case the GPU test runs -- and
(3) not too loose: float32 numpy emulations of plausible kernel mistakes leave a bound somewhere while the whole-volume
rel L2 the older tests assert stays below 1e-4; (4) the share of voxels with the two-candidate latitude is capped.

Largest err/bound of the float32 oracle per operator over all cases (each test prints its own; torch CPU):
    advect sample 0.20  g_d 0.33  g_vel 0.19   transport 0.27   warp3d fwd 0.14  g_imgs 0.07  g_coords 0.13
    smoothing 0.26  adjoint 0.24   Adam m' 0.58  v' 0.46  x' 0.97 (the half-ulp of the final subtraction: tight by nature)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nfs_oracle as O
from tests import field_ref as FR
from tests import maccormack_ref as MR

EPS = FR.EPS
CASES = [(s, C, k) for (s, C) in FR.field_cases() for k in FR.KINDS]


def _id(c):
    return "%s-C%d-%s" % ("x".join(map(str, c[0])), c[1], c[2])


def _id2(c):
    return "%s-C%d" % ("x".join(map(str, c[0])), c[1])


def _relL2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _amp(shape, cv, **kw):
    """(A per voxel, the largest A among the voxels that scatter into each cell [*shape]; 1 where none does)"""
    axes = FR.trace(shape, cv, **kw)
    A = FR._prod(FR.amplification(axes))
    dest = np.ones(shape)
    for idx, _w in MR._corners(axes):
        np.maximum.at(dest, tuple(idx), A)
    return A, dest


def _oracle_advect(d, v, g, dtype):
    """O.advect and its two gradients by autograd, in ``dtype``"""
    dt = torch.tensor(d, dtype=dtype)[None].requires_grad_()
    vt = torch.tensor(v, dtype=dtype)[None].requires_grad_()
    out = O.advect(dt, vt)
    (out * torch.tensor(g, dtype=dtype)[None]).sum().backward()
    return out[0].detach().numpy(), dt.grad[0].numpy(), vt.grad[0].numpy()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_advect_reference_is_the_float64_oracle_and_covers_the_float32_oracle(case):
    """sample, g_d and g_vel: float64 oracle to 1e-12 of the largest value (times the amplification A the float64 oracle's
    own un-clamped weights carry outside the volume), float32 oracle inside every bound; g_vel by vel_excess"""
    shape, C, kind = case
    if C == 1 and min(shape) >= 4:                      # the smoke-like density of the GPU test's forward cases
        ds, vs, _ = FR.make_case(shape, C, kind, "smoke")
        ss, bss = FR.sample(ds, vs)
        o32s = O.advect(torch.tensor(ds)[None], torch.tensor(vs)[None])[0].numpy()
        assert FR.err_ratio(np.abs(o32s - ss), bss) <= 1.0
    d, v, rng = FR.make_case(shape, C, kind)
    g = rng.randn(*d.shape).astype(np.float32)
    s, bs = FR.sample(d, v)
    ref = FR.advect_adjoint(d, v, g)
    A, A_dest = _amp(shape, v)
    o64, gd64, gv64 = _oracle_advect(d, v, g, torch.float64)
    assert (np.abs(s - o64) <= 1e-12 * np.abs(d).max() * A[..., None]).all()
    # per element: a cell is held to 1e-12 times the largest A among the voxels that scatter into it, a voxel's velocity
    # gradient to 1e-12 times its own A -- plain 1e-12 wherever every stencil involved lies inside the volume
    assert (np.abs(ref["g_d"] - gd64) <= 1e-12 * max(np.abs(gd64).max(), 1.0) * A_dest[..., None]).all()
    tol_v = 1e-12 * max(np.abs(gv64).max(), 1.0) * A[..., None]
    near = np.abs(ref["vel_cand"] - gv64[None, None]).min(axis=(0, 1))
    assert (near <= tol_v).all()
    if kind in FR.CAPPED_KINDS and ref["unsure"].any():
        assert (np.abs(ref["g_vel"] - gv64) <= tol_v)[~ref["unsure"]].all()
    print("%-24s A == 1 on %.0f %% of the voxels and %.0f %% of the cells, largest A %.3g" % (
        _id(case), 100 * (A == 1).mean(), 100 * (A_dest == 1).mean(), A.max()))
    o32, gd32, gv32 = _oracle_advect(d, v, g, torch.float32)
    r = (FR.err_ratio(np.abs(o32 - s), bs), FR.err_ratio(np.abs(gd32 - ref["g_d"]), ref["bound_d"]),
         FR.vel_ratio(ref, gv32))
    print("%-24s float32 oracle err/bound: sample %.3f g_d %.3f g_vel %.3f" % ((_id(case),) + r))
    assert max(r) <= 1.0, (case, r)
    # the lean stencil's bound (fewer roundings) still covers the float32 oracle where no weight is amplified
    if FR.takes_lean(shape, C) and kind in ("tiny", "zero"):
        _, bl = FR.sample(d, v, stencil="lean")
        assert FR.err_ratio(np.abs(o32 - s), bl) <= 1.0


@pytest.mark.parametrize("case", [c for c in CASES if c[2] in FR.CAPPED_KINDS], ids=_id)
def test_latitude_cap(case):
    """'random' and 'far': at most 1 % of the voxels lie within face_margin of a face (where either of two cells is
    accepted for g_vel); 'integer' and 'tiny' exist to exercise that latitude.  No voxel is left out of a comparison"""
    shape, C, kind = case
    d, v, rng = FR.make_case(shape, C, kind)
    ref = FR.advect_adjoint(d, v, np.ones(d.shape, np.float32))
    share = float(ref["unsure"].mean())
    print("%-24s unsure %.3f %%" % (_id(case), 100 * share))
    assert share <= 0.01, (case, share)


@pytest.mark.parametrize("sc", FR.TRANSPORT_CASES, ids=_id2)
def test_transport_reference(sc):
    """O.transport forwards (scale 1), backwards (-1) and in one step over two frames (2) in float64 to 1e-12 A; the
    float32 oracle with the temporal filter's accumulation inside the bound"""
    shape, C = sc
    w_g, w_a = FR.TRANSPORT_W_G, FR.TRANSPORT_W_ADD
    for kind in FR.TRANSPORT_KINDS:
        g, u, rng = FR.make_case(shape, C, kind)
        add = rng.randn(*g.shape).astype(np.float32)
        worst = 0.0
        for scale, (a, b, rec) in zip(FR.TRANSPORT_SCALES, ((0, 1, True), (1, 0, True), (0, 2, False))):
            out, bound = FR.transport(g, u, scale, w_g, add, w_a)
            plain, _ = FR.transport(g, u, scale)
            A, _ = _amp(shape, u, scale=scale)
            for dtype in (torch.float64, torch.float32):
                t = O.transport(torch.tensor(g, dtype=dtype)[None],
                                torch.tensor(u, dtype=dtype)[None].repeat(2, 1, 1, 1, 1), a, b, recursive=rec)[0]
                if dtype == torch.float64:
                    assert (np.abs(t.numpy() - plain) <= 1e-12 * np.abs(g).max() * A[..., None]).all()
                else:
                    got = (np.float32(w_g) * t + np.float32(w_a) * torch.tensor(add)).numpy()
                    worst = max(worst, FR.err_ratio(np.abs(got - out), bound))
        print("transport %s C%d %s float32 oracle err/bound %.3f" % (shape, C, kind, worst))
        assert worst <= 1.0


def test_two_dimensional_sample_is_the_three_dimensional_one_with_a_single_plane():
    """2-D as D == 1: O.advect2d in float64 and float32 against sample on [1,H,W,C] with a zero first velocity component"""
    H, W, C = 13, 17, 3
    rng = np.random.RandomState(2)
    d = (rng.randn(H, W, C) * 2.0 - 0.5).astype(np.float32)
    v = (rng.uniform(-3, 3, (H, W, 2)) * np.asarray([2.0 / (H - 1), 2.0 / (W - 1)])).astype(np.float32)
    v3 = np.concatenate([np.zeros((H, W, 1), np.float32), v], -1)[None]
    s, b = FR.sample(d[None], v3)
    o64 = O.advect2d(torch.tensor(d, dtype=torch.float64)[None], torch.tensor(v, dtype=torch.float64)[None])[0].numpy()
    A, _ = _amp((1, H, W), v3)
    assert (np.abs(s[0] - o64) <= 1e-12 * np.abs(d).max() * A[0][..., None]).all()
    o32 = O.advect2d(torch.tensor(d)[None], torch.tensor(v)[None])[0].numpy()
    assert FR.err_ratio(np.abs(o32 - s[0]), b[0]) <= 1.0


@pytest.mark.parametrize("shape", FR.WARP_SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_warp3d_reference(shape, C):
    """explicit coordinates [B,3,X,Y,Z], batched source: O.batch_warp3d (FAST_WARP off) and autograd"""
    assert not O.FAST_WARP
    imgs, coords, g = FR.warp_case(shape, C)
    s, bs = FR.warp_fwd(imgs, coords)
    refs = FR.warp_adjoint(imgs, coords, g)
    res = {}
    for dtype in (torch.float64, torch.float32):
        it = torch.tensor(imgs, dtype=dtype).requires_grad_()
        ct = torch.tensor(coords, dtype=dtype).requires_grad_()
        out = O.batch_warp3d(it, ct, [2, *shape])
        (out * torch.tensor(g, dtype=dtype)).sum().backward()
        res[dtype] = (out.detach().numpy(), it.grad.numpy(), np.moveaxis(ct.grad.numpy(), 1, -1))
    o, gi, gc = res[torch.float64]
    amps = [_amp(shape, coords[b], explicit=True) for b in range(2)]
    o32, gi32, gc32 = res[torch.float32]
    r = [FR.err_ratio(np.abs(o32 - s), bs), 0.0, 0.0]
    for b, ref in enumerate(refs):
        A, A_dest = amps[b]                                  # per element, as in the advect test
        assert (np.abs(s[b] - o[b]) <= 1e-12 * np.abs(imgs).max() * A[..., None]).all()
        assert (np.abs(ref["g_d"] - gi[b]) <= 1e-12 * np.abs(gi).max() * A_dest[..., None]).all()
        near = np.abs(ref["vel_cand"] - gc[b][None, None]).min(axis=(0, 1))
        assert (near <= 1e-12 * np.abs(gc).max() * A[..., None]).all()
        r[1] = max(r[1], FR.err_ratio(np.abs(gi32[b] - ref["g_d"]), ref["bound_d"]))
        r[2] = max(r[2], FR.vel_ratio(ref, gc32[b]))
    print("warp3d %s C%d float32 oracle err/bound: fwd %.3f g_imgs %.3f g_coords %.3f" % ((shape, C) + tuple(r)))
    assert max(r) <= 1.0


def _smooth32(d, k):
    """the float32 oracle's pre-activation"""
    x = torch.tensor(d)[None, None]
    return F.conv3d(x, O.smooth_kernel3d(k)[None, None], padding=1)[0, 0].numpy() if k > 0 else d


@pytest.mark.parametrize("shape", FR.SMOOTH_SHAPES + FR.SMOOTH_SHAPES_16)
@pytest.mark.parametrize("k", FR.SMOOTH_KS)
def test_smooth_reference(shape, k):
    d = FR.smooth_input(shape)
    g = np.random.RandomState(3).randn(*shape).astype(np.float32)
    out, pre, bound = FR.smooth(d, k)
    res = {}
    for dtype in (torch.float64, torch.float32):
        dt = torch.tensor(d, dtype=dtype)[None, ..., None].requires_grad_()
        o = O.smooth3d_relu(dt, k)
        (o[0, ..., 0] * torch.tensor(g, dtype=dtype)).sum().backward()
        res[dtype] = (o[0, ..., 0].detach().numpy(), dt.grad[0, ..., 0].numpy())
    o64, g64 = res[torch.float64]
    scale = max(np.abs(d).max(), 1e-30)
    assert np.abs(out - o64).max() <= 1e-12 * scale
    adj, _ = FR.smooth_adjoint(g, pre >= 0, k)
    assert np.abs(adj - g64).max() <= 1e-12 * np.abs(g).max()
    # the transpose is the transpose: <smooth(a), b> == <a, smooth_T(b)>
    a = np.random.RandomState(4).randn(*shape)
    assert abs((FR.smooth_linear(a, k) * g).sum() - (a * FR.smooth_T(g, k)).sum()) <= 1e-12 * np.abs(a).sum()
    # an all-zero neighbourhood gives pre == 0 exactly and a zero bound
    assert (pre[FR.smooth_linear(np.abs(d), k) == 0] == 0).all()
    o32, g32 = res[torch.float32]
    adj32, b32 = FR.smooth_adjoint(g, _smooth32(d, k) >= 0, k)
    r = (FR.err_ratio(np.abs(o32 - out), bound), FR.err_ratio(np.abs(g32 - adj32), b32))
    print("smooth %s k=%g float32 oracle err/bound: fwd %.3f adjoint %.3f" % (shape, k, r[0], r[1]))
    assert max(r) <= 1.0


def _lr_t32(lr, t):
    f = np.float32
    return float(f(lr) * np.sqrt(f(1) - f(FR.B2) ** f(t)) / (f(1) - f(FR.B1) ** f(t)))


@pytest.mark.parametrize("n", FR.ADAM_NS)
def test_adam_reference(n):
    """three chained steps from non-zero moments: O.TFAdam in float64 to 1e-12, in float32 inside the bounds (chained from
    the float32 oracle's own previous state, as the GPU test chains from the kernel's)"""
    x0, m0, v0, gs = FR.adam_case(n)
    lr = 1e-2
    worst = [0.0, 0.0, 0.0]
    for dtype in (torch.float64, torch.float32):
        opt = O.TFAdam(FR.B1, FR.B2, FR.ADAM_EPS)
        opt.m, opt.v, opt.t = torch.tensor(m0, dtype=dtype), torch.tensor(v0, dtype=dtype), 4
        x = torch.tensor(x0, dtype=dtype)
        for g in gs:
            xp, mp, vp = x.numpy().copy(), opt.m.numpy().copy(), opt.v.numpy().copy()
            x = opt.step(x, torch.tensor(g, dtype=dtype), lr)
            if dtype == torch.float64:
                lr_t = lr * np.sqrt(1 - FR.B2 ** opt.t) / (1 - FR.B1 ** opt.t)
            else:
                lr_t = _lr_t32(lr, opt.t)
            x1, m1, v1, bx, bm, bv = FR.adam(xp, mp, vp, g, lr_t, FR.B1, FR.B2, FR.ADAM_EPS)
            for j, (got, want, bound) in enumerate(((opt.m, m1, bm), (opt.v, v1, bv), (x, x1, bx))):
                err = np.abs(got.numpy() - want)
                if dtype == torch.float64:
                    assert err.max() <= 1e-12 * max(np.abs(want).max(), 1e-30)
                else:
                    worst[j] = max(worst[j], FR.err_ratio(err, bound))
    print("adam n=%d float32 oracle err/bound: m' %.3f v' %.3f x' %.3f" % ((n,) + tuple(worst)))
    assert max(worst) <= 1.0
    # exact no-op where g == 0 and m == v == 0 (what the ever-skipping relies on)
    z = np.zeros(3, np.float32)
    x1, m1, v1, bx, bm, bv = FR.adam(x0[:3], z, z, z, 1e-2, FR.B1, FR.B2, FR.ADAM_EPS)
    assert (x1 == x0[:3]).all() and not m1.any() and not v1.any() and not bm.any() and not bv.any()


# ---- (3) sensitivity: float32 emulations of plausible kernel mistakes --------------------------------------------------
f32 = np.float32


def lean32(d, vel, g=None, weight_unclamped=False, zero_clamped=True):
    """the lean stencil in float32 numpy (csrc/warp.hip: lean_cell, lean_sample, lean_grad): sample [D,H,W] and, with g,
    the velocity gradient [D,H,W,3].  weight_unclamped: mistake (b); zero_clamped=False: mistake (a)"""
    dims = d.shape
    idx = np.meshgrid(*[np.arange(n, dtype=f32) for n in dims], indexing="ij")
    b, w, h, inside = [], [], [], []
    for k, n in enumerate(dims):
        hk = f32(0.5) * f32(n - 1)
        x = (idx[k] - vel[..., k] * hk).astype(f32)
        c = np.clip(x, f32(0), f32(n - 1))
        bk = np.minimum(np.floor(c), f32(n - 2))
        w.append(((x if weight_unclamped else c) - bk).astype(f32))
        b.append(bk.astype(np.int64))
        h.append(hk)
        inside.append((x >= 0) & (x < f32(n - 1)))
    p = {c: d[b[0] + c[0], b[1] + c[1], b[2] + c[2]] for c in np.ndindex(2, 2, 2)}
    e = {r: p[r + (1,)] - p[r + (0,)] for r in np.ndindex(2, 2)}
    a = {r: (w[2] * e[r] + p[r + (0,)]).astype(f32) for r in e}
    g0, g1 = a[0, 1] - a[0, 0], a[1, 1] - a[1, 0]
    b0, b1 = (w[1] * g0 + a[0, 0]).astype(f32), (w[1] * g1 + a[1, 0]).astype(f32)
    s = (w[0] * (b1 - b0) + b0).astype(f32)
    if g is None:
        return s
    f0, f1 = w[1] * (e[0, 1] - e[0, 0]) + e[0, 0], w[1] * (e[1, 1] - e[1, 0]) + e[1, 0]
    comps = (b1 - b0, w[0] * (g1 - g0) + g0, w[0] * (f1 - f0) + f0)
    gv = np.stack([-g * comps[k] * np.where(inside[k] | (not zero_clamped), h[k], f32(0)) for k in range(3)], -1)
    return s, gv.astype(f32)


def smooth32(d, k, drop_halo_at=None):
    """the separable smoothing in float32 numpy, x then y then z as the kernel; drop_halo_at = x: mistake (e), column x
    reads a zero in place of its right-hand neighbour (a tile edge without its halo)"""
    wa = f32(1) / f32(k + 2)
    wb = f32(k) * wa
    a = d.astype(f32)
    for axis in (2, 1, 0):
        pad = [(0, 0)] * 3
        pad[axis] = (1, 1)
        p = np.pad(a, pad)
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -2), slice(2, None)
        right = p[tuple(hi)].copy()
        if axis == 2 and drop_halo_at is not None:
            right[:, :, drop_halo_at] = 0
        a = (wa * right + (wb * a + wa * p[tuple(lo)]).astype(f32)).astype(f32)
    return a


def _confine(good, bad, ref_norm):
    """On volumes this small (16k voxels at the most) ONE voxel wrong by the size of a typical value already moves the
    whole-volume rel L2 by 1 / sqrt(16k) = 8e-3, so a mistake that strikes a whole plane, column or border shell is seen by
    the L2 tests here whatever it is; what they cannot see is the same mistake where it does little damage.  So a mistake
    is kept on at most four elements, the most damaged ones whose sum still leaves the rel L2 below 1e-4 (the L2 of the
    confined form is below 1e-4 by this construction; the unconfined one is printed next to it).  What is shown is that
    the bounds see a deviation of that size on single elements"""
    dev = np.abs(bad.astype(np.float64) - good).reshape(-1)
    budget = (0.9e-4 * ref_norm) ** 2
    keep = []
    for i in np.argsort(-dev):
        if dev[i] == 0 or len(keep) == 4:
            break
        if dev[i] ** 2 <= budget:
            keep.append(i)
            budget -= dev[i] ** 2
    out = good.copy().reshape(-1)
    out[keep] = bad.reshape(-1)[keep]
    return out.reshape(good.shape), len(keep)


def _caught(name, good, bad, ref, bound, confine=True):
    """good: the float32 emulation without the mistake (inside every bound), bad: with it.  The mistake must leave a bound
    on at least one element while the rel L2 against the reference stays below 1e-4"""
    good, bad = np.asarray(good), np.asarray(bad)
    assert FR.err_ratio(np.abs(good - ref), bound) <= 1.0, name + ": the emulation itself is outside a bound"
    hit, whole = int((bad != good).sum()), _relL2(bad, ref)
    if confine:
        all_hit = hit
        bad, hit = _confine(good, bad, np.linalg.norm(ref))
        assert hit > 0, name
        name += " [everywhere: %d elements, rel L2 %.2e]" % (all_hit, whole)
    l2 = _relL2(bad, ref)
    r = FR.err_ratio(np.abs(bad - ref), bound)
    print("mistake %s\n        on %4d elements: rel L2 %.2e, worst err/bound %.3g" % (name, hit, l2, r))
    assert l2 < 1e-4, (name, l2)
    assert r > 1.0, (name, r)


def test_bounds_catch_emulated_kernel_mistakes_the_l2_tests_cannot_see():
    shape = (12, 20, 68)
    d, v, rng = FR.make_case(shape, 1, "random")
    d3 = d[..., 0]
    g = rng.randn(*shape).astype(f32)
    s_ref, s_bound = FR.sample(d, v, stencil="lean")
    s_ref, s_bound = s_ref[..., 0], s_bound[..., 0]
    adj = FR.advect_adjoint(d, v, g[..., None], stencil="lean")
    good_s, good_gv = lean32(d3, v, g)

    # (a) the velocity gradient is not zeroed on an axis whose trace lies outside the volume
    _, bad_gv = lean32(d3, v, g, zero_clamped=False)
    assert FR.vel_ratio(adj, good_gv) <= 1.0
    bad_c, kept = _confine(good_gv, bad_gv, np.linalg.norm(adj["g_vel"]))
    assert kept > 0
    print("mistake (a) g_vel not zeroed on a clamped axis [everywhere: %d elements, rel L2 %.2e]\n"
          "        on %4d elements: rel L2 %.2e, worst err/bound %.3g" % (
              int((bad_gv != good_gv).sum()), _relL2(bad_gv, adj["g_vel"]), kept, _relL2(bad_c, adj["g_vel"]),
              FR.vel_ratio(adj, bad_c)))
    assert _relL2(bad_c, adj["g_vel"]) < 1e-4 and FR.vel_ratio(adj, bad_c) > 1.0
    # (b) the interpolation weight is taken from the unclamped coordinate
    _caught("(b) weight from the unclamped coordinate", good_s, lean32(d3, v, weight_unclamped=True), s_ref, s_bound)
    # (c) the last partial group of 4 voxels is left at a stale value: the previous iteration's sample (the velocity one
    #     small Adam step earlier), generic shape with n % 4 == 3
    gshape = (11, 9, 13)
    dg, vg, rg = FR.make_case(gshape, 1, "random")
    sg_ref, sg_bound = FR.sample(dg, vg)
    n = int(np.prod(gshape))
    good_g = O.advect(torch.tensor(dg)[None], torch.tensor(vg)[None])[0].numpy()
    v_prev = (vg + f32(1e-3) * rg.randn(*vg.shape).astype(f32) * f32(2.0 / 12)).astype(f32)
    stale = O.advect(torch.tensor(dg)[None], torch.tensor(v_prev)[None])[0].numpy()
    bad_g = good_g.copy().reshape(-1)
    bad_g[n - n % 4:] = stale.reshape(-1)[n - n % 4:]
    _caught("(c) last n % 4 voxels left at the previous iteration's value", good_g, bad_g.reshape(good_g.shape), sg_ref,
            sg_bound, confine=False)
    # (d) one border plane samples the neighbouring plane
    shifted = np.concatenate([d3[1:], d3[-1:]])
    bad_s = good_s.copy()
    bad_s[0] = lean32(shifted, v)[0]
    _caught("(d) plane 0 samples plane 1's density", good_s, bad_s, s_ref, s_bound)
    # (e) smoothing with one tile-edge column missing its halo neighbour
    sshape, k = (51, 7, 129), 3.0
    ds = FR.smooth_input(sshape)
    out, pre, sb = FR.smooth(ds, k)
    _caught("(e) smoothing column 64 without its right-hand halo", np.maximum(smooth32(ds, k), 0),
            np.maximum(smooth32(ds, k, drop_halo_at=64), 0), out, sb)
    # (f) the smoothing adjoint masks with pre > 0 instead of pre >= 0
    gs = np.random.RandomState(9).randn(*sshape).astype(f32)
    pre32 = smooth32(ds, k)
    want, wb = FR.smooth_adjoint(gs, pre32 >= 0, k)
    assert (pre32 == 0).sum() > 100
    _caught("(f) smoothing adjoint masks with pre > 0", smooth32(gs * (pre32 >= 0), k), smooth32(gs * (pre32 > 0), k),
            want, wb)
    # (g) the Adam tail elements (n % 4) are skipped
    x0, m0, v0, gsA = FR.adam_case(1003)
    lr_t = _lr_t32(1e-3, 5)
    x1, m1, v1, bx, bm, bv = FR.adam(x0, m0, v0, gsA[0], lr_t, FR.B1, FR.B2, FR.ADAM_EPS)
    opt = O.TFAdam(FR.B1, FR.B2, FR.ADAM_EPS)
    opt.m, opt.v, opt.t = torch.tensor(m0), torch.tensor(v0), 4
    good_x = opt.step(torch.tensor(x0), torch.tensor(gsA[0]), 1e-3).numpy()
    bad_x = good_x.copy()
    bad_x[1000:] = x0[1000:]
    _caught("(g) Adam skips the n % 4 tail", good_x, bad_x, x1, bx, confine=False)
    bad_m = opt.m.numpy().copy()
    bad_m[1000:] = m0[1000:]
    assert FR.err_ratio(np.abs(bad_m - m1), bm) > 1.0 >= FR.err_ratio(np.abs(opt.m.numpy() - m1), bm)


def test_live_decision_reference():
    """lean_live: on a field with exact-zero regions and a plateau the eight choices agree away from faces, both answers
    occur, and a dead voxel has an exactly zero float64 velocity gradient"""
    shape = (9, 10, 92)
    d, v, rng = FR.make_case(shape, 1, "random", density="smoke")
    L = FR.lean_live(d[..., 0], v)
    ref = FR.advect_adjoint(d, v, np.ones(d.shape, np.float32), stencil="lean")
    sure = ~ref["unsure"]
    assert (L[:, sure] == L[0, sure]).all()
    assert 0.05 < L[0].mean() < 0.95
    assert not ref["g_vel"][~L[0] & sure].any()


def test_a_value_that_is_not_a_number_never_passes():
    """err_ratio and vel_ratio give a ratio above 1 (inf) for a NaN or an infinity in any element, whatever the bound"""
    ref = np.array([1.0, 0.1, -2.0])
    for bad in (np.nan, np.inf, -np.inf):
        got = ref.copy()
        got[1] = bad
        assert FR.err_ratio(np.abs(got - ref), np.full(3, 1e-6)) > 1.0
        assert FR.err_ratio(np.abs(got - ref), np.full(3, np.inf)) > 1.0
    assert FR.err_ratio(np.abs(ref - ref), np.zeros(3)) == 0.0
    assert FR.err_ratio(np.array([0.0, 1e-7]), np.array([0.0, 1e-6])) == pytest.approx(0.1)
    assert FR.err_ratio(np.array([1e-9, 0.0]), np.array([0.0, 1.0])) > 1.0       # an error where the bound is zero
    d, v, rng = FR.make_case((5, 3, 4), 1, "random")
    g = rng.randn(*d.shape).astype(np.float32)
    adj = FR.advect_adjoint(d, v, g)
    assert FR.vel_ratio(adj, adj["g_vel"]) == 0.0
    for bad in (np.nan, np.inf):
        gv = adj["g_vel"].copy()
        gv[2, 1, 3, 0] = bad
        assert FR.vel_ratio(adj, gv) > 1.0
        assert FR.vel_ratio(adj, np.full_like(gv, bad)) > 1.0

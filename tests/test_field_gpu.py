"""The first-order field path element by element: advect and its adjoint (lean and generic stencils), the fused Adam
update and its variants, the live mask, transport_step, warp3d, the smoothing with its sign-bit mask and ApplyAdam, each
element against the float64 restatement of tests/field_ref.py within its own derived bound.  Every check prints the
largest err / bound it saw (pytest -s), so the slack stays visible.  The variants that share a stencil (adv_next, live,
ever, slabs) are chained to the checked ones bit for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import field_ref as FR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_T = float(np.float32(3e-3))
ADAM = (FR.B1, FR.B2, FR.ADAM_EPS)


@pytest.fixture(scope="module")
def ops():
    import neural_flow_style_amd.ops as ops
    return ops


def T(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(_bits(a), _bits(b))


def check(name, got, ref, bound):
    r = FR.err_ratio(np.abs(np.asarray(got, dtype=np.float64) - ref), bound)
    print("%-64s max err/bound %.3g" % (name, r))
    assert r <= 1.0, (name, r)


def check_vel(name, got, ref):
    """every component within its bound of one of the candidates (one and the same value away from faces)"""
    r = FR.vel_ratio(ref, got)
    print("%-64s max err/bound %.3g (%d voxels with two candidates)" % (name, r, int(ref["unsure"].sum())))
    assert r <= 1.0, (name, r)


def _sid(s):
    return "x".join(map(str, s))


def _cid(c):
    return "%s-C%d" % (_sid(c[0]), c[1])


def _stencil(shape, C):
    return "lean" if FR.takes_lean(shape, C) else "generic"


@functools.lru_cache(maxsize=None)
def case(shape, C, kind, density="randn"):
    d, v, rng = FR.make_case(shape, C, kind, density)
    g = rng.randn(*d.shape).astype(np.float32)
    return d, v, g


def densities(shape, C):
    return ("randn", "smoke") if C == 1 and min(shape) >= 4 else ("randn",)


# ---- advect: forward and gradients ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", FR.field_cases(), ids=_cid)
def test_advect_fwd(ops, sc):
    shape, C = sc
    for kind in FR.KINDS:
        for dens in densities(shape, C):
            d, v, _ = case(shape, C, kind, dens)
            out = ops.advect_fwd(T(d), T(v))
            s, b = FR.sample(d, v, stencil=_stencil(shape, C))
            check("advect_fwd %s %s %s (%s)" % (_cid(sc), kind, dens, _stencil(shape, C)), N(out), s, b)


@pytest.mark.parametrize("sc", FR.field_cases(), ids=_cid)
def test_advect_bwd(ops, sc):
    """g_vel alone (the lean MODE 1 where it applies), both gradients (generic, float atomics), and g_d accumulated onto
    what its buffer held -- each against advect_adjoint, g_vel by vel_excess"""
    shape, C = sc
    for kind in FR.KINDS:
        d, v, g = case(shape, C, kind)
        init = np.random.RandomState(5).randn(*d.shape).astype(np.float32)
        dt, vt, gt = T(d), T(v), T(g)
        name = "%s %s" % (_cid(sc), kind)
        none_d, gv = ops.advect_bwd(dt, vt, gt, need_d=False)
        assert none_d is None
        st = _stencil(shape, C)
        gen = FR.advect_adjoint(d, v, g)
        check_vel("advect_bwd g_vel alone %s (%s)" % (name, st), N(gv), gen if st == "generic" else
                  FR.advect_adjoint(d, v, g, stencil="lean"))
        gd, gv2 = ops.advect_bwd(dt, vt, gt)
        check("advect_bwd g_d %s" % name, N(gd), gen["g_d"], gen["bound_d"])
        check_vel("advect_bwd g_vel with g_d %s (generic)" % name, N(gv2), gen)
        acc = T(init)
        gd3, gv3 = ops.advect_bwd(dt, vt, gt, g_d_acc=acc)
        assert gd3 is acc and same(gv3, gv2)
        ref_i = FR.advect_adjoint(d, v, g, init_d=init)
        check("advect_bwd g_d accumulated %s" % name, N(gd3), ref_i["g_d"], ref_i["bound_d"])


# ---- the fused Adam update (MODE 2) and the variants chained to it -------------------------------------------------
def _state(shape, rng, dead=None):
    m = (rng.randn(*shape, 3) * 0.1).astype(np.float32)
    u = (rng.rand(*shape, 3) * 0.01).astype(np.float32)
    if dead is not None:
        m[dead] = 0.0
        u[dead] = 0.0
    return m, u


@pytest.mark.parametrize("shape", FR.LEAN_SHAPES, ids=_sid)
def test_fused_adam_is_applyadam_on_the_kernels_own_gradient(ops, shape):
    """two consecutive advect_bwd_adam steps from non-zero moments: vel, m and v against field_ref.adam applied to the
    gradient the MODE 1 launch writes for the same inputs (itself held to float64 by test_advect_bwd), every element.
    Where g_out == 0 and m == v == 0 all three buffers keep their bits (the ever-skipping relies on it)"""
    n = int(np.prod(shape))
    for kind in FR.KINDS:
        d, v0, g = case(shape, 1, kind)
        rng = np.random.RandomState(n + len(kind))
        dead = (rng.rand(*shape) < 0.3)
        m0, u0 = _state(shape, rng, dead)
        dt, vel, m, u = T(d), T(v0), T(m0), T(u0)
        for step in range(2):
            gs = rng.randn(*shape, 1).astype(np.float32)
            gs[dead] = 0.0
            gt = T(gs)
            _, gv = ops.advect_bwd(dt, vel, gt, need_d=False)
            before = [N(t).copy() for t in (vel, m, u)]
            ops.advect_bwd_adam(dt, vel, gt, m, u, LR_T, *ADAM)
            x1, m1, v1, bx, bm, bv = FR.adam(before[0], before[1], before[2], N(gv), LR_T, *ADAM)
            name = "%s %s step %d" % (_sid(shape), kind, step)
            check("advect_bwd_adam m   " + name, N(m), m1, bm)
            check("advect_bwd_adam v   " + name, N(u), v1, bv)
            check("advect_bwd_adam vel " + name, N(vel), x1, bx)
            for t, b in zip((vel, m, u), before):
                assert np.array_equal(N(t).view(np.int32)[dead], b.view(np.int32)[dead]), name


def _fused(ops, d, v, m, u, g, **kw):
    vel, mm, uu = T(v), T(m), T(u)
    ops.advect_bwd_adam(d, vel, g, mm, uu, LR_T, *ADAM, **kw)
    return vel, mm, uu


@pytest.mark.parametrize("shape", FR.LEAN_SHAPES, ids=_sid)
def test_variant_chain_is_bit_identical(ops, shape):
    """adv_next == advect_fwd of the updated velocity; the live forms leave everything else unchanged"""
    for kind in FR.KINDS:
        for dens in densities(shape, 1):
            d, v, g = case(shape, 1, kind, dens)
            rng = np.random.RandomState(3)
            m0, u0 = _state(shape, rng)
            dt, gt = T(d), T(g)
            plain = _fused(ops, dt, v, m0, u0, gt)
            adv = torch.full(shape, 7.0, device="cuda")
            withfwd = _fused(ops, dt, v, m0, u0, gt, adv_next=adv)
            assert all(same(a, b) for a, b in zip(plain, withfwd))
            fwd = ops.advect_fwd(dt, plain[0])
            assert same(adv, fwd[..., 0])
            live0 = ops.live_mask(*shape, dt)
            assert same(ops.advect_fwd(dt, T(v), live=live0), ops.advect_fwd(dt, T(v)))
            adv2, live = torch.full(shape, 7.0, device="cuda"), ops.live_mask(*shape, dt)
            withlive = _fused(ops, dt, v, m0, u0, gt, adv_next=adv2, live_next=live)
            assert all(same(a, b) for a, b in zip(plain, withlive)) and same(adv2, adv)
            live1 = ops.live_mask(*shape, dt)
            ops.advect_fwd(dt, plain[0], live=live1)
            assert same(live, live1)


@pytest.mark.parametrize("shape", [(3, 5, 68), (9, 10, 92), (12, 20, 68)], ids=_sid)
def test_ever_skipping_is_bit_identical_over_three_steps(ops, shape):
    """_live_ever == _live on the smoke-like density for every velocity kind, `ever` zeroed alongside m and v: velocity,
    moments, next sample and mask after each of three steps.  Both ways of skipping run: on the two larger shapes 'tiny'
    and 'zero' leave whole waves (four aligned mask words) empty next to waves that are partly live (a word neither empty
    nor full: only some lanes take part), and 'far', whose traces all end on the empty border, skips every wave"""
    n = int(np.prod(shape))
    for kind in FR.KINDS:
        d, v, _ = case(shape, 1, kind, "smoke")
        dt = T(d)
        runs = []
        for ever_on in (False, True):
            vel, m, u = T(v), torch.zeros(shape + (3,), device="cuda"), torch.zeros(shape + (3,), device="cuda")
            live = ops.live_mask(*shape, dt)
            ever = ops.live_mask(*shape, dt) if ever_on else None
            # the buffer of the next sample holds the current one on entry, like the mask: a voxel that is skipped keeps
            # its velocity, so its sample is not written again
            adv = ops.advect_fwd(dt, vel, live=live)[..., 0].contiguous()
            rs = np.random.RandomState(8)
            trace = []
            for step in range(3):
                gt = T(rs.randn(*shape, 1).astype(np.float32))
                ops.advect_bwd_adam(dt, vel, gt, m, u, LR_T, *ADAM, adv_next=adv, live_next=live, ever=ever)
                trace.append([t.clone() for t in (vel, m, u, adv, live)])
            runs.append((trace, ever))
        for a, b in zip(runs[0][0], runs[1][0]):
            assert [same(x, y) for x, y in zip(a, b)] == [True] * 5, kind     # vel, m, v, next sample, mask
        words = N(runs[1][1]).view(np.uint64)
        partial = int(((words != 0) & (words != np.uint64(2 ** 64 - 1)))[:n // 64].sum())
        waves_empty = int((words.reshape(-1, 4) == 0).all(1).sum())
        print("ever %-9s %-8s %3d mask words partly set, %3d of %3d waves empty" % (
            _sid(shape), kind, partial, waves_empty, words.size // 4))
        # the velocity moves only where the mask is set (a set bit need not move it: every axis may be clamped)
        changed = (N(runs[1][0][2][0]).view(np.int32) != v.view(np.int32)).any(-1)
        ever_bits, _ = _unpack(runs[1][1], n)
        assert not (changed & ~ever_bits.reshape(shape)).any(), kind
        moved = bool(changed.any())
        if kind == "far" and shape != (3, 5, 68):
            assert not words.any()
        if kind in ("tiny", "zero") and shape != (3, 5, 68):
            assert waves_empty > 0 and partial > 0 and moved, kind


def _splits(D):
    return [(0, 1), (D - 1, 1), (1, D - 2), (0, D), (0, D // 3), (D // 3, D - D // 3)]


@pytest.mark.parametrize("shape", [(12, 20, 68), (9, 10, 92)], ids=_sid)
def test_slab_forms_are_the_same_planes_of_the_whole_volume_call(ops, shape):
    D, H, W = shape
    for kind in FR.KINDS:
        d, v, g = case(shape, 1, kind)
        rng = np.random.RandomState(4)
        m0, u0 = _state(shape, rng)
        dt, gt = T(d), T(g)
        whole_fwd = ops.advect_fwd(dt, T(v))[..., 0]
        adv = torch.empty(shape, device="cuda")
        whole = _fused(ops, dt, v, m0, u0, gt, adv_next=adv)
        d3 = dt[..., 0].contiguous()
        for z0, nz in _splits(D):
            assert nz * H * W % 4 == 0
            sl = slice(z0, z0 + nz)
            assert same(ops.advect_fwd_slab(d3, T(v[sl]), z0), whole_fwd[sl]), (kind, z0, nz)
            for with_next in (False, True):
                vs, ms, us = T(v[sl]), T(m0[sl]), T(u0[sl])
                nxt = torch.empty((nz, H, W), device="cuda") if with_next else None
                ops.advect_bwd_adam_slab(d3, vs, T(g[sl]), ms, us, z0, LR_T, *ADAM, adv_next=nxt)
                assert same(vs, whole[0][sl]) and same(ms, whole[1][sl]) and same(us, whole[2][sl]), (kind, z0, nz)
                if with_next:
                    assert same(nxt, adv[sl]), (kind, z0, nz)


def test_slab_with_a_voxel_count_no_multiple_of_four_is_refused_and_writes_nothing(ops):
    from neural_flow_style_amd import _lib
    shape = (4, 3, 5)
    d, v, g = case(shape, 1, "random")
    d3 = T(d[..., 0])
    out = torch.full((1, 3, 5), 7.0, device="cuda")
    with pytest.raises(_lib.NfsError) as e:
        ops.advect_fwd_slab(d3, T(v[1:2]), 1, out=out)
    assert e.value.code == _lib.NFS_EINVAL and bool((out == 7.0).all())
    vs, ms, us = T(v[1:2]), torch.ones((1, 3, 5, 3), device="cuda"), torch.ones((1, 3, 5, 3), device="cuda")
    for nxt in (None, out):
        with pytest.raises(_lib.NfsError) as e:
            ops.advect_bwd_adam_slab(d3, vs, T(g[1:2]), ms, us, 1, LR_T, *ADAM, adv_next=nxt)
        assert e.value.code == _lib.NFS_EINVAL
    assert same(vs, T(v[1:2])) and bool((ms == 1).all()) and bool((us == 1).all()) and bool((out == 7.0).all())


def _unpack(mask_f32, n):
    words = N(mask_f32.view(torch.int64)).view(np.uint64)
    b = np.unpackbits(words.view(np.uint8), bitorder="little")
    return b[:n].astype(bool), b[n:]


@pytest.mark.parametrize("shape", FR.LEAN_SHAPES, ids=_sid)
def test_live_mask_is_the_float64_decision(ops, shape):
    """bit = 'the eight corners of the back-traced cell are not all equal'; within face_margin of a face either cell's
    decision is accepted; no bit beyond the volume.  Densities with equal neighbours: halves ('tiny'), the smoke field"""
    n = int(np.prod(shape))
    for kind, dens in (("tiny", "randn"), ("integer", "randn"), ("random", "smoke"), ("integer", "smoke"), ("far", "smoke")):
        if dens == "smoke" and min(shape) < 3:
            continue
        d, v, _ = case(shape, 1, kind, dens)
        if kind == "integer" and dens == "randn":
            d = (np.round(d) / 1.0).astype(np.float32)              # whole numbers: many equal neighbours
        live = ops.live_mask(*shape, T(d))
        ops.advect_fwd(T(d), T(v), live=live)
        got, beyond = _unpack(live, n)
        got = got.reshape(shape)
        L = FR.lean_live(d[..., 0], v)
        ok = (L == got[None]).any(0)
        print("live mask %-10s %-8s %-6s live %.1f %%, %d voxels with more than one accepted answer" % (
            _sid(shape), kind, dens, 100 * got.mean(), int((L != L[0]).any(0).sum())))
        assert ok.all(), (shape, kind, dens, np.argwhere(~ok)[:4])
        assert not beyond.any()


# ---- transport_step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", FR.TRANSPORT_CASES, ids=_cid)
def test_transport_step(ops, sc):
    """w_g * advect(g, scale * u) + w_addend * addend and the plain crossing, lean (C = 1, 3) and generic"""
    shape, C = sc
    st = "lean" if FR.transport_takes_lean(shape, C) else "generic"
    w_g, w_a = FR.TRANSPORT_W_G, FR.TRANSPORT_W_ADD
    for kind in FR.TRANSPORT_KINDS:
        g, u, add = case(shape, C, kind)
        gt, ut, at = T(g), T(u), T(add)
        for scale in FR.TRANSPORT_SCALES:
            out = ops.transport_step(gt, ut, scale=scale, w_g=w_g, addend=at, w_addend=w_a)
            ref, b = FR.transport(g, u, scale, w_g, add, w_a, stencil=st)
            check("transport_step %s %s scale %+g addend (%s)" % (_cid(sc), kind, scale, st), N(out), ref, b)
            out = ops.transport_step(gt, ut, scale=scale)
            ref, b = FR.transport(g, u, scale, stencil=st)
            check("transport_step %s %s scale %+g plain  (%s)" % (_cid(sc), kind, scale, st), N(out), ref, b)


# ---- warp3d: explicit coordinates ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FR.WARP_SHAPES, ids=_sid)
@pytest.mark.parametrize("C", [1, 3])
def test_warp3d(ops, shape, C):
    """coordinates in [-1.3, 1.3], B = 2; Z == 1 takes the gather without 8-byte pairs"""
    imgs, coords, g = FR.warp_case(shape, C)
    out = ops.warp3d_fwd(T(imgs), T(coords))
    s, b = FR.warp_fwd(imgs, coords)
    check("warp3d_fwd %s C%d" % (_sid(shape), C), N(out), s, b)
    gi, gc = ops.warp3d_bwd(T(imgs), T(coords), T(g))
    gi, gc = N(gi), N(gc)
    for bi, ref in enumerate(FR.warp_adjoint(imgs, coords, g)):
        check("warp3d_bwd g_imgs %s C%d b%d" % (_sid(shape), C, bi), gi[bi], ref["g_d"], ref["bound_d"])
        check_vel("warp3d_bwd g_coords %s C%d b%d" % (_sid(shape), C, bi), np.moveaxis(gc[bi], 0, -1), ref)


# ---- smoothing -----------------------------------------------------------------------------------------------------
def smooth_checks(ops, shape, k, tag=""):
    """forward: value, sign-bit encoding, +0 on an all-zero neighbourhood; adjoint on the kernel's own mask"""
    d = FR.smooth_input(shape)
    g = np.random.RandomState(3).randn(*shape).astype(np.float32)
    out = ops.smooth3d_relu_fwd(T(d), k)
    o = N(out)
    word = o.view(np.uint32)
    ref, pre, bound = FR.smooth(d, k)
    name = "%s k=%g%s" % (_sid(shape), k, tag)
    check("smooth3d_relu_fwd " + name, o.astype(np.float64), ref, bound)
    assert (word[pre < -bound] == 0x80000000).all(), name
    assert (word[pre > bound] >> 31 == 0).all(), name
    empty = FR.smooth_linear(np.abs(d), k) == 0
    assert (word[empty] == 0).all() and (empty.any() or min(shape) < 3), name
    assert (word[(word >> 31) == 1] == 0x80000000).all(), name          # a set sign bit only ever on a zero
    mask = (word >> 31) == 0
    gd = ops.smooth3d_relu_bwd(out, T(g), k)
    adj, b = FR.smooth_adjoint(g, mask, k)
    check("smooth3d_relu_bwd " + name, N(gd), adj, b)
    return o, N(gd)


@pytest.mark.parametrize("shape", FR.SMOOTH_SHAPES, ids=_sid)
def test_smooth3d_relu(ops, shape):
    for k in FR.SMOOTH_KS:
        smooth_checks(ops, shape, k)


def test_smooth3d_relu_sixteen_row_instance_in_a_child_process(ops, tmp_path):
    """NFS_SM_ROWS is read once per process: a fresh child with NFS_SM_ROWS=16 runs the same checks at (26,17,55) and
    (3,33,28) and hands back its outputs, which must be this process's (the 8-row instance at these sizes) bit for bit"""
    path = str(tmp_path / "rows16.npz")
    env = dict(os.environ, NFS_SM_ROWS="16", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "tests.test_field_gpu", path], cwd=ROOT, env=env, timeout=240,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    theirs = np.load(path)
    for shape in FR.SMOOTH_SHAPES_16:
        for k in FR.SMOOTH_KS:
            o, gd = smooth_checks(ops, shape, k, " (this process)")
            key = "%s_%g" % (_sid(shape), k)
            assert np.array_equal(o.view(np.int32), theirs["o_" + key].view(np.int32)), key
            assert np.array_equal(gd.view(np.int32), theirs["g_" + key].view(np.int32)), key


# ---- ApplyAdam -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FR.ADAM_NS)
def test_adam_tf_step(ops, n):
    """three steps, each element against field_ref.adam chained from the kernel's own previous state"""
    x0, m0, v0, gs = FR.adam_case(n)
    x, m, v = T(x0), T(m0), T(v0)
    for step, g in enumerate(gs):
        before = [N(t).copy() for t in (x, m, v)]
        ops.adam_tf_step(x, m, v, T(g), LR_T, *ADAM)
        x1, m1, v1, bx, bm, bv = FR.adam(before[0], before[1], before[2], g, LR_T, *ADAM)
        check("adam_tf_step m n=%d step %d" % (n, step), N(m), m1, bm)
        check("adam_tf_step v n=%d step %d" % (n, step), N(v), v1, bv)
        check("adam_tf_step x n=%d step %d" % (n, step), N(x), x1, bx)


if __name__ == "__main__":
    # the child of test_smooth3d_relu_sixteen_row_instance_in_a_child_process
    assert os.environ.get("NFS_SM_ROWS") == "16"
    import neural_flow_style_amd.ops as _ops
    res = {}
    for _shape in FR.SMOOTH_SHAPES_16:
        for _k in FR.SMOOTH_KS:
            _o, _g = smooth_checks(_ops, _shape, _k, " (16-row child)")
            res["o_%s_%g" % (_sid(_shape), _k)] = _o
            res["g_%s_%g" % (_sid(_shape), _k)] = _g
    np.savez(sys.argv[1], **res)

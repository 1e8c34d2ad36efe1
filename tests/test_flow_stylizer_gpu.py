"""``--carrier_steps`` of ``target_field 'g'`` (styler_3p): the carrier field is a velocity and the particles are carried
through it in K Euler steps.  One frame's gradient at K = 4 against a 'p' styler of the same configuration evaluated at
var = path[K] - p (the losses, and g_u against the float64 adjoint of that styler's g_v along the kernel's path), a
three-frame run at K = 4 with ``apply_carrier``, and K = 1 on the branch that stood before the flag.

The scene is tests/test_carrier_stylizer_gpu.py's: synthetic weights, 16^3, a carrier grid of 4 x 5 x 3, two uniform views,
three frames of 300 / 280 / 310 blob particles."""
import functools

import numpy as np
import pytest
import torch

from tests import flow_ref as FREF
from tests.test_carrier_stylizer_gpu import CARRIER, COUNTS, RES, _params, _styler, rel, scene

pytestmark = pytest.mark.gpu

K = 4


@pytest.mark.parametrize("interp", ["cubic", "linear"])
@pytest.mark.parametrize("mode,v_batch,w_pressure", [("sequential", 1, 0.0), ("sum", 2, 0.0), ("sum", 2, 1e3)])
def test_gradient_of_one_frame_at_four_steps(mode, v_batch, w_pressure, interp):
    """the 'g' styler at K = 4 and a non-zero u against the 'p' styler at var = path[K] - p: the losses agree, and g_u is
    the float64 adjoint of the 'p' styler's g_v, both to relative L2 <= 1e-3 (the project's bar for gradient parity)"""
    from neural_flow_style_amd import ops
    sc = scene()
    cubic = interp == "cubic"
    sg = _styler("g", views_mode=mode, v_batch=v_batch, w_pressure=w_pressure, carrier_interp=interp, carrier_steps=K)
    sp = _styler("p", views_mode=mode, v_batch=v_batch, w_pressure=w_pressure)
    assert sg._carrier and sg._carrier_steps == K and sg._var_shape(7) == tuple(CARRIER) + (3,)
    for st in (sg, sp):
        st.loss.set_style_image(st._style_feature(st.style_img, RES[1:]))
    p = sg._dev(sc["p"][0])
    u = sg._dev(sc["u"] * 4)                               # (up to two cells of the 16^3 grid over the whole flow)
    path = ops.flow_fwd(u, p, K, cubic=cubic)
    v = (path[K] - p).contiguous()
    assert float(v.abs().max()) > 1e-3
    assert rel(v.cpu(), ops.g2p_fwd(u, p, cubic=cubic).cpu()) > 1e-3          # (the flow is not the one-sample map)
    batches = [(i, i + v_batch) for i in range(0, 2, v_batch)] if mode == "sequential" else [(0, 2)]
    for lo, hi in batches:
        l_g, g_u = sg._value_and_grad(p, None, u, RES, sg._rot(lo, hi), view_shard=False)
        l_p, g_v = sp._value_and_grad(p, None, v, RES, sp._rot(lo, hi), view_shard=False)
        assert tuple(g_u.shape) == tuple(CARRIER) + (3,) and tuple(g_v.shape) == (COUNTS[0], 3)
        want, _ = FREF.adjoint(u, path, g_v, cubic)
        rl = abs(float(l_g.sum()) - float(l_p.sum())) / abs(float(l_p.sum()))
        rg = rel(g_u.cpu(), want.cpu())
        print("'g' at K = %d against 'p' %s %s v_batch %d pressure %g views %d:%d  loss rel %.3g  g_u rel-L2 %.3g"
              % (K, interp, mode, v_batch, w_pressure, lo, hi, rl, rg))
        assert float(g_u.abs().max()) > 0 and float(g_v.abs().max()) > 0
        assert rl <= 1e-3, rl
        assert rg <= 1e-3, rg


@functools.lru_cache(maxsize=None)
def _run_flow():
    st = _styler("g", F=3, iter=3, lr=0.002, views_mode="sum", v_batch=2, carrier_steps=K)
    return st, st.run(_params())


def test_run_at_four_steps_and_apply_carrier():
    from neural_flow_style_amd import ops
    st, res = _run_flow()
    ps = scene()["p"]
    assert res["carrier_resolution"] == CARRIER and len(res["opt"]) == 3
    assert np.asarray(res["l"]).shape == (1, 9) and np.isfinite(res["l"]).all()
    assert res["d"].shape == (3,) + tuple(RES) + (1,) and res["r"].shape == (3, RES[1], RES[2], 3)
    dev = lambda a: torch.tensor(a, device="cuda")
    for t, n in enumerate(COUNTS):
        u, p, v = res["opt"][t], res["p"][t], res["v"][t]
        assert u.shape == tuple(CARRIER) + (3,) and p.shape == (n, 3) and v.shape == (n, 3)
        assert np.isfinite(u).all() and np.isfinite(p).all() and np.isfinite(v).all()
        np.testing.assert_allclose(p, ps[t] + v, rtol=0, atol=1e-7)
        assert np.array_equal(v, p - ps[t])
        assert np.array_equal(p, st.apply_carrier(u, ps[t]))
        assert np.array_equal(p, ops.flow_fwd(dev(u), dev(ps[t]), K, cubic=True)[K].cpu().numpy())
        assert float(np.abs(v).max()) > 1e-4 and float(np.abs(u).max()) > 1e-4
    # any other particle set, on the device too; and the field means the K-step map, not the one-sample one
    other = np.random.RandomState(62).uniform(-0.1, 1.1, (777, 3)).astype(np.float32)
    u = scene()["u"] * 4
    want = ops.flow_fwd(dev(u), dev(other), K, cubic=True)[K]
    got = st.apply_carrier(u, other)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want.cpu().numpy())
    assert torch.equal(st.apply_carrier(dev(u), dev(other)), want)
    assert not np.array_equal(got, ops.carrier_displace(dev(u), dev(other))[0].cpu().numpy())
    assert np.array_equal(st.apply_carrier(u * 0, other), other)


def test_one_step_takes_the_branch_that_stood(monkeypatch):
    """with the flow's operators patched to raise, a ``carrier_steps 1`` run completes and is the displacement of before"""
    from neural_flow_style_amd import ops
    from neural_flow_style_amd import transform as T

    def never(*a, **k):
        raise AssertionError("carrier_steps 1 reached the flow")
    for mod, name in ((ops, "flow_fwd"), (ops, "flow_bwd"), (ops, "flow_grad"), (T, "carrier_flow")):
        monkeypatch.setattr(mod, name, never)
    st = _styler("g", F=1, iter=2, lr=0.002, views_mode="sum", v_batch=2, carrier_steps=1)
    assert st._carrier_steps == 1
    ps = scene()["p"]
    res = st.run({"p": ps[:1]})
    dev = lambda a: torch.tensor(a, device="cuda")
    u, p, v = res["opt"][0], res["p"][0], res["v"][0]
    assert np.isfinite(res["l"]).all() and float(np.abs(u).max()) > 1e-4
    assert np.array_equal(v, ops.g2p_fwd(dev(u), dev(ps[0]), cubic=True).cpu().numpy())
    assert np.array_equal(p, st.apply_carrier(u, ps[0]))
    np.testing.assert_allclose(p, ps[0] + v, rtol=0, atol=1e-7)

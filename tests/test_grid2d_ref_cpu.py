"""tests/grid2d_ref.py pinned to the existing references (stream_ref, potential_ref, oracle.curl), its transposes by the
dot-product identity, the invariants of the float32 velocities, and one step of the reference loop against the
hand-composed pieces."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import grid2d_ref as R
from tests import potential_ref as PR
from tests import stream_ref as SR

SHAPES = [(2, 2), (3, 5), (13, 18)]


def _rand(kind, H, W, seed, dtype=np.float64):
    return np.random.RandomState(seed).randn(*R.var_shape(kind, H, W)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES + [(2, 9), (33, 70)])
def test_velocities_are_the_d1_restriction_of_the_3d_references(shape, dtype):
    """components 1, 2 of the 3-D velocities on the [1,H,W,.] embedding, component 0 exactly zero -- the same bits in
    float32 (every difference rounded once, one sum)"""
    H, W = shape
    psi, phi, a = _rand("s", H, W, 1, dtype), _rand("p", H, W, 2, dtype), _rand("sp", H, W, 3, dtype)
    s3 = np.zeros((1, H, W, 3), dtype)
    s3[0, ..., 2] = psi
    v3 = SR.velocity(s3)
    assert not v3[..., 0].any() and np.array_equal(v3[0, ..., 1:], R.velocity("s", psi))
    v3 = PR.velocity(phi[None])
    assert not v3[..., 0].any() and np.array_equal(v3[0, ..., 1:], R.velocity("p", phi))
    a4 = np.zeros((1, H, W, 4), dtype)
    a4[0, ..., 2], a4[0, ..., 3] = a[..., 0], a[..., 1]
    v3 = PR.helmholtz_velocity(a4)
    assert not v3[..., 0].any() and np.array_equal(v3[0, ..., 1:], R.velocity("sp", a))
    # 's' is the reference's curl(is_2d=True) with its two channels reversed, no scale factor
    c = O.curl(torch.tensor(psi)[None, ..., None], is_2d=True)[0].numpy()
    assert np.array_equal(c[..., ::-1], R.velocity("s", psi))
    v = _rand("v", H, W, 4, dtype)
    assert np.array_equal(R.velocity("v", v), v)
    # the torch form the reference loop differentiates
    for kind, x in (("s", psi), ("p", phi), ("sp", a), ("v", v)):
        assert np.array_equal(R.torch_velocity(kind, torch.tensor(x)).numpy(), R.velocity(kind, x))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_transposes_by_the_dot_product_identity(kind, shape):
    H, W = shape
    x, g = _rand(kind, H, W, 5), np.random.RandomState(6).randn(H, W, 2)
    lhs, rhs = (R.velocity(kind, x) * g).sum(), (x * R.velocity_T(kind, g)).sum()
    assert abs(lhs - rhs) <= 1e-12 * np.abs(R.velocity(kind, x) * g).sum(), (lhs, rhs)
    A = R.velocity_T(kind, g, absolute=True)
    assert (np.abs(R.velocity_T(kind, g)) <= A + 1e-12).all()
    assert R.velocity_T(kind, np.ones_like(g), absolute=True).max() <= 6.0     # at most 3 terms per axis meet
    # and it is autograd's transpose of the torch form
    xt = torch.tensor(x, requires_grad=True)
    (R.torch_velocity(kind, xt) * torch.tensor(g)).sum().backward()
    assert np.abs(xt.grad.numpy() - R.velocity_T(kind, g)).max() <= 1e-12


@pytest.mark.parametrize("shape", [(13, 18), (24, 32), (33, 70)])
def test_float32_stream_velocity_is_divergence_free_and_potential_velocity_rotation_free(shape):
    H, W = shape
    psi, phi = R.make_var("s", H, W, 2.5, 7), R.make_var("p", H, W, 2.5, 8)
    vs, vp = R.velocity("s", psi), R.velocity("p", phi)
    assert vs.dtype == np.float32 and vp.dtype == np.float32
    div, rot = np.abs(R.divergence(vs)).max(), np.abs(R.rotation(vp)).max()
    print("%s: max |div| %.3e (bound %.3e), max |rot| %.3e (bound %.3e)" % (shape, div, R.divergence_bound(psi), rot,
                                                                            R.rotation_bound(phi)))
    assert div <= R.divergence_bound(psi) and rot <= R.rotation_bound(phi)
    assert R.rotation_bound(phi) == 2.0 ** -22 * PR.max_forward_difference(phi[None])
    # the converse holds for neither: the bounds are not vacuous
    assert np.abs(R.rotation(vs)).max() > 1e3 * R.divergence_bound(psi)
    assert np.abs(R.divergence(vp)).max() > 1e3 * R.rotation_bound(phi)
    # 'sp': each part contributes its own half
    a = np.stack([psi, phi], -1).astype(np.float64)
    v = R.velocity("sp", a)
    assert np.abs(R.divergence(v) - R.divergence(R.velocity("p", a[..., 1]))).max() <= 1e-12
    assert np.abs(R.rotation(v) - R.rotation(R.velocity("s", a[..., 0]))).max() <= 1e-12


def _case(H, W, F, seed=3):
    from neural_flow_style_amd import synthetic as S
    rng = np.random.RandomState(seed)
    d = [S.blob_density2d(H, W, rng)]
    u = [S.curl_velocity2d(H, W, rng, max_cells=1.5) for _ in range(F)]
    for t in range(F - 1):
        d.append(O.advect2d(torch.tensor(d[-1])[None, ..., None], torch.tensor(u[t])[None])[0, ..., 0].numpy())
    return d, u, S.style_image(H, W, rng)


def test_synthetic_2d_inputs():
    from neural_flow_style_amd import synthetic as S
    d = S.blob_density2d(24, 32, np.random.RandomState(1))
    assert d.shape == (24, 32) and d.dtype == np.float32 and d.min() == 0.0 and 0.5 < d.max() <= 1.0
    assert np.array_equal(d, S.blob_density2d(24, 32, np.random.RandomState(1)))
    v = S.curl_velocity2d(24, 32, np.random.RandomState(1), max_cells=2.0)
    assert v.shape == (24, 32, 2) and v.dtype == np.float32
    cells = np.abs(v) * (np.array([24, 32]) - 1) / 2
    assert abs(cells.max() - 2.0) < 1e-5


@pytest.mark.parametrize("kind", ["v", "d", "sp"])
def test_one_step_of_the_reference_loop_is_the_hand_composed_pieces(kind):
    """12 x 16, one frame, one step: advect2d -> clip -> plugin_to_loss_net -> vgg19_features -> style_loss, autograd,
    one TFAdam step"""
    H, W = 12, 16
    d, u, simg = _case(H, W, 1)
    w = O.synthetic_vgg19_weights(123, upto="conv2_1")
    cfg = dict(grid_variable=kind, num_frames=1, interp=1, frames_per_opt=1, window_sigma=0.0, iter=1, lr=0.01,
               style_layer=["conv1_1", "conv2_1"], w_style_layer=[1.0, 0.5], w_style=1.0, upto="conv2_1")
    init = None if kind == "d" else [R.make_var(kind, H, W, 0.4, 9)]
    hist, outs, vels, imgs = R.sequence_run(cfg, d, u, w, simg, init=init)
    dt = torch.tensor(d[0], dtype=torch.float64)[None, ..., None]
    x0 = dt[0].clone() if kind == "d" else torch.tensor(init[0], dtype=torch.float64)
    x = x0.clone().requires_grad_()
    if kind == "d":
        adv = x[None]
    else:
        def fd(a, axis):
            df = torch.diff(a, dim=axis)
            return torch.cat([df, df.narrow(axis, df.shape[axis] - 1, 1)], dim=axis)
        vel = x if kind == "v" else torch.stack([-fd(x[..., 0], 1) + fd(x[..., 1], 0), fd(x[..., 0], 0) + fd(x[..., 1], 1)], -1)
        adv = O.advect2d(dt, vel[None])
    img = adv.clamp(0, 1)
    feats = O.vgg19_features(O.plugin_to_loss_net(img), w, "conv2_1")
    sfe = O.style_target_features(torch.tensor(simg, dtype=torch.float64)[None], w, cfg["style_layer"], upto="conv2_1")
    loss, _ = O.style_loss(feats, sfe, cfg["style_layer"], cfg["w_style_layer"], 1.0)
    (g,) = torch.autograd.grad(loss, x)
    new = O.TFAdam().step(x0, g, 0.01)
    new = x0 + (new - x0) * (dt[0] if kind == "d" else 1.0)      # (update = new - old, 'd' masked; then g_opt += update)
    loss = loss.detach()
    assert hist == [[float(loss)]]
    # (float64; autograd may sum the two parts' gradients in another order than the hand composition: 1e-12, not bits)
    np.testing.assert_allclose(outs[0], new.numpy(), rtol=1e-12, atol=1e-15)
    assert imgs[0].shape == (H, W, 1) and imgs[0].min() >= 0 and imgs[0].max() <= 1
    lg = R.loss_and_gradient(kind, d[0], x0.numpy(), cfg, w, sfe)
    assert lg[0] == float(loss)
    np.testing.assert_allclose(lg[1], g.numpy(), rtol=1e-12, atol=1e-18)

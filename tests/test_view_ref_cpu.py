"""tests/view_ref.py against torch autograd through the oracle (oracle.rotate, oracle.render, oracle.render_unnormalised)
in float64, and its weight-count helper against the tiled rotate adjoint's fixed-point bound."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import view_ref as VR


def _rot(th, ph, scale=1.0):
    import neural_flow_style_amd.transform as T
    return torch.tensor(scale * (T.rot_y_3d(th) @ T.rot_z_3d(ph)), dtype=torch.float32)


CASES = [
    ((7, 6, 9), _rot(0.0, 0.0)),
    ((7, 6, 9), _rot(40.0, -25.0)),            # large angle: many clamped samples
    ((9, 5, 8), _rot(-60.0, 35.0, 1.4)),       # scaled: whole corner regions clamp onto one voxel
    ((1, 6, 7), _rot(20.0, 10.0)),             # an axis of length 1
    ((8, 1, 5), _rot(-30.0, 15.0, 0.7)),
]


def _volume(shape, seed):
    return torch.tensor(np.random.RandomState(seed).uniform(-0.3, 1.0, shape), dtype=torch.float64)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_rotate_and_adjoint_match_oracle(case):
    shape, R = CASES[case]
    d = _volume(shape, case).requires_grad_()
    ref = O.rotate(d[None, ..., None], R.double()[None])[0, ..., 0]
    st = VR.Stencil(R, shape)
    s, err = st.sample(d.detach())
    assert float((s - ref.detach()).abs().max()) <= 1e-12
    assert bool((err > 0).all())
    g = torch.tensor(np.random.RandomState(10 + case).randn(*shape))
    (gd,) = torch.autograd.grad(ref, d, g, retain_graph=True)
    sc = st.scatter(g)
    assert float((sc["ref"] - gd).abs().max()) <= 1e-12 * max(1.0, float(gd.abs().max()))
    # the magnitudes bound the adjoint; with g = 1 the adjoint is the weight count
    assert bool((sc["m1"] >= sc["ref"].abs() - 1e-12).all())
    w = VR.weight_per_voxel(R, shape)
    (w_o,) = torch.autograd.grad(ref, d, torch.ones(shape, dtype=torch.float64))
    assert float((w - w_o).abs().max()) <= 1e-11


@pytest.mark.parametrize("case", range(len(CASES)))
def test_ray_modes_match_oracle(case):
    shape, R = CASES[case]
    tau = 0.3
    s = torch.tensor(np.random.RandomState(case).uniform(0.0, 2.0, shape)).requires_grad_()
    g = torch.tensor(np.random.RandomState(5 + case).randn(*shape[1:]))
    r = VR.ray(s.detach(), torch.zeros(shape, dtype=torch.float64), tau, g)
    x = s[None, ..., None]
    for mode, key in (("img", "img"), (True, "liquid"), ("max", "max"), ("mean", "mean")):
        if mode == "img":
            out = O.render_unnormalised(x, tau)[0, ..., 0]
        else:
            out = O.render(x, tau, liquid=mode)[0, ..., 0]
        assert float((r[key] - out.detach()).abs().max()) <= 1e-12, key
        (gs,) = torch.autograd.grad(out, s, g, retain_graph=True)
        gk = {"img": "grad", "liquid": "grad_liquid", "max": "grad_max", "mean": "grad_mean"}[key]
        assert float((r[gk] - gs).abs().max()) <= 1e-12, gk
    assert float((r["raysum"] - s.detach().sum(0)).abs().max()) <= 1e-12
    # the closed form the oracle keeps for the same adjoint
    cf = O.render_adjoint_closed_form(s.detach()[None, ..., None], tau, g[None, ..., None])[0, ..., 0]
    assert float((r["grad"] - cf).abs().max()) <= 1e-12


def test_max_mode_splits_ties():
    s = torch.tensor([[1.0, 3.0], [3.0, 2.0], [3.0, 0.5], [0.0, 2.0]])[..., None]      # [D=4, H=2, W=1]
    g = torch.tensor([[6.0], [4.0]])
    r = VR.ray(s, torch.zeros_like(s), 0.1, g)
    assert r["grad_max"][:, 0, 0].tolist() == [0.0, 3.0, 3.0, 0.0]
    assert r["grad_max"][:, 1, 0].tolist() == [4.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("D,seg_len", [(16, 4), (18, 5), (23, 6), (40, 10)])
def test_segments_recombine(D, seg_len):
    """u, the seg triple and (A, B) give back the whole ray's image, ray sum and gradient"""
    H, W, tau = 3, 5, 0.4
    rng = np.random.RandomState(D)
    s = torch.tensor(rng.uniform(0.0, 1.5, (D, H, W)))
    g = torch.tensor(rng.randn(H, W))
    nseg = (D + seg_len - 1) // seg_len
    c = VR.coef(s, torch.zeros_like(s), tau, nseg, seg_len, g)
    r = VR.ray(s, torch.zeros_like(s), tau, g)
    segs = VR.segments(D, seg_len)
    assert sorted(z for lo, hi in segs for z in range(lo, hi + 1)) == list(range(D))
    for z in range(D):
        assert [k for k, (lo, hi) in enumerate(segs) if lo <= z <= hi] == [(D - 1 - z) // seg_len]
    S, Is = c["seg"][0], c["seg"][1]
    P = torch.cumsum(S, 0) - S
    img = (torch.exp(-tau * P) * Is).sum(0)
    assert float((img - r["img"]).abs().max()) <= 1e-12
    assert float((S.sum(0) - r["raysum"]).abs().max()) <= 1e-12
    assert float((c["grad"] - r["grad"]).abs().max()) <= 1e-12
    G, e = VR.coef_grad(c["u"], c["ab"], seg_len)
    assert float((G - r["grad"]).abs().max()) <= 1e-12
    # the per-block bound the coefficient kernel writes: |A| max|u| + |B| >= every sample gradient
    ab = c["ab"]
    bnd = ab[..., 0].abs() * c["seg"][2] + ab[..., 1].abs()
    assert float(bnd.max()) >= float(r["grad"].abs().max()) - 1e-12


def test_bounds_grow_with_sample_error():
    """a sample error budget moves every ray bound, and a zero budget leaves only roundings"""
    s = torch.tensor(np.random.RandomState(3).uniform(0.0, 1.0, (20, 4, 4)))
    g = torch.ones(4, 4, dtype=torch.float64)
    r0 = VR.ray(s, torch.zeros_like(s), 0.05, g)
    r1 = VR.ray(s, torch.full_like(s, 1e-6), 0.05, g)
    for k in ("e_raysum", "e_img", "e_liquid", "e_grad", "e_max"):
        assert bool((r1[k] > r0[k]).all()), k
    assert float(r0["e_img"].max()) < 1e-4 * float(r0["img"].abs().max())


def _weight_max(R, G):
    return float(VR.weight_per_voxel(R, (G, G, G)).max())


@pytest.mark.parametrize("G", [24, 64])
def test_rotation_weights_stay_below_the_fixed_point_bound(G):
    """the tiled adjoint's launcher bound (4 max(D,H,W) per view + 8) holds for rotations, with margin; it does not
    for a scaled matrix -- the kernel raises it for any view that is no rotation"""
    from neural_flow_style_amd import synthetic as S
    bf1 = VR.bound_factor(1, (G, G, G))
    mats = [torch.tensor(np.asarray(m, np.float32)) for m in S.uniform_views(8)] + [_rot(45.0, 35.0), _rot(-60.0, 40.0)]
    for R in mats:
        assert _weight_max(R, G) < bf1 / 2
    # 1.4 x identity clamps a corner region of ~(0.14 G)^3 samples onto the corner voxel
    # a 0.1x shrink stacks ~1000 samples in every interior voxel
    if G == 64:
        assert _weight_max(torch.eye(3) * 1.4, G) > bf1
        w = VR.weight_per_voxel(torch.eye(3) * 0.1, (G, G, G))
        assert 900 < float(w[30:34, 30:34, 30:34].min()) and float(w.max()) > bf1


def test_scaled_matrix_weight_at_100():
    """1.4 x identity at 100^3 puts ~2.8k weight on the corner voxel; the launcher bound is 408, the int64 sums wrap
    past 1024 at max |g| = 1 -- the case test_view_path_gpu.py runs with g = 1"""
    w = VR.weight_per_voxel(torch.eye(3) * 1.4, (100, 100, 100))
    assert VR.bound_factor(1, (100,) * 3) == 408.0
    assert 2700 < float(w.max()) < 4000 and float(w[0, 0, 0]) == float(w.max())

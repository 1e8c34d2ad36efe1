"""tests/maccormack_ref.py pinned without a GPU: its closed-form adjoint against torch.autograd through the oracle's
MacCormack scheme in float64 (the oracle's own limiter decisions as ``keep``, its float64 first-order sample as
``d_fwd``), and the two conditions that keep the GPU test honest on the shapes and seeds it runs: few voxels near a
cell face, and a limiter that fires on a share of the elements that gives both branches of the adjoint weight."""
import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import maccormack_ref as MR


def _oracle_pieces(d, v):
    """float64 tensors with a leading batch axis, the oracle's d_fwd and its limiter decisions"""
    d64 = torch.tensor(d, dtype=torch.float64)[None].requires_grad_()
    v64 = torch.tensor(v, dtype=torch.float64)[None].requires_grad_()
    dims = d.shape[:-1]
    g = O.mgrid(*dims, dtype=torch.float64).unsqueeze(0)
    vp = v64.permute(0, len(dims) + 1, *range(1, len(dims) + 1))
    warp = O.batch_warp3d if len(dims) == 3 else O.batch_warp2d
    with torch.no_grad():
        F = warp(d64, g - vp, [1, *dims])
        B = warp(F, g + vp, [1, *dims])
        A = F + (d64 - B) * 0.5
        lo, hi = O._stencil_extrema(d64, g - vp)
        keep = (A > hi) | (lo > A)
    return d64, v64, F[0].numpy(), keep[0].numpy()


@pytest.mark.parametrize("case", MR.CASES, ids=lambda c: c[0])
def test_reference_adjoint_is_autograd_through_the_oracle_in_float64(case):
    d, v, rng = MR.make_case(case)
    d64, v64, F, keep = _oracle_pieces(d, v)
    g = rng.randn(*d.shape)
    out = O.advect_maccormack(d64, v64)
    (out * torch.tensor(g)[None]).sum().backward()
    ref = MR.adjoint(d64[0].detach().numpy(), v64[0].detach().numpy(), F, keep, g)
    # g_vel where a trace sits on a lattice node (the 'integer' cases; float64 rounding decides the side there): the
    # nearest of the candidates the two cells sharing the face give -- elsewhere the candidates are one and the same
    want_v = v64.grad[0].numpy()
    near_v = np.abs(ref["vel_cand"] - want_v[None, None]).min(axis=(0, 1))
    if case[3] == "random":
        assert not ref["unsure"].any() or np.abs(ref["g_vel"] - want_v)[~ref["unsure"]].max() <= 1e-10 * np.abs(want_v).max()
    for name, err_map, want in (("g_d", np.abs(ref["g_d"] - d64.grad[0].numpy()), d64.grad[0].numpy()),
                                ("g_vel", near_v, want_v)):
        scale = max(float(np.abs(want).max()), 1e-300)
        err = float(err_map.max())
        print("%-14s %-5s max |ref - autograd| / max|grad| = %.2e" % (case[0], name, err / scale))
        assert err <= 1e-10 * scale, (case[0], name, err, scale)
    # both branches of the adjoint are exercised, and an element's gradient moves by more than any bound when its
    # decision is flipped: the mask matters
    if keep.any() and not keep.all():
        flipped = MR.adjoint(d64[0].detach().numpy(), v64[0].detach().numpy(), F, ~keep, g)
        assert np.abs(flipped["g_d"] - ref["g_d"]).max() > 1e-3


@pytest.mark.parametrize("case", [c for c in MR.CASES if c[3] == "random"], ids=lambda c: c[0])
def test_gpu_cases_have_few_unsure_voxels_and_a_limiter_that_fires(case):
    """the float32 inputs of the GPU test: at most 1 % of the voxels within 1e-4 cells of a face (where the test accepts
    either neighbouring cell's derivative), and the limiter fires on 5 ... 50 % of the elements"""
    d, v, rng = MR.make_case(case)
    _, _, F, keep = _oracle_pieces(d, v)
    ref = MR.adjoint(d, v, F.astype(np.float32), keep, rng.randn(*d.shape).astype(np.float32))
    unsure, fired = float(ref["unsure"].mean()), float(keep.mean())
    print("%-14s unsure %.2f %%, limiter fires on %.1f %% of the elements" % (case[0], 100 * unsure, 100 * fired))
    assert unsure <= 0.01, (case[0], unsure)
    assert 0.05 <= fired <= 0.50, (case[0], fired)


def test_bounds_are_small_against_the_gradients_and_cover_a_float32_replay():
    """the bounds must bite (a few 1e-5 of the gradient scale on these grids, not a loose tolerance) and must cover a
    float32 evaluation of the same formulas on the host"""
    case = MR.CASES[0]
    d, v, rng = MR.make_case(case)
    _, _, F, keep = _oracle_pieces(d, v)
    F32 = F.astype(np.float32)
    g = rng.randn(*d.shape).astype(np.float32)
    ref = MR.adjoint(d, v, F32, keep, g)
    sd, sv = np.abs(ref["g_d"]).max(), np.abs(ref["g_vel"]).max()
    assert np.median(ref["bound_d"]) < 1e-5 * sd and ref["bound_d"].max() < 1e-3 * sd
    assert np.median(ref["bound_vel"]) < 1e-4 * sv and ref["bound_vel"].max() < 1e-2 * sv
    assert ref["quantum"] < 2.0 ** -30 * np.abs(g).max()
    # mask round trip as the kernels pack it
    words = np.zeros((keep.size + 63) // 64, dtype=np.uint64)
    e = np.flatnonzero(keep.reshape(-1)).astype(np.uint64)
    np.bitwise_or.at(words, (e >> np.uint64(6)).astype(np.int64), np.uint64(1) << (e & np.uint64(63)))
    assert np.array_equal(MR.unpack_mask(words.view(np.int64), keep.shape), keep)

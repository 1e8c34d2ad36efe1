"""libnfs_emission.so element by element.  Every output is ONE rounding of a product the existing entry points also form,
so every comparison is for equality: emission_fwd against colour_clamp_gather(c) * e, emission_bwd against
clamp01_bwd(g_q, c) * e, the fused Adam form against emission_bwd + adam_tf_step over three consecutive steps.

Voxel counts 1, 5, 105 (5 * 7 * 3: n * C is no multiple of 4 at C = 1, 3) and 2^20 + 3 (many blocks and a tail lane), C = 1..4,
aligned arrays and views offset by one float (the 16-byte path must fall back).  The colours hold exact 0, exact 1, -0.0,
values below and above the range and a NaN; e holds +0.0, -0.0 (a run of each, as empty space is) and positive values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 105, (1 << 20) + 3]
SPECIAL = [0.0, 1.0, -0.0, -0.25, 1.25, float("nan")]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _off(t, offset):
    """the same values in a buffer whose base is 16-byte aligned (offset 0) or one float past that (offset 1)"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * offset
    return v


def _inputs(n, C, seed, offset):
    g_ = torch.Generator().manual_seed(seed)
    c = torch.rand(n, C, generator=g_) * 1.6 - 0.3
    e = torch.rand(n, generator=g_) * 1.9 + 0.1
    g = (torch.rand(n, C, generator=g_) + 0.5) * torch.where(torch.rand(n, C, generator=g_) < 0.5, -1.0, 1.0)
    flat = c.view(-1)
    for i, s in enumerate(SPECIAL):                    # (every special colour the array has room for, scattered)
        for pos in {(7 * i + 3) % flat.numel(), (flat.numel() - 1 - i) % flat.numel(), (1031 * (i + 1)) % flat.numel()}:
            flat[pos] = s
    if n >= 5:
        e[n // 5: n // 5 + max(n // 10, 1)] = 0.0      # runs of empty space: +0.0 and the ReLU's -0.0
        e[n // 2: n // 2 + max(n // 10, 1)] = -0.0
    return [_off(t.cuda(), offset) for t in (c, e, g)]


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_values(got, ref):
    """equal as values (torch.equal: -0.0 == +0.0, NaN equals nothing), NaN positions compared on their own"""
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, ref)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_forward_equals_clamp_times_e(n, C, offset):
    from neural_flow_style_amd import ops
    c, e, _ = _inputs(n, C, 100 * C + offset, offset)
    c0, e0 = c.clone(), e.clone()
    out = _off(torch.full((n, C), 7.0, device="cuda"), offset)
    got = ops.emission_fwd(c, e, out=out)
    assert got is out
    ref = ops.colour_clamp_gather(c0) * e0.unsqueeze(-1)
    _check_values(got, ref)
    assert torch.equal(torch.signbit(got), torch.signbit(ref))               # the zeros' signs: the same product's
    assert _same_bits(c, c0) and _same_bits(e, e0)                             # the inputs as they were
    if n >= 5:
        assert bool((got[e0 == 0] == 0).all()) and bool((e0 == 0).any())
    # the fresh-output form
    assert _same_bits(ops.emission_fwd(c, e), got)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_adjoint_equals_masked_gradient_times_e(n, C, offset):
    from neural_flow_style_amd import ops
    c, e, g = _inputs(n, C, 200 * C + offset, offset)
    c0, e0, g0 = c.clone(), e.clone(), g.clone()
    out = _off(torch.full((n, C), 7.0, device="cuda"), offset)
    got = ops.emission_bwd(g, c, e, out=out)
    ref = ops.clamp01_bwd(g0, c0) * e0.unsqueeze(-1)
    _check_values(got, ref)
    inside = (c0 >= 0) & (c0 <= 1)                                             # (exact 0, exact 1 and -0.0 are inside; NaN is not)
    assert torch.equal(torch.signbit(got)[inside], torch.signbit(ref)[inside])
    assert not bool(torch.signbit(got)[~inside].any())                         # outside: +0
    assert bool((got[~inside] == 0).all())
    assert bool((got[inside & (e0 > 0).unsqueeze(-1)] != 0).all())             # a boundary colour passes its gradient
    assert _same_bits(c, c0) and _same_bits(e, e0) and _same_bits(g, g0)


def _hyper(t, lr=0.01, b1=0.9, b2=0.999, eps=1e-8):
    b1p, b2p = np.float32(b1) ** t, np.float32(b2) ** t
    return float(np.float32(lr) * np.sqrt(np.float32(1) - b2p) / (np.float32(1) - b1p)), b1, b2, eps


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_fused_adam_equals_adjoint_then_adam(n, C, offset):
    """three consecutive steps: c, m and v bit for bit those of emission_bwd followed by adam_tf_step (which takes
    16-byte aligned arrays: the composed side runs on aligned copies)"""
    from neural_flow_style_amd import ops
    c, e, _ = _inputs(n, C, 300 * C + offset, offset)
    e0 = e.clone()
    m, v = _off(torch.zeros(n, C, device="cuda"), offset), _off(torch.zeros(n, C, device="cuda"), offset)
    c2, m2, v2 = c.clone(), torch.zeros(n, C, device="cuda"), torch.zeros(n, C, device="cuda")
    for t in (1, 2, 3):
        g = _inputs(n, C, 300 * C + offset + 17 * t, offset)[2]
        g0 = g.clone()
        ops.emission_bwd_adam(g, c, e, m, v, *_hyper(t))
        ops.adam_tf_step(c2, m2, v2, ops.emission_bwd(g0, c2, e0), *_hyper(t))
        assert _same_bits(c, c2) and _same_bits(m, m2) and _same_bits(v, v2), t
        assert _same_bits(g, g0) and _same_bits(e, e0)
    assert bool(torch.isfinite(c[~torch.isnan(c2)]).all())
    if n >= 105:
        assert bool((m != 0).any()) and not _same_bits(c, _inputs(n, C, 300 * C + offset, offset)[0])      # it moved


def test_the_state_takes_the_fused_form():
    """TFAdamState.step_through_emission against TFAdamState.step on the stand-alone adjoint"""
    from neural_flow_style_amd import engine, ops
    c, e, _ = _inputs(105, 3, 5, 0)
    c, c2 = c.view(5, 7, 3, 3).contiguous(), c.view(5, 7, 3, 3).clone()
    e = e.view(5, 7, 3).contiguous()
    A, B = engine.TFAdamState(), engine.TFAdamState()
    for t in range(3):
        g = _inputs(105, 3, 50 + t, 0)[2].view(5, 7, 3, 3).contiguous()
        A.step_through_emission(c, e, g, 0.02)
        B.step(c2, ops.emission_bwd(g, c2, e), 0.02)
    assert _same_bits(c, c2) and _same_bits(A.m, B.m) and _same_bits(A.v, B.v)


def test_device_pointer_refusals():
    from neural_flow_style_amd import _lib, ops
    c, e, g = _inputs(105, 3, 9, 0)
    m, v = torch.zeros_like(c), torch.zeros_like(c)
    p = ops._ptr
    with pytest.raises(_lib.NfsError, match="must not alias"):
        ops.emission_fwd(c, e, out=c)
    with pytest.raises(_lib.NfsError, match="must not alias"):
        ops.emission_bwd(g, c, e, out=g)
    with pytest.raises(_lib.NfsError, match="must not alias"):
        ops.emission_bwd(g, c, e, out=c)
    with pytest.raises(_lib.NfsError, match="must not alias"):
        ops.emission_bwd_adam(g, c, e, m, m, 1e-3)
    with pytest.raises(_lib.NfsError, match="must not alias"):
        ops.emission_bwd_adam(g, c, e, g, v, 1e-3)
    with pytest.raises(_lib.NfsError, match="must not alias"):
        ops.emission_bwd_adam(g, c, e, c, v, 1e-3)
    q = torch.empty_like(c)
    for bad_n in (0, -3):
        with pytest.raises(_lib.NfsError, match="n must be at least 1"):
            _lib.call("nfs_emission_fwd", p(c), p(e), p(q), bad_n, 3, ops._stream())
    for bad_C in (0, 5):
        with pytest.raises(_lib.NfsError, match="C must be 1..4"):
            _lib.call("nfs_emission_bwd", p(g), p(c), p(e), p(q), 105, bad_C, ops._stream())
    with pytest.raises(_lib.NfsError, match="null pointer"):
        _lib.call("nfs_emission_bwd_adam", p(g), p(c), None, p(m), p(v), 105, 3, 1e-3, 0.9, 0.999, 1e-8, ops._stream())
    with pytest.raises(ValueError, match="grey volume"):
        ops.emission_fwd(c, e[:-1].contiguous())

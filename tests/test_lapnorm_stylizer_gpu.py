"""optimizer='lapnorm' through the grid stylizers: ``engine.GridStylizer`` on a 12 x 10 x 14 grid with two views,
``grid2d.GridStylizer2D`` on 24 x 20, ``styler_grid.Styler`` in both dimensions; thinned synthetic VGG, style layers conv1_1,
conv2_1, conv3_1.  The optimizer's tests do not depend on the loss chain (which has its own): the gradient is taken from the
stylizer and the update is held to the rule  x <- fma(-lr, lap_normalize(g), x)  element by element."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lapnorm_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ["conv1_1", "conv2_1", "conv3_1"]
TARGETS = ("v", "s", "p", "sp", "d")
SHAPE3, SHAPE2 = (12, 10, 14), (24, 20)
# a length in the variable's units: a third of a cell of the shortest axis per pyramid level and step ('d': a density step)
LR3, LR2 = (1.0 / 3.0) * 2.0 / (SHAPE3[1] - 1), (1.0 / 3.0) * 2.0 / (SHAPE2[1] - 1)


def T(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def same(a, b):
    return torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def case3():
    """density (a 14^3 blob field cropped to 12 x 10 x 14), two views, the loss -- built once, read only"""
    from neural_flow_style_amd import engine, vgg
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd import transform as Tr
    rng = np.random.RandomState(17)
    d0 = np.ascontiguousarray(S.blob_density(14, rng)[1:13, 2:12, :])
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv3_1"), "cuda:0")
    loss = engine.RenderStyleLoss(net, LAYERS, [1.0] * 3, 1.0, transmit=0.05)
    loss.set_style_image(S.style_image(SHAPE3[1], SHAPE3[2], rng))
    return d0, Tr.rot_to_device(S.uniform_views(2), "cuda:0"), loss


@functools.lru_cache(maxsize=None)
def case2():
    from neural_flow_style_amd import engine, vgg
    from neural_flow_style_amd import synthetic as S
    rng = np.random.RandomState(19)
    d0 = S.blob_density2d(*SHAPE2, rng)
    net = vgg.VGG(vgg.synthetic_weights(123, upto="conv3_1"), "cuda:0")
    loss = engine.ImageStyleLoss(net, LAYERS, [1.0] * 3, 1.0)
    loss.set_style_image(S.style_image(*SHAPE2, rng))
    return d0, loss


def make3(kind, order=1, **kw):
    from neural_flow_style_amd import engine
    d0, rot, loss = case3()
    kw.setdefault("lr", LR3)
    gs = engine.GridStylizer(loss, T(d0), k=3, target=kind, optimizer="lapnorm", adv_order=order, **kw)
    return gs, (lambda: gs.gradient(rot)), (lambda: gs.step(rot))


def make2(kind, order=1, **kw):
    from neural_flow_style_amd.grid2d import GridStylizer2D
    d0, loss = case2()
    kw.setdefault("lr", LR2)
    gs = GridStylizer2D(loss, T(d0), target=kind, optimizer="lapnorm", adv_order=order, **kw)
    return gs, gs.gradient, gs.step


def channels_last(g, nd):
    grid = tuple(g.shape[:nd])
    return g.reshape(grid + (g.numel() // int(np.prod(grid)),))


# ---- one step is the rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", TARGETS)
@pytest.mark.parametrize("nd", [3, 2])
def test_three_steps_are_the_rule_element_by_element(nd, kind, order):
    from neural_flow_style_amd import engine, util
    gs, gradient, step = (make3 if nd == 3 else make2)(kind, order, graph=False)
    assert isinstance(gs.adam, engine.LapDescentState) and gs.adam.lap_n == 3
    if kind != "d":
        assert float(gs.var.abs().max()) == 0                     # a zero start
    for i in range(3):
        before = gs.var.clone()
        _, g = gradient()
        assert tuple(g.shape) == tuple(gs.var.shape) or g.numel() == gs.var.numel()
        g32 = util.lap_normalize(channels_last(g.contiguous(), nd), scale_n=3, is_3d=nd == 3)
        want64 = R.normalized(channels_last(g, nd).cpu().numpy(), 3, nd == 3)
        r = R.rel(g32.cpu().numpy(), want64)
        loss = float(step())
        ok, worst = R.one_rounding(gs.var.cpu().numpy().reshape(-1), before.cpu().numpy().reshape(-1), gs.lr,
                                   g32.cpu().numpy().reshape(-1))
        moved = float((gs.var - before).abs().max())
        print("%d-D %-2s order %d step %d: loss %.5g, g^ rel L2 %.2e, worst %.3f of one rounding, max |dx| %.3g"
              % (nd, kind, order, i, loss, r, worst, moved))
        assert np.isfinite(loss) and float(g.abs().max()) > 0 and moved > 0
        assert r < 2e-5
        assert ok, worst


# ---- bit identities -------------------------------------------------------------------------------------------------------------
def same_losses(nd, la, lb):
    """3-D: the very numbers.  2-D: the variable is held to bits; the loss SCALAR of ``engine.ImageStyleLoss`` is summed with
    float atomics and differs in its last bit between two identical eager calls (seen here: 15813878.0 against 15813877.0 at
    step 0, before any update), so it is held to the bar tests/test_grid2d_stylizer_gpu.py holds it to, rtol 1e-5"""
    if nd == 3:
        return la == lb
    np.testing.assert_allclose(la, lb, rtol=1e-5)
    return True


def _three_steps(make, kind, monkeypatch, env=None, **kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    gs, _, step = make(kind, 1, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return [float(step()) for _ in range(3)], gs


@pytest.mark.parametrize("nd", [3, 2])
def test_the_fused_step_is_the_composition_bit_for_bit(nd, monkeypatch):
    """NFS_FUSE_ADVECT=0 (descent_step, then the forward advect by itself) against the default ('v', order 1)"""
    make = make3 if nd == 3 else make2
    la, a = _three_steps(make, "v", monkeypatch, graph=False)
    lb, b = _three_steps(make, "v", monkeypatch, env={"NFS_FUSE_ADVECT": "0"}, graph=False)
    assert a.fuse_advect and not b.fuse_advect
    if nd == 3:
        assert a._adv_target() is not None and a._adv_valid() and b._adv_target() is None
    assert same(a.var, b.var) and same_losses(nd, la, lb)
    assert float(a.var.abs().max()) > 0


@pytest.mark.parametrize("kind", ["v", "sp", "d"])
@pytest.mark.parametrize("nd", [3, 2])
def test_graph_replay_is_the_eager_step_bit_for_bit(nd, kind, monkeypatch):
    make = make3 if nd == 3 else make2
    la, a = _three_steps(make, kind, monkeypatch, graph=False)
    lb, b = _three_steps(make, kind, monkeypatch, graph=True)
    assert a._replay is None or a._replay.graph is None
    assert b._replay is not None and b._replay.graph is not None
    assert same(a.var, b.var) and same_losses(nd, la, lb)


def test_dead_region_skipping_leaves_every_bit(monkeypatch):
    la, a = _three_steps(make3, "v", monkeypatch, graph=False)
    lb, b = _three_steps(make3, "v", monkeypatch, env={"NFS_DEAD_SKIP": "0"}, graph=False)
    assert a.dead_skip and not b.dead_skip
    assert bool(a._live_kw()) and not b._live_kw()               # (the mask the fused update wrote is in use)
    assert same(a.var, b.var) and la == lb


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------
_RANK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from neural_flow_style_amd import engine, vgg
from neural_flow_style_amd import synthetic as S, transform as T
world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) %% torch.cuda.device_count())
torch.cuda.set_device(dev)
if world > 1:
    dist.init_process_group("gloo")
G, V = 16, 4
rng = np.random.RandomState(5)
d0 = S.blob_density(G, rng)
simg = S.style_image(G, G, rng)
net = vgg.VGG(vgg.synthetic_weights(123, upto="conv3_1"), dev)
loss = engine.RenderStyleLoss(net, ["conv1_1", "conv2_1", "conv3_1"], [1.0] * 3, 1.0, transmit=0.02)
loss.set_style_image(simg)
gs = engine.GridStylizer(loss, torch.tensor(d0, device=dev), k=3, target="v", lr=0.5 * 2 / (G - 1), optimizer="lapnorm",
                         process_group=dist.group.WORLD if world > 1 else None)
assert gs.slab is None
gs.var.copy_(torch.tensor(S.curl_velocity(G, rng, max_cells=0.5)))
rot = T.rot_to_device(S.uniform_views(V), dev)[rank::world].contiguous()
ls = [float(gs.step(rot)) for _ in range(3)]
np.savez(sys.argv[1] + ".%%d.npz" %% rank, l=np.asarray(ls), var=gs.var.cpu().numpy())
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


def test_two_ranks_sharing_the_views_keep_bit_identical_replicas(tmp_path):
    """views sharded over two gloo ranks on one GPU: the all-reduce mode (the normalisation must see the summed gradient;
    ``gs.slab is None`` is asserted in every rank), the bound of the other two-rank grid tests -- after the steps both
    replicas of the variable are bit-identical, both ranks report the same losses, and the first loss is the one-rank
    run's to rtol 2e-6"""
    from tests.ranks import require_gpus_for, run_ranks
    require_gpus_for(2)
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NFS_SLAB_SHARD"):
        env.pop(k, None)
    subprocess.run([sys.executable, str(script), str(tmp_path / "one")], check=True, env=env, timeout=300)
    run_ranks([sys.executable, str(script), str(tmp_path / "two")], 2, env, timeout=300)
    one = np.load(str(tmp_path / "one") + ".0.npz")
    r0, r1 = (np.load(str(tmp_path / "two") + ".%d.npz" % r) for r in (0, 1))
    assert np.array_equal(r0["var"].view(np.int32), r1["var"].view(np.int32))
    assert np.array_equal(r0["l"], r1["l"])
    np.testing.assert_allclose(r0["l"][0], one["l"][0], rtol=2e-6)
    print("lapnorm losses, one rank:", one["l"], "two ranks:", r0["l"])


# ---- styler_grid ---------------------------------------------------------------------------------------------------------------------
def test_styler_run_follows_the_cosine_schedule_bit_for_bit():
    """lr_decay = 2, iter = 3, one key frame, one octave: result['opt'] is the test's own loop over
    ``engine.GridStylizer.step`` with ``gs.lr = util.cosine_decay(i, 3, lr, 2)`` set before step i (and the frame loop's
    re-assignment g_opt += nan_to_num(var) - g_opt between the steps): the schedule is wired and is the reference's"""
    from neural_flow_style_amd import engine, util
    from neural_flow_style_amd.styler_grid import Styler
    from tests.test_sequence_gpu import _cfg_for, sequence_case, v_init_for
    G, lr = 16, 0.4 * 2 / 15
    d, u, simg = sequence_case(G, 1)
    vi = v_init_for(G, 1)
    st = Styler(_cfg_for(G, 1, simg, optimizer="lapnorm", lap_n=3, lr_decay=2.0, iter=3, lr=lr, window_sigma=0.0))
    st.load_img([G, G])
    res = st.run({"d": d, "v": u, "v_init": vi})
    assert np.isfinite(res["l_frames"]).all() and np.asarray(res["l_frames"]).shape == (3, 1)

    gs = engine.GridStylizer(st.loss, T(d[0]), k=st.k, target="v", lr=lr, optimizer="lapnorm", lap_n=3)
    g_opt, lrs = T(vi[0]), []
    for i in range(3):
        gs.var.copy_(g_opt)
        gs.lr = float(util.cosine_decay(i, 3, lr, 2.0))
        lrs.append(gs.lr)
        gs.step(st._rot())
        g_opt = g_opt + (torch.nan_to_num(gs.var) - g_opt)
    assert lrs[0] == pytest.approx(2 * lr) and lrs[0] > lrs[1] > lrs[2] > lr
    assert same(T(res["opt"][0]), g_opt)
    # ... and not the constant-lr run
    flat = Styler(_cfg_for(G, 1, simg, optimizer="lapnorm", iter=3, lr=lr, window_sigma=0.0))
    flat.load_img([G, G])
    assert not np.array_equal(flat.run({"d": d, "v": u, "v_init": vi})["opt"][0], res["opt"][0])


def test_styler_smoke_3d_two_key_frames_two_octaves_helmholtz_pair():
    from neural_flow_style_amd.styler_grid import Styler
    from tests.test_sequence_gpu import _cfg_for, sequence_case
    G = 16
    d, u, simg = sequence_case(G, 2)
    st = Styler(_cfg_for(G, 2, simg, grid_variable="sp", optimizer="lapnorm", lap_n=3, lr_decay=2.0, iter=2,
                         lr=0.3 * 2 / (G - 1), window_sigma=1.0, octave_n=2, octave_scale=2))
    st.load_img([G, G])
    res = st.run({"d": d, "v": u})
    assert res["octave_sizes"] == [[8, 8, 8], [G, G, G]] and len(res["l"]) == 2
    assert np.isfinite(np.asarray(res["l_frames"])).all() and np.asarray(res["l_frames"]).shape == (4, 2)
    assert len(res["opt"]) == 2 and all(x.shape == (G, G, G, 4) and np.isfinite(x).all() for x in res["opt"])
    assert all(x.shape == (G, G, G, 3) and np.isfinite(x).all() for x in res["v"])
    assert res["d"].shape == (2, G, G, G, 1) and np.isfinite(res["d"]).all()
    assert any(np.abs(x).max() > 0 for x in res["opt"])


def test_styler_smoke_2d_velocity():
    from tests.test_grid2d_stylizer_gpu import H, W, _styler, sequence_case
    d, u, simg = sequence_case(1)
    res = _styler(1, simg, optimizer="lapnorm", lap_n=3, lr_decay=2.0, iter=3, lr=0.3 * 2 / (H - 1), window_sigma=0.0).run(
        {"d": d[:1], "v": u[:1]})
    assert np.isfinite(np.asarray(res["l_frames"])).all() and np.asarray(res["l_frames"]).shape == (3, 1)
    assert res["opt"][0].shape == (H, W, 2) and np.isfinite(res["opt"][0]).all() and np.abs(res["opt"][0]).max() > 0
    assert res["d"].shape == (1, H, W, 1) and np.isfinite(res["d"]).all() and res["r"].shape == (1, H, W, 3)


# ---- construction errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", ["styler_3p", "styler_2p"])
def test_particle_stylers_refuse_lapnorm(module):
    """a pyramid needs a grid; particle attributes have none"""
    import importlib
    from tests.test_sequence_gpu import _config
    Styler = importlib.import_module("neural_flow_style_amd." + module).Styler
    with pytest.raises(ValueError, match="optimizer lapnorm"):
        Styler(_config(optimizer="lapnorm"))
    with pytest.raises(ValueError, match="lap_n"):
        Styler(_config(optimizer="adam", lap_n=-1))
    with pytest.raises(ValueError, match="lr_decay"):
        Styler(_config(optimizer="adam", lr_decay=0.0))

"""The grid-sequence stylizer coarse to fine (``styler_grid.Styler`` with ``octave_n`` > 1): 20^3 run as 11^3 -> 20^3
(20 // 1.8 = 11), F = 3 frames, 2 views, iter = 2, style layers up to conv3_1 -- against the oracle's loop octave by
octave, against its own composition out of one-octave runs, and over two ranks."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import nfs_oracle as O
from tests import ranks
from tests import resize_ref as R
from tests.test_sequence_gpu import _cfg_for, rel, sequence_case, v_init_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, Gc, F, ITER = 20, 11, 3, 2
FULL, COARSE = (G, G, G), (Gc, Gc, Gc)
# The learning rate of the run that is held to the oracle.  The first Adam step of an octave moves every component by
# +-lr whatever the size of its gradient (m / sqrt(v) = g / |g|), so a component whose gradient is at the rounding floor
# takes its sign from the last bit of the chain, and that bit depends on state outside the test (which kernels earlier
# tests of the process have run).  One such component is off by 2 lr.  v_init_for draws the variable at 0.3 / (G - 1) per
# component: at a tenth of that a decision of this kind moves the variable by a fifth of its own size in one voxel, not
# by more than its size (lr = 0.02, the default of _cfg_for, is 1.3 times the variable at G = 20), and the comparison
# measures the loop.  The bars are those of test_grid_sequence_matches_oracle_loop either way.
LR_ORACLE = 0.03 / (G - 1)


@functools.lru_cache(maxsize=None)
def _case():
    d, u, simg = sequence_case(G, F)
    return d, u, simg, v_init_for(G, F)


def _init_for(kind, seed=30):
    """small non-zero initial variables at full resolution ('v': tests.test_sequence_gpu.v_init_for)"""
    if kind == "v":
        return _case()[3]
    C = {"s": 3, "sp": 4}[kind]
    rng = np.random.RandomState(seed)
    return [(rng.randn(G, G, G, C) * 0.3 / (G - 1)).astype(np.float32) for _ in range(F)]


def _styler(res=G, **over):
    from neural_flow_style_amd.styler_grid import Styler
    simg = _case()[2]
    st = Styler(_cfg_for(res, F, simg, iter=ITER, **over))
    st.load_img([res, res])
    return st


def _factor(kind, n_in, n_out):
    return 1.0 if kind == "v" else float(R.potential_factor(n_in, n_out))


def _resize_dev(x, size, factor=1.0):
    from neural_flow_style_amd import ops
    return ops.resize3d(torch.tensor(np.asarray(x, np.float32)).cuda(), size, "bilinear", True, factor).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _two_octave_v_run():
    d, u, _, vi = _case()
    st = _styler(octave_n=2, lr=LR_ORACLE)
    return st, st.run({"d": d, "v": u, "v_init": vi})


def test_result_of_a_two_octave_run():
    _, res = _two_octave_v_run()
    assert res["octave_sizes"] == [[Gc] * 3, [G] * 3]
    assert len(res["l"]) == 2 and all(len(l) == ITER * F for l in res["l"])
    assert np.asarray(res["l_frames"]).shape == (2 * ITER, F) and np.isfinite(np.asarray(res["l_frames"])).all()
    assert [x for row in res["l_frames"][:ITER] for x in row] == res["l"][0]
    assert len(res["d_intm"]) == 1 and res["d_intm"][0].shape == (F, Gc, Gc, 3) and res["d_intm"][0].dtype == np.uint8
    assert res["d"].shape == (F, G, G, G, 1) and res["r"].shape == (F, G, G, 3) and res["r"].dtype == np.uint8
    assert len(res["opt"]) == F and all(x.shape == (G, G, G, 3) for x in res["opt"])
    assert len(res["opt_octave"]) == 2
    assert all(res["opt_octave"][0][t].shape == (Gc, Gc, Gc, 3) for t in range(F))
    assert all(np.array_equal(res["opt_octave"][1][t], res["opt"][t]) for t in range(F))


def test_every_octave_matches_the_oracle_loop():
    """octave o against ``O.grid_sequence_run`` at the octave's size on inputs resampled by the restatement; octave 1
    starts from the stylizer's own octave-0 result (Adam's per-voxel sign flips at the noise floor do not compound across
    octaves), so each octave is the situation of test_grid_sequence_matches_oracle_loop and takes its bars"""
    d, u, _, vi = _case()
    st, res = _two_octave_v_run()
    ocfg = dict(vars(_cfg_for(G, F, _case()[2], iter=ITER, lr=LR_ORACLE)))
    ocfg["upto"] = "conv3_1"
    w = O.synthetic_vgg19_weights(123, upto="conv3_1")
    down = lambda xs: [R.resize3d(x, COARSE, "bilinear", True) for x in xs]
    starts = [down(vi), [R.resize3d(res["opt_octave"][0][t], FULL, "bilinear", True) for t in range(F)]]
    inputs = [(down(d), down(u)), (d, u)]
    for o, size in enumerate((COARSE, FULL)):
        cfg_o = dict(ocfg, resolution=list(size))
        simg_o = st._style_feature(st.style_img, list(size[1:]))
        hist, outs, d_fin = O.grid_sequence_run(cfg_o, inputs[o][0], np.stack(inputs[o][1]), w, simg_o, st.rot_mat_,
                                                v_init=starts[o])
        got = np.asarray(res["l_frames"][o * ITER:(o + 1) * ITER])
        print("octave %d losses, worst relative difference %.3g" % (o, np.abs(got / np.asarray(hist) - 1).max()))
        np.testing.assert_allclose(got, hist, rtol=2e-3)
        for t in range(F):
            print("octave %d frame %d variable rel %.3g" % (o, t, rel(res["opt_octave"][o][t], outs[t])))
            assert rel(res["opt_octave"][o][t], outs[t]) < 2e-2, (o, t)
            if o == 1:
                print("frame %d density rel %.3g" % (t, rel(res["d"][t], d_fin[t])))
                assert rel(res["d"][t], d_fin[t]) < 1e-3, t


@pytest.mark.parametrize("kind", ("v", "sp"))
def test_hand_off_between_octaves_is_the_resample_bit_for_bit(kind):
    from neural_flow_style_amd import ops
    d, u = _case()[:2]
    init = _init_for(kind)
    st = _styler(octave_n=2, grid_variable=kind)
    st.prepare({"d": d, "v": u, kind + "_init": init})
    f_in = _factor(kind, FULL, COARSE)
    for t, x in st.key_frame_variables().items():                  # octave 0 starts from the resampled '_init'
        assert torch.equal(x, ops.resize3d(torch.tensor(init[t]).cuda(), COARSE, "bilinear", True, f_in)), t
    st.iterate()
    before = {t: x.clone() for t, x in st.key_frame_variables().items()}
    assert st.next_octave() == list(FULL)
    after = st.key_frame_variables()
    f = _factor(kind, COARSE, FULL)
    assert kind == "v" or f == float(np.float32(19.0 / 10.0))
    for t in range(F):
        assert tuple(after[t].shape[:3]) == FULL
        assert torch.equal(after[t], ops.resize3d(before[t], FULL, "bilinear", True, f)), t
    # the inputs of the new octave are the full-resolution originals themselves
    assert all(np.array_equal(st._st.d[t].cpu().numpy(), d[t]) for t in range(F))
    st.iterate()
    res = st.finish()
    assert all(np.array_equal(res["opt_octave"][0][t], before[t].cpu().numpy()) for t in range(F))
    with pytest.raises(ValueError):
        st.next_octave()                                            # there is no third octave


@pytest.mark.parametrize("kind,adv_order", [("s", 1), ("sp", 1), ("v", 2)])
def test_two_octaves_equal_their_composition(kind, adv_order):
    """run A: one octave at 11^3 on inputs resampled with ops.resize3d; run B: one octave at 20^3 starting from A's
    result, resampled with the factor of its kind -- the two-octave run is the same code on the same numbers"""
    d, u = _case()[:2]
    init = _init_for(kind)
    key = kind + "_init"
    both = _styler(octave_n=2, grid_variable=kind, adv_order=adv_order).run({"d": d, "v": u, key: init})
    f_in, f = _factor(kind, FULL, COARSE), _factor(kind, COARSE, FULL)
    a = _styler(Gc, octave_n=1, grid_variable=kind, adv_order=adv_order).run(
        {"d": [_resize_dev(x, COARSE) for x in d], "v": [_resize_dev(x, COARSE) for x in u],
         key: [_resize_dev(x, COARSE, f_in) for x in init]})
    b = _styler(G, octave_n=1, grid_variable=kind, adv_order=adv_order).run(
        {"d": d, "v": u, key: [_resize_dev(x, FULL, f) for x in a["opt"]]})
    np.testing.assert_allclose(both["l"][0], a["l"][0], rtol=1e-5)
    np.testing.assert_allclose(both["l"][1], b["l"][0], rtol=1e-5)
    for t in range(F):
        assert rel(both["opt_octave"][0][t], a["opt"][t]) < 1e-5, t
        assert rel(both["opt"][t], b["opt"][t]) < 1e-5, t
    assert rel(both["d"], b["d"]) < 1e-5


_RANK_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from tests.test_grid_octaves_gpu import _case, _styler
world = int(os.environ.get("WORLD_SIZE", "1"))
torch.cuda.set_device(0)
if world > 1:
    dist.init_process_group("gloo")
d, u, _, vi = _case()
st = _styler(octave_n=2)
if world > 1:
    st.pg = dist.group.WORLD
res = st.run({"d": d, "v": u, "v_init": vi})
if int(os.environ.get("RANK", "0")) == 0:
    np.savez(sys.argv[1], l=np.asarray(res["l_frames"]), opt=np.stack(res["opt"]), d=res["d"],
             n_intm=len(res["d_intm"][0]))
if world > 1:
    dist.barrier(); dist.destroy_process_group()
"""


def test_frames_sharded_over_two_ranks_reproduce_the_single_rank_run(tmp_path):
    """two ranks sharing the one GPU: every rank resamples its own frames and variables, no new exchange"""
    ranks.require_gpus_for(2)
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % {"root": ROOT})
    env = dict(os.environ, PYTHONPATH=ROOT)
    one, two = tmp_path / "one.npz", tmp_path / "two.npz"
    ranks.run_ranks([sys.executable, str(script), str(one)], 1, env, timeout=300)
    ranks.run_ranks([sys.executable, str(script), str(two)], 2, env, timeout=300)
    a, b = np.load(one), np.load(two)
    np.testing.assert_allclose(b["l"], a["l"], rtol=1e-5)
    assert rel(b["opt"], a["opt"]) < 1e-5
    assert rel(b["d"], a["d"]) < 1e-5
    assert int(a["n_intm"]) == F and 0 < int(b["n_intm"]) < F      # (renders of the key frames rank 0 holds)


def test_density_variable_refuses_octaves():
    with pytest.raises(ValueError, match="octave_n=1"):
        _styler(octave_n=2, grid_variable="d")


def test_lbfgs_runs_through_the_octaves():
    d, u, _, vi = _case()
    res = _styler(octave_n=2, optimizer="lbfgs").run({"d": d, "v": u, "v_init": vi})
    l = np.asarray(res["l_frames"])
    print("lbfgs losses per iteration:", l.sum(1))
    assert l.shape == (2 * ITER, F) and np.isfinite(l).all()
    assert l[-1].sum() < l[ITER].sum()                              # the loss falls within the last octave


def test_one_octave_staged_equals_run():
    d, u, _, vi = _case()
    a = _styler(octave_n=1).run({"d": d, "v": u, "v_init": vi})
    st = _styler(octave_n=1)
    st.prepare({"d": d, "v": u, "v_init": vi})
    for _ in range(ITER):
        st.iterate()
    b = st.finish()
    assert set(a) == set(b) and a["octave_sizes"] == b["octave_sizes"] == [[G] * 3]
    assert a["d_intm"] == b["d_intm"] == [] and len(a["l"]) == len(b["l"]) == 1
    np.testing.assert_allclose(b["l_frames"], a["l_frames"], rtol=1e-5)
    np.testing.assert_allclose(b["l"], a["l"], rtol=1e-5)
    assert rel(np.stack(b["opt"]), np.stack(a["opt"])) < 1e-5 and rel(b["d"], a["d"]) < 1e-5
    assert np.array_equal(b["r"], a["r"]) or np.abs(b["r"].astype(int) - a["r"].astype(int)).max() <= 1

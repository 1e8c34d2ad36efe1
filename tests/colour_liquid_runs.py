"""Seeded default-flag runs of the two colour stylizers, shared by tests/test_colour_liquid_stylizer_gpu.py and the fixture
script tests/golden/make_colour_liquid_fixture.py: neither ``colour_render`` nor ``colour_background`` is set, so they are
the smoke render of the commit before those flags.  Nothing of the package or of the test suite is imported at module
level: the fixture script loads this file by path and runs it against whichever checkout is first on sys.path."""
import numpy as np

N = 400
RES = [17, 12, 12]


def particle_scene():
    """the scene of tests/test_colour_stylizer_gpu.py (the same seed and draws): particles, densities, colours, style"""
    from neural_flow_style_amd import synthetic as S
    rng = np.random.RandomState(31)
    F = 2
    p = [rng.uniform(0.1, 0.9, (N, 3)).astype(np.float32) for _ in range(F)]
    r = [(rng.uniform(0.8, 1.2, (N, 1)) * 1000).astype(np.float32) for _ in range(F)]
    c_init = rng.uniform(-0.15, 1.15, (F, N, 3)).astype(np.float32)
    simg = S.style_image(RES[1], RES[2], rng)
    return dict(p=p, r=r, c_init=c_init, simg=simg, F=F)


def unchanged_grid_run():
    """grid_variable 'c' at its defaults: two frames of the grid test's scene under the temporal filter, three views, two
    Adam steps, the 'tiled' transpose (bit-reproducible variables)"""
    from tests.test_colour_grid_stylizer_gpu import _params, _styler
    st, _ = _styler(F=2, iter=2, window_sigma=1.0, lr=0.01, style_mask=True, w_tv=0.01, colour_bwd_route="tiled")
    res = st.run(_params(2))
    return {"l": np.asarray(res["l_frames"], np.float64), "opt": np.stack(res["opt"]), "c": np.stack(res["c"]),
            "r": np.asarray(res["r"])}


def unchanged_particle_run():
    """target_field 'c' at its defaults: the particle test's two frames, three views (one Adam step per view), two steps"""
    from neural_flow_style_amd.styler_3p import Styler
    from tests import colour_runs as RUNS
    sc = particle_scene()
    cfg = RUNS.base_config(RES, "c", F=sc["F"], style_target=sc["simg"], iter=2, window_sigma=1.0, lr=0.01,
                           style_mask=True, w_tv=0.01)
    st = Styler(cfg)
    st.load_img(RES[1:])
    res = st.run({"p": sc["p"], "r": sc["r"], "c_init": sc["c_init"]})
    return {"l": np.asarray(res["l"], np.float64), "opt": np.stack(res["opt"]), "r": np.asarray(res["r"])}

"""Seeded ``styler_3p.Styler`` runs shared by tests/test_colour_stylizer_gpu.py and the fixture script
tests/golden/make_colour_unchanged_fixture.py.  Nothing of the package is imported at module level: the fixture script
loads this file by path and runs it against whichever checkout is first on sys.path."""
import numpy as np

G_UNCHANGED = 12


def config(**over):
    from neural_flow_style_amd.config import get_config
    cfg, _ = get_config([])
    cfg.network = "vgg_19.ckpt"
    cfg.data_dir = "/nonexistent"
    cfg.synthetic_weights = True          # no converted checkpoint offline: explicit opt-in
    for k, v in over.items():
        setattr(cfg, k, v)
    cfg.rng = np.random.RandomState(cfg.seed)
    return cfg


def base_config(res, target, F=1, **over):
    kw = dict(resolution=list(res), domain=list(res), radius=0.5, nsize=1, support=4, rest_density=1000, k=3, clip=False,
              target_field=target, num_frames=F, batch_size=1, frames_per_opt=1, window_sigma=0, interp=1, lr=0.01,
              iter=2, octave_n=1, octave_scale=1.8, style_layer=["conv1_1", "conv2_1"], w_style_layer=[1, 1],
              w_style=1.0, w_content=0, transmit=0.3, rotate=True, n_views=3, v_batch=1, sample_type="uniform", phi0=0,
              phi1=0, phi_unit=0, theta0=-10, theta1=10, theta_unit=10, resize_scale=1.0, views_mode="sequential",
              num_kernels=1, kernel_scale=2, w_pressure=0, w_density=0, w_tv=0, style_mask=False)
    kw.update(over)
    return config(**kw)


def unchanged_target_run(target):
    """a small 'p' or 'd' run of the 3-D particle stylizer: two frames under the temporal filter, three views, two
    Adam steps.  -> dict of arrays (loss history, variables, density volumes, images)"""
    from neural_flow_style_amd import synthetic as S
    from neural_flow_style_amd.styler_3p import Styler
    G, n, F = G_UNCHANGED, 500, 2
    rng = np.random.RandomState(17)
    ps = [S.blob_particles(n, rng) for _ in range(F)]
    rs = [rng.uniform(0.2, 1.0, (n, 1)).astype(np.float32) for _ in range(F)]
    simg = S.style_image(G, G, rng)
    cfg = base_config([G, G, G], target, F=F, window_sigma=1.0, lr=0.05 if target == "d" else 0.002,
                      w_pressure=1e3 if target == "p" else 0, w_tv=0.01, style_target=simg)
    st = Styler(cfg)
    st.load_img([G, G])
    res = st.run({"p": ps, "r": rs})
    return {"l": np.asarray(res["l"], np.float64), "opt": np.stack(res["opt"]), "d": np.asarray(res["d"]),
            "r": np.asarray(res["r"]), "p": np.stack(res["p"])}

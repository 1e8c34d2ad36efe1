"""The scene and configurations of target_field 'pc' shared by tests/test_absorb_cpu.py and tests/test_joint_stylizer_gpu.py:
the particle scene of tests/colour_liquid_runs.py (400 particles, 17 x 12 x 12, two frames), displacements drawn by
RandomState(77).uniform(-0.02, 0.02), the liquid colour render at transmit 0.2 over a non-white background, the three
uniform views theta = -10, 0, 10, synthetic weights, conv1_1 and conv2_1."""
import functools

import numpy as np
import torch

from oracle import nfs_oracle as O
from tests import colour_liquid_runs as LRUNS
from tests import colour_runs as RUNS

RES = LRUNS.RES
N = LRUNS.N
TRANSMIT = 0.2
BG = [0.2, 0.6, 0.05]                     # not white
LAYERS = ["conv1_1", "conv2_1"]


@functools.lru_cache(maxsize=None)
def scene():
    """particles, densities, colours (some outside [0,1]) and style of LRUNS.particle_scene, the displacements, the float64
    loss network and its style features: computed once and left alone"""
    sc = LRUNS.particle_scene()
    v = np.random.RandomState(77).uniform(-0.02, 0.02, (N, 3)).astype(np.float32)
    w64 = {k: (np.asarray(a, np.float64), np.asarray(b, np.float64))
           for k, (a, b) in O.synthetic_vgg19_weights(123, upto="conv2_1").items()}
    sfe = O.style_target_features(torch.tensor(np.asarray(sc["simg"], np.float64))[None], w64, LAYERS, upto="conv2_1")
    return dict(sc, v=v, w64=w64, sfe=sfe)


def config(F=1, **over):
    kw = dict(colour_render="liquid", colour_background=BG, transmit=TRANSMIT, style_layer=list(LAYERS))
    kw.update(over)
    return RUNS.base_config(RES, "pc", F=F, style_target=scene()["simg"], **kw)


def ref_cfg(cfg=None, **over):
    """the configuration as the float64 reference reads it (a dict)"""
    return dict(vars(cfg if cfg is not None else config(**over)))


def uniform_views():
    """the view matrices a styler of ``config()`` holds (sample_type 'uniform': theta = -10, 0, 10)"""
    from neural_flow_style_amd import transform as T
    c = config()
    mats, _ = T.rot_mat(c.phi0, c.phi1, c.phi_unit, c.theta0, c.theta1, c.theta_unit, sample_type=c.sample_type, rng=c.rng,
                        nv=c.n_views)
    assert len(mats) == 3
    return mats

"""Writes tests/golden/colour_liquid_unchanged.npz: the default-flag runs of tests/colour_liquid_runs.py (both colour
stylizers, the smoke render) as the commit BEFORE --colour_render computed them on an MI355X
(tests/test_colour_liquid_stylizer_gpu.py compares the current build against them).

    python tests/golden/make_colour_liquid_fixture.py CHECKOUT OUT.npz

CHECKOUT: a built checkout of the commit to record (its package and its tests are imported); the runs themselves are this
file's neighbour tests/colour_liquid_runs.py.  Every run is made twice.  The grid run takes the 'tiled' transpose and its
variables and images are bit-reproducible: the script refuses to write a fixture whose two runs differ there.  The particle
run's splat adds with float atomics: its two runs must agree to the tolerances the test holds the current build to."""
import importlib.util
import os
import sys

import numpy as np


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def main(checkout, out):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.abspath(checkout))
    spec = importlib.util.spec_from_file_location("colour_liquid_runs", os.path.join(here, "..", "colour_liquid_runs.py"))
    runs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(runs)
    import neural_flow_style_amd
    assert os.path.abspath(neural_flow_style_amd.__file__).startswith(os.path.abspath(checkout)), neural_flow_style_amd.__file__
    arrays = {}
    a, b = runs.unchanged_grid_run(), runs.unchanged_grid_run()
    for k in ("opt", "c", "r"):
        assert np.array_equal(a[k], b[k]), "run-to-run difference in grid/%s: no bit-exact fixture possible" % k
    np.testing.assert_allclose(a["l"], b["l"], rtol=1e-5)
    arrays.update({"grid_" + k: v for k, v in a.items()})
    a, b = runs.unchanged_particle_run(), runs.unchanged_particle_run()
    np.testing.assert_allclose(a["l"], b["l"], rtol=1e-5)
    assert _rel(a["opt"], b["opt"]) <= 1e-5 and np.abs(a["r"].astype(np.int32) - b["r"].astype(np.int32)).max() <= 1
    arrays.update({"particle_" + k: v for k, v in a.items()})
    np.savez_compressed(out, **arrays)
    print("wrote", out, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

"""Writes tests/golden/colour_unchanged_targets.npz: the 'p' and 'd' runs of tests/colour_runs.py as the commit BEFORE
target_field 'c' computed them on an MI355X (tests/test_colour_stylizer_gpu.py compares the current build's bits).
A commit that changes a kernel's roundings on purpose records the fixture again from its own build and says so in that
test's docstring (so far: StoreInput / GradInput of render.hip rounding every operation).

    python tests/golden/make_colour_unchanged_fixture.py CHECKOUT OUT.npz

CHECKOUT: a built checkout of the commit to record (its package is imported); the runs themselves are this file's
neighbour tests/colour_runs.py.  Every run is made twice: the script refuses to write a fixture the recorded build does
not itself reproduce bit for bit."""
import importlib.util
import os
import sys

import numpy as np


def main(checkout, out):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.abspath(checkout))
    spec = importlib.util.spec_from_file_location("colour_runs", os.path.join(here, "..", "colour_runs.py"))
    runs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(runs)
    import neural_flow_style_amd
    assert os.path.abspath(neural_flow_style_amd.__file__).startswith(os.path.abspath(checkout)), neural_flow_style_amd.__file__
    arrays = {}
    for target in ("p", "d"):
        a, b = runs.unchanged_target_run(target), runs.unchanged_target_run(target)
        for k in a:
            assert np.array_equal(a[k], b[k]), "run-to-run difference in %s/%s: no bit-exact fixture possible" % (target, k)
            arrays["%s_%s" % (target, k)] = a[k]
    np.savez_compressed(out, **arrays)
    print("wrote", out, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

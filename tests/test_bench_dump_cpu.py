"""bench.py --dump-outputs, --steps and --full without a GPU: the files dump_outputs() writes (float32 / float64, the
64 MB budget, the seeded sample of an array larger than its share), the refusal of fewer than one timed step, and --full
off by default."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_types_budget_and_a_fixed_sample(tmp_path):
    big = torch.arange(16_000_000, dtype=torch.float32).view(400, 200, 200)  # 64 MB (more than its share), exact in float32
    arrays = {"loss": torch.tensor(2.5), "small": torch.arange(10, dtype=torch.float64), "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["big.npy", "loss.npy", "small.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= bench.DUMP_BYTES
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in files}
    assert got["loss"].dtype == np.float32 and float(got["loss"]) == 2.5
    assert got["small"].dtype == np.float64 and np.array_equal(got["small"], np.arange(10))
    s = got["big"]
    assert s.dtype == np.float32 and s.ndim == 1 and 1_000_000 < s.size < big.numel()
    assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < big.numel()            # distinct flat positions, in order
    assert np.array_equal(s, big.view(-1).numpy()[s.astype(np.int64)])
    for f in files:                                                                     # the same sample every run
        assert np.array_equal(np.load(str(tmp_path / "b" / f)), got[f[:-4]])


def test_steps_below_one_are_refused(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.steps == 7 and a.dump_outputs == "out"


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "10", "--full", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.full is True and a.no_cpu_baseline

"""bench.py's --dump-outputs writer and --full switch, without a GPU: small arrays are written
whole in float32 with their shape, an array past the 64 MB budget becomes a sample at the
same seeded indices in every call, and a plain run asks for neither the roofline nor the
CPU baseline."""
import sys

import numpy as np
import torch

import bench  # the repository root is on sys.path (conftest.py)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 4096 + 4 * 1000)
    big = torch.arange(5000, dtype=torch.float64).reshape(50, 100)
    arrays = {"loss": torch.tensor(1.5), "ids": torch.arange(6, dtype=torch.int32).reshape(2, 3),
              "big": big}
    bench.dump_outputs(tmp_path / "a", arrays)
    bench.dump_outputs(tmp_path / "b", arrays)
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    b = {p.stem: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    assert set(a) == set(b) == {"loss", "ids", "big"}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].shape == () and a["loss"] == 1.5
    assert a["ids"].shape == (2, 3) and (a["ids"] == np.arange(6).reshape(2, 3)).all()
    # the sample: within the budget, elements of the array, the same ones in both calls
    assert a["big"].ndim == 1 and 0 < a["big"].size < 5000
    assert sum(v.nbytes for v in a.values()) <= 4 * 1000
    assert np.isin(a["big"], big.numpy()).all() and len(np.unique(a["big"])) > 100
    assert (a["big"] == b["big"]).all()


def test_plain_run_skips_the_extra_measurements(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2"])
    args = bench.parse()
    assert not args.full and args.no_roofline and args.no_cpu_baseline
    assert args.dump_outputs is None and args.steps == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and not args.no_roofline and not args.no_cpu_baseline
    assert args.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    args = bench.parse()
    assert args.no_cpu_baseline and not args.no_roofline

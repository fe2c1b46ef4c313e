"""CPU-side tests of bench.py's host logic (no GPU): the options of a plain run and the --dump-outputs writer."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def test_plain_run_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert (a.steps, a.full, a.dump_outputs) == (3, True, "out")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_whole_when_it_fits(tmp_path):
    arrays = {"loss": torch.tensor([1.5]), "logits": torch.randn(4, 7), "rank": torch.arange(4, dtype=torch.int32)}
    shapes = bench.dump_outputs(str(tmp_path), arrays)
    assert shapes == {"loss": [1], "logits": [4, 7], "rank": [4]}
    for name, t in arrays.items():
        a = np.load(os.path.join(tmp_path, name + ".npy"))
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, t.float().numpy())


def test_dump_outputs_samples_what_does_not_fit(tmp_path):
    """Over budget: small arrays stay whole, large ones become the same seeded sample on every call."""
    g = torch.Generator().manual_seed(0)
    arrays = {"small": torch.randn(10, generator=g), "big": torch.randn(5000, generator=g), "bigger": torch.randn(9000, generator=g)}
    budget = 4 * 2010
    shapes = bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    assert shapes == {"small": [10], "big": [1000], "bigger": [1000]}
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", n + ".npy")) - 128 for n in arrays) <= budget
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)
    for name in arrays:
        a, b = (np.load(os.path.join(tmp_path, d, name + ".npy")) for d in "ab")
        np.testing.assert_array_equal(a, b)
        assert np.isin(a, arrays[name].numpy()).all()

"""bench.py's command line and its --dump-outputs writer, as far as they go without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_the_default_and_steps_are_taken_as_given():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "0"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 0, False, None)
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--dump-outputs", "d", "--disconnected"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def test_dump_outputs_formats_order_and_fixed_sample(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(3)
    small = torch.randn(2, 3, 4, 5, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ints = torch.arange(24, dtype=torch.int64).reshape(4, 6) * 2 ** 40
    arrays = {"small": small, "ints": ints, "flags": torch.tensor([True, False, True]), "absent": None,
              "scalar": torch.tensor(1.5)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["flags", "ints", "scalar", "small"]
    assert got["small"].dtype == np.float32 and np.array_equal(got["small"], small.float().numpy())  # logical NCHW order
    assert got["ints"].dtype == np.float64 and np.array_equal(got["ints"], ints.numpy().astype(np.float64))
    assert got["flags"].tolist() == [1.0, 0.0, 1.0] and got["scalar"].shape == () and float(got["scalar"]) == 1.5
    # over the budget: every array is cut to its share, the same elements in every run, within the budget in all
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    big = {"x": torch.randn(50, 100, generator=g), "y": torch.arange(9000, dtype=torch.int64), "z": torch.ones(10)}
    bench.dump_outputs(str(tmp_path / "b"), big)
    bench.dump_outputs(str(tmp_path / "c"), {k: v.clone() for k, v in big.items()})
    total = 0
    for name, t in big.items():
        b, c = np.load(tmp_path / "b" / (name + ".npy")), np.load(tmp_path / "c" / (name + ".npy"))
        assert np.array_equal(b, c)
        total += b.nbytes
        if name == "z":
            assert b.shape == (10,)
            continue
        n = 4000 // 3 // b.itemsize
        idx = torch.randint(t.numel(), (n,), generator=torch.Generator().manual_seed(0))
        assert b.shape == (n,) and np.array_equal(b, t.reshape(-1)[idx].numpy().astype(b.dtype))
    assert total <= 4000

"""bench.py's options beside the launcher: what a plain run does and what --full adds, the step count, and the output dump
that lets two builds be compared output for output (--dump-outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default_and_steps_are_checked():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def test_dump_outputs_samples_long_arrays_the_same_way_every_time(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"loss": torch.tensor([0.25], dtype=torch.float64), "params": torch.randn(5000, generator=g),
              "grads": torch.randn(5000, generator=g), "small": torch.arange(12.0).reshape(3, 4)}
    n = bench.dump_outputs(str(tmp_path / "a"), arrays, sample=1000)
    bench.dump_outputs(str(tmp_path / "b"), arrays, sample=1000)
    got = {k: np.load(str(tmp_path / "a" / f"{k}.npy")) for k in arrays}
    assert n == sum(v.nbytes for v in got.values()) == 4 * (1 + 1000 + 1000 + 12)
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["small"], arrays["small"].numpy()) and got["loss"].tolist() == [0.25]
    for k in ("params", "grads"):
        assert np.array_equal(got[k], np.load(str(tmp_path / "b" / f"{k}.npy")))      # a fixed sample
        full = arrays[k].numpy()
        pos = np.searchsorted(np.sort(full), got[k])
        assert got[k].shape == (1000,) and np.isin(got[k], full).all() and len(set(pos.tolist())) == 1000
    # the same positions in every array of one length: parameter i beside gradient i
    pi = [int(np.nonzero(arrays["params"].numpy() == v)[0][0]) for v in got["params"][:50]]
    gi = [int(np.nonzero(arrays["grads"].numpy() == v)[0][0]) for v in got["grads"][:50]]
    assert pi == gi == sorted(pi)


def test_dump_outputs_refuses_more_than_its_budget(tmp_path):
    with pytest.raises(ValueError, match="budget"):
        bench.dump_outputs(str(tmp_path / "d"), {"x": torch.zeros(300)}, sample=1000, budget=1000)
    assert not (tmp_path / "d").exists()
    assert bench.DUMP_BUDGET == 64 << 20 and 2 * 4 * bench.DUMP_SAMPLE < bench.DUMP_BUDGET    # parameters + gradients


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "outs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "tiles/s" and d["higher_is_better"] is True
    assert d["dtype"] == bench.parse([]).dtype and d["ms_per_step"] > 0
    assert abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert not {"roofline", "step_other_mode", "eval", "miou_vs_ref", "data_path", "cpu_baseline"} & set(d)   # --full only
    got = {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert set(got) == {"loss", "params", "grads", "bn_running_mean", "bn_running_var"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert abs(float(got["loss"][0]) - d["loss"]) <= 1e-6
    assert got["params"].shape == got["grads"].shape == (bench.DUMP_SAMPLE,) and np.abs(got["grads"]).max() > 0

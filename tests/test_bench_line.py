"""bench.py's plain run against its --full run, and --dump-outputs: the CPU side (options, the sampled dump) and, with -m gpu, a
plain run end to end twice with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("no_cpu_baseline", "no_parity_mode", "no_other_configs", "no_probe", "no_sustained")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_off_everything_but_the_headline(monkeypatch):
    plain = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not plain.full and plain.steps == 7 and plain.warmup == 2 and plain.dump_outputs is None
    assert all(getattr(plain, k) for k in FULL_ONLY)
    full = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert full.full and full.dump_outputs == "out" and not any(getattr(full, k) for k in FULL_ONLY)
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_float32_and_a_fixed_sample(tmp_path):
    big = torch.arange(bench.DUMP_SAMPLE * 3 // 2, dtype=torch.float64)     # value == flat index
    small = torch.rand(2, 3, 4, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "scalar": small.sum()})
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("big", "small", "scalar")}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["small"].shape == (2, 3, 4) and np.array_equal(a["small"], small.float().numpy()) and a["scalar"].shape == ()
    assert a["big"].shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(a["big"]) >= 0) and a["big"][-1] < big.numel()
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))            # same arguments, same sample


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
           "--lr-size", "64", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_plain_run_line_and_outputs_repeat(tmp_path):
    """A plain run prints the headline only, its rate is its K timed steps, and two runs with the same arguments write the same
    arrays: inputs and the last step's outputs (the step is bit-reproducible, tests/test_gpu_chain.py)."""
    out, arrays = _plain_run(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "images/sec" and out["higher_is_better"] is True
    assert out["value"] == pytest.approx(2 * 1e3 / out["ms_per_step"], rel=0.01)
    assert not {"roofline", "parity_mode", "other_configs", "cpu_baseline", "box_reference", "power", "host"} & set(out)
    assert sorted(arrays) == ["ema", "grad", "loss", "lr", "params", "sr"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in arrays.values())
    assert sum(v.nbytes for v in arrays.values()) <= 64 << 20
    assert arrays["lr"].shape == (2, 3, 64, 64) and arrays["sr"].shape == (2, 3, 256, 256)
    assert float(arrays["loss"]) == pytest.approx(out["loss"], rel=1e-6)
    _, again = _plain_run(tmp_path / "b")
    for name, v in arrays.items():
        assert np.array_equal(v, again[name]), name

"""bench.py's command line: a plain run prints the headline line without the `--full` legs,
and `--dump-outputs DIR` writes the last timed step's outputs, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
FULL_ONLY = ("strict_fp32", "c5_256", "c4_encoder_latents", "cpu_baseline")


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "8", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, timeout=240, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_line_and_dump(cuda, tmp_path):
    res = _run(tmp_path / "a")
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "patterns/s" and res["higher_is_better"] is True
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - 8 / (res["ms_per_step"] / 1e3)) <= 1e-2 * res["value"]
    assert "f16x3" in res["dtype"]
    # the legs behind --full did not run
    assert not any(k in res for k in FULL_ONLY)
    assert res["roofline"] is None and res["kernel_families_ms_per_step"] == {}
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("loss", "kl", "rec", "params", "grads")}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in a)
    for n, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), n
    assert a["loss"].shape == a["kl"].shape == a["rec"].shape == (1,)
    assert abs(float(a["loss"][0]) - res["loss"]) <= 1e-6 * abs(res["loss"]) + 1e-6
    from latice.model import VariationalAutoEncoderRawData
    numel = sum(p.numel() for p in VariationalAutoEncoderRawData(32, 16, 128).parameters())
    assert a["params"].shape == a["grads"].shape == (numel,)
    assert np.abs(a["grads"]).max() > 0
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    # same arguments, same inputs, same step: the second run dumps the same arrays
    _run(tmp_path / "b")
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy")), n

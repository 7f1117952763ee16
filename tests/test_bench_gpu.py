"""bench.py contract (driver-facing): one JSON line with the agreed keys, roofline (--full) and timing fields sane.
Runs the real script in a child process at reduced depth (the line is then marked invalid by the script itself)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_emits_the_contract_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n_layers", "2", "--steps", "3", "--warmup",
                        "1", "--full", "--no_cpu_baseline"], capture_output=True, text=True, timeout=500, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    assert [ln for ln in r.stdout.splitlines() if ln.strip()] == lines, r.stdout[-2000:]   # nothing else on stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["unit"] == "samples/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9


@pytest.mark.gpu
def test_bench_fails_on_a_set_gemm_error_word():
    """A timed-out split-K exchange during the run (the workspace's sticky error word, injected after the warm-up) must
    not produce a valid-looking line: every optimizer step of the timed region is skipped on the device, the JSON says
    `invalid`, the exit status is non-zero."""
    env = dict(os.environ, FVQA_BENCH_INJECT_GEMM_ERROR="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n_layers", "2", "--steps", "3", "--warmup",
                        "1", "--no_cpu_baseline"], capture_output=True, text=True, timeout=500, cwd=ROOT, env=env)
    assert r.returncode != 0, r.stdout[-1000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert "split-K exchange" in d["invalid"]


@pytest.mark.gpu
def test_plain_bench_times_the_steps_only_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run (no --full) prints the headline line without the figures that take runs of their own, and --dump-outputs
    writes what the last timed step handed its caller: float32 arrays, finite, within 64 MB, the losses summing to the line's."""
    import numpy as np
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n_layers", "2", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=500, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "step_roofline", "loss"):
        assert k in d, k
    for k in ("roofline", "other_configs", "cpu_baseline"):
        assert k not in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "samples/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    files = sorted(os.listdir(out))
    assert files == sorted(f"{n}.npy" for n in ("losses", "grad_norm", "trainables", "grads")), files
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10**6
    got = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["losses"].shape == (3,) and abs(float(got["losses"].sum()) - d["loss"]) <= 1e-3 * abs(d["loss"])
    assert got["grad_norm"].shape == (1,) and got["grad_norm"][0] > 0
    assert got["trainables"].shape == got["grads"].shape and got["trainables"].size > 3 * 10**6
    assert np.abs(got["grads"]).max() > 0

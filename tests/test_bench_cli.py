"""bench.py command-line contract: the plain run's result line, --full
being opt-in, and --dump-outputs writing reproducible float arrays.

Runs on either device (bench.py shrinks itself on CPU-only machines);
the shape is kept tiny so the two subprocess runs stay quick."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO_ROOT = Path(__file__).resolve().parent.parent

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--pop", "64",
        "--symbols", "4", "--candles", "64000"]


def _run(extra):
    r = subprocess.run(
        [sys.executable, str(REPO_ROOT / "bench.py"), *ARGS, *extra],
        capture_output=True, text=True, timeout=300, cwd=REPO_ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    dirs = [tmp_path_factory.mktemp(f"dump{i}") for i in range(2)]
    outs = [_run(["--dump-outputs", str(d)]) for d in dirs]
    return dirs, outs


def test_plain_result_line(two_runs):
    _, (out, _) = two_runs
    assert out["metric"] == "backtested_1m_candles_per_sec_ga_pop_eval"
    assert out["unit"] == "candles/s"
    assert out["higher_is_better"] is True
    assert out["dtype"] == "fp32"
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0 and out["value"] > 0
    evals = out["config"]["candle_evals_per_step_per_gpu"] * out["n_gpus"]
    assert out["value"] == pytest.approx(
        evals / (out["ms_per_step"] / 1000.0), rel=1e-9)
    # the extra workloads only run behind --full
    assert out["config"]["continuous"] == {}
    assert out["config"]["secondary"] == {}


def test_dump_outputs_are_float_and_reproducible(two_runs):
    (d0, d1), (out, _) = two_runs
    names = sorted(p.name for p in d0.glob("*.npy"))
    assert names == ["fitness.npy", "metrics_mean.npy",
                     "metrics_sample.npy", "population.npy"]
    assert sorted(p.name for p in d1.glob("*.npy")) == names
    total = 0
    for n in names:
        a, b = np.load(d0 / n), np.load(d1 / n)
        assert a.dtype in (np.float32, np.float64), n
        assert a.size > 0 and np.isfinite(a).all(), n
        assert a.shape == b.shape and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 * 1000 * 1000
    pop = out["config"]["global_batch"]
    fit = np.load(d0 / "fitness.npy")
    assert fit.shape == (pop,)
    assert np.load(d0 / "population.npy").shape[0] == pop
    assert float(fit.max()) == pytest.approx(
        out["config"]["best_fitness"], rel=1e-6)


def test_steps_must_be_positive():
    r = subprocess.run(
        [sys.executable, str(REPO_ROOT / "bench.py"), "--steps", "0"],
        capture_output=True, text=True, timeout=300, cwd=REPO_ROOT)
    assert r.returncode != 0 and "--steps" in r.stderr

"""bench.py's command line: a plain run prints the headline line only, --full adds the figures that take runs of their
own, --dump-outputs writes the state the timed passes end at, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "per_pass_median_ms", "per_pass_ms", "useful_fp64_tflops", "cpu_baseline")


def test_dump_outputs_writes_npy(tmp_path):
    import bench
    d = tmp_path / "a" / "b"
    bench.dump_outputs(str(d), {"state": np.arange(5.0), "x": np.ones((2, 3), dtype=np.float32)})
    assert sorted(os.listdir(d)) == ["state.npy", "x.npy"]
    assert np.load(d / "state.npy").dtype == np.float64 and np.array_equal(np.load(d / "state.npy"), np.arange(5.0))
    assert np.load(d / "x.npy").dtype == np.float32
    with pytest.raises(AssertionError):  # integers are not a benchmark output
        bench.dump_outputs(str(d), {"i": np.arange(5)})
    with pytest.raises(AssertionError):  # 64 MB in all
        bench.dump_outputs(str(d), {"big": np.broadcast_to(np.zeros(1), (bench.DUMP_LIMIT_BYTES // 8 + 1,))})


def test_help_lists_the_options():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt


def _bench(*args):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout  # the result line is the only stdout output
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs(tmp_path):
    """configs[1] (the smallest rig, set up in under a second), 3 timed passes: the plain line holds the headline
    entries and none of the --full figures, the --full line holds both, and the two runs end at the same state.
    Tolerance: the same build runs the same f64 passes twice, so any difference is summation order inside a pass
    (eps = 2.2e-16) through three solves; 1e-10 relative leaves six digits for the systems' conditioning."""
    a, b = str(tmp_path / "plain"), str(tmp_path / "full")
    common = ["--config", "2", "--steps", "3", "--warmup", "2"]
    plain = _bench(*common, "--dump-outputs", a)
    full = _bench(*common, "--full", "--no-cpu-baseline", "--dump-outputs", b)
    for line in (plain, full):
        for k in HEADLINE:
            assert k in line, k
        assert line["steps"] == 3 and line["unit"] == "iterations/s" and line["dtype"] == "f64"
        assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert not [k for k in FULL_ONLY if k in plain]
    assert "roofline" in full and "cpu_baseline" not in full
    assert os.listdir(a) == ["state.npy"] and os.listdir(b) == ["state.npy"]
    sa, sb = np.load(os.path.join(a, "state.npy")), np.load(os.path.join(b, "state.npy"))
    assert sa.dtype == np.float64 and sa.shape == sb.shape and sa.size > 0 and np.isfinite(sa).all()
    assert np.allclose(sa, sb, rtol=1e-10, atol=1e-12)

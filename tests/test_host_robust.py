"""Robust-term surface of the C++ host layer (kalibr_amd/host/kalibr_backend.*, tests/cpp/test_host_robust.cpp): the
M-estimator classes, CalibrationProblem's setters, GpuLinearSystemSolver's forwarding and calibrateCameras'
cornerUncertainty.

CPU: the estimator classes give the restatement's values (tests/robust_ref.py) and the reference's names; a solver
without robust terms makes the setters throw and calibrateCameras with a corner uncertainty over it fails before any
stage runs.
GPU: Optimizer2::optimize() over GpuLinearSystemSolver with a Huber policy equals kb_optimize on the same problem (same
iterations, state 1e-12); computeHessian ignores the estimator but keeps invR; calibrateCameras with cornerUncertainty =
0.5 returns 0.5 x the default run's parameterStdDev (rel 1e-8) with the same batches accepted.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from kalibr_amd import build as B
from kalibr_amd import synth

from . import robust_ref as R
from .host_problem import write_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory, oracle_mod):
    if not os.path.exists(B.OUT):
        B.build()
    B.build_host()
    out = str(tmp_path_factory.mktemp("host_robust") / "test_host_robust")
    ob = os.path.join(ROOT, "oracle", "_build")
    cmd = ["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "test_host_robust.cpp"),
           "-I", os.path.join(ROOT, "tests", "cpp"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kalibr_amd", "host"),
           "-I", os.path.join(ROOT, "oracle"),
           "-L", os.path.join(ROOT, "kalibr_amd"), "-lkalibr_backend", "-lkalibr_hip",
           "-L", ob, "-lkb_oracle", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "kalibr_amd") + ":" + ob]
    subprocess.run(cmd, check=True)
    return out


def _run(driver, *args):
    r = subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_estimator_classes_match_the_restatement(driver):
    r = _run(driver, "estimators")
    pts = np.array([0.0, 1.0, 3.999, 4.0, 16.0, 400.0])
    eps = R.blake_zisserman_epsilon(2, 0.999, 0.1)
    want = {1: (R.HUBER, 2.0, "Huber(2)"), 2: (R.CAUCHY, 4.0, "Cauchy (4)"),
            3: (R.GEMAN_MCCLURE, 9.0, "Geman McClure (9)"), 4: (R.BLAKE_ZISSERMAN, eps, None), 0: (R.NONE, 0.0, "none")}
    for kind, (name, param, label) in want.items():
        got = r[str(kind)]
        assert got["kind"] == kind
        assert abs(got["parameter"] - param) <= 1e-15 * max(1.0, abs(param))
        ref = R.weight(name, param, pts)
        assert np.abs(np.array(got["w"]) - ref).max() <= 1e-15, (kind, got["w"], ref)
        if label is not None:
            assert got["name"] == label
    assert r["4"]["name"].startswith("Blake-Zisserman(9") and r["4"]["name"].endswith("e-06)")
    assert r["1"]["w"][2] == 1.0 and r["1"]["w"][3] == 1.0 and r["1"]["w"][4] == 0.5  # s = k^2: the k / sqrt(s) branch
    assert r["df3_throws"] == 1
    assert r["weighted"] == [1, 0, 1, 0]


def test_solver_without_robust_terms_refuses(driver, tmp_path):
    p = synth.make_problem([synth.PINHOLE_RADTAN] * 3, 24, seed=5150)
    path = str(tmp_path / "p.bin")
    write_problem(path, p)
    r = _run(driver, "unsupported", path)
    assert r["supports"] == 0 and r["setter_throws"] == 3
    assert "need a stage solver with robust terms" in r["calibrate_message"]
    assert r["solvers_made"] == 1  # the probe only: refused before any stage ran


@pytest.mark.gpu
def test_host_loop_equals_the_device_loop_with_a_huber_policy(driver, tmp_path):
    clean = synth.make_config(1, n_frames=12)
    p, _ = R.contaminate(clean, 11)
    path = str(tmp_path / "p.bin")
    write_problem(path, p)
    r = _run(driver, "optimize-gpu", path)
    print(r)
    assert r["host_iterations"] == r["device_iterations"] >= 2 and r["host_failed"] == r["device_failed"]
    assert r["state_diff"] <= 1e-12
    assert abs(r["J_host"] - r["J_device"]) <= 1e-12 * r["J_device"] and r["J_host"] < r["J_start"]
    # the outliers are down-weighted at the optimum: w < 1 exactly where s >= k^2
    assert 0 < r["downweighted"] < 0.1 * r["n_terms"] and r["weight_flag_mismatches"] == 0
    # computeHessian (useMEstimator = false): the estimator is ignored, invR kept
    assert r["hess_diff"] == 0.0 and r["weighted_diff"] > 0.0
    assert r["scale_rel_err"] <= 1e-12


@pytest.mark.gpu
def test_parameter_std_dev_scales_with_the_corner_uncertainty(driver, tmp_path):
    p = synth.make_problem([synth.PINHOLE_RADTAN] * 3, 24, seed=5150)
    path = str(tmp_path / "p.bin")
    write_problem(path, p)
    a = _run(driver, "stddev-gpu", path, 1.0)
    b = _run(driver, "stddev-gpu", path, 0.5)
    # the corner uncertainty enters the final batch problem only: the stage sequence accepts the same batches
    assert a["batch_accepted"] == b["batch_accepted"] and a["accepted_batches"] == b["accepted_batches"] > 0
    assert a["final_state"] == b["final_state"]
    sa, sb = np.array(a["std_dev"]), np.array(b["std_dev"])
    assert sa.size == sb.size == 3 * 8 + 2 * 6 and np.all(sa > 0)
    print(float(np.abs(sb / (0.5 * sa) - 1.0).max()))
    assert np.all(np.abs(sb - 0.5 * sa) <= 1e-8 * 0.5 * sa)
